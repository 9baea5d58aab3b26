// The body of decode_self_merge_kernel and its gated instance (attention.hip): included verbatim into both kernels, so that the
// ungated one compiles exactly as before.  Not a header: no include guard.
    const int hv4 = (p.h * p.dv) >> 2;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * hv4) return;
    const int row = idx / hv4, c4 = idx - row * hv4, hd = (c4 * 4) / p.dv;
    const float2* ml = reinterpret_cast<const float2*>(p.part_ml);
    const size_t hv = (size_t)p.h * p.dv;
    float M = -INFINITY;
    for (int c = 0; c < chunks; ++c) M = fmaxf(M, ml[((size_t)c * rows + row) * p.h + hd].x);
    float L = 0.f;
    f32x4 O = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < chunks; ++c) {
        const float2 v = ml[((size_t)c * rows + row) * p.h + hd];
        if (v.y > 0.f) {
            const float w = expf(v.x - M);
            L += v.y * w;
            O += *reinterpret_cast<const f32x4*>(p.part_o + ((size_t)c * rows + row) * hv + c4 * 4) * w;
        }
    }
    *reinterpret_cast<f32x4*>(p.out + (size_t)row * p.ldo + c4 * 4) = O / L;
