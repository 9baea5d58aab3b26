// The body of decode_self_attention_kernel and its gated instance (attention.hip): included verbatim into both kernels, so that the
// ungated one compiles exactly as before.  Not a header: no include guard.
    static_assert(KB * 64 <= 256, "phase 0 lists one position per thread");
    __shared__ int slots[KB * 64];
    __shared__ uint8_t pads[KB * 64];
    __shared__ float sc[kSelfMaxHeads][KB * 64];
    __shared__ __attribute__((aligned(16))) float red[256 * 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = blockIdx.x, t = p.t;
    const int hk = p.h * p.dk;                       // == h * dv (checked on the host)

    if (tid <= t) {
        const int slot = tid == t ? r : p.anc[(size_t)r * p.anc_ld + tid];
        slots[tid] = slot;
        pads[tid] = p.padflag[(size_t)tid * p.pad_ld + slot];
    }
    int ecol[CH];
    bool evalid[CH];
    f32x4 q4[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const int e = c * 256 + lane * 4;
        evalid[c] = e < hk;
        ecol[c] = min(e, hk - 4);
        q4[c] = *reinterpret_cast<const f32x4*>(p.q + (size_t)r * p.ldq + ecol[c]);
        if (!evalid[c]) q4[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    __syncthreads();

    const int group = p.dk >> 2;                     // lanes per head: a power of two <= 16
    const float scale_div = sqrtf((float)p.dk);
    const int niter = (t - wave + 4) >> 2;           // keys wave, wave+4, ... <= t
    for (int i0 = 0; i0 < niter; i0 += 4) {
        f32x4 k4[4][CH];
        int jj[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {                // four keys in flight per wave
            jj[u] = min(wave + 4 * (i0 + u), t);
            const float* krow = p.kcache + (size_t)jj[u] * p.pos_stride + (size_t)slots[jj[u]] * p.ldkv;
#pragma unroll
            for (int c = 0; c < CH; ++c) k4[u][c] = *reinterpret_cast<const f32x4*>(krow + ecol[c]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool live = i0 + u < niter;
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                float part = (q4[c][0] * k4[u][c][0] + q4[c][1] * k4[u][c][1]) + (q4[c][2] * k4[u][c][2] + q4[c][3] * k4[u][c][3]);
                for (int off = 1; off < group; off <<= 1) part += __shfl_xor(part, off, 64);
                if (live && evalid[c] && (lane & (group - 1)) == 0)
                    sc[(c * 256 + lane * 4) / p.dk][jj[u]] = pads[jj[u]] ? -INFINITY : part / scale_div;
            }
        }
    }
    __syncthreads();

    for (int hd = wave; hd < p.h; hd += 4) {
        if constexpr (KB == 1) {
            const float s = lane <= t ? sc[hd][lane] : -INFINITY;
            const float mx = wave_max(s);
            const float e = lane <= t ? expf(s - mx) : 0.f;
            const float sum = wave_sum(e);
            if (lane <= t) sc[hd][lane] = e / sum;
        } else {                                     // keys lane, lane + 64, ...: per-lane max / sum first, then the wave's
            float s[KB], e[KB], mx = -INFINITY, part = 0.f;
#pragma unroll
            for (int u = 0; u < KB; ++u) {
                s[u] = lane + 64 * u <= t ? sc[hd][lane + 64 * u] : -INFINITY;
                mx = fmaxf(mx, s[u]);
            }
            mx = wave_max(mx);
#pragma unroll
            for (int u = 0; u < KB; ++u) {
                e[u] = lane + 64 * u <= t ? expf(s[u] - mx) : 0.f;
                part += e[u];
            }
            const float sum = wave_sum(part);
#pragma unroll
            for (int u = 0; u < KB; ++u)
                if (lane + 64 * u <= t) sc[hd][lane + 64 * u] = e[u] / sum;
        }
    }
    __syncthreads();

    const int cols = hk >> 2;                        // float4 columns of the output row (<= 256)
    const int groups = 256 / cols;                   // key groups working in parallel
    const int col = tid % cols, g = tid / cols;
    const int hd = (col * 4) / p.dv;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    // keys g, g+groups, ... <= t (0 when g > t); threads past the last whole key group (256 % cols != 0) idle
    const int nkeys = g < groups ? (t - g + groups) / groups : 0;
    for (int i0 = 0; i0 < nkeys; i0 += 4) {
        f32x4 v4[4];
        int jj[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            jj[u] = min(g + groups * (i0 + u), t);
            v4[u] = *reinterpret_cast<const f32x4*>(p.vcache + (size_t)jj[u] * p.pos_stride + (size_t)slots[jj[u]] * p.ldkv + col * 4);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i0 + u < nkeys) acc += v4[u] * sc[hd][jj[u]];
    }
    if (g > 0) *reinterpret_cast<f32x4*>(red + (size_t)tid * 4) = acc;
    __syncthreads();
    if (g == 0) {
        for (int gg = 1; gg < groups; ++gg) acc += *reinterpret_cast<const f32x4*>(red + (size_t)(gg * cols + col) * 4);
        *reinterpret_cast<f32x4*>(p.out + (size_t)r * p.ldo + col * 4) = acc;
    }
