// The body of meshed_mix and its gated instance (rowops.hip): included verbatim into both kernels, so that the
// ungated one compiles exactly as before.  Not a header: no include guard.
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int l = 0; l < levels; ++l) {
            const f32x4 al = reinterpret_cast<const f32x4*>(alpha)[(size_t)l * n4 + i];
            const f32x4 xv = reinterpret_cast<const f32x4*>(enc)[(size_t)l * n4 + i];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = acc[j] + sigmoidf_(al[j]) * xv[j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = acc[j] / divisor;
        reinterpret_cast<f32x4*>(out)[i] = acc;
    }
