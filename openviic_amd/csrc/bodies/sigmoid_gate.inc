// The body of sigmoid_gate and its gated instance (rowops.hip): included verbatim into both kernels, so that the
// ungated one compiles exactly as before.  Not a header: no include guard.
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const f32x4 av = reinterpret_cast<const f32x4*>(a)[i], gv = reinterpret_cast<const f32x4*>(g)[i];
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = av[j] * sigmoidf_(gv[j]);
        reinterpret_cast<f32x4*>(y)[i] = o;
    }
