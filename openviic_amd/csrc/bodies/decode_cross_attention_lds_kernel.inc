// The body of decode_cross_attention_lds_kernel and its gated instance (attention.hip): included verbatim into both kernels, so that the
// ungated one compiles exactly as before.  Not a header: no include guard.
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x, hd = blockIdx.y, lvl = blockIdx.z;
    const int N = p.n, W = p.width;
    float* Xs = lds;                         // [128][68]: a chunk of K rows, later of V rows
    float* qs = Xs + kCrossChunk * kLdQK;    // [W][64]
    float* sc = qs + W * 64;                 // [W][N]

    const float* kg = p.kx + (size_t)lvl * p.level_stride + (size_t)b * N * p.ldkv;
    const float* vg = p.vx + (size_t)lvl * p.level_stride + (size_t)b * N * p.ldkv;
    const int c4 = tid & 15, r0 = tid >> 4, col = c4 * 4;
    for (int idx = tid; idx < W * 16; idx += 256) {
        const int i = idx >> 4, cc = (idx & 15) * 4;
        f32x4 qv = {0.f, 0.f, 0.f, 0.f};
        if (cc < p.dk) qv = *reinterpret_cast<const f32x4*>(p.q + (size_t)(b * W + i) * p.ldq + hd * p.dk + cc);
        *reinterpret_cast<f32x4*>(qs + i * 64 + cc) = qv;
    }
    const float scale_div = sqrtf((float)p.dk);
    const int k4n = (p.dk + 3) >> 2;
    for (int k0 = 0; k0 < N; k0 += kCrossChunk) {
        const int nc = min(kCrossChunk, N - k0);
        for (int r = r0; r < nc; r += 16) {
            f32x4 kv = {0.f, 0.f, 0.f, 0.f};
            if (col < p.dk) kv = *reinterpret_cast<const f32x4*>(kg + (size_t)(k0 + r) * p.ldkv + hd * p.dk + col);
            *reinterpret_cast<f32x4*>(Xs + r * kLdQK + col) = kv;
        }
        __syncthreads();
        for (int idx = tid; idx < W * nc; idx += 256) {
            const int i = idx / nc, j = idx - i * nc;
            const f32x4* kr = reinterpret_cast<const f32x4*>(Xs + j * kLdQK);
            const f32x4* qr = reinterpret_cast<const f32x4*>(qs + i * 64);
            float acc = 0.f;
            for (int c = 0; c < k4n; ++c) {
                const f32x4 a = qr[c], kk = kr[c];
                acc += (a[0] * kk[0] + a[1] * kk[1]) + (a[2] * kk[2] + a[3] * kk[3]);
            }
            float s = acc / scale_div;
            if (p.encmask && p.encmask[(size_t)b * N + k0 + j]) s = -INFINITY;
            sc[i * N + k0 + j] = s;
        }
        __syncthreads();
    }
    for (int i = wave; i < W; i += 4) {
        float mx = -INFINITY;
        for (int j = lane; j < N; j += 64) mx = fmaxf(mx, sc[i * N + j]);
        mx = wave_max(mx);
        float sum = 0.f;
        for (int j = lane; j < N; j += 64) {
            const float e = expf(sc[i * N + j] - mx);
            sc[i * N + j] = e;
            sum += e;
        }
        sum = wave_sum(sum);
        for (int j = lane; j < N; j += 64) sc[i * N + j] = sc[i * N + j] / sum;
    }
    // out[i][d] = sum_j P[i][j] V[j][d], j ascending; W * d_v <= 512 outputs: at most two per thread
    const int nout = W * p.dv;
    float acc[2] = {0.f, 0.f};
    for (int k0 = 0; k0 < N; k0 += kCrossChunk) {
        const int nc = min(kCrossChunk, N - k0);
        __syncthreads();                                   // the probabilities are complete / the previous chunk is consumed
        for (int r = r0; r < nc; r += 16) {
            f32x4 vv = {0.f, 0.f, 0.f, 0.f};
            if (col < p.dv) vv = *reinterpret_cast<const f32x4*>(vg + (size_t)(k0 + r) * p.ldkv + hd * p.dv + col);
            *reinterpret_cast<f32x4*>(Xs + r * kLdQK + col) = vv;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int idx = tid + 256 * u;
            if (idx < nout) {
                const int i = idx / p.dv, d = idx - i * p.dv;
                for (int j = 0; j < nc; ++j) acc[u] += sc[i * N + k0 + j] * Xs[j * kLdQK + d];
            }
        }
    }
    float* og = p.out + (size_t)lvl * p.out_level_stride;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int idx = tid + 256 * u;
        if (idx < nout) {
            const int i = idx / p.dv, d = idx - i * p.dv;
            og[(size_t)(b * W + i) * p.ldo + hd * p.dv + d] = acc[u];
        }
    }
