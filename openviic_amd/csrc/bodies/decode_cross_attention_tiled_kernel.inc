// The body of decode_cross_attention_tiled_kernel and its gated instance (attention.hip): included verbatim into both kernels, so that the
// ungated one compiles exactly as before.  Not a header: no include guard.
    constexpr int NT = 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x, hd = min((int)blockIdx.y * 4 + wave, p.heads - 1), lvl = blockIdx.z;
    const bool live = (int)blockIdx.y * 4 + wave < p.heads;
    const int N = p.n, W = p.width;
    const int r = lane & 15, kq = lane >> 4;
    const float* kg = p.kx + (size_t)lvl * p.level_stride + (size_t)b * N * p.ldkv + hd * p.dk;
    const float* vg = p.vx + (size_t)lvl * p.level_stride + (size_t)b * N * p.ldkv + hd * p.dv;
    const float* qg = p.q + (size_t)(b * W + min(r, W - 1)) * p.ldq + hd * p.dk;
    const uint8_t* mrow = p.encmask ? p.encmask + (size_t)b * N : nullptr;

    f32x4 qf[SB];
#pragma unroll
    for (int S = 0; S < SB; ++S) qf[S] = *reinterpret_cast<const f32x4*>(qg + 16 * S + 4 * kq);
    if (r >= W) {
#pragma unroll
        for (int S = 0; S < SB; ++S) qf[S] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const float scale_div = sqrtf((float)p.dk);
    const int vc = 4 * min(r, (p.dv >> 2) - 1);
    float m_run = -INFINITY, l_run = 0.f;
    f32x4 acc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int k0 = 0; k0 < N; k0 += 16 * NT) {
        f32x4 kf[NT][SB];
#pragma unroll
        for (int T = 0; T < NT; ++T) {
            const float* krow = kg + (size_t)min(k0 + 16 * T + r, N - 1) * p.ldkv + 4 * kq;
#pragma unroll
            for (int S = 0; S < SB; ++S) kf[T][S] = *reinterpret_cast<const f32x4*>(krow + 16 * S);
        }
        uint8_t mk[NT][4];
#pragma unroll
        for (int T = 0; T < NT; ++T)
#pragma unroll
            for (int g = 0; g < 4; ++g) mk[T][g] = 0;
        if (mrow) {
#pragma unroll
            for (int T = 0; T < NT; ++T)
#pragma unroll
                for (int g = 0; g < 4; ++g) mk[T][g] = mrow[min(k0 + 16 * T + 4 * kq + g, N - 1)];
        }
        f32x4 st[NT];
#pragma unroll
        for (int T = 0; T < NT; ++T) st[T] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int S = 0; S < SB; ++S)
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int T = 0; T < NT; ++T) st[T] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[T][S][e], qf[S][e], st[T], 0, 0, 0);
        f32x4 vf[NT][4];
#pragma unroll
        for (int T = 0; T < NT; ++T)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                vf[T][g] = *reinterpret_cast<const f32x4*>(vg + (size_t)min(k0 + 16 * T + 4 * kq + g, N - 1) * p.ldkv + vc);

        float mx = -INFINITY;
#pragma unroll
        for (int T = 0; T < NT; ++T)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int key = k0 + 16 * T + 4 * kq + g;
                float s = st[T][g] / scale_div;
                if (key >= N || mk[T][g]) s = -INFINITY;
                st[T][g] = s;
                mx = fmaxf(mx, s);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);
        const bool none = m_new == -INFINITY;
        const float alpha = none ? 1.f : expf(m_run - m_new);
        float sum = 0.f;
#pragma unroll
        for (int T = 0; T < NT; ++T)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float e = none ? 0.f : expf(st[T][g] - m_new);
                st[T][g] = e;
                sum += e;
            }
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        l_run = l_run * alpha + sum;
        m_run = m_new;
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = acc[e] * alpha;
#pragma unroll
        for (int T = 0; T < NT; ++T)
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[T][g][e], st[T][g], acc[e], 0, 0, 0);
    }
    if (live && r < W) {
        float* orow = p.out + (size_t)lvl * p.out_level_stride + (size_t)(b * W + r) * p.ldo + hd * p.dv;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int dvb = 16 * kq + 4 * g;
            if (dvb < p.dv)
                *reinterpret_cast<f32x4*>(orow + dvb) = f32x4{acc[0][g] / l_run, acc[1][g] / l_run, acc[2][g] / l_run, acc[3][g] / l_run};
        }
    }
