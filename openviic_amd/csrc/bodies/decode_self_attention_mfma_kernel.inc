// The body of decode_self_attention_mfma_kernel and its gated instance (attention.hip): included verbatim into both kernels, so that the
// ungated one compiles exactly as before.  Not a header: no include guard.
    constexpr int kPos = CHUNKED ? kSelfChunk : 64;      // positions the workgroup lists (one per lane of wave 0)
    __shared__ unsigned short keyinfo[NT * 16];          // (position << 3) | local slot
    __shared__ uint8_t keypad[NT * 16];
    __shared__ uint8_t sl[OVC_MAX_BEAM][kPos];           // local slot of beam i at position j0 + j
    __shared__ int nkeys_shared;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x, t = p.t, W = p.width;
    const int j0 = CHUNKED ? (int)blockIdx.z * kSelfChunk : 0;
    const int hd = min((int)blockIdx.y * 4 + wave, p.h - 1);
    const bool live = (int)blockIdx.y * 4 + wave < p.h;          // surplus waves redo the last head, store nothing
    const int r = lane & 15, kq = lane >> 4;

    // this wave's query fragments (independent of the key list: in flight while wave 0 builds it)
    const float* qg = p.q + (size_t)(b * W + min(r, W - 1)) * p.ldq + hd * p.dk;
    f32x4 qf[SB];
#pragma unroll
    for (int S = 0; S < SB; ++S) qf[S] = *reinterpret_cast<const f32x4*>(qg + 16 * S + 4 * kq);

    if (wave == 0) {
        const int j = j0 + lane;
        const int wj = j == 0 ? 1 : W;                        // slots of position j's cache block that belong to this image
        int slot[OVC_MAX_BEAM];
        uint8_t pad[OVC_MAX_BEAM];
        unsigned mask = 0;
        if (j <= t && lane < kPos) {
#pragma unroll
            for (int i = 0; i < OVC_MAX_BEAM; ++i)             // all loads first: ancestor slots and the block's <pad> flags
                slot[i] = i < W ? (j == t ? i : p.anc[(size_t)(b * W + i) * p.anc_ld + j] - b * wj) : 0;
#pragma unroll
            for (int l = 0; l < OVC_MAX_BEAM; ++l) pad[l] = l < wj ? p.padflag[(size_t)j * p.pad_ld + b * wj + l] : 0;
#pragma unroll
            for (int i = 0; i < OVC_MAX_BEAM; ++i)
                if (i < W) {
                    const int s = min(max(slot[i], 0), wj - 1);   // a corrupt table can never index outside the image's block
                    sl[i][j - j0] = (uint8_t)s;
                    mask |= 1u << s;
                }
        }
        const int cnt = __popc(mask);
        int incl = cnt;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int up = __shfl_up(incl, off, 64);
            if (lane >= off) incl += up;
        }
        int n = incl - cnt;
#pragma unroll
        for (int l = 0; l < OVC_MAX_BEAM; ++l)
            if (mask & (1u << l)) {
                if (n < NT * 16) { keyinfo[n] = (unsigned short)((j << 3) | l); keypad[n] = pad[l]; }
                ++n;
            }
        if (lane == 63) nkeys_shared = min(incl, NT * 16);
    }
    __syncthreads();
    const int nkeys = nkeys_shared;

    // ---- K fragments of the listed keys: tile T holds keys 16 T .. 16 T + 15, lane r loads key 16 T + r -------------
    f32x4 kf[NT][SB];
#pragma unroll
    for (int T = 0; T < NT; ++T) {
        if (16 * T < nkeys) {                                  // wave-uniform
            const int info = keyinfo[min(16 * T + r, nkeys - 1)];
            const int j = info >> 3, l = info & 7;
            const float* krow = p.kcache + (size_t)j * p.pos_stride + (size_t)(b * (j == 0 ? 1 : W) + l) * p.ldkv + hd * p.dk + 4 * kq;
#pragma unroll
            for (int S = 0; S < SB; ++S) kf[T][S] = *reinterpret_cast<const f32x4*>(krow + 16 * S);
        }
    }
    if (r >= W) {
#pragma unroll
        for (int S = 0; S < SB; ++S) qf[S] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    f32x4 st[NT];
#pragma unroll
    for (int T = 0; T < NT; ++T) st[T] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int T = 0; T < NT; ++T) {
        if (16 * T < nkeys) {
#pragma unroll
            for (int S = 0; S < SB; ++S)
#pragma unroll
                for (int e = 0; e < 4; ++e) st[T] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[T][S][e], qf[S][e], st[T], 0, 0, 0);
        }
    }

    // ---- V fragments (in flight during the softmax): lane (r, kq), register g <-> key 16 T + 4 kq + g, columns 4 r .. ----
    const int vc = 4 * min(r, (p.dv >> 2) - 1);
    f32x4 vf[NT][4];
#pragma unroll
    for (int T = 0; T < NT; ++T) {
        if (16 * T < nkeys) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int info = keyinfo[min(16 * T + 4 * kq + g, nkeys - 1)];
                const int j = info >> 3, l = info & 7;
                vf[T][g] = *reinterpret_cast<const f32x4*>(p.vcache + (size_t)j * p.pos_stride +
                                                           (size_t)(b * (j == 0 ? 1 : W) + l) * p.ldkv + hd * p.dv + vc);
            }
        }
    }

    // ---- scale, validity, softmax over the keys of this lane's beam column -------------------------------------------
    const float scale_div = sqrtf((float)p.dk);
    const int beam = min(r, W - 1);
    float mx = -INFINITY;
#pragma unroll
    for (int T = 0; T < NT; ++T) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int key = 16 * T + 4 * kq + g;
            float s = -INFINITY;
            if (key < nkeys) {
                const int info = keyinfo[key];
                if (!keypad[key] && sl[beam][(info >> 3) - j0] == (info & 7)) s = st[T][g] / scale_div;
            }
            st[T][g] = s;
            mx = fmaxf(mx, s);
        }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mref = CHUNKED && mx == -INFINITY ? 0.f : mx;     // no key in this chunk: every exponential is exactly 0
    float sum = 0.f;
#pragma unroll
    for (int T = 0; T < NT; ++T)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float e = expf(st[T][g] - mref);
            st[T][g] = e;
            sum += e;
        }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    if constexpr (!CHUNKED) {
#pragma unroll
        for (int T = 0; T < NT; ++T)
#pragma unroll
            for (int g = 0; g < 4; ++g) st[T][g] = st[T][g] / sum;
    }

    // ---- O^T = V^T P^T -----------------------------------------------------------------------------------------------
    f32x4 acc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int T = 0; T < NT; ++T) {
        if (16 * T < nkeys) {
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[T][g][e], st[T][g], acc[e], 0, 0, 0);
        }
    }
    if (live && r < W) {
        float* orow;
        if constexpr (CHUNKED) {
            const size_t prow = (size_t)blockIdx.z * gridDim.x * W + b * W + r;     // [chunk][row]
            orow = p.part_o + prow * p.h * p.dv + hd * p.dv;
            if (kq == 0) reinterpret_cast<float2*>(p.part_ml)[prow * p.h + hd] = make_float2(mx, sum);
        } else {
            orow = p.out + (size_t)(b * W + r) * p.ldo + hd * p.dv;
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int dvb = 16 * kq + 4 * g;
            if (dvb < p.dv) *reinterpret_cast<f32x4*>(orow + dvb) = f32x4{acc[0][g], acc[1][g], acc[2][g], acc[3][g]};
        }
    }
