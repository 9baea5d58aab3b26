// The body of layer_norm_rows and its gated instance (rowops.hip): included verbatim into both kernels, so that the
// ungated one compiles exactly as before.  Not a header: no include guard.
    // every argument in ONE scalar round trip (hipcc otherwise fetches `rows` for the guard below first and the pointers in a
    // second, dependent round: the kernel is nothing but a chain of round trips -- gemm.hip, round 4)
    asm volatile("" ::"s"(x), "s"(part_stride), "s"(bias), "s"(residual), "s"(gamma), "s"(beta), "s"(add), "s"(add_rows), "s"(zero_rows),
                 "s"(eps), "s"(y), "s"(rows), "s"(d));
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int nvec = d >> 2;
    float* yrow = y + (size_t)row * d;
    // The row's "write zeros instead" flag travels WITH the row's loads and is applied as a select on the way out.  (Until round 4
    // this was an early `if (cleared) { store zeros; return; }` behind the loads in the source -- hipcc moved the test in front of
    // them and waited for the byte: one whole extra round trip in every launch that takes the flags.)
    // (an unconditional load from an always-valid address: a load inside `if (zero_rows)` gets a full s_waitcnt at the join)
    const uint8_t cleared_byte = *(zero_rows ? zero_rows + row : reinterpret_cast<const uint8_t*>(gamma));
    const bool cleared = zero_rows != nullptr && cleared_byte != 0;
    // column group of (lane, i), clamped in-range: out-of-range lanes load a valid address and are masked later
    int col[kVecs];
#pragma unroll
    for (int i = 0; i < kVecs; ++i) col[i] = min(lane + i * 64, nvec - 1);
    f32x4 part[kParts][kVecs], bv[kVecs], rv[kVecs];
#pragma unroll
    for (int s = 0; s < kParts; ++s)
#pragma unroll
        for (int i = 0; i < kVecs; ++i)
            part[s][i] = reinterpret_cast<const f32x4*>(x + s * part_stride + (size_t)row * d)[col[i]];
    if (kBias) {
#pragma unroll
        for (int i = 0; i < kVecs; ++i) bv[i] = reinterpret_cast<const f32x4*>(bias)[col[i]];
    }
#ifdef OVC_LN_RES_ROW                   // the level-keyed instance (level_dropout.hip): one residual row under every level's block
    if (kRes) {
#pragma unroll
        for (int i = 0; i < kVecs; ++i) rv[i] = reinterpret_cast<const f32x4*>(residual + (size_t)(OVC_LN_RES_ROW) * d)[col[i]];
    }
#else
    if (kRes) {
#pragma unroll
        for (int i = 0; i < kVecs; ++i) rv[i] = reinterpret_cast<const f32x4*>(residual + (size_t)row * d)[col[i]];
    }
#endif
    // gamma / beta do not depend on the row's moments: fetched now, not after them (one memory round trip less
    // on a kernel that is nothing but a chain of them)
    f32x4 gv[kVecs], bev[kVecs];
#pragma unroll
    for (int i = 0; i < kVecs; ++i) {
        gv[i] = reinterpret_cast<const f32x4*>(gamma)[col[i]];
        bev[i] = reinterpret_cast<const f32x4*>(beta)[col[i]];
    }
    f32x4 v[kVecs];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < kVecs; ++i) {
        v[i] = part[0][i];
#pragma unroll
        for (int s = 1; s < kParts; ++s) v[i] += part[s][i];
        if (kBias) v[i] += bv[i];
#ifdef OVC_LN_MASK
        OVC_LN_MASK(v[i], col[i]);      // the dropout instances (layer_norm_rows_dropout): the finished projection, before the residual
#endif
        if (kRes) v[i] += rv[i];
        if (lane + i * 64 < nvec) sum += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
    }
    const float mean = wave_sum(sum) / (float)d;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < kVecs; ++i) {
        if (lane + i * 64 < nvec) {
            const f32x4 t = v[i] - mean;
            sq += (t[0] * t[0] + t[1] * t[1]) + (t[2] * t[2] + t[3] * t[3]);
        }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)d + eps);
    const f32x4* ar = add ? reinterpret_cast<const f32x4*>(add + (size_t)(row % add_rows) * d) : nullptr;
#pragma unroll
    for (int i = 0; i < kVecs; ++i) {
        const int c = lane + i * 64;
        if (c < nvec) {
            f32x4 o = (v[i] - mean) * rstd * gv[i] + bev[i];
            if (ar) o += ar[c];
            if constexpr (kPostTenths > 0) o = ((float)kPostTenths / 10.f) * o + rv[i];
            if (cleared) o = f32x4{0.f, 0.f, 0.f, 0.f};
            reinterpret_cast<f32x4*>(yrow)[c] = o;
        }
    }
