// The body of bw_layer_norm_dropout_kernel and its row-mapped form (backward.hip): included verbatim into both.  OVC_BW_MASK_ROW is
// the mask row of `row`.  Not a header: no include guard.
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const size_t o = (size_t)row * d;
    if (zero_rows && zero_rows[row]) {
        for (int c = lane; c < d; c += 64) { dx[o + c] = 0.f; prod[o + c] = 0.f; dyc[o + c] = 0.f; dproj[o + c] = 0.f; }
        return;
    }
    const uint64_t seed = (uint64_t)*drop.seed;
    float s = 0.f;
    for (int c = lane; c < d; c += 64) s += x[o + c];
    const float mean = wave_sum(s) / d;
    float v = 0.f;
    for (int c = lane; c < d; c += 64) { const float t = x[o + c] - mean; v += t * t; }
    const float rstd = 1.f / sqrtf(wave_sum(v) / d + eps);
    float a = 0.f, b = 0.f;
    for (int c = lane; c < d; c += 64) {
        const float xh = (x[o + c] - mean) * rstd, g = gamma[c] * dy[o + c];
        a += g; b += g * xh;
    }
    a = wave_sum(a) / d; b = wave_sum(b) / d;
    for (int c = lane; c < d; c += 64) {
        const float xh = (x[o + c] - mean) * rstd, g = dy[o + c];
        dx[o + c] = rstd * (gamma[c] * g - a - xh * b);
        prod[o + c] = g * xh;
        dyc[o + c] = g;
    }
    // The masked copy in a loop of its own, from the dx this lane stored.  With dproj formed inside the loop above, the compiler
    // contracted gamma g - a - xh b otherwise than in bw_layer_norm_kernel (whose unrolled rounds fuse gamma g - a and whose odd last
    // round rounds the product first), and dx missed the plain kernel's bits at every width with an odd number of 64-column rounds.
    for (int c = lane; c < d; c += 64)
        dproj[o + c] = ovc_dropout_keep(seed, drop.site, (uint64_t)(OVC_BW_MASK_ROW) * (uint64_t)drop.cols + (uint64_t)c, drop.thr) ? dx[o + c] * drop.scale : 0.f;
