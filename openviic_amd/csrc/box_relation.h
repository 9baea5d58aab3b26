#pragma once
// The box-relation embedding emb(i, j) of a region pair (models/utils.py:156-216), shared by the forward (rowops.hip,
// box_relation_kernel) and its backward (backward.hip, bw_box_relation_kernel): both form every value with these expressions, so
// the backward's recomputed embedding is the forward's, bit for bit.
#include "common.h"

struct BoxGeom { float cx, cy, w, h; };

__device__ __forceinline__ BoxGeom box_geom(const float* __restrict__ b) {
    return BoxGeom{(b[0] + b[2]) * 0.5f, (b[1] + b[3]) * 0.5f, (b[2] - b[0]) + 1.0f, (b[3] - b[1]) + 1.0f};
}

// the four log-ratios of query box i against key box j
__device__ __forceinline__ void box_relation_logs(const BoxGeom& i, const BoxGeom& j, float g[4]) {
    g[0] = logf(fmaxf(fabsf((i.cx - j.cx) / i.w), 1e-3f));
    g[1] = logf(fmaxf(fabsf((i.cy - j.cy) / i.h), 1e-3f));
    g[2] = logf(i.w / j.w);
    g[3] = logf(i.h / j.h);
}

// the trigonometric embedding's angle of log-ratio gc at frequency q of nf = d_g / 8: embedding = [sin(ang) for c, q] ++ [cos(ang)],
// f_q = wave_len^(-q / nf)
__device__ __forceinline__ float box_relation_angle(float gc, int q, int nf) {
    const float freq = 1.0f / powf(1000.0f, (float)q / (float)nf);
    return (100.0f * gc) * freq;
}
