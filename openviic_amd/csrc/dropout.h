// Training dropout (include/ovc.h, ovc_forward_backward_dropout): the counter-based keep decision shared by the GEMM epilogue
// (gemm.hip), the backward kernels (backward.hip) and ovc_dropout_mask.  Mirrored bit for bit on the host by
// openviic_amd/dropout.py.
//
//   idx  = row * cols + col                          (64-bit; cols = the product's logical column count)
//   r    = Philox4x32-10(counter = (lo32(idx >> 2), hi32(idx >> 2), site, 0), key = (lo32(seed), hi32(seed)))[idx & 3]
//   keep = r >= thr,  thr = uint32(floor(p * 2^32 + 0.5)) clamped to 2^32 - 1;  out = keep ? x * s : 0,  s = fp32(1 / (1 - p))
//
// The decision is a pure function of (seed, site, row, col): never of the tiling, grid, stream or batch position of a launch, so
// the forward's masks and the backward's regenerated ones agree, and every tiling / graph replay gives the same bits.
#pragma once
#include "common.h"

struct DropoutSite {
    const int64_t* seed;     // device: the 64-bit key (the training workspace's seed slot)
    uint32_t site;           // counter word 2 (include/ovc.h: site numbering)
    uint32_t thr;            // keep iff r >= thr
    float scale;             // s = fp32(1 / (1 - p))
    int cols;                // logical column count of the masked tensor
};

__host__ __device__ __forceinline__ uint32_t ovc_mulhi32(uint32_t a, uint32_t b) {
    return (uint32_t)(((uint64_t)a * b) >> 32);
}

// Philox4x32-10 (Salmon et al., SC'11), word `w` of the output block
__device__ __forceinline__ uint32_t ovc_philox_word(uint64_t key, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, int w) {
    uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t lo0 = 0xD2511F53u * c0, hi0 = ovc_mulhi32(0xD2511F53u, c0);
        const uint32_t lo1 = 0xCD9E8D57u * c2, hi1 = ovc_mulhi32(0xCD9E8D57u, c2);
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return w == 0 ? c0 : (w == 1 ? c1 : (w == 2 ? c2 : c3));
}

__device__ __forceinline__ bool ovc_dropout_keep(uint64_t seed, uint32_t site, uint64_t idx, uint32_t thr) {
    const uint64_t g = idx >> 2;
    return ovc_philox_word(seed, (uint32_t)g, (uint32_t)(g >> 32), site, 0u, (int)(idx & 3)) >= thr;
}

// Host: the per-site constants from p (the caller has checked 0 <= p < 1)
static inline uint32_t ovc_dropout_threshold(float p) {
    const double t = (double)p * 4294967296.0 + 0.5;
    return t >= 4294967295.0 ? 0xffffffffu : (uint32_t)t;
}
static inline float ovc_dropout_scale(float p) { return (float)(1.0 / (1.0 - (double)p)); }
