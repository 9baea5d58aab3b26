// Training dropout (include/ovc.h, ovc_forward_backward_dropout): the counter-based keep decision shared by the GEMM epilogue
// (gemm.hip), the backward kernels (backward.hip) and ovc_dropout_mask.  Mirrored bit for bit on the host by
// openviic_amd/dropout.py.
//
//   idx  = row * cols + col                          (64-bit; cols = the product's logical column count)
//   r    = Philox4x32-10(counter = (lo32(idx >> 2), hi32(idx >> 2), site, level), key = (lo32(seed), hi32(seed)))[idx & 3]
//   keep = r >= thr,  thr = uint32(floor(p * 2^32 + 0.5)) clamped to 2^32 - 1;  out = keep ? x * s : 0,  s = fp32(1 / (1 - p))
//
// level is 0 everywhere but at the meshed decoder's enc_attn.dropout, which one module applies once per encoder level: there it is
// the level, with the decoder row b * T + t the same at every level (ovc_dropout_keep_level).
//
// The decision is a pure function of (seed, site, level, row, col): never of the tiling, grid, stream or batch position of a
// launch, so the forward's masks and the backward's regenerated ones agree, and every tiling / graph replay gives the same bits.
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

// Philox4x32-10 (Salmon et al., SC'11): the output block of counter (c0..c3) under `key`, left in c0..c3
__device__ __forceinline__ void ovc_philox_block(uint64_t key, uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3) {
    uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t lo0 = 0xD2511F53u * c0, hi0 = ovc_mulhi32(0xD2511F53u, c0);
        const uint32_t lo1 = 0xCD9E8D57u * c2, hi1 = ovc_mulhi32(0xCD9E8D57u, c2);
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// word `w` of the output block
__device__ __forceinline__ uint32_t ovc_philox_word(uint64_t key, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, int w) {
    ovc_philox_block(key, c0, c1, c2, c3);
    return w == 0 ? c0 : (w == 1 ? c1 : (w == 2 ? c2 : c3));
}

__device__ __forceinline__ bool ovc_dropout_keep(uint64_t seed, uint32_t site, uint64_t idx, uint32_t thr) {
    const uint64_t g = idx >> 2;
    return ovc_philox_word(seed, (uint32_t)g, (uint32_t)(g >> 32), site, 0u, (int)(idx & 3)) >= thr;
}

// The level-keyed decision (ovc_forward_backward_level_dropout): ONE nn.Dropout module applied once per encoder level, as the meshed
// decoder applies enc_attn.dropout -- the level is counter word 3, so the levels' masks are independent, level 0 is
// ovc_dropout_keep bit for bit, and the mask is a pure function of (seed, site, level, row, col).
__device__ __forceinline__ bool ovc_dropout_keep_level(uint64_t seed, uint32_t site, uint32_t level, uint64_t idx, uint32_t thr) {
    const uint64_t g = idx >> 2;
    return ovc_philox_word(seed, (uint32_t)g, (uint32_t)(g >> 32), site, level, (int)(idx & 3)) >= thr;
}

// The four keep decisions of element group g (elements 4 g .. 4 g + 3 of the site's index space) as bits 0..3: one Philox block.
// Bit j is ovc_dropout_keep(seed, site, 4 g + j, thr).
__device__ __forceinline__ uint32_t ovc_dropout_keep4(uint64_t key, uint32_t site, uint64_t g, uint32_t thr) {
    uint32_t c0 = (uint32_t)g, c1 = (uint32_t)(g >> 32), c2 = site, c3 = 0u;
    ovc_philox_block(key, c0, c1, c2, c3);
    return (c0 >= thr ? 1u : 0u) | (c1 >= thr ? 2u : 0u) | (c2 >= thr ? 4u : 0u) | (c3 >= thr ? 8u : 0u);
}

// The same block at encoder level `level` (counter word 3): bit j is ovc_dropout_keep_level(seed, site, level, 4 g + j, thr), and level
// 0 is ovc_dropout_keep4.  A function of its own, so that ovc_dropout_keep4's callers keep their code.
__device__ __forceinline__ uint32_t ovc_dropout_keep4_level(uint64_t key, uint32_t site, uint32_t level, uint64_t g, uint32_t thr) {
    uint32_t c0 = (uint32_t)g, c1 = (uint32_t)(g >> 32), c2 = site, c3 = level;
    ovc_philox_block(key, c0, c1, c2, c3);
    return (c0 >= thr ? 1u : 0u) | (c1 >= thr ? 2u : 0u) | (c2 >= thr ? 4u : 0u) | (c3 >= thr ? 8u : 0u);
}

// Dropout inside the beam search (ovc_beam_search_dropout): row r of decode step t is beam slot r % width of image r / width
// (width = 1 at step 0, the beam size k later), and its decoder-side masks are keyed by the MASK ROW
//   mrow(b, slot, t) = (b * k + slot) * T + t                                        (T = max_len; k = 1: xe_loss's b * T + t)
// The teacher-forced recompute of a final beam (ovc_sequence_backward_dropout) reaches the same rows through a table built from
// the beam's ancestor slots.
struct DecodeRowKey { int width, k, T, t; };
__device__ __forceinline__ uint64_t ovc_decode_mask_row(const DecodeRowKey& key, int row) {
    const int b = row / key.width, slot = row - b * key.width;
    return ((uint64_t)b * (uint64_t)key.k + (uint64_t)slot) * (uint64_t)key.T + (uint64_t)key.t;
}

// Host: the per-site constants from p (the caller has checked 0 <= p < 1)
static inline uint32_t ovc_dropout_threshold(float p) {
    const double t = (double)p * 4294967296.0 + 0.5;
    return t >= 4294967295.0 ? 0xffffffffu : (uint32_t)t;
}
static inline float ovc_dropout_scale(float p) { return (float)(1.0 / (1.0 - (double)p)); }

// ---- row-keyed launches (rowops.hip, backward.hip) ----------------------------------------------
// LayerNorm(keep ? v * s : 0 + residual) with v = sum_s parts[s] + bias, the AddNorm of a decode-step projection at a dropout site:
// nparts in {1, 2, 4} (1: `parts` is the finished product, bias already applied, bias == nullptr), residual required.  v has the
// bits the plain AddNorm forms.  Row r is masked as mask row ovc_decode_mask_row(key, r).  gate: nullptr = ungated.
int ovc_layer_norm_parts_dropout(const float* parts, int nparts, long part_stride, const float* bias, const float* residual,
                                 const float* gamma, const float* beta, const uint8_t* zero_rows, float eps, float* y, int rows, int d,
                                 const DropoutSite& drop, const DecodeRowKey& key, hipStream_t stream, const int32_t* gate);
// x[r, :] = (keep ? x[r, :] * s : 0) + residual[r, :] in place (residual may be nullptr), cols a multiple of 4.  The mask row of
// row r is rowmap[r] when rowmap != nullptr (the teacher-forced recompute), else ovc_decode_mask_row(key, r) (the search).
int ovc_dropout_rows(float* x, const float* residual, int rows, int cols, const DropoutSite& drop, const DecodeRowKey& key,
                     const int32_t* rowmap, hipStream_t stream, const int32_t* gate);

// ---- level-keyed row launches (level_dropout.hip): the meshed decoder's enc_attn.dropout in the search and the sequence form -------
// The rows are stacked blocks of level_rows rows, one block per encoder level: stacked row m is decoder row r = m % level_rows at level
// m / level_rows, its residual row is r, and its mask is the level-keyed one (counter word 3) at the MASK ROW of r.
// LayerNorm((keep ? v * s : 0) + residual[r]) with v the finished projection (bias applied): the AddNorm of a decode step, mask row
// ovc_decode_mask_row(key, r).  gate: nullptr = ungated.
int ovc_layer_norm_level_dropout(const float* v, const float* residual, const float* gamma, const float* beta, float eps, float* y, int rows,
                                 int level_rows, int d, const DropoutSite& drop, const DecodeRowKey& key, hipStream_t stream,
                                 const int32_t* gate);
// x[m, :] = (keep ? x[m, :] * s : 0) + residual[r, :] in place, mask row rowmap[r]: the teacher-forced recompute.
int ovc_dropout_rows_level(float* x, const float* residual, int rows, int level_rows, int cols, const DropoutSite& drop,
                           const int32_t* rowmap, hipStream_t stream);
