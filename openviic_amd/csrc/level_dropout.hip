// Level-keyed dropout (ovc_forward_backward_level_dropout): the row kernels of the meshed decoder's
// enc_attn.dropout, ONE nn.Dropout module that the layer applies once per encoder level.  Counter word 3 of the keep decision is the
// level (csrc/dropout.h, ovc_dropout_keep_level); the loss form's masked epilogue is gemm_f32_mfma_level_dropout (gemm.hip).  The search
// and the sequence form (ovc_beam_search_level_dropout, ovc_sequence_backward_level_dropout) key the same
// decision by the search's mask rows: their kernels are the second half of this file.
#include <algorithm>
#include "backward.h"

namespace {

// bw_layer_norm_dropout_kernel (backward.hip) over stacked blocks of level_rows rows, one block per encoder level (the meshed
// decoder's shared AddNorm): row r is masked as decoder row r % level_rows at level r / level_rows.  The body is the shared one,
// untouched: inside it the keep decision is spelled ovc_dropout_keep(seed, site, idx, thr), and this instance reads that spelling
// as the level-keyed decision of the row's level.  dx, prod and dyc keep the plain kernel's bits (the body's loops are its loops),
// and level 0's dproj is bw_layer_norm_dropout_kernel's.  One wave per row; d <= 2048.
__global__ __launch_bounds__(256) void bw_layer_norm_dropout_level_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                                          const float* __restrict__ dy, const uint8_t* __restrict__ zero_rows,
                                                                          float eps, int rows, int d, float* __restrict__ dx,
                                                                          float* __restrict__ prod, float* __restrict__ dyc,
                                                                          float* __restrict__ dproj, DropoutSite drop, int level_rows) {
#define OVC_BW_MASK_ROW (uint32_t)(row % level_rows)
#define ovc_dropout_keep(seed, site, idx, thr) ovc_dropout_keep_level(seed, site, (uint32_t)(row / level_rows), idx, thr)
#include "bodies/bw_layer_norm_dropout.inc"
#undef ovc_dropout_keep
#undef OVC_BW_MASK_ROW
}

// keep[r * cols + c] = the level-keyed keep decision of (site, level, r, c): backward.hip's dropout_mask_kernel at one level
__global__ void dropout_mask_level_kernel(const int64_t* __restrict__ seed_ptr, uint32_t site, uint32_t level, uint32_t thr, long rows,
                                          long cols, uint8_t* __restrict__ keep) {
    const uint64_t seed = (uint64_t)*seed_ptr;
    const uint64_t n = (uint64_t)rows * (uint64_t)cols;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        keep[i] = ovc_dropout_keep_level(seed, site, level, i, thr) ? 1 : 0;
}

// ---- the search and the sequence form (ovc_beam_search_level_dropout, ovc_sequence_backward_level_dropout) ----
// There the mask row of a decoder row is not the row itself: a decode step's row r is beam slot r % width of image r / width (mask
// row ovc_decode_mask_row), a recomputed row reads its mask row from the table built from the search's slots.  The stacked row m of
// the shared AddNorm is decoder row r = m % level_rows at level m / level_rows; the quotient comes from a host-computed constant
// (magic = floor(2^32 / level_rows) + 1: mulhi is never low and at most one high, corrected once -- gemm.hip's fast_div).
__device__ __forceinline__ int level_of_row(int m, unsigned magic, int level_rows) {
    if (level_rows == 1) return m;
    const unsigned q = __umulhi((unsigned)m, magic);
    return (int)(q * (unsigned)level_rows > (unsigned)m ? q - 1 : q);
}

// The AddNorm of the meshed decode step at enc_attn.dropout: rowops.hip's layer_norm_rows_dropout<kVecs, 1, false> over the stacked
// rows, with the level as counter word 3 and ONE residual row (x1[r]) under every level's block.  The body is the shared one; the
// residual row is its OVC_LN_RES_ROW hook, absent in every other instance.  One wave per row, one Philox block per float4.
#define OVC_LN_PARAMS                                                                                                          \
    const float* __restrict__ x, long part_stride, const float* __restrict__ bias, const float* __restrict__ residual,           \
        const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ add, int add_rows,            \
        const uint8_t* __restrict__ zero_rows, float eps, float* __restrict__ y, int rows, int d
template <int kVecs>
__global__ __launch_bounds__(256) void layer_norm_rows_level_dropout(OVC_LN_PARAMS, DropoutSite drop, DecodeRowKey key, int level_rows,
                                                                     unsigned level_magic, const int32_t* __restrict__ gate) {
    if (gate && ovc_gate_closed(gate)) return;
    constexpr int kParts = 1;
    constexpr bool kBias = false, kRes = true;
    constexpr int kPostTenths = 0;
    const uint64_t drop_seed = (uint64_t)*drop.seed;
#define OVC_LN_LEVEL level_of_row(row, level_magic, level_rows)
#define OVC_LN_RES_ROW (row - OVC_LN_LEVEL * level_rows)
#define OVC_LN_MASK(vec, c)                                                                                                     \
    do {                                                                                                                        \
        const int level_ = OVC_LN_LEVEL;                                                                                        \
        const uint64_t g_ = ((ovc_decode_mask_row(key, row - level_ * level_rows) * (uint64_t)drop.cols) >> 2) + (uint64_t)(c); \
        const uint32_t keep_ = ovc_dropout_keep4_level(drop_seed, drop.site, (uint32_t)level_, g_, drop.thr);                   \
        _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_) vec[j_] = (keep_ >> j_) & 1u ? vec[j_] * drop.scale : 0.f;             \
    } while (0)
#include "bodies/layer_norm_rows.inc"
#undef OVC_LN_MASK
#undef OVC_LN_RES_ROW
#undef OVC_LN_LEVEL
}
#undef OVC_LN_PARAMS

// rowops.hip's dropout_rows_kernel at a level, through the row table: x[m, :] = (keep ? x[m, :] * s : 0) + residual[r, :] with mask row
// rowmap[r], r = m % level_rows, level m / level_rows (the recompute of ovc_sequence_backward_level_dropout)
__global__ __launch_bounds__(256) void dropout_rows_level_kernel(float* __restrict__ x, const float* __restrict__ residual, int rows, int cols,
                                                                 DropoutSite drop, const int32_t* __restrict__ rowmap, int level_rows,
                                                                 unsigned level_magic) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const uint64_t seed = (uint64_t)*drop.seed;
    const int level = level_of_row(row, level_magic, level_rows), r = row - level * level_rows;
    const uint64_t g0 = ((uint64_t)(uint32_t)rowmap[r] * (uint64_t)drop.cols) >> 2;
    f32x4* xr = reinterpret_cast<f32x4*>(x + (size_t)row * cols);
    const f32x4* rr = reinterpret_cast<const f32x4*>(residual + (size_t)r * cols);
    for (int c = lane; c < (cols >> 2); c += 64) {
        f32x4 v = xr[c];
        const uint32_t keep = ovc_dropout_keep4_level(seed, drop.site, (uint32_t)level, g0 + (uint64_t)c, drop.thr);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (keep >> j) & 1u ? v[j] * drop.scale : 0.f;
        v += rr[c];
        xr[c] = v;
    }
}

// bw_layer_norm_dropout_level_kernel under a row table: mask row rowmap[row % level_rows], level row / level_rows.  The same body
// include, so dx, prod and dyc keep the plain kernel's bits.
__global__ __launch_bounds__(256) void bw_layer_norm_dropout_level_mapped_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                                                 const float* __restrict__ dy,
                                                                                 const uint8_t* __restrict__ zero_rows, float eps, int rows,
                                                                                 int d, float* __restrict__ dx, float* __restrict__ prod,
                                                                                 float* __restrict__ dyc, float* __restrict__ dproj,
                                                                                 DropoutSite drop, int level_rows,
                                                                                 const int32_t* __restrict__ rowmap) {
#define OVC_BW_MASK_ROW (uint32_t)rowmap[row % level_rows]
#define ovc_dropout_keep(seed, site, idx, thr) ovc_dropout_keep_level(seed, site, (uint32_t)(row / level_rows), idx, thr)
#include "bodies/bw_layer_norm_dropout.inc"
#undef ovc_dropout_keep
#undef OVC_BW_MASK_ROW
}

// keep[i * cols + c] = the level-keyed keep decision of (site, level, mask_rows[i], c): backward.hip's dropout_mask_rows_kernel at one
// level
__global__ void dropout_mask_rows_level_kernel(const int64_t* __restrict__ seed_ptr, uint32_t site, uint32_t level, uint32_t thr,
                                               const int32_t* __restrict__ rowmap, long rows, long cols, uint8_t* __restrict__ keep) {
    const uint64_t seed = (uint64_t)*seed_ptr;
    const uint64_t n = (uint64_t)rows * (uint64_t)cols;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = i / (uint64_t)cols, c = i - r * (uint64_t)cols;
        keep[i] = ovc_dropout_keep_level(seed, site, level, (uint64_t)(uint32_t)rowmap[r] * (uint64_t)cols + c, thr) ? 1 : 0;
    }
}

inline unsigned level_magic_of(int level_rows) {
    return level_rows > 1 ? (unsigned)(((uint64_t)1 << 32) / (uint64_t)level_rows + 1) : 0u;
}

}  // namespace

int ovc_layer_norm_level_dropout(const float* v, const float* residual, const float* gamma, const float* beta, float eps, float* y, int rows,
                                 int level_rows, int d, const DropoutSite& drop, const DecodeRowKey& key, hipStream_t stream,
                                 const int32_t* gate) {
    if (!v || !residual || !gamma || !beta || !y || rows <= 0 || d <= 0 || (d & 3) || d > 2048) return OVC_EINVAL;
    if (level_rows <= 0 || rows % level_rows || rows / level_rows > OVC_MAX_LEVELS) return OVC_EINVAL;
    if (!drop.seed || drop.cols != d || key.width < 1 || key.k < key.width || key.T < 1 || key.t < 0 || key.t >= key.T) return OVC_EINVAL;
    if (!ovc_aligned16(v) || !ovc_aligned16(y) || !ovc_aligned16(residual) || !ovc_aligned16(gamma) || !ovc_aligned16(beta)) return OVC_EINVAL;
    const int vecs = ((d >> 2) + 63) / 64;
    const dim3 grid((rows + 3) / 4), block(256);
    const unsigned magic = level_magic_of(level_rows);
#define OVC_LN_LEVEL_DROP(V) hipLaunchKernelGGL((layer_norm_rows_level_dropout<V>), grid, block, 0, stream, v, 0L, (const float*)nullptr, \
                                                residual, gamma, beta, (const float*)nullptr, 0, (const uint8_t*)nullptr, eps, y, rows, d, \
                                                drop, key, level_rows, magic, gate)
    if (vecs <= 1) OVC_LN_LEVEL_DROP(1);
    else if (vecs <= 2) OVC_LN_LEVEL_DROP(2);
    else if (vecs <= 4) OVC_LN_LEVEL_DROP(4);
    else OVC_LN_LEVEL_DROP(8);
#undef OVC_LN_LEVEL_DROP
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

int ovc_dropout_rows_level(float* x, const float* residual, int rows, int level_rows, int cols, const DropoutSite& drop,
                           const int32_t* rowmap, hipStream_t stream) {
    if (!x || !residual || !rowmap || rows <= 0 || cols <= 0 || (cols & 3) || !drop.seed || drop.cols != cols || !ovc_aligned16(x) ||
        !ovc_aligned16(residual) || level_rows <= 0 || rows % level_rows || rows / level_rows > OVC_MAX_LEVELS) return OVC_EINVAL;
    hipLaunchKernelGGL(dropout_rows_level_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, x, residual, rows, cols, drop, rowmap,
                       level_rows, level_magic_of(level_rows));
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

int ovc_bw_layer_norm_dropout_level_mapped(const float* x, const float* gamma, const float* dy, const uint8_t* zero_rows, float eps,
                                           int rows, int d, float* dx, float* prod, float* dyc, float* dproj, const DropoutSite& drop,
                                           int level_rows, const int32_t* rowmap, hipStream_t s) {
    if (d > 2048 || !drop.seed || drop.cols != d || !rowmap || level_rows <= 0 || rows % level_rows) return OVC_EINVAL;
    hipLaunchKernelGGL(bw_layer_norm_dropout_level_mapped_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, x, gamma, dy, zero_rows, eps, rows,
                       d, dx, prod, dyc, dproj, drop, level_rows, rowmap);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

extern "C" int ovc_dropout_mask_rows_level(const int64_t* seed, int site, int level, const int32_t* mask_rows, long rows, long cols, float p,
                                           uint8_t* keep, ovc_stream stream) {
    if (!seed || !keep || !mask_rows || site < 0 || site >= OVC_DROPOUT_SITES || level < 0 || level >= OVC_MAX_LEVELS || rows < 0 ||
        cols < 0 || !(p >= 0.f && p < 1.f))
        return OVC_EINVAL;
    if (rows == 0 || cols == 0) return OVC_OK;
    if (const int rc = ovc_device_guard()) return rc;
    const uint64_t n = (uint64_t)rows * (uint64_t)cols;
    const unsigned blocks = (unsigned)std::min<uint64_t>((n + 255) / 256, 8192);
    hipLaunchKernelGGL(dropout_mask_rows_level_kernel, dim3(blocks), dim3(256), 0, ovc_hip_stream(stream), seed, (uint32_t)site,
                       (uint32_t)level, ovc_dropout_threshold(p), mask_rows, rows, cols, keep);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

// Test hook (tests/test_meshed_scst_dropout_gpu.py): the level-keyed AddNorm of a meshed decode step alone, as the search launches it.
// v [levels * level_rows][d] the finished projections, residual [level_rows][d], y [levels * level_rows][d]; (width, k, T, t) the step's
// row key.  OVC_EINVAL, nothing launched: what ovc_layer_norm_level_dropout refuses, p outside [0, 1), a site out of range.
extern "C" int ovc_debug_add_norm_level_dropout(const float* v, const float* residual, const float* gamma, const float* beta, float eps,
                                                float* y, int levels, int level_rows, int d, const int64_t* seed, int site, float p,
                                                int width, int k, int T, int t, const int32_t* gate, ovc_stream stream) {
    if (!seed || !(p >= 0.f && p < 1.f) || site < 0 || site >= OVC_DROPOUT_SITES || levels < 1 || levels > OVC_MAX_LEVELS || level_rows < 1)
        return OVC_EINVAL;
    if (const int rc = ovc_device_guard()) return rc;
    const DropoutSite drop{seed, (uint32_t)site, ovc_dropout_threshold(p), ovc_dropout_scale(p), d};
    return ovc_layer_norm_level_dropout(v, residual, gamma, beta, eps, y, levels * level_rows, level_rows, d, drop,
                                        DecodeRowKey{width, k, T, t}, ovc_hip_stream(stream), gate);
}

int ovc_bw_layer_norm_dropout_level(const float* x, const float* gamma, const float* dy, const uint8_t* zero_rows, float eps, int rows,
                                    int d, float* dx, float* prod, float* dyc, float* dproj, const DropoutSite& drop, int level_rows,
                                    hipStream_t s) {
    if (d > 2048 || !drop.seed || drop.cols != d || level_rows <= 0 || rows % level_rows) return OVC_EINVAL;
    hipLaunchKernelGGL(bw_layer_norm_dropout_level_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, x, gamma, dy, zero_rows, eps, rows, d,
                       dx, prod, dyc, dproj, drop, level_rows);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

extern "C" int ovc_dropout_mask_level(const int64_t* seed, int site, int level, long rows, long cols, float p, uint8_t* keep,
                                      ovc_stream stream) {
    if (!seed || !keep || site < 0 || site >= OVC_DROPOUT_SITES || level < 0 || level >= OVC_MAX_LEVELS || rows < 0 || cols < 0 ||
        !(p >= 0.f && p < 1.f))
        return OVC_EINVAL;
    if (rows == 0 || cols == 0) return OVC_OK;
    if (const int rc = ovc_device_guard()) return rc;
    const uint64_t n = (uint64_t)rows * (uint64_t)cols;
    const unsigned blocks = (unsigned)std::min<uint64_t>((n + 255) / 256, 8192);
    hipLaunchKernelGGL(dropout_mask_level_kernel, dim3(blocks), dim3(256), 0, ovc_hip_stream(stream), seed, (uint32_t)site,
                       (uint32_t)level, ovc_dropout_threshold(p), rows, cols, keep);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}
