// Level-keyed dropout (ovc_forward_backward_level_dropout): the row kernels of the meshed decoder's
// enc_attn.dropout, ONE nn.Dropout module that the layer applies once per encoder level.  Counter word 3 of the keep decision is the
// level (csrc/dropout.h, ovc_dropout_keep_level); the forward's masked epilogue is gemm_f32_mfma_level_dropout (gemm.hip).
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

}  // namespace

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
