// Device kernels of the training backward (ovc_forward_backward, engine.hip).  Declarations and contracts: backward.h.
// Everything here is deterministic by construction: each output element is written by one lane, and every sum over rows,
// queries, keys or columns runs in an order fixed by the shape alone.
#include <cmath>
#include "backward.h"
#include "box_relation.h"

namespace {

constexpr int kChunk = 64;             // rows per partial of the column sums

__global__ __launch_bounds__(256) void bw_transpose_kernel(const float* __restrict__ src, long lds, int rows, int cols,
                                                           float* __restrict__ dst, long ldd, int rows_pad) {
    __shared__ float tile[64][65];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int r0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
    for (int i = wv; i < 64; i += 4) {
        const int r = r0 + i, c = c0 + lane;
        tile[i][lane] = (r < rows && c < cols) ? src[(size_t)r * lds + c] : 0.f;
    }
    __syncthreads();
    for (int i = wv; i < 64; i += 4) {
        const int c = c0 + i, r = r0 + lane;
        if (c < cols && r < rows_pad) dst[(size_t)c * ldd + r] = tile[lane][i];
    }
}

__global__ __launch_bounds__(256) void bw_rowsum_kernel(const float* __restrict__ src, long ld, int rows, int n,
                                                        float* __restrict__ dst) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* p = src + (size_t)row * ld;
    float s = 0.f;
    for (int j = lane; j < n; j += 64) s += p[j];
    s = wave_sum(s);
    if (lane == 0) dst[row] = s;
}

__global__ __launch_bounds__(256) void bw_colsum_part_kernel(const float* __restrict__ src, long ld, int rows, int cols,
                                                             float* __restrict__ part) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= cols) return;
    const int r0 = blockIdx.y * kChunk, r1 = min(rows, r0 + kChunk);
    float s = 0.f;
    for (int r = r0; r < r1; ++r) s += src[(size_t)r * ld + c];
    part[(size_t)blockIdx.y * cols + c] = s;
}

__global__ __launch_bounds__(256) void bw_colsum_final_kernel(const float* __restrict__ part, int nchunks, int cols,
                                                              float* __restrict__ dst) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= cols) return;
    float s = 0.f;
    for (int i = 0; i < nchunks; ++i) s += part[(size_t)i * cols + c];
    dst[c] = s;
}

// one wave per row; d <= 2048 (32 columns per lane)
__global__ __launch_bounds__(256) void bw_layer_norm_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                            const float* __restrict__ dy, const uint8_t* __restrict__ zero_rows,
                                                            float eps, int rows, int d, float* __restrict__ dx,
                                                            float* __restrict__ prod, float* __restrict__ dyc) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const size_t o = (size_t)row * d;
    if (zero_rows && zero_rows[row]) {
        for (int c = lane; c < d; c += 64) { dx[o + c] = 0.f; prod[o + c] = 0.f; dyc[o + c] = 0.f; }
        return;
    }
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
}

// bw_layer_norm_kernel plus the masked copy of dx (the gradient of the pre-norm sum x) for a dropout site on the projection inside x.
// The body's loops are bw_layer_norm_kernel's, statement for statement, and dproj is formed from the stored dx in a loop of its own:
// dx, prod and dyc then have the plain kernel's bits at every width (tests/test_backward_gpu.py holds all three instances to that)
__global__ __launch_bounds__(256) void bw_layer_norm_dropout_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                                    const float* __restrict__ dy, const uint8_t* __restrict__ zero_rows,
                                                                    float eps, int rows, int d, float* __restrict__ dx,
                                                                    float* __restrict__ prod, float* __restrict__ dyc,
                                                                    float* __restrict__ dproj, DropoutSite drop) {
#define OVC_BW_MASK_ROW row
#include "bodies/bw_layer_norm_dropout.inc"
#undef OVC_BW_MASK_ROW
}

// bw_layer_norm_dropout_kernel with the mask row of row r taken from rowmap[r] (ovc_sequence_backward_dropout: the rows of a
// generated sequence are masked as the search masked them, csrc/dropout.h)
__global__ __launch_bounds__(256) void bw_layer_norm_dropout_mapped_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                                    const float* __restrict__ dy, const uint8_t* __restrict__ zero_rows,
                                                                    float eps, int rows, int d, float* __restrict__ dx,
                                                                    float* __restrict__ prod, float* __restrict__ dyc,
                                                                    float* __restrict__ dproj, DropoutSite drop,
                                                                           const int32_t* __restrict__ rowmap) {
#define OVC_BW_MASK_ROW (uint32_t)rowmap[row]
#include "bodies/bw_layer_norm_dropout.inc"
#undef OVC_BW_MASK_ROW
}

__global__ void bw_relu_dropout_kernel(float* __restrict__ g, const float* __restrict__ act, float scale, long n) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        g[i] = act[i] > 0.f ? g[i] * scale : 0.f;
}

// keep[r * cols + c] = the keep decision of (site, r, c): what the kernels above and the dropout GEMM instances use
__global__ void dropout_mask_kernel(const int64_t* __restrict__ seed_ptr, uint32_t site, uint32_t thr, long rows, long cols,
                                    uint8_t* __restrict__ keep) {
    const uint64_t seed = (uint64_t)*seed_ptr;
    const uint64_t n = (uint64_t)rows * (uint64_t)cols;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        keep[i] = ovc_dropout_keep(seed, site, i, thr) ? 1 : 0;
}

// keep[i * cols + c] = the keep decision of (site, rowmap[i], c): dropout_mask_kernel over an arbitrary list of mask rows
__global__ void dropout_mask_rows_kernel(const int64_t* __restrict__ seed_ptr, uint32_t site, uint32_t thr, const int32_t* __restrict__ rowmap,
                                         long rows, long cols, uint8_t* __restrict__ keep) {
    const uint64_t seed = (uint64_t)*seed_ptr;
    const uint64_t n = (uint64_t)rows * (uint64_t)cols;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = i / (uint64_t)cols, c = i - r * (uint64_t)cols;
        keep[i] = ovc_dropout_keep(seed, site, (uint64_t)(uint32_t)rowmap[r] * (uint64_t)cols + c, thr) ? 1 : 0;
    }
}

__global__ void bw_relu_kernel(float* __restrict__ g, const float* __restrict__ act, long n) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        if (!(act[i] > 0.f)) g[i] = 0.f;
}

// one wave per (b, head, query row); LDS: q and dout of the row (dk <= 64), scores / dP of the nk keys.  GEO: the encoder's geometry
// bias log(max(g, 1e-6)) + s added to the scaled, masked score in the forward's operation order (attention.hip); the <false>
// instance is the kernel without it, instruction for instruction.
template <bool GEO>
__global__ __launch_bounds__(64) void bw_attention_rows_kernel(AttnBwdArgs a) {
    extern __shared__ float sm[];
    float* qs = sm; float* os = sm + 64; float* s = sm + 128; float* dp = s + a.nk;
    const int lane = threadIdx.x;
    const int i = blockIdx.x % a.nq, bh = blockIdx.x / a.nq, hh = bh % a.h, b = bh / a.h;
    const size_t qrow = (size_t)b * a.nq + i;
    const int dk = a.dk;
    if (lane < dk) { qs[lane] = a.q[qrow * a.ldq + hh * dk + lane]; os[lane] = a.dout[qrow * a.ldo + hh * dk + lane]; }
    __syncthreads();
    const uint8_t* mrow = a.mask ? a.mask + (size_t)b * a.mask_b + (size_t)i * a.mask_r : nullptr;
    const size_t po = (((size_t)b * a.h + hh) * a.nq + i) * a.nk;
    float mx = -INFINITY;
    for (int j = lane; j < a.nk; j += 64) {
        const float* kr = a.k + ((size_t)b * a.nk + j) * a.ldkv + hh * dk;
        const float* vr = a.v + ((size_t)b * a.nk + j) * a.ldkv + hh * dk;
        float sc = 0.f, g = 0.f;
        for (int t = 0; t < dk; ++t) { sc = fmaf(qs[t], kr[t], sc); g = fmaf(os[t], vr[t], g); }
        sc = (mrow && mrow[j]) ? -INFINITY : sc / a.scale;
        if (GEO) sc = logf(fmaxf(a.geometry[po + j], 1e-6f)) + sc;
        s[j] = sc; dp[j] = g;
        mx = fmaxf(mx, sc);
    }
    mx = wave_max(mx);
    float sum = 0.f;
    for (int j = lane; j < a.nk; j += 64) sum += s[j] == -INFINITY ? 0.f : expf(s[j] - mx);
    sum = wave_sum(sum);
    float delta = 0.f;
    for (int j = lane; j < a.nk; j += 64) {
        const float p = (s[j] == -INFINITY || !(sum > 0.f)) ? 0.f : expf(s[j] - mx) / sum;
        s[j] = p;
        delta = fmaf(p, dp[j], delta);
    }
    delta = wave_sum(delta);
    for (int j = lane; j < a.nk; j += 64) {
        const float p = s[j], g = p * (dp[j] - delta);
        dp[j] = g;
        a.P[po + j] = p; a.dS[po + j] = g;
    }
    __syncthreads();
    if (lane < dk) {
        float acc = 0.f;
        for (int j = 0; j < a.nk; ++j) acc = fmaf(dp[j], a.k[((size_t)b * a.nk + j) * a.ldkv + hh * dk + lane], acc);
        a.dq[qrow * a.lddq + hh * dk + lane] = acc / a.scale;
    }
}

// one wave per (b, head, key): lanes over the head's columns, queries in ascending order
__global__ __launch_bounds__(64) void bw_attention_keys_kernel(AttnBwdArgs a) {
    const int lane = threadIdx.x;
    const int j = blockIdx.x % a.nk, bh = blockIdx.x / a.nk, hh = bh % a.h, b = bh / a.h;
    const int dk = a.dk;
    if (lane >= dk) return;
    const size_t po = ((size_t)b * a.h + hh) * a.nq * a.nk + j;
    float gk = 0.f, gv = 0.f;
    for (int i = 0; i < a.nq; ++i) {
        const size_t qrow = (size_t)b * a.nq + i;
        const float ds = a.dS[po + (size_t)i * a.nk], p = a.P[po + (size_t)i * a.nk];
        gk = fmaf(ds, a.q[qrow * a.ldq + hh * dk + lane], gk);
        gv = fmaf(p, a.dout[qrow * a.ldo + hh * dk + lane], gv);
    }
    const size_t krow = (size_t)b * a.nk + j;
    a.dk_out[krow * a.lddkv + hh * dk + lane] = gk / a.scale;
    a.dv_out[krow * a.lddkv + hh * dk + lane] = gv;
}

// bw_attention_rows_kernel with p.m memory slots behind the nk real keys (ovc_bw_attention_mem): slot keys / values are the
// forward's fp32 products mem_scale * m, never masked; LDS: 128 + 2 (nk + m) floats
__global__ __launch_bounds__(64) void bw_attention_rows_mem_kernel(AttnBwdMemArgs p) {
    extern __shared__ float sm[];
    const AttnBwdArgs& a = p.a;
    const int nkt = a.nk + p.m;
    float* qs = sm; float* os = sm + 64; float* s = sm + 128; float* dp = s + nkt;
    const int lane = threadIdx.x;
    const int i = blockIdx.x % a.nq, bh = blockIdx.x / a.nq, hh = bh % a.h, b = bh / a.h;
    const size_t qrow = (size_t)b * a.nq + i;
    const int dk = a.dk, hk = a.h * a.dk;
    if (lane < dk) { qs[lane] = a.q[qrow * a.ldq + hh * dk + lane]; os[lane] = a.dout[qrow * a.ldo + hh * dk + lane]; }
    __syncthreads();
    const uint8_t* mrow = a.mask ? a.mask + (size_t)b * a.mask_b + (size_t)i * a.mask_r : nullptr;
    float mx = -INFINITY;
    for (int j = lane; j < nkt; j += 64) {
        float sc = 0.f, g = 0.f;
        if (j < a.nk) {
            const float* kr = a.k + ((size_t)b * a.nk + j) * a.ldkv + hh * dk;
            const float* vr = a.v + ((size_t)b * a.nk + j) * a.ldkv + hh * dk;
            for (int t = 0; t < dk; ++t) { sc = fmaf(qs[t], kr[t], sc); g = fmaf(os[t], vr[t], g); }
            sc = (mrow && mrow[j]) ? -INFINITY : sc / a.scale;
        } else {
            const float* kr = p.m_k + (size_t)(j - a.nk) * hk + hh * dk;
            const float* vr = p.m_v + (size_t)(j - a.nk) * hk + hh * dk;
            for (int t = 0; t < dk; ++t) {
                const float kx = kr[t] * p.mem_scale_k, vx = vr[t] * p.mem_scale_v;
                sc = fmaf(qs[t], kx, sc); g = fmaf(os[t], vx, g);
            }
            sc = sc / a.scale;
        }
        s[j] = sc; dp[j] = g;
        mx = fmaxf(mx, sc);
    }
    mx = wave_max(mx);
    float sum = 0.f;
    for (int j = lane; j < nkt; j += 64) sum += s[j] == -INFINITY ? 0.f : expf(s[j] - mx);
    sum = wave_sum(sum);
    float delta = 0.f;
    for (int j = lane; j < nkt; j += 64) {
        const float pj = (s[j] == -INFINITY || !(sum > 0.f)) ? 0.f : expf(s[j] - mx) / sum;
        s[j] = pj;
        delta = fmaf(pj, dp[j], delta);
    }
    delta = wave_sum(delta);
    const size_t po = (((size_t)b * a.h + hh) * a.nq + i) * nkt;
    for (int j = lane; j < nkt; j += 64) {
        const float pj = s[j], g = pj * (dp[j] - delta);
        dp[j] = g;
        a.P[po + j] = pj; a.dS[po + j] = g;
    }
    __syncthreads();
    if (lane < dk) {
        float acc = 0.f;
        for (int j = 0; j < a.nk; ++j) acc = fmaf(dp[j], a.k[((size_t)b * a.nk + j) * a.ldkv + hh * dk + lane], acc);
        for (int sl = 0; sl < p.m; ++sl) acc = fmaf(dp[a.nk + sl], p.m_k[(size_t)sl * hk + hh * dk + lane] * p.mem_scale_k, acc);
        a.dq[qrow * a.lddq + hh * dk + lane] = acc / a.scale;
    }
}

// The column sums of one key column `col` of the [nq][nk + m] scratch rows of (image b, head hh), for the lane's column of the head:
// gk = sum_i dS[i][col] q[i], gv = sum_i P[i][col] dout[i], ONE fmaf chain each over the queries in ascending order.  Shared by the
// two kernels below only: bw_attention_keys_kernel keeps its own loop (and with it its instructions).
__device__ __forceinline__ void bw_mem_column_sums(const AttnBwdArgs& a, int m, int b, int hh, int col, int lane, float& gk, float& gv) {
    const int dk = a.dk;
    const size_t ld = (size_t)a.nk + m;
    const size_t po = ((size_t)b * a.h + hh) * a.nq * ld + col;
    gk = 0.f; gv = 0.f;
    for (int i = 0; i < a.nq; ++i) {
        const size_t qrow = (size_t)b * a.nq + i;
        const float ds = a.dS[po + (size_t)i * ld], pj = a.P[po + (size_t)i * ld];
        gk = fmaf(ds, a.q[qrow * a.ldq + hh * dk + lane], gk);
        gv = fmaf(pj, a.dout[qrow * a.ldo + hh * dk + lane], gv);
    }
}

// the keys pass over scratch rows of nk + m entries: one wave per (image, head, real key), the real keys' gradients
__global__ __launch_bounds__(64) void bw_attention_keys_mem_kernel(AttnBwdMemArgs p) {
    const AttnBwdArgs& a = p.a;
    const int lane = threadIdx.x;
    const int j = blockIdx.x % a.nk, bh = blockIdx.x / a.nk, hh = bh % a.h, b = bh / a.h;
    const int dk = a.dk;
    if (lane >= dk) return;
    float gk, gv;
    bw_mem_column_sums(a, p.m, b, hh, j, lane, gk, gv);
    const size_t krow = (size_t)b * a.nk + j;
    a.dk_out[krow * a.lddkv + hh * dk + lane] = gk / a.scale;
    a.dv_out[krow * a.lddkv + hh * dk + lane] = gv;
}

// one wave per (image, head, slot): the image's share of d(m_k) / d(m_v), queries in ascending order, both scales applied here
__global__ __launch_bounds__(64) void bw_attention_slots_kernel(AttnBwdMemArgs p) {
    const AttnBwdArgs& a = p.a;
    const int lane = threadIdx.x;
    const int sl = blockIdx.x % p.m, bh = blockIdx.x / p.m, hh = bh % a.h, b = bh / a.h;
    const int dk = a.dk, hk = a.h * a.dk;
    if (lane >= dk) return;
    float gk, gv;
    bw_mem_column_sums(a, p.m, b, hh, a.nk + sl, lane, gk, gv);
    const size_t o = ((size_t)b * p.m + sl) * hk + hh * dk + lane;
    p.part_k[o] = (gk / a.scale) * p.mem_scale_k;
    p.part_v[o] = gv * p.mem_scale_v;
}

// one workgroup: count of non-pad targets and the summed negative log-likelihood, thread partials over rows t, t + 256, ...
// then a fixed LDS tree; afterwards every row's weight
__global__ __launch_bounds__(256) void bw_loss_kernel(const float* __restrict__ logits_t, long ldt, const float* __restrict__ lse,
                                                      const int32_t* __restrict__ tgt, int pad, int rows, float* __restrict__ w_row,
                                                      float* __restrict__ loss) {
    __shared__ float nll[256], cnt[256];
    const int t = threadIdx.x;
    float a = 0.f, c = 0.f;
    for (int r = t; r < rows; r += 256) {
        const int w = tgt[r];
        if (w == pad) continue;
        a -= (logits_t[(size_t)w * ldt + r] - lse[2 * r]) - lse[2 * r + 1];
        c += 1.f;
    }
    nll[t] = a; cnt[t] = c;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) { nll[t] += nll[t + off]; cnt[t] += cnt[t + off]; }
        __syncthreads();
    }
    const float count = cnt[0];
    if (t == 0) *loss = nll[0] / count;
    const float inv = 1.f / count;
    for (int r = t; r < rows; r += 256) w_row[r] = tgt[r] == pad ? 0.f : inv;
}

// 64 words x 64 rows per workgroup: dlogit written transposed (along rows) and, through LDS, row-major (along words)
__global__ __launch_bounds__(256) void bw_dlogit_kernel(const float* __restrict__ logits_t, long ldt, const float* __restrict__ lse,
                                                        const int32_t* __restrict__ tgt, const float* __restrict__ w_row, int rows,
                                                        int V, float* __restrict__ dl_t, float* __restrict__ dl, long ldv) {
    __shared__ float tile[64][65];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int r0 = blockIdx.x * 64, w0 = blockIdx.y * 64;
    for (int i = wv; i < 64; i += 4) {
        const int w = w0 + i, r = r0 + lane;
        float g = 0.f;
        if (w < V && r < rows) {
            const float p = expf((logits_t[(size_t)w * ldt + r] - lse[2 * r]) - lse[2 * r + 1]);
            g = (p - (tgt[r] == w ? 1.f : 0.f)) * w_row[r];
        }
        if (w < V && r < ldt) dl_t[(size_t)w * ldt + r] = g;
        tile[i][lane] = g;
    }
    __syncthreads();
    for (int i = wv; i < 64; i += 4) {
        const int r = r0 + i, w = w0 + lane;
        if (r < rows && w < ldv) dl[(size_t)r * ldv + w] = tile[lane][i];
    }
}

// Label smoothing.  Row sums of the log-probabilities: lanes along rows (every load coalesced), one wave per (64 rows, slice of
// kLpSlice words), the slice's words in ascending order: part[slice][r] = sum_v ((logit - M) - log S)
constexpr int kLpSlice = 64;

__global__ __launch_bounds__(256) void bw_logp_rowsum_part_kernel(const float* __restrict__ logits_t, long ldt,
                                                                  const float* __restrict__ lse, int rows, int V,
                                                                  float* __restrict__ part) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int r = blockIdx.x * 64 + lane, slice = blockIdx.y * 4 + wv;
    const int w0 = slice * kLpSlice;
    if (r >= rows || w0 >= V) return;
    const float mx = lse[2 * r], ls = lse[2 * r + 1];
    const int w1 = min(w0 + kLpSlice, V);
    float acc = 0.f;
#pragma unroll 8
    for (int w = w0; w < w1; ++w) acc += (logits_t[(size_t)w * ldt + r] - mx) - ls;
    part[(size_t)slice * ldt + r] = acc;
}

// the slices in ascending order
__global__ __launch_bounds__(256) void bw_logp_rowsum_final_kernel(const float* __restrict__ part, long ldt, int rows, int slices,
                                                                   float* __restrict__ lp_sum) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    float acc = 0.f;
    for (int i = 0; i < slices; ++i) acc += part[(size_t)i * ldt + r];
    lp_sum[r] = acc;
}

// bw_loss_kernel for the smoothed loss: one workgroup, thread partials over rows t, t + 256, ... of
// C - conf logp[tgt] - u ((sum_v logp - logp[tgt]) - logp[pad]) and of the kept-row count, the same fixed LDS tree, then every
// row's weight: w_mean (reduction 0) or 1 / count on kept rows, 0 on pad rows
__global__ __launch_bounds__(256) void bw_smoothed_loss_kernel(const float* __restrict__ logits_t, long ldt,
                                                               const float* __restrict__ lse, const float* __restrict__ lp_sum,
                                                               const int32_t* __restrict__ tgt, int pad, int rows, float conf, float u,
                                                               float C, int reduction, float w_mean, float* __restrict__ w_row,
                                                               float* __restrict__ loss) {
    __shared__ float tot[256], cnt[256];
    const int t = threadIdx.x;
    float a = 0.f, c = 0.f;
    for (int r = t; r < rows; r += 256) {
        const int w = tgt[r];
        if (w == pad) continue;
        const float lt = (logits_t[(size_t)w * ldt + r] - lse[2 * r]) - lse[2 * r + 1];
        const float lpad = (logits_t[(size_t)pad * ldt + r] - lse[2 * r]) - lse[2 * r + 1];
        a += (C - conf * lt) - u * ((lp_sum[r] - lt) - lpad);
        c += 1.f;
    }
    tot[t] = a; cnt[t] = c;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) { tot[t] += tot[t + off]; cnt[t] += cnt[t + off]; }
        __syncthreads();
    }
    const float inv = reduction == 0 ? w_mean : 1.f / cnt[0];
    if (t == 0) *loss = reduction == 0 ? tot[0] * w_mean : tot[0] / cnt[0];
    for (int r = t; r < rows; r += 256) w_row[r] = tgt[r] == pad ? 0.f : inv;
}

// bw_dlogit_kernel's tile with the smoothed target distribution: g = (p - t[r, w]) w_row[r], t = conf at the target, 0 at pad, u
// elsewhere; a row of weight 0 gets +0
__global__ __launch_bounds__(256) void bw_smoothed_dlogit_kernel(const float* __restrict__ logits_t, long ldt,
                                                                 const float* __restrict__ lse, const int32_t* __restrict__ tgt,
                                                                 const float* __restrict__ w_row, int pad, float conf, float u,
                                                                 int rows, int V, float* __restrict__ dl_t, float* __restrict__ dl,
                                                                 long ldv) {
    __shared__ float tile[64][65];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int r0 = blockIdx.x * 64, w0 = blockIdx.y * 64;
    for (int i = wv; i < 64; i += 4) {
        const int w = w0 + i, r = r0 + lane;
        float g = 0.f;
        if (w < V && r < rows) {
            const float wr = w_row[r];
            if (wr != 0.f) {
                const float p = expf((logits_t[(size_t)w * ldt + r] - lse[2 * r]) - lse[2 * r + 1]);
                g = (p - (tgt[r] == w ? conf : w == pad ? 0.f : u)) * wr;
            }
        }
        if (w < V && r < ldt) dl_t[(size_t)w * ldt + r] = g;
        tile[i][lane] = g;
    }
    __syncthreads();
    for (int i = wv; i < 64; i += 4) {
        const int r = r0 + i, w = w0 + lane;
        if (r < rows && w < ldv) dl[(size_t)r * ldv + w] = tile[lane][i];
    }
}

// Soft targets (distillation).  The stored logits are transposed (coalesced along rows), the teacher is row-major [rows][V]
// (coalesced along words): each operand is read along its own contiguous axis and the teacher's 64 rows x 64 words tile is turned
// through LDS.  Per (row, slice of kLpSlice words) the partials of
//   kl = sum_v pt > 0 ? pt (lt - lq) : 0        and        mass = sum_v pt,        pt = exp(lt), lq = (logit - M) - log S
// One workgroup per (64 rows, slice): the four waves form the terms (tt: the teacher tile, then pt in place; tk: the kl terms),
// then wave 0 sums the slice's kl terms and wave 1 its pt in ascending words, one lane per row.  Words past V and rows past
// `rows` contribute +0.
__global__ __launch_bounds__(256) void bw_soft_rowsum_part_kernel(const float* __restrict__ logits_t, long ldt,
                                                                  const float* __restrict__ lse, const float* __restrict__ teacher,
                                                                  int rows, int V, float* __restrict__ part_kl,
                                                                  float* __restrict__ part_mass) {
    __shared__ float tt[64][65], tk[64][65];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int r0 = blockIdx.x * 64, slice = blockIdx.y, w0 = slice * kLpSlice;
    // every global load is unconditional at a clamped (always valid) address, so a thread's 16 loads of a phase are in flight
    // together; what lies past the edges is replaced after the load
    float v[16];
    {
        const int wc = min(w0 + lane, V - 1);
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = teacher[(size_t)min(r0 + wv + 4 * j, rows - 1) * V + wc];
#pragma unroll
        for (int j = 0; j < 16; ++j) tt[wv + 4 * j][lane] = (r0 + wv + 4 * j < rows && w0 + lane < V) ? v[j] : -INFINITY;
    }
    __syncthreads();
    const int r = r0 + lane, rc = min(r, rows - 1);
    const float mx = lse[2 * rc], ls = lse[2 * rc + 1];
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = logits_t[(size_t)min(w0 + wv + 4 * j, V - 1) * ldt + rc];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int i = wv + 4 * j;
        float term = 0.f, pt = 0.f;
        if (w0 + i < V && r < rows) {
            const float lt = tt[lane][i];
            pt = expf(lt);
            if (pt > 0.f) term = pt * (lt - ((v[j] - mx) - ls));
        }
        tt[lane][i] = pt;              // read and written by this thread alone
        tk[i][lane] = term;
    }
    __syncthreads();
    if (wv > 1 || r >= rows) return;
    float acc = 0.f;
    if (wv == 0) {
#pragma unroll 8
        for (int i = 0; i < kLpSlice; ++i) acc += tk[i][lane];
        part_kl[(size_t)slice * ldt + r] = acc;
    } else {
#pragma unroll 8
        for (int i = 0; i < kLpSlice; ++i) acc += tt[lane][i];
        part_mass[(size_t)slice * ldt + r] = acc;
    }
}

// the slices in ascending order, both sums
__global__ __launch_bounds__(256) void bw_soft_rowsum_final_kernel(const float* __restrict__ part_kl,
                                                                   const float* __restrict__ part_mass, long ldt, int rows, int slices,
                                                                   float* __restrict__ kl, float* __restrict__ mass) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    float a = 0.f, b = 0.f;
#pragma unroll 8
    for (int i = 0; i < slices; ++i) { a += part_kl[(size_t)i * ldt + r]; b += part_mass[(size_t)i * ldt + r]; }
    kl[r] = a; mass[r] = b;
}

// bw_loss_kernel for the soft-target loss: one workgroup, thread partials over rows t, t + 256, ... of
// (1 - lambda) (-logp[tgt]) + lambda kl_r and of the kept-row count, the same fixed LDS tree, then every row's weight
__global__ __launch_bounds__(256) void bw_soft_loss_kernel(const float* __restrict__ logits_t, long ldt, const float* __restrict__ lse,
                                                           const float* __restrict__ kl, const int32_t* __restrict__ tgt, int pad,
                                                           int rows, float hard, float soft, float* __restrict__ w_row,
                                                           float* __restrict__ loss) {
    __shared__ float tot[256], cnt[256];
    const int t = threadIdx.x;
    float a = 0.f, c = 0.f;
    for (int r = t; r < rows; r += 256) {
        const int w = tgt[r];
        if (w == pad) continue;
        const float nll = -((logits_t[(size_t)w * ldt + r] - lse[2 * r]) - lse[2 * r + 1]);
        a += hard * nll + soft * kl[r];
        c += 1.f;
    }
    tot[t] = a; cnt[t] = c;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) { tot[t] += tot[t + off]; cnt[t] += cnt[t + off]; }
        __syncthreads();
    }
    const float count = cnt[0];
    if (t == 0) *loss = tot[0] / count;
    const float inv = 1.f / count;
    for (int r = t; r < rows; r += 256) w_row[r] = tgt[r] == pad ? 0.f : inv;
}

// bw_dlogit_kernel's tile with the soft-target rule: g = w_row ((1 - lambda) (q - [w == tgt]) + lambda (mass q - pt)); the
// teacher's tile comes in along words and is read along rows through the same LDS array, before g takes it; a row of weight 0 gets +0
__global__ __launch_bounds__(256) void bw_soft_dlogit_kernel(const float* __restrict__ logits_t, long ldt, const float* __restrict__ lse,
                                                             const float* __restrict__ teacher, const float* __restrict__ mass,
                                                             const int32_t* __restrict__ tgt, const float* __restrict__ w_row,
                                                             float hard, float soft, int rows, int V, float* __restrict__ dl_t,
                                                             float* __restrict__ dl, long ldv) {
    __shared__ float tile[64][65];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int r0 = blockIdx.x * 64, w0 = blockIdx.y * 64;
    // the one LDS array holds the teacher's tile first (in along words, out along rows into registers), then g (in along rows, out
    // along words).  Every global load is unconditional at a clamped (always valid) address, so a thread's 16 loads of a phase
    // are in flight together; what lies past the edges is never used.
    float lt[16], x[16];
    {
        const int wc = min(w0 + lane, V - 1);
#pragma unroll
        for (int j = 0; j < 16; ++j) lt[j] = teacher[(size_t)min(r0 + wv + 4 * j, rows - 1) * V + wc];
#pragma unroll
        for (int j = 0; j < 16; ++j) tile[wv + 4 * j][lane] = lt[j];
    }
    __syncthreads();
    const int r = r0 + lane, rc = min(r, rows - 1);
#pragma unroll
    for (int j = 0; j < 16; ++j) lt[j] = tile[lane][wv + 4 * j];
#pragma unroll
    for (int j = 0; j < 16; ++j) x[j] = logits_t[(size_t)min(w0 + wv + 4 * j, V - 1) * ldt + rc];
    const float mx = lse[2 * rc], ls = lse[2 * rc + 1], wr = r < rows ? w_row[rc] : 0.f, ms = mass[rc];
    const int tg = tgt[rc];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int i = wv + 4 * j, w = w0 + i;
        float g = 0.f;
        if (w < V && wr != 0.f) {
            const float q = expf((x[j] - mx) - ls);
            const float pt = expf(lt[j]);
            g = (hard * (q - (tg == w ? 1.f : 0.f)) + soft * (ms * q - pt)) * wr;
        }
        if (w < V && r < ldt) dl_t[(size_t)w * ldt + r] = g;
        tile[i][lane] = g;
    }
    __syncthreads();
    for (int i = wv; i < 64; i += 4) {
        const int r = r0 + i, w = w0 + lane;
        if (r < rows && w < ldv) dl[(size_t)r * ldv + w] = tile[lane][i];
    }
}

// one workgroup per word; each thread keeps up to 8 columns (d <= 2048)
__global__ __launch_bounds__(256) void bw_embedding_kernel(const int32_t* __restrict__ tok, int rows, int pad,
                                                           const float* __restrict__ dx, int d, float* __restrict__ out) {
    const int w = blockIdx.x, t = threadIdx.x;
    float acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = 0.f;
    if (w != pad) {
        for (int r = 0; r < rows; ++r) {
            if (tok[r] != w) continue;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int c = t + 256 * k;
                if (c < d) acc[k] += dx[(size_t)r * d + c];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int c = t + 256 * k;
        if (c < d) out[(size_t)w * d + c] = acc[k];
    }
}

__global__ void bw_tokens_kernel(const int64_t* __restrict__ tokens, int rows, int V, int32_t* __restrict__ tok32) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < rows) tok32[r] = (int)min(max(tokens[r], (int64_t)0), (int64_t)V - 1);
}

__global__ void scale_kernel(const float* __restrict__ x, const float* __restrict__ s, float* __restrict__ y, long n) {
    const float f = *s;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) y[i] = x[i] * f;
}

unsigned blocks_for(long n, int per = 256) { return (unsigned)std::min<long>((n + per - 1) / per, 4096); }

}  // namespace

int ovc_bw_transpose(const float* src, long lds, int rows, int cols, float* dst, long ldd, int rows_pad, hipStream_t s) {
    if (rows_pad < rows || ldd < rows_pad || cols <= 0 || rows_pad <= 0) return OVC_EINVAL;
    hipLaunchKernelGGL(bw_transpose_kernel, dim3((rows_pad + 63) / 64, (cols + 63) / 64), dim3(256), 0, s, src, lds, rows, cols, dst,
                       ldd, rows_pad);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

int ovc_bw_rowsum(const float* src, long ld, int rows, int n, float* dst, hipStream_t s) {
    hipLaunchKernelGGL(bw_rowsum_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, src, ld, rows, n, dst);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

int ovc_bw_colsum(const float* src, long ld, int rows, int cols, float* part, float* dst, hipStream_t s) {
    const int chunks = (rows + kChunk - 1) / kChunk;
    hipLaunchKernelGGL(bw_colsum_part_kernel, dim3((cols + 255) / 256, chunks), dim3(256), 0, s, src, ld, rows, cols, part);
    OVC_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(bw_colsum_final_kernel, dim3((cols + 255) / 256), dim3(256), 0, s, part, chunks, cols, dst);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

int ovc_bw_layer_norm(const float* x, const float* gamma, const float* dy, const uint8_t* zero_rows, float eps, int rows, int d,
                      float* dx, float* prod, float* dyc, hipStream_t s) {
    if (d > 2048) return OVC_EINVAL;
    hipLaunchKernelGGL(bw_layer_norm_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, x, gamma, dy, zero_rows, eps, rows, d, dx, prod, dyc);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

int ovc_bw_relu(float* g, const float* act, long n, hipStream_t s) {
    hipLaunchKernelGGL(bw_relu_kernel, dim3(blocks_for(n)), dim3(256), 0, s, g, act, n);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

int ovc_bw_layer_norm_dropout(const float* x, const float* gamma, const float* dy, const uint8_t* zero_rows, float eps, int rows, int d,
                              float* dx, float* prod, float* dyc, float* dproj, const DropoutSite& drop, hipStream_t s) {
    if (d > 2048 || !drop.seed || drop.cols != d) return OVC_EINVAL;
    hipLaunchKernelGGL(bw_layer_norm_dropout_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, x, gamma, dy, zero_rows, eps, rows, d, dx,
                       prod, dyc, dproj, drop);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

int ovc_bw_layer_norm_dropout_mapped(const float* x, const float* gamma, const float* dy, const uint8_t* zero_rows, float eps, int rows,
                                     int d, float* dx, float* prod, float* dyc, float* dproj, const DropoutSite& drop,
                                     const int32_t* rowmap, hipStream_t s) {
    if (d > 2048 || !drop.seed || drop.cols != d || !rowmap) return OVC_EINVAL;
    hipLaunchKernelGGL(bw_layer_norm_dropout_mapped_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, x, gamma, dy, zero_rows, eps, rows, d,
                       dx, prod, dyc, dproj, drop, rowmap);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

int ovc_bw_relu_dropout(float* g, const float* act, float scale, long n, hipStream_t s) {
    hipLaunchKernelGGL(bw_relu_dropout_kernel, dim3(blocks_for(n)), dim3(256), 0, s, g, act, scale, n);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

int ovc_bw_attention(const AttnBwdArgs& a, hipStream_t s) {
    if (a.dk > 64 || a.dk <= 0 || a.nk <= 0 || a.nq <= 0) return OVC_EINVAL;
    const size_t lds = (128 + 2 * (size_t)a.nk) * sizeof(float);
    if (a.geometry) hipLaunchKernelGGL(bw_attention_rows_kernel<true>, dim3(a.B * a.h * a.nq), dim3(64), lds, s, a);
    else hipLaunchKernelGGL(bw_attention_rows_kernel<false>, dim3(a.B * a.h * a.nq), dim3(64), lds, s, a);
    OVC_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(bw_attention_keys_kernel, dim3(a.B * a.h * a.nk), dim3(64), 0, s, a);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

int ovc_bw_attention_mem(const AttnBwdMemArgs& p, hipStream_t s) {
    const AttnBwdArgs& a = p.a;
    if (a.dk > 64 || a.dk <= 0 || a.nk <= 0 || a.nq <= 0 || a.B <= 0 || p.m <= 0) return OVC_EINVAL;
    if (!p.m_k || !p.m_v || !p.part_k || !p.part_v || !p.colpart || !p.d_mk || !p.d_mv) return OVC_EINVAL;
    const size_t lds = (128 + 2 * ((size_t)a.nk + p.m)) * sizeof(float);
    if (lds > 64 * 1024) return OVC_EINVAL;
    hipLaunchKernelGGL(bw_attention_rows_mem_kernel, dim3(a.B * a.h * a.nq), dim3(64), lds, s, p);
    OVC_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(bw_attention_keys_mem_kernel, dim3(a.B * a.h * a.nk), dim3(64), 0, s, p);
    OVC_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(bw_attention_slots_kernel, dim3(a.B * a.h * p.m), dim3(64), 0, s, p);
    OVC_RETURN_IF_LAUNCH_FAILED();
    const int cols = p.m * a.h * a.dk;
    if (const int rc = ovc_bw_colsum(p.part_k, cols, a.B, cols, p.colpart, p.d_mk, s)) return rc;
    return ovc_bw_colsum(p.part_v, cols, a.B, cols, p.colpart, p.d_mv, s);
}

int ovc_bw_xent(const float* logits_t, long ldt, const float* lse, const int32_t* tgt, int pad, int rows, int V, float* w_row,
                float* loss, float* dl_t, float* dl, long ldv, hipStream_t s) {
    hipLaunchKernelGGL(bw_loss_kernel, dim3(1), dim3(256), 0, s, logits_t, ldt, lse, tgt, pad, rows, w_row, loss);
    OVC_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(bw_dlogit_kernel, dim3((ldt + 63) / 64, (ldv + 63) / 64), dim3(256), 0, s, logits_t, ldt, lse, tgt, w_row,
                       rows, V, dl_t, dl, ldv);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

int ovc_bw_dlogit(const float* logits_t, long ldt, const float* lse, const int32_t* tgt, const float* w_row, int rows, int V,
                  float* dl_t, float* dl, long ldv, hipStream_t s) {
    hipLaunchKernelGGL(bw_dlogit_kernel, dim3((ldt + 63) / 64, (ldv + 63) / 64), dim3(256), 0, s, logits_t, ldt, lse, tgt, w_row,
                       rows, V, dl_t, dl, ldv);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

size_t ovc_bw_smoothed_part_floats(int rows, int V) {
    return (size_t)((V + kLpSlice - 1) / kLpSlice) * (((size_t)rows + 3) & ~(size_t)3);
}

int ovc_bw_xent_smoothed(const float* logits_t, long ldt, const float* lse, const int32_t* tgt, int pad, int rows, int V,
                         const SmoothedLoss& l, float* lp_part, float* lp_sum, float* w_row, float* loss, float* dl_t, float* dl,
                         long ldv, hipStream_t s) {
    if (rows <= 0 || V <= 0 || pad < 0 || pad >= V || ldt < rows || ldt > (((long)rows + 3) & ~3L) || !lp_part || !lp_sum ||
        (l.reduction != 0 && l.reduction != 1))
        return OVC_EINVAL;           // lp_part's rows are ldt apart: ovc_bw_smoothed_part_floats sizes them for rows padded to 4
    const int slices = (V + kLpSlice - 1) / kLpSlice;
    hipLaunchKernelGGL(bw_logp_rowsum_part_kernel, dim3((rows + 63) / 64, (slices + 3) / 4), dim3(256), 0, s, logits_t, ldt, lse, rows,
                       V, lp_part);
    OVC_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(bw_logp_rowsum_final_kernel, dim3((rows + 255) / 256), dim3(256), 0, s, lp_part, ldt, rows, slices, lp_sum);
    OVC_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(bw_smoothed_loss_kernel, dim3(1), dim3(256), 0, s, logits_t, ldt, lse, lp_sum, tgt, pad, rows, l.conf, l.u, l.C,
                       l.reduction, l.w_mean, w_row, loss);
    OVC_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(bw_smoothed_dlogit_kernel, dim3((ldt + 63) / 64, (ldv + 63) / 64), dim3(256), 0, s, logits_t, ldt, lse, tgt,
                       w_row, pad, l.conf, l.u, rows, V, dl_t, dl, ldv);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

int ovc_bw_xent_soft(const float* logits_t, long ldt, const float* lse, const int32_t* tgt, int pad, int rows, int V, const SoftLoss& l,
                     const float* teacher, float* part, float* kl, float* mass, float* w_row, float* loss, float* dl_t, float* dl,
                     long ldv, hipStream_t s) {
    if (rows <= 0 || V <= 0 || pad < 0 || pad >= V || ldt < rows || ldt > (((long)rows + 3) & ~3L) || !teacher || !part || !kl || !mass)
        return OVC_EINVAL;           // the partials' rows are ldt apart: ovc_bw_smoothed_part_floats sizes them for rows padded to 4
    const int slices = (V + kLpSlice - 1) / kLpSlice;
    float* part_mass = part + ovc_bw_smoothed_part_floats(rows, V);
    hipLaunchKernelGGL(bw_soft_rowsum_part_kernel, dim3((rows + 63) / 64, slices), dim3(256), 0, s, logits_t, ldt, lse, teacher, rows,
                       V, part, part_mass);
    OVC_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(bw_soft_rowsum_final_kernel, dim3((rows + 255) / 256), dim3(256), 0, s, part, part_mass, ldt, rows, slices, kl,
                       mass);
    OVC_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(bw_soft_loss_kernel, dim3(1), dim3(256), 0, s, logits_t, ldt, lse, kl, tgt, pad, rows, l.hard, l.soft, w_row,
                       loss);
    OVC_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(bw_soft_dlogit_kernel, dim3((ldt + 63) / 64, (ldv + 63) / 64), dim3(256), 0, s, logits_t, ldt, lse, teacher,
                       mass, tgt, w_row, l.hard, l.soft, rows, V, dl_t, dl, ldv);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

int ovc_bw_embedding(const int32_t* tok, int rows, int pad, const float* dx, int d, int V, float* out, hipStream_t s) {
    if (d > 2048) return OVC_EINVAL;
    hipLaunchKernelGGL(bw_embedding_kernel, dim3(V), dim3(256), 0, s, tok, rows, pad, dx, d, out);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

int ovc_bw_tokens(const int64_t* tokens, int rows, int V, int32_t* tok32, hipStream_t s) {
    hipLaunchKernelGGL(bw_tokens_kernel, dim3((rows + 255) / 256), dim3(256), 0, s, tokens, rows, V, tok32);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

// Test hook (include/ovc.h): ovc_bw_attention_mem on caller-supplied buffers.
extern "C" int ovc_debug_attention_mem_backward(const float* q, const float* k, const float* v, const float* dout, const uint8_t* mask,
                                                const float* m_k, const float* m_v, int B, int n, int h, int dk, int m, float* P,
                                                float* dS, float* dq, float* dk_out, float* dv_out, float* part_k, float* part_v,
                                                float* colpart, float* d_mk, float* d_mv, ovc_stream stream) {
    if (!q || !k || !v || !dout || !P || !dS || !dq || !dk_out || !dv_out || B <= 0 || n <= 0 || h <= 0 || m <= 0) return OVC_EINVAL;
    if (const int rc = ovc_device_guard()) return rc;
    const int hk = h * dk;
    AttnBwdMemArgs p{};
    p.a.q = q; p.a.ldq = hk; p.a.k = k; p.a.v = v; p.a.ldkv = hk; p.a.dout = dout; p.a.ldo = hk;
    p.a.mask = mask; p.a.mask_b = n; p.a.mask_r = 0;
    p.a.B = B; p.a.nq = n; p.a.nk = n; p.a.h = h; p.a.dk = dk; p.a.scale = sqrtf((float)dk);
    p.a.P = P; p.a.dS = dS; p.a.dq = dq; p.a.lddq = hk; p.a.dk_out = dk_out; p.a.dv_out = dv_out; p.a.lddkv = hk;
    p.m_k = m_k; p.m_v = m_v; p.m = m; p.mem_scale_k = sqrtf((float)dk); p.mem_scale_v = sqrtf((float)m);
    p.part_k = part_k; p.part_v = part_v; p.colpart = colpart; p.d_mk = d_mk; p.d_mv = d_mv;
    return ovc_bw_attention_mem(p, ovc_hip_stream(stream));
}

extern "C" int ovc_scale(const float* x, const float* scale, float* y, long n, ovc_stream stream) {
    if (!x || !scale || !y || n < 0) return OVC_EINVAL;
    if (n == 0) return OVC_OK;
    if (const int rc = ovc_device_guard()) return rc;
    hipLaunchKernelGGL(scale_kernel, dim3(blocks_for(n)), dim3(256), 0, ovc_hip_stream(stream), x, scale, y, n);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

extern "C" int ovc_dropout_mask(const int64_t* seed, int site, long rows, long cols, float p, uint8_t* keep, ovc_stream stream) {
    if (!seed || !keep || site < 0 || site >= OVC_DROPOUT_SITES || rows < 0 || cols < 0 || !(p >= 0.f && p < 1.f)) return OVC_EINVAL;
    if (rows == 0 || cols == 0) return OVC_OK;
    if (const int rc = ovc_device_guard()) return rc;
    const uint64_t n = (uint64_t)rows * (uint64_t)cols;
    const unsigned blocks = (unsigned)std::min<uint64_t>((n + 255) / 256, 8192);
    hipLaunchKernelGGL(dropout_mask_kernel, dim3(blocks), dim3(256), 0, ovc_hip_stream(stream), seed, (uint32_t)site,
                       ovc_dropout_threshold(p), rows, cols, keep);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

extern "C" int ovc_dropout_mask_rows(const int64_t* seed, int site, const int32_t* mask_rows, long rows, long cols, float p, uint8_t* keep,
                                     ovc_stream stream) {
    if (!seed || !keep || !mask_rows || site < 0 || site >= OVC_DROPOUT_SITES || rows < 0 || cols < 0 || !(p >= 0.f && p < 1.f))
        return OVC_EINVAL;
    if (rows == 0 || cols == 0) return OVC_OK;
    if (const int rc = ovc_device_guard()) return rc;
    const uint64_t n = (uint64_t)rows * (uint64_t)cols;
    const unsigned blocks = (unsigned)std::min<uint64_t>((n + 255) / 256, 8192);
    hipLaunchKernelGGL(dropout_mask_rows_kernel, dim3(blocks), dim3(256), 0, ovc_hip_stream(stream), seed, (uint32_t)site,
                       ovc_dropout_threshold(p), mask_rows, rows, cols, keep);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

// ---- the cross-level (CaMo) encoder's tail (engine.hip, bw_cross_level_tail) ----------------------------------------------------
namespace {

// bw_layer_norm_kernel for y = alpha * LN(x + r) + r (the tail's AddNorm, rowops.hip kPostTenths): the pre-norm sum is formed here as
// the forward formed it (x + r, one fp32 add), dx = the gradient of that sum through the norm only (the identity into r is the
// caller's), prod / dyc take the alpha factor (gamma's and beta's gradients)
__global__ __launch_bounds__(256) void bw_layer_norm_post_kernel(const float* __restrict__ x, const float* __restrict__ r,
                                                                 const float* __restrict__ gamma, const float* __restrict__ dy,
                                                                 float alpha, float eps, int rows, int d, float* __restrict__ dx,
                                                                 float* __restrict__ prod, float* __restrict__ dyc) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const size_t o = (size_t)row * d;
    float s = 0.f;
    for (int c = lane; c < d; c += 64) s += x[o + c] + r[o + c];
    const float mean = wave_sum(s) / d;
    float v = 0.f;
    for (int c = lane; c < d; c += 64) { const float t = (x[o + c] + r[o + c]) - mean; v += t * t; }
    const float rstd = 1.f / sqrtf(wave_sum(v) / d + eps);
    float a = 0.f, b = 0.f;
    for (int c = lane; c < d; c += 64) {
        const float xh = ((x[o + c] + r[o + c]) - mean) * rstd, g = gamma[c] * (alpha * dy[o + c]);
        a += g; b += g * xh;
    }
    a = wave_sum(a) / d; b = wave_sum(b) / d;
    for (int c = lane; c < d; c += 64) {
        const float xh = ((x[o + c] + r[o + c]) - mean) * rstd, g = alpha * dy[o + c];
        dx[o + c] = rstd * (gamma[c] * g - a - xh * b);
        prod[o + c] = g * xh;
        dyc[o + c] = g;
    }
}

// no __restrict__ here or in bw_sum_kernel: the output may be an input
__global__ void bw_leaky_kernel(const float* g, const float* act, float scale, float slope, float* out, long n) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        out[i] = (g[i] * scale) * (act[i] > 0.f ? 1.f : slope);
}

__global__ void bw_sum_kernel(const float* a, long lda, const float* b, long ldb, const float* c, long ldc, int rows, int cols, float* y,
                              long ldy) {
    const long n = (long)rows * cols;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long r = i / cols, k = i - r * cols;
        float s = a[r * lda + k] + b[r * ldb + k];
        if (c) s += c[r * ldc + k];
        y[r * ldy + k] = s;
    }
}

}  // namespace

int ovc_bw_layer_norm_post(const float* x, const float* r, const float* gamma, const float* dy, float alpha, float eps, int rows, int d,
                           float* dx, float* prod, float* dyc, hipStream_t s) {
    if (d > 2048 || rows <= 0) return OVC_EINVAL;
    hipLaunchKernelGGL(bw_layer_norm_post_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, x, r, gamma, dy, alpha, eps, rows, d, dx, prod,
                       dyc);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

int ovc_bw_leaky(const float* g, const float* act, float scale, float slope, float* out, long n, hipStream_t s) {
    hipLaunchKernelGGL(bw_leaky_kernel, dim3(blocks_for(n)), dim3(256), 0, s, g, act, scale, slope, out, n);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

int ovc_bw_sum(const float* a, long lda, const float* b, long ldb, const float* c, long ldc, int rows, int cols, float* y, long ldy,
               hipStream_t s) {
    if (!a || !b || !y || rows <= 0 || cols <= 0) return OVC_EINVAL;
    hipLaunchKernelGGL(bw_sum_kernel, dim3(blocks_for((long)rows * cols)), dim3(256), 0, s, a, lda, b, ldb, c, ldc, rows, cols, y, ldy);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

// ---- the meshed decoder's gate block (engine.hip, bw_meshed_decoder_layer) -------------------------------------------------------
namespace {

// mixed = (sum_l sigmoid(a_l) e_l) / divisor (rowops.hip, meshed_mix): per element and level
//   d(e_l) = (d(mixed) sigmoid(a_l)) / divisor,   d(a_l) = ((d(mixed) e_l) sigmoid'(a_l)) / divisor.
// With t = exp(-|a|) in (0, 1]: sigmoid(a) = 1 / (1 + t) or t / (1 + t) by the sign of a, and sigmoid'(a) = t / (1 + t)^2 <= 1 / 4 -- no
// overflow for any finite a, and no cancellation in 1 - sigmoid for large a.  One lane per four elements: d(mixed) is read once,
// every level's two outputs are written with 16-byte stores by that lane alone.
template <int LEVELS>
__global__ __launch_bounds__(256) void bw_meshed_mix_kernel(const float* __restrict__ dmixed, const float* __restrict__ alpha,
                                                            const float* __restrict__ enc, long n4, float divisor,
                                                            float* __restrict__ denc, float* __restrict__ dalpha) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const f32x4 dm = reinterpret_cast<const f32x4*>(dmixed)[i];
#pragma unroll
        for (int l = 0; l < LEVELS; ++l) {
            const f32x4 al = reinterpret_cast<const f32x4*>(alpha)[(size_t)l * n4 + i];
            const f32x4 ev = reinterpret_cast<const f32x4*>(enc)[(size_t)l * n4 + i];
            f32x4 de, da;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float t = expf(-fabsf(al[j])), r = 1.f / (1.f + t);
                const float sig = al[j] >= 0.f ? r : t * r;
                de[j] = (dm[j] * sig) / divisor;
                da[j] = ((dm[j] * ev[j]) * ((t * r) * r)) / divisor;
            }
            reinterpret_cast<f32x4*>(denc)[(size_t)l * n4 + i] = de;
            reinterpret_cast<f32x4*>(dalpha)[(size_t)l * n4 + i] = da;
        }
    }
}

// out[i] = ((acc[i] + src[i]) + src[stride + i]) + ... over `levels` blocks in ascending order (acc may be nullptr: the sum starts
// from block 0); out may be acc
__global__ void bw_sum_levels_kernel(const float* acc, const float* src, int levels, long stride, long n, float* out) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        float s = acc ? acc[i] + src[i] : src[i];
        for (int l = 1; l < levels; ++l) s += src[l * stride + i];
        out[i] = s;
    }
}

}  // namespace

int ovc_bw_meshed_mix(const float* dmixed, const float* alpha, const float* enc, int levels, long n, float divisor, float* denc,
                      float* dalpha, hipStream_t s) {
    if (!dmixed || !alpha || !enc || !denc || !dalpha || levels < 1 || levels > OVC_MAX_LEVELS || n <= 0 || (n & 3)) return OVC_EINVAL;
    if (!ovc_aligned16(dmixed) || !ovc_aligned16(alpha) || !ovc_aligned16(enc) || !ovc_aligned16(denc) || !ovc_aligned16(dalpha))
        return OVC_EINVAL;                                                                             // float4 accesses
    const dim3 grid(blocks_for(n / 4)), block(256);
    switch (levels) {
    case 1: hipLaunchKernelGGL(bw_meshed_mix_kernel<1>, grid, block, 0, s, dmixed, alpha, enc, n / 4, divisor, denc, dalpha); break;
    case 2: hipLaunchKernelGGL(bw_meshed_mix_kernel<2>, grid, block, 0, s, dmixed, alpha, enc, n / 4, divisor, denc, dalpha); break;
    case 3: hipLaunchKernelGGL(bw_meshed_mix_kernel<3>, grid, block, 0, s, dmixed, alpha, enc, n / 4, divisor, denc, dalpha); break;
    default: hipLaunchKernelGGL(bw_meshed_mix_kernel<4>, grid, block, 0, s, dmixed, alpha, enc, n / 4, divisor, denc, dalpha); break;
    }
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

int ovc_bw_sum_levels(const float* acc, const float* src, int levels, long stride, long n, float* out, hipStream_t s) {
    if (!src || !out || levels < 1 || levels > OVC_MAX_LEVELS || n <= 0 || stride < n) return OVC_EINVAL;
    hipLaunchKernelGGL(bw_sum_levels_kernel, dim3(blocks_for(n)), dim3(256), 0, s, acc, src, levels, stride, n, out);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

// ---- the attention-on-attention gate (engine.hip, bw_aoa_gate) --------------------------------------------
namespace {

// out = i * sigmoid(a) (rowops.hip, sigmoid_gate): per element d(i) = d(out) sigmoid(a) and d(a) = (d(out) i) sigmoid'(a), with
// t = exp(-|a|) as in bw_meshed_mix_kernel -- finite for every finite a, and sigmoid'(a) = t / (1 + t)^2 underflows to 0 for large
// |a| without passing through 1 - sigmoid.  One lane per four elements of a row (d % 4 == 0, so four elements never straddle two
// rows): three 16-byte loads, and the two 16-byte stores land d(i) at columns [0, d) and d(a) at columns [d, 2d) of the row of the
// [rows][2d] block, the left operand of the one K = 2d product against the staged [W_i ; W_g].
__global__ __launch_bounds__(256) void bw_aoa_gate_kernel(const float* __restrict__ dout, const float* __restrict__ info,
                                                          const float* __restrict__ gate, long n4, int d4,
                                                          float* __restrict__ dcat) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const f32x4 g = reinterpret_cast<const f32x4*>(dout)[i];
        const f32x4 iv = reinterpret_cast<const f32x4*>(info)[i];
        const f32x4 av = reinterpret_cast<const f32x4*>(gate)[i];
        f32x4 di, da;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float t = expf(-fabsf(av[j])), r = 1.f / (1.f + t);
            const float sig = av[j] >= 0.f ? r : t * r;
            di[j] = g[j] * sig;
            da[j] = (g[j] * iv[j]) * ((t * r) * r);
        }
        const long row = i / d4, at = row * 2 * d4 + (i - row * d4);
        reinterpret_cast<f32x4*>(dcat)[at] = di;
        reinterpret_cast<f32x4*>(dcat)[at + d4] = da;
    }
}

}  // namespace

int ovc_bw_aoa_gate(const float* dout, const float* info, const float* gate, long n, int d, float* dcat, hipStream_t s) {
    if (!dout || !info || !gate || !dcat || n <= 0 || (n & 3) || d <= 0 || (d & 3) || n % d != 0) return OVC_EINVAL;
    if (!ovc_aligned16(dout) || !ovc_aligned16(info) || !ovc_aligned16(gate) || !ovc_aligned16(dcat)) return OVC_EINVAL;   // float4 accesses
    hipLaunchKernelGGL(bw_aoa_gate_kernel, dim3(blocks_for(n / 4)), dim3(256), 0, s, dout, info, gate, n / 4, d / 4, dcat);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

// ---- the geometric (object-relation) encoder's bias (engine.hip, issue_train_body) ------------------------
namespace {

constexpr int kBoxTile = 64;           // keys staged per round
constexpr int kBoxThreads = 256;
constexpr int kBoxOuts = 5;            // outputs per thread: ceil(16 (64 + 1) / 256)

// no __restrict__: element-wise, acc is read and written by the same lane
__global__ void bw_accumulate4_kernel(float* acc, const float* src, long n4) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const f32x4 a = reinterpret_cast<const f32x4*>(acc)[i], b = reinterpret_cast<const f32x4*>(src)[i];
        reinterpret_cast<f32x4*>(acc)[i] = a + b;
    }
}
__global__ void bw_accumulate_kernel(float* acc, const float* src, long n) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) acc[i] = acc[i] + src[i];
}

// One workgroup per (image b, query region i).  Per round of 64 keys: the keys' four log-ratios, then the embedding emb [64][d_g]
// (every sin / cos once) and d(a) [h][64] = w >= 1e-6 ? dG / w : 0 go to LDS; output o = (head, c) -- c == d_g: the bias -- is owned
// by thread o % 256 and continues ONE fmaf chain over the keys in ascending order across the rounds.  part [B*N][h (d_g + 1)].
// LDS: (64 d_g + 64 h + 256) floats <= 21 KB.
__global__ __launch_bounds__(kBoxThreads) void bw_box_relation_kernel(const float* __restrict__ boxes, const float* __restrict__ w,
                                                                      const float* __restrict__ dG, int n, int h, int d_g, int trig,
                                                                      float* __restrict__ part) {
    extern __shared__ float sm[];
    float* emb = sm;                              // [64][d_g]
    float* da = emb + kBoxTile * d_g;             // [h][64]
    float* logs = da + h * kBoxTile;              // [64][4]
    const int tid = threadIdx.x;
    const int b = blockIdx.x / n, i = blockIdx.x - b * n;
    const BoxGeom gi = box_geom(boxes + ((size_t)b * n + i) * 4);
    const int per = d_g + 1, nout = h * per;
    int ohd[kBoxOuts], oc[kBoxOuts];
    float acc[kBoxOuts];
#pragma unroll
    for (int r = 0; r < kBoxOuts; ++r) {
        const int o = tid + kBoxThreads * r;
        ohd[r] = o / per; oc[r] = o - ohd[r] * per; acc[r] = 0.f;
    }
    for (int j0 = 0; j0 < n; j0 += kBoxTile) {
        const int nt = min(kBoxTile, n - j0);
        if (tid < nt) {
            float g[4];
            box_relation_logs(gi, box_geom(boxes + ((size_t)b * n + j0 + tid) * 4), g);
            float* dst = trig ? logs + tid * 4 : emb + tid * 4;       // without the trigonometric embedding emb is the log-ratios
            dst[0] = g[0]; dst[1] = g[1]; dst[2] = g[2]; dst[3] = g[3];
        }
        for (int e = tid; e < h * kBoxTile; e += kBoxThreads) {
            const int hd = e / kBoxTile, jj = e - hd * kBoxTile;
            float v = 0.f;
            if (jj < nt) {
                const size_t o = (((size_t)b * h + hd) * n + i) * n + j0 + jj;
                const float wv = w[o];
                v = wv >= 1e-6f ? dG[o] / wv : 0.f;
            }
            da[e] = v;
        }
        if (trig) {
            __syncthreads();
            const int nf = d_g / 8, half = d_g / 2;
            for (int e = tid; e < nt * half; e += kBoxThreads) {
                const int jj = e / half, cq = e - jj * half, c = cq / nf, q = cq - c * nf;
                const float ang = box_relation_angle(logs[jj * 4 + c], q, nf);
                emb[jj * d_g + cq] = sinf(ang);
                emb[jj * d_g + half + cq] = cosf(ang);
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < kBoxOuts; ++r) {
            if (tid + kBoxThreads * r >= nout) continue;
            const float* dr = da + ohd[r] * kBoxTile;
            float s = acc[r];
            if (oc[r] < d_g) {
                const float* er = emb + oc[r];
                for (int jj = 0; jj < nt; ++jj) s = fmaf(dr[jj], er[jj * d_g], s);
            } else {
                for (int jj = 0; jj < nt; ++jj) s += dr[jj];
            }
            acc[r] = s;
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < kBoxOuts; ++r) {
        const int o = tid + kBoxThreads * r;
        if (o < nout) part[(size_t)blockIdx.x * nout + o] = acc[r];
    }
}

// sum [h][d_g + 1] -> dfc_w [h][d_g] and dfc_b [h][kBoxBiasStride]: element 0 of a group is the gradient, the padding behind it 0 (a
// gradient arena is compared and summed as a whole: its padding must not depend on what the allocator left there)
__global__ void bw_box_relation_write_kernel(const float* __restrict__ sum, int h, int d_g, float* __restrict__ dfc_w,
                                             float* __restrict__ dfc_b) {
    const int o = blockIdx.x * blockDim.x + threadIdx.x, per = d_g + 1;
    if (o >= h * per) return;
    const int hd = o / per, c = o - hd * per;
    if (c < d_g) dfc_w[hd * d_g + c] = sum[o];
    else
        for (int p = 0; p < kBoxBiasStride; ++p) dfc_b[hd * kBoxBiasStride + p] = p == 0 ? sum[o] : 0.f;
}

inline size_t box_pad4(size_t n) { return (n + 3) & ~(size_t)3; }

}  // namespace

int ovc_bw_accumulate(float* acc, const float* src, long n, hipStream_t s) {
    if (!acc || !src || n <= 0) return OVC_EINVAL;
    if (n % 4 == 0 && ovc_aligned16(acc) && ovc_aligned16(src))
        hipLaunchKernelGGL(bw_accumulate4_kernel, dim3(blocks_for(n / 4)), dim3(256), 0, s, acc, src, n / 4);
    else
        hipLaunchKernelGGL(bw_accumulate_kernel, dim3(blocks_for(n)), dim3(256), 0, s, acc, src, n);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

size_t ovc_bw_box_relation_scratch_floats(int B, int N, int h, int d_g) {
    if (B < 1 || N < 1 || h < 1 || d_g < 1) return 0;
    const size_t rows = (size_t)B * N, nout = (size_t)h * (d_g + 1);
    return box_pad4(rows * nout) + box_pad4(((rows + kChunk - 1) / kChunk) * nout) + box_pad4(nout);
}

int ovc_bw_box_relation(const float* boxes, const float* w, const float* dG, int B, int N, int h, int d_g, int trig, float* scratch,
                        float* dfc_w, float* dfc_b, hipStream_t s) {
    if (!boxes || !w || !dG || !scratch || !dfc_w || !dfc_b) return OVC_EINVAL;
    if (!ovc_aligned16(boxes) || !ovc_aligned16(w) || !ovc_aligned16(dG) || !ovc_aligned16(scratch) || !ovc_aligned16(dfc_w) ||
        !ovc_aligned16(dfc_b)) return OVC_EINVAL;
    if (B < 1 || N < 1 || N > 1024 || h < 1 || h > 16 || (long)B * N > 0x7fffffffL / 2) return OVC_EINVAL;
    if (trig ? (d_g < 8 || d_g > 64 || d_g % 8 != 0) : d_g != 4) return OVC_EINVAL;
    const int rows = B * N, nout = h * (d_g + 1);
    float* part = scratch;
    float* colpart = part + box_pad4((size_t)rows * nout);
    float* sum = colpart + box_pad4((size_t)((rows + kChunk - 1) / kChunk) * nout);
    const size_t lds = ((size_t)kBoxTile * d_g + (size_t)kBoxTile * h + kBoxTile * 4) * sizeof(float);
    hipLaunchKernelGGL(bw_box_relation_kernel, dim3(rows), dim3(kBoxThreads), lds, s, boxes, w, dG, N, h, d_g, trig ? 1 : 0, part);
    OVC_RETURN_IF_LAUNCH_FAILED();
    if (const int rc = ovc_bw_colsum(part, nout, rows, nout, colpart, sum, s)) return rc;
    hipLaunchKernelGGL(bw_box_relation_write_kernel, dim3((nout + 255) / 256), dim3(256), 0, s, sum, h, d_g, dfc_w, dfc_b);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

// Test hooks (include/ovc.h; tests/test_geometric_train_gpu.py): ovc_bw_box_relation and ovc_bw_attention on caller-supplied buffers.
extern "C" size_t ovc_debug_box_relation_backward_floats(int B, int N, int h, int d_g) {
    return ovc_bw_box_relation_scratch_floats(B, N, h, d_g);
}

extern "C" int ovc_debug_box_relation_backward(const float* boxes, const float* w, const float* dG, int B, int N, int h, int d_g, int trig,
                                               float* scratch, size_t scratch_floats, float* dfc_w, float* dfc_b, ovc_stream stream) {
    if (B < 1 || N < 1 || h < 1 || d_g < 1 || scratch_floats < ovc_bw_box_relation_scratch_floats(B, N, h, d_g)) return OVC_EINVAL;
    if (const int rc = ovc_device_guard()) return rc;
    return ovc_bw_box_relation(boxes, w, dG, B, N, h, d_g, trig, scratch, dfc_w, dfc_b, ovc_hip_stream(stream));
}

extern "C" int ovc_debug_attention_backward(const float* q, const float* k, const float* v, const float* dout, const uint8_t* mask,
                                            const float* geometry, int B, int nq, int nk, int h, int dk, float* P, float* dS, float* dq,
                                            float* dk_out, float* dv_out, ovc_stream stream) {
    if (!q || !k || !v || !dout || !P || !dS || !dq || !dk_out || !dv_out || B <= 0 || nq <= 0 || nk <= 0 || h <= 0) return OVC_EINVAL;
    if (dk <= 0 || dk > 64 || nk > 8000 || (long)B * h * std::max(nq, nk) > 0x7fffffffL / 2) return OVC_EINVAL;   // LDS: 128 + 2 nk floats
    if (const int rc = ovc_device_guard()) return rc;
    const int hk = h * dk;
    AttnBwdArgs a{};
    a.q = q; a.ldq = hk; a.k = k; a.v = v; a.ldkv = hk; a.dout = dout; a.ldo = hk;
    a.mask = mask; a.mask_b = nk; a.mask_r = 0;
    a.B = B; a.nq = nq; a.nk = nk; a.h = h; a.dk = dk; a.scale = sqrtf((float)dk);
    a.P = P; a.dS = dS; a.dq = dq; a.lddq = hk; a.dk_out = dk_out; a.dv_out = dv_out; a.lddkv = hk;
    a.geometry = geometry;
    return ovc_bw_attention(a, ovc_hip_stream(stream));
}

extern "C" int ovc_debug_aoa_gate_backward(const float* dout, const float* info, const float* gate, long n, int d, float* dcat,
                                           ovc_stream stream) {
    if (const int rc = ovc_device_guard()) return rc;
    return ovc_bw_aoa_gate(dout, info, gate, n, d, dcat, ovc_hip_stream(stream));
}

extern "C" int ovc_debug_meshed_mix_backward(const float* dmixed, const float* alpha, const float* enc, int levels, long n, float divisor,
                                             float* denc, float* dalpha, ovc_stream stream) {
    if (const int rc = ovc_device_guard()) return rc;          // one device per process (include/ovc.h)
    return ovc_bw_meshed_mix(dmixed, alpha, enc, levels, n, divisor, denc, dalpha, ovc_hip_stream(stream));
}

// ---- Test hooks (include/ovc.h, "the kernels of the training backward on caller buffers"; tests/test_backward_gpu.py) ------------
// Each validates everything it can on the host, BEFORE the device guard (so the refusals hold on a machine with no GPU and write
// nothing), then calls the launcher the engine calls.
namespace {

inline bool dbg_f32(const void* p) { return p && (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }        // a float / int32 array
inline bool dbg_f32_or_null(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
inline bool dbg_i64(const void* p) { return p && (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }        // an int64 array
inline long dbg_pad4(long n) { return (n + 3) & ~3L; }
constexpr long kDbgGridY = 65535;                                                                     // tiles along a grid's y
inline bool dbg_prob(float p) { return p >= 0.f && p < 1.f; }                                         // NaN: false

}  // namespace

extern "C" int ovc_debug_bw_transpose(const float* src, long lds, int rows, int cols, float* dst, long ldd, int rows_pad,
                                      ovc_stream stream) {
    if (!dbg_f32(src) || !dbg_f32(dst) || rows <= 0 || cols <= 0 || lds < cols || rows_pad < rows || ldd < rows_pad) return OVC_EINVAL;
    if (((long)cols + 63) / 64 > kDbgGridY) return OVC_EINVAL;
    if (const int rc = ovc_device_guard()) return rc;
    return ovc_bw_transpose(src, lds, rows, cols, dst, ldd, rows_pad, ovc_hip_stream(stream));
}

extern "C" int ovc_debug_bw_rowsum(const float* src, long ld, int rows, int n, float* dst, ovc_stream stream) {
    if (!dbg_f32(src) || !dbg_f32(dst) || rows <= 0 || n <= 0 || ld < n) return OVC_EINVAL;
    if (const int rc = ovc_device_guard()) return rc;
    return ovc_bw_rowsum(src, ld, rows, n, dst, ovc_hip_stream(stream));
}

extern "C" int ovc_debug_bw_colsum(const float* src, long ld, int rows, int cols, float* part, size_t part_floats, float* dst,
                                   ovc_stream stream) {
    if (!dbg_f32(src) || !dbg_f32(part) || !dbg_f32(dst) || rows <= 0 || cols <= 0 || ld < cols) return OVC_EINVAL;
    const long chunks = ((long)rows + kChunk - 1) / kChunk;
    if (chunks > kDbgGridY || part_floats < (size_t)chunks * (size_t)cols) return OVC_EINVAL;
    if (const int rc = ovc_device_guard()) return rc;
    return ovc_bw_colsum(src, ld, rows, cols, part, dst, ovc_hip_stream(stream));
}

extern "C" int ovc_debug_bw_layer_norm(int form, const float* x, const float* r, const float* gamma, const float* dy,
                                       const uint8_t* zero_rows, float alpha, float eps, int rows, int d, float* dx, float* prod,
                                       float* dyc, float* dproj, const int64_t* seed, int site, float p, int drop_cols,
                                       const int32_t* rowmap, ovc_stream stream) {
    if (form < 0 || form > 3 || !dbg_f32(x) || !dbg_f32(gamma) || !dbg_f32(dy) || !dbg_f32(dx) || !dbg_f32(prod) || !dbg_f32(dyc))
        return OVC_EINVAL;
    if (rows <= 0 || d <= 0 || d > 2048 || !(eps >= 0.f)) return OVC_EINVAL;
    const bool drop = form == 1 || form == 2;
    if (drop ? (!dbg_f32(dproj) || !dbg_i64(seed) || site < 0 || site >= OVC_DROPOUT_SITES || !dbg_prob(p) || drop_cols != d)
             : (dproj || seed)) return OVC_EINVAL;
    if (form == 2 ? !dbg_f32(rowmap) : rowmap != nullptr) return OVC_EINVAL;
    if (form == 3 ? (!dbg_f32(r) || zero_rows) : r != nullptr) return OVC_EINVAL;
    if (const int rc = ovc_device_guard()) return rc;
    hipStream_t s = ovc_hip_stream(stream);
    if (form == 0) return ovc_bw_layer_norm(x, gamma, dy, zero_rows, eps, rows, d, dx, prod, dyc, s);
    if (form == 3) return ovc_bw_layer_norm_post(x, r, gamma, dy, alpha, eps, rows, d, dx, prod, dyc, s);
    const DropoutSite drop_site{seed, (uint32_t)site, ovc_dropout_threshold(p), ovc_dropout_scale(p), drop_cols};
    if (form == 1) return ovc_bw_layer_norm_dropout(x, gamma, dy, zero_rows, eps, rows, d, dx, prod, dyc, dproj, drop_site, s);
    return ovc_bw_layer_norm_dropout_mapped(x, gamma, dy, zero_rows, eps, rows, d, dx, prod, dyc, dproj, drop_site, rowmap, s);
}

extern "C" int ovc_debug_bw_relu(float* g, const float* act, int dropout, float p, long n, ovc_stream stream) {
    if (!dbg_f32(g) || !dbg_f32(act) || n <= 0 || (dropout != 0 && dropout != 1) || (dropout && !dbg_prob(p))) return OVC_EINVAL;
    if (const int rc = ovc_device_guard()) return rc;
    if (dropout) return ovc_bw_relu_dropout(g, act, ovc_dropout_scale(p), n, ovc_hip_stream(stream));
    return ovc_bw_relu(g, act, n, ovc_hip_stream(stream));
}

extern "C" int ovc_debug_bw_leaky(const float* g, const float* act, float scale, float slope, float* out, long n, ovc_stream stream) {
    if (!dbg_f32(g) || !dbg_f32(act) || !dbg_f32(out) || n <= 0) return OVC_EINVAL;
    if (const int rc = ovc_device_guard()) return rc;
    return ovc_bw_leaky(g, act, scale, slope, out, n, ovc_hip_stream(stream));
}

extern "C" int ovc_debug_bw_sum(const float* a, long lda, const float* b, long ldb, const float* c, long ldc, int rows, int cols,
                                float* y, long ldy, ovc_stream stream) {
    if (!dbg_f32(a) || !dbg_f32(b) || !dbg_f32_or_null(c) || !dbg_f32(y) || rows <= 0 || cols <= 0) return OVC_EINVAL;
    if (lda < cols || ldb < cols || (c && ldc < cols) || ldy < cols) return OVC_EINVAL;
    if (const int rc = ovc_device_guard()) return rc;
    return ovc_bw_sum(a, lda, b, ldb, c, ldc, rows, cols, y, ldy, ovc_hip_stream(stream));
}

extern "C" int ovc_debug_bw_sum_levels(const float* acc, const float* src, int levels, long stride, long n, float* out,
                                       ovc_stream stream) {
    if (!dbg_f32_or_null(acc) || !dbg_f32(src) || !dbg_f32(out) || levels < 1 || levels > OVC_MAX_LEVELS || n <= 0 || stride < n)
        return OVC_EINVAL;
    if (const int rc = ovc_device_guard()) return rc;
    return ovc_bw_sum_levels(acc, src, levels, stride, n, out, ovc_hip_stream(stream));
}

extern "C" int ovc_debug_bw_accumulate(float* acc, const float* src, long n, ovc_stream stream) {
    if (!dbg_f32(acc) || !dbg_f32(src) || n <= 0) return OVC_EINVAL;
    if (const int rc = ovc_device_guard()) return rc;
    return ovc_bw_accumulate(acc, src, n, ovc_hip_stream(stream));
}

extern "C" size_t ovc_debug_bw_loss_part_floats(int rows, int V) {
    return rows > 0 && V > 0 ? ovc_bw_smoothed_part_floats(rows, V) : 0;
}

extern "C" int ovc_debug_bw_loss(int head, const float* logits_t, long ldt, const float* lse, const int32_t* tgt, int pad, int rows,
                                 int V, float param, int reduction, const float* teacher, float* part, size_t part_floats, float* row_a,
                                 float* row_b, float* w_row, float* loss, float* dl_t, float* dl, long ldv, ovc_stream stream) {
    if (head < 0 || head > 3 || !dbg_f32(logits_t) || !dbg_f32(lse) || !dbg_f32(tgt) || !dbg_f32(w_row) || !dbg_f32(dl_t) || !dbg_f32(dl))
        return OVC_EINVAL;
    if (rows <= 0 || V <= 0 || pad < 0 || pad >= V || ldt < rows || ldt > dbg_pad4(rows) || ldv < V || (ldv + 63) / 64 > kDbgGridY)
        return OVC_EINVAL;
    if (head == 1 ? loss != nullptr : !dbg_f32(loss)) return OVC_EINVAL;
    const size_t need = ovc_bw_smoothed_part_floats(rows, V);
    if (head == 2) {
        if (!dbg_f32(part) || part_floats < need || !dbg_f32(row_a) || row_b || teacher) return OVC_EINVAL;
        if (!dbg_prob(param) || (reduction != 0 && reduction != 1) || (param > 0.f && V <= 2)) return OVC_EINVAL;
    } else if (head == 3) {
        if (!dbg_f32(part) || part_floats < 2 * need || !dbg_f32(row_a) || !dbg_f32(row_b) || !dbg_f32(teacher)) return OVC_EINVAL;
        if (!(param >= 0.f && param <= 1.f)) return OVC_EINVAL;
    } else if (part || row_a || row_b || teacher) {
        return OVC_EINVAL;
    }
    if (const int rc = ovc_device_guard()) return rc;
    hipStream_t s = ovc_hip_stream(stream);
    if (head == 0) return ovc_bw_xent(logits_t, ldt, lse, tgt, pad, rows, V, w_row, loss, dl_t, dl, ldv, s);
    if (head == 1) return ovc_bw_dlogit(logits_t, ldt, lse, tgt, w_row, rows, V, dl_t, dl, ldv, s);
    if (head == 2) {
        // the constants of engine.hip's make_smoothed_loss: float64, rounded once
        const double sm = param, conf = 1.0 - sm, u = sm > 0.0 ? sm / (V - 2) : 0.0;
        const auto xlogx = [](double v) { return v > 0 ? v * std::log(v) : 0.0; };
        const SmoothedLoss l{(float)conf, (float)u, (float)(xlogx(conf) + (V - 2) * xlogx(u)), (float)(1.0 / ((double)rows * V)), reduction};
        return ovc_bw_xent_smoothed(logits_t, ldt, lse, tgt, pad, rows, V, l, part, row_a, w_row, loss, dl_t, dl, ldv, s);
    }
    const SoftLoss l{(float)(1.0 - (double)param), param};                     // ovc_forward_backward_distill's two weights
    return ovc_bw_xent_soft(logits_t, ldt, lse, tgt, pad, rows, V, l, teacher, part, row_a, row_b, w_row, loss, dl_t, dl, ldv, s);
}

extern "C" int ovc_debug_bw_embedding(const int32_t* tok, int rows, int pad, const float* dx, int d, int V, float* out, ovc_stream stream) {
    if (!dbg_f32(tok) || !dbg_f32(dx) || !dbg_f32(out) || rows <= 0 || d <= 0 || d > 2048 || V <= 0 || pad < 0 || pad >= V) return OVC_EINVAL;
    if (const int rc = ovc_device_guard()) return rc;
    return ovc_bw_embedding(tok, rows, pad, dx, d, V, out, ovc_hip_stream(stream));
}

extern "C" int ovc_debug_bw_tokens(const int64_t* tokens, int rows, int V, int32_t* tok32, ovc_stream stream) {
    if (!dbg_i64(tokens) || !dbg_f32(tok32) || rows <= 0 || V <= 0) return OVC_EINVAL;
    if (const int rc = ovc_device_guard()) return rc;
    return ovc_bw_tokens(tokens, rows, V, tok32, ovc_hip_stream(stream));
}

extern "C" int ovc_debug_bw_attention(const float* q, long ldq, const float* k, const float* v, long ldkv, const float* dout, long ldo,
                                      const uint8_t* mask, long mask_b, long mask_r, const float* geometry, int B, int nq, int nk, int h,
                                      int dk, float* P, float* dS, float* dq, long lddq, float* dk_out, float* dv_out, long lddkv,
                                      ovc_stream stream) {
    if (!dbg_f32(q) || !dbg_f32(k) || !dbg_f32(v) || !dbg_f32(dout) || !dbg_f32_or_null(geometry) || !dbg_f32(P) || !dbg_f32(dS) ||
        !dbg_f32(dq) || !dbg_f32(dk_out) || !dbg_f32(dv_out)) return OVC_EINVAL;
    if (B <= 0 || nq <= 0 || nk <= 0 || h <= 0 || dk <= 0 || dk > 64 || nk > 8000) return OVC_EINVAL;               // LDS: 128 + 2 nk floats
    if ((long)B * h * std::max(nq, nk) > 0x7fffffffL / 2) return OVC_EINVAL;
    const long hk = (long)h * dk;
    if (ldq < hk || ldkv < hk || ldo < hk || lddq < hk || lddkv < hk) return OVC_EINVAL;
    if (mask && (mask_b < 0 || mask_r < 0 || (mask_r != 0 && mask_r < nk))) return OVC_EINVAL;
    if (const int rc = ovc_device_guard()) return rc;
    AttnBwdArgs a{};
    a.q = q; a.ldq = ldq; a.k = k; a.v = v; a.ldkv = ldkv; a.dout = dout; a.ldo = ldo;
    a.mask = mask; a.mask_b = mask_b; a.mask_r = mask_r;
    a.B = B; a.nq = nq; a.nk = nk; a.h = h; a.dk = dk; a.scale = sqrtf((float)dk);
    a.P = P; a.dS = dS; a.dq = dq; a.lddq = lddq; a.dk_out = dk_out; a.dv_out = dv_out; a.lddkv = lddkv;
    a.geometry = geometry;
    return ovc_bw_attention(a, ovc_hip_stream(stream));
}
