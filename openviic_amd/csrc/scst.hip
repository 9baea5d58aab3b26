// The self-critical baseline, advantage and loss gradient (ovc_scst_advantage, include/ovc.h): what the reference's train_scst
// (vi_trainer.py:121-158) does between the search and loss.backward().  Small and latency-bound: B*S rewards, B*S*T log-probabilities.
//
// One workgroup per chunk of 64 images.  A lane owns one (image, beam) pair: the baseline and advantage in float64 from the fp32
// rewards, the advantage rounded to fp32 once for the gradient, its T log-probabilities summed ascending in float64.  The gradient,
// one value per pair, is then stored over the pair's T positions by the whole workgroup (16-byte stores where T % 4 == 0).  The
// three running numbers are float64 sums in the project's column-sum order: ascending inside an image, the chunk's images
// ascending, the chunks ascending (a second one-wave launch; a batch of one chunk finishes in the first).  No atomics; every value
// is written by exactly one lane with plain vector stores.
#include "common.h"

#pragma clang fp contract(off)          // every product and sum below rounds once, as written (openviic_amd/scst.py mirrors it)

namespace {

constexpr int kImages = 64;             // images per chunk: the column-sum convention
constexpr int kThreads = 256;
constexpr int kPairs = kImages * OVC_MAX_BEAM;
constexpr int kPartial = 4;             // doubles per chunk in scratch: loss terms, rewards, baselines, (pad)

// the float64 sum of an image's fp32 rewards, ascending: exact whenever it fits 53 bits (always, for equal rewards)
__device__ __forceinline__ double reward_sum(const float* __restrict__ r, int S) {
    double sum = (double)r[0];
    for (int j = 1; j < S; ++j) sum = sum + (double)r[j];
    return sum;
}

// stats[q] of the finished sums: the mean over the B*S pairs (loss, reward) or over the B images (baseline), rounded to fp32 once
__device__ __forceinline__ void write_stat(float* __restrict__ stats, int q, double sum, int B, int S) {
    stats[q] = q == 3 ? 0.f : (float)(sum / (q == 2 ? (double)B : (double)B * (double)S));
}

__global__ __launch_bounds__(kThreads) void scst_advantage_kernel(const float* __restrict__ reward, const float* __restrict__ logp,
                                                                  int B, int S, int T, int vec4, float* __restrict__ grad_logp,
                                                                  float* __restrict__ stats, double* __restrict__ partial) {
    __shared__ double term_s[kPairs];           // -(mean_t logp) * advantage of each pair of the chunk
    __shared__ float grad_s[kPairs];            // the pair's gradient value
    __shared__ double image_s[3][kImages];      // per image: its loss terms, its rewards, its baseline
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * kImages;
    const int images = B - b0 < kImages ? B - b0 : kImages;
    const int pairs = images * S;

    // 1. one lane per (image, beam)
    for (int p = tid; p < pairs; p += kThreads) {
        const int img = p / S, s = p - img * S;
        const float* r = reward + (size_t)(b0 + img) * S;
        // baseline and advantage in float64 from the fp32 rewards; the gradient carries the advantage rounded to fp32 once (equal
        // rewards give an exact 0), the loss term below the unrounded one
        const double a64 = (double)r[s] - reward_sum(r, S) / (double)S;
        const float a = (float)a64;
        grad_s[p] = (-a / (float)(B * S)) / (float)T;           // the outer mean's scaling first, then the inner mean's
        const float* x = logp + ((size_t)(b0 + img) * S + s) * T;
        double acc = 0.0;
        if (vec4) {
            const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
#pragma unroll 4
            for (int i = 0; i < (T >> 2); ++i) {
                const f32x4 v = x4[i];
                acc = acc + (double)v[0];
                acc = acc + (double)v[1];
                acc = acc + (double)v[2];
                acc = acc + (double)v[3];
            }
        } else {
#pragma unroll 8
            for (int t = 0; t < T; ++t) acc = acc + (double)x[t];
        }
        term_s[p] = -(acc / (double)T) * a64;
    }
    __syncthreads();

    // 2. the gradient over every position of the chunk's pairs: contiguous in memory from the chunk's first element
    float* g0 = grad_logp + (size_t)b0 * S * T;
    if (vec4) {
        f32x4* g4 = reinterpret_cast<f32x4*>(g0);
        const int T4 = T >> 2;
        for (int i = tid; i < pairs * T4; i += kThreads) {
            const float g = grad_s[i / T4];
            g4[i] = f32x4{g, g, g, g};
        }
    } else {
        for (int i = tid; i < pairs * T; i += kThreads) g0[i] = grad_s[i / T];
    }

    // 3. per image, beams ascending; then the chunk's images ascending, one lane per quantity
    if (tid < images) {
        const float* r = reward + (size_t)(b0 + tid) * S;
        double loss = term_s[tid * S];
        for (int j = 1; j < S; ++j) loss = loss + term_s[tid * S + j];
        const double sum = reward_sum(r, S);
        image_s[0][tid] = loss;
        image_s[1][tid] = sum;
        image_s[2][tid] = sum / (double)S;
    }
    __syncthreads();
    if (tid < 3) {
        double sum = image_s[tid][0];
        for (int i = 1; i < images; ++i) sum = sum + image_s[tid][i];
        if (gridDim.x == 1) write_stat(stats, tid, sum, B, S);
        else partial[(size_t)blockIdx.x * kPartial + tid] = sum;
    } else if (tid == 3 && gridDim.x == 1) {
        write_stat(stats, 3, 0.0, B, S);
    }
}

__global__ __launch_bounds__(OVC_WAVE) void scst_stats_kernel(const double* __restrict__ partial, int chunks, int B, int S,
                                                              float* __restrict__ stats) {
    const int q = threadIdx.x;
    if (q > 3) return;
    double sum = 0.0;
    if (q < 3) {
        sum = partial[q];
        for (int c = 1; c < chunks; ++c) sum = sum + partial[(size_t)c * kPartial + q];
    }
    write_stat(stats, q, sum, B, S);
}

inline bool shape_ok(int B, int S, int T) {
    return B >= 1 && S >= 1 && S <= OVC_MAX_BEAM && T >= 1 && T <= OVC_MAX_LEN && (long)B * S <= 0x7fffffffL / T;
}

}  // namespace

extern "C" size_t ovc_scst_advantage_bytes(int B, int S, int T) {
    if (!shape_ok(B, S, T)) return 0;
    return (size_t)((B + kImages - 1) / kImages) * kPartial * sizeof(double);
}

extern "C" int ovc_scst_advantage(const float* reward, const float* logp, int B, int S, int T, float* grad_logp, float* stats,
                                  void* scratch, size_t scratch_bytes, ovc_stream stream) {
    const size_t need = ovc_scst_advantage_bytes(B, S, T);
    if (need == 0 || !reward || !logp || !grad_logp || !stats || !scratch) return OVC_EINVAL;
    if ((reinterpret_cast<uintptr_t>(scratch) & 7u) != 0) return OVC_EINVAL;
    if (scratch_bytes < need) return OVC_EWORKSPACE;
    if (const int rc = ovc_device_guard()) return rc;
    const int chunks = (B + kImages - 1) / kImages;
    const int vec4 = (T % 4 == 0 && ovc_aligned16(logp) && ovc_aligned16(grad_logp)) ? 1 : 0;
    double* partial = static_cast<double*>(scratch);
    hipLaunchKernelGGL(scst_advantage_kernel, dim3((unsigned)chunks), dim3(kThreads), 0, ovc_hip_stream(stream), reward, logp, B, S, T,
                       vec4, grad_logp, stats, partial);
    OVC_RETURN_IF_LAUNCH_FAILED();
    if (chunks > 1) {
        hipLaunchKernelGGL(scst_stats_kernel, dim3(1), dim3(OVC_WAVE), 0, ovc_hip_stream(stream), partial, chunks, B, S, stats);
        OVC_RETURN_IF_LAUNCH_FAILED();
    }
    return OVC_OK;
}
