// The optimizer step: one multi-tensor Adam update per parameter group (ovc_adam_step, include/ovc.h; torch/optim/adam.py's
// single-tensor form, the optimizer of the reference's trainers).  Memory-bound: 28 bytes per element, nothing is reused.
//
// Work is cut into chunks of kChunk elements (a tensor's last chunk is shorter); a chunk table in device memory maps a chunk to
// (tensor, first element), so a 512-element bias costs one chunk and the 5 M-element embedding is 1276 of them, spread over the
// chip.  Workgroups stride over the chunk table.  Inside a chunk a tensor whose four pointers share their offset in a 16-byte line
// runs a scalar head (up to 3 elements, until the line starts), 16-byte loads and stores over the body and a scalar tail;
// pointers that disagree run the whole chunk in the scalar form.  Every element is read and written by exactly one lane, through
// one function with a fixed operation order and no contraction: the same bits whatever the path, the grid and the stream.
#include "common.h"

#pragma clang fp contract(off)          // every product and sum below rounds once, as written (openviic_amd/optim.py mirrors it)

namespace {

constexpr int kChunk = 4096;            // elements: 256 lanes x 4 float4 x 4 arrays in flight per workgroup
constexpr int kThreads = 256;
constexpr unsigned kMaxBlocks = 2048;   // 256 CUs x 8 workgroups

// the table's pointers are device memory: said in the type, so the accesses are global_load / global_store, not flat ones
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) f32x4 gf32x4;

struct adam_scalars {
    float w1;          // 1 - beta1
    float beta2;
    float w2;          // 1 - beta2
    float step_size;   // lr / (1 - beta1^t)
    float bc2_sqrt;    // sqrt(1 - beta2^t)
    float eps;
};

// m' = m + (g - m) w1;  v' = beta2 v + (w2 g) g;  p' = p - (step_size m') / (sqrt(v') / bc2_sqrt + eps)
__device__ __forceinline__ void adam_element(float& p, float g, float& m, float& v, float scale, const adam_scalars& s) {
    g = g * scale;
    m = m + (g - m) * s.w1;
    v = s.beta2 * v + (s.w2 * g) * g;
    const float denom = sqrtf(v) / s.bc2_sqrt + s.eps;      // sqrtf and / are correctly rounded in this build (no fast-math)
    p = p - (s.step_size * m) / denom;
}

__device__ __forceinline__ void adam_scalar_at(const ovc_adam_tensor& t, long i, float scale, const adam_scalars& s) {
    gfloat* pp = (gfloat*)t.param + i;
    gfloat* pm = (gfloat*)t.exp_avg + i;
    gfloat* pv = (gfloat*)t.exp_avg_sq + i;
    float p = *pp, m = *pm, v = *pv;
    adam_element(p, *((const gfloat*)t.grad + i), m, v, scale, s);
    *pp = p;
    *pm = m;
    *pv = v;
}

__global__ __launch_bounds__(kThreads) void adam_step_kernel(const ovc_adam_tensor* __restrict__ table,
                                                             int n_tensors, const ovc_adam_chunk* __restrict__ chunks, int n_chunks,
                                                             const float* __restrict__ grad_scale, const adam_scalars s) {
    const float scale = grad_scale ? *grad_scale : 1.f;
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const ovc_adam_chunk ch = chunks[c];
        if (ch.tensor < 0 || ch.tensor >= n_tensors || ch.first < 0) continue;     // a chunk table that is not this tensor table's
        const ovc_adam_tensor t = table[ch.tensor];
        const long first = ch.first;
        const long left = t.count - first;
        if (left <= 0) continue;
        const int len = left < kChunk ? (int)left : kChunk;
        const uintptr_t ap = reinterpret_cast<uintptr_t>(t.param + first);
        const bool same_line = ((ap ^ reinterpret_cast<uintptr_t>(t.grad + first)) & 15u) == 0 &&
                               ((ap ^ reinterpret_cast<uintptr_t>(t.exp_avg + first)) & 15u) == 0 &&
                               ((ap ^ reinterpret_cast<uintptr_t>(t.exp_avg_sq + first)) & 15u) == 0;
        if (!same_line) {                                         // uniform per chunk: no 16-byte access fits all four arrays
            for (int i = threadIdx.x; i < len; i += kThreads) adam_scalar_at(t, first + i, scale, s);
            continue;
        }
        int head = (int)((16u - (unsigned)(ap & 15u)) & 15u) >> 2;      // elements before the next 16-byte line (pointers: 4-byte aligned)
        head = head < len ? head : len;
        const int body = (len - head) >> 2;                       // float4 groups
        const int tail = (len - head) & 3;
        if ((int)threadIdx.x < head) adam_scalar_at(t, first + threadIdx.x, scale, s);
        if ((int)threadIdx.x < tail) adam_scalar_at(t, first + head + 4 * body + threadIdx.x, scale, s);
        gf32x4* p4 = (gf32x4*)(t.param + first + head);
        const gf32x4* g4 = (const gf32x4*)(t.grad + first + head);
        gf32x4* m4 = (gf32x4*)(t.exp_avg + first + head);
        gf32x4* v4 = (gf32x4*)(t.exp_avg_sq + first + head);
        for (int i = threadIdx.x; i < body; i += kThreads) {
            f32x4 p = p4[i], m = m4[i], v = v4[i];
            const f32x4 g = g4[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float pj = p[j], mj = m[j], vj = v[j];
                adam_element(pj, g[j], mj, vj, scale, s);
                p[j] = pj; m[j] = mj; v[j] = vj;
            }
            p4[i] = p;
            m4[i] = m;
            v4[i] = v;
        }
    }
}

// ---- the global L2 norm of the gradients and the clip coefficient (ovc_grad_norm, include/ovc.h) ---------------------------------
// Pass 1, one workgroup per chunk (workgroups stride over the chunk table as above): element e of the chunk belongs to lane
// (e / 4) % 256 whatever the pointer's alignment, so a lane's elements are the float4 groups lane, lane + 256, lane + 512,
// lane + 768 of the chunk, taken in ascending address order through one fmaf chain.  A group past the end contributes
// fmaf(0, 0, acc), which is acc bit for bit (acc is never -0), so all four loads are issued before the first use.  Then the xor
// butterfly of wave_sum (32, 16, 8, 4, 2, 1), and (w0 + w1) + (w2 + w3) over the four waves in LDS.  Lane 0 stores the partial.
constexpr int kWaves = kThreads / OVC_WAVE;
constexpr int kGroupsPerLane = kChunk / (4 * kThreads);

__global__ __launch_bounds__(kThreads) void grad_norm_partial_kernel(const ovc_adam_tensor* __restrict__ table, int n_tensors,
                                                                     const ovc_adam_chunk* __restrict__ chunks, int n_chunks,
                                                                     float* __restrict__ partials) {
    __shared__ float wave_sums[kWaves];
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const ovc_adam_chunk ch = chunks[c];
        const gfloat* g = nullptr;
        int len = 0;                                              // a chunk that is not this table's: a partial of 0
        if (ch.tensor >= 0 && ch.tensor < n_tensors && ch.first >= 0) {
            const long left = table[ch.tensor].count - ch.first;
            len = left <= 0 ? 0 : left < kChunk ? (int)left : kChunk;
            g = (const gfloat*)table[ch.tensor].grad + ch.first;
        }
        f32x4 v[kGroupsPerLane];
        if ((reinterpret_cast<uintptr_t>(g) & 15u) == 0) {        // uniform per chunk
            const gf32x4* g4 = (const gf32x4*)g;
#pragma unroll
            for (int k = 0; k < kGroupsPerLane; ++k) {
                const int e = 4 * ((int)threadIdx.x + k * kThreads);
                if (e + 4 <= len) {
                    v[k] = g4[e >> 2];
                } else {                                          // the tensor's last, partial group (or nothing)
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[k][j] = e + j < len ? g[e + j] : 0.f;
                }
            }
        } else {                                                  // a view 4, 8 or 12 bytes into a line: the same elements, scalar loads
#pragma unroll
            for (int k = 0; k < kGroupsPerLane; ++k) {
                const int e = 4 * ((int)threadIdx.x + k * kThreads);
#pragma unroll
                for (int j = 0; j < 4; ++j) v[k][j] = e + j < len ? g[e + j] : 0.f;
            }
        }
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < kGroupsPerLane; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = fmaf(v[k][j], v[k][j], acc);
        acc = wave_sum(acc);
        if ((threadIdx.x & (OVC_WAVE - 1)) == 0) wave_sums[threadIdx.x / OVC_WAVE] = acc;
        __syncthreads();
        if (threadIdx.x == 0) partials[c] = (wave_sums[0] + wave_sums[1]) + (wave_sums[2] + wave_sums[3]);
        __syncthreads();                                          // wave_sums is written again for the next chunk
    }
}

// Pass 2, one workgroup: lane l adds partials l, l + 256, ... ascending in float64, the same butterfly and tree in float64, the
// sum rounded to fp32 once, sqrtf (correctly rounded), and torch's clip_grad_norm_ arithmetic in fp32.  Lane 0 stores both values.
__global__ __launch_bounds__(kThreads) void grad_norm_final_kernel(const float* __restrict__ partials, int n_chunks, float max_norm,
                                                                   int clip, float* __restrict__ out) {
    __shared__ double wave_sums[kWaves];
    double acc = 0.0;
    for (long base = threadIdx.x; base < n_chunks; base += 8 * kThreads) {    // eight loads in flight; + 0.0 keeps acc's bits
        float p[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) p[k] = base + k * kThreads < n_chunks ? partials[base + k * kThreads] : 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) acc += (double)p[k];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if ((threadIdx.x & (OVC_WAVE - 1)) == 0) wave_sums[threadIdx.x / OVC_WAVE] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float total = sqrtf((float)((wave_sums[0] + wave_sums[1]) + (wave_sums[2] + wave_sums[3])));
        float coef = 1.f;
        if (clip) {
            coef = max_norm / (total + 1e-6f);
            coef = coef > 1.f ? 1.f : coef;                       // torch.clamp(max=1): a NaN stays a NaN
        }
        out[0] = total;
        out[1] = coef;
    }
}

}  // namespace

extern "C" long ovc_adam_chunk_count(const int64_t* counts, int n_tensors) {
    if (!counts || n_tensors < 0) return -1;
    long total = 0;
    for (int i = 0; i < n_tensors; ++i) {
        if (counts[i] < 0 || counts[i] > OVC_ADAM_MAX_COUNT) return -1;
        total += (long)((counts[i] + kChunk - 1) / kChunk);
    }
    return total > 0x7fffffffL ? -1 : total;
}

extern "C" long ovc_adam_chunk_fill(const int64_t* counts, int n_tensors, ovc_adam_chunk* chunks, long capacity) {
    const long total = ovc_adam_chunk_count(counts, n_tensors);
    if (total < 0 || !chunks || capacity < total) return -1;
    long at = 0;
    for (int i = 0; i < n_tensors; ++i)
        for (int64_t first = 0; first < counts[i]; first += kChunk) chunks[at++] = ovc_adam_chunk{i, (int32_t)first};
    return total;
}

extern "C" int ovc_adam_step(const ovc_adam_tensor* table, int n_tensors, const ovc_adam_chunk* chunks, long n_chunks, double lr,
                             double beta1, double beta2, double eps, long step, const float* grad_scale, ovc_stream stream) {
    if (n_tensors < 0 || n_chunks < 0 || n_chunks > 0x7fffffffL || step < 1) return OVC_EINVAL;
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !(lr >= 0.0)) return OVC_EINVAL;
    if (n_tensors == 0 || n_chunks == 0) return OVC_OK;
    if (!table || !chunks) return OVC_EINVAL;
    if (const int rc = ovc_device_guard()) return rc;
    // the step's scalars, in double as torch prepares them (adam.py _single_tensor_adam), each rounded to fp32 once
    const double bc1 = 1.0 - pow(beta1, (double)step);
    const double bc2_sqrt = sqrt(1.0 - pow(beta2, (double)step));
    adam_scalars s;
    s.w1 = (float)(1.0 - beta1);
    s.beta2 = (float)beta2;
    s.w2 = (float)(1.0 - beta2);
    s.step_size = (float)(lr / bc1);
    s.bc2_sqrt = (float)bc2_sqrt;
    s.eps = (float)eps;
    const unsigned blocks = n_chunks < (long)kMaxBlocks ? (unsigned)n_chunks : kMaxBlocks;
    hipLaunchKernelGGL(adam_step_kernel, dim3(blocks), dim3(kThreads), 0, ovc_hip_stream(stream), table, n_tensors, chunks, (int)n_chunks,
                       grad_scale, s);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

extern "C" int ovc_grad_norm(const ovc_adam_tensor* table, int n_tensors, const ovc_adam_chunk* chunks, long n_chunks, double max_norm,
                             float* partials, float* out, ovc_stream stream) {
    if (n_tensors < 0 || n_chunks < 0 || n_chunks > 0x7fffffffL || max_norm != max_norm || !out) return OVC_EINVAL;
    if (n_chunks > 0 && (!table || !chunks || !partials)) return OVC_EINVAL;
    if (const int rc = ovc_device_guard()) return rc;
    const int clip = max_norm > 0.0 && max_norm <= 3.4028234663852886e38;      // <= 0, +inf, beyond fp32: measure only
    if (n_chunks > 0) {
        const unsigned blocks = n_chunks < (long)kMaxBlocks ? (unsigned)n_chunks : kMaxBlocks;
        hipLaunchKernelGGL(grad_norm_partial_kernel, dim3(blocks), dim3(kThreads), 0, ovc_hip_stream(stream), table, n_tensors, chunks,
                           (int)n_chunks, partials);
        OVC_RETURN_IF_LAUNCH_FAILED();
    }
    hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(kThreads), 0, ovc_hip_stream(stream), partials, (int)n_chunks,
                       clip ? (float)max_norm : 0.f, clip, out);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}
