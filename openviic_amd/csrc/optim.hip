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
