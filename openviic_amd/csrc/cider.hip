// The SCST reward on the device: CIDEr-D of generated captions from token ids (ovc_cider_reward, include/ovc.h; the reference's
// evaluation/cider/cider_scorer.py on strings).  One wave per hypothesis, everything in LDS and registers, float64 throughout.
#include "common.h"

namespace {

constexpr int kOrders = 4;                      // n-gram orders 1..4
constexpr int kMaxWaves = 4;                    // waves (hypotheses) per workgroup
constexpr unsigned kMaxLds = 64u * 1024u;       // dynamic LDS a launch may ask for without raising the kernel's attribute

__host__ __device__ inline int next_pow2(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}
// LDS of one wave: keys [cap] u64 | weight [cap] f64 | head [cap] i32 | words [T rounded to even] i32, cap = pow2 >= 4 T
__host__ __device__ inline unsigned wave_lds_bytes(int T) { return (unsigned)next_pow2(4 * T) * 20u + (unsigned)((T + 1) & ~1) * 4u; }

// LDS written by some lanes of the wave and read by others: the wave runs in lockstep and its LDS operations complete in order;
// the fences keep the compiler from moving an access across the point
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ double wave_sum_f64(double v) {       // one butterfly: a fixed order, the same bits in every lane
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ uint64_t mix(uint64_t x) {
    const uint64_t y = (x ^ (x >> 32)) * 0x9E3779B97F4A7C15ull;
    return y ^ (y >> 29);
}

__device__ __forceinline__ int order_of(uint64_t key) {          // 0-based n-gram order: the highest non-empty 16-bit field
    return (key >> 48) ? 3 : (key >> 32) ? 2 : (key >> 16) ? 1 : 0;
}

__global__ __launch_bounds__(kMaxWaves * OVC_WAVE) void cider_reward_kernel(const ovc_cider c, const int64_t* __restrict__ ids,
                                                                            const int32_t* __restrict__ rows, int S, int T,
                                                                            int hyps, int waves, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int lane = threadIdx.x & (OVC_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / OVC_WAVE);
    const int hyp = blockIdx.x * waves + wave;
    if (hyp >= hyps) return;                                     // whole waves leave: there is no workgroup barrier below
    const int cap = next_pow2(4 * T);
    unsigned char* base = lds + (size_t)wave * wave_lds_bytes(T);
    uint64_t* keys = reinterpret_cast<uint64_t*>(base);
    double* weight = reinterpret_cast<double*>(base + (size_t)cap * 8);
    int32_t* head = reinterpret_cast<int32_t*>(base + (size_t)cap * 16);
    int32_t* words = head + cap;

    // 1. decode: clamp, keep up to and including the first <eos>, drop the specials
    const int64_t* tok = ids + (size_t)hyp * T;
    const uint64_t below = (1ull << lane) - 1ull;
    int L = 0;
    for (int t0 = 0; t0 < T; t0 += OVC_WAVE) {
        const int t = t0 + lane;
        int64_t w = t < T ? tok[t] : (int64_t)c.pad_idx;
        w = w < 0 ? 0 : (w >= c.vocab ? c.vocab - 1 : w);
        const uint64_t ends = __ballot(t < T && w == c.eos_idx);
        const bool live = t < T && (ends == 0 || lane <= __ffsll((unsigned long long)ends) - 1);
        const bool keep = live && w != c.pad_idx && w != c.bos_idx && w != c.eos_idx && w != c.unk_idx;
        const uint64_t kept = __ballot(keep);
        if (keep) words[L + __popcll(kept & below)] = (int32_t)w;
        L += __popcll(kept);
        if (ends) break;
    }
    L = __builtin_amdgcn_readfirstlane(L);
    if (L == 0) {                                                // every term of every sum is 0
        if (lane == 0) out[hyp] = 0.f;
        return;
    }
    wave_sync();

    // 2. the keys of all n-grams, sorted; distinct keys with their term frequencies
    int total = 0;
    for (int n = 1; n <= kOrders; ++n) {
        const int cnt = L - n + 1;
        if (cnt <= 0) break;
        for (int i = lane; i < cnt; i += OVC_WAVE) {
            uint64_t key = 0;
            for (int j = 0; j < n; ++j) key |= (uint64_t)(words[i + j] + 1) << (16 * j);
            keys[total + i] = key;
        }
        total += cnt;
    }
    const int P = next_pow2(total);                              // <= cap: total <= 4 L <= 4 T
    for (int i = total + lane; i < P; i += OVC_WAVE) keys[i] = ~0ull;
    wave_sync();
    for (int k = 2; k <= P; k <<= 1) {                           // bitonic sort, ascending
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < (P >> 1); t += OVC_WAVE) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const uint64_t a = keys[lo], b = keys[hi];
                if ((a > b) == ((lo & k) == 0)) { keys[lo] = b; keys[hi] = a; }
            }
            wave_sync();
        }
    }
    int D = 0;
    for (int i0 = 0; i0 < total; i0 += OVC_WAVE) {
        const int i = i0 + lane;
        const bool first = i < total && (i == 0 || keys[i] != keys[i - 1]);
        const uint64_t firsts = __ballot(first);
        if (first) head[D + __popcll(firsts & below)] = i;
        D += __popcll(firsts);
    }
    D = __builtin_amdgcn_readfirstlane(D);
    wave_sync();

    // 3. tf-idf weights and the hypothesis' norms
    double sq[kOrders] = {0.0, 0.0, 0.0, 0.0};
    const uint32_t mask = (uint32_t)c.hash_size - 1u;
    for (int d = lane; d < D; d += OVC_WAVE) {
        const int start = head[d], end = d + 1 < D ? head[d + 1] : total;
        const uint64_t key = keys[start];
        double idf = c.ref_len;
        if (c.hash_size > 0) {
            uint32_t slot = (uint32_t)mix(key) & mask;
            for (int probe = 0; probe < c.hash_size; ++probe) {
                const uint64_t k = c.hash_key[slot];
                if (k == key) { idf = c.hash_idf[slot]; break; }
                if (k == 0) break;
                slot = (slot + 1) & mask;
            }
        }
        const double w = (double)(end - start) * idf;
        weight[d] = w;
        const int n = order_of(key);
#pragma unroll
        for (int m = 0; m < kOrders; ++m) sq[m] += n == m ? w * w : 0.0;
    }
    double norm_h[kOrders];
#pragma unroll
    for (int m = 0; m < kOrders; ++m) norm_h[m] = sqrt(wave_sum_f64(sq[m]));
    const double len_h = (double)(L - 1);                        // the reference's "length": the number of bigrams

    // 4. similarity to every reference of the image
    int row = rows[hyp / S];
    row = row < 0 ? 0 : (row >= c.n_images ? c.n_images - 1 : row);
    int r0 = 0, r1 = 0;
    if (c.n_images > 0) { r0 = c.image_ref[row]; r1 = c.image_ref[row + 1]; }
    double score[kOrders] = {0.0, 0.0, 0.0, 0.0};
    for (int r = r0; r < r1; ++r) {
        const int e0 = c.ref_entry[r], e1 = c.ref_entry[r + 1];
        double val[kOrders] = {0.0, 0.0, 0.0, 0.0};
        for (int d = lane; d < D; d += OVC_WAVE) {
            const uint64_t key = keys[head[d]];
            int lo = e0, hi = e1;                                // the first entry with entry_key >= key
            while (lo < hi) {
                const int mid = lo + ((hi - lo) >> 1);
                if (c.entry_key[mid] < key) lo = mid + 1; else hi = mid;
            }
            const double rw = (lo < e1 && c.entry_key[lo] == key) ? c.entry_w[lo] : 0.0;
            const double v = fmin(weight[d], rw) * rw;
            const int n = order_of(key);
#pragma unroll
            for (int m = 0; m < kOrders; ++m) val[m] += n == m ? v : 0.0;
        }
        const double delta = len_h - c.ref_length[r];
        const double penalty = exp(-(delta * delta) / (2.0 * c.sigma * c.sigma));
#pragma unroll
        for (int m = 0; m < kOrders; ++m) {
            double v = wave_sum_f64(val[m]);
            const double norm_r = c.ref_norm[(size_t)r * kOrders + m];
            if (norm_h[m] != 0.0 && norm_r != 0.0) v /= norm_h[m] * norm_r;
            score[m] += v * penalty;
        }
    }

    // 5. mean over the orders, over the references, times 10; one rounding to fp32
    if (lane == 0) {
        double s = 0.0;
        if (r1 > r0) s = (((score[0] + score[1]) + score[2]) + score[3]) / (double)kOrders / (double)(r1 - r0) * 10.0;
        out[hyp] = (float)s;
    }
}

}  // namespace

extern "C" int ovc_cider_reward(const ovc_cider* c, const int64_t* ids, const int32_t* rows, int B, int S, int T,
                                float* reward_out, ovc_stream stream) {
    if (!c || !ids || !rows || !reward_out || B < 1 || S < 1 || T < 1 || T > OVC_MAX_LEN) return OVC_EINVAL;
    if (c->vocab < 1 || c->vocab > 65535 || c->n_images < 0 || c->n_refs < 0 || c->hash_size < 0 ||
        (c->hash_size & (c->hash_size - 1)) != 0 || !(c->sigma > 0.0))
        return OVC_EINVAL;
    if (c->hash_size > 0 && (!c->hash_key || !c->hash_idf)) return OVC_EINVAL;
    if (c->n_images > 0 && (!c->image_ref || !c->ref_entry || !c->ref_norm || !c->ref_length)) return OVC_EINVAL;
    if ((long)B * S > 0x7fffffffL / T) return OVC_EINVAL;
    if (const int rc = ovc_device_guard()) return rc;
    const int hyps = B * S;
    const unsigned per_wave = wave_lds_bytes(T);
    int waves = (int)(kMaxLds / per_wave);
    waves = waves > kMaxWaves ? kMaxWaves : waves;               // >= 3: T = 256 needs 21 504 bytes per wave
    hipLaunchKernelGGL(cider_reward_kernel, dim3((unsigned)((hyps + waves - 1) / waves)), dim3(waves * OVC_WAVE), waves * per_wave,
                       ovc_hip_stream(stream), *c, ids, rows, S, T, hyps, waves, reward_out);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}
