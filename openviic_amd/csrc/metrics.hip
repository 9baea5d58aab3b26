// The evaluation metrics' integer statistics on the device: BLEU-1..4 counts and ROUGE-L LCS lengths of generated captions from
// token ids (ovc_caption_metrics, include/ovc.h; the reference's evaluation/bleu/bleu_scorer.py and evaluation/rouge/rouge.py on
// strings).  One wave per caption, everything in LDS and registers, integers only.
#include "common.h"

namespace {

constexpr int kOrders = 4;                      // n-gram orders 1..4
constexpr int kMaxWaves = 4;                    // waves (captions) per workgroup
constexpr int kWords = OVC_MAX_LEN / OVC_WAVE;  // 64-bit words of the LCS bit vector
constexpr unsigned kMaxLds = 64u * 1024u;       // dynamic LDS a launch may ask for without raising the kernel's attribute

__host__ __device__ inline int next_pow2(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}
// LDS of one wave: keys [cap] u64 | head [cap] i32 | raw [T rounded to even] i32 | words [same] i32, cap = pow2 >= 4 T
__host__ __device__ inline unsigned wave_lds_bytes(int T) { return (unsigned)next_pow2(4 * T) * 12u + (unsigned)((T + 1) & ~1) * 8u; }

// LDS written by some lanes of the wave and read by others: the wave runs in lockstep and its LDS operations complete in order;
// the fences keep the compiler from moving an access across the point
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ int order_of(uint64_t key) {          // 0-based n-gram order: the highest non-empty 16-bit field
    return (key >> 48) ? 3 : (key >> 32) ? 2 : (key >> 16) ? 1 : 0;
}

__global__ __launch_bounds__(kMaxWaves * OVC_WAVE) void caption_metrics_kernel(const ovc_eval_corpus c, const int64_t* __restrict__ ids,
                                                                               const int32_t* __restrict__ rows, int T, int B, int waves,
                                                                               int64_t* __restrict__ clean_out, int32_t* __restrict__ stats_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int lane = threadIdx.x & (OVC_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / OVC_WAVE);
    const int hyp = blockIdx.x * waves + wave;
    if (hyp >= B) return;                                        // whole waves leave: there is no workgroup barrier below
    const int cap = next_pow2(4 * T);
    const int t_even = (T + 1) & ~1;
    unsigned char* base = lds + (size_t)wave * wave_lds_bytes(T);
    uint64_t* keys = reinterpret_cast<uint64_t*>(base);
    int32_t* head = reinterpret_cast<int32_t*>(base + (size_t)cap * 8);
    int32_t* raw = head + cap;
    int32_t* words = raw + t_even;
    const uint64_t below = (1ull << lane) - 1ull;

    // 1. clean: clamp, cut at the first <eos>, drop the specials, THEN collapse consecutive equal words
    const int64_t* tok = ids + (size_t)hyp * T;
    int Lr = 0;
    for (int t0 = 0; t0 < T; t0 += OVC_WAVE) {
        const int t = t0 + lane;
        int64_t w = t < T ? tok[t] : (int64_t)c.pad_idx;
        w = w < 0 ? 0 : (w >= c.vocab ? c.vocab - 1 : w);
        const uint64_t ends = __ballot(t < T && w == c.eos_idx);
        const bool live = t < T && (ends == 0 || lane <= __ffsll((unsigned long long)ends) - 1);
        const bool keep = live && w != c.pad_idx && w != c.bos_idx && w != c.eos_idx && w != c.unk_idx;
        const uint64_t kept = __ballot(keep);
        if (keep) raw[Lr + __popcll(kept & below)] = (int32_t)w;
        Lr += __popcll(kept);
        if (ends) break;
    }
    Lr = __builtin_amdgcn_readfirstlane(Lr);
    wave_sync();
    int L = 0;
    for (int i0 = 0; i0 < Lr; i0 += OVC_WAVE) {
        const int i = i0 + lane;
        const bool keep = i < Lr && (i == 0 || raw[i] != raw[i - 1]);
        const uint64_t kept = __ballot(keep);
        if (keep) words[L + __popcll(kept & below)] = raw[i];
        L += __popcll(kept);
    }
    L = __builtin_amdgcn_readfirstlane(L);
    wave_sync();
    int64_t* clean = clean_out + (size_t)hyp * T;
    for (int t = lane; t < T; t += OVC_WAVE) clean[t] = t < L ? (int64_t)words[t] : (t == L ? (int64_t)c.eos_idx : (int64_t)c.pad_idx);

    int row = rows[hyp];
    row = row < 0 ? 0 : (row >= c.n_images ? c.n_images - 1 : row);
    int r0 = 0, r1 = 0, g0 = 0, g1 = 0;
    if (c.n_images > 0) { r0 = c.image_ref[row]; r1 = c.image_ref[row + 1]; g0 = c.image_gram[row]; g1 = c.image_gram[row + 1]; }
    else row = 0;
    const int stride = OVC_METRIC_STATS + c.max_refs;
    int32_t* stats = stats_out + (size_t)hyp * stride;

    // 2. BLEU: the sorted keys of all n-grams, distinct keys with their counts, clipped by the image's maximum counts
    int correct[kOrders] = {0, 0, 0, 0};
    if (L > 0) {
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
        const int P = next_pow2(total);                          // <= cap: total <= 4 L <= 4 T
        for (int i = total + lane; i < P; i += OVC_WAVE) keys[i] = ~0ull;
        wave_sync();
        for (int k = 2; k <= P; k <<= 1) {                       // bitonic sort, ascending
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
        for (int d = lane; d < D; d += OVC_WAVE) {
            const int start = head[d], end = d + 1 < D ? head[d + 1] : total;
            const uint64_t key = keys[start];
            int lo = g0, hi = g1;                                // the first entry with gram_key >= key
            while (lo < hi) {
                const int mid = lo + ((hi - lo) >> 1);
                if (c.gram_key[mid] < key) lo = mid + 1; else hi = mid;
            }
            const int most = (lo < g1 && c.gram_key[lo] == key) ? c.gram_max[lo] : 0;
            const int hit = end - start < most ? end - start : most;
            const int n = order_of(key);
#pragma unroll
            for (int m = 0; m < kOrders; ++m) correct[m] += n == m ? hit : 0;
        }
#pragma unroll
        for (int m = 0; m < kOrders; ++m) correct[m] = wave_sum_i32(correct[m]);
    }

    // 3. the closest reference length: min((abs(l - testlen), l)), so a tie goes to the shorter
    int reflen = 0, best = 0x7fffffff;
    for (int r = r0; r < r1; ++r) {
        const int l = c.ref_words[r];
        const int diff = l > L ? l - L : L - l;
        if (diff < best || (diff == best && l < reflen)) { best = diff; reflen = l; }
    }

    // 4. ROUGE-L: the bit-parallel LCS against every reference.  Lane j of word w holds caption token 64 w + j; the empty
    //    caption is the one EMPTY token
    const int Lh = L > 0 ? L : 1;
    const int nw = (Lh + OVC_WAVE - 1) / OVC_WAVE;
    uint32_t mine[kWords];
#pragma unroll
    for (int w = 0; w < kWords; ++w) {
        const int j = w * OVC_WAVE + lane;
        mine[w] = j < L ? (uint32_t)(words[j] + 1) : 0xffffffffu;         // no 16-bit code equals it
    }
    if (L == 0 && lane == 0) mine[0] = (uint32_t)(c.pad_idx + 1);
    for (int r = r0; r < r1; ++r) {
        const int k = r - r0;
        if (k >= c.max_refs) break;
        const int q0 = c.ref_token[r], q1 = c.ref_token[r + 1];
        uint64_t V[kWords];
#pragma unroll
        for (int w = 0; w < kWords; ++w) V[w] = ~0ull;
        for (int q = q0; q < q1; q += OVC_WAVE) {
            const int left = q1 - q < OVC_WAVE ? q1 - q : OVC_WAVE;
            const uint32_t loaded = lane < left ? (uint32_t)c.token_code[q + lane] : 0u;
            for (int i = 0; i < left; ++i) {
                const uint32_t code = (uint32_t)__shfl((int)loaded, i, OVC_WAVE);
                uint64_t carry = 0;
#pragma unroll
                for (int w = 0; w < kWords; ++w) {
                    if (w < nw) {
                        const uint64_t M = __ballot(mine[w] == code);
                        const uint64_t U = V[w] & M;
                        const uint64_t s1 = V[w] + U;
                        const uint64_t s2 = s1 + carry;
                        carry = (uint64_t)(s1 < U) | (uint64_t)(s2 < s1);
                        V[w] = s2 | (V[w] & ~M);
                    }
                }
            }
        }
        int lcs = 0;
#pragma unroll
        for (int w = 0; w < kWords; ++w) {
            if (w < nw) {
                const int bits = Lh - w * OVC_WAVE;
                const uint64_t low = bits >= OVC_WAVE ? ~0ull : ((1ull << bits) - 1ull);
                lcs += __popcll(~V[w] & low);
            }
        }
        if (lane == 0) stats[OVC_METRIC_STATS + k] = lcs;
    }
    for (int k = r1 - r0 + lane; k < c.max_refs; k += OVC_WAVE) stats[OVC_METRIC_STATS + k] = -1;

    if (lane == 0) {
#pragma unroll
        for (int m = 0; m < kOrders; ++m) {
            stats[m] = correct[m];
            stats[kOrders + m] = L - m > 0 ? L - m : 0;
        }
        stats[8] = L;
        stats[9] = reflen;
        stats[10] = Lh;
        stats[11] = row;
    }
}

}  // namespace

extern "C" size_t ovc_caption_metrics_bytes(int B, int T, int max_refs) {
    if (B < 1 || T < 1 || T > OVC_MAX_LEN || max_refs < 0 || max_refs > OVC_METRIC_MAX_REFS) return 0;
    if ((long)B > 0x7fffffffL / T || (long)B > 0x7fffffffL / (OVC_METRIC_STATS + max_refs)) return 0;
    return (size_t)B * (size_t)(OVC_METRIC_STATS + max_refs) * sizeof(int32_t);
}

extern "C" int ovc_caption_metrics(const ovc_eval_corpus* c, const int64_t* ids, const int32_t* rows, int B, int T, int64_t* clean_out,
                                   int32_t* stats_out, size_t stats_bytes, ovc_stream stream) {
    if (!c || !ids || !rows || !clean_out || !stats_out) return OVC_EINVAL;
    if (c->vocab < 1 || c->vocab > 65535 || c->n_images < 0 || c->n_refs < 0) return OVC_EINVAL;
    const size_t need = ovc_caption_metrics_bytes(B, T, c->max_refs);
    if (need == 0) return OVC_EINVAL;
    if (c->n_images > 0 && (!c->image_ref || !c->image_gram || !c->ref_token)) return OVC_EINVAL;
    if (c->n_refs > 0 && !c->ref_words) return OVC_EINVAL;
    if (stats_bytes < need) return OVC_EWORKSPACE;
    if (const int rc = ovc_device_guard()) return rc;
    const unsigned per_wave = wave_lds_bytes(T);
    int waves = (int)(kMaxLds / per_wave);
    waves = waves > kMaxWaves ? kMaxWaves : waves;               // T = 256 needs 14 336 bytes per wave: 4 waves fit
    hipLaunchKernelGGL(caption_metrics_kernel, dim3((unsigned)((B + waves - 1) / waves)), dim3(waves * OVC_WAVE), waves * per_wave,
                       ovc_hip_stream(stream), *c, ids, rows, T, B, waves, clean_out, stats_out);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}
