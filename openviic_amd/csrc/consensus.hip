// Consensus reranking and diversity statistics of a caption set on the device: the S candidates of an image scored against each
// other from token ids (ovc_caption_set, include/ovc.h).  Pairwise CIDEr-D with the idf of a fixed corpus, the consensus
// (minimum-Bayes-risk) score and pick, and the integer counts of mBLEU and Div-n.  Two launches: one wave per caption writes its
// sorted tf-idf vector to the workspace, then one workgroup per image, one wave per caption, compares siblings by binary search.
// The decode, key, sort and idf routines are copies of cider.hip's (as metrics.hip's are), so that file's code does not change.
#include "common.h"

namespace {

constexpr int kOrders = 4;                      // n-gram orders 1..4
constexpr int kMaxWaves = 4;                    // waves (captions) per workgroup of the vectors launch
constexpr unsigned kMaxLds = 64u * 1024u;       // dynamic LDS a launch may ask for without raising the kernel's attribute

__host__ __device__ inline int next_pow2(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}
// LDS of one wave of the vectors launch: keys [cap] u64 | head [cap] i32 | words [T rounded to even] i32, cap = pow2 >= 4 T
__host__ __device__ inline unsigned wave_lds_bytes(int T) { return (unsigned)next_pow2(4 * T) * 12u + (unsigned)((T + 1) & ~1) * 4u; }

// The workspace: per caption at most E = 4 T distinct n-grams.  keys [N][E] u64 | weight [N][E] f64 | norm [N][4] f64 |
// tf [N][E] i32 | meta [N][4] i32 (L, bigrams, distinct keys D, 0), N = B S
struct set_tables {
    uint64_t* key;
    double* weight;
    double* norm;
    int32_t* tf;
    int32_t* meta;
    int E;
};
inline size_t caption_bytes(int T) { return (size_t)(4 * T) * 20u + 48u; }
inline set_tables carve(void* workspace, int N, int T) {
    set_tables t;
    const size_t E = (size_t)(4 * T), n = (size_t)N;
    unsigned char* p = static_cast<unsigned char*>(workspace);
    t.key = reinterpret_cast<uint64_t*>(p);
    t.weight = reinterpret_cast<double*>(p + n * E * 8);
    t.norm = reinterpret_cast<double*>(p + n * E * 16);
    t.tf = reinterpret_cast<int32_t*>(p + n * E * 16 + n * 32);
    t.meta = reinterpret_cast<int32_t*>(p + n * E * 20 + n * 32);
    t.E = (int)E;
    return t;
}

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

__device__ __forceinline__ int wave_sum_i32(int v) {
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

// ---- launch 1: the tf-idf vector of every caption ---------------------------------------------------------------------------
__global__ __launch_bounds__(kMaxWaves * OVC_WAVE) void caption_vectors_kernel(const ovc_cider c, const int64_t* __restrict__ ids, int T,
                                                                               int hyps, int waves, const set_tables ws) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int lane = threadIdx.x & (OVC_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / OVC_WAVE);
    const int hyp = blockIdx.x * waves + wave;
    if (hyp >= hyps) return;                                     // whole waves leave: there is no workgroup barrier below
    const int cap = next_pow2(4 * T);
    unsigned char* base = lds + (size_t)wave * wave_lds_bytes(T);
    uint64_t* keys = reinterpret_cast<uint64_t*>(base);
    int32_t* head = reinterpret_cast<int32_t*>(base + (size_t)cap * 8);
    int32_t* words = head + cap;
    double* norm_out = ws.norm + (size_t)hyp * kOrders;
    int32_t* meta_out = ws.meta + (size_t)hyp * 4;

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
    if (L == 0) {                                                // the empty caption: no keys, zero norms
        if (lane < kOrders) norm_out[lane] = 0.0;
        if (lane < 4) meta_out[lane] = 0;
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
    D = __builtin_amdgcn_readfirstlane(D);                       // <= total <= 4 T = E
    wave_sync();

    // 3. tf-idf weights and norms; the distinct keys go to the workspace in ascending order
    uint64_t* key_out = ws.key + (size_t)hyp * ws.E;
    double* weight_out = ws.weight + (size_t)hyp * ws.E;
    int32_t* tf_out = ws.tf + (size_t)hyp * ws.E;
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
        key_out[d] = key;
        weight_out[d] = w;
        tf_out[d] = end - start;
        const int n = order_of(key);
#pragma unroll
        for (int m = 0; m < kOrders; ++m) sq[m] += n == m ? w * w : 0.0;
    }
    double norm[kOrders];
#pragma unroll
    for (int m = 0; m < kOrders; ++m) norm[m] = sqrt(wave_sum_f64(sq[m]));
    if (lane == 0) {
#pragma unroll
        for (int m = 0; m < kOrders; ++m) norm_out[m] = norm[m];
        meta_out[0] = L;
        meta_out[1] = L - 1;                                     // the reference's "length": the number of bigrams
        meta_out[2] = D;
        meta_out[3] = 0;
    }
}

// ---- launch 2: every caption against its siblings -----------------------------------------------------------------------------
// LDS of a workgroup: per wave its fp32 score, its four distinct-n-gram counts and its length
struct set_shared {
    float score[OVC_MAX_BEAM];
    int32_t distinct[OVC_MAX_BEAM][kOrders];
    int32_t length[OVC_MAX_BEAM];
};

__global__ __launch_bounds__(OVC_MAX_BEAM * OVC_WAVE) void caption_pairs_kernel(const set_tables ws, int S, double sigma,
                                                                                float* __restrict__ pair_out, float* __restrict__ score_out,
                                                                                int32_t* __restrict__ best_out, int32_t* __restrict__ stats_out,
                                                                                int32_t* __restrict__ image_out) {
    __shared__ set_shared sh;
    const int lane = threadIdx.x & (OVC_WAVE - 1);
    const int i = __builtin_amdgcn_readfirstlane(threadIdx.x / OVC_WAVE);     // blockDim.x == S * 64: every wave has a caption
    const int b = blockIdx.x;
    const size_t first = (size_t)b * S, me = first + i;
    const int E = ws.E;

    const int L = ws.meta[me * 4];
    int D = ws.meta[me * 4 + 2];
    D = D < 0 ? 0 : (D > E ? E : D);
    int Lj[OVC_MAX_BEAM], Dj[OVC_MAX_BEAM];
#pragma unroll
    for (int j = 0; j < OVC_MAX_BEAM; ++j) {
        Lj[j] = j < S ? ws.meta[(first + j) * 4] : 0;
        const int d = j < S ? ws.meta[(first + j) * 4 + 2] : 0;
        Dj[j] = d < 0 ? 0 : (d > E ? E : d);
    }

    // 1. one pass over this caption's distinct keys; each looks itself up in every sibling's sorted entries
    const uint64_t* my_key = ws.key + me * E;
    const double* my_weight = ws.weight + me * E;
    const int32_t* my_tf = ws.tf + me * E;
    double val[OVC_MAX_BEAM][kOrders];
#pragma unroll
    for (int j = 0; j < OVC_MAX_BEAM; ++j)
#pragma unroll
        for (int m = 0; m < kOrders; ++m) val[j][m] = 0.0;
    int correct[kOrders] = {0, 0, 0, 0}, fresh[kOrders] = {0, 0, 0, 0};
    for (int d = lane; d < D; d += OVC_WAVE) {
        const uint64_t key = my_key[d];
        const double w = my_weight[d];
        const int tf = my_tf[d];
        const int n = order_of(key);
        int most = 0;
        bool seen = false;
#pragma unroll
        for (int j = 0; j < OVC_MAX_BEAM; ++j) {
            if (j < S && j != i) {
                const uint64_t* their_key = ws.key + (first + j) * E;
                int lo = 0, hi = Dj[j];                          // the first entry with key >= key
                while (lo < hi) {
                    const int mid = lo + ((hi - lo) >> 1);
                    if (their_key[mid] < key) lo = mid + 1; else hi = mid;
                }
                const bool hit = lo < Dj[j] && their_key[lo] == key;
                const double rw = hit ? ws.weight[(first + j) * E + lo] : 0.0;
                const int rtf = hit ? ws.tf[(first + j) * E + lo] : 0;
                const double v = fmin(w, rw) * rw;
#pragma unroll
                for (int m = 0; m < kOrders; ++m) val[j][m] += n == m ? v : 0.0;
                most = rtf > most ? rtf : most;
                seen = seen || (hit && j < i);
            }
        }
        const int clipped = tf < most ? tf : most;
#pragma unroll
        for (int m = 0; m < kOrders; ++m) {
            correct[m] += n == m ? clipped : 0;
            fresh[m] += (n == m && !seen) ? 1 : 0;
        }
    }
#pragma unroll
    for (int m = 0; m < kOrders; ++m) {
        correct[m] = wave_sum_i32(correct[m]);
        fresh[m] = wave_sum_i32(fresh[m]);
    }

    // 2. CIDEr-D against each sibling as the single reference, and against all of them: the reference scorer's operation order
    double norm_h[kOrders];
#pragma unroll
    for (int m = 0; m < kOrders; ++m) norm_h[m] = ws.norm[me * kOrders + m];
    const double len_h = (double)ws.meta[me * 4 + 1];
    double score[kOrders] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < OVC_MAX_BEAM; ++j) {
        if (j < S) {
            float pair = 0.f;
            if (j != i) {
                const double delta = len_h - (double)ws.meta[(first + j) * 4 + 1];
                const double penalty = exp(-(delta * delta) / (2.0 * sigma * sigma));
                double one[kOrders];
#pragma unroll
                for (int m = 0; m < kOrders; ++m) {
                    double v = wave_sum_f64(val[j][m]);
                    const double norm_r = ws.norm[(first + j) * kOrders + m];
                    if (norm_h[m] != 0.0 && norm_r != 0.0) v /= norm_h[m] * norm_r;
                    one[m] = v * penalty;
                    score[m] += one[m];
                }
                pair = (float)((((one[0] + one[1]) + one[2]) + one[3]) / (double)kOrders / 1.0 * 10.0);
            }
            if (lane == 0) pair_out[me * S + j] = pair;
        }
    }
    float mine = 0.f;
    if (S > 1) mine = (float)((((score[0] + score[1]) + score[2]) + score[3]) / (double)kOrders / (double)(S - 1) * 10.0);

    // 3. the caption's integers: BLEU counts against the siblings; the closest sibling length, a tie going to the shorter
    int reflen = 0, gap = 0x7fffffff;
#pragma unroll
    for (int j = 0; j < OVC_MAX_BEAM; ++j) {
        if (j < S && j != i) {
            const int l = Lj[j];
            const int diff = l > L ? l - L : L - l;
            if (diff < gap || (diff == gap && l < reflen)) { gap = diff; reflen = l; }
        }
    }
    if (lane == 0) {
        score_out[me] = mine;
        int32_t* stats = stats_out + me * OVC_SET_STATS;
#pragma unroll
        for (int m = 0; m < kOrders; ++m) {
            stats[m] = correct[m];
            stats[kOrders + m] = L - m > 0 ? L - m : 0;
        }
        stats[8] = L;
        stats[9] = reflen;
        sh.score[i] = mine;
        sh.length[i] = L;
#pragma unroll
        for (int m = 0; m < kOrders; ++m) sh.distinct[i][m] = fresh[m];
    }
    __syncthreads();                                             // the one meeting of an image's waves

    // 4. the image: the pick and the totals, one lane, ascending over the captions
    if (threadIdx.x == 0) {
        int best = 0, words = 0, empty = 0;
        int distinct[kOrders] = {0, 0, 0, 0}, total[kOrders] = {0, 0, 0, 0};
        for (int s = 0; s < S; ++s) {
            if (sh.score[s] > sh.score[best]) best = s;          // strictly greater: a tie stays with the lower index
            const int l = sh.length[s];
            words += l;
            empty += l == 0 ? 1 : 0;
#pragma unroll
            for (int m = 0; m < kOrders; ++m) {
                distinct[m] += sh.distinct[s][m];
                total[m] += l - m > 0 ? l - m : 0;
            }
        }
        best_out[b] = best;
        int32_t* image = image_out + (size_t)b * OVC_SET_IMAGE;
#pragma unroll
        for (int m = 0; m < kOrders; ++m) {
            image[m] = distinct[m];
            image[kOrders + m] = total[m];
        }
        image[8] = words;
        image[9] = empty;
    }
}

}  // namespace

extern "C" size_t ovc_caption_set_workspace_bytes(int B, int S, int T) {
    if (B < 1 || S < 1 || S > OVC_MAX_BEAM || T < 1 || T > OVC_MAX_LEN) return 0;
    if ((long)B * S > 0x7fffffffL / T) return 0;                 // B S T < 2^31
    return (size_t)B * (size_t)S * caption_bytes(T);
}

extern "C" int ovc_caption_set(const ovc_cider* c, const int64_t* ids, int B, int S, int T, float* pair_out, float* score_out,
                               int32_t* best_out, int32_t* stats_out, int32_t* image_out, void* workspace, size_t workspace_bytes,
                               ovc_stream stream) {
    if (!c || !ids || !pair_out || !score_out || !best_out || !stats_out || !image_out || !workspace) return OVC_EINVAL;
    if (c->vocab < 1 || c->vocab > 65535 || c->hash_size < 0 || (c->hash_size & (c->hash_size - 1)) != 0 || !(c->sigma > 0.0))
        return OVC_EINVAL;
    if (c->hash_size > 0 && (!c->hash_key || !c->hash_idf)) return OVC_EINVAL;
    const size_t need = ovc_caption_set_workspace_bytes(B, S, T);
    if (need == 0 || (reinterpret_cast<uintptr_t>(workspace) & 7u) != 0) return OVC_EINVAL;
    if (workspace_bytes < need) return OVC_EWORKSPACE;
    if (const int rc = ovc_device_guard()) return rc;
    const int hyps = B * S;
    const set_tables ws = carve(workspace, hyps, T);
    const unsigned per_wave = wave_lds_bytes(T);
    int waves = (int)(kMaxLds / per_wave);
    waves = waves > kMaxWaves ? kMaxWaves : waves;               // T = 256 needs 13 312 bytes per wave: 4 waves fit
    hipLaunchKernelGGL(caption_vectors_kernel, dim3((unsigned)((hyps + waves - 1) / waves)), dim3(waves * OVC_WAVE), waves * per_wave,
                       ovc_hip_stream(stream), *c, ids, T, hyps, waves, ws);
    OVC_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(caption_pairs_kernel, dim3((unsigned)B), dim3(S * OVC_WAVE), 0, ovc_hip_stream(stream), ws, S, c->sigma,
                       pair_out, score_out, best_out, stats_out, image_out);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}
