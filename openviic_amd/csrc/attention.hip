// Attention kernels.
//
//  attention_mfma_kernel   general scaled-dot-product attention on projected heads, used by the
//                          encoder (nq = nk = regions, optional geometry bias / memory slots), the
//                          teacher-forced decoder and the DLCT-style cross form (nq != nk, per-query
//                          mask).  Q.K^T and P.V run on the matrix cores (v_mfma_f32_32x32x2_f32),
//                          the softmax row reduce on wavefront shuffles.
//  decode_self_attention   one query row per beam against its own history through the ancestor
//                          table (no cache re-ordering), nq = 1.
//  decode_cross_attention  the k beams of one image share that image's projected encoder K/V: one wave per
//                          (image, head), everything in registers, both contractions on v_mfma_f32_16x16x4_f32
//                          (d_k in {16, 32, 64}); head sizes 4 and 8 take an LDS-staged VALU kernel.
//
// Reference call sites: models/modules/attentions.py:51-55, :102-111, :171-183.
#include <cstdlib>
#include <mutex>

#include "common.h"

namespace {

constexpr int kQTile = 64;        // query rows per workgroup
constexpr int kLdQK = 68;         // LDS row stride (floats) of the Q / K / V images: 64 + 4
                                  // (68 r mod 64 = 4 r: conflict-free ds_read_b128 per lane group)

struct AttnArgs {
    const float* q; const float* k; const float* v; float* out;
    int b, nq, nk, h, dk, dv;
    const uint8_t* mask; long mask_sb, mask_sq;
    const float* geometry;
    const float* mem_k; const float* mem_v; int m; float mem_scale_k, mem_scale_v;
    int nkp;                       // nk + m rounded up to a multiple of 32
    int qtiles;
};

__global__ __launch_bounds__(256) void attention_mfma_kernel(AttnArgs p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int qt = blockIdx.x % p.qtiles;
    const int hd = (blockIdx.x / p.qtiles) % p.h;
    const int b = blockIdx.x / (p.qtiles * p.h);
    const int q0 = qt * kQTile;
    const int nkt = p.nk + p.m;            // real keys + memory slots
    const int lds_s = p.nkp + 4;           // row stride of the score / probability image

    float* Qs = lds;                       // [64][68]
    float* Ks = Qs + kQTile * kLdQK;       // [nkp][68]
    float* Vs = Ks + p.nkp * kLdQK;        // [nkp][68]
    float* Ss = Vs + p.nkp * kLdQK;        // [64][nkp+4]

    // ---- stage Q, K, V (zero-filled outside the valid region) -------------------------------
    {
        const int c4 = tid & 15, r0 = tid >> 4;           // 16 float4 per 64-wide row, 16 rows per pass
        const int col = c4 * 4;
        for (int r = r0; r < kQTile; r += 16) {
            f32x4 val = {0.f, 0.f, 0.f, 0.f};
            if (q0 + r < p.nq && col < p.dk)
                val = *reinterpret_cast<const f32x4*>(p.q + ((size_t)b * p.nq + q0 + r) * (p.h * p.dk) + hd * p.dk + col);
            *reinterpret_cast<f32x4*>(Qs + r * kLdQK + col) = val;
        }
        for (int r = r0; r < p.nkp; r += 16) {
            f32x4 kv = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
            if (r < p.nk) {
                if (col < p.dk) kv = *reinterpret_cast<const f32x4*>(p.k + ((size_t)b * p.nk + r) * (p.h * p.dk) + hd * p.dk + col);
                if (col < p.dv) vv = *reinterpret_cast<const f32x4*>(p.v + ((size_t)b * p.nk + r) * (p.h * p.dv) + hd * p.dv + col);
            } else if (r < nkt) {
                const int mr = r - p.nk;
                if (col < p.dk) kv = *reinterpret_cast<const f32x4*>(p.mem_k + (size_t)mr * (p.h * p.dk) + hd * p.dk + col) * p.mem_scale_k;
                if (col < p.dv) vv = *reinterpret_cast<const f32x4*>(p.mem_v + (size_t)mr * (p.h * p.dv) + hd * p.dv + col) * p.mem_scale_v;
            }
            *reinterpret_cast<f32x4*>(Ks + r * kLdQK + col) = kv;
            *reinterpret_cast<f32x4*>(Vs + r * kLdQK + col) = vv;
        }
    }
    __syncthreads();

    const int frow = lane & 31, half = lane >> 5;
    // ---- S = Q K^T / sqrt(dk), masked, geometry-biased -> LDS ----------------------------------
    {
        const int ktiles = p.nkp >> 5;
        const int ksteps = (p.dk + 7) >> 3;
        const float inv_scale = sqrtf((float)p.dk);
        for (int tile = wave; tile < 2 * ktiles; tile += 4) {
            const int tq = tile / ktiles, tk = tile - tq * ktiles;
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            const float* ap = Qs + (tq * 32 + frow) * kLdQK + half * 4;
            const float* bp = Ks + (tk * 32 + frow) * kLdQK + half * 4;
            for (int kk = 0; kk < ksteps; ++kk) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(ap + kk * 8);
                const f32x4 bb = *reinterpret_cast<const f32x4*>(bp + kk * 8);
#pragma unroll
                for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], bb[s], acc, 0, 0, 0);
            }
            const int kj = tk * 32 + frow;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qi = tq * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                const int gq = q0 + qi;
                float s = acc[r] / inv_scale;
                if (kj >= nkt) {
                    s = -INFINITY;
                } else if (kj < p.nk && gq < p.nq) {
                    if (p.mask && p.mask[(size_t)b * p.mask_sb + (size_t)gq * p.mask_sq + kj]) s = -INFINITY;
                    if (p.geometry)
                        s = logf(fmaxf(p.geometry[(((size_t)b * p.h + hd) * p.nq + gq) * p.nk + kj], 1e-6f)) + s;
                }
                Ss[qi * lds_s + kj] = s;
            }
        }
    }
    __syncthreads();

    // ---- row softmax: 4 lanes per row, wavefront-shuffle reduce ------------------------------------
    {
        const int row = tid >> 2, part = tid & 3;
        float* srow = Ss + row * lds_s;
        float mx = -INFINITY;
        for (int j = part; j < p.nkp; j += 4) mx = fmaxf(mx, srow[j]);
        mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
        float sum = 0.f;
        for (int j = part; j < p.nkp; j += 4) {
            const float e = expf(srow[j] - mx);
            srow[j] = e;
            sum += e;
        }
        sum += __shfl_xor(sum, 1, 64);
        sum += __shfl_xor(sum, 2, 64);
        for (int j = part; j < p.nkp; j += 4) srow[j] = srow[j] / sum;
    }
    __syncthreads();

    // ---- O = P V ------------------------------------------------------------------------------------------
    {
        const int vtiles = (p.dv + 31) >> 5;
        const int ksteps = p.nkp >> 3;
        for (int tile = wave; tile < 2 * vtiles; tile += 4) {
            const int tq = tile / vtiles, tn = tile - tq * vtiles;
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            const float* ap = Ss + (tq * 32 + frow) * lds_s + half * 4;
            const float* bp = Vs + (half * 4) * kLdQK + tn * 32 + frow;
            for (int kk = 0; kk < ksteps; ++kk) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(ap + kk * 8);
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], bp[(kk * 8 + s) * kLdQK], acc, 0, 0, 0);
            }
            const int col = tn * 32 + frow;
            if (col < p.dv) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int gq = q0 + tq * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    if (gq < p.nq) p.out[((size_t)b * p.nq + gq) * (p.h * p.dv) + hd * p.dv + col] = acc[r];
                }
            }
        }
    }
}


// -------------------------------------------------------------------------------------------------
// attention_regs_kernel: the same operator with the scores kept in accumulator registers.
//
// One workgroup per (image, head); wave w owns queries 32 w .. 32 w + 31 and ALL keys.  K and V of the (image,
// head) go to LDS once with fully coalesced 256-byte row reads and are shared by the waves; each wave's Q fragment
// comes straight from global memory into registers.
//   S^T[key][q] = K Q^T  (v_mfma_f32_32x32x2_f32, A = K rows from LDS, B = Q rows): the accumulator of key tile tk
//       has the QUERY on the lane (q = lane & 31) and 16 keys on its registers (key = 32 tk + (r&3) + 8 (r>>2) +
//       4 (lane>>5)), so scale, mask, geometry bias and the softmax over keys are register arithmetic plus ONE
//       __shfl_xor(32) per reduction -- no score image in LDS, no scalar LDS stores (the general kernel above
//       spends most of its time there: 0.13 of the MFMA peak).
//   O^T[dv][q] = V^T P^T: the probabilities are used where they are, as the B operand: MFMA step (tk, r) contracts
//       over the two keys base_r and base_r + 4 that the two lane halves hold in register r; the A operand
//       V[key][dv = lane & 31] is a conflict-free 128-byte ds_read_b32 per half.
//   The output tile goes through LDS once (the K image is free by then) so that rows leave as whole 256-byte lines.
// NKT = key tiles of 32 (real keys + memory slots, <= 6); KG = 8-deep d groups of Q.K (dk <= 8 KG);
// DVT = 32-wide tiles of d_v.  Numerics: scores and probabilities as in the general kernel (same scale, mask,
// geometry order, expf, division); only the order of the softmax sum and of the P.V sum over keys differs.
// -------------------------------------------------------------------------------------------------
template <int NKT, int KG, int DVT>
__global__ __launch_bounds__(256) void attention_regs_kernel(AttnArgs p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hd = blockIdx.x % p.h, b = blockIdx.x / p.h;
    const int nkt = p.nk + p.m;
    constexpr int kRows = NKT * 32;
    const int k_rows = max(kRows, ((p.nq + 31) >> 5) * 32);           // the K image doubles as the output staging area
    float* Ks = lds;                          // [k_rows][68]
    float* Vs = Ks + k_rows * kLdQK;          // [kRows][68]

    // ---- K, V -> LDS (zero-filled outside the valid region), Q fragment -> registers ------------------------------
    // All 256 threads stage (waves beyond the query tiles only help here), and all of a thread's global loads are
    // issued before the first LDS store: a load -> store loop would pay one memory round trip per pass.
    {
        const int c4 = tid & 15, col = c4 * 4, r0 = tid >> 4;
        constexpr int kPasses = kRows / 16;
        f32x4 kv[kPasses], vv[kPasses];
#pragma unroll
        for (int i = 0; i < kPasses; ++i) {
            const int r = r0 + 16 * i;
            const bool real = r < p.nk, slot = !real && r < nkt;
            const int mr = min(max(r - p.nk, 0), max(p.m - 1, 0));
            // one address per matrix, always valid: a real key row, a memory slot, or (padding) row 0 -- zeroed below
            const float* ks = slot ? p.mem_k + (size_t)mr * (p.h * p.dk) + hd * p.dk
                                   : p.k + ((size_t)b * p.nk + (real ? r : 0)) * (p.h * p.dk) + hd * p.dk;
            const float* vs = slot ? p.mem_v + (size_t)mr * (p.h * p.dv) + hd * p.dv
                                   : p.v + ((size_t)b * p.nk + (real ? r : 0)) * (p.h * p.dv) + hd * p.dv;
            kv[i] = *reinterpret_cast<const f32x4*>(ks + min(col, p.dk - 4));
            vv[i] = *reinterpret_cast<const f32x4*>(vs + min(col, p.dv - 4));
        }
#pragma unroll
        for (int i = 0; i < kPasses; ++i) {
            const int r = r0 + 16 * i;
            const bool real = r < p.nk, slot = !real && r < nkt;
            f32x4 kx = kv[i], vx = vv[i];
            if (slot) { kx = kx * p.mem_scale_k; vx = vx * p.mem_scale_v; }
            if ((!real && !slot) || col >= p.dk) kx = f32x4{0.f, 0.f, 0.f, 0.f};
            if ((!real && !slot) || col >= p.dv) vx = f32x4{0.f, 0.f, 0.f, 0.f};
            *reinterpret_cast<f32x4*>(Ks + r * kLdQK + col) = kx;
            *reinterpret_cast<f32x4*>(Vs + r * kLdQK + col) = vx;
        }
    }
    const int qwaves = (p.nq + 31) >> 5;                        // waves that own queries; the others only staged
    const int qi = lane & 31, half = lane >> 5;
    const int gq = wave * 32 + qi;                              // this lane's query
    const bool q_ok = gq < p.nq;
    f32x4 qf[KG];
    {
        const float* qrow = p.q + ((size_t)b * p.nq + min(gq, p.nq - 1)) * (p.h * p.dk) + hd * p.dk;
#pragma unroll
        for (int kk = 0; kk < KG; ++kk) {
            const int d = 8 * kk + 4 * half;
            qf[kk] = *reinterpret_cast<const f32x4*>(qrow + min(d, p.dk - 4));
            if (!q_ok || d >= p.dk) qf[kk] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    __syncthreads();

    // ---- S^T = K Q^T ---------------------------------------------------------------------------------------------------
    f32x16 st[NKT];
#pragma unroll
    for (int tk = 0; tk < NKT; ++tk)
#pragma unroll
        for (int r = 0; r < 16; ++r) st[tk][r] = 0.f;
    if (wave < qwaves) {
#pragma unroll
    for (int kk = 0; kk < KG; ++kk) {
        f32x4 kf[NKT];
#pragma unroll
        for (int tk = 0; tk < NKT; ++tk) kf[tk] = *reinterpret_cast<const f32x4*>(Ks + (tk * 32 + qi) * kLdQK + 8 * kk + 4 * half);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int tk = 0; tk < NKT; ++tk) st[tk] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[tk][s], qf[kk][s], st[tk], 0, 0, 0);
    }
    }
    __syncthreads();                                            // every wave is done with the K image
    if (wave >= qwaves) return;

    // ---- scale, mask, geometry bias; softmax over the keys of this lane's query -------------------------------------------
    const float inv_scale = sqrtf((float)p.dk);
    const uint8_t* mrow = p.mask ? p.mask + (size_t)b * p.mask_sb + (size_t)min(gq, p.nq - 1) * p.mask_sq : nullptr;
    const float* grow = p.geometry ? p.geometry + (((size_t)b * p.h + hd) * p.nq + min(gq, p.nq - 1)) * p.nk : nullptr;
    float mx = -INFINITY;
#pragma unroll
    for (int tk = 0; tk < NKT; ++tk)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int kj = tk * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            float s = st[tk][r] / inv_scale;
            if (kj >= nkt) {
                s = -INFINITY;
            } else if (kj < p.nk) {
                if (mrow && mrow[kj]) s = -INFINITY;
                if (grow) s = logf(fmaxf(grow[kj], 1e-6f)) + s;
            }
            st[tk][r] = s;
            mx = fmaxf(mx, s);
        }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float sum = 0.f;
#pragma unroll
    for (int tk = 0; tk < NKT; ++tk)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float e = expf(st[tk][r] - mx);
            st[tk][r] = e;
            sum += e;
        }
    sum += __shfl_xor(sum, 32, 64);
#pragma unroll
    for (int tk = 0; tk < NKT; ++tk)
#pragma unroll
        for (int r = 0; r < 16; ++r) st[tk][r] = st[tk][r] / sum;

    // ---- O^T = V^T P^T ---------------------------------------------------------------------------------------------------
    f32x16 ot[DVT];
#pragma unroll
    for (int t = 0; t < DVT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) ot[t][r] = 0.f;
#pragma unroll
    for (int tk = 0; tk < NKT; ++tk)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float* vrow = Vs + (tk * 32 + (r & 3) + 8 * (r >> 2) + 4 * half) * kLdQK + qi;     // this half's key of step (tk, r)
#pragma unroll
            for (int t = 0; t < DVT; ++t) ot[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(vrow[t * 32], st[tk][r], ot[t], 0, 0, 0);
        }

    // ---- output: accumulator (dv on registers, query on the lane) -> LDS [query][dv] -> whole rows to memory ---------------
    float* Os = Ks + wave * 32 * kLdQK;
#pragma unroll
    for (int t = 0; t < DVT; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            *reinterpret_cast<f32x4*>(Os + qi * kLdQK + t * 32 + 8 * j + 4 * half) =
                f32x4{ot[t][4 * j], ot[t][4 * j + 1], ot[t][4 * j + 2], ot[t][4 * j + 3]};
    // (each wave reads back only what it wrote itself: no workgroup barrier, the compiler's lgkmcnt wait orders it)
    {
        const int c4 = lane & 15, col = c4 * 4;
#pragma unroll
        for (int pass = 0; pass < 8; ++pass) {
            const int row = pass * 4 + (lane >> 4);
            const int oq = wave * 32 + row;
            if (oq < p.nq && col < p.dv)
                *reinterpret_cast<f32x4*>(p.out + ((size_t)b * p.nq + oq) * (p.h * p.dv) + hd * p.dv + col) =
                    *reinterpret_cast<const f32x4*>(Os + row * kLdQK + col);
        }
    }
}

// -------------------------------------------------------------------------------------------------
// attention_tiled_kernel: the same operator without a limit on the number of keys or queries (round 4; shapes beyond the
// register instances: more than 192 keys, or more than 128 keys for more than 128 queries).  The reference has
// none (attentions.py:44-58 works on any nk, :158-185 appends its 40 memory slots to any nk): bottom-up feature sets carry up
// to 100 regions per image (+ 40 slots = 140 keys), grid features 14 x 14 = 196 cells, the DLCT form regions + cells.
//
// One workgroup per (image, head, 128 queries), a wave per 32 queries -- the register layout of attention_regs_kernel
// (S^T = K Q^T with the query on the lane, O^T = V^T P^T with the probabilities as the B operand) -- but the keys pass
// through LDS in tiles of 128, in ascending order, under an online softmax: per query a running maximum M and a running sum
// L of exp(s - M); a tile whose maximum raises M rescales L and the output accumulators by exp(M_old - M_new), which is a
// per-lane scalar here because a lane's accumulator registers all belong to ITS query.  The tile order is fixed, so a result
// depends on nothing but the operands (no timing, no batch size).  Fully masked rows end with L = 0 and give 0 / 0 = NaN,
// as the reference's softmax over a row of -inf does.  Numerics vs the kernels above: the division by the softmax sum
// happens once at the end instead of per probability (~1 ulp per output); shapes with nk + m <= 192 and nq <= 128 never come
// here (they have register instances), so nothing that ran before round 4 changes a bit.
// KG = 8-deep d groups of Q.K (dk <= 8 KG); DVT = 32-wide tiles of d_v.
// -------------------------------------------------------------------------------------------------
template <int KG, int DVT>
__global__ __launch_bounds__(256) void attention_tiled_kernel(AttnArgs p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int NKT = 4, kRows = NKT * 32;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int qt = blockIdx.x % p.qtiles;
    const int hd = (blockIdx.x / p.qtiles) % p.h;
    const int b = blockIdx.x / (p.qtiles * p.h);
    const int nkt = p.nk + p.m;
    float* Ks = lds;                          // [128][68]; doubles as the output staging area at the end
    float* Vs = Ks + kRows * kLdQK;           // [128][68]

    const int qi = lane & 31, half = lane >> 5;
    const int gq = qt * kRows + wave * 32 + qi;                 // this lane's query
    const bool q_ok = gq < p.nq;
    const bool wave_live = qt * kRows + wave * 32 < p.nq;       // wave-uniform: waves past the last query only stage
    f32x4 qf[KG];
    {
        const float* qrow = p.q + ((size_t)b * p.nq + min(gq, p.nq - 1)) * (p.h * p.dk) + hd * p.dk;
#pragma unroll
        for (int kk = 0; kk < KG; ++kk) {
            const int d = 8 * kk + 4 * half;
            qf[kk] = *reinterpret_cast<const f32x4*>(qrow + min(d, p.dk - 4));
            if (!q_ok || d >= p.dk) qf[kk] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    const float inv_scale = sqrtf((float)p.dk);
    const uint8_t* mrow = p.mask ? p.mask + (size_t)b * p.mask_sb + (size_t)min(gq, p.nq - 1) * p.mask_sq : nullptr;
    const float* grow = p.geometry ? p.geometry + (((size_t)b * p.h + hd) * p.nq + min(gq, p.nq - 1)) * p.nk : nullptr;

    float m_run = -INFINITY, l_run = 0.f;
    f32x16 ot[DVT];
#pragma unroll
    for (int t = 0; t < DVT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) ot[t][r] = 0.f;

    for (int k0 = 0; k0 < nkt; k0 += kRows) {
        // ---- this tile's K, V rows -> LDS (zero-filled past the last key); every load issued before the first LDS store ------
        {
            const int c4 = tid & 15, col = c4 * 4, r0 = tid >> 4;
            constexpr int kPasses = kRows / 16;
            f32x4 kv[kPasses], vv[kPasses];
#pragma unroll
            for (int i = 0; i < kPasses; ++i) {
                const int kr = k0 + r0 + 16 * i;
                const bool real = kr < p.nk, slot = !real && kr < nkt;
                const int mr = min(max(kr - p.nk, 0), max(p.m - 1, 0));
                const float* ks = slot ? p.mem_k + (size_t)mr * (p.h * p.dk) + hd * p.dk
                                       : p.k + ((size_t)b * p.nk + (real ? kr : 0)) * (p.h * p.dk) + hd * p.dk;
                const float* vs = slot ? p.mem_v + (size_t)mr * (p.h * p.dv) + hd * p.dv
                                       : p.v + ((size_t)b * p.nk + (real ? kr : 0)) * (p.h * p.dv) + hd * p.dv;
                kv[i] = *reinterpret_cast<const f32x4*>(ks + min(col, p.dk - 4));
                vv[i] = *reinterpret_cast<const f32x4*>(vs + min(col, p.dv - 4));
            }
#pragma unroll
            for (int i = 0; i < kPasses; ++i) {
                const int r = r0 + 16 * i, kr = k0 + r;
                const bool real = kr < p.nk, slot = !real && kr < nkt;
                f32x4 kx = kv[i], vx = vv[i];
                if (slot) { kx = kx * p.mem_scale_k; vx = vx * p.mem_scale_v; }
                if ((!real && !slot) || col >= p.dk) kx = f32x4{0.f, 0.f, 0.f, 0.f};
                if ((!real && !slot) || col >= p.dv) vx = f32x4{0.f, 0.f, 0.f, 0.f};
                *reinterpret_cast<f32x4*>(Ks + r * kLdQK + col) = kx;
                *reinterpret_cast<f32x4*>(Vs + r * kLdQK + col) = vx;
            }
        }
        __syncthreads();

        if (wave_live) {
            // ---- S^T = K Q^T for the tile's 128 keys ---------------------------------------------------------------------------
            f32x16 st[NKT];
#pragma unroll
            for (int tk = 0; tk < NKT; ++tk)
#pragma unroll
                for (int r = 0; r < 16; ++r) st[tk][r] = 0.f;
#pragma unroll
            for (int kk = 0; kk < KG; ++kk) {
                f32x4 kf[NKT];
#pragma unroll
                for (int tk = 0; tk < NKT; ++tk) kf[tk] = *reinterpret_cast<const f32x4*>(Ks + (tk * 32 + qi) * kLdQK + 8 * kk + 4 * half);
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int tk = 0; tk < NKT; ++tk) st[tk] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[tk][s], qf[kk][s], st[tk], 0, 0, 0);
            }
            // ---- scale, mask, geometry bias; the tile's maximum for this lane's query ----------------------------------------
            float mx = -INFINITY;
#pragma unroll
            for (int tk = 0; tk < NKT; ++tk)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int kj = k0 + tk * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    float s = st[tk][r] / inv_scale;
                    if (kj >= nkt) {
                        s = -INFINITY;
                    } else if (kj < p.nk) {
                        if (mrow && mrow[kj]) s = -INFINITY;
                        if (grow) s = logf(fmaxf(grow[kj], 1e-6f)) + s;
                    }
                    st[tk][r] = s;
                    mx = fmaxf(mx, s);
                }
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float m_new = fmaxf(m_run, mx);
            const bool none = m_new == -INFINITY;                    // every key so far masked: nothing to add, nothing to rescale
            const float alpha = none ? 1.f : expf(m_run - m_new);    // m_run = -inf, m_new finite: 0 (L and O are 0 anyway)
            float sum = 0.f;
#pragma unroll
            for (int tk = 0; tk < NKT; ++tk)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float e = none ? 0.f : expf(st[tk][r] - m_new);
                    st[tk][r] = e;
                    sum += e;
                }
            sum += __shfl_xor(sum, 32, 64);
            l_run = l_run * alpha + sum;
            m_run = m_new;
#pragma unroll
            for (int t = 0; t < DVT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) ot[t][r] *= alpha;
            // ---- O^T += V^T E^T -------------------------------------------------------------------------------------------------
#pragma unroll
            for (int tk = 0; tk < NKT; ++tk)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float* vrow = Vs + (tk * 32 + (r & 3) + 8 * (r >> 2) + 4 * half) * kLdQK + qi;
#pragma unroll
                    for (int t = 0; t < DVT; ++t) ot[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(vrow[t * 32], st[tk][r], ot[t], 0, 0, 0);
                }
        }
        __syncthreads();                                             // every wave is done with this tile's images
    }
    if (!wave_live) return;

    // ---- normalise; accumulator (dv on registers, query on the lane) -> LDS [query][dv] -> whole rows to memory -----------------
    float* Os = Ks + wave * 32 * kLdQK;
#pragma unroll
    for (int t = 0; t < DVT; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            *reinterpret_cast<f32x4*>(Os + qi * kLdQK + t * 32 + 8 * j + 4 * half) =
                f32x4{ot[t][4 * j] / l_run, ot[t][4 * j + 1] / l_run, ot[t][4 * j + 2] / l_run, ot[t][4 * j + 3] / l_run};
    {
        const int c4 = lane & 15, col = c4 * 4;
#pragma unroll
        for (int pass = 0; pass < 8; ++pass) {
            const int row = pass * 4 + (lane >> 4);
            const int oq = qt * kRows + wave * 32 + row;
            if (oq < p.nq && col < p.dv)
                *reinterpret_cast<f32x4*>(p.out + ((size_t)b * p.nq + oq) * (p.h * p.dv) + hd * p.dv + col) =
                    *reinterpret_cast<const f32x4*>(Os + row * kLdQK + col);
        }
    }
}

}  // namespace

// ---- which instance an ovc_attention launch takes ------------------------------------------------------------------------------
// ONE selection function for the launcher below and for the form query of the test hook (ovc_debug_attention_form): the choice
// is a function of (nq, nk, m, dk, dv) alone and is coded family * 100 + NKT * 10 + C (include/ovc.h), C = 1, 2, 3 for
// max(dk, dv) <= 16, 32, 64 -- (KG, DVT) = (2, 1), (4, 1), (8, 2):
//   1 NKT C   attention_regs_kernel<NKT, KG, DVT>   up to 192 keys (nk + m: NKT = 1..6 tiles of 32; 128 regions + 40 memory slots
//                                                   and a bit, so that the shipped meshed-memory configuration stays here for
//                                                   every N <= 128) for up to 128 queries: one workgroup per (image, head), a wave
//                                                   per 32 queries, scores never leave the accumulators
//   2 0 C     attention_tiled_kernel<KG, DVT>       more than 192 keys, or more than 128 keys for more than 128 queries: key tiles
//                                                   of 128 under an online softmax, any nq and nk
//   3 0 0     attention_mfma_kernel                 more than 128 queries with at most 128 keys: the LDS-score kernel, 64-query tiles
// OVC_EINVAL for what the operator refuses from these five numbers.  OVC_ATTENTION_GENERAL (hooks build only) keeps every shape
// off the register instances.
constexpr int kFormAttRegs = 100, kFormAttTiled = 200, kFormAttLds = 300;

static int attention_form(int nq, int nk, int m, int dk, int dv) {
    if (nq <= 0 || nk <= 0 || m < 0) return OVC_EINVAL;
    if (dk <= 0 || dv <= 0 || (dk & 3) || (dv & 3) || dk > 64 || dv > 64) return OVC_EINVAL;
    const int nkt = (nk + m + 31) / 32, waves = (nq + 31) / 32, hmax = dk > dv ? dk : dv;
    const int cls = hmax <= 16 ? 1 : hmax <= 32 ? 2 : 3;
    if (nkt <= 6 && waves <= 4 && !OVC_HOOK_ENV("OVC_ATTENTION_GENERAL")) return kFormAttRegs + nkt * 10 + cls;
    if (nk + m > 128) return kFormAttTiled + cls;
    return kFormAttLds;
}

extern "C" int ovc_debug_attention_form(int nq, int nk, int m, int dk, int dv) { return attention_form(nq, nk, m, dk, dv); }

extern "C" int ovc_attention(const float* q, const float* k, const float* v, int b, int nq, int nk, int h,
                             int dk, int dv, const uint8_t* mask, long mask_sb, long mask_sq,
                             const float* geometry, const float* mem_k, const float* mem_v, int m,
                             float mem_scale_k, float mem_scale_v, float* out, ovc_stream stream) {
    if (!q || !k || !v || !out || b <= 0 || nq <= 0 || nk <= 0 || h <= 0) return OVC_EINVAL;
    if (const int rc = ovc_device_guard()) return rc;      // kernel attributes below are raised once per process
    const int form = attention_form(nq, nk, m, dk, dv);
    if (form < 0) return form;
    if (m > 0 && (!mem_k || !mem_v)) return OVC_EINVAL;
    if (!ovc_aligned16(q) || !ovc_aligned16(k) || !ovc_aligned16(v) || !ovc_aligned16(out)) return OVC_EINVAL;
    if (m > 0 && (!ovc_aligned16(mem_k) || !ovc_aligned16(mem_v))) return OVC_EINVAL;
    AttnArgs p{};
    p.q = q; p.k = k; p.v = v; p.out = out;
    p.b = b; p.nq = nq; p.nk = nk; p.h = h; p.dk = dk; p.dv = dv;
    p.mask = mask; p.mask_sb = mask_sb; p.mask_sq = mask_sq;
    p.geometry = geometry;
    p.mem_k = mem_k; p.mem_v = mem_v; p.m = m; p.mem_scale_k = mem_scale_k; p.mem_scale_v = mem_scale_v;
    p.nkp = ((nk + m + 31) / 32) * 32;
    p.qtiles = (nq + kQTile - 1) / kQTile;
    const int nkt = (nk + m + 31) / 32, waves = (nq + 31) / 32;
    switch (form) {
#define OVC_ATT(NKT, C, KG, DVT)                                                                                      \
    case kFormAttRegs + NKT * 10 + C: {                                                                               \
        const int k_rows = nkt * 32 > waves * 32 ? nkt * 32 : waves * 32;    /* the K image doubles as the output staging area */ \
        const size_t bytes = sizeof(float) * (size_t)(k_rows + nkt * 32) * kLdQK;                                     \
        static std::once_flag once;                                                                                   \
        std::call_once(once, [] {                                                                                     \
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(attention_regs_kernel<NKT, KG, DVT>),            \
                                      hipFuncAttributeMaxDynamicSharedMemorySize, 112 * 1024);                        \
        });                                                                                                           \
        hipLaunchKernelGGL((attention_regs_kernel<NKT, KG, DVT>), dim3(b * h), dim3(256), bytes, ovc_hip_stream(stream), p); \
    } break
#define OVC_ATT_H(NKT) OVC_ATT(NKT, 1, 2, 1); OVC_ATT(NKT, 2, 4, 1); OVC_ATT(NKT, 3, 8, 2)
        OVC_ATT_H(1); OVC_ATT_H(2); OVC_ATT_H(3); OVC_ATT_H(4); OVC_ATT_H(5); OVC_ATT_H(6);
#undef OVC_ATT_H
#undef OVC_ATT
#define OVC_ATT_TILED(C, KG, DVT)                                                                                     \
    case kFormAttTiled + C: {                                                                                         \
        p.qtiles = (nq + 127) / 128;                                                                                  \
        const size_t bytes = sizeof(float) * (size_t)(2 * 128) * kLdQK;                                               \
        static std::once_flag once;                                                                                   \
        std::call_once(once, [] {                                                                                     \
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(attention_tiled_kernel<KG, DVT>),                \
                                      hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);                         \
        });                                                                                                           \
        hipLaunchKernelGGL((attention_tiled_kernel<KG, DVT>), dim3(b * h * p.qtiles), dim3(256), bytes, ovc_hip_stream(stream), p); \
    } break
        OVC_ATT_TILED(1, 2, 1); OVC_ATT_TILED(2, 4, 1); OVC_ATT_TILED(3, 8, 2);
#undef OVC_ATT_TILED
        case kFormAttLds: {
            const size_t lds_bytes = sizeof(float) * ((size_t)kQTile * kLdQK + 2 * (size_t)p.nkp * kLdQK + (size_t)kQTile * (p.nkp + 4));
            static std::once_flag attr_once;
            std::call_once(attr_once, [] {
                (void)hipFuncSetAttribute(reinterpret_cast<const void*>(attention_mfma_kernel),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
            });
            hipLaunchKernelGGL(attention_mfma_kernel, dim3(b * h * p.qtiles), dim3(256), lds_bytes, ovc_hip_stream(stream), p);
        } break;
        default: return OVC_EINVAL;
    }
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

// =================================================================================================
// Decode-time attention (engine only)
// =================================================================================================

// One workgroup per beam row, all heads at once.
//   phase 0  the row's ancestor slots and pad flags for positions 0..t go to LDS (breaks the dependent
//            anc -> K load chain: every K/V load below is independent and can be in flight together)
//   phase 1  wave w takes keys w, w+4, ...: a key row [h*dk] is read fully coalesced (float4 per lane,
//            256 floats per instruction), multiplied with the matching q registers and reduced inside
//            each head's dk/4-lane group by shuffles -> sc[head][key]
//   phase 2  softmax over the t+1 keys of each head (one wave per head, lane = key)
//   phase 3  out = P V: thread = (float4 column, key group); groups are combined through LDS
constexpr int kSelfMaxHeads = 32;

// CH = float4-per-lane instructions per key row (h*dk / 256 rounded up): compile-time so that the loads of
// several keys can be issued back to back with clamped (always valid) addresses and no branches.
// KB = blocks of 64 positions held in LDS: 1 for t < 64, 4 for t < OVC_MAX_LEN (phase 2 then reduces each head over
// its KB blocks per lane before the wave reduction; KB = 1 is the round-1 kernel unchanged).
template <int CH, int KB = 1>
__global__ __launch_bounds__(256) void decode_self_attention_kernel(DecodeSelfArgs p) {
#include "bodies/decode_self_attention_kernel.inc"
}
template <int CH, int KB = 1>
__global__ __launch_bounds__(256) void decode_self_attention_kernel_gated(DecodeSelfArgs p, const int32_t* __restrict__ gate) {
    if (ovc_gate_closed(gate)) return;
#include "bodies/decode_self_attention_kernel.inc"
}

// Per-image form with ancestor de-duplication (round 3).  The k beams of an image descend from one another: at step t
// their histories name, per position j, only a few DISTINCT cache rows (measured on the BASELINE workload: 0.43 of the
// k (t + 1) rows the per-row kernel above reads -- one copy per beam).  The rows a position can name are the image's own
// width_j slots of that position's cache block (width_0 = 1, width_j = k), so the union is found with a k-bit mask per
// position.  One workgroup per (image, 4 heads), one wave per head, no LDS for data -- the structure of the
// cross-attention kernel below with a gathered key list:
//   wave 0   lane j <= t ORs the local slots of the image's beams at position j into a mask, a wave scan turns the
//            population counts into list offsets, and every (position, slot) that some beam names becomes one key
//            n -> (j, l) of an LDS list (<= 16 NT entries), with its <pad> flag and each beam's slot per position
//   S^T[key][beam] = K Q^T  on v_mfma_f32_16x16x4_f32, the beams as the 16-wide N dimension: every distinct key row is
//            read once and scored against all beams; a (key, beam) pair counts only if the beam's history names that
//            slot at that position (sl[beam][j] == l) -- the others get -inf, i.e. probability exactly 0
//   softmax over the keys held in accumulator registers, O^T = V^T P^T with the probabilities as the B operand.
// Key tiles past the end of the list are skipped with wave-uniform branches.  NT = key tiles the instance can hold
// (worst case k (t + 1) keys, chosen by the host), SB = d_k / 16.
//
// CHUNKED (t >= 64): the workgroup takes the kSelfChunk positions of chunk blockIdx.z only (at most 16 W listed keys, so
// NT = W tiles) and writes its softmax partials -- the beam's chunk maximum M, sum L = sum exp(s - M) and the unnormalised
// O = sum exp(s - M) v -- to p.part_ml / p.part_o; decode_self_merge_kernel combines the chunks.  A beam that names no
// unpadded key in the chunk writes M = -inf, L = 0, O = 0 (its exponentials are taken against 0, never -inf - -inf).
template <int NT, int SB, bool CHUNKED = false>
__global__ __launch_bounds__(256) void decode_self_attention_mfma_kernel(DecodeSelfArgs p) {
#include "bodies/decode_self_attention_mfma_kernel.inc"
}
template <int NT, int SB, bool CHUNKED = false>
__global__ __launch_bounds__(256) void decode_self_attention_mfma_kernel_gated(DecodeSelfArgs p, const int32_t* __restrict__ gate) {
    if (ovc_gate_closed(gate)) return;
#include "bodies/decode_self_attention_mfma_kernel.inc"
}

// The chunks of one (row, head) in ascending order: M = max_c M_c, then L = sum_c L_c exp(M_c - M) and O likewise, one
// division at the end (the order and the partition are functions of t alone: the bits do not depend on B or on the launch).
// A chunk with L_c = 0 named no key for the beam and is passed over.  Thread = one float4 of an output row.
__global__ __launch_bounds__(256) void decode_self_merge_kernel(DecodeSelfArgs p, int rows, int chunks) {
#include "bodies/decode_self_merge_kernel.inc"
}
__global__ __launch_bounds__(256) void decode_self_merge_kernel_gated(DecodeSelfArgs p, int rows, int chunks, const int32_t* __restrict__ gate) {
    if (ovc_gate_closed(gate)) return;
#include "bodies/decode_self_merge_kernel.inc"
}

// ---- which instance a decode self-attention launch takes ---------------------------------------------------------------
// ONE selection function for the launcher below and for the form query of the test hook (ovc_debug_decode_self_form): the
// choice is a function of (t, width, rows, h, d_k, per_row) alone and is coded as family * 100 + a * 10 + b (include/ovc.h):
//   1 NT SB   decode_self_attention_mfma_kernel<NT, SB>         t < 64, d_k >= 16, at most 112 listed keys in the worst case
//   2 NT SB   decode_self_attention_mfma_kernel<NT, SB, true>   t >= 64, d_k >= 16: one workgroup per chunk of kSelfChunk
//             + decode_self_merge_kernel                        positions (at most 16 W listed keys: NT = W tiles), then the merge
//   3 CH KB   decode_self_attention_kernel<CH, KB>              everything else (d_k in {4, 8}, more than 112 keys, per_row):
//                                                               KB = 1 for t < 64, 4 blocks of 64 positions from there
// t < 64 never takes a chunked instance, so the bits of those steps are the round-3 kernels'.  per_row forces family 3 where
// the de-duplicated kernels are eligible (the A/B switch of the hooks build, and the test hook).
constexpr int kFormSelfMfma = 100, kFormSelfChunked = 200, kFormSelfRows = 300;
constexpr int kFormCrossMfma = 400, kFormCrossTiled = 500, kFormCrossLds = 600;

static int decode_self_form(int t, int W, int rows, int h, int dk, bool per_row) {
    if (t < 0 || t >= OVC_MAX_LEN || h <= 0 || h > kSelfMaxHeads) return OVC_EINVAL;
    if ((dk & (dk - 1)) || dk < 4 || dk > 64) return OVC_EINVAL;                            // dk in {4,8,16,32,64}
    const int hk = h * dk;
    if (hk > 1024) return OVC_EINVAL;
    const bool per_image = !per_row && W >= 1 && W <= OVC_MAX_BEAM && rows % W == 0 && dk >= 16;
    const int SB = dk >> 4, CH = hk <= 256 ? 1 : hk <= 512 ? 2 : 4;
    if (t >= 64) {
        if (per_image) return kFormSelfChunked + (W <= 1 ? 1 : W <= 2 ? 2 : W <= 4 ? 4 : W <= 5 ? 5 : 8) * 10 + SB;
        return kFormSelfRows + CH * 10 + 4;
    }
    // per-image kernel with ancestor de-duplication: the image's rows in one workgroup, at most 112 listed keys
    const int worst = t == 0 ? 1 : W * (t + 1);
    if (per_image && worst <= 112) {
        const int tiles = (worst + 15) / 16;
        return kFormSelfMfma + (tiles <= 1 ? 1 : tiles <= 2 ? 2 : tiles <= 4 ? 4 : 7) * 10 + SB;
    }
    return kFormSelfRows + CH * 10 + 1;
}

static int decode_self_attention_as(const DecodeSelfArgs& p, int rows, bool per_row, hipStream_t stream, const int32_t* gate) {
    if (p.dk != p.dv) return OVC_EINVAL;
    const int form = decode_self_form(p.t, p.width, rows, p.h, p.dk, per_row);
    if (form < 0) return form;
    const int W = p.width;
    const bool chunked = form >= kFormSelfChunked && form < kFormSelfRows;
    if (chunked && (!p.part_o || !p.part_ml)) return OVC_EINVAL;
    const int chunks = (p.t + kSelfChunk) / kSelfChunk;
    switch (form) {
#define OVC_SELF(NT, SB)                                                                                             \
    case kFormSelfMfma + NT * 10 + SB: {                                                                             \
        const dim3 grid(rows / W, (p.h + 3) / 4), block(256);                                                        \
        if (gate) hipLaunchKernelGGL((decode_self_attention_mfma_kernel_gated<NT, SB>), grid, block, 0, stream, p, gate); \
        else hipLaunchKernelGGL((decode_self_attention_mfma_kernel<NT, SB>), grid, block, 0, stream, p);            \
    } break
#define OVC_SELF_CHUNKED(NT, SB)                                                                                     \
    case kFormSelfChunked + NT * 10 + SB: {                                                                          \
        const dim3 grid(rows / W, (p.h + 3) / 4, chunks), block(256);                                                \
        if (gate) hipLaunchKernelGGL((decode_self_attention_mfma_kernel_gated<NT, SB, true>), grid, block, 0, stream, p, gate); \
        else hipLaunchKernelGGL((decode_self_attention_mfma_kernel<NT, SB, true>), grid, block, 0, stream, p);      \
    } break
#define OVC_SELF_ROWS(CH, KB)                                                                                        \
    case kFormSelfRows + CH * 10 + KB:                                                                               \
        if (gate) hipLaunchKernelGGL((decode_self_attention_kernel_gated<CH, KB>), dim3(rows), dim3(256), 0, stream, p, gate); \
        else hipLaunchKernelGGL((decode_self_attention_kernel<CH, KB>), dim3(rows), dim3(256), 0, stream, p);       \
        break
#define OVC_SELF_SB(M, NT) M(NT, 1); M(NT, 2); M(NT, 4)
        OVC_SELF_SB(OVC_SELF, 1); OVC_SELF_SB(OVC_SELF, 2); OVC_SELF_SB(OVC_SELF, 4); OVC_SELF_SB(OVC_SELF, 7);
        OVC_SELF_SB(OVC_SELF_CHUNKED, 1); OVC_SELF_SB(OVC_SELF_CHUNKED, 2); OVC_SELF_SB(OVC_SELF_CHUNKED, 4);
        OVC_SELF_SB(OVC_SELF_CHUNKED, 5); OVC_SELF_SB(OVC_SELF_CHUNKED, 8);
        OVC_SELF_ROWS(1, 1); OVC_SELF_ROWS(2, 1); OVC_SELF_ROWS(4, 1);
        OVC_SELF_ROWS(1, 4); OVC_SELF_ROWS(2, 4); OVC_SELF_ROWS(4, 4);
#undef OVC_SELF_SB
#undef OVC_SELF_ROWS
#undef OVC_SELF_CHUNKED
#undef OVC_SELF
        default: return OVC_EINVAL;
    }
    OVC_RETURN_IF_LAUNCH_FAILED();
    if (chunked) {                                         // the chunks' partials -> out
        const int threads = rows * ((p.h * p.dv) >> 2);
        if (gate) hipLaunchKernelGGL(decode_self_merge_kernel_gated, dim3((threads + 255) / 256), dim3(256), 0, stream, p, rows, chunks, gate);
        else hipLaunchKernelGGL(decode_self_merge_kernel, dim3((threads + 255) / 256), dim3(256), 0, stream, p, rows, chunks);
        OVC_RETURN_IF_LAUNCH_FAILED();
    }
    return OVC_OK;
}

int ovc_decode_self_attention(const DecodeSelfArgs& p, int rows, hipStream_t stream, const int32_t* gate) {
    static const bool per_row = OVC_HOOK_ENV("OVC_SELF_ATTENTION_ROWS") != nullptr;     // A/B switch: the round-1 per-row kernel
    return decode_self_attention_as(p, rows, per_row, stream, gate);
}

// Decode cross-attention: the k beams of an image share the image's projected encoder K/V.
//
// decode_cross_attention_mfma_kernel -- one wave per (image, head, level), no LDS, both contractions on
// the matrix cores (v_mfma_f32_16x16x4_f32) with the beams as the 16-wide N dimension:
//   S^T[key][beam] = K Q^T : A = K rows (16 keys per tile), B = Q^T.  Lane (r = lane & 15, kq = lane >> 4)
//       loads float4 K[key r][16 S + 4 kq ..] / Q[beam r][16 S + 4 kq ..] and feeds element e to MFMA
//       (S, e); both operands use the same d <-> (S, kq, e) assignment, so every d is summed once.
//   softmax over keys: the accumulator has the beam on the lane (col = lane & 15) and the keys on
//       registers (row = 4 kq + reg): reduce over registers, then __shfl_xor 16 / 32 across the four kq lanes.
//   O^T[dv][beam] = V^T P^T : the probabilities stay in the accumulator registers and are used directly as
//       the B operand (lane (beam, kq), register reg  <->  key 16 T + 4 kq + reg); A = V^T is loaded as
//       float4 V[key][4 r ..] (a fully coalesced 256-byte head slice per key) and element e' feeds MFMA e',
//       whose output row r is dv = 4 r + e'.  Four MFMA results give each lane float4s of consecutive dv.
// K and V are read from HBM exactly once with 16-byte loads; the kernel is bound by that stream
// (52 MB per layer-step at B = 256).
// NT = key tiles (16 keys each), SB = d_k / 16: compile-time so that every load below is unconditional
// (hipcc branches around a guarded load and waits vmcnt(0) after it, serialising the whole K/V stream).
template <int NT, int SB>
__global__ __launch_bounds__(256) void decode_cross_attention_mfma_kernel(DecodeCrossArgs p) {
#include "bodies/decode_cross_attention_mfma_kernel.inc"
}
template <int NT, int SB>
__global__ __launch_bounds__(256) void decode_cross_attention_mfma_kernel_gated(DecodeCrossArgs p, const int32_t* __restrict__ gate) {
    if (ovc_gate_closed(gate)) return;
#include "bodies/decode_cross_attention_mfma_kernel.inc"
}

// The same kernel for more than 128 regions (round 4; the reference has no limit): the keys pass through the wave in chunks
// of 64 (four 16-key tiles), in ascending order, under an online softmax -- a running maximum and sum per beam column, the
// output accumulators rescaled by exp(M_old - M_new) when a chunk raises the maximum (a per-lane scalar: a lane's accumulator
// registers all belong to ITS beam).  Fixed chunk order: results depend on the operands only.  N <= 128 never comes here.
template <int SB>
__global__ __launch_bounds__(256) void decode_cross_attention_tiled_kernel(DecodeCrossArgs p) {
#include "bodies/decode_cross_attention_tiled_kernel.inc"
}
template <int SB>
__global__ __launch_bounds__(256) void decode_cross_attention_tiled_kernel_gated(DecodeCrossArgs p, const int32_t* __restrict__ gate) {
    if (ovc_gate_closed(gate)) return;
#include "bodies/decode_cross_attention_tiled_kernel.inc"
}

// Head sizes 4 and 8 (not multiples of the 16-deep MFMA k block): VALU dots on LDS-staged rows.  The scores of all N keys
// stay in LDS; K and then V of the (image, head) pass through in chunks of 128 rows, ascending, so any region count fits
// (round 4) and the sums keep the key order of the one-shot form.
// Exercised by tests/test_engine_gpu.py::test_unusual_dimensions_against_oracle (d_k = 8 and d_k = 4 cases) and, against fp64 at
// the operator level with every other decode attention instance, by tests/test_decode_attention_gpu.py.
constexpr int kCrossChunk = 128;

__global__ __launch_bounds__(256) void decode_cross_attention_lds_kernel(DecodeCrossArgs p) {
#include "bodies/decode_cross_attention_lds_kernel.inc"
}
__global__ __launch_bounds__(256) void decode_cross_attention_lds_kernel_gated(DecodeCrossArgs p, const int32_t* __restrict__ gate) {
    if (ovc_gate_closed(gate)) return;
#include "bodies/decode_cross_attention_lds_kernel.inc"
}

// Which instance a decode cross-attention launch takes (shared with ovc_debug_decode_cross_form; the coding continues the
// self-attention's): 4 NT SB = decode_cross_attention_mfma_kernel<NT, SB> (N <= 64: NT = 4, N <= 128: NT = 8),
// 5 0 SB = decode_cross_attention_tiled_kernel<SB> (N > 128), 6 0 0 = decode_cross_attention_lds_kernel (d_k not 16 / 32 / 64).
static int decode_cross_form(int N, int W, int dk, int dv) {
    if (N <= 0 || N > OVC_MAX_REGIONS || W <= 0 || W > OVC_MAX_BEAM) return OVC_EINVAL;
    if (dk > 64 || dv > 64 || dk <= 0 || dv <= 0 || (dk & 3) || (dv & 3)) return OVC_EINVAL;
    if (dk == 16 || dk == 32 || dk == 64) {
        const int SB = dk >> 4;
        if (N > 128) return kFormCrossTiled + SB;   // more regions than the register-resident instances hold: key chunks + online softmax
        return kFormCrossMfma + (N <= 64 ? 4 : 8) * 10 + SB;
    }
    return kFormCrossLds;
}

int ovc_decode_cross_attention(const DecodeCrossArgs& p, int B, int h, int levels, hipStream_t stream, const int32_t* gate) {
    if (p.heads != h) return OVC_EINVAL;
    const int form = decode_cross_form(p.n, p.width, p.dk, p.dv);
    if (form < 0) return form;
    const dim3 grid(B, (h + 3) / 4, levels), block(256);
    switch (form) {
#define OVC_CROSS(NT, SB)                                                                                            \
    case kFormCrossMfma + NT * 10 + SB:                                                                              \
        if (gate) hipLaunchKernelGGL((decode_cross_attention_mfma_kernel_gated<NT, SB>), grid, block, 0, stream, p, gate); \
        else hipLaunchKernelGGL((decode_cross_attention_mfma_kernel<NT, SB>), grid, block, 0, stream, p);           \
        break
#define OVC_CROSS_TILED(SB)                                                                                          \
    case kFormCrossTiled + SB:                                                                                       \
        if (gate) hipLaunchKernelGGL(decode_cross_attention_tiled_kernel_gated<SB>, grid, block, 0, stream, p, gate); \
        else hipLaunchKernelGGL(decode_cross_attention_tiled_kernel<SB>, grid, block, 0, stream, p);                \
        break
        OVC_CROSS(4, 1); OVC_CROSS(4, 2); OVC_CROSS(4, 4); OVC_CROSS(8, 1); OVC_CROSS(8, 2); OVC_CROSS(8, 4);
        OVC_CROSS_TILED(1); OVC_CROSS_TILED(2); OVC_CROSS_TILED(4);
#undef OVC_CROSS_TILED
#undef OVC_CROSS
        case kFormCrossLds: {
            const size_t lds_bytes = sizeof(float) * ((size_t)kCrossChunk * kLdQK + (size_t)p.width * 64 + (size_t)p.width * p.n);
            static std::once_flag attr_once;
            std::call_once(attr_once, [] {
                (void)hipFuncSetAttribute(reinterpret_cast<const void*>(decode_cross_attention_lds_kernel),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
                (void)hipFuncSetAttribute(reinterpret_cast<const void*>(decode_cross_attention_lds_kernel_gated),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            });
            if (gate) hipLaunchKernelGGL(decode_cross_attention_lds_kernel_gated, dim3(B, h, levels), dim3(256), lds_bytes, stream, p, gate);
            else hipLaunchKernelGGL(decode_cross_attention_lds_kernel, dim3(B, h, levels), dim3(256), lds_bytes, stream, p);
        } break;
        default: return OVC_EINVAL;
    }
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

// =================================================================================================
// Test hooks: the two launchers above on caller buffers, and the instance each launch takes (include/ovc.h)
// =================================================================================================
// What the engine's model_ok / heads_ok never send is OVC_EINVAL here, with nothing launched.
static bool debug_heads_ok(int h, int dk) {
    return (dk == 4 || dk == 8 || dk == 16 || dk == 32 || dk == 64) && h >= 1 && h <= kSelfMaxHeads && h * dk <= 1024;
}
static bool debug_self_shape_ok(int t, int W, int rows, int h, int dk) {
    return debug_heads_ok(h, dk) && t >= 0 && t < OVC_MAX_LEN && W >= 1 && W <= OVC_MAX_BEAM && rows >= 1 && rows % W == 0 &&
           (t > 0 || W == 1);                                   // position 0 holds one slot per image: width_0 = 1
}
static bool debug_cross_shape_ok(int N, int W, int h, int dk) {
    return debug_heads_ok(h, dk) && N >= 1 && N <= OVC_MAX_REGIONS && W >= 1 && W <= OVC_MAX_BEAM;
}

extern "C" int ovc_debug_decode_self_form(int t, int width, int rows, int h, int d_k, int per_row) {
    if (!debug_self_shape_ok(t, width, rows, h, d_k)) return OVC_EINVAL;
    return decode_self_form(t, width, rows, h, d_k, per_row != 0);
}

extern "C" int ovc_debug_decode_cross_form(int N, int width, int h, int d_k) {
    if (!debug_cross_shape_ok(N, width, h, d_k)) return OVC_EINVAL;
    return decode_cross_form(N, width, d_k, d_k);
}

extern "C" size_t ovc_debug_decode_self_partial_bytes(int t, int rows, int h, int d_k) {
    if (t < 64 || t >= OVC_MAX_LEN || rows < 1 || !debug_heads_ok(h, d_k)) return 0;
    const size_t chunks = (size_t)(t + kSelfChunk) / kSelfChunk;
    return sizeof(float) * chunks * rows * ((size_t)h * d_k + 2 * (size_t)h);      // part_o, then part_ml
}

extern "C" int ovc_debug_decode_self_attention(const float* q, int ldq, const float* kcache, const float* vcache, size_t pos_stride,
                                               int ldkv, const int32_t* anc, int anc_ld, const uint8_t* padflag, int pad_ld, int t,
                                               int width, int rows, int h, int d_k, float* out, int ldo, void* partials,
                                               size_t partial_bytes, const int32_t* gate, int per_row, ovc_stream stream) {
    if (!q || !kcache || !vcache || !padflag || !out || (t > 0 && !anc)) return OVC_EINVAL;
    if (!debug_self_shape_ok(t, width, rows, h, d_k)) return OVC_EINVAL;
    const int hk = h * d_k;
    if (ldq < hk || ldkv < hk || ldo < hk || (ldq & 3) || (ldkv & 3) || (ldo & 3) || (pos_stride & 3)) return OVC_EINVAL;
    if (anc_ld < t || pad_ld < rows) return OVC_EINVAL;
    if (!ovc_aligned16(q) || !ovc_aligned16(kcache) || !ovc_aligned16(vcache) || !ovc_aligned16(out)) return OVC_EINVAL;
    const size_t need = ovc_debug_decode_self_partial_bytes(t, rows, h, d_k);
    if (need && (!partials || !ovc_aligned16(partials) || partial_bytes < need)) return OVC_EINVAL;
    if (const int rc = ovc_device_guard()) return rc;
    DecodeSelfArgs p{};
    p.q = q; p.ldq = ldq; p.kcache = kcache; p.vcache = vcache; p.pos_stride = pos_stride; p.ldkv = ldkv;
    p.anc = anc; p.anc_ld = anc_ld; p.padflag = padflag; p.pad_ld = pad_ld;
    p.t = t; p.width = width; p.h = h; p.dk = d_k; p.dv = d_k;
    p.out = out; p.ldo = ldo;
    if (need) {
        const size_t chunks = (size_t)(t + kSelfChunk) / kSelfChunk;
        p.part_o = static_cast<float*>(partials);
        p.part_ml = p.part_o + chunks * rows * hk;
    }
    return decode_self_attention_as(p, rows, per_row != 0, ovc_hip_stream(stream), gate);
}

extern "C" int ovc_debug_decode_cross_attention(const float* q, int ldq, const float* kx, const float* vx, size_t level_stride, int ldkv,
                                                const uint8_t* encmask, int N, int width, int B, int heads, int d_k, int levels,
                                                float* out, size_t out_level_stride, int ldo, const int32_t* gate, ovc_stream stream) {
    if (!q || !kx || !vx || !out || B < 1 || levels < 1 || levels > OVC_MAX_LEVELS) return OVC_EINVAL;
    if (!debug_cross_shape_ok(N, width, heads, d_k)) return OVC_EINVAL;
    const int hk = heads * d_k;
    if (ldq < hk || ldkv < hk || ldo < hk || (ldq & 3) || (ldkv & 3) || (ldo & 3) || (level_stride & 3) || (out_level_stride & 3)) return OVC_EINVAL;
    if (!ovc_aligned16(q) || !ovc_aligned16(kx) || !ovc_aligned16(vx) || !ovc_aligned16(out)) return OVC_EINVAL;
    if (const int rc = ovc_device_guard()) return rc;
    DecodeCrossArgs p{};
    p.q = q; p.ldq = ldq; p.kx = kx; p.vx = vx; p.level_stride = level_stride; p.ldkv = ldkv;
    p.encmask = encmask; p.n = N; p.width = width; p.heads = heads; p.dk = d_k; p.dv = d_k;
    p.out = out; p.out_level_stride = out_level_stride; p.ldo = ldo;
    return ovc_decode_cross_attention(p, B, heads, levels, ovc_hip_stream(stream), gate);
}

// =================================================================================================
// Cross-attention maps (ovc_cross_attention_maps): the probabilities themselves, to memory
// =================================================================================================
//
// cross_attention_maps_kernel -- P = softmax(q K^T / sqrt(d_k), masked keys -> -inf) of ovc_attention's operands without the
// values: the rule of include/ovc.h, the arithmetic of the forward kernels above (fp32 dot product on the matrix cores, ONE
// division by sqrtf(d_k), expf(s - max), ONE division by the sum).
//
// One workgroup per (image, head, 128 queries), a wave per 32 queries, the register layout of attention_regs_kernel:
//   S^T[key][q] = K Q^T on v_mfma_f32_32x32x2_f32 with the QUERY on the lane (q = lane & 31) and 16 keys of each 32-key tile on
//   its accumulator registers (key = 32 tk + (r & 3) + 8 (r >> 2) + 4 (lane >> 5)): scale, mask and the softmax over keys are
//   register arithmetic plus one __shfl_xor(32) per reduction.
// Keys pass through LDS in tiles of kMapKeys = 128 (four accumulators per wave).
//   One tile (nk + m <= 128, every shipped configuration): the scores are formed once and stay in registers.
//   More tiles: three sweeps over the tiles in ascending order -- the row maximum, then the sum of expf(s - max), then the
//   probabilities -- each forming a tile's scores again from the same operands, so the three see the same bits and the result
//   is the rule's: no running maximum, no rescaling.  Nothing is read back from the map.
// A query's sum adds its lane's keys tile by tile in register order, then the other half's: only that order differs from the
// forward kernels (include/ovc.h).
// Output: a wave turns its [key][query] registers into a [32 queries][128 keys] image in LDS (its own region: no workgroup
// barrier) and rows leave as contiguous keys, one float4 per lane, 512 bytes per row and tile.  p.kp = nk + m rounded up to 4
// floats are written per row (the tail past nk + m holds 0, or NaN in a row without a valid key); nothing beyond it.
// A row whose keys are all masked is NaN in every valid key, as the reference's softmax over a row of -inf.
// KG = 8-deep d groups of Q.K (dk <= 8 KG).
constexpr int kMapKeys = 128;
constexpr int kMapLd = kMapKeys + 4;      // row stride (floats) of a wave's output image

struct MapArgs {
    const float* q; const float* k; float* maps;
    int nq, nk, h, dk;
    const uint8_t* mask; long mask_sb, mask_sq;
    const float* mem_k; int m; float mem_scale_k;
    long map_sb, map_sh, map_sq;          // strides (floats) of image, head and query row of the map; keys are contiguous
    int kp;                               // nk + m rounded up to a multiple of 4
    int qtiles;
};

template <int KG>
__global__ __launch_bounds__(256) void cross_attention_maps_kernel(MapArgs p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int NKT = kMapKeys / 32;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int qt = blockIdx.x % p.qtiles;
    const int hd = (blockIdx.x / p.qtiles) % p.h;
    const int b = blockIdx.x / (p.qtiles * p.h);
    const int nkt = p.nk + p.m;
    const int tiles = (nkt + kMapKeys - 1) / kMapKeys;
    float* Ks = lds;                                               // [128][68]
    float* Ps = Ks + kMapKeys * kLdQK + wave * 32 * kMapLd;        // this wave's [32][132]

    const int qi = lane & 31, half = lane >> 5;
    const int gq = qt * kMapKeys + wave * 32 + qi;                 // this lane's query
    const bool q_ok = gq < p.nq;
    const bool wave_live = qt * kMapKeys + wave * 32 < p.nq;       // wave-uniform: waves past the last query only stage
    f32x4 qf[KG];
    {
        const float* qrow = p.q + ((size_t)b * p.nq + min(gq, p.nq - 1)) * (p.h * p.dk) + hd * p.dk;
#pragma unroll
        for (int kk = 0; kk < KG; ++kk) {
            const int d = 8 * kk + 4 * half;
            qf[kk] = *reinterpret_cast<const f32x4*>(qrow + min(d, p.dk - 4));
            if (!q_ok || d >= p.dk) qf[kk] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    const float inv_scale = sqrtf((float)p.dk);
    const uint8_t* mrow = p.mask ? p.mask + (size_t)b * p.mask_sb + (size_t)min(gq, p.nq - 1) * p.mask_sq : nullptr;
    float* orow = p.maps + (size_t)b * p.map_sb + (size_t)hd * p.map_sh;

    f32x16 st[NKT];
    // The masked, scaled scores of key tile k0 .. k0 + 127 into st: the tile's K rows -> LDS (zero-filled past the last key,
    // every load issued before the first LDS store, none of them conditional), S^T = K Q^T, then scale and mask.  All four
    // waves stage and meet at both barriers; a wave without queries skips the arithmetic.
    auto scores = [&](int k0) {
        {
            const int c4 = tid & 15, col = c4 * 4, r0 = tid >> 4;
            constexpr int kPasses = kMapKeys / 16;
            // Every load is unconditional and from ONE base with a clamped (always valid) row: the image's keys here, the slot
            // keys -- only where the call has slots, a workgroup-uniform branch -- below.  Which VALUE a row takes is chosen
            // afterwards; no address is ever chosen between the two bases (p.mem_k is NULL without slots).
            f32x4 kv[kPasses], mv[kPasses];
#pragma unroll
            for (int i = 0; i < kPasses; ++i) {
                const int kr = min(k0 + r0 + 16 * i, p.nk - 1);
                kv[i] = *reinterpret_cast<const f32x4*>(p.k + ((size_t)b * p.nk + kr) * (p.h * p.dk) + hd * p.dk + min(col, p.dk - 4));
                mv[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            if (p.m > 0) {
#pragma unroll
                for (int i = 0; i < kPasses; ++i) {
                    const int mr = min(max(k0 + r0 + 16 * i - p.nk, 0), p.m - 1);
                    mv[i] = *reinterpret_cast<const f32x4*>(p.mem_k + (size_t)mr * (p.h * p.dk) + hd * p.dk + min(col, p.dk - 4)) * p.mem_scale_k;
                }
            }
#pragma unroll
            for (int i = 0; i < kPasses; ++i) {
                const int r = r0 + 16 * i, kr = k0 + r;
                f32x4 kx = kr < p.nk ? kv[i] : mv[i];               // a real key, else a slot key
                if (kr >= nkt || col >= p.dk) kx = f32x4{0.f, 0.f, 0.f, 0.f};
                *reinterpret_cast<f32x4*>(Ks + r * kLdQK + col) = kx;
            }
        }
        __syncthreads();
        if (wave_live) {
#pragma unroll
            for (int tk = 0; tk < NKT; ++tk)
#pragma unroll
                for (int r = 0; r < 16; ++r) st[tk][r] = 0.f;
#pragma unroll
            for (int kk = 0; kk < KG; ++kk) {
                f32x4 kf[NKT];
#pragma unroll
                for (int tk = 0; tk < NKT; ++tk) kf[tk] = *reinterpret_cast<const f32x4*>(Ks + (tk * 32 + qi) * kLdQK + 8 * kk + 4 * half);
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int tk = 0; tk < NKT; ++tk) st[tk] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[tk][s], qf[kk][s], st[tk], 0, 0, 0);
            }
            // per 32-key tile the mask bytes of this lane's 16 keys: unconditional loads at clamped (always valid) positions,
            // in flight together; a call without a mask (workgroup-uniform) loads nothing
#pragma unroll
            for (int tk = 0; tk < NKT; ++tk) {
                uint8_t mb[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) mb[r] = 0;
                if (p.mask) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) mb[r] = mrow[min(k0 + tk * 32 + (r & 3) + 8 * (r >> 2) + 4 * half, p.nk - 1)];
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int kj = k0 + tk * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    const float s = st[tk][r] / inv_scale;
                    st[tk][r] = (kj >= nkt || (kj < p.nk && mb[r])) ? -INFINITY : s;
                }
            }
        }
        __syncthreads();                                           // every wave is done with the K image
    };
    auto tile_max = [&](float mx) {
#pragma unroll
        for (int tk = 0; tk < NKT; ++tk)
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, st[tk][r]);
        return mx;
    };
    // st <- expf(st - mx); returns sum + the tile's exponentials, added in register order
    auto tile_exp = [&](float mx, float sum) {
#pragma unroll
        for (int tk = 0; tk < NKT; ++tk)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float e = expf(st[tk][r] - mx);
                st[tk][r] = e;
                sum += e;
            }
        return sum;
    };
    // st / sum -> the wave's LDS image [query][key] -> the map's rows, contiguous keys
    auto tile_store = [&](int k0, float sum) {
#pragma unroll
        for (int tk = 0; tk < NKT; ++tk)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                *reinterpret_cast<f32x4*>(Ps + qi * kMapLd + tk * 32 + 8 * j + 4 * half) =
                    f32x4{st[tk][4 * j] / sum, st[tk][4 * j + 1] / sum, st[tk][4 * j + 2] / sum, st[tk][4 * j + 3] / sum};
        // (the wave reads back only what it wrote itself: no workgroup barrier, the compiler's lgkmcnt wait orders it)
        const int col = (lane & 31) * 4;
#pragma unroll
        for (int pass = 0; pass < 16; ++pass) {
            const int row = pass * 2 + half;
            const int oq = qt * kMapKeys + wave * 32 + row;
            if (oq < p.nq && k0 + col < p.kp)
                *reinterpret_cast<f32x4*>(orow + (size_t)oq * p.map_sq + k0 + col) = *reinterpret_cast<const f32x4*>(Ps + row * kMapLd + col);
        }
    };

    if (tiles == 1) {
        scores(0);
        if (!wave_live) return;
        float mx = tile_max(-INFINITY);
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        float sum = tile_exp(mx, 0.f);
        sum += __shfl_xor(sum, 32, 64);
        tile_store(0, sum);
        return;
    }
    float mx = -INFINITY, sum = 0.f;
    for (int t = 0; t < tiles; ++t) {
        scores(t * kMapKeys);
        if (wave_live) mx = tile_max(mx);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    for (int t = 0; t < tiles; ++t) {
        scores(t * kMapKeys);
        if (wave_live) sum = tile_exp(mx, sum);
    }
    sum += __shfl_xor(sum, 32, 64);
    for (int t = 0; t < tiles; ++t) {
        scores(t * kMapKeys);
        if (wave_live) {
            (void)tile_exp(mx, 0.f);
            tile_store(t * kMapKeys, sum);
        }
    }
}

// maps [b][h][nq][row stride map_sq]: image stride map_sb, head stride map_sh (floats; include/ovc.h)
extern "C" int ovc_cross_attention_maps(const float* q, const float* k, int b, int nq, int nk, int h, int dk, const uint8_t* mask,
                                        long mask_sb, long mask_sq, const float* mem_k, int m, float mem_scale_k, float* maps,
                                        long map_sb, long map_sh, long map_sq, ovc_stream stream) {
    if (!q || !k || !maps || b <= 0 || nq <= 0 || nk <= 0 || h <= 0) return OVC_EINVAL;
    if (const int rc = ovc_device_guard()) return rc;      // the kernel attribute below is raised once per process
    if (dk <= 0 || (dk & 3) || dk > 64) return OVC_EINVAL;
    if (m < 0 || (m > 0 && !mem_k)) return OVC_EINVAL;
    if (!ovc_aligned16(q) || !ovc_aligned16(k) || !ovc_aligned16(maps) || (m > 0 && !ovc_aligned16(mem_k))) return OVC_EINVAL;
    const long kp = ((long)nk + m + 3) & ~3L;
    // float4 row stores: every stride a multiple of 4 floats, a row at least kp wide, rows / heads / images that do not overlap
    if ((map_sq & 3) || (map_sh & 3) || (map_sb & 3) || map_sq < kp || map_sh < (long)nq * map_sq || map_sb < (long)h * map_sh)
        return OVC_EINVAL;
    const long qtiles = ((long)nq + kMapKeys - 1) / kMapKeys;
    if (kp > 0x7fffffffL || (long)b * h * qtiles > 0x7fffffffL) return OVC_EINVAL;
    MapArgs p{};
    p.q = q; p.k = k; p.maps = maps;
    p.nq = nq; p.nk = nk; p.h = h; p.dk = dk;
    p.mask = mask; p.mask_sb = mask_sb; p.mask_sq = mask_sq;
    p.mem_k = mem_k; p.m = m; p.mem_scale_k = mem_scale_k;
    p.map_sb = map_sb; p.map_sh = map_sh; p.map_sq = map_sq;
    p.kp = (int)kp; p.qtiles = (int)qtiles;
    // LDS: the K tile [128][68] and four output images [32][132]: 102 400 bytes, above the 64 KiB a launch gets by default
    constexpr size_t bytes = sizeof(float) * ((size_t)kMapKeys * kLdQK + 4 * 32 * (size_t)kMapLd);
    const dim3 grid((unsigned)(b * h * qtiles)), block(256);
#define OVC_MAPS(KG)                                                                                                  \
    do {                                                                                                              \
        static bool fits = false;                                                                                     \
        static std::once_flag once;                                                                                   \
        std::call_once(once, [] {                                                                                     \
            fits = hipFuncSetAttribute(reinterpret_cast<const void*>(cross_attention_maps_kernel<KG>),               \
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess;         \
            if (!fits) (void)hipGetLastError();                                                                       \
        });                                                                                                           \
        if (!fits) return OVC_EINVAL;                      /* a device without that much LDS per workgroup */         \
        hipLaunchKernelGGL((cross_attention_maps_kernel<KG>), grid, block, bytes, ovc_hip_stream(stream), p);         \
    } while (0)
    if (dk <= 16) OVC_MAPS(2); else if (dk <= 32) OVC_MAPS(4); else OVC_MAPS(8);
#undef OVC_MAPS
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

// Test hook (tests/test_attention_maps_gpu.py): the kernel on raw operands, as run_decoder_layer launches it for one level --
// q [b, nq, h*d_k], k [b, nk, h*d_k], mask [b, nk] (NULL: none), m slot keys m_k [m, h*d_k] scaled by sqrtf(d_k) -> P [b, h, nq,
// ld] with ld = nk + m rounded up to 4.
extern "C" int ovc_debug_cross_attention_maps(const float* q, const float* k, const uint8_t* mask, const float* m_k, int b, int nq,
                                              int nk, int h, int d_k, int m, float* P, ovc_stream stream) {
    if (d_k <= 0 || nq <= 0 || nk <= 0 || h <= 0 || m < 0) return OVC_EINVAL;
    const long ld = ((long)nk + m + 3) & ~3L;
    return ovc_cross_attention_maps(q, k, b, nq, nk, h, d_k, mask, nk, 0, m_k, m, sqrtf((float)d_k), P, (long)h * nq * ld,
                                    (long)nq * ld, ld, stream);
}
