// gemm_rows16_f32 -- the four-chain K-order class for products with a handful of rows (round 4; included by gemm.hip).
//
// The reference's own prediction loop decodes ONE image at a time (trainers/base_trainer.py:75-80): M = B * beam = 5 rows per
// decode-step product, 40 at B = 8.  The 32 x 32 instances of gemm_f32_mfma spend 6.6 us on such a launch whatever the tiling
//  while a dependent launch that reads its predecessor's output and writes costs 1.75 us
// (tools/phase_floor_probe.hip): the kernel's own latency -- a cooperative tile load, two barriers per K tile, a 64-MFMA chain of
// v_mfma_f32_32x32x2_f32 per wave of which 27 rows in 32 are padding -- is what a 5-row product pays for.  This instance:
//
//   * 16-row tiles on v_mfma_f32_16x16x4_f32: the SAME dependent fma chain per output element (k ascending, four k per
//     instruction instead of two), so the bits are those of every other instance of the class, in a quarter of the matrix time
//     (32 cycles per four k against 2 x 64);
//   * one wave per chain, as in the 32 x 32 instances (chain c = the 8-deep k groups g with g % 4 == c, summed ((c0+c1)+c2)+c3
//     through LDS at the end), but each wave fetches ITS OWN quarter of A and W -- the k groups of its chain -- with 16-byte loads
//     issued all at once, turns them into MFMA operand order through a wave-private LDS region (a lane group kq supplies ONE k of
//     every instruction: a transpose of what 16-byte loads deliver) and runs its whole chain: ONE global round trip and no workgroup barrier
//     before the chain reduction, whatever K is (512 k per pass);
//   * bias / ReLU / raw K-slice partials / N segments as in gemm_f32_mfma's epilogue; no residual, no second input block, no
//     statistics (tiling_fits keeps such products on the 32 x 32 instances).
//
// NB = 16-column blocks per workgroup (the workgroup's tile is 16 x 16 NB).
#pragma once

constexpr int kRows16Ldt = 132;          // LDS row stride (floats): 128 k of one chain + 4 (operand reads: two-way bank conflicts at most)
constexpr int kRows16Chunk = 512;        // k per pass: 16 periods of four 8-deep groups, one group per chain

// Grid: x = column tile over all segments, y = row tile (times the tuner's co-running copies), z = K slice.  The LDS regions allow
// one workgroup (NB = 2) or two (NB = 1) per CU, so a wave may hold every load of a pass in registers: amdgpu_waves_per_eu says so
// (without it hipcc budgets for eight waves per SIMD and serialises the loads behind 78 registers).
template <int NB>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) void gemm_rows16_f32(GemmArgs p, int tiles_m, int tiles_n_per_seg, int kslice) {
#include "bodies/gemm_rows16_f32.inc"
}

// The gated instance (GemmLaunchOpts::gate, ovc_beam_search_gated).
template <int NB>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) void gemm_rows16_f32_gated(GemmArgs p, int tiles_m, int tiles_n_per_seg,
                                                                                                         int kslice, const int32_t* __restrict__ gate) {
    if (ovc_gate_closed(gate)) return;
#include "bodies/gemm_rows16_f32.inc"
}
