// The body of the fp32 MFMA kernels (gemm.hip): included verbatim into gemm_f32_mfma and gemm_f32_mfma_score, which differ only in
// OVC_GEMM_F32_EPILOGUE, the statement that stores the wave's finished accumulator tiles.  Not a header: no include guard.
    using Cfg = TileConfig<BM, BN, WM, WN, WK, BK, NC>;
    constexpr int LDT = Cfg::LDT;
    constexpr int kVecPerRow = BK / 4;               // float4 per tile row
    constexpr int kRowsPerPass = 256 / kVecPerRow;   // tile rows covered by one pass of the 256 loader threads
    extern __shared__ __attribute__((aligned(16))) float lds[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wk = wave / (WM * WN);
    const int wm = (wave / WN) % WM, wn = wave % WN;

    // ---- ONE scalar round trip: the tile map and every argument the first tile's loads (and the epilogue's addresses) depend on.
    //      The empty asm pins them in SGPRs here, so hipcc issues all the s_loads back to back in front of it instead of
    //      sinking each next to its first use behind the previous one's wait (five dependent rounds before round 4). ----
    const TileMap t = tmap;
    const float* const a1_ptr = p.A1;
    const float* const w0_ptr = p.seg[0].W;
    const float* const bias0_ptr = p.seg[0].bias;
    float* const c0_ptr = p.seg[0].C;
    const float* const a2_shared = p.A2;
    uint8_t* const zero_rows_ptr = p.zero_rows_out;
    const int arg_lda1 = p.lda1, arg_lda2 = p.lda2, arg_K1 = p.K1, arg_K2 = p.K2, arg_M = p.M, arg_seg_n = p.seg_n, arg_nseg = p.nseg;
    // (one statement: one s_waitcnt; "what the epilogue addresses with" rides along -- otherwise one more round trip behind the K loop)
    asm volatile("" ::"s"(t.nwg), "s"(t.tiles_m), "s"(t.tiles_n_all), "s"(t.tiles_n_per_seg), "s"(t.xcd_pm), "s"(t.pm_shift), "s"(t.sub_m),
                 "s"(t.sub_n), "s"(t.sub_m_magic), "s"(t.seg_magic), "s"(t.group_m), "s"(t.group_size), "s"(t.gm_last),
                 "s"(t.group_size_magic), "s"(t.group_m_magic), "s"(t.gm_last_magic), "s"(t.kslice), "s"(a1_ptr), "s"(w0_ptr),
                 "s"(bias0_ptr), "s"(c0_ptr), "s"(arg_lda1), "s"(arg_K1), "s"(arg_K2), "s"(arg_M), "s"(arg_seg_n), "s"(arg_nseg),
                 "s"(a2_shared), "s"(zero_rows_ptr), "s"(arg_lda2), "s"(p.R), "s"(p.ldc), "s"(p.ldr), "s"(p.res_mod), "s"(p.act),
                 "s"(p.part_stride), "s"(p.stats), "s"(p.stats_t), "s"(p.stats_ld));

    int tile_m, tile_n_all;
    tile_coords_fast(t, (int)blockIdx.x, tile_m, tile_n_all);
    const int seg = arg_nseg == 1 ? 0 : fast_div(tile_n_all, t.seg_magic, t.tiles_n_per_seg);
    const int tile_n = tile_n_all - seg * t.tiles_n_per_seg;
    const int m0 = tile_m * BM, n0 = tile_n * BN;

    // single-segment products (every decode-step product but q|k|v): the segment's pointers came with the first round trip.
    // (Fetching the first THREE segments' pointers that way as well -- q|k|v -- measured slower: 18.4k against 18.6k captions/s
    // on one stream, 24.52k against 24.63k on four; the longer first batch delays everything else.)
    const float* __restrict__ W = arg_nseg == 1 ? w0_ptr : p.seg[seg].W;
    const float* __restrict__ seg_bias = arg_nseg == 1 ? bias0_ptr : p.seg[seg].bias;
    float* __restrict__ seg_C = arg_nseg == 1 ? c0_ptr : p.seg[seg].C;
    const int K = arg_K1 + arg_K2;
    // Cross-workgroup K split (gridDim.y slices): this workgroup covers [kbase, kbase + K / gridDim.y) and writes a
    // raw partial tile.  It halves / quarters the operand bytes a CU pulls through its L2 port for the M = 1280
    // decode shapes, whose 32x32 tiles are bound by that port rather than by the matrix cores.
    const int kslice = t.kslice;
    const int kbase = (int)blockIdx.y * kslice;
    const int nkt = (kslice + BK - 1) / BK;

    constexpr int kBufFloats = (BM + BN) * LDT;   // one buffer: A tile then B tile

    f32x4 stage_a[Cfg::kLoadA], stage_b[Cfg::kLoadB];

    // Branch-free tile loads: a runtime "load or zero" choice per element makes hipcc branch around
    // every load and wait vmcnt(0) in between (serialised L2 round trips).  Instead the address is
    // clamped in-bounds and the load is unconditional; a K tail (never present in the model shapes) is
    // zeroed when the registers are written to LDS.  Which of A1 / A2 a K tile comes from is
    // wave-uniform because K1 is a multiple of BK whenever K2 > 0.
    const bool k_tail = (K % BK) != 0 || (p.K1 % BK) != 0;   // uniform; false for every real shape
    bool a_ok = true, w_ok = true;

    // Tile loads are raw buffer loads: the per-lane byte offset (row * ld + 4-float column group) is fixed for
    // the whole K loop and the K position travels in the instruction's scalar offset, so the loop spends no
    // vector instructions on addresses (+4..5 % on the 128x128 loop, tools/gemm_ablation.hip).  Rows past M / N
    // fall outside the descriptor's range and read as zero; a K tail is zeroed when the registers go to LDS.
    const __amdgpu_buffer_rsrc_t rsrc_a1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a1_ptr), 0, arg_M * arg_lda1 * 4, 0x00020000);
    // per-segment second block (meshed level gates); the segment table is only consulted when there IS a second block
    const float* a2 = arg_K2 ? (p.seg[seg].A2 ? p.seg[seg].A2 : a2_shared) : a1_ptr;
    const __amdgpu_buffer_rsrc_t rsrc_a2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a2), 0,
                                                                              arg_K2 ? arg_M * arg_lda2 * 4 : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrc_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(W), 0, arg_seg_n * K * 4, 0x00020000);
    int off_a1[Cfg::kLoadA], off_a2[Cfg::kLoadA], off_w[Cfg::kLoadB];
    {
        const int kq = tid % kVecPerRow;
#pragma unroll
        for (int i = 0; i < Cfg::kLoadA; ++i) {
            const int row = m0 + tid / kVecPerRow + i * kRowsPerPass;
            off_a1[i] = (row * arg_lda1 + kq * 4) * 4;
            off_a2[i] = (row * arg_lda2 + kq * 4) * 4;
        }
#pragma unroll
        for (int i = 0; i < Cfg::kLoadB; ++i) off_w[i] = ((n0 + tid / kVecPerRow + i * kRowsPerPass) * K + kq * 4) * 4;
    }
    auto load_tile = [&](int kt) {
        const int k0 = kbase + kt * BK;
        const bool second = k0 >= p.K1;                       // uniform: which of A1 | A2 this K tile comes from
        if (k_tail) {
            const int kq = tid % kVecPerRow;
            a_ok = (second ? k0 - p.K1 : k0) + kq * 4 < (second ? p.K2 : p.K1);
            w_ok = k0 + kq * 4 < K;
        }
        if (!second) {
#pragma unroll
            for (int i = 0; i < Cfg::kLoadA; ++i)
                stage_a[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_a1, off_a1[i], k0 * 4, 0));
        } else {
#pragma unroll
            for (int i = 0; i < Cfg::kLoadA; ++i)
                stage_a[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_a2, off_a2[i], (k0 - p.K1) * 4, 0));
        }
#pragma unroll
        for (int i = 0; i < Cfg::kLoadB; ++i)
            stage_b[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_w, off_w[i], k0 * 4, 0));
    };
    // The loaded registers are first touched here, after the MFMA block of the previous tile, so the
    // global-load latency hides under the matrix work (issue early / write late).
    // K1 fold (GemmArgs::zero_rows_out): the workgroups of the first column tile add up the A rows they stage anyway
    const bool row_sums = zero_rows_ptr != nullptr && tile_n_all == 0;        // uniform
    float rs[Cfg::kLoadA];
#pragma unroll
    for (int i = 0; i < Cfg::kLoadA; ++i) rs[i] = 0.f;
    auto store_tile = [&](int buf) {
        const int kq = tid % kVecPerRow;
        if (k_tail) {
#pragma unroll
            for (int i = 0; i < Cfg::kLoadA; ++i)
                if (!a_ok) stage_a[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < Cfg::kLoadB; ++i)
                if (!w_ok) stage_b[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        if (row_sums) {
#pragma unroll
            for (int i = 0; i < Cfg::kLoadA; ++i) rs[i] += (stage_a[i][0] + stage_a[i][1]) + (stage_a[i][2] + stage_a[i][3]);
        }
#pragma unroll
        for (int i = 0; i < Cfg::kLoadA; ++i) {
            const int row = tid / kVecPerRow + i * kRowsPerPass;
            *reinterpret_cast<f32x4*>(lds + buf * kBufFloats + row * LDT + kq * 4) = stage_a[i];
        }
#pragma unroll
        for (int i = 0; i < Cfg::kLoadB; ++i) {
            const int row = tid / kVecPerRow + i * kRowsPerPass;
            *reinterpret_cast<f32x4*>(lds + buf * kBufFloats + (BM + row) * LDT + kq * 4) = stage_b[i];
        }
    };

    f32x16 acc[NC][Cfg::TM][Cfg::TN];
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
            for (int j = 0; j < Cfg::TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[c][i][j][r] = 0.f;

    const int frag_row = lane & 31;
    const int frag_k = (lane >> 5) * 4;

    // the MFMA block of one K tile (LDS buffer `buf`)
    auto compute_tile = [&](int buf) {
        const float* a_base = lds + buf * kBufFloats + (wm * Cfg::kWaveM + frag_row) * LDT + frag_k;
        const float* b_base = lds + buf * kBufFloats + (BM + wn * Cfg::kWaveN + frag_row) * LDT + frag_k;
        // 8-deep k-groups of this K tile, in order.  One chain: every group goes to accumulator set 0.  Four chains:
        // group kk belongs to chain kk & 3 (K tiles and K slices start on multiples of 32, so this is the global
        // group index mod 4); this wave owns chains wk + WK * c, kept in set c.
        constexpr int kGroupsPerWave = Cfg::kChains == 1 ? BK / 8 : (BK / 32) * NC;
#pragma unroll
        for (int g = 0; g < kGroupsPerWave; ++g) {
            const int set = Cfg::kChains == 1 ? 0 : g % NC;
            const int kk = Cfg::kChains == 1 ? g : 4 * (g / NC) + wk + WK * (g % NC);
            f32x4 a[Cfg::TM], b[Cfg::TN];
#pragma unroll
            for (int i = 0; i < Cfg::TM; ++i)
                a[i] = *reinterpret_cast<const f32x4*>(a_base + i * 32 * LDT + kk * 8);
#pragma unroll
            for (int j = 0; j < Cfg::TN; ++j)
                b[j] = *reinterpret_cast<const f32x4*>(b_base + j * 32 * LDT + kk * 8);
            // Raised priority around the MFMA cluster: hipcc then keeps the cluster contiguous instead of
            // threading the next tile's loads / address arithmetic through it (+8..20 % on the 128x128 loop,
            // tools/gemm_ablation.hip).
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
                    for (int j = 0; j < Cfg::TN; ++j)
                        acc[set][i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][s], b[j][s], acc[set][i][j], 0, 0, 0);
            __builtin_amdgcn_s_setprio(0);
        }
    };

    // Prefetch distance two for the tiles of up to 64 x 64 (round 3): the tile AFTER next is requested before this tile's MFMA block,
    // into a second set of staging registers, so that a K iteration no longer has to cover a whole L2 round trip -- with 16 K
    // tiles or fewer per output tile and an MFMA block of a fraction of a microsecond these loops were chains of load latencies
    // (steady state 0.94 us per 64-deep K tile where the matrix pipe needs 0.53).  Same instructions in the same order on every
    // accumulator: the bits do not change.  Measured: cross-q 12.9 -> 11.6 us, output projection 11.5 -> 10.6, q|k|v 22.6 -> 21.7,
    // FFN 27.6 -> 26.6, encoder q|k|v 160 -> 155, vocabulary^T 109.9 -> 106.3; captions/s +1.3 % (four streams), +2.7 % (one).
    // Not for the larger tiles (their second register set costs a resident workgroup: 128 x 64 160.9 -> 166.4 us) nor for the
    // K-tile-64 instances with chains in two waves (96-register cap: 13 spilled).  With two LDS buffers on top (one barrier per
    // K tile instead of two) every shape got slower again (encoder q|k|v 154.6 -> 163.8 us): LDS residency beats the barrier.
#ifdef OVC_NO_PF2                   // A/B builds only: tools/ab_bench.sh against a library compiled with -DOVC_NO_PF2
    constexpr bool kPF2 = false;
#else
    constexpr bool kPF2 = BM * BN <= 64 * 64 && Cfg::kBufs == 1 && !(WK == 2 && BK == 64);
#endif
    constexpr int kDepth = 2;       // staging register sets = tiles requested ahead (3 and 4 measured: slower on every shape --
                                    // 32x32 cross-q 11.9 / 12.6 / 12.5 us, 64x64 vocabulary^T 105.7 / 110.2 / 113.3 -- even without spills)
    bool done = false;
    if constexpr (kPF2) {
        if (!k_tail && p.K2 == 0 && !row_sums && nkt >= kDepth) {
            f32x4 sa[kDepth][Cfg::kLoadA], sb[kDepth][Cfg::kLoadB];
            auto load_set = [&](int kt, auto set_tag) {
                constexpr int S = decltype(set_tag)::value;
                const int k0 = kbase + kt * BK;
#pragma unroll
                for (int i = 0; i < Cfg::kLoadA; ++i)
                    sa[S][i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_a1, off_a1[i], k0 * 4, 0));
#pragma unroll
                for (int i = 0; i < Cfg::kLoadB; ++i)
                    sb[S][i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_w, off_w[i], k0 * 4, 0));
            };
            auto store_set = [&](auto set_tag) {
                constexpr int S = decltype(set_tag)::value;
                const int kq = tid % kVecPerRow;
#pragma unroll
                for (int i = 0; i < Cfg::kLoadA; ++i)
                    *reinterpret_cast<f32x4*>(lds + (tid / kVecPerRow + i * kRowsPerPass) * LDT + kq * 4) = sa[S][i];
#pragma unroll
                for (int i = 0; i < Cfg::kLoadB; ++i)
                    *reinterpret_cast<f32x4*>(lds + (BM + tid / kVecPerRow + i * kRowsPerPass) * LDT + kq * 4) = sb[S][i];
            };
            // tile j waits in register set j % kDepth.  One step: tile kt is in LDS and its set is free -> request tile kt + kDepth
            // into it, run tile kt's MFMA block, move tile kt + 1 (requested kDepth - 1 blocks ago) to LDS.
            auto step = [&](int kt, auto cur_tag) {
                constexpr int C = decltype(cur_tag)::value;
                if (kt + kDepth < nkt) load_set(kt + kDepth, cur_tag);
                compute_tile(0);
                if (kt + 1 < nkt) {
                    __syncthreads();
                    store_set(std::integral_constant<int, (C + 1) % kDepth>{});
                    __syncthreads();
                }
            };
            load_set(0, std::integral_constant<int, 0>{});
            if constexpr (kDepth > 1) load_set(1, std::integral_constant<int, 1 % kDepth>{});
            if constexpr (kDepth > 2) load_set(2, std::integral_constant<int, 2 % kDepth>{});
            if constexpr (kDepth > 3) load_set(3, std::integral_constant<int, 3 % kDepth>{});
            store_set(std::integral_constant<int, 0>{});
            __syncthreads();
            for (int kt = 0; kt < nkt; kt += kDepth) {
                step(kt, std::integral_constant<int, 0>{});
                if constexpr (kDepth > 1) { if (kt + 1 < nkt) step(kt + 1, std::integral_constant<int, 1 % kDepth>{}); }
                if constexpr (kDepth > 2) { if (kt + 2 < nkt) step(kt + 2, std::integral_constant<int, 2 % kDepth>{}); }
                if constexpr (kDepth > 3) { if (kt + 3 < nkt) step(kt + 3, std::integral_constant<int, 3 % kDepth>{}); }
            }
            __syncthreads();
            done = true;
        }
    }
    if (!done) {
        load_tile(0);
        store_tile(0);
        __syncthreads();
        for (int kt = 0; kt < nkt; ++kt) {
            const int buf = Cfg::kBufs == 2 ? (kt & 1) : 0;
            if (kt + 1 < nkt) load_tile(kt + 1);
            compute_tile(buf);
            if (kt + 1 < nkt) {
                if (Cfg::kBufs == 1) __syncthreads();
                store_tile(Cfg::kBufs == 2 ? (buf ^ 1) : 0);
            }
            __syncthreads();
        }
    }

    if (row_sums) {
        // the kVecPerRow consecutive lanes that staged one row hold its partial sums: butterfly inside that group
#pragma unroll
        for (int i = 0; i < Cfg::kLoadA; ++i) {
            float v = rs[i];
#pragma unroll
            for (int off = 1; off < kVecPerRow; off <<= 1) v += __shfl_xor(v, off, 64);
            const int row = m0 + tid / kVecPerRow + i * kRowsPerPass;
            if (tid % kVecPerRow == 0 && row < arg_M) zero_rows_ptr[row] = (v == 0.f) ? 1 : 0;
        }
    }

    // Chain reduction, always in chain order ((c0 + c1) + c2) + c3 whatever the wave layout: chain c lives in wave
    // c % WK, accumulator set c / WK.  Waves wk > 0 park their sets in LDS (the tile buffers are free after the last
    // barrier), wave wk == 0 adds everything up and runs the epilogue.
    if (Cfg::kChains > 1) {
        float* red = lds;
        const int wtile = wm * WN + wn;
        auto red_index = [&](int w, int c, int i, int j, int r) {
            return ((((((w - 1) * NC + c) * (WM * WN) + wtile) * Cfg::TM + i) * Cfg::TN + j) * 16 + r) * 64 + lane;
        };
        if (WK > 1) {
            if (wk > 0) {
#pragma unroll
                for (int c = 0; c < NC; ++c)
#pragma unroll
                    for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
                        for (int j = 0; j < Cfg::TN; ++j)
#pragma unroll
                            for (int r = 0; r < 16; ++r) red[red_index(wk, c, i, j, r)] = acc[c][i][j][r];
            }
            __syncthreads();
            if (wk > 0) return;
        }
#pragma unroll
        for (int chain = 1; chain < Cfg::kChains; ++chain) {
            constexpr int kW = WK;
            const int w = chain % kW, c = chain / kW;          // compile-time after unrolling
#pragma unroll
            for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
                for (int j = 0; j < Cfg::TN; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        acc[0][i][j][r] += w == 0 ? acc[c][i][j][r] : red[red_index(w, c, i, j, r)];
        }
    }

    OVC_GEMM_F32_EPILOGUE;
