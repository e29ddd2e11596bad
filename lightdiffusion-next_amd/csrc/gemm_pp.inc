// "Ping-pong" GEMM / implicit-GEMM main loop for large problems (included by gemm.hip, inside namespace ldx).
//
// 256 x BN tile (BN = 128 / 160 / 256), 512 threads = 8 waves as 4 (M) x 2 (N), 64 x BN/2 per wave, one workgroup per CU, all
// 160 KiB of LDS.  Measured 1.45-1.49 PFLOP/s at 8192^3 bf16 on random data (profiles/ubench/gemm_pp.hip) against 0.85 for the
// register-staged 128 x 128 kernel of gemm.hip.  What changes:
//  * operands go global -> LDS by LDS-DMA (buffer_load_dwordx4 ... lds, 1 KiB per wave-instruction: no VGPR staging, no
//    ds_write pass).  The DMA writes lane l at base + 16 l, so the LDS image keeps the 128-B rows and the 16-B-chunk XOR
//    swizzle of the kernel above by swizzling the SOURCE: lane (row l >> 3, position l & 7) fetches chunk (l & 7) ^ (row & 7).
//    Rows outside M / N / the conv halo use an out-of-range buffer offset and land as zeros, exactly like the register path.
//  * LDS is a ring of five 32-KiB half-tiles in the order A(0) W(0) A(1) W(1) ...  Phase p (two per K-tile) issues half-tile
//    p + 4 into the slot half-tile p - 1 occupied, reads its fragments from half-tiles p / p + 1, and waits with a COUNTED
//    vmcnt until half-tile p + 2 has landed: two to three half-tiles (64-96 KiB per CU) stay in flight across the barriers.
//  * waves 0-3 and 4-7 (one of each on every SIMD) run the same phase sequence ONE BARRIER APART: while one group issues the
//    MFMAs of a phase out of registers, the other does its ds_reads, DMA issue and waits for the next phase.
// Hazards (b_n = n-th workgroup barrier; group 0 runs mem(p) before b_2p and its MFMAs after it, group 1 one barrier later):
//  RAW  half-tile p + 2 is waited for by every wave inside mem(p) (group 0 before b_2p, group 1 before b_2p+1) and first read
//       in mem(p + 1), which group 0 starts after b_2p+1;
//  WAR  the slot of half-tile p - 1 is refilled in mem(p); its last reads (mem(p - 1), completed by lgkmcnt(0) before the
//       barrier that ends that part) precede b_2p-1 for both groups, and group 0 issues the refill after b_2p-1.
// Descriptors, the DMA itself and the counted wait are make_srd / lds_dma16 / lds_dma4 / vm_wait of ldx_device.h.
constexpr int PP_HALF = 256 * 128, PP_NSLOT = 5, PP_GM = 4;
constexpr int PP_LDS = PP_NSLOT * PP_HALF;

// F8: MX fp8 operands (GemmArgs::f8; plain mode, BN <= 192 or BN = 224).  A K-tile is still 128 B per row = 128 k, ONE block-scaled 16x16x128 MFMA per
// (i, j) and K-tile; the E8M0 scale dwords of the K-tile (256 for the A rows, BN for the W rows) ride in the unused tail of the W
// half-tile's ring slot: one extra 4-byte-per-lane DMA per wave and K-tile (waves 0-3 the A rows, waves 4-7 the W rows), read back with
// ds_read_b32 beside the fragments (lane group g4 uses byte g4, see mfma16_mx).
// BN = 224 (SX): the widest W half-tile that still leaves room for the 2 KiB of scales in a 32-KiB slot.  Its fourth W DMA round only has
// rows 192..223, i.e. work for waves 0-3; waves 4-7 spend that instruction on the scales instead, as ONE 16-byte-per-lane DMA of 256
// consecutive row dwords (even waves the A rows, odd waves the W rows; the two copies of each write identical bytes), so that every wave
// still issues exactly LB instructions per W half-tile and the counted vmcnt holds.  Scale rows past M / N read whatever follows them
// in the scale array (or zeros past its end): they only ever meet zero-filled operand rows of outputs that are not stored.
//
// MODE 2 (GemmArgs::up2x): the nearest-2x upsample + 3x3 conv as four 2 x 2 convs over the stored image, one per output parity (py, px), in one launch.  The loader, ring
// and MFMA loop are MODE 1's; the tap walk is 2 x 2 from (oy - (1 - py), ox - (1 - px)), rows are the M / 4 pixels of the STORED image, and the launch has four times the
// tile rows, each a (phase, row band) pair; the W panel of phase 2 py + px starts phase * N * K elements into the phase weights.  Two orders of the tile rows:
//  * up2x = 2, phase-major (what the planner asks for): the grouped order below then hands an XCD row bands of ONE phase, so its L2 streams one of the four weight matrices;
//  * up2x = 1, band-major: a band's four phases form one group of PP_GM = 4 tile rows and share their A rows in one XCD's L2, but every XCD streams all four matrices.
// The weights are the larger operand: per launch the phase-major order fetches 0.71x / 0.76x of what the 9-tap op fetches (FETCH_SIZE, SD1.5 1024^2: 32^2 -> 64^2 C 1280 /
// 64^2 -> 128^2 C 640), the band-major order 1.71x / 1.79x; the times are within 1.5 % of each other (profiles/upconv_phase/README.md).  The output stage maps a row back to
// its pixel (gemm_epilogue_up2x).  A compile-time variant: a runtime branch in the tap walk put the tap state of MODE 1 into scratch.
template <typename T, int MODE, int BN, bool LNF = false, bool F8 = false>
__device__ __forceinline__ void gemm_pp_body(const GemmArgs& p, const int block) {
    constexpr bool CONV = MODE != 0, PH = MODE == 2;
    static_assert(!PH || (!LNF && !F8 && PP_GM == 4), "phase-form up conv: 16-bit operands; band-major order: a band's four phases form one tile-row group");
    constexpr int BM = 256, WM = 4, MI = 4, NJ = BN / 32, NJ0 = (NJ + 1) / 2, LB = (BN + 63) / 64;
    constexpr int OOB = (int)0x80000000;
    static_assert(!F8 || (MODE == 0 && !LNF && (BN <= 192 || BN == 224)), "MX fp8 ping-pong tiles: plain GEMM, scales in the W slot's tail");
    constexpr bool SX = F8 && BN == 224;
    constexpr int ES = F8 ? 1 : 2;              // bytes per element
    constexpr int KE = 128 / ES, CE = 16 / ES;  // elements per K-tile / per 16-B chunk
    constexpr int LW = LB + ((F8 && !SX) ? 1 : 0);       // DMA instructions per wave for a W half-tile (+ its scales)
    constexpr int SC_OFF = SX ? BN * 128 : LB * 64 * 128;       // F8: scale area inside the W slot, behind the LB * 64 rows the W DMAs write (rows >= BN land as zeros): 256 A-row dwords, then the W-row dwords
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using V8 = typename Vec<T>::v8;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    LDX_PP_STAMP(0);
    const int grp = wave >> 2;
    const int wm = wave >> 1, wn = wave & 1;
    const int l15 = lane & 15, g4 = lane >> 4;

    const int M = PH ? p.M >> 2 : p.M;           // rows of one problem (PH: of one phase = the pixels of the stored images)
    const int tiles_n = (p.N + BN - 1) / BN, tiles_m = (PH ? 4 : 1) * ((M + BM - 1) / BM), ntiles = tiles_m * tiles_n;
    const int S = p.splitk > 1 ? p.splitk : 1;
    const int lin = xcd_remap(block, ntiles * S);
    const int bid = lin % ntiles, split = lin / ntiles;
    // grouped order: PP_GM tile rows at a time, column-major inside the group, so that the ~32 tiles an XCD runs at once form a
    // compact 2-D block of the output (fewer distinct A / W panels per L2: 8192^3 1.33 -> 1.49 PFLOP/s)
    const int gsz = PP_GM * tiles_n, gi = bid / gsz, within = bid - gi * gsz;
    const int gm_eff = min(PP_GM, tiles_m - gi * PP_GM);
    const int tm = gi * PP_GM + within % gm_eff, tn = within / gm_eff;
    // PH: tile row tm of the launch -> (phase, row band).  up2x = 1: band-major, tm = 4 band + phase; up2x = 2: phase-major, tm = phase * bands + band
    int phase = 0, band = tm;
    if (PH) {
        const int bands = tiles_m >> 2;
        if (p.up2x == 2) { phase = tm / bands; band = tm - phase * bands; } else { phase = tm & 3; band = tm >> 2; }
    }
    const int py = phase >> 1, px = phase & 1;
    const int m0 = band * BM, n0 = tn * BN;
    const int nk_all = (p.K + KE - 1) / KE;
    const int kt_begin = (int)((long)split * nk_all / S), kt_end = (int)((long)(split + 1) * nk_all / S);
    const int nk = kt_end - kt_begin;

    // ---- descriptors and per-lane offsets (same windows / zero-padding rules as gemm_tile_body) ----
    const int srow = tid >> 3;                       // + 64 j: the row of this lane in DMA instruction j of its wave
    const int gchunk = (lane & 7) ^ (srow & 7);      // source chunk that belongs at LDS position lane & 7 of that row
    const char* __restrict__ Ap = (const char*)p.A;
    const char* __restrict__ Wp = (const char*)p.W;
    const int wrow = PH ? p.Win : p.Wout;       // pixels per row of the image the GEMM rows walk
    const int hw = CONV ? (PH ? p.Hin : p.Hout) * wrow : 1;
    const int b0 = CONV ? m0 / hw : 0;
    const long img = (long)p.Hin * p.Win * p.lda;
    int row0 = 0;
    if (CONV) {
        const int oy0 = (m0 - b0 * hw) / wrow;
        row0 = max(oy0 * p.stride - (p.pad0 ? 0 : 1), 0);
        if (p.resize) row0 = min((int)floorf((float)row0 * ((float)p.Hin / (float)p.Hv)), p.Hin - 1);
    }
    const long a_base = (MODE == 0) ? (long)m0 * p.lda : (long)b0 * img + (long)row0 * p.Win * p.lda;
    const long a_total = (MODE == 0) ? (long)(p.M - 1) * p.lda + p.K : ((long)(M / hw) * p.Hin * p.Win - 1) * p.lda + p.Cin;
    const i32x4 rA = make_srd(Ap + a_base * ES, (a_total - a_base) * ES);
    const i32x4 rW = make_srd(Wp + ((long)phase * p.N + n0) * p.K * ES, ((long)p.N * p.K - (long)n0 * p.K) * ES);
    // F8: this wave's scale stream (waves 0-3: 64 A rows each, waves 4-7: 64 W rows each)
    const bool sc_w = SX ? (wave & 1) : grp;
    const i32x4 rS = !F8 ? rA : sc_w ? make_srd(p.SW + n0, ((long)nk_all * p.sw_ld - n0) * 4) : make_srd(p.SA + m0, ((long)nk_all * p.sa_ld - m0) * 4);
    const int sc_row = (wave & 3) * 64 + lane;
    const int sc_voff = !F8 ? OOB : SX ? lane * 16 : grp ? ((sc_row < BN && n0 + sc_row < p.N) ? sc_row * 4 : OOB) : ((m0 + sc_row < p.M) ? sc_row * 4 : OOB);
    const int sc_ld4 = F8 ? (sc_w ? p.sw_ld : p.sa_ld) * 4 : 0;
    const bool has_a2 = (MODE == 1) && p.A2 != nullptr;
    const i32x4 rA2 = make_srd(has_a2 ? (const char*)p.A2 + (long)m0 * p.lda2 * 2 : Ap, has_a2 ? ((long)(p.M - m0 - 1) * p.lda2 + p.Cin2) * 2 : 0);

    int a_voff[4], a_pix[4], a_oy[4], a_ox[4], a2_voff[4], w_voff[LB];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int m = m0 + srow + 64 * j;
        const bool ok = m < M;
        if (MODE == 0) {
            a_voff[j] = ok ? ((srow + 64 * j) * p.lda + gchunk * CE) * ES : OOB;
            a_pix[j] = a_oy[j] = a_ox[j] = 0;
            a2_voff[j] = OOB;
        } else {
            const int b = m / hw, rem = m - b * hw;
            const int oy = rem / wrow, ox = rem - oy * wrow;
            a_pix[j] = ok ? (int)(((long)(b - b0) * img + gchunk * 8) * 2) : OOB;
            a_oy[j] = PH ? oy - (1 - py) : oy * p.stride - (p.pad0 ? 0 : 1);
            a_ox[j] = PH ? ox - (1 - px) : ox * p.stride - (p.pad0 ? 0 : 1);
            a_voff[j] = OOB;
            a2_voff[j] = (has_a2 && ok) ? ((srow + 64 * j) * p.lda2 + gchunk * 8) * 2 : OOB;
        }
    }
#pragma unroll
    for (int j = 0; j < LB; ++j) {
        const int r = srow + 64 * j;
        w_voff[j] = (n0 + r < p.N && r < BN) ? (r * p.K + gchunk * CE) * ES : OOB;
    }
    const float rs_y = (MODE == 1 && p.resize) ? (float)p.Hin / (float)p.Hv : 1.f;
    const float rs_x = (MODE == 1 && p.resize) ? (float)p.Win / (float)p.Wv : 1.f;
    int st_ky = 0, st_kx = 0, st_ci = 0;        // conv tap state: issue_a() is called with kt = 0, 1, 2, ... in order
    bool st_new_tap = true;
    if (MODE == 1 && kt_begin > 0) {
        const int k0 = kt_begin * BK, tap = k0 / p.Cin;
        if (tap >= 9) { st_ky = 3; st_kx = 0; st_ci = k0 - 9 * p.Cin; }
        else { st_ci = k0 - tap * p.Cin; st_ky = tap / 3; st_kx = tap - st_ky * 3; }
    }
    const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
    const unsigned lds0 = lds_base + wave * 1024;     // + slot * PP_HALF + j * 8192

    auto issue_a = [&](int kt, int slot) __attribute__((always_inline)) {
        const unsigned dst = lds0 + slot * PP_HALF;
        const int k0 = (kt_begin + kt) * KE;
        if (MODE == 0) {
            const bool kdead = (k0 + KE > p.K) && (k0 + gchunk * CE >= p.K);      // ragged last K-tile: chunks past K land as 0
#pragma unroll
            for (int j = 0; j < 4; ++j) lds_dma16(rA, kdead ? OOB : a_voff[j], k0 * ES, dst + j * 8192);
        } else {
            const bool seg2 = !PH && st_ky == 3;       // second input (GemmArgs::A2): a 10th "tap" over plain rows (wave-uniform)
            if (st_new_tap) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    int iy = a_oy[j] + st_ky, ix = a_ox[j] + st_kx;
                    const bool ok = a_pix[j] != OOB && iy >= 0 && iy < p.Hv && ix >= 0 && ix < p.Wv;
                    if (!PH && p.resize) {   // nearest: src = min(floor(dst * in/out), in-1)  (torch upsample_nearest)
                        iy = min((int)floorf((float)iy * rs_y), p.Hin - 1);
                        ix = min((int)floorf((float)ix * rs_x), p.Win - 1);
                    }
                    const int v = ok ? a_pix[j] + ((iy - row0) * p.Win + ix) * p.lda * 2 : OOB;
                    a_voff[j] = seg2 ? a2_voff[j] : v;
                }
            }
            const int soff = st_ci * 2;
            const i32x4 rr = seg2 ? rA2 : rA;
#pragma unroll
            for (int j = 0; j < 4; ++j) lds_dma16(rr, a_voff[j], soff, dst + j * 8192);
            st_ci += BK;
            st_new_tap = false;
            if (!seg2 && st_ci >= p.Cin) { st_ci = 0; st_new_tap = true; if (++st_kx == (PH ? 2 : 3)) { st_kx = 0; ++st_ky; } }
        }
    };
    auto issue_w = [&](int kt, int slot) __attribute__((always_inline)) {
        const unsigned dst = lds0 + slot * PP_HALF;
        const int k0 = (kt_begin + kt) * KE;
        const bool kdead = (MODE == 0) && (k0 + KE > p.K) && (k0 + gchunk * CE >= p.K);
#pragma unroll
        for (int j = 0; j < LB; ++j) {
            if (SX && j == LB - 1 && grp) lds_dma16(rS, sc_voff, (kt_begin + kt) * sc_ld4, lds_base + slot * PP_HALF + SC_OFF + (wave & 1) * 1024);
            else lds_dma16(rW, kdead ? OOB : w_voff[j], k0 * ES, dst + j * 8192);
        }
        if constexpr (F8 && !SX) lds_dma4(rS, sc_voff, (kt_begin + kt) * sc_ld4, lds_base + slot * PP_HALF + SC_OFF + grp * 1024 + (wave & 3) * 256);
    };

    // fragment read offsets: logical chunk q of row r lives at r * 128 + ((q ^ (r & 7)) << 4), q = 4 ks + g4; the ks = 1 offset is ^ 64
    const int fx = (g4 ^ (l15 & 7)) << 4;
    const int a_off = (wm * 64 + l15) * 128 + fx;            // + i * 2048
    const int b_off = (wn * (BN / 2) + l15) * 128 + fx;      // + j * 2048

    f32x4 acc[MI][NJ];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    f32x4 lnacc[LNF ? MI : 1];
#pragma unroll
    for (int i = 0; i < (LNF ? MI : 1); ++i) lnacc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};

    LDX_PP_STAMP(1);
    issue_a(0, 0); issue_w(0, 1);
    if (nk > 1) {
        issue_a(1, 2); issue_w(1, 3);
        vm_wait<4 + LW>();
    } else {
        vm_wait<0>();
    }
    asm volatile("s_barrier" ::: "memory");
    LDX_PP_STAMP(2);
    if (grp == 1) asm volatile("s_barrier" ::: "memory");

    V8 af[F8 ? 1 : MI][2], bf[F8 ? 1 : NJ0][2];
    uint4 aq[F8 ? MI : 1][2], bq[F8 ? NJ0 : 1][2];      // F8: the two 16-B halves of a 32-byte operand (k 16 g4.. and 64 + 16 g4..)
    int csa[F8 ? MI : 1], csb[F8 ? NJ0 : 1];            // F8: scale dwords, own block's byte moved to bits 0..7
    int slot = 0;                     // ring slot of half-tile 2 t (= A of K-tile t); W of K-tile t sits in the next one
    for (int t = 0; t < nk; ++t) {
        const int slot1 = slot + 1 >= PP_NSLOT ? slot + 1 - PP_NSLOT : slot + 1;
        const char* sa = smem + slot * PP_HALF;
        const char* sb = smem + slot1 * PP_HALF;
        const bool more = t + 2 < nk;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int j0 = h ? NJ0 : 0, nj = h ? NJ - NJ0 : NJ0;
            // ---------------- memory part: DMA issue for half-tile p + 4, fragment reads of phase p ----------------
            if (more) {     // half-tile p + 4 takes the slot of half-tile p - 1
                if (h == 0) issue_a(t + 2, slot == 0 ? PP_NSLOT - 1 : slot - 1);
                else issue_w(t + 2, slot);
            }
            if (h == 0) {
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) {
                        const uint4 u = *(const uint4*)(sa + ((a_off + i * 2048) ^ (ks * 64)));
                        if constexpr (F8) aq[i][ks] = u; else af[i][ks] = as_v8<T>(u);
                    }
                if constexpr (F8) {
#pragma unroll
                    for (int i = 0; i < MI; ++i) csa[i] = (int)(*(const uint32_t*)(sb + SC_OFF + (wm * 64 + i * 16 + l15) * 4) >> (8 * g4));
                }
            }
#pragma unroll
            for (int j = 0; j < NJ0; ++j)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
                    if (j < nj) {
                        const uint4 u = *(const uint4*)(sb + ((b_off + (j0 + j) * 2048) ^ (ks * 64)));
                        if constexpr (F8) bq[j][ks] = u; else bf[j][ks] = as_v8<T>(u);
                    }
            if constexpr (F8) {
#pragma unroll
                for (int j = 0; j < NJ0; ++j)
                    if (j < nj) csb[j] = (int)(*(const uint32_t*)(sb + SC_OFF + 1024 + (wn * (BN / 2) + (j0 + j) * 16 + l15) * 4) >> (8 * g4));
            }
            if (more) vm_wait<4 + LW>();
            else vm_wait<0>();
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            // ---------------- compute part: registers only ----------------
            __builtin_amdgcn_s_setprio(1);
            if constexpr (F8) {
                auto op8 = [](const uint4& lo, const uint4& hi) { return (i32x8){(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w}; };
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < NJ0; ++j)
                        if (j < nj) acc[i][j0 + j] = mfma16_mx(op8(bq[j][0], bq[j][1]), op8(aq[i][0], aq[i][1]), acc[i][j0 + j], csb[j], csa[i]);
            } else
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < NJ0; ++j)
                        if (j < nj) acc[i][j0 + j] = mfma16(bf[j][ks], af[i][ks], acc[i][j0 + j]);
            if constexpr (LNF) {           // folded LayerNorm: row sums (wn = 0) / sums of squares (wn = 1) from the A fragments, once per K-tile
                if (h == 0) {
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                        for (int i = 0; i < MI; ++i) lnacc[i] = mfma16(wn ? af[i][ks] : ones_v8<T>(), af[i][ks], lnacc[i]);
                }
            }
            __builtin_amdgcn_s_setprio(0);
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_barrier" ::: "memory");
        }
        slot = slot + 2 >= PP_NSLOT ? slot + 2 - PP_NSLOT : slot + 2;
    }
    if (grp == 0) asm volatile("s_barrier" ::: "memory");
    LDX_PP_STAMP(3);

    if constexpr (LNF) {
        float ln1[MI], ln2[MI];
        __syncthreads();            // both wave groups are past their last fragment reads; no DMA is in flight (the loop ended on vmcnt(0))
        ln_exchange<MI, BM>(lnacc, (float*)smem, wm * 64, wn, l15, g4, p.K, p.ln_eps, ln1, ln2);
        gemm_epilogue<T, BM, BN, WM, MI, NJ, true>(p, acc, m0, n0, wm, wn, l15, g4, split, S, ln1, ln2);
    } else if constexpr (PH) {
        gemm_epilogue_up2x<T, BM, BN, WM, MI, NJ>(p, acc, m0, n0, wm, wn, l15, g4, phase);
    } else {
        gemm_epilogue<T, BM, BN, WM, MI, NJ, false, !F8>(p, acc, m0, n0, wm, wn, l15, g4, split, S);
    }
    LDX_PP_STAMP(6);
    LDX_PP_STAMP(4);
}

template <typename T, int MODE, int BN, bool LNF = false, bool F8 = false>
__global__ __launch_bounds__(512, 2) void gemm_pp_kernel(const GemmArgs p) {
    gemm_pp_body<T, MODE, BN, LNF, F8>(p, blockIdx.x);
}

// two independent plain GEMMs in one launch (see gemm2_kernel): the second problem's tiles are appended to the first's
template <typename T, int BN, bool F8 = false>
__global__ __launch_bounds__(512, 2) void gemm_pp2_kernel(const GemmArgs a, const GemmArgs b, const int tiles_a) {
    if ((int)blockIdx.x < tiles_a) gemm_pp_body<T, 0, BN, false, F8>(a, blockIdx.x);
    else gemm_pp_body<T, 0, BN, false, F8>(b, blockIdx.x - tiles_a);
}

template <typename T, int MODE, int BN, bool LNF = false, bool F8 = false>
static void launch_pp_inst(const GemmArgs& a, int S, hipStream_t s) {
    const int tiles = (MODE == 2 ? 4 * ((a.M / 4 + 255) / 256) : (a.M + 255) / 256) * ((a.N + BN - 1) / BN) * S;      // MODE 2: four phases of M / 4 rows each
    static DevOnce once;
    set_dyn_lds(once, (const void*)gemm_pp_kernel<T, MODE, BN, LNF, F8>, PP_LDS);
    hipLaunchKernelGGL((gemm_pp_kernel<T, MODE, BN, LNF, F8>), dim3(tiles), dim3(512), PP_LDS, s, a);
}
template <typename T, int BN, bool F8 = false>
static void launch_pp2_inst(const GemmArgs& a, const GemmArgs& b, hipStream_t s) {
    const int ta = ((a.M + 255) / 256) * ((a.N + BN - 1) / BN), tb = ((b.M + 255) / 256) * ((b.N + BN - 1) / BN);
    static DevOnce once;
    set_dyn_lds(once, (const void*)gemm_pp2_kernel<T, BN, F8>, PP_LDS);
    hipLaunchKernelGGL((gemm_pp2_kernel<T, BN, F8>), dim3(ta + tb), dim3(512), PP_LDS, s, a, b, ta);
}
