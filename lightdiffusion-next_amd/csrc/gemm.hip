// MFMA GEMM / implicit-GEMM 3x3 convolution for gfx950.
//
// Replaces, on the reference hot path, every F.linear (cond/cast.py:107) and conv (cast.py:174)
// of UNetModel1 / VAE Decoder / CLIP: Linear, Conv2d 1x1, Conv2d 3x3 (stride 1|2, pad 1) and
// Upsample1's nearest-resize + conv, with the bias / time-embedding add / GEGLU / residual-add
// epilogues of ResBlock1._forward (ResBlock.py:315-335), BasicTransformerBlock._forward
// (transformer.py:186-245) and SpatialTransformer.forward (transformer.py:342-377) fused in.
//
// Tiling: 128x128 output tile per 256-thread workgroup (4 waves, 2x2, 64x64 per wave as 4x4
// MFMA 16x16x32 tiles), BK = 64, double-buffered LDS (2 x 32 KiB), register-staged global loads
// issued one K-tile ahead (cdna guide T14) so the HBM/L2 latency hides under 32 MFMAs per wave.
// LDS rows are 128 B (64 x 16-bit) with a 16-B-chunk XOR swizzle (chunk ^= row & 7), which makes
// both the ds_write_b128 staging and the ds_read_b128 fragment reads bank-conflict free.
// The MFMA is issued as D = W_frag x A_frag so each lane ends up with 4 consecutive output
// channels of one output row -> 8-byte coalesced epilogue stores into the NHWC activation.
#include <stdlib.h>
#include "gemm_common.h"
#include "ldx_switches.h"

namespace ldx {


// BM x BN workgroup tile, 4 waves as 2x2, each wave (BM/2) x (BN/2) = MI x NJ MFMA tiles of 16x16.
// 128x128 / 128x160 for large problems; 64x64 for short-K problems whose 128-wide tiling would leave most CUs
// idle (they are latency-bound: 4-5x more, smaller workgroups hide the HBM/L2 latency with thread-level parallelism).
// WM = waves along M (2: 4 waves / 256 threads, two workgroups per CU; 4: 8 waves / 512 threads with a 256-row tile, one
// workgroup per CU — 25 % fewer L2->LDS bytes per flop for the large-M problems that are bound by that traffic).
// F8: A / W are MX fp8 bytes (GemmArgs::f8): a K-tile is still 128 B per row = 128 elements, one 16x16x128 block-scaled MFMA
// per (i, j) and K-tile instead of two 16x16x32; the E8M0 scales bypass LDS (one dword per row and K-tile, prefetched with
// the tile).  Same LDS layout, staging, split-K and epilogue as the 16-bit kernel.
template <typename T, int MODE, int BM, int BN, int WM, bool F8, bool LNF = false>
__device__ __forceinline__ void gemm_tile_body(const GemmArgs& p, const int block) {
    static_assert(!F8 || MODE == 0, "MX fp8 operands: plain GEMM only");
    static_assert(!LNF || (MODE == 0 && !F8), "folded LayerNorm: plain 16-bit GEMM only");
    constexpr int ES = F8 ? 1 : 2;              // bytes per A / W element
    constexpr int KE = 128 / ES;                // elements per K-tile (= BK for 16-bit)
    constexpr int CE = 16 / ES;                 // elements per 16-B staging chunk
    constexpr int NT = WM * 128;                // threads
    constexpr int RPP = NT / 8;                 // tile rows staged per pass (8 threads x 16 B per 128-B row)
    constexpr int LA = BM / RPP, LB = (BN + RPP - 1) / RPP;   // staging chunks per thread (A rows, W rows; BN = 160 at 64 rows per pass is ragged)
    constexpr int MI = BM / WM / 16;            // 16-row MFMA tiles per wave
    constexpr int NJ = BN / 2 / 16;             // 16-column MFMA tiles per wave
    constexpr int STAGE_BYTES = stage_bytes<BM, BN>();
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using V8 = typename Vec<T>::v8;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;     // wm in [0, WM)
    const int l15 = lane & 15, g4 = lane >> 4;

    const int tiles_n = (p.N + BN - 1) / BN;   // BN = template tile width
    const int tiles_m = (p.M + BM - 1) / BM;
    const int ntiles = tiles_m * tiles_n;
    const int S = p.splitk > 1 ? p.splitk : 1;
    const int lin = xcd_remap(block, ntiles * S);
    const int bid = lin % ntiles, split = lin / ntiles;      // same-split tiles adjacent: neighbours share panels
    const int tm = bid / tiles_n, tn = bid % tiles_n;
    const int m0 = tm * BM, n0 = tn * BN;
    const int nk_all = (p.K + KE - 1) / KE;      // K % 8 == 0; a ragged last K-tile is zero-filled by the loader
    const int kt_begin = (int)((long)split * nk_all / S), kt_end = (int)((long)(split + 1) * nk_all / S);
    const int nk = kt_end - kt_begin;

    // ---- per-thread staging coordinates: 4 A chunks + NJ W chunks of 16 B per K-tile ----
    // Loads go through buffer descriptors (buffer_load_dwordx4 ... offen with an SGPR K offset): the per-lane
    // byte offsets are loop-invariant (plain GEMM) or change only when the 3x3 tap changes (conv), and rows
    // outside M / N / the zero-padding halo use an out-of-range offset, which the hardware returns as 0 —
    // no exec-mask branches, no 64-bit address arithmetic in the K loop.
    const int srow = tid >> 3;        // 0..RPP-1 (+RPP*j)
    const int schunk = tid & 7;       // 16-B chunk within the 128-B K-slice
    constexpr int OOB = (int)0x80000000;
    const char* __restrict__ Ap = (const char*)p.A;
    const char* __restrict__ Wp = (const char*)p.W;
    const int hw = (MODE == 1) ? p.Hout * p.Wout : 1;
    const int b0 = (MODE == 1) ? m0 / hw : 0;
    const long img = (long)p.Hin * p.Win * p.lda;                       // conv: elements per input image
    // conv: the buffer window starts at the first input row this tile can touch, so that in-window byte offsets
    // stay far below 2^31 even when one image is >= 2 GiB (VAE decode at 2048^2: 2048*2048*256 ch * 2 B)
    int row0 = 0;
    if (MODE == 1) {
        const int oy0 = (m0 - b0 * hw) / p.Wout;
        row0 = max(oy0 * p.stride - (p.pad0 ? 0 : 1), 0);
        if (p.resize) row0 = min((int)floorf((float)row0 * ((float)p.Hin / (float)p.Hv)), p.Hin - 1);
    }
    const long a_base = (MODE == 0) ? (long)m0 * p.lda : (long)b0 * img + (long)row0 * p.Win * p.lda;
    const long a_total = (MODE == 0) ? (long)(p.M - 1) * p.lda + p.K : ((long)(p.M / hw) * p.Hin * p.Win - 1) * p.lda + p.Cin;
    const long a_rem = (a_total - a_base) * ES;
    const long w_rem = ((long)p.N * p.K - (long)n0 * p.K) * ES;
    const __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc((void*)(Ap + a_base * ES), 0, (int)(a_rem > 0x7fffffffL ? 0x7fffffffL : a_rem), RSRC_RAW_WORD3);
    const __amdgpu_buffer_rsrc_t rW = __builtin_amdgcn_make_buffer_rsrc((void*)(Wp + (long)n0 * p.K * ES), 0, (int)(w_rem > 0x7fffffffL ? 0x7fffffffL : w_rem), RSRC_RAW_WORD3);

    int a_voff[LA];                   // plain: final byte offset ; conv: per-tap byte offset (recomputed per tap)
    int a_pix[LA];                    // conv: byte offset of this row's batch image + chunk
    int a_oy[LA], a_ox[LA];
#pragma unroll
    for (int j = 0; j < LA; ++j) {
        const int m = m0 + srow + RPP * j;
        const bool ok = m < p.M;
        if (MODE == 0) {
            a_voff[j] = ok ? ((srow + RPP * j) * p.lda + schunk * CE) * ES : OOB;
            a_pix[j] = a_oy[j] = a_ox[j] = 0;
        } else {
            const int b = m / hw, rem = m - b * hw;
            const int oy = rem / p.Wout, ox = rem - oy * p.Wout;
            a_pix[j] = ok ? (int)(((long)(b - b0) * img + schunk * 8) * 2) : OOB;
            a_oy[j] = oy * p.stride - (p.pad0 ? 0 : 1);
            a_ox[j] = ox * p.stride - (p.pad0 ? 0 : 1);
            a_voff[j] = OOB;
        }
    }
    // second conv input (GemmArgs::A2): always a defined descriptor (0 records without A2) — a conditionally initialised one sent
    // the whole conv instantiation through scratch (12 B / lane, ESRGAN 26.8 -> 33.8 ms)
    const bool has_a2 = (MODE == 1) && p.A2 != nullptr;
    const long rem2 = has_a2 ? ((long)(p.M - m0 - 1) * p.lda2 + p.Cin2) * 2 : 0;
    const __amdgpu_buffer_rsrc_t rA2 = __builtin_amdgcn_make_buffer_rsrc(
        has_a2 ? (void*)((const char*)p.A2 + (long)m0 * p.lda2 * 2) : (void*)p.A, 0, (int)(rem2 > 0x7fffffffL ? 0x7fffffffL : (rem2 > 0 ? rem2 : 0)), RSRC_RAW_WORD3);
    int a2_voff[(MODE == 1) ? LA : 1];
#pragma unroll
    for (int j = 0; j < ((MODE == 1) ? LA : 1); ++j)
        a2_voff[j] = (has_a2 && m0 + srow + RPP * j < p.M) ? ((srow + RPP * j) * p.lda2 + schunk * 8) * 2 : OOB;
    int w_voff[LB];
#pragma unroll
    for (int j = 0; j < LB; ++j) {
        const int n = n0 + srow + RPP * j;
        w_voff[j] = (n < p.N && srow + RPP * j < BN) ? ((srow + RPP * j) * p.K + schunk * CE) * ES : OOB;
    }
    const float rs_y = (MODE == 1 && p.resize) ? (float)p.Hin / (float)p.Hv : 1.f;
    const float rs_x = (MODE == 1 && p.resize) ? (float)p.Win / (float)p.Wv : 1.f;

    uint4 ra[LA], rb[LB];
    // MX scales: lane (l15, g4) of tile i needs byte g4 of dword SA[kt][m0 + wm*(BM/WM) + 16 i + l15] (same for W rows)
    uint32_t rsa[F8 ? MI : 1], rsb[F8 ? NJ : 1];
    int sa_voff[F8 ? MI : 1], sb_voff[F8 ? NJ : 1];
    __amdgpu_buffer_rsrc_t rSA, rSW;
    if (F8) {
        const long sa_rem = ((long)nk_all * p.sa_ld - m0) * 4, sw_rem = ((long)nk_all * p.sw_ld - n0) * 4;
        rSA = __builtin_amdgcn_make_buffer_rsrc((void*)(p.SA + m0), 0, (int)(sa_rem > 0x7fffffffL ? 0x7fffffffL : sa_rem), RSRC_RAW_WORD3);
        rSW = __builtin_amdgcn_make_buffer_rsrc((void*)(p.SW + n0), 0, (int)(sw_rem > 0x7fffffffL ? 0x7fffffffL : sw_rem), RSRC_RAW_WORD3);
#pragma unroll
        for (int i = 0; i < MI; ++i) { const int r = wm * (BM / WM) + i * 16 + l15; sa_voff[i] = (m0 + r < p.M) ? r * 4 : OOB; }
#pragma unroll
        for (int j = 0; j < NJ; ++j) { const int r = wn * (BN / 2) + j * 16 + l15; sb_voff[j] = (n0 + r < p.N) ? r * 4 : OOB; }
    }
    int st_ky = 0, st_kx = 0, st_ci = 0;   // conv: gload() is called with kt = 0,1,2,... in order
    bool st_new_tap = true;
    if (MODE == 1 && kt_begin > 0) {
        const int k0 = kt_begin * BK, tap = k0 / p.Cin;
        if (tap >= 9) { st_ky = 3; st_kx = 0; st_ci = k0 - 9 * p.Cin; }      // inside the second-input segment
        else { st_ci = k0 - tap * p.Cin; st_ky = tap / 3; st_kx = tap - st_ky * 3; }
    }
    auto ld128 = [](const __amdgpu_buffer_rsrc_t& r, int voff, int soff) {
        const auto v = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0);
        return make_uint4(v[0], v[1], v[2], v[3]);
    };
    auto gload = [&](int kt) __attribute__((always_inline)) {
        const int k0 = (kt_begin + kt) * KE;
        // ragged last K-tile (plain GEMM only; conv has K = 9*Cin, Cin % 64 == 0): chunks past K read as 0
        const bool kdead = (k0 + KE > p.K) && (k0 + schunk * CE >= p.K);
        if (F8) {          // out-of-range rows read scale byte 0 (2^-127) against zero-filled operands
#pragma unroll
            for (int i = 0; i < MI; ++i) rsa[i] = __builtin_amdgcn_raw_buffer_load_b32(rSA, sa_voff[i], (kt_begin + kt) * p.sa_ld * 4, 0);
#pragma unroll
            for (int j = 0; j < NJ; ++j) rsb[j] = __builtin_amdgcn_raw_buffer_load_b32(rSW, sb_voff[j], (kt_begin + kt) * p.sw_ld * 4, 0);
        }
        if (MODE == 0) {
#pragma unroll
            for (int j = 0; j < LA; ++j) ra[j] = ld128(rA, kdead ? OOB : a_voff[j], k0 * ES);
        } else {
            const bool seg2 = st_ky == 3;       // second input (GemmArgs::A2): a 10th "tap" over plain rows (wave-uniform)
            if (st_new_tap) {           // wave-uniform: once per (ky,kx) tap
#pragma unroll
                for (int j = 0; j < LA; ++j) {
                    int iy = a_oy[j] + st_ky, ix = a_ox[j] + st_kx;
                    const bool ok = a_pix[j] != OOB && iy >= 0 && iy < p.Hv && ix >= 0 && ix < p.Wv;
                    if (p.resize) {   // nearest: src = min(floor(dst * in/out), in-1)  (torch upsample_nearest)
                        iy = min((int)floorf((float)iy * rs_y), p.Hin - 1);
                        ix = min((int)floorf((float)ix * rs_x), p.Win - 1);
                    }
                    const int v = ok ? a_pix[j] + ((iy - row0) * p.Win + ix) * p.lda * 2 : OOB;
                    a_voff[j] = seg2 ? a2_voff[j] : v;
                }
            }
            const int soff = st_ci * 2;
            const __amdgpu_buffer_rsrc_t rr = seg2 ? rA2 : rA;
#pragma unroll
            for (int j = 0; j < LA; ++j) ra[j] = ld128(rr, a_voff[j], soff);
            st_ci += BK;
            st_new_tap = false;
            if (!seg2 && st_ci >= p.Cin) { st_ci = 0; st_new_tap = true; if (++st_kx == 3) { st_kx = 0; ++st_ky; } }
        }
#pragma unroll
        for (int j = 0; j < LB; ++j) rb[j] = ld128(rW, kdead ? OOB : w_voff[j], k0 * ES);
    };
    auto lstore = [&](int stage) __attribute__((always_inline)) {
        char* sA = smem + stage * STAGE_BYTES;
        char* sB = sA + BM * BK * 2;
#pragma unroll
        for (int j = 0; j < (MI > NJ ? MI : NJ); ++j) {
            const int row = srow + RPP * j;
            const int off = row * 128 + ((schunk ^ (row & 7)) << 4);
            if (j < LA) *(uint4*)(sA + off) = ra[j < LA ? j : 0];
            if (j < LB && (BN % RPP == 0 || row < BN)) *(uint4*)(sB + off) = rb[j < LB ? j : 0];
        }
    };

    f32x4 acc[MI][NJ];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // Residual operand (GemmArgs::R) fetched NOW instead of in the epilogue: its latency hides under the K loop (the short-K projections of the
    // transformer blocks spend a visible part of their time waiting for it after the last MFMA).  Only full 4-column groups of live rows are
    // prefetched, the same predicate the epilogue's vector path uses; split-K and GEGLU launches keep the late read.
    constexpr bool RPRE = !F8 && MI * NJ <= 20;
    uint2 rpre[RPRE ? MI * NJ : 1];
    const bool use_rpre = RPRE && p.R && p.splitk <= 1 && !p.geglu && !p.C8;
    if (use_rpre) {
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int m = m0 + wm * (BM / WM) + i * 16 + l15, n = n0 + wn * (BN / 2) + j * 16 + 4 * g4;
                rpre[i * NJ + j] = (m < p.M && n + 3 < p.N) ? *(const uint2*)((const T*)p.R + (long)m * p.ldr + n) : make_uint2(0u, 0u);
            }
    }
    f32x4 lnacc[LNF ? MI : 1];                           // folded LayerNorm: row sums (wn = 0) / sums of squares (wn = 1), see ln_exchange
#pragma unroll
    for (int i = 0; i < (LNF ? MI : 1); ++i) lnacc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};

#ifndef LDX_GEMM_NO_T14
    // Staging schedule (guide T14): the registers always hold the NEXT tile's loads.  Top of iteration kt: write tile kt+1 to the
    // other LDS stage (its loads have had a whole iteration to land) and immediately re-issue the loads of tile kt+2, then compute
    // tile kt; one barrier per K-tile.  Compared with load -> compute -> write -> barrier this keeps loads in flight across the
    // barrier and overlaps the LDS write pass with the other waves' MFMAs.
    int csa[F8 ? MI : 1], csb[F8 ? NJ : 1];              // the CURRENT tile's scales, own block's byte moved to bits 0..7
    auto take_scales = [&]() {
        if (F8) {
#pragma unroll
            for (int i = 0; i < MI; ++i) csa[i] = (int)(rsa[i] >> (8 * g4));
#pragma unroll
            for (int j = 0; j < NJ; ++j) csb[j] = (int)(rsb[j] >> (8 * g4));
        }
    };
    gload(0);
    lstore(0);
    take_scales();
    if (nk > 1) gload(1);
    __syncthreads();

    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        int nsa[F8 ? MI : 1], nsb[F8 ? NJ : 1];
        if (kt + 1 < nk) {
            lstore(cur ^ 1);
            if (F8) {
#pragma unroll
                for (int i = 0; i < MI; ++i) nsa[i] = (int)(rsa[i] >> (8 * g4));
#pragma unroll
                for (int j = 0; j < NJ; ++j) nsb[j] = (int)(rsb[j] >> (8 * g4));
            }
            if (kt + 2 < nk) gload(kt + 2);
        }
#else
    gload(0);
    lstore(0);
    __syncthreads();

    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        const bool more = (kt + 1) < nk;
        int csa[F8 ? MI : 1], csb[F8 ? NJ : 1];          // this K-tile's scales, own block's byte moved to bits 0..7
        if (F8) {
#pragma unroll
            for (int i = 0; i < MI; ++i) csa[i] = (int)(rsa[i] >> (8 * g4));
#pragma unroll
            for (int j = 0; j < NJ; ++j) csb[j] = (int)(rsb[j] >> (8 * g4));
        }
        if (more) gload(kt + 1);
#endif
        const char* sA = smem + cur * STAGE_BYTES;
        const char* sB = sA + BM * BK * 2;
        if (F8) {
            i32x8 af8[MI], bf8[NJ];
            auto frag = [&](const char* base, int row) {
                // operand registers 0-3 of lane group g hold k = 16 g + 0..15, registers 4-7 hold k = 64 + 16 g + 0..15, and the
                // scale of lane group b applies to k = 32 b .. 32 b + 31 (measured: profiles/ubench/mx_layout.hip)
                const uint4 lo = *(const uint4*)(base + row * 128 + ((g4 ^ (row & 7)) << 4));
                const uint4 hi = *(const uint4*)(base + row * 128 + (((4 + g4) ^ (row & 7)) << 4));
                return (i32x8){(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
            };
#pragma unroll
            for (int i = 0; i < MI; ++i) af8[i] = frag(sA, wm * (BM / WM) + i * 16 + l15);
#pragma unroll
            for (int j = 0; j < NJ; ++j) bf8[j] = frag(sB, wn * (BN / 2) + j * 16 + l15);
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j) acc[i][j] = mfma16_mx(bf8[j], af8[i], acc[i][j], csb[j], csa[i]);
        } else
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            V8 af[MI], bf[NJ];
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                const int row = wm * (BM / WM) + i * 16 + l15;
                const int ch = (ks * 4 + g4) ^ (row & 7);
                af[i] = as_v8<T>(*(const uint4*)(sA + row * 128 + (ch << 4)));
            }
            if constexpr (LNF) {
#pragma unroll
                for (int i = 0; i < MI; ++i) lnacc[i] = mfma16(wn ? af[i] : ones_v8<T>(), af[i], lnacc[i]);
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int row = wn * (BN / 2) + j * 16 + l15;
                const int ch = (ks * 4 + g4) ^ (row & 7);
                bf[j] = as_v8<T>(*(const uint4*)(sB + row * 128 + (ch << 4)));
            }
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j) acc[i][j] = mfma16(bf[j], af[i], acc[i][j]);
        }
#ifndef LDX_GEMM_NO_T14
        if (F8 && kt + 1 < nk) {
#pragma unroll
            for (int i = 0; i < MI; ++i) csa[i] = nsa[i];
#pragma unroll
            for (int j = 0; j < NJ; ++j) csb[j] = nsb[j];
        }
#else
        if (more) lstore(cur ^ 1);
#endif
        __syncthreads();
    }

    if constexpr (LNF) {
        float ln1[MI], ln2[MI];
        ln_exchange<MI, BM>(lnacc, (float*)smem, wm * (BM / WM), wn, l15, g4, p.K, p.ln_eps, ln1, ln2);     // the K loop ended with a barrier
        gemm_epilogue<T, BM, BN, WM, MI, NJ, true>(p, acc, m0, n0, wm, wn, l15, g4, split, S, ln1, ln2);
    } else {
        gemm_epilogue<T, BM, BN, WM, MI, NJ, false, RPRE ? MI * NJ : 1, !F8>(p, acc, m0, n0, wm, wn, l15, g4, split, S, nullptr, nullptr, rpre, use_rpre);
    }
}

template <typename T, int MODE, int BM, int BN, int WM = 2, bool F8 = false, bool LNF = false>
__global__ __launch_bounds__(WM * 128, WM == 2 ? 2 : 1) void gemm_kernel(const GemmArgs p) {
    gemm_tile_body<T, MODE, BM, BN, WM, F8, LNF>(p, blockIdx.x);
}
// Two independent plain GEMMs in one launch (Flux double blocks: the 4096-row image stream and the 256-row text stream run the
// same layer shapes with different weights): the second problem's tiles are appended to the first's, so they fill the
// partly empty last round of workgroups instead of running as a launch of their own at low occupancy.
template <typename T, int BM, int BN, bool F8>
__global__ __launch_bounds__(256, 2) void gemm2_kernel(const GemmArgs a, const GemmArgs b, const int tiles_a) {
    if ((int)blockIdx.x < tiles_a) gemm_tile_body<T, 0, BM, BN, 2, F8>(a, blockIdx.x);
    else gemm_tile_body<T, 0, BM, BN, 2, F8>(b, blockIdx.x - tiles_a);
}

// The split-K reduce launches' epilogue operands for one row and 4 consecutive columns (n % 4 == 0, n + 3 < N)
struct SkOperands { float4 bias, rv, gate; float r[4], r2[4]; };
// Round 6: split in two so that the callers can request them WITH the partials (one memory round trip per row instead of two): the per-column part
// (bias / per-image vector / gate: the same for every row a thread of the GroupNorm-producing reduce owns) and the per-row residuals, raw.
template <typename T>
static __device__ __forceinline__ void sk_load_col_operands(const GemmArgs& p, const long m, const int n, const float* rv, SkOperands& o) {
    const float* zf = p.ws;                  // readable, 16-byte aligned: what a missing operand loads (and the select below drops)
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 tb = *(const float4*)(p.bias ? p.bias + n : zf);
    const float4 tr = *(const float4*)(rv ? rv + n : zf);
    const float4 tg = *(const float4*)(p.gate ? p.gate + (long)(m / p.rows_per_batch) * p.gate_ld + n : zf);
    o.bias = p.bias ? tb : z4; o.rv = rv ? tr : z4; o.gate = p.gate ? tg : make_float4(1.f, 1.f, 1.f, 1.f);
}
template <typename T>
static __device__ __forceinline__ void sk_load_row_operands(const GemmArgs& p, const long m, const int n, uint2& t1, uint2& t2) {
    const float* zf = p.ws;
    t1 = *(const uint2*)(p.R ? (const void*)((const T*)p.R + m * p.ldr + n) : (const void*)zf);
    t2 = *(const uint2*)(p.R2 ? (const void*)((const T*)p.R2 + m * p.ldr2 + n) : (const void*)zf);
}
template <typename T>
static __device__ __forceinline__ void sk_load_operands(const GemmArgs& p, const long m, const int n, const float* rv, SkOperands& o) {
    uint2 t1, t2;
    sk_load_col_operands<T>(p, m, n, rv, o);
    sk_load_row_operands<T>(p, m, n, t1, t2);
    unpack4<T>(t1, o.r); unpack4<T>(t2, o.r2);
}
// v -> the stored values, in gemm_epilogue's operation order
template <typename T>
static __device__ __forceinline__ void sk_apply_operands(const GemmArgs& p, const SkOperands& o, float (&v)[4]) {
    const float bb[4] = {o.bias.x, o.bias.y, o.bias.z, o.bias.w}, rr[4] = {o.rv.x, o.rv.y, o.rv.z, o.rv.w}, gg[4] = {o.gate.x, o.gate.y, o.gate.z, o.gate.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float x = v[c];
        if (p.bias) x += bb[c];
        if (p.rowvec) x += rr[c];
        if (p.act == 1) x = x / (1.0f + __expf(-1.702f * x));
        else if (p.act == 2) x = gelu_tanh_f(x);
        else if (p.act == 3) x = x > 0.f ? x : 0.2f * x;
        if (p.gate) x *= gg[c];
        if (p.oscale != 0.f) x *= p.oscale;
        if (p.R) x += o.r[c];
        if (p.R2) x = fmaf(x, p.oscale2, o.r2[c]);
        v[c] = x;
    }
}

// sum the split-K partials (fixed order -> deterministic) and apply the epilogue; one thread per 4 columns
template <typename T>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const GemmArgs p) {
    const int nq = (p.N + 3) / 4;
    const long total = (long)p.M * nq;
    const T* __restrict__ Rp = (const T*)p.R;
    T* __restrict__ Cp = (T*)p.C;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int m = (int)(idx / nq), n = (int)(idx % nq) * 4;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        const bool full = n + 3 < p.N;
        const float* rv = p.rowvec ? p.rowvec + (long)(m / p.rows_per_batch) * p.rowvec_ld : nullptr;
        SkOperands o;
        uint2 o1 = make_uint2(0u, 0u), o2 = o1;
        if (full) { sk_load_col_operands<T>(p, m, n, rv, o); sk_load_row_operands<T>(p, m, n, o1, o2); }      // in flight together with the partials (round 6)
        if (full) {
            // four partial loads in flight at a time (the adds stay in split order: deterministic)
            int sidx = 0;
            const size_t stride = (size_t)p.M * p.N;
            const float* w = p.ws + (size_t)m * p.N + n;
            for (; sidx + 4 <= p.splitk; sidx += 4) {
                const float4 t0 = *(const float4*)(w + (size_t)sidx * stride), t1 = *(const float4*)(w + (size_t)(sidx + 1) * stride);
                const float4 t2 = *(const float4*)(w + (size_t)(sidx + 2) * stride), t3 = *(const float4*)(w + (size_t)(sidx + 3) * stride);
                v[0] += t0.x; v[1] += t0.y; v[2] += t0.z; v[3] += t0.w;
                v[0] += t1.x; v[1] += t1.y; v[2] += t1.z; v[3] += t1.w;
                v[0] += t2.x; v[1] += t2.y; v[2] += t2.z; v[3] += t2.w;
                v[0] += t3.x; v[1] += t3.y; v[2] += t3.z; v[3] += t3.w;
            }
            for (; sidx < p.splitk; ++sidx) { const float4 t = *(const float4*)(w + (size_t)sidx * stride); v[0] += t.x; v[1] += t.y; v[2] += t.z; v[3] += t.w; }
        } else {
            for (int sidx = 0; sidx < p.splitk; ++sidx) {
                const float* w = p.ws + ((size_t)sidx * p.M + m) * p.N + n;
                for (int r = 0; r < 4 && n + r < p.N; ++r) v[r] += w[r];
            }
        }
        if (full) {
            // Epilogue operands as UNCONDITIONAL 16 / 8-byte loads (a null operand reads the workspace instead and is discarded by a select): written as
            // `if (p.bias) x += p.bias[n + r]` per element, hipcc emitted one global load + s_waitcnt vmcnt(0) per element and operand — two dozen memory
            // latencies in a row, 13 - 31 us per reduce launch, 0.65 ms of the 1024^2 step (profiles/r05/bench_kernel_stats.csv).  Same operations, same order.
            unpack4<T>(o1, o.r); unpack4<T>(o2, o.r2);
            sk_apply_operands<T>(p, o, v);
        } else
        for (int r = 0; r < 4 && n + r < p.N; ++r) {
            float x = v[r];
            if (p.bias) x += p.bias[n + r];
            if (rv) x += rv[n + r];
            if (p.act == 1) x = x / (1.0f + __expf(-1.702f * x));
            else if (p.act == 2) x = gelu_tanh_f(x);
            else if (p.act == 3) x = x > 0.f ? x : 0.2f * x;
            if (p.gate) x *= p.gate[(long)(m / p.rows_per_batch) * p.gate_ld + n + r];
            if (p.oscale != 0.f) x *= p.oscale;
            if (Rp) x += to_f32(Rp[(long)m * p.ldr + n + r]);
            if (p.R2) x = fmaf(x, p.oscale2, to_f32(((const T*)p.R2)[(long)m * p.ldr2 + n + r]));
            v[r] = x;
        }
        if (full) {
            if (Cp) { const uint2 pk = pack4<T>(v[0], v[1], v[2], v[3]); *(uint2*)(Cp + (long)m * p.ldc + n) = pk; if (p.dup_rows) *(uint2*)(Cp + ((long)m + p.dup_rows) * p.ldc + n) = pk; }
            if (p.Cf) *(float4*)(p.Cf + (long)m * p.ldcf + n) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            for (int r = 0; r < 4 && n + r < p.N; ++r) {
                if (Cp) { Cp[(long)m * p.ldc + n + r] = from_f32<T>(v[r]); if (p.dup_rows) Cp[((long)m + p.dup_rows) * p.ldc + n + r] = from_f32<T>(v[r]); }
                if (p.Cf) p.Cf[(long)m * p.ldcf + n + r] = v[r];
            }
        }
    }
}

// Split-K reduce that also produces the consumer GroupNorm's statistics (GemmArgs::gn_partial with splitk > 1): one workgroup per chunk of
// gn_hw / gn_nchunk rows of one image x ALL columns.  Thread (rl, quad) owns 4 fixed columns and every R-th row of the chunk, so its sums of the
// rounded outputs are per column; LDS [R][N][2]; then one thread per (group, statistic) adds its gn_cpg columns over the R row lanes in a
// fixed order (deterministic, no atomics).  Same partial layout as the GEMM epilogue's: gn_partial[b][chunk][G][2].
template <typename T>
__global__ __launch_bounds__(1024) void splitk_reduce_gn_kernel(const GemmArgs p, const int R) {
    extern __shared__ float red_gn[];
    const int nq = p.N >> 2, tid = threadIdx.x;
    const int rl = tid / nq, n = (tid - rl * nq) * 4;
    const int RB = p.gn_hw / p.gn_nchunk;
    const int b = blockIdx.y, chunk = blockIdx.x;
    const long row0 = (long)b * p.gn_hw + (long)chunk * RB;
    T* __restrict__ Cp = (T*)p.C;
    const size_t stride = (size_t)p.M * p.N;
    float gs[4] = {0.f, 0.f, 0.f, 0.f}, gq[4] = {0.f, 0.f, 0.f, 0.f};
    if (rl < R) {
        SkOperands o;                                         // per-column operands: one image per chunk, one column quad per thread -> loaded once
        sk_load_col_operands<T>(p, row0, n, p.rowvec ? p.rowvec + (long)(row0 / p.rows_per_batch) * p.rowvec_ld : nullptr, o);
        // U rows x SB splits of partial loads in flight per thread.  (Round 5: with one split at a time a chunk of R rows — one row per thread, what the
        // 16^2 / 32^2 levels get — paid one memory latency per split: 20 us for S = 11 at M = 512, as long as the GEMM in front of it.)  The adds stay in
        // split order: same bits as before.
        constexpr int U = 2, SB = 4;
        for (int r = rl; r < RB; r += R * U) {
            float v[U][4];
            bool live[U];
#pragma unroll
            for (int u = 0; u < U; ++u) { live[u] = r + u * R < RB; v[u][0] = v[u][1] = v[u][2] = v[u][3] = 0.f; }
            uint2 o1[U], o2[U];                               // the rows' residuals, requested with the first partials (round 6: they used to follow the last partial's arrival — a second round trip per row)
#pragma unroll
            for (int u = 0; u < U; ++u) { o1[u] = o2[u] = make_uint2(0u, 0u); if (live[u]) sk_load_row_operands<T>(p, row0 + r + u * R, n, o1[u], o2[u]); }
            for (int s0 = 0; s0 < p.splitk; s0 += SB) {
                float4 t[U][SB];
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int sb = 0; sb < SB; ++sb)
                        t[u][sb] = (live[u] && s0 + sb < p.splitk) ? *(const float4*)(p.ws + (size_t)(s0 + sb) * stride + (size_t)(row0 + r + u * R) * p.N + n) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int sb = 0; sb < SB; ++sb) {
                    if (s0 + sb < p.splitk) {      // (adding the zeros of a missing split would turn a -0 sum into +0)
#pragma unroll
                        for (int u = 0; u < U; ++u) { v[u][0] += t[u][sb].x; v[u][1] += t[u][sb].y; v[u][2] += t[u][sb].z; v[u][3] += t[u][sb].w; }
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!live[u]) continue;
                const long m = row0 + r + u * R;
                unpack4<T>(o1[u], o.r); unpack4<T>(o2[u], o.r2);
                sk_apply_operands<T>(p, o, v[u]);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float xr = to_f32(from_f32<T>(v[u][c]));      // statistics of the values as stored
                    gs[c] += xr; gq[c] = fmaf(xr, xr, gq[c]);
                }
                { const uint2 pk = pack4<T>(v[u][0], v[u][1], v[u][2], v[u][3]); *(uint2*)(Cp + (long)m * p.ldc + n) = pk; if (p.dup_rows) *(uint2*)(Cp + ((long)m + p.dup_rows) * p.ldc + n) = pk; }
                if (p.Cf) *(float4*)(p.Cf + (long)m * p.ldcf + n) = make_float4(v[u][0], v[u][1], v[u][2], v[u][3]);
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) { red_gn[((long)rl * p.N + n + c) * 2] = gs[c]; red_gn[((long)rl * p.N + n + c) * 2 + 1] = gq[c]; }
    }
    __syncthreads();
    // 8 lanes per (group, statistic): lane k adds elements k, k + 8, .. of the R x cpg column sums, then a 3-step butterfly — a fixed tree, so still
    // deterministic (one thread per pair walked 80 dependent LDS reads at N = 1280: ~4 us of a 14 us launch)
    if (tid < p.gn_G * 2 * 8 && (int)blockDim.x >= p.gn_G * 2 * 8) {
        const int pr = tid >> 3, k = tid & 7, g = pr >> 1, st = pr & 1, c0 = g * p.gn_cpg, ne = R * p.gn_cpg;
        float a = 0.f;
        for (int e = k; e < ne; e += 8) { const int l = e / p.gn_cpg, c = e - l * p.gn_cpg; a += red_gn[((long)l * p.N + c0 + c) * 2 + st]; }
        a += __shfl_xor(a, 1); a += __shfl_xor(a, 2); a += __shfl_xor(a, 4);
        if (k == 0) p.gn_partial[(((long)b * p.gn_nchunk + chunk) * p.gn_G + g) * 2 + st] = a;
    } else if ((int)blockDim.x < p.gn_G * 2 * 8 && tid < p.gn_G * 2) {
        const int g = tid >> 1, st = tid & 1, c0 = g * p.gn_cpg;
        float a = 0.f;
        for (int l = 0; l < R; ++l)
            for (int c = 0; c < p.gn_cpg; ++c) a += red_gn[((long)l * p.N + c0 + c) * 2 + st];
        p.gn_partial[(((long)b * p.gn_nchunk + chunk) * p.gn_G + g) * 2 + st] = a;
    }
}

// ---- launch: the instantiations behind what gemm_pick chose (gemm_pick.cpp: the pick, its shape rules and the planner's queries) ----
template <typename T, int MODE, int BM, int BN, int WM = 2, bool F8 = false, bool LNF = false>
static void launch_gemm_inst(const GemmArgs& a, int S, hipStream_t s) {
    const int tiles = ((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN) * S;
    const size_t lds = 2 * stage_bytes<BM, BN>();
    static DevOnce once;
    set_dyn_lds(once, (const void*)gemm_kernel<T, MODE, BM, BN, WM, F8, LNF>, (int)lds);
    hipLaunchKernelGGL((gemm_kernel<T, MODE, BM, BN, WM, F8, LNF>), dim3(tiles), dim3(WM * 128), lds, s, a);
}

// the register-staged instantiations (GF_TILE, GF_TILE_MX) by the pick's tile
template <typename T, int MODE>
static void launch_gemm_tile(const GemmArgs& a, const GemmPick& p, hipStream_t s) {
    const int tile = p.bm * 1000 + p.bn;
    if constexpr (MODE == 0) {
        if (p.f8 && tile == 256128) return launch_gemm_inst<T, 0, 256, 128, 4, true>(a, p.S, s);      // opt-in (LDX_GEMM_TILE)
        if (p.f8 && tile == 64064) return launch_gemm_inst<T, 0, 64, 64, 2, true>(a, p.S, s);
        if (p.f8 && tile == 128160) return launch_gemm_inst<T, 0, 128, 160, 2, true>(a, p.S, s);
        if (p.f8 && tile == 128128) return launch_gemm_inst<T, 0, 128, 128, 2, true>(a, p.S, s);
        if (p.lnf && tile == 64064) return launch_gemm_inst<T, 0, 64, 64, 2, false, true>(a, 1, s);
        if (p.lnf && tile == 128160) return launch_gemm_inst<T, 0, 128, 160, 2, false, true>(a, 1, s);
        if (p.lnf && tile == 128128) return launch_gemm_inst<T, 0, 128, 128, 2, false, true>(a, 1, s);
    }
    const bool lean = !p.f8 && !p.lnf;
    if (lean && tile == 128032) return launch_gemm_inst<T, MODE, 128, 32>(a, p.S, s);
    if (lean && tile == 128064) return launch_gemm_inst<T, MODE, 128, 64>(a, p.S, s);
    if (lean && tile == 64064) return launch_gemm_inst<T, MODE, 64, 64>(a, p.S, s);
    if (lean && tile == 128160) return launch_gemm_inst<T, MODE, 128, 160>(a, p.S, s);
    if (lean && tile == 128128) return launch_gemm_inst<T, MODE, 128, 128>(a, p.S, s);
    fprintf(stderr, "ldx: gemm_pick chose a %d x %d tile (mode %d, f8 %d, ln-fold %d) that has no instantiation\n", p.bm, p.bn, MODE, (int)p.f8, (int)p.lnf);
    abort();
}

template <typename T>
static void launch_gemm_t(const GemmArgs& a, const GemmPick& p, hipStream_t s) {
    if (p.family == GF_RING) launch_gemm_ring(a, DTypeOf<T>::v, s);
    else if (p.family == GF_PP || p.family == GF_PP_MX) launch_gemm_pp(a, p.bn, p.lnf, p.S, DTypeOf<T>::v, s);
    else if (a.mode == 0) launch_gemm_tile<T, 0>(a, p, s);
    else launch_gemm_tile<T, 1>(a, p, s);
    if (p.reduce == RED_LAUNCH_GN) {       // reduce + GroupNorm statistics (gemm_gn_fuse set the geometry, gemm_gn_check held it to this launch)
        int R = 1;
        const int nchunk = splitk_gn_geom(a, a.gn_hw, a.gn_G, a.gn_nchunk, &R);
        hipLaunchKernelGGL((splitk_reduce_gn_kernel<T>), dim3(nchunk, a.M / a.gn_hw), dim3((a.N / 4) * R), (size_t)R * a.N * 2 * sizeof(float), s, a, R);
    } else if (p.reduce == RED_LAUNCH) {
        long total = (long)a.M * ((a.N + 3) / 4);
        int grid = (int)((total + 255) / 256); if (grid > 2048) grid = 2048;
        hipLaunchKernelGGL((splitk_reduce_kernel<T>), dim3(grid), dim3(256), 0, s, a);
    }
}

void launch_gemm(const GemmArgs& a0, DType dt, hipStream_t s) {
    GemmArgs a = a0; a.ep_general = g_sw.ep_general;
    const GemmPick p = gemm_pick(a);
    if (!p.launches) return;
    gemm_gn_check(a);
    if (p.family == GF_CONV_PATCH) { launch_conv_patch(a, dt, s); return; }
    if (p.reduce != RED_IN_KERNEL) a.sk_count = nullptr;        // the kernels reduce in place iff sk_count is set
    if (dt == DT_BF16) launch_gemm_t<__bf16>(a, p, s); else launch_gemm_t<_Float16>(a, p, s);
}

template <typename T, bool F8>
static void launch_gemm2_t(const GemmArgs& a, const GemmArgs& b, hipStream_t s) {
    const int ta = ((a.M + 127) / 128) * ((a.N + 127) / 128), tb = ((b.M + 127) / 128) * ((b.N + 127) / 128);
    const size_t lds = 2 * stage_bytes<128, 128>();
    static DevOnce once;
    set_dyn_lds(once, (const void*)gemm2_kernel<T, 128, 128, F8>, (int)lds);
    hipLaunchKernelGGL((gemm2_kernel<T, 128, 128, F8>), dim3(ta + tb), dim3(256), lds, s, a, b, ta);
}
void launch_gemm2(const GemmArgs& a, const GemmArgs& b, DType dt, hipStream_t s) {
    if (a.M <= 0 || a.N <= 0) { launch_gemm(b, dt, s); return; }
    if (b.M <= 0 || b.N <= 0) { launch_gemm(a, dt, s); return; }
    const GemmPick p = gemm_pick(a, &b);
    GemmArgs x = a, y = b; x.splitk = y.splitk = 1; x.ep_general = y.ep_general = g_sw.ep_general;
    if (p.family == GF_PP2 || p.family == GF_PP2_MX) launch_gemm_pp2(x, y, p.bn, dt, s);
    else if (dt == DT_BF16) { if (p.f8) launch_gemm2_t<__bf16, true>(x, y, s); else launch_gemm2_t<__bf16, false>(x, y, s); }
    else { if (p.f8) launch_gemm2_t<_Float16, true>(x, y, s); else launch_gemm2_t<_Float16, false>(x, y, s); }
}

// ------------------------------------------------------------------------------------------
// Skinny GEMM (tiny M): HBM-bound on the weight matrix.  One workgroup = 4 waves x 4 output columns each; the
// (<= 4 row) activation block is staged once in LDS as fp32, and every wave keeps 4 independent 16-byte weight
// streams in flight so the loads pipeline.
template <typename T>
__global__ __launch_bounds__(256) void skinny_kernel(const SkinnyArgs p) {
    extern __shared__ float sx[];                          // [mrows][K]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n0 = (blockIdx.x * 4 + wave) * 4;
    for (int mb = 0; mb < p.M; mb += 4) {
        const int mr = min(4, p.M - mb);
        __syncthreads();
        for (int i = threadIdx.x; i < mr * p.K; i += 256) {
            float xv = p.x[(long)(mb + i / p.K) * p.ldx + (i % p.K)];
            if (p.in_act) xv = xv / (1.0f + expf(-xv));
            sx[i] = xv;
        }
        __syncthreads();
        if (n0 >= p.N) continue;
        float acc[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) acc[r][mi] = 0.f;
        const T* __restrict__ w = (const T*)p.W;
        for (int k = lane * 8; k < p.K; k += 64 * 8) {
            uint4 wv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) wv[r] = (n0 + r < p.N) ? *(const uint4*)(w + (long)(n0 + r) * p.K + k) : make_uint4(0, 0, 0, 0);
            float xr[4][8];
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int e = 0; e < 8; ++e) xr[mi][e] = mi < mr ? sx[mi * p.K + k + e] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float wf[8];
                unpack8<T>(wv[r], wf);
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[r][mi] = fmaf(xr[mi][e], wf[e], acc[r][mi]);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) {
                const float v = wave_sum(acc[r][mi]);
                const int m = mb + mi, n = n0 + r;
                if (lane == 0 && mi < mr && n < p.N) {
                    float o = v + (p.bias ? p.bias[n] : 0.f);
                    if (p.out_act) o = o / (1.0f + expf(-o));
                    if (p.accum) o += p.out[(long)m * p.ldo + n];
                    p.out[(long)m * p.ldo + n] = o;
                }
            }
    }
}

// The same with MX fp8 weights (SkinnyArgs::W8): the activation block goes through the MX rule while it is staged — per 32 consecutive k: amax, E8M0 scale,
// e4m3 round-to-nearest-even, back to fp32 (oracle mx_fake_quant; the value a block-scaled MFMA would see) — and every lane streams 16 weights per 16-byte load,
// dequantised with the scale byte of their block.  fp32 accumulation.  HBM-bound like the 16-bit kernel, at half the bytes.
constexpr int SKM_RG = 4;
__global__ __launch_bounds__(256) void skinny_mx_kernel(const SkinnyArgs p) {
    extern __shared__ float sx[];                          // [mrows][K]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nkb = p.K >> 5;
    for (int mb = 0; mb < p.M; mb += 4) {
        const int mr = min(4, p.M - mb);
        __syncthreads();
        for (int blk = threadIdx.x; blk < mr * nkb; blk += 256) {      // one thread per 32-element block
            const int mi = blk / nkb, kb = blk - mi * nkb;
            const float* src = p.x + (long)(mb + mi) * p.ldx + kb * 32;
            float f[32];
            float amax = 0.f;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const float4 t = *(const float4*)(src + 4 * c);
                f[4 * c] = t.x; f[4 * c + 1] = t.y; f[4 * c + 2] = t.z; f[4 * c + 3] = t.w;
            }
#pragma unroll
            for (int i = 0; i < 32; ++i) { if (p.in_act) f[i] = f[i] / (1.0f + expf(-f[i])); amax = fmaxf(amax, fabsf(f[i])); }
            const int e = mx_scale_e8m0(amax);
            const float inv = mx_inv_scale(e), sc = __uint_as_float((uint32_t)e << 23);
            float* dst = sx + (long)mi * p.K + kb * 32;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int w = (int)mx_pack4(f[4 * c] * inv, f[4 * c + 1] * inv, f[4 * c + 2] * inv, f[4 * c + 3] * inv);
                const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8(w, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8(w, true);
                *(float4*)(dst + 4 * c) = make_float4(lo[0] * sc, lo[1] * sc, hi[0] * sc, hi[1] * sc);
            }
        }
        __syncthreads();
        // SKM_RG groups of 4 output rows per wave: the staged (and quantised) activation serves 64 rows of W per workgroup instead of 16
        for (int rg = 0; rg < SKM_RG; ++rg) {
        const int n0 = ((blockIdx.x * 4 + wave) * SKM_RG + rg) * 4;
        if (n0 >= p.N) break;
        float acc[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) acc[r][mi] = 0.f;
        const uint8_t* __restrict__ w8 = (const uint8_t*)p.W8;
        for (int k = lane * 16; k < p.K; k += 64 * 16) {
            uint4 wv[4]; uint32_t sd[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool ok = n0 + r < p.N;
                wv[r] = ok ? *(const uint4*)(w8 + (long)(n0 + r) * p.K + k) : make_uint4(0, 0, 0, 0);
                sd[r] = ok ? p.SW[(long)(k >> 7) * p.sw_ld + n0 + r] : 0u;
            }
            float xr[4][16];
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int e = 0; e < 16; ++e) xr[mi][e] = mi < mr ? sx[mi * p.K + k + e] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float sc = __uint_as_float(((sd[r] >> (8 * ((k >> 5) & 3))) & 0xffu) << 23);
                const int wq[4] = {(int)wv[r].x, (int)wv[r].y, (int)wv[r].z, (int)wv[r].w};
                float wf[16];               // the lane's 16 weights share one block: unscaled products first, the scale once per row and block
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8(wq[c], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8(wq[c], true);
                    wf[4 * c] = lo[0]; wf[4 * c + 1] = lo[1]; wf[4 * c + 2] = hi[0]; wf[4 * c + 3] = hi[1];
                }
#pragma unroll
                for (int mi = 0; mi < 4; ++mi) {
                    if (mi < mr) {          // wave-uniform: only the live activation rows (Flux: one or two)
                        float t = 0.f;
#pragma unroll
                        for (int e = 0; e < 16; ++e) t = fmaf(xr[mi][e], wf[e], t);
                        acc[r][mi] = fmaf(t, sc, acc[r][mi]);
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) {
                const float v = wave_sum(acc[r][mi]);
                const int m = mb + mi, n = n0 + r;
                if (lane == 0 && mi < mr && n < p.N) {
                    float o = v + (p.bias ? p.bias[n] : 0.f);
                    if (p.out_act) o = o / (1.0f + expf(-o));
                    if (p.accum) o += p.out[(long)m * p.ldo + n];
                    p.out[(long)m * p.ldo + n] = o;
                }
            }
        }
    }
}

void launch_skinny(const SkinnyArgs& a, DType dt, hipStream_t s) {
    if (a.M <= 0 || a.N <= 0) return;
    dim3 grid((a.N + 15) / 16), block(256);
    const size_t lds = (size_t)4 * a.K * sizeof(float);
    if (a.W8 && (a.K & 31) == 0) {
        static DevOnce once;
        set_dyn_lds(once, (const void*)skinny_mx_kernel, 160 * 1024);
        hipLaunchKernelGGL(skinny_mx_kernel, dim3((a.N + 16 * SKM_RG - 1) / (16 * SKM_RG)), block, lds, s, a);
        return;
    }
    if (dt == DT_BF16) {
        static DevOnce once;
    set_dyn_lds(once, (const void*)skinny_kernel<__bf16>, 160 * 1024);
        hipLaunchKernelGGL((skinny_kernel<__bf16>), grid, block, lds, s, a);
    } else {
        static DevOnce once;
    set_dyn_lds(once, (const void*)skinny_kernel<_Float16>, 160 * 1024);
        hipLaunchKernelGGL((skinny_kernel<_Float16>), grid, block, lds, s, a);
    }
}

}  // namespace ldx
