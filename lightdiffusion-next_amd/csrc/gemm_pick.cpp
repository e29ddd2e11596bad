// Which kernel a GEMM / convolution runs (ldx_kernels.h: GemmPick) and every shape rule and planner query around that choice: pure host arithmetic over the launch
// arguments and the switches of ldx_switches.h (g_sw, g_launch_sw), no engine and no device.  The kernels, their launchers and the instantiation tables are in
// gemm.hip, gemm_pp*.hip, gemm_ring.hip and conv_patch.hip; what a rule needs to know of a kernel's geometry is in ldx_geometry.h.
#include "ldx_kernels.h"
#include "ldx_switches.h"

#include <cstdio>
#include <cstdlib>

namespace ldx {

// geometry of the reduce + GroupNorm-statistics launch: R row lanes of N / 4 threads (<= 1024 threads, >= 2 * G), chunks of RB rows; 0 = not applicable
int splitk_gn_geom(const GemmArgs& a, int HW, int G, int max_chunks, int* R_out) {
    if (a.N % 4 || !a.C || a.N % G || HW <= 0 || a.M % HW) return 0;
    const int nq = a.N / 4;
    if (nq > 512 || nq < 1) return 0;
    int R = nq <= 128 ? 8 : (nq <= 256 ? 4 : 2);        // a power of two (chunks of R rows must tile the image); up to 1024 threads: the kernel is latency-bound
    if (nq * R < 2 * G) return 0;
    if (gn_uses_small_kernel(a.M / HW, HW, a.N, G)) return 0;      // the one-launch small GroupNorm kernel takes this one (norm.hip): faster than apply-only
    const int lim = max_chunks < g_sw.skgn_chunks ? max_chunks : g_sw.skgn_chunks;
    // rows per chunk: a multiple of R dividing HW, as small as keeps nchunk <= lim (more workgroups), at least R
    int RB = 0;
    for (int cand = R; cand <= HW; cand += R) if (HW % cand == 0 && HW / cand <= lim) { RB = cand; break; }
    if (!RB) return 0;
    *R_out = R;
    return HW / RB;
}

// tile selection: the {BM, BN} the heuristics ask for; gemm_pick maps it to the instantiation that exists for the launch's mode and flags
struct TileSel { int bm, bn; };
// The ping-pong cost model, shared by the single launch (gemm_tile), the MX fp8 one (mx_pp_bn) and the two-problem one (gemm2_pp_bn), which differ in how they
// count tiles and in their constants: of the candidate widths (rate 0 or a tile count of 0: not a candidate) that give at least 192 workgroups — fewer would
// leave a quarter of the CUs idle — the one with the lowest cost = rounds x slots x tile area / rate, if that beats the 128-row kernel's cost_old by 5 %
// (LDX_PP=2: always).  Returns its width, 0 = keep the 128-row kernel.
template <int NC, typename TileCount>
static int pp_cost_model(const int (&cand)[NC], const double (&rate)[NC], TileCount tiles, double cost_old) {
    double best = 1e30; int best_bn = 0;
    for (int c = 0; c < NC; ++c) {
        if (rate[c] <= 0) continue;
        const long t = tiles(cand[c]);
        if (t < 192) continue;
        const double cost = (double)((t + 255) / 256) * 256.0 * 256.0 * cand[c] / rate[c];
        if (cost < best) { best = cost; best_bn = cand[c]; }
    }
    return best_bn && (g_sw.pp >= 2 || best < 0.95 * cost_old) ? best_bn : 0;
}

// Planner rule (gemm_tile asks it): the shapes the register-staged 64 x 64 tiles serve today — fewer than 400 tiles of 128 x 128 and a short K — whose
// 64 x 160 tiling still gives (nearly) every CU a workgroup.  LDX_RING=0 switches the kernel off, 2 takes every plain GEMM with N % 160 == 0 that fills the chip.
bool gemm_ring_ok(int M, int N, int K, bool plain, int splitk) {
    const int mode = g_launch_sw.ring;
    if (!mode || !plain || splitk > 1 || N % GR_BN || K % BK || K < 2 * BK || M <= 0) return false;
    const long t = (long)((M + GR_BM - 1) / GR_BM) * (N / GR_BN);
    if (mode >= 2) return t >= 192;
    return t >= 192 && t <= 512;
}

static inline TileSel gemm_tile(int M, int N, int K, bool geglu, int splitk, bool allow_pp = true, bool plain = false) {      // plain: a GEMM (224 / 192 wide ping-pong tiles exist), not a conv
    if (g_sw.tile) return {g_sw.tile / 1000, g_sw.tile % 1000};
    if (!geglu && N <= 32 && splitk <= 1) return {128, 32};          // ESRGAN dense-block convs (growth 32), 3-channel output convs
    if (!geglu && N <= 64 && splitk <= 1 && (long)((M + 127) / 128) >= 400) return {128, 64};
    // Large problems: the 256-row ping-pong kernel (gemm_pp.inc; one 8-wave workgroup per CU, LDS-DMA ring) when a simple cost model
    // says so.  Isolated rates on MI355X (profiles/kprobe.py pp, bf16): 256 x 256 tiles 1.2-1.4 PFLOP/s, 256 x 160 0.95-1.2, 256 x 128
    // ~1.0 on long K, against 0.72-0.96 for the register-staged 128-row kernel; short-K problems (a handful of K-tiles) are bound by
    // per-launch fixed costs and the output write instead and gain nothing, and N = 128 (VAE 1024^2 level) loses.
    // cost = rounds x slots x tile area / rate; LDX_PP: 0 off, 1 model (default), 2 whenever a candidate fills >= 3/4 of the CUs.
    // GEGLU up-projections (N = 8 C, an erf per output pair in the output stage) gain from the 256-wide tiles already at K = 640: M 8192 N 5120 K 640 105 us on
    // 128 x 128, 97 on 256 x 128, 84 on 256 x 256 (profiles/r06/geglu_tiles.txt)
    if (allow_pp && g_sw.pp && M >= 1024 && N >= 256 && (K >= g_sw.pp_mink || (geglu && K >= 640))) {
        const long S = splitk > 1 ? splitk : 1, mt = (M + 255) / 256;
        const int cand[5] = {256, 224, 192, 160, 128};
        const double rate[5] = {1.35, plain ? g_sw.pp_r224 : 0, plain ? g_sw.pp_r192 : 0, 1.15, 0.92};
        const int bo = geglu ? 128 : ((N % 160 == 0 && N % 128 != 0) ? 160 : 128);
        const long to = (long)((M + 127) / 128) * ((N + bo - 1) / bo) * S;
        const auto tiles = [&](int c) -> long { return (geglu && c != 128 && c != 256) ? 0 : mt * ((N + c - 1) / c) * S; };      // GEGLU pairs value / gate columns inside 64-column slabs: wave tiles of 64 or 128 columns
        const int bn = pp_cost_model(cand, rate, tiles, (double)((to + 511) / 512) * 512.0 * 128.0 * bo / 0.84);
        // (round 6) a ragged 128-wide ping-pong tiling (N = 320: 3 column tiles for 2.5) against 160-wide register-staged tiles that fit one per CU: measured equal
        // (M 16384 N 320 K 2880: 61.4 vs 60.0 us, profiles/r06/conv_tiles.txt), and only the exact tiling can feed the consumer GroupNorm's statistics
        const bool ragged_tie = bn == 128 && N % 128 != 0 && N % bo == 0 && to <= 256;
        if (bn && (g_sw.pp >= 2 || !ragged_tie)) return {256, bn};
    }
    if (geglu) return {128, 128};
    int bn = (N % 160 == 0 && N % 128 != 0) ? 160 : 128;
    // wave quantisation: 257..511 tiles of 128x128 put two workgroups on some CUs and one on the rest (the launch takes as
    // long as the doubly-loaded CUs); if 128x160 tiles fit one per CU, every CU runs a single, 1.25x larger tile instead
    if (bn == 128 && N % 160 == 0 && splitk <= 2 && !g_sw.no_tile160) {
        const long t128 = (long)((M + 127) / 128) * ((N + 127) / 128), t160 = (long)((M + 127) / 128) * (N / 160);
        if (t128 > 256 && t128 < 512 && t160 <= 256) bn = 160;      // with splitk == 2 (gemm_choose_splitk's one-per-CU rule): 2 x t160 <= 512 workgroups
    }
    const long tiles = (long)((M + 127) / 128) * ((N + bn - 1) / bn) * (splitk > 1 ? splitk : 1);
    // < 0.8 of one round of 2 workgroups x 256 CUs and a short K loop (latency-bound): go small.
    // Long-K problems (3x3 convs) keep the big tile: measured 112 us (128x128) vs 125 us (64x64) at 64^2, 640->640;
    // 2048x1280x1280 went 27.6 -> 18.8 us with 64x64.
    if (tiles < 400 && K <= 24 * BK) {
        // Round 5: where a 64 x 160 tiling still gives every CU work, the LDS-DMA ring kernel (gemm_ring.hip: 45.7 instead of 32 flop per operand byte AND
        // three to four K-tiles in flight) takes the launch.  (The same tile on THIS kernel's register-staged loop measured slower than 64 x 64: 25.6 vs
        // 22.8 us at 2048 x 1280 x 1280 — one K-tile in flight per CU; profiles/r05/ab_caches_tile64x160.txt.)
        if (gemm_ring_ok(M, N, K, plain, splitk)) return {64, 160};
        return {64, 64};
    }
    return {128, bn};
}

// MX fp8 operands: 256-row ping-pong tile width (160 / 128) or 0 = keep the 128-row kernel.  The cost model with the MX
// rates (isolated Flux shapes, profiles/mx_probe.py); the quantised-output epilogue needs 64-column wave tiles (BN = 128).
static int mx_pp_bn(long tiles_m256, long tiles_m128, int N, int K, int S, bool c8, long ym256 = 0, long ym128 = 0, int yN = 0) {      // y*: the second problem of a two-problem launch
    if (!g_sw.pp || N < 256 || K < g_sw.pp_mink_mx) return 0;
    // per-round rates from the 8192^3 sweep (profiles/ubench/README.md): wider tiles move fewer operand bytes per flop, and N = 3072 fits one round of 224s
    const int cand[4] = {224, 192, 160, 128};
    const double rate[4] = {g_sw.mx_r224, g_sw.mx_r192, 1.93, 1.75};
    const long to = tiles_m128 * ((N + 127) / 128) * S + ym128 * ((yN + 127) / 128);
    const auto tiles = [&](int c) -> long { return (c8 && c != 128 && c != 192) ? 0 : tiles_m256 * ((N + c - 1) / c) * S + ym256 * ((yN + c - 1) / c); };
    return pp_cost_model(cand, rate, tiles, (double)((to + 511) / 512) * 512.0 * 128.0 * 128.0 / 1.2);
}

// 256-row ping-pong tiles for a two-problem launch: the cost model over the combined tile count; 0 = keep 128 x 128
static int gemm2_pp_bn(const GemmArgs& a, const GemmArgs& b) {
    if (!g_sw.pp || a.f8 || b.f8 || a.K < g_sw.pp_mink || b.K < g_sw.pp_mink || a.N < 256 || b.N < 256 || a.M + b.M < 1024) return 0;
    const int cand[5] = {256, 224, 192, 160, 128};
    const double rate[5] = {1.35, g_sw.pp_r224, g_sw.pp_r192, 1.15, 0.92};
    const long to = (long)((a.M + 127) / 128) * ((a.N + 127) / 128) + (long)((b.M + 127) / 128) * ((b.N + 127) / 128);
    const auto tiles = [&](int c) -> long { return (long)((a.M + 255) / 256) * ((a.N + c - 1) / c) + (long)((b.M + 255) / 256) * ((b.N + c - 1) / c); };
    return pp_cost_model(cand, rate, tiles, (double)((to + 511) / 512) * 512.0 * 128.0 * 128.0 / 0.84);
}

bool gemm_sk_fixup(const GemmArgs& a) {
    // OPT-IN at build AND run time (-DLDX_SK_FIXUP_BUILD, LDX_SK_FIXUP=1): measured on the SD1.5 1024^2 step, same box, round 4: reduce launches 14.55 / 14.71 ms, in-kernel reduction up to
    // S = 2: 14.73 (neutral), up to S = 3 / 4: 14.69 / 14.84 (+0.13 ms) — the last arriver's S serial slab reads sit in the tail of the launch,
    // while the reduce kernel spreads the same bytes over the whole chip (and also emits the GroupNorm partials).
#ifndef LDX_SK_FIXUP_BUILD
    return false;      // the in-kernel path is not compiled in (gemm_common.h): it costs every instantiation registers
#else
    if (!g_sw.sk_fixup || !a.sk_count || !a.ws || a.splitk < 2 || a.splitk > g_sw.sk_fixup_max || a.geglu) return false;
    return (long)((a.M + 63) / 64) * ((a.N + 31) / 32) <= SK_COUNTERS;      // an upper bound on the tile count of any tile shape
#endif
}

// conv_patch.hip: the shapes and epilogues its kernels take
bool conv_patch_ok(const GemmArgs& a) {
    if (a.dup_rows) return false;          // the dual store of a shared CFG prefix lives in the general output stage (gemm_common.h)
    if (!g_launch_sw.conv_patch || a.mode != 1 || a.stride != 1 || a.A2 || a.pad0 || a.f8 || a.C8 || a.ln_c1 || a.geglu || a.rowvec || a.gate || a.splitk > 1) return false;
    const bool narrow = a.N <= 16;      // conv_last / conv_out: 3 or 4 output channels, element-wise epilogue (no residuals), loader-wave kernel with one column tile
    if (!narrow && a.N != 32 && a.N != 64 && a.N != 128) return false;
    if (narrow && (a.R || a.R2 || a.gn_partial || !g_launch_sw.conv_patch_ws)) return false;
    if (a.act != 0 && a.act != 3) return false;
    if (a.Cin % 64 || a.Cin < 64 || a.K != 9 * a.Cin || a.Hout % CP_TH || a.Wout % CP_TW || a.Hv != a.Hout || a.Wv != a.Wout) return false;      // Cin % 64: 3 Cin / 32 steps in groups of 6
    if (a.lda % 8 || (!narrow && ((a.C && a.ldc % 4) || (a.R && a.ldr % 4) || (a.R2 && a.ldr2 % 4) || (a.Cf && a.ldcf % 4)))) return false;
    const long nimg = a.M / ((long)a.Hout * a.Wout);
    if (nimg * a.Hin * a.Win * a.lda * 2 >= 0x7fffffffL) return false;      // 32-bit buffer offsets
    const long ntiles = nimg * (a.Hout / CP_TH) * (a.Wout / CP_TW);
    if (a.gn_partial && (a.N != 128 || a.gn_cpg != 4 || a.gn_G != 32 || a.gn_hw != a.Hout * a.Wout || a.gn_nchunk != (a.Hout / CP_TH) * (a.Wout / CP_TW))) return false;
    return ntiles >= (narrow ? 64 : 256);      // at least one tile per CU; the 3 / 4-channel tails win from 64 tiles on (UNet out conv at 128^2 x 2: 39 -> see profiles/r05)
}
// gemm_gn_fuse's question for this kernel: chunks per image if the epilogue can produce the consumer GroupNorm's statistics, else 0
int conv_patch_gn_chunks(const GemmArgs& a, int HW, int G) {
    GemmArgs t = a; t.gn_partial = nullptr;
    if (!conv_patch_ok(t) || a.N != 128 || G != 32 || HW != a.Hout * a.Wout) return 0;
    return (a.Hout / CP_TH) * (a.Wout / CP_TW);
}

// The one place that decides which kernel a launch runs (ldx_kernels.h): pure arithmetic over the arguments and g_sw.
GemmPick gemm_pick(const GemmArgs& a, const GemmArgs* b) {
    GemmPick p{GF_TILE, 0, 0, 0, false, false, 1, RED_NONE, 1};
    const auto tile = [&p](GemmFamily f, int bm, int bn, int wm = 2) { p.family = f; p.bm = bm; p.bn = bn; p.wm = wm; return p; };
    if (b && (a.M <= 0 || a.N <= 0)) return gemm_pick(*b);
    if (b && (b->M <= 0 || b->N <= 0)) return gemm_pick(a);
    if (b) {        // two problems: both plain mode, no split-K, no GEGLU, same operand kind (16-bit or MX); 128 x 128 tiles, or 256-row ping-pong tiles
        int bn = 0;
        if (a.f8 && b->f8 && a.M + b->M >= 1024 && b->N >= 256)       // MX: the two streams of a Flux double block / the two halves of linear1
            bn = mx_pp_bn((a.M + 255) / 256, (a.M + 127) / 128, a.N, a.K < b->K ? a.K : b->K, 1, a.C8 || b->C8, (b->M + 255) / 256, (b->M + 127) / 128, b->N);
        if (!bn) bn = gemm2_pp_bn(a, *b);
        p.f8 = a.f8 != 0;
        return bn ? tile(p.f8 ? GF_PP2_MX : GF_PP2, 256, bn, 0) : tile(p.f8 ? GF_TILE2_MX : GF_TILE2, 128, 128);
    }
    if (a.M <= 0 || a.N <= 0) { p.launches = 0; return p; }
    if (a.mode == 1 && a.up2x) return tile(GF_PP, 256, 160, 0);      // phase-form up conv (gemm_upconv_phase made the arguments): the one instantiation of gemm_pp.inc's MODE 2
    if (a.mode == 1 && conv_patch_ok(a)) return tile(GF_CONV_PATCH, CONV_PATCH_BM, a.N <= 16 ? 16 : a.N, 0);      // conv_patch.hip: narrow 3x3 convs with the input patch resident in LDS
    p.f8 = a.mode == 0 && a.f8;
    p.lnf = a.mode == 0 && !p.f8 && a.ln_c1;      // LayerNorm folded in (no split-K): the tile shapes a transformer block's q|k|v / q / GEGLU projections take
    if (a.splitk > 1 && a.ws && !a.geglu && !p.lnf) {
        p.S = a.splitk; p.reduce = gemm_sk_fixup(a) ? RED_IN_KERNEL : a.gn_partial ? RED_LAUNCH_GN : RED_LAUNCH;      // in-kernel: by the last workgroup of every tile
        p.launches = p.reduce == RED_IN_KERNEL ? 1 : 2;
    }
    if (p.f8) {        // MX fp8 operands: a K-tile holds 128 elements, so the tile heuristics see K / 2
        const int fw = g_sw.tile % 1000;
        const int bn = g_sw.tile ? (g_sw.tile / 1000 == 256 ? (fw == 192 ? 192 : a.C8 ? 128 : (fw == 224 ? 224 : fw == 160 ? 160 : 128)) : 0)
                                 : (a.M >= 1024 ? mx_pp_bn((a.M + 255) / 256, (a.M + 127) / 128, a.N, a.K, p.S, a.C8 != nullptr) : 0);
        if (bn) return tile(GF_PP_MX, 256, bn, 0);
        const TileSel t = gemm_tile(a.M, a.N, a.K / 2, a.geglu != 0, p.S, false);      // (256 x 128 register-staged only when forced)
        if (t.bm == 256 && t.bn == 128) return tile(GF_TILE_MX, 256, 128, 4);
        return t.bm == 64 ? tile(GF_TILE_MX, 64, 64) : tile(GF_TILE_MX, 128, t.bn == 160 && !a.C8 ? 160 : 128);
    }
    const TileSel t = gemm_tile(a.M, a.N, a.K, a.geglu != 0, p.S, true, a.mode == 0 && !a.ln_c1);
    if (t.bm == 256) {        // ping-pong: the widths that exist — LayerNorm fold 160 / 128, GEGLU 256 / 128 (two or one 64-column slabs per wave), convs 256 / 160 / 128, plain GEMMs all five
        const int w = t.bn;
        if (p.lnf) return tile(GF_PP, 256, w != 128 && !a.geglu ? 160 : 128, 0);
        if (a.geglu) return tile(GF_PP, 256, w == 256 ? 256 : 128, 0);
        if (a.mode == 1) return tile(GF_PP, 256, w == 256 || w == 160 ? w : 128, 0);
        return tile(GF_PP, 256, w == 256 || w == 224 || w == 192 || w == 160 ? w : 128, 0);
    }
    if (p.lnf) return t.bm == 64 ? tile(GF_TILE, 64, 64) : tile(GF_TILE, 128, t.bn == 160 && !a.geglu ? 160 : 128);
    if (t.bn == 32) return tile(GF_TILE, 128, 32);
    if (t.bm == 128 && t.bn == 64) return tile(GF_TILE, 128, 64);
    if (a.geglu && t.bm == 64) return tile(GF_TILE, 128, 128);      // (forced tiles only) the GEGLU pairing needs 64-column wave tiles
    if (a.mode == 0 && t.bm == 64 && t.bn == 160 && p.S == 1 && a.K % BK == 0) return tile(GF_RING, 64, 160, 0);      // gemm_ring.hip
    return t.bm == 64 ? tile(GF_TILE, 64, 64) : tile(GF_TILE, 128, t.bn == 160 ? 160 : 128);
}

// The phase form of a nearest-2x upsample + 3x3 conv (ldx_kernels.h).  What it needs: an exact doubling of a stored image whose rows are whole 16-pixel blocks (the output
// stage maps a 16-row block with one division), whole 16-column blocks, bias as the only epilogue operand, a 16-bit output and one K segment.  The planner (`planned`) also
// leaves the 9-tap op alone where it was given K splits — few rows under a long K: the phase form has no split-K variant, and four phases of so few rows leave most CUs
// idle (SD1.5 at 1024^2: the 16^2 -> 32^2 conv, M 2048 N 1280 sk3) — and where the ping-pong kernels are switched off or a tile is forced (LDX_PP=0, LDX_GEMM_TILE, LDX_SPLITK).
bool gemm_upconv_phase(const GemmArgs& g, bool planned, GemmArgs* ph) {
    if (g.mode != 1 || g.up2x || g.stride != 1 || g.pad0 || g.Hin <= 0 || g.Win <= 0 || g.Hout != 2 * g.Hin || g.Wout != 2 * g.Win || g.Hv != g.Hout || g.Wv != g.Wout || g.Win % 16) return false;
    if (g.Cin <= 0 || g.Cin % BK || g.K != 9 * g.Cin || g.N % 16 || g.M <= 0 || g.M != (g.M / (g.Hout * g.Wout)) * g.Hout * g.Wout) return false;
    if (!g.C || !g.bias || g.Cf || g.A2 || g.R || g.R2 || g.rowvec || g.gate || g.gn_partial || g.dup_rows || g.geglu || g.act || g.oscale != 0.f || g.C8 || g.f8 || g.ln_c1) return false;
    if (planned && (g.splitk > 1 || !g_sw.pp || g_sw.tile || g_sw.splitk)) return false;
    if (ph) {
        *ph = g;
        ph->up2x = 1; ph->K = 4 * g.Cin; ph->Hv = g.Hin; ph->Wv = g.Win; ph->resize = 0;
        ph->splitk = 1; ph->ws = nullptr; ph->sk_count = nullptr;
    }
    return true;
}

// Planner query (GemmArgs::gn_partial): can the epilogue of the kernel gemm_pick gives `a` — or its split-K reduce launch — produce the consumer GroupNorm's
// statistics?  LDX_GN_FUSE=0 switches the fusion off.
int gemm_gn_fuse(GemmArgs& a, int HW, int G, int max_chunks) {
    if (!g_sw.gn_fuse || a.f8 || a.C8 || a.geglu || a.ln_c1 || a.up2x || !a.C || G <= 0 || a.N % G || a.N % 4 || HW <= 0 || a.M % HW) return 0;
    GemmArgs t = a; t.gn_partial = nullptr;
    const GemmPick p = gemm_pick(t);
    const int cpg = a.N / G;
    int nchunk = 0;
    if (p.family == GF_CONV_PATCH) nchunk = conv_patch_gn_chunks(a, HW, G);        // one chunk per 32 x 16-pixel tile (N = 128 only), or no fusion
    else if (p.reduce == RED_LAUNCH) { int R = 1; nchunk = g_sw.gn_fuse_splitk ? splitk_gn_geom(a, HW, G, max_chunks, &R) : 0; }      // split-K: the reduce launch produces the statistics (splitk_reduce_gn_kernel)
    else {        // the tile's own epilogue (with the in-kernel split-K reduction: run by the last workgroup of a tile)
        const bool wide_ok = p.bm == 256 && p.bn > 160 && g_sw.gn_fuse_wide && a.N % p.bn == 0 && a.M % p.bm == 0;      // the column-major output stage of the ping-pong tiles (gemm_common.h GNW): whole tiles only
        if ((p.bn > 160 && !wide_ok) || p.bn % cpg || HW % p.bm || (p.bn / cpg) * 2 > 256) return 0;          // epilogue support (gemm_common.h GNS / GNW); groups must not straddle tile columns, tiles must not straddle images
        nchunk = HW / p.bm;
    }
    if (!nchunk || nchunk > max_chunks) return 0;
    a.gn_cpg = cpg; a.gn_G = G; a.gn_hw = HW; a.gn_nchunk = nchunk;
    return nchunk;
}
bool gemm_gn_fuse_enabled() { return g_sw.gn_fuse; }

// Last defence for GemmArgs::gn_partial: the geometry the plan carries must be what gemm_gn_fuse says about this very launch.  Planner and launcher ask the same
// gemm_pick, so this fires only on a bug inside that one function or on arguments changed after planning — and then aborts instead of feeding the GroupNorm stale rows.
void gemm_gn_check(const GemmArgs& a) {
    GemmArgs t = a;
    const int nchunk = a.gn_partial ? gemm_gn_fuse(t, a.gn_hw, a.gn_G, a.gn_nchunk) : 0;
    if (!a.gn_partial || (nchunk == a.gn_nchunk && t.gn_cpg == a.gn_cpg)) return;
    fprintf(stderr, "ldx: GroupNorm-statistics geometry mismatch: planned for %d chunks of an image of %d rows, %d channels per group; this launch gives %d chunks\n", a.gn_nchunk, a.gn_hw, a.gn_cpg, nchunk);
    abort();
}

// heuristic shared with the planner: how many K splits for an (M, N, K) problem
int gemm_choose_splitk(int M, int N, int K, bool geglu) {
    if (geglu) return 1;
    if (g_sw.splitk && K % BK == 0 && K / BK >= g_sw.splitk * 2) return g_sw.splitk;
    const int bn = (N % 160 == 0 && N % 128 != 0) ? 160 : 128;
    const int tiles = ((M + 127) / 128) * ((N + bn - 1) / bn);
    const int nk = K / BK;
    // one workgroup per CU (193..256 tiles, or that many 160-wide ones) runs a long K loop alone: a CU advances two co-resident
    // workgroups by one K-tile each in about the time a lone one needs for its own, so halving K for twice the workgroups nearly
    // halves the launch; the fp32 partials + reduce pass cost ~15 us (64^2-level 3x3 convs 640 -> 640: 122 -> ~80 us)
    if (!g_sw.no_split2 && K % BK == 0 && nk >= 60) {
        const long mt = (M + 127) / 128;
        const long t160 = (N % 160 == 0) ? mt * (N / 160) : 0;
        if ((tiles > 192 && tiles <= 256) || (tiles > 256 && tiles < 512 && t160 > 192 && t160 <= 256)) return 2;
    }
    // a split costs a second (reduce) launch of ~9 us: only worth it for long K (3x3 convs, FF down-projection)
    if (tiles >= 200 || nk < 40 || K % BK) return 1;
    int s = (440 + tiles / 2) / tiles;        // ~400-480 workgroups: 40 tiles -> 11 (measured best 10), 160 tiles -> 3
    if (s > nk / 5) s = nk / 5;
    if (s > 16) s = 16;
    return s < 2 ? 1 : s;
}

}  // namespace ldx
