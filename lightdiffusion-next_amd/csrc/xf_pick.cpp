// The stage choice of one SpatialTransformer of a UNet plan (ldx_kernels.h: XfPick; ldx_switches.h: PlanSwitches), the shape rules of the row-block kernels it asks
// (rowgemm_ok, xattn_block_ok, ff_block_ok) and the GroupNorm pick: pure host arithmetic, no engine and no device.
// Engine::emit_xf emits what xf_pick says, Engine::fuse_gn_rowgemm asks xf_proj_in_rowgemm, ldx_op_xf_pick shows the pick to tests (tests/golden/xf_picks.json).
#include "ldx_kernels.h"
#include "ldx_switches.h"

namespace ldx {

// The shapes the row-block kernels take (rowgemm.hip, xattn_block.hip, ff_block.hip)
bool rowgemm_ok(const RowGemmArgs& a) {
    if (!g_plan_sw.rowgemm || (a.K != 320 && a.K != 640) || (a.K == 640 && !g_plan_sw.rowgemm640) || a.N <= 0 || a.N % a.K || a.M <= 0 || a.ldx % 8 || a.ldy % 8 || (a.R && a.ldr % 4) || a.pro < 0 || a.pro > 2) return false;
    const int bm = 128 * 320 / a.K;
    if (a.pro >= 1 && (!a.g || !a.b)) return false;
    if (a.pro == 2 && (!a.partial || a.G != 32 || a.HW % bm || a.M % a.HW || a.nchunk < 1 || a.nchunk > GN_NCHUNK)) return false;
    return true;
}
bool xattn_block_ok(const XAttnArgs& a) {
    return g_plan_sw.xattn_fuse && a.C == XA_C && a.heads == XA_H && a.Mk >= 1 && a.Mk <= XA_MK && a.N % XA_BM == 0 && a.M % a.N == 0 && a.ldh % 8 == 0 && a.ldk % 4 == 0 && a.ldv % 8 == 0;
}
bool ff_block_ok(const FFBlockArgs& a) {
    return g_plan_sw.ff_fuse && a.C == FB_C && a.inner == FB_I && a.M > 0 && a.ldh % 8 == 0 && a.b1 != nullptr;
}

// What launch_groupnorm launches (norm.hip)
bool gn_uses_small_kernel(int B, long HW, int C, int G) {
    return G > 0 && (C / G) % 8 == 0 && HW * (C / G) <= g_plan_sw.gn_small_max && (long)G * B >= 32;
}
// The row-block producer's side of the fused statistics (rowgemm.hip writes one row per row block and image): the conditions Engine::fuse_gn_stats plans under
int rowgemm_gn_chunks(const RowGemmArgs& a, int HW, int G, int max_chunks) {
    const int bm = a.K > 0 ? rowblock_rows(a.K) : 0;
    if (!gemm_gn_fuse_enabled() || bm <= 0 || a.pro == 2 || a.N != a.K || G != 32 || HW <= 0 || a.M <= 0 || a.M % HW || HW % bm || HW / bm > max_chunks) return 0;
    if (gn_uses_small_kernel((int)(a.M / HW), HW, a.N, G)) return 0;      // the one-launch small GroupNorm kernel takes it (norm.hip)
    return HW / bm;
}
struct GnGeom { int CH, TX, RY; };
static inline GnGeom gn_geom(int C) {
    const int cpp = C / 8;
    int ch = 1;                                   // chunks per thread: 1, 2 or 4 (template instances)
    while (ch < 4 && (cpp / ch > 256 || cpp % ch)) ch *= 2;
    GnGeom g; g.CH = ch; g.TX = cpp / ch; g.RY = 256 / g.TX; if (g.RY < 1) g.RY = 1;
    return g;
}
GnPick gn_pick(const GroupNormArgs& a) {
    GnPick p{};
    if (a.stats_chunks <= 0 && gn_uses_small_kernel(a.B, a.HW, a.C, a.G)) {
        p.kind = GN_SMALL; p.grid1[0] = a.G; p.grid1[1] = a.B; p.launches = 1;
        return p;
    }
    const GnGeom g = gn_geom(a.C);
    p.CH = g.CH; p.TX = g.TX; p.RY = g.RY;
    if (a.stats_chunks > 0) {           // statistics came with the producer's epilogue: apply only, behind a fold of more rows than gn_apply wants
        p.kind = a.stats_chunks > GN_NCHUNK ? GN_FOLD_APPLY : GN_APPLY;
        p.nchunk = p.kind == GN_FOLD_APPLY ? GN_FOLD : a.stats_chunks;
        if (p.kind == GN_FOLD_APPLY) { p.grid1[0] = GN_FOLD; p.grid1[1] = a.B; }
    } else {
        p.kind = GN_STATS_APPLY;
        // enough pixel chunks to fill the chip (~1024 workgroups), but >= 4 pixels per thread row
        int nchunk = (1024 + a.B - 1) / a.B;
        const int maxc = (a.HW + g.RY * 4 - 1) / (g.RY * 4);
        if (nchunk > maxc) nchunk = maxc;
        if (nchunk > GN_NCHUNK) nchunk = GN_NCHUNK;
        if (nchunk < 1) nchunk = 1;
        p.nchunk = nchunk; p.grid1[0] = nchunk; p.grid1[1] = a.B;
        p.lds = (int)((size_t)g.RY * a.C * 2 * sizeof(float));
    }
    int nblk = (a.HW + g.RY * 8 - 1) / (g.RY * 8);
    if (nblk > 512) nblk = 512;
    if (nblk < 1) nblk = 1;
    p.grid2[0] = nblk; p.grid2[1] = a.B;
    p.launches = p.kind == GN_APPLY ? 1 : 2;
    return p;
}

long rowblock_count(long M, int K) { const int bm = rowblock_rows(K); return (M + bm - 1) / bm * (K / 320); }
// Planner rule for the row-block kernels (rowgemm / xattn_block / ff_block): one workgroup per row block and one workgroup per CU, so below ~3/4 of the
// CUs the tile GEMMs win (SD1.5 512^2 has 64 row blocks per launch: step 6.14 -> 6.83 ms with the row-block kernels) and smaller problems stay on the
// separate launches.  LDX_ROWBLOCK_MINWG moves the limit (0: always).
// In a shared CFG prefix (half the batch: 128 row blocks at 1024^2, bs = 1) the limit is lower: the alternative there is the SAME number of rows on LayerNorm +
// tile-GEMM launches, which measured slower (LN 12.1 + GEMM 46.3 us against 40.6 for the row-block launch of the full batch; profiles/r06/share_*.txt).
bool rowblock_fills_chip(long workgroups, bool prefix) {
    const long min_wg = g_plan_sw.rowblock_minwg, min_wg_prefix = g_plan_sw.rowblock_minwg_prefix;
    return workgroups >= (prefix ? (min_wg_prefix < min_wg ? min_wg_prefix : min_wg) : min_wg);
}
// rowgemm for M rows of an N x K projection behind prologue `pro`: the kernel's own shape rule (operands are only ever tested for being there) and the chip-fill rule.
// Round 6: with nothing to fuse in front (pro = 0: to_out / proj_out + residual) the kernel only competes with the plain tile GEMM, whose output stage went
// lean: at K = 640 and many rows (CFG batch 16: M = 65 536) the tile GEMM wins (92 against 156 us per launch); at bs = 1 (M = 8192) the two are level in the
// step (13.27 against 13.28 ms) and the row block stays.
static char pick_operand[16];
static bool rowgemm_takes(long M, int N, int K, int pro, bool prefix, int HW = 0, int gn_chunks = 0) {
    if (pro == 0 && K == 640 && M > g_plan_sw.plain640_maxm) return false;
    RowGemmArgs a{};
    a.X = a.W = a.Y = pick_operand; a.ldx = K; a.ldy = N; a.M = M; a.N = N; a.K = K; a.pro = pro;
    if (pro == 0) { a.R = pick_operand; a.ldr = N; } else { a.g = a.b = (const float*)pick_operand; }
    if (pro == 2) { a.partial = (const float*)pick_operand; a.nchunk = gn_chunks; a.HW = HW; a.G = 32; }
    return rowgemm_ok(a) && rowblock_fills_chip(rowblock_count(M, K), prefix);
}
// SpatialTransformer norm + proj_in as one rowgemm launch with the GroupNorm apply as its prologue: the producer of the input wrote the statistics
// (1 .. GN_NCHUNK rows per image) and the plain GEMM would not be split-K
bool xf_proj_in_rowgemm(int C, long M, int HW, bool prefix, int gn_chunks) {
    return gn_chunks > 0 && gn_chunks <= GN_NCHUNK && gemm_choose_splitk(M, C, C, false) == 1 && rowgemm_takes(M, C, C, 2, prefix, HW, gn_chunks);
}
XfPick xf_pick(const XfShape& s) {
    const int C = s.C;
    const long M = (long)s.B * s.HW, Mp = s.Bshare > 0 ? (long)s.Bshare * s.HW : M;      // rows of the full batch and of the shared prefix
    const bool prefix = Mp != M;
    XfPick p{};
    // Folded LayerNorms (XfBlockW::ln_fold): the q|k|v / q / GEGLU GEMM reads h itself, accumulates each row's statistics from its own A
    // fragments and normalises in its epilogue (GemmArgs::ln_c1): no LayerNorm launch, no normalised copy of h.  A split-K consumer keeps a
    // plain (affine-free) LayerNorm launch in front of the folded weights.
    // Per level: folded where the row-block kernels do not take the level's projections (fewer than ~192 row blocks) and the level is small (measured,
    // same box: 512^2 step 6.00 -> 5.88 ms with all three levels folded, 430 -> 382 launches; 1024^2 14.23 -> 14.25 with only the 32^2 level folded
    // (neutral), 14.29 when the 64^2 level's rowgemm launches are replaced too; 8192 rows at C = 1280 (latent 256^2: HiresFix) lose 8 % of an evaluation:
    // the folded GEGLU projection runs on the 128-row tiles instead of the ping-pong ones).  The limit is on rows x C; LDX_LNFOLD_MAXROWS moves it
    // (rows at C = 320; 0: never).  The row blocks are counted on the full batch, under a shared prefix against the prefix limit.
    const bool rowblocks = (C == 320 || C == 640) && rowblock_fills_chip(rowblock_count(M, C), prefix);
    p.fold = s.ln_fold && !rowblocks && M * C <= g_plan_sw.lnfold_maxrows * 320;      // 8192 rows at C = 320, 2048 at C = 1280
    p.proj_in_rowgemm = xf_proj_in_rowgemm(C, Mp, s.HW, prefix, s.gn_chunks);
    auto norm_gemm = [&](long rows, int N, bool geglu, bool rowblock, bool pfx) {
        if (!p.fold) return rowblock && rowgemm_takes(rows, N, C, 1, pfx) ? XS_ROWBLOCK : XS_LN_GEMM;
        return gemm_choose_splitk(rows, N, C, geglu) == 1 ? XS_FOLDED : XS_LN_FOLDED;
    };
    auto out_gemm = [&](long rows, bool rowblock, bool pfx) { return rowblock && rowgemm_takes(rows, C, C, 0, pfx) ? XS_ROWBLOCK : XS_TILE; };
    auto n_ops = [](XfStage st) { return st == XS_LN_GEMM || st == XS_LN_FOLDED ? 2 : 1; };
    auto block = [&](long rows, bool pfx) {          // the self-attention half runs on `rows` rows, everything behind it on the full batch
        XfBlockPick b{};
        b.qkv = norm_gemm(rows, 3 * C, false, true, pfx);
        b.o1 = out_gemm(rows, true, pfx);
        XAttnArgs xa{};          // the row stride of the batched k|v projection is a sum of 2 C over the transformers: as divisible as 2 C
        xa.M = M; xa.N = s.HW; xa.C = C; xa.heads = s.heads; xa.Mk = s.Mc; xa.ldh = C; xa.ldk = xa.ldv = 2 * C;
        b.xattn = !p.fold && xattn_block_ok(xa) && rowblock_fills_chip((M + 127) / 128, false);
        b.q2 = norm_gemm(M, C, false, g_plan_sw.rowgemm_x2, false);          // C = 640: LayerNorm + q projection as one row-block launch
        b.o2 = out_gemm(M, g_plan_sw.rowgemm_x2, false);
        FFBlockArgs fa{};
        fa.M = M; fa.C = C; fa.inner = 4 * C; fa.ldh = C; fa.b1 = (const float*)pick_operand;
        b.ffblock = !p.fold && ff_block_ok(fa) && rowblock_fills_chip((M + 127) / 128, false);
        b.ff1 = norm_gemm(M, 8 * C, true, false, false);
        b.ops = n_ops(b.qkv) + 2 + (b.xattn ? 1 : n_ops(b.q2) + 2) + (b.ffblock ? 1 : n_ops(b.ff1) + 1);
        return b;
    };
    p.first = block(Mp, prefix);
    p.rest = block(M, false);
    p.proj_out = out_gemm(M, g_plan_sw.rowgemm_po, false);
    p.ops_outer = (p.proj_in_rowgemm ? 1 : 2) + 1;
    return p;
}

}  // namespace ldx
