// The stage choice of one SpatialTransformer of a UNet plan (ldx_kernels.h: PlanSwitches, XfPick): pure host arithmetic, no engine and no device.
// Engine::emit_xf emits what xf_pick says, Engine::fuse_gn_rowgemm asks xf_proj_in_rowgemm, ldx_op_xf_pick shows the pick to tests (tests/golden/xf_picks.json).
#include "ldx_kernels.h"

#include <cstdlib>

namespace ldx {

#ifndef LDX_LNFOLD_MAXROWS_DEFAULT
#define LDX_LNFOLD_MAXROWS_DEFAULT 8192      // rows of a transformer level up to which its LayerNorms are folded into the consuming GEMMs (emit_xf)
#endif
// Read once when the library loads and deliberately NOT re-read by reload_dispatch_env(): plans bake these decisions into their op lists, and a reload between
// planning and launching would make the two disagree (the reason gemm.hip gives for its own switches).
static long env_long(const char* name, long dflt) { const char* v = getenv(name); return v ? atol(v) : dflt; }
static bool env_unless_0(const char* name) { const char* v = getenv(name); return !(v && atoi(v) == 0); }
PlanSwitches::PlanSwitches()
    : rowblock_minwg(env_long("LDX_ROWBLOCK_MINWG", 192)), rowblock_minwg_prefix(env_long("LDX_ROWBLOCK_MINWG_PREFIX", 96)),
      plain640_maxm(env_long("LDX_ROWGEMM_PLAIN640_MAXM", 16384)), lnfold_maxrows(env_long("LDX_LNFOLD_MAXROWS", LDX_LNFOLD_MAXROWS_DEFAULT)),
      gn_small_max(env_long("LDX_GN_SMALL_MAX", 256 * 80)),
      rowgemm(env_unless_0("LDX_ROWGEMM")), rowgemm640(env_unless_0("LDX_ROWGEMM640")), rowgemm_x2(env_unless_0("LDX_ROWGEMM_X2")), rowgemm_po(env_unless_0("LDX_ROWGEMM_PO")),
      xattn_fuse(env_unless_0("LDX_XATTN_FUSE")), ff_fuse(env_unless_0("LDX_FF_FUSE")),
      cfg_share_copy(getenv("LDX_CFG_SHARE_COPY") && atoi(getenv("LDX_CFG_SHARE_COPY")) != 0), cfg_share_minrows(env_long("LDX_CFG_SHARE_MINROWS", 8192)),
      fused_skip(!getenv("LDX_NO_FUSED_SKIP")), q_prescale(getenv("LDX_NO_QPRESCALE") == nullptr), lnfold(env_unless_0("LDX_LNFOLD")), emb_table(env_unless_0("LDX_EMB_TABLE")),
      plan_cache_gib(getenv("LDX_PLAN_CACHE_GIB") ? atof(getenv("LDX_PLAN_CACHE_GIB")) : 16.0), mx_fuse(getenv("LDX_MX_FUSE") ? atoi(getenv("LDX_MX_FUSE")) : 7),
      flux_fp8_attn(env_unless_0("LDX_FLUX_FP8_ATTN")), flux_group(env_unless_0("LDX_FLUX_GROUP")), flux_mod_fp8(env_unless_0("LDX_FLUX_MOD_FP8")),
      vae_attn_chunk_mib(env_long("LDX_VAE_ATTN_CHUNK_MIB", 2048)) {}
const PlanSwitches g_plan_sw;

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
