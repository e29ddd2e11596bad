// The one place that reads the environment (ldx_switches.h): one reader per parse rule, every switch's name and default, and the switch objects themselves, so that no
// other translation unit's static initialiser depends on the order they are built in.
#include "ldx_switches.h"

#include <cstdlib>

#include "ldx_kernels.h"

namespace ldx {

// a number with a default
static long env_long(const char* name, long dflt) { const char* v = getenv(name); return v ? atol(v) : dflt; }
static int env_int(const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; }
static double env_double(const char* name, double dflt) { const char* v = getenv(name); return v ? atof(v) : dflt; }
static float env_float_or_nan(const char* name) { const char* v = getenv(name); return v ? (float)atof(v) : __builtin_nanf(""); }
static bool env_unless_0(const char* name) { const char* v = getenv(name); return !(v && atoi(v) == 0); }      // on unless set to 0
static bool env_nonzero(const char* name) { const char* v = getenv(name); return v && atoi(v) != 0; }
static bool env_set(const char* name) { return getenv(name) != nullptr; }                                       // set at all, even to nothing

GemmSwitches::GemmSwitches()
    : pp(env_int("LDX_PP", 1)), pp_mink(env_int("LDX_PP_MINK", 1024)), pp_mink_mx(env_int("LDX_PP_MINK_MX", 2048)),
      pp_r224(env_double("LDX_PP224_RATE", 1.33)), pp_r192(env_double("LDX_PP192_RATE", 1.29)),
      mx_r224(env_double("LDX_MX224_RATE", 2.08)), mx_r192(env_double("LDX_MX192_RATE", 2.1)),
      tile(env_int("LDX_GEMM_TILE", 0)),
      no_tile160(env_set("LDX_NO_TILE160")), no_split2(env_set("LDX_NO_SPLIT2")),
      splitk(env_int("LDX_SPLITK", 0)),
      skgn_chunks(env_int("LDX_SKGN_CHUNKS", GN_NCHUNK)),
      gn_fuse(env_unless_0("LDX_GN_FUSE")), gn_fuse_splitk(env_unless_0("LDX_GN_FUSE_SPLITK")), gn_fuse_wide(env_unless_0("LDX_GN_FUSE_WIDE")),
      sk_fixup(env_nonzero("LDX_SK_FIXUP")), sk_fixup_max(env_int("LDX_SK_FIXUP_MAX", SK_FIXUP_MAX_S)),
      ep_general(env_int("LDX_EP_GENERAL", 0)) {}
const GemmSwitches g_sw;

AttnSwitches::AttnSwitches()
    : pipe(env_unless_0("LDX_ATTN_PIPE")), pipe128(env_unless_0("LDX_ATTN_PIPE128")),
      pipe_minwg40(env_long("LDX_ATTN_PIPE_MINWG", 256)), pipe_minwg128(env_long("LDX_ATTN_PIPE_MINWG", 192)),      // one name, two defaults: D = 40 / D = 128
      pipe_thr(env_float_or_nan("LDX_ATTN_PIPE_THR")), pipe_kb(env_unless_0("LDX_ATTN_PIPE_KB")),
      attn32(env_int("LDX_ATTN32", 1)), ap(env_int("LDX_ATTN32_AP", 1)), ap_minwg(env_long("LDX_ATTN32_AP_MINWG", 256)),
      kvb(env_int("LDX_ATTN32_KVB", 64)), var(env_int("LDX_ATTN32_VAR", 1)),
      kpf(env_unless_0("LDX_ATTN_KPF")), g32_mask(env_int("LDX_ATTN32G", 7)), g32_minwg(env_long("LDX_ATTN32G_MINWG", 16)),
      a512(env_unless_0("LDX_ATTN512")), a512_splits(env_int("LDX_ATTN512_SPLITS", 0)) {}
AttnSwitches g_attn_sw;
void reload_dispatch_env() { g_attn_sw = AttnSwitches(); }

#ifndef LDX_LNFOLD_MAXROWS_DEFAULT
#define LDX_LNFOLD_MAXROWS_DEFAULT 8192      // rows of a transformer level up to which its LayerNorms are folded into the consuming GEMMs (emit_xf)
#endif
PlanSwitches::PlanSwitches()
    : rowblock_minwg(env_long("LDX_ROWBLOCK_MINWG", 192)), rowblock_minwg_prefix(env_long("LDX_ROWBLOCK_MINWG_PREFIX", 96)),
      plain640_maxm(env_long("LDX_ROWGEMM_PLAIN640_MAXM", 16384)), lnfold_maxrows(env_long("LDX_LNFOLD_MAXROWS", LDX_LNFOLD_MAXROWS_DEFAULT)),
      gn_small_max(env_long("LDX_GN_SMALL_MAX", 256 * 80)),
      rowgemm(env_unless_0("LDX_ROWGEMM")), rowgemm640(env_unless_0("LDX_ROWGEMM640")), rowgemm_x2(env_unless_0("LDX_ROWGEMM_X2")), rowgemm_po(env_unless_0("LDX_ROWGEMM_PO")),
      xattn_fuse(env_unless_0("LDX_XATTN_FUSE")), ff_fuse(env_unless_0("LDX_FF_FUSE")),
      cfg_share_copy(env_nonzero("LDX_CFG_SHARE_COPY")), cfg_share_minrows(env_long("LDX_CFG_SHARE_MINROWS", 8192)),
      fused_skip(!env_set("LDX_NO_FUSED_SKIP")), q_prescale(!env_set("LDX_NO_QPRESCALE")), lnfold(env_unless_0("LDX_LNFOLD")), emb_table(env_unless_0("LDX_EMB_TABLE")),
      plan_cache_gib(env_double("LDX_PLAN_CACHE_GIB", 16.0)), mx_fuse(env_int("LDX_MX_FUSE", 7)),
      flux_fp8_attn(env_unless_0("LDX_FLUX_FP8_ATTN")), flux_group(env_unless_0("LDX_FLUX_GROUP")), flux_mod_fp8(env_unless_0("LDX_FLUX_MOD_FP8")),
      vae_attn_chunk_mib(env_long("LDX_VAE_ATTN_CHUNK_MIB", 2048)) {}
const PlanSwitches g_plan_sw;

LaunchSwitches::LaunchSwitches()
    : ring(env_int("LDX_RING", 1)), conv_patch(env_unless_0("LDX_CONV_PATCH")), conv_patch_ws(env_unless_0("LDX_CONV_PATCH_WS")),
      cp_abl(env_int("LDX_CP_ABL", 0)), rg_abl(env_int("LDX_RG_ABL", 0)), ln_lpr(env_int("LDX_LN_LPR", 0)),
      attn_mx_qt(env_int("LDX_ATTN_MX_QT", 1)), attn512_abl(env_int("LDX_ATTN512_ABL", 0)), attn512_var(env_int("LDX_ATTN512_VAR", 0)),
      attn_pipe_abl(env_int("LDX_ATTN_PIPE_ABL", 0)), xa_dbg(env_int("LDX_XA_DBG", 0)), debug_nan(env_set("LDX_DEBUG_NAN")) {}
const LaunchSwitches g_launch_sw;

UNetSwitches::UNetSwitches() : cfg_share(env_int("LDX_CFG_SHARE", 1)), upconv_phase(env_int("LDX_UPCONV_PHASE", 1)) {}

}  // namespace ldx
