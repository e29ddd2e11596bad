// Every LDX_* environment switch of the native library: the structs here; their objects, every name and default, and the only reads of the environment in
// ldx_switches.cpp.  A switch is read at one of three times:
//   at load, never again       GemmSwitches, PlanSwitches, LaunchSwitches
//   at load and again on reload_dispatch_env() (C ABI: ldx_reload_env)      AttnSwitches
//   when a UNetEngine is constructed      UNetSwitches
// No launch path reads the environment.
#pragma once

namespace ldx {

// The switches behind which kernel a GEMM / convolution runs (gemm_pick.cpp); "set at all" stays apart from "non-zero" where the two differ.  Deliberately NOT re-read by
// reload_dispatch_env(): plans bake these decisions into their op arguments (splitk, gn_nchunk), and a reload between planning and launching would make the two disagree.
struct GemmSwitches {
    int pp, pp_mink, pp_mink_mx;       // LDX_PP, LDX_PP_MINK, LDX_PP_MINK_MX: ping-pong kernel: 0 off, 1 cost model, 2 whenever a candidate fills >= 3/4 of the CUs; its shortest K
    double pp_r224, pp_r192;           // LDX_PP224_RATE, LDX_PP192_RATE: cost-model rates of the 224 / 192 wide tiles (0: never)
    double mx_r224, mx_r192;           // LDX_MX224_RATE, LDX_MX192_RATE
    int tile;                          // LDX_GEMM_TILE: experiment switch: BM * 1000 + BN for every launch
    bool no_tile160, no_split2;        // LDX_NO_TILE160, LDX_NO_SPLIT2: set at all, even to nothing
    int splitk;                        // LDX_SPLITK: experiment switch: K splits wherever K allows
    int skgn_chunks;                   // LDX_SKGN_CHUNKS: experiment switch: chunks per image of the reduce + GroupNorm launch (fewer = fatter workgroups)
    bool gn_fuse, gn_fuse_splitk, gn_fuse_wide;      // LDX_GN_FUSE, LDX_GN_FUSE_SPLITK, LDX_GN_FUSE_WIDE = 0: off
    bool sk_fixup; int sk_fixup_max;   // LDX_SK_FIXUP non-zero, LDX_SK_FIXUP_MAX
    int ep_general;                    // LDX_EP_GENERAL -> GemmArgs::ep_general
    GemmSwitches();
};
extern const GemmSwitches g_sw;

// Every runtime LDX_ATTN* switch behind attn_pick (attn_pick.cpp).  Experiments and tests that flip one inside a process call reload_dispatch_env() after changing the environment.
struct AttnSwitches {
    bool pipe, pipe128;            // LDX_ATTN_PIPE / LDX_ATTN_PIPE128 = 0: the pipelined D = 40 / D = 128 kernels off (attn32ap / attn32, attn32g instead)
    long pipe_minwg40, pipe_minwg128;      // LDX_ATTN_PIPE_MINWG: fewest 256-query workgroups they take (256: the chip; 192: three quarters of the CUs in one round)
    float pipe_thr;                // LDX_ATTN_PIPE_THR: their rescale threshold (tests force the rare path with small values); NaN = the type's own
    bool pipe_kb;                  // LDX_ATTN_PIPE_KB = 0 (experiment): the exact maximum on every key block even with AttnArgs::knorm_ws
    int attn32;                    // LDX_ATTN32 = 0: D = 40 back on the 16x16 kernel.  On 32x32x16 MFMAs: +4.6 % in isolation, +2.2 % on the whole step
    // LDX_ATTN32_AP, the 8-wave two-group kernel (round 3, attn32ap.inc) when its 512-query workgroups still fill the chip (LDX_ATTN32_AP_MINWG): 0 off, 1 (default) phases
    // separated by the barriers only (hipcc interleaves the next PV MFMAs with the softmax), 2 strict phases, 3 strict + s_setprio around the MFMAs.
    // Same box, B2 H8 N16384 D40: attn32_kernel 1.197 ms, strict 1.14-1.21, default 1.12-1.15; step 60.02 -> 61.18 it/s.
    int ap; long ap_minwg;
    // attn32_kernel: LDX_ATTN32_VAR 1: V^T fragments prefetched before the softmax (1.219 -> 1.206 ms at B2 H8 N16384, twice on one box); 0: read at the PV MFMAs, and then
    // LDX_ATTN32_KVB = 128 (experiment) stages 128 keys per block from Mk = 1024 on
    int kvb, var;
    bool kpf;                      // LDX_ATTN_KPF = 0: attn32g without its K fragment prefetch ring (round 3): hipcc's just-in-time reads
    // head dims served by the generic 32x32x16 kernel (LDX_ATTN32G bit mask 1: D=80, 2: D=160, 4: D=128, 8: D=64).  Default 7: same-box step A/B 54.76 -> 55.34 it/s with
    // D = 80 and 160; D = 128 (Flux, VALU denominator instead of a fifth d tile) 19.6 -> 18.4 ms of attention per forward; D = 64 only appears with a causal mask or a
    // bias on this path.  LDX_ATTN32G_MINWG 64 -> 16: +0.9 % on the 512^2 step (the 16x16 D = 160 instantiation spills)
    int g32_mask; long g32_minwg;
    bool a512; int a512_splits;    // LDX_ATTN512 = 0: no D = 512 kernel (the VAE falls back to GEMMs and a row softmax); LDX_ATTN512_SPLITS > 0 forces its key-split count
    AttnSwitches();
};
extern AttnSwitches g_attn_sw;
// re-reads every field of AttnSwitches, and nothing else (tests / same-process A/B runs only)
void reload_dispatch_env();

// Every LDX_* switch behind the stage choice of a SpatialTransformer and the one-launch GroupNorm (xf_pick.cpp), and the engines' own planning switches.
// Deliberately NOT re-read by reload_dispatch_env(): plans bake these decisions into their op lists, and a reload between planning and launching would make the two disagree.
struct PlanSwitches {
    long rowblock_minwg, rowblock_minwg_prefix;      // LDX_ROWBLOCK_MINWG / _PREFIX: fewest workgroups a row-block launch may have (rowblock_fills_chip)
    long plain640_maxm;                              // LDX_ROWGEMM_PLAIN640_MAXM: most rows of a K = 640 rowgemm without a prologue
    long lnfold_maxrows;                             // LDX_LNFOLD_MAXROWS: rows at C = 320 up to which a level folds its LayerNorms (0: never)
    long gn_small_max;                               // LDX_GN_SMALL_MAX: elements per (image, group) the one-launch GroupNorm kernel takes
    bool rowgemm, rowgemm640, rowgemm_x2, rowgemm_po, xattn_fuse, ff_fuse;      // LDX_ROWGEMM, LDX_ROWGEMM640, LDX_ROWGEMM_X2, LDX_ROWGEMM_PO, LDX_XATTN_FUSE, LDX_FF_FUSE: 0 switches the kernel (or that use of it) off
    // the engines' own planning and weight-packing switches (engine*.cpp say what each is for)
    bool cfg_share_copy; long cfg_share_minrows;     // LDX_CFG_SHARE_COPY != 0: the shared CFG prefix is handed over by copy launches only; LDX_CFG_SHARE_MINROWS: rows per half from which share mode 1 shares
    bool fused_skip, q_prescale, lnfold, emb_table;  // LDX_NO_FUSED_SKIP / LDX_NO_QPRESCALE set (to anything): off; LDX_LNFOLD / LDX_EMB_TABLE = 0: off
    double plan_cache_gib;                           // LDX_PLAN_CACHE_GIB: GiB of stashed arenas the plan cache keeps
    int mx_fuse;                                     // LDX_MX_FUSE: 1 GEMM epilogue, 2 attention, 4 LayerNorm write the MX shadow themselves
    bool flux_fp8_attn, flux_group, flux_mod_fp8;    // LDX_FLUX_FP8_ATTN / LDX_FLUX_GROUP / LDX_FLUX_MOD_FP8 = 0: off
    long vae_attn_chunk_mib;                         // LDX_VAE_ATTN_CHUNK_MIB: score rows per chunk of the VAE's three-GEMM attention, in MiB (0: one chunk)
    PlanSwitches();
};
extern const PlanSwitches g_plan_sw;

// The launchers' own experiment, ablation and debug switches: each belongs to one launcher (or its shape rule) and changes which instantiation it runs or what it
// passes to the kernel.
struct LaunchSwitches {
    int ring;                      // LDX_RING (gemm_ring_ok): 0 switches the ring kernel off, 2 takes every plain GEMM with N % 160 == 0 that fills the chip
    bool conv_patch;               // LDX_CONV_PATCH = 0: no patch-resident conv (conv_patch_ok)
    bool conv_patch_ws;            // LDX_CONV_PATCH_WS = 0: every wave loads and multiplies (the kernel N = 128 uses)
    int cp_abl;                    // LDX_CP_ABL: conv_patch timing ablations (wrong results): 1 no patch loads, 2 no weight loads, 4 no MFMAs (N = 32), 8 no stores, 16 no fragment reads (N = 32), 32 no per-tile offset recomputation (loader-wave kernel)
    int rg_abl;                    // LDX_RG_ABL -> RowGemmArgs::abl
    int ln_lpr;                    // LDX_LN_LPR: 32 / 64 force the LayerNorm kernel's lanes per row where the row fits
    int attn_mx_qt;                // LDX_ATTN_MX_QT = 2: the four-wave attn_mx instantiation (launch_attn_mx has the measurements)
    int attn512_abl, attn512_var;  // LDX_ATTN512_ABL: timing ablations of attn512_kernel (bf16); LDX_ATTN512_VAR (experiment): KPF * 10 + NCH
    int attn_pipe_abl;             // LDX_ATTN_PIPE_ABL: timing ablations of the pipelined kernels; only builds with -DLDX_ATTN_ABLATE look at it
    int xa_dbg;                    // LDX_XA_DBG: copied to xattn_block.hip's device symbol at its first launch (builds with -DXA_ABLATE)
    bool debug_nan;                // LDX_DEBUG_NAN set (to anything): Engine::exec_ops reports the first GEMM whose 16-bit output holds a NaN / Inf
    LaunchSwitches();
};
extern const LaunchSwitches g_launch_sw;

struct UNetSwitches {
    int cfg_share;                 // LDX_CFG_SHARE: 0 off, 1 where it pays (share_for), 2 whenever possible
    int upconv_phase;              // LDX_UPCONV_PHASE: 0: every up conv stays a 9-tap op; 1 / 2: phase form, tiles phase-major / band-major (GemmArgs::up2x)
    UNetSwitches();                // reads the environment as it is now: one per UNetEngine
};

}  // namespace ldx
