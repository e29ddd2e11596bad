// Kernel geometry that a host-side pick or shape rule (gemm_pick.cpp, attn_pick.cpp, xf_pick.cpp) shares with the kernel it describes: tile extents, LDS row
// strides and the dynamic-LDS formulas, each written once.  No device code; the kernel files hold a static_assert where they derive the same number on their own.
#pragma once

namespace ldx {

// ---- GEMM / convolution ----
constexpr int BK = 64;                  // elements per K-tile of the 16-bit main loops (gemm.hip, gemm_pp.inc, gemm_ring.hip)
constexpr int GR_BM = 64, GR_BN = 160;  // gemm_ring.hip: tile rows and columns
constexpr int CP_TH = 16, CP_TW = 32;   // conv_patch.hip: output pixels per tile, rows x columns
constexpr int CONV_PATCH_BM = 512;      // ... as output rows: GemmPick::bm of the patch kernel
static_assert(CP_TH * CP_TW == CONV_PATCH_BM, "GemmPick::bm of the patch kernel");

// ---- attention (attention.hip, attn32ap.inc) ----
constexpr int AT_KV = 64;         // keys per block
// attn_kernel's LDS row strides.  K rows: KS*64 B + 32 B pad -> the four 16-lane groups of ds_read_b128 are conflict-free
// (brute-forced over the real lane groups).  V rows: >= DT*32 B and == 32 (mod 64) so the 8 key rows a
// 32-lane half touches in one ds_read_b64_tr_b16 tile the 64 banks.
constexpr int attn_krowb(int KS) { return KS * 64 + 32; }
constexpr int attn_vrowb(int DT) { return (DT * 32) % 64 == 0 ? DT * 32 + 32 : DT * 32; }
constexpr int attn_lds(int KS, int DT) { return 2 * AT_KV * (attn_krowb(KS) + attn_vrowb(DT)); }      // two stages of K and V rows
// attn32_kernel / attn32ap_kernel: K / V row strides 144 / 192 B: 160 / 160 had 2-way conflicts on every fragment read (SQ_LDS_BANK_CONFLICT 88.1 M -> 21.0 M cycles per launch;
// same time at D = 40, which is VALU / MFMA bound)
constexpr int A32_KROW = 144, A32_VROW = 192;
constexpr int attn32_lds(int KVB) { return 2 * KVB * (A32_KROW + A32_VROW); }      // two stages of KVB keys (attn32ap_kernel: KVB = 64)
// LDS row strides of the generic kernel (attn32g_kernel), same rules as attn32_kernel: K rows an odd number of 16-B chunks, V rows 64 B times an
// odd number (LDX_G32_OLD_ROWS at build time restores the first layout for A/B)
#ifdef LDX_G32_OLD_ROWS
#define G32_KROW(NKS) (((NKS) & 1) ? (NKS) * 32 : (NKS) * 32 + 32)
#define G32_VROW(NDT) ((NDT) * 64 + 32)
#else
#define G32_KROW(NKS) ((NKS) * 32 + 16)
#define G32_VROW(NDT) (((NDT) & 1) ? (NDT) * 64 : (NDT) * 64 + 64)
#endif
constexpr int attn32g_lds(int NKS, int NDT) { return 2 * AT_KV * (G32_KROW(NKS) + G32_VROW(NDT)); }
// attn_pipe.hip (D = 40), attn_pipe128.hip (D = 128): stages x 64 keys x (K row + V row)
constexpr int ATTN40P_LDS = 2 * 64 * (144 + 192), ATTN128P_LDS = 3 * 64 * (272 + 320);
constexpr int ATTN512_QB = 128, ATTN512_KV = 32, ATTN512_LDS = 2 * ATTN512_KV * ((512 * 2 + 16) + (512 * 2 + 64));      // attn512.hip: queries per workgroup, keys per block, two stages of K and V rows
constexpr int AM_KB = 128;        // attn_mx.hip: keys per block (AttnMxArgs::Lp is a multiple)

// ---- row-block kernels ----
constexpr int XA_C = 320, XA_H = 8, XA_BM = 128, XA_MK = 80;      // xattn_block.hip: width, heads, rows per workgroup, most context tokens
constexpr int FB_C = 320, FB_I = 1280;                            // ff_block.hip: width, inner width

}  // namespace ldx
