// One sixth of the 16-bit ping-pong instantiations (gemm_pp.inc): included by gemm_pp_{bf16,f16}_{0,1,2}.hip, which define LDX_PP_T (element type),
// LDX_PP_SFX (bf16 / f16) and LDX_PP_PART — 0: plain GEMMs incl. the LayerNorm-folded ones, 1: implicit-GEMM convs + the narrow two-problem launches,
// 2: the wide two-problem launches.  (The phase-form up conv, MODE 2, is instantiated in gemm_pp_up2x.hip: libldx_upconv.so.)  As ONE translation unit these kernels took 700 s to compile (the output stage of gemm_common.h is instantiated in each of the
// 40 kernel bodies); as six they build in parallel with gemm.hip and gemm_pp_mx.hip (≈ 250 s each).  gemm_pp.hip keeps the dispatchers.
#include "gemm_common.h"

namespace ldx {

#include "gemm_pp.inc"

#define LDX_PP_CAT2(a, b) a##b
#define LDX_PP_CAT(a, b) LDX_PP_CAT2(a, b)
#define LDX_PP_FN(name) LDX_PP_CAT(name, LDX_PP_SFX)
using PPT = LDX_PP_T;

#if LDX_PP_PART == 0
void LDX_PP_FN(launch_pp_plain_)(const GemmArgs& a, int bn, bool lnf, int S, hipStream_t s) {
    if (lnf) {            // folded LayerNorm (GemmArgs::ln_c1), no split-K
        if (bn == 160 && !a.geglu) launch_pp_inst<PPT, 0, 160, true>(a, 1, s); else launch_pp_inst<PPT, 0, 128, true>(a, 1, s);
    } else {
        if (bn == 256) launch_pp_inst<PPT, 0, 256>(a, S, s);             // also GEGLU (two 64-column slabs per wave)
        else if (bn == 224 && !a.geglu) launch_pp_inst<PPT, 0, 224>(a, S, s);
        else if (bn == 192 && !a.geglu) launch_pp_inst<PPT, 0, 192>(a, S, s);
        else if (bn == 160 && !a.geglu) launch_pp_inst<PPT, 0, 160>(a, S, s);
        else launch_pp_inst<PPT, 0, 128>(a, S, s);
    }
}
#elif LDX_PP_PART == 1
void LDX_PP_FN(launch_pp_conv_)(const GemmArgs& a, int bn, int S, hipStream_t s) {
    if (bn == 256) launch_pp_inst<PPT, 1, 256>(a, S, s);
    else if (bn == 160) launch_pp_inst<PPT, 1, 160>(a, S, s);
    else launch_pp_inst<PPT, 1, 128>(a, S, s);
}
void LDX_PP_FN(launch_pp2_narrow_)(const GemmArgs& a, const GemmArgs& b, int bn, hipStream_t s) {
    if (bn == 160) launch_pp2_inst<PPT, 160>(a, b, s);
    else launch_pp2_inst<PPT, 128>(a, b, s);
}
#else
void LDX_PP_FN(launch_pp2_wide_)(const GemmArgs& a, const GemmArgs& b, int bn, hipStream_t s) {
    if (bn == 256) launch_pp2_inst<PPT, 256>(a, b, s);
    else if (bn == 224) launch_pp2_inst<PPT, 224>(a, b, s);
    else launch_pp2_inst<PPT, 192>(a, b, s);
}
#endif

}  // namespace ldx
