// Which kernel launch_attention takes (ldx_kernels.h: AttnPick) and the shape rules of the attention kernels: pure host arithmetic over the arguments and
// AttnSwitches (ldx_switches.h), no engine and no device.  The kernels, their launchers and the instantiation tables are in attention.hip, attn_pipe*.hip,
// attn512.hip and attn_mx.hip; the LDS geometry a pick reports is in ldx_geometry.h.
#include "ldx_kernels.h"
#include "ldx_switches.h"

namespace ldx {

// Shapes the special-purpose kernels take.  attn512.hip: one head of D = 512 (VAE mid-block attention)
static bool attn512_ok(const AttnArgs& a) {
    return a.D == 512 && !a.causal && !a.bias && !a.O8 && a.Nq > 0 && a.Mk > 0 && a.B > 0 && a.H > 0 && a.ldq % 8 == 0 && a.ldk % 8 == 0 && a.ldv % 8 == 0 && a.ldo % 4 == 0;
}
// its key splits: enough workgroups for the chip (>= 224 of 256 CUs), never more than 8, each split at least 16 key blocks
static int attn512_splits(const AttnArgs& a, int force) {
    const long wgs = (long)((a.Nq + ATTN512_QB - 1) / ATTN512_QB) * a.H * a.B;
    const int nblk = (a.Mk + ATTN512_KV - 1) / ATTN512_KV;
    int s = force > 0 ? force : (int)((255 + wgs) / wgs);
    if (s > 8) s = 8;
    while (s > 1 && nblk / s < 16) --s;
    if (force > 0 && s > nblk) s = nblk;
    return s < 1 ? 1 : s;
}
// attn_pipe.hip (D = 40, 16-bit output) and attn_pipe128.hip (D = 128, 16-bit or MX fp8 output): whole 256-query workgroups, whole pairs of key blocks, 16-byte rows
bool attn_pipe_ok(const AttnArgs& a) {
    if ((a.D != 40 && a.D != 128) || a.causal || a.bias || a.Nq % 256 || a.Mk % 128 || a.Mk < 256 || a.ldq % 8 || a.ldk % 8 || a.ldv % 8) return false;
    if (a.D == 40) return !a.O8 && a.ldo % 4 == 0;
    return a.O8 ? (a.ldo8 % 16 == 0 && ((uintptr_t)a.O8 & 15) == 0) : (a.ldo % 8 == 0 && ((uintptr_t)a.O & 15) == 0);
}
// the head dim the generic 32x32x16 kernel takes `a` at, 0: not taken
static int attn32g_dim(const AttnArgs& a, const AttnSwitches& w) {
    if (!w.g32_mask || a.causal || a.bias || (long)((a.Nq + 127) / 128) * a.H * a.B < w.g32_minwg) return 0;
    const int bit = a.D == 80 ? 1 : a.D == 160 ? 2 : a.D == 128 ? 4 : a.D == 64 ? 8 : 0;
    return (w.g32_mask & bit) ? a.D : 0;
}

AttnPick attn_pick(const AttnArgs& a) {
    const AttnSwitches& w = g_attn_sw;
    AttnPick p{};
    p.thr = w.pipe_thr;
    p.mx_out = attn32g_dim(a, w) == 128;
    if (a.Nq <= 0 || a.B <= 0) return p;
    auto take = [&](AttnFamily f, int t0, int t1, int t2, int qb, int block, int lds) {
        p.family = f; p.targ[0] = t0; p.targ[1] = t1; p.targ[2] = t2; p.qb = qb; p.block = block; p.lds = lds;
        p.grid = (unsigned)(((a.Nq + qb - 1) / qb) * a.H * a.B);
        p.nsplit = p.launches = 1;
    };
    const long wg256 = (long)((a.Nq + 255) / 256) * a.H * a.B;      // 256-query workgroups
    if (w.a512 && attn512_ok(a)) {
        take(AF_ATTN512, 0, 0, 0, ATTN512_QB, 256, ATTN512_LDS);
        p.nsplit_want = attn512_splits(a, w.a512_splits);
        p.nsplit = a.nsplit > 1 && a.split_ws ? a.nsplit : 1;        // no workspace: one workgroup walks all keys of its query block
        p.grid *= (unsigned)p.nsplit;
        p.launches = p.nsplit > 1 ? 2 : 1;
        return p;
    }
    // D = 40 self-attention of the large levels: the software-pipelined one-wave-per-SIMD kernel when its 256-query workgroups fill the chip;
    // D = 128 (Flux): the same pipeline when one round of them covers at least three quarters of the CUs
    if (attn_pipe_ok(a) && (a.D == 40 ? w.pipe && wg256 >= w.pipe_minwg40 : w.pipe128 && wg256 >= w.pipe_minwg128)) {
        if (a.D == 40) take(AF_ATTN40P, 0, 0, 0, 256, 256, ATTN40P_LDS); else take(AF_ATTN128P, 0, 0, 0, 256, 256, ATTN128P_LDS);
        p.knorm = a.knorm_ws && w.pipe_kb;
        p.launches = p.knorm ? 2 : 1;
        return p;
    }
    if (const int d = attn32g_dim(a, w)) {
        const bool ones = d == 80 || d == 160;                        // the denominator from a ones row of V (one d tile more at 160); 128, 64: summed on the VALU
        const int nks = d / 16, ndt = d / 32 + (ones ? 1 : 0);        // k-steps of 16, d tiles of 32
        take(AF_ATTN32G, nks, ndt, ones, 128, 256, attn32g_lds(nks, ndt));
        p.kpf = w.kpf;
        return p;
    }
    // 16x16 kernel: KS = ceil(D/32) contraction steps, DT output tiles with room for the ones column at d = D (the instantiations that exist, by largest D)
    static const struct { int dmax, ks, dt; } ladder[] = {{15, 1, 1}, {31, 1, 2}, {32, 1, 3}, {47, 2, 3}, {63, 2, 4}, {64, 2, 5}, {79, 3, 5}, {95, 3, 6}, {96, 3, 7},
                                                          {127, 4, 8}, {128, 4, 9}, {159, 5, 10}, {1 << 30, 5, 11}};
    int i = 0;
    while (a.D > ladder[i].dmax) ++i;
    const int ks = ladder[i].ks, dt = ladder[i].dt;
    if (ks == 2 && dt == 3 && w.attn32 && !a.causal && !a.bias && a.D > 32 && a.D % 8 == 0 && wg256 >= 512) {      // D = 40 (SD1.5 level 0) on 32x32x16 MFMAs
        if (w.ap && a.Mk >= 64 && (long)((a.Nq + 511) / 512) * a.H * a.B >= w.ap_minwg) {
            int var = w.ap == 2 ? 0 : w.ap == 3 ? 1 : 2;      // the kernel's VAR: 2 = phases separated by the barriers only
#ifdef LDX_ATTN_ABLATE      // profiles/ubench/README.md round 3, measured and not adopted (correct, bit-identical): 6 split softmax (VAR & 64), +6 %; 7 K fragments read a phase early (VAR & 128), +-0.5 %;
            // timing ablations (wrong results): 4 no MFMAs, 8 no softmax, 12 neither (staging + barriers + fragment reads), 34 the default schedule without the 64 fma of exp2(s * c - m * c)
            var = w.ap == 6 ? 66 : w.ap == 7 ? 130 : w.ap == 4 || w.ap == 8 || w.ap == 12 || w.ap == 34 ? w.ap : var;
#endif
            take(AF_ATTN32AP, var, 0, 0, 512, 512, attn32_lds(64));
            return p;
        }
        const int kvb = w.var != 1 && w.kvb == 128 && a.Mk >= 1024 ? 128 : 64;
        take(AF_ATTN32, kvb, w.var == 1, 0, 256, 256, attn32_lds(kvb));
        return p;
    }
    // 64 queries per wave (QT = 4) when the accumulators fit (DT <= 3) and the grid still fills the chip.  D >= 144 (DT >= 10): two 16-query tiles per wave need 12 more
    // VGPRs than the file has (40 B of scratch per lane, hipcc -Rpass-analysis): one tile per wave there.  Only small grids / masked calls get here (attn32g takes the rest).
    const int qt = dt <= 3 && wg256 >= 512 && !a.causal ? 4 : dt >= 10 ? 1 : 2;
    take(AF_ATTN, ks, dt, qt, 64 * qt, 256, attn_lds(ks, dt));
    return p;
}

// attn_mx.hip: operands there, 16-byte rows, the V^T buffer padded to whole key blocks
bool attn_mx_ok(const AttnMxArgs& a) {
    return a.Q8 && a.K8 && a.V8T && a.SQ && a.SK && a.SV && (a.O || (a.O8 && a.SO)) && a.B > 0 && a.H > 0 && a.Nq > 0 && a.Mk > 0 && a.ldq8 % 16 == 0 && a.ldk8 % 16 == 0 &&
           a.Lp % AM_KB == 0 && a.Lp >= a.Mk && (!a.O || a.ldo % 4 == 0) && (!a.O8 || a.ldo8 % 4 == 0);
}

}  // namespace ldx
