// TAESD decoder (the sampler loops' latent preview) as a static launch plan over the weight-resident 64-channel conv kernel (taesd.hip).
// Reference: src/AutoEncoders/taesd.py — Decoder2 :105-135, Block :45-74, Clamp :30-42, TAESD.decode :224-237, taesd_preview :257-313.
// Keys are the nn.Sequential's own indices: 1 (conv 4 -> 64), 3 / 4 / 5, 8 / 9 / 10, 13 / 14 / 15 and 18 (Blocks: <i>.conv.0 / .2 / .4),
// 7 / 12 / 17 (the bias-free convs behind the Upsamples), 19 (conv 64 -> 3).
//
// Every activation is a [B * H * W][64] 16-bit buffer.  The latent's 4 channels are padded to 64 against zero weights by the prep launch, which also applies
// Clamp; a Block is three launches (bias + ReLU, bias + ReLU, bias + skip + ReLU); nearest x2 is folded into the gather of the conv behind it; the output
// conv writes the call's fp32 image and / or 8-bit preview itself.  1 + 1 + 30 + 3 + 1 = 36 launches.
// The skip stream of a level (what conv_in / an upconv starts and three Blocks add to) is kept in fp32 beside its 16-bit copy: the convs multiply the
// 16-bit copy, the skip is added from and stored to the fp32 one, so the stream is not rounded once per Block.  Against the reference's fp32 decoder
// that takes the distance of a bf16 decode from 7.1e-3 to 5.7e-3 in rel-L2 and the preview bytes that are more than one code off to a quarter.
#include "engine.h"

#include <cstdio>

namespace ldx {

int TaesdEngine::validate() const {
    if (cfg.latent_channels != 4) { set_error("unsupported TAESD config: latent_channels must be 4 (taesd_preview cuts or pads every latent to 4 channels, taesd.py:268-277)"); return LDX_EINVAL; }
    return LDX_OK;
}

// [CoutPad][ky][kx][64] <- [Cout][Cin][ky][kx], zero rows / channels above Cout / Cin
bool TaesdEngine::mk_conv64(const std::string& pre, int Cout, int Cin, bool bias, LinearW& out) {
    const HostTensor* w = get(pre + ".weight", {Cout, Cin, 3, 3});
    if (!w) return false;
    const int rows = (Cout + 31) / 32 * 32;
    out.N = Cout; out.K = 9 * 64;
    out.w = pack16(rows, (size_t)9 * 64, {conv_piece(w, Cout, Cin, 64)});
    out.b = nullptr;
    if (bias) {
        const HostTensor* b = get(pre + ".bias", {Cout});
        if (!b) return false;
        out.b = pack32((size_t)(Cout + 3) / 4 * 4, {{b, nullptr, 0, Cout, 0}});
        if (!out.b) return false;
    }
    return out.w != nullptr;
}

int TaesdEngine::finalize() {
    if (finalized) return LDX_OK;
    HIP_OK(hipSetDevice(device));
    static const int block_idx[10] = {3, 4, 5, 8, 9, 10, 13, 14, 15, 18};
    bool ok = mk_conv64("1", 64, cfg.latent_channels, true, ta_first);
    for (int i = 0; ok && i < 10; ++i)
        for (int j = 0; ok && j < 3; ++j) ok = mk_conv64(std::to_string(block_idx[i]) + ".conv." + std::to_string(2 * j), 64, 64, true, ta_blocks[i].c[j]);
    for (int u = 0; ok && u < 3; ++u) ok = mk_conv64(std::to_string(7 + 5 * u), 64, 64, false, ta_up[u]);
    ok = ok && mk_conv64("19", 3, 64, true, ta_last);
    if (!ok) return weights_failed();
    host.clear();
    finalized = true;
    return LDX_OK;
}

int TaesdEngine::plan(int B, int h, int w) {
    return build_plan(PlanKey{B, h, w}, [&]() -> int {
        struct F32 { bool valid = false; size_t off = 0; };          // an fp32 [M][64] buffer of the arena: the skip stream
        auto f32_new = [&](long M) { F32 f; f.valid = true; f.off = a_alloc((size_t)M * 64 * 4); return f; };
        auto f32_ptr = [&](const F32& f) { return f.valid ? (float*)((uintptr_t)cur.arena + f.off) : nullptr; };
        auto f32_free = [&](F32& f) { if (f.valid) a_free(f.off); f.valid = false; };
        auto conv = [&](const char* name, Act X, const LinearW& wt, int Hin, int Win, int up, Act Y, F32 Rf, F32 Yf, int relu) {
            Op& o = emit(OP_TAESD_CONV, name);
            TaesdConvArgs& a = o.tconv;
            a.X = ptr(X); a.W = wt.w; a.bias = wt.b; a.Rf = f32_ptr(Rf); a.Yf = f32_ptr(Yf); a.Y = Y.valid ? ptr(Y) : nullptr;
            a.B = B; a.Hin = Hin; a.Win = Win; a.up = up; a.relu = relu; a.out3 = Y.valid ? 0 : 1;
            const double M = (double)B * (Hin << up) * (Win << up);
            o.flops = 2.0 * M * wt.N * wt.K;
            o.bytes = 2.0 * ((double)B * Hin * Win * 64 + (double)wt.N * wt.K + (Y.valid ? M * 64 : 0.0)) + (Y.valid ? 0.0 : M * 3 * 5) + 4.0 * M * 64 * ((Rf.valid ? 1 : 0) + (Yf.valid ? 1 : 0));
            snprintf(o.klabel, sizeof(o.klabel), "taesd_conv_kernel<%s,%d>", dt_name(), Y.valid ? 2 : 1);
            cur.flops += o.flops;
        };
        int H = h, W = w;
        Act x = new_act(B * H * W, 64);
        emit(OP_TAESD_PREP, "taesd.prep").tprep = TaesdPrepArgs{nullptr, ptr(x), B, cfg.latent_channels, (long)H * W};      // the latent is the call's
        Act cur_a = new_act(B * H * W, 64);          // the stream's 16-bit copy ...
        F32 cur_f = f32_new((long)B * H * W);        // ... and the stream
        conv("taesd.conv_in", x, ta_first, H, W, 0, cur_a, F32{}, cur_f, 1);
        release(x);
        int bi = 0;
        auto block = [&](const TaesdBlockW& bw, bool stream_goes_on) {
            const int M = B * H * W;
            Act t1 = new_act(M, 64), t2 = new_act(M, 64);
            F32 nf = stream_goes_on ? f32_new(M) : F32{};          // the level's last Block feeds an upconv or conv_out: they read the 16-bit copy alone
            conv("taesd.block.conv0", cur_a, bw.c[0], H, W, 0, t1, F32{}, F32{}, 1);
            conv("taesd.block.conv2", t1, bw.c[1], H, W, 0, t2, F32{}, F32{}, 1);
            conv("taesd.block.conv4", t2, bw.c[2], H, W, 0, t1, cur_f, nf, 1);          // + skip, then the Block's fuse ReLU
            release(t2); release(cur_a); f32_free(cur_f);
            cur_a = t1; cur_f = nf;
        };
        for (int level = 0; level < 4; ++level) {
            const int nb = level < 3 ? 3 : 1;
            if (level) {
                Act nx = new_act(B * 4 * H * W, 64);
                cur_f = f32_new((long)B * 4 * H * W);
                conv("taesd.upconv", cur_a, ta_up[level - 1], H, W, 1, nx, F32{}, cur_f, 0);
                release(cur_a); cur_a = nx; H *= 2; W *= 2;
            }
            for (int k = 0; k < nb; ++k) block(ta_blocks[bi++], k + 1 < nb);
        }
        conv("taesd.conv_out", cur_a, ta_last, H, W, 0, Act{}, F32{}, F32{}, 0);
        release(cur_a);
        return LDX_OK;
    });
}

int TaesdEngine::run(const float* z, int B, int h, int w, float* out_f32, uint8_t* out_u8, int flux, hipStream_t st) {
    if (!finalized) { set_error("ldx_taesd_decode: not a finalized TAESD engine"); return LDX_ESTATE; }
    if (!z || (!out_f32 && !out_u8) || B <= 0 || h <= 0 || w <= 0 || (long)B * h * w * 64 >= (1L << 31)) {
        set_error("ldx_taesd_decode: bad argument (null latent, no output, or 64 * B * h * w >= 2^31)"); return LDX_EINVAL; }
    HIP_OK(hipSetDevice(device));
    // the call's three pointers and the flux flag are what a captured graph has baked in (Engine::run_bound): a caller that wants replays keeps its
    // latent and output buffers (TAESDEngine does in graph mode)
    Bindings b; b.x = z; b.out = out_f32; b.out8 = out_u8; b.flux = flux ? 1 : 0;
    return run_planned(PlanKey{B, h, w}, [&] { return plan(B, h, w); }, b, st);
}

}  // namespace ldx
