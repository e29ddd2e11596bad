// VAE decoder and encoder on the same planner / kernels as the UNet (engine.cpp).
//
//   Decoder.forward            src/AutoEncoders/VariationalAE.py:532-567
//   ResnetBlock.forward        src/AutoEncoders/ResBlock.py:383-406      (GroupNorm eps 1e-6, swish)
//   AttnBlock.forward          src/Attention/Attention.py:159-178        (1 head, D = C = 512)
//   Upsample.forward           src/AutoEncoders/VariationalAE.py:209-221 (nearest 2x + conv3x3)
//   AutoencodingEngine.decode  :130-145 (post_quant_conv) ; VAE.decode :690-722 (clamp, NHWC)
#include <algorithm>
#include <cmath>
#include <cstring>

#include "engine.h"

namespace ldx {

bool VaeEngine::mk_vae_res(const std::string& pre, int Cin, int Cout, ResW& r) {
    r.Cin = Cin; r.Cout = Cout; r.eps = 1e-6f; r.has_emb = false;
    if (!mk_norm(pre + ".norm1", Cin, r.gn1) || !mk_conv3(pre + ".conv1", Cout, Cin, Cin, r.conv1)) return false;
    if (!mk_norm(pre + ".norm2", Cout, r.gn2)) return false;
    r.has_skip = Cin != Cout;
    // x = nin_shortcut(x); return x + h (ResBlock.py:383-406): folded into conv2 as a second K segment, like the UNet's ResBlock1
    if (r.has_skip && Cin % 64 == 0 && g_plan_sw.fused_skip) return mk_fused_skip(pre + ".conv2", pre + ".nin_shortcut", Cin, Cout, r);
    if (!mk_conv3(pre + ".conv2", Cout, Cout, Cout, r.conv2)) return false;
    if (r.has_skip && !mk_linear(pre + ".nin_shortcut", Cout, Cin, true, r.skip, true)) return false;
    return true;
}

bool VaeEngine::mk_vae_attn(const std::string& pre, int C, VaeAttnW& a) {
    if (!mk_norm(pre + ".norm", C, a.norm) || !mk_linear(pre + ".q", C, C, true, a.q, true) || !mk_linear(pre + ".k", C, C, true, a.k, true)) return false;
    // v is used as the A operand (V^T = Wv . h^T); its bias is folded through the softmax (rows sum to 1)
    // into the output projection's bias: b' = Wp . bv + bp.
    if (!mk_linear(pre + ".v", C, C, false, a.v, true)) return false;
    const HostTensor* wp = get(pre + ".proj_out.weight", {C, C, 1, 1});
    const HostTensor* bp = get(pre + ".proj_out.bias", {C});
    const HostTensor* bv = get(pre + ".v.bias", {C});
    if (!wp || !bp || !bv) return false;
    a.proj.N = C; a.proj.K = C;
    a.proj.w = pack16(C, C, {rows_piece(wp, 0, C, C)});
    a.proj.b = upload32(C, [&](size_t i) {
        double acc = bp->at(i);
        for (int k = 0; k < C; ++k) acc += (double)wp->at(i * C + k) * (double)bv->at(k);
        return (float)acc;
    });
    if (!a.proj.w || !a.proj.b) return false;
    if (C == 512) {       // the flash kernel's operands: one [3C][C] projection, q | k | v rows as attention.hip's fused q|k|v (V row-major: no V^T GEMM)
        const HostTensor *wq = get(pre + ".q.weight", {C, C, 1, 1}), *wk = get(pre + ".k.weight", {C, C, 1, 1}), *wv = get(pre + ".v.weight", {C, C, 1, 1});
        const HostTensor *bq = get(pre + ".q.bias", {C}), *bk = get(pre + ".k.bias", {C});
        if (!wq || !wk || !wv || !bq || !bk) return false;
        a.qkv.N = 3 * C; a.qkv.K = C;
        a.qkv.w = pack16((size_t)3 * C, C, {rows_piece(wq, 0, C, C), rows_piece(wk, C, C, C), rows_piece(wv, (size_t)2 * C, C, C)});
        a.qkv.b = upload32((size_t)3 * C, [&](size_t i) { return i < (size_t)C ? bq->at(i) : (i < (size_t)2 * C ? bk->at(i - C) : 0.f); });
        if (!a.qkv.w || !a.qkv.b) return false;
    }
    return true;
}

int VaeEngine::finalize() {
    if (finalized) return LDX_OK;
    const ldx_vae_config& v = cfg;
    auto bad = [&](const char* m) { set_error(std::string("unsupported VAE config: ") + m); return LDX_EINVAL; };
    if (v.ch <= 0 || v.ch % 64) return bad("ch must be a multiple of 64");
    if (v.num_levels < 1 || v.num_levels > 8 || v.z_channels < 1 || v.z_channels > 16 || v.out_ch < 1 || v.out_ch > 4) return bad("levels/channels");
    HIP_OK(hipSetDevice(device));
    bool ok = true;
    int block_in = v.ch * v.ch_mult[v.num_levels - 1];
    ok = ok && mk_conv3("decoder.conv_in", block_in, v.z_channels, 64, vae_conv_in);
    ok = ok && mk_vae_res("decoder.mid.block_1", block_in, block_in, vae_mid1);
    ok = ok && mk_vae_attn("decoder.mid.attn_1", block_in, vae_attn);
    ok = ok && mk_vae_res("decoder.mid.block_2", block_in, block_in, vae_mid2);
    vae_up.assign(v.num_levels, {}); vae_upconv.assign(v.num_levels, LinearW{}); vae_has_up.assign(v.num_levels, false);
    for (int lv = v.num_levels - 1; ok && lv >= 0; --lv) {
        const int block_out = v.ch * v.ch_mult[lv];
        for (int i = 0; ok && i <= v.num_res_blocks; ++i) {
            ResW r;
            ok = mk_vae_res("decoder.up." + std::to_string(lv) + ".block." + std::to_string(i), block_in, block_out, r);
            vae_up[lv].push_back(r);
            block_in = block_out;
        }
        if (ok && lv != 0) {
            vae_has_up[lv] = true;
            ok = mk_conv3("decoder.up." + std::to_string(lv) + ".upsample.conv", block_in, block_in, block_in, vae_upconv[lv]);
        }
    }
    ok = ok && mk_norm("decoder.norm_out", block_in, vae_norm_out) && mk_conv3("decoder.conv_out", v.out_ch, block_in, block_in, vae_conv_out);
    if (ok && v.use_post_quant) {
        const HostTensor* w = get("post_quant_conv.weight", {v.z_channels, v.z_channels, 1, 1});
        const HostTensor* b = get("post_quant_conv.bias", {v.z_channels});
        ok = w && b;
        if (ok) {
            const int zc = v.z_channels;
            vae_pq = pack32((size_t)zc * zc + zc, {{w, nullptr, 0, zc * zc, 0}, {b, nullptr, (size_t)zc * zc, zc, 0}});
            ok = vae_pq != nullptr;
        }
    }
    // ---- optional encoder (Encoder.__init__, VariationalAE.py:257-377) ----
    if (ok && host.count("encoder.conv_in.weight")) {
        vae_has_enc = true;
        const int in_px = 3;
        ok = mk_conv3("encoder.conv_in", v.ch, in_px, 64, enc_conv_in);
        enc_down.assign(v.num_levels, {}); enc_downconv.assign(v.num_levels, LinearW{});
        int bin = v.ch;
        for (int lv = 0; ok && lv < v.num_levels; ++lv) {
            const int bout = v.ch * v.ch_mult[lv];
            for (int i = 0; ok && i < v.num_res_blocks; ++i) {
                ResW r;
                ok = mk_vae_res("encoder.down." + std::to_string(lv) + ".block." + std::to_string(i), bin, bout, r);
                enc_down[lv].push_back(r);
                bin = bout;
            }
            if (ok && lv != v.num_levels - 1) ok = mk_conv3("encoder.down." + std::to_string(lv) + ".downsample.conv", bin, bin, bin, enc_downconv[lv]);
        }
        ok = ok && mk_vae_res("encoder.mid.block_1", bin, bin, enc_mid1) && mk_vae_attn("encoder.mid.attn_1", bin, enc_attn) &&
             mk_vae_res("encoder.mid.block_2", bin, bin, enc_mid2) && mk_norm("encoder.norm_out", bin, enc_norm_out) &&
             mk_conv3("encoder.conv_out", 2 * v.z_channels, bin, bin, enc_conv_out);
        if (ok && v.use_post_quant) {
            const int zc2 = 2 * v.z_channels;
            const HostTensor* w = get("quant_conv.weight", {zc2, zc2, 1, 1});
            const HostTensor* b = get("quant_conv.bias", {zc2});
            ok = w && b;
            if (ok) { enc_qc = pack32((size_t)zc2 * zc2 + zc2, {{w, nullptr, 0, zc2 * zc2, 0}, {b, nullptr, (size_t)zc2 * zc2, zc2, 0}}); ok = enc_qc != nullptr; }
        }
    }
    if (!ok) return weights_failed();
    host.clear();
    finalized = true;
    return LDX_OK;
}

// AttnBlock: x + proj(softmax(q k^T / sqrt(C)) v), one head of width C, as three GEMMs + a row softmax
void VaeEngine::emit_vae_attn(const VaeAttnW& a, Act X, Act OUT, int B, int H, int W) {
    const int N = H * W, M = B * N, C = a.q.N;
    Act hn = new_act(M, C);
    op_gn("vae.attn.norm", X, hn, B, N, a.norm, 1e-6f, false);
    {
        // C = 512 (every SD VAE): flash attention, one head of D = 512 (attn512.hip) — q | k | v in one projection, the scores stay in the CUs.
        // Before round 5 (and still for other widths / LDX_ATTN512=0): q k^T GEMM -> row softmax -> p v GEMM through HBM, below.
        AttnArgs probe{}; probe.D = C; probe.B = B; probe.H = 1; probe.Nq = N; probe.Mk = N; probe.ldq = probe.ldk = probe.ldv = 3 * C; probe.ldo = C;
        if (a.qkv.w && attn_pick(probe).family == AF_ATTN512) {
            Act qkv = new_act(M, 3 * C);
            op_gemm("vae.attn.qkv", hn, a.qkv, qkv, Act{});
            release(hn);
            Act o = new_act(M, C);
            const char* base = (const char*)ptr(qkv);
            op_attn("vae.attn.flash", base, 3 * C, base + (size_t)C * 2, 3 * C, base + (size_t)2 * C * 2, 3 * C, o, B, 1, N, N, C);
            release(qkv);
            op_gemm("vae.attn.proj", o, a.proj, OUT, X);
            release(o);
            return;
        }
    }
    Act q = new_act(M, C), k = new_act(M, C);
    op_gemm("vae.attn.q", hn, a.q, q, Act{});
    op_gemm("vae.attn.k", hn, a.k, k, Act{});
    Act o = new_act(M, C);
    for (int b = 0; b < B; ++b) {
        // V^T[C][N] = Wv[C][C] . hn_b[N][C]^T   (weights as the A operand, activations as "W": no Act holds the weights, so the op is built here; unsplit)
        Act vt = new_act(C, N);
        { Op& oo = emit(OP_GEMM, "vae.attn.vT");
          GemmArgs& g = oo.g = gemm_linear_args(a.v.w, C, ptr(rows(hn, b * N, N)), C, N, C);
          g.C = ptr(vt); g.ldc = N; g.splitk = 1;
          oo.flops = 2.0 * C * (double)N * C; snprintf(oo.klabel, sizeof(oo.klabel), "gemm_kernel<%s,0>", dt_name());
          cur.flops += oo.flops; }
        // Query rows in chunks of Rc: S_c[Rc][N] = q_c k_b^T, row softmax, O_c = P_c V.  The score matrix is never materialised as a whole
        // (N x N at 2048^2 is 8 GiB and was the arena's peak; at 4096^2 it would be 128 GiB): one chunk is <= 2 GiB, so a 1024^2 decode still runs
        // the three launches it always ran and a 2048^2 decode 4 x 3 (measured at 2048^2: one chunk 69.3 ms, 512 MiB chunks 71.9, 128 MiB 72.1; the
        // arena peak then sits at the 2048^2 x 128-channel conv level, 6.5 GiB instead of 8.45).  LDX_VAE_ATTN_CHUNK_MIB overrides (0 = one chunk).
        const long chunk_mib = g_plan_sw.vae_attn_chunk_mib;
        int Rc = N;
        if (chunk_mib > 0) {
            long r = (chunk_mib << 20) / ((long)N * 2);
            r = (r / 256) * 256;
            if (r < 256) r = 256;
            if (r < N) Rc = (int)r;
        }
        Act S = new_act(Rc, N);
        for (int r0 = 0; r0 < N; r0 += Rc) {
            const int nr = std::min(Rc, N - r0);
            Act Sc = rows(S, 0, nr);
            { LinearW kw; kw.w = ptr(rows(k, b * N, N)); kw.b = nullptr; kw.N = N; kw.K = C;
              op_gemm("vae.attn.qk", rows(q, b * N + r0, nr), kw, Sc, Act{}); }
            { Op& oo = emit(OP_SOFTMAX, "vae.attn.softmax"); oo.sm = SoftmaxArgs{ptr(Sc), nr, N, N, 1.0f / std::sqrt((float)C)};
              oo.bytes = 2.0 * 2.0 * nr * (double)N; snprintf(oo.klabel, sizeof(oo.klabel), "softmax_rows"); }
            // O_c[nr][C] = P_c[nr][N] . V[N][C]  with W = V^T[C][N]
            { LinearW vw; vw.w = ptr(vt); vw.b = nullptr; vw.N = C; vw.K = N;
              op_gemm("vae.attn.pv", Sc, vw, rows(o, b * N + r0, nr), Act{}); }
        }
        release(S); release(vt);
    }
    release(q); release(k); release(hn);
    op_gemm("vae.attn.proj", o, a.proj, OUT, X);
    release(o);
}

int VaeEngine::plan_decode(int B, int h, int w) {
    const ldx_vae_config& v = cfg;
    return build_plan(PlanKey{B, h, w, 1}, [&]() -> int {
        cur.gn_ws_off = a_alloc(gn_ws_bytes(B, (long)h * w * 64));
        int H = h, W = w;
        Act x0 = new_act(B * H * W, 64);
        emit(OP_VAEPREP, "vae.prep").vprep = VaePrepArgs{nullptr, ptr(x0), B, v.z_channels, H * W, 64, vae_pq, vae_pq ? vae_pq + v.z_channels * v.z_channels : nullptr};      // z is the call's
        int C = v.ch * v.ch_mult[v.num_levels - 1];
        Act hcur = new_act(B * H * W, C);
        op_conv("vae.conv_in", x0, B, H, W, 64, vae_conv_in, 1, H, W, hcur, Act{});
        cur.flops -= 2.0 * B * H * W * (double)C * 9.0 * (64 - v.z_channels);
        release(x0);
        auto res = [&](const ResW& r) { Act o = new_act(B * H * W, r.Cout); emit_res(r, hcur, o, B, H, W); release(hcur); hcur = o; };
        res(vae_mid1);
        { Act o = new_act(B * H * W, C); emit_vae_attn(vae_attn, hcur, o, B, H, W); release(hcur); hcur = o; }
        res(vae_mid2);
        for (int lv = v.num_levels - 1; lv >= 0; --lv) {
            for (auto& r : vae_up[lv]) res(r);
            if (vae_has_up[lv]) {
                const int Cc = vae_up[lv].back().Cout;
                Act o = new_act(B * 2 * H * 2 * W, Cc);
                op_conv("vae.up", hcur, B, H, W, Cc, vae_upconv[lv], 1, 2 * H, 2 * W, o, Act{});
                release(hcur); hcur = o; H *= 2; W *= 2;
            }
        }
        const int Cl = vae_up[0].back().Cout;
        Act t = new_act(B * H * W, Cl);
        op_gn("vae.norm_out", hcur, t, B, H * W, vae_norm_out, 1e-6f, true);
        release(hcur);
        float* pix = arena_ptr<float>((size_t)B * H * W * v.out_ch * 4);
        op_conv("vae.conv_out", t, B, H, W, Cl, vae_conv_out, 1, H, W, Act{}, Act{}, nullptr, 0, pix, v.out_ch);
        release(t);
        emit(OP_CLAMP, "vae.clamp").clamp = ClampArgs{pix, nullptr, (size_t)(B * H * W * v.out_ch)};
        fuse_gn_stats();
        return LDX_OK;
    });
}

int VaeEngine::run_decode(const float* z, int B, int h, int w, float* out, hipStream_t st) {
    if (!finalized) { set_error("ldx_vae_decode: not a finalized VAE engine"); return LDX_ESTATE; }
    if (!z || !out || B <= 0 || h <= 0 || w <= 0) { set_error("ldx_vae_decode: bad argument"); return LDX_EINVAL; }
    if ((h * w) % 8) { set_error("ldx_vae_decode: h*w must be a multiple of 8 (attention row length)"); return LDX_EINVAL; }
    HIP_OK(hipSetDevice(device));
    Bindings b; b.x = z; b.out = out;
    return run_planned(PlanKey{B, h, w, 1}, [&] { return plan_decode(B, h, w); }, b, st);
}

// Encoder.forward (VariationalAE.py:378-413) + quant_conv: pixels -> moments
int VaeEngine::plan_encode(int B, int Hpx, int Wpx) {
    const ldx_vae_config& v = cfg;
    return build_plan(PlanKey{B, Hpx, Wpx, 2}, [&]() -> int {
        cur.gn_ws_off = a_alloc(gn_ws_bytes(B, (long)Hpx * Wpx));
        int H = Hpx, W = Wpx;
        Act x0 = new_act(B * H * W, 64);
        emit(OP_PIXPREP, "vae.enc.prep").pix = PixelsPrepArgs{nullptr, ptr(x0), B, 3, H * W, 64, 2.0f, -1.0f};      // the pixels are the call's
        Act hcur = new_act(B * H * W, v.ch);
        op_conv("vae.enc.conv_in", x0, B, H, W, 64, enc_conv_in, 1, H, W, hcur, Act{});
        cur.flops -= 2.0 * B * H * W * (double)v.ch * 9.0 * (64 - 3);
        release(x0);
        auto res = [&](const ResW& r) { Act o = new_act(B * H * W, r.Cout); emit_res(r, hcur, o, B, H, W); release(hcur); hcur = o; };
        for (int lv = 0; lv < v.num_levels; ++lv) {
            for (auto& r : enc_down[lv]) res(r);
            if (lv != v.num_levels - 1) {
                // Downsample: F.pad(x, (0,1,0,1)) then 3x3 stride-2 conv without padding (VariationalAE.py:224-254)
                const int Cc = enc_down[lv].back().Cout, Ho = H / 2, Wo = W / 2;
                Act o = new_act(B * Ho * Wo, Cc);
                op_conv("vae.enc.down", hcur, B, H, W, Cc, enc_downconv[lv], 2, Ho, Wo, o, Act{}, nullptr, 0, nullptr, 0, [](GemmArgs& g) { g.pad0 = 1; });
                release(hcur); hcur = o; H = Ho; W = Wo;
            }
        }
        res(enc_mid1);
        { Act o = new_act(B * H * W, enc_mid1.Cout); emit_vae_attn(enc_attn, hcur, o, B, H, W); release(hcur); hcur = o; }
        res(enc_mid2);
        const int Cl = enc_mid2.Cout, zc2 = 2 * v.z_channels;
        Act t = new_act(B * H * W, Cl);
        op_gn("vae.enc.norm_out", hcur, t, B, H * W, enc_norm_out, 1e-6f, true);
        release(hcur);
        float* mom = arena_ptr<float>((size_t)B * H * W * zc2 * 4);
        op_conv("vae.enc.conv_out", t, B, H, W, Cl, enc_conv_out, 1, H, W, Act{}, Act{}, nullptr, 0, mom, zc2);
        release(t);
        emit(OP_MOMENTS, "vae.enc.quant_conv").mix = MixArgs{mom, zc2, nullptr, B, zc2, H * W, enc_qc, enc_qc ? enc_qc + zc2 * zc2 : nullptr};
        fuse_gn_stats();
        return LDX_OK;
    });
}

int VaeEngine::run_encode(const float* px, int B, int H, int W, float* moments, hipStream_t st) {
    if (!finalized) { set_error("ldx_vae_encode: not a finalized VAE engine"); return LDX_ESTATE; }
    if (!vae_has_enc) { set_error("ldx_vae_encode: encoder.* weights were not loaded"); return LDX_EMISSING; }
    const int f = 1 << (cfg.num_levels - 1);
    // sizes that are not multiples of f are legal in the reference (vae_encode_crop_pixels is a no-op, VariationalAE.py:
    // 677-688): every Downsample yields floor(H/2)
    if (!px || !moments || B <= 0 || H < f || W < f || ((H / f) * (W / f)) % 8) {
        set_error("ldx_vae_encode: bad argument (H, W >= downscale factor; latent h*w multiple of 8)"); return LDX_EINVAL; }
    HIP_OK(hipSetDevice(device));
    Bindings b; b.x = px; b.out = moments;
    return run_planned(PlanKey{B, H, W, 2}, [&] { return plan_encode(B, H, W); }, b, st);
}

}  // namespace ldx
