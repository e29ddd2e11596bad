// SAM image encoder (segment_anything's ImageEncoderViT, the network behind ADetailer's masks: src/AutoDetailer/SAM.py:157-182 loads ViT-B) as a static launch
// plan: the linears, LayerNorms and the neck's convs on the shared GEMM / norm kernels, the rest on sam.hip.  Keys are segment_anything's own with
// "image_encoder." stripped.
//
//   x = patch_embed(img) + pos_embed                       conv 16 x 16 / 16 as a GEMM over gathered patch rows [B * S * S][768]
//   per block:  x += proj(attn(qkv(LN1(x))))               window blocks: LN1(x) is zero-padded to whole windows and partitioned first, the result cropped back
//               x += lin2(gelu_erf(lin1(LN2(x))))
//   attention:  softmax(0.125 q.k + rel_h[q][k_h] + rel_w[q][k_w]) v, the two rel terms computed from the unscaled q and the [2 n - 1][64] tables
//   neck:       conv 1 x 1, LayerNorm over channels, conv 3 x 3, LayerNorm over channels -> fp32 [B][C][S][S]
// The residual stream x is 16-bit; LayerNorm eps is 1e-6 everywhere.  Padded window tokens are zero rows after the norm, so their k and v are the qkv bias: they
// are attended to like any other key, as the published model does.
#include "engine.h"

#include <cstdio>

namespace ldx {

int SamEngine::validate() const {
    const ldx_sam_config& c = cfg;
    auto bad = [&](const char* m) { set_error(std::string("unsupported SAM config: ") + m); return LDX_EINVAL; };
    if (c.num_heads <= 0 || c.embed_dim <= 0 || c.embed_dim != c.num_heads * 64) return bad("the head dimension embed_dim / num_heads must be 64 (ViT-B, ViT-L; ViT-H has 80)");
    if (c.image_size <= 0 || c.image_size % 16 || c.image_size > 4096) return bad("image_size must be a multiple of the patch size 16, at most 4096");
    if (c.depth <= 0 || c.depth > 32) return bad("depth must be 1 .. 32 (global_attn_mask has 32 bits)");
    if (c.mlp_dim <= 0 || c.mlp_dim % 8) return bad("mlp_dim must be a multiple of 8");
    if (c.out_chans <= 0 || c.out_chans % 64) return bad("out_chans must be a multiple of 64");
    if (c.window_size <= 0) return bad("window_size must be positive");
    return LDX_OK;
}

int SamEngine::finalize() {
    if (finalized) return LDX_OK;
    HIP_OK(hipSetDevice(device));
    const ldx_sam_config& c = cfg;
    const int E = c.embed_dim, S = c.image_size / 16, C = c.out_chans;
    // the official checkpoints carry tables of exactly 2 n - 1 rows; the reference's interpolation of other lengths is not built
    for (int i = 0; i < c.depth; ++i) {
        const int n = (c.global_attn_mask >> i) & 1 ? S : c.window_size;
        for (const char* name : {"rel_pos_h", "rel_pos_w"}) {
            const std::string key = "blocks." + std::to_string(i) + ".attn." + name;
            auto it = host.find(key);
            if (it == host.end()) continue;          // reported as missing below
            const std::vector<int64_t>& sh = it->second.shape;
            if (sh.size() != 2 || sh[0] != 2 * n - 1 || sh[1] != 64) {
                set_error(key + ": a relative-position table must be [2 n - 1][64] with n = " + std::to_string(n) + " (tables of another length are not interpolated)");
                return LDX_EINVAL;
            }
        }
    }
    auto vec32 = [&](const std::string& key, std::initializer_list<int64_t> shape, float*& out) {
        const HostTensor* t = get(key, shape);
        if (!t) return false;
        out = pack32(t->numel, {{t, nullptr, 0, (int)t->numel, 0}});
        return out != nullptr;
    };
    bool ok = true;
    {
        const HostTensor* w = get("patch_embed.proj.weight", {E, 3, 16, 16});
        const HostTensor* b = get("patch_embed.proj.bias", {E});
        ok = w && b;
        if (ok) {
            sam_patch.N = E; sam_patch.K = 768;
            sam_patch.w = pack16(E, 768, {rows_piece(w, 0, E, 768)});
            sam_patch.b = pack32(E, {{b, nullptr, 0, E, 0}});
            ok = sam_patch.w && sam_patch.b;
        }
    }
    ok = ok && vec32("pos_embed", {1, S, S, E}, sam_pos);
    sam_blocks.resize(c.depth);
    for (int i = 0; ok && i < c.depth; ++i) {
        SamBlockW& W = sam_blocks[i];
        const std::string p = "blocks." + std::to_string(i);
        W.global = (c.global_attn_mask >> i) & 1;
        const int n = W.global ? S : c.window_size;
        ok = mk_norm(p + ".norm1", E, W.ln1) && mk_linear(p + ".attn.qkv", 3 * E, E, true, W.qkv) && vec32(p + ".attn.rel_pos_h", {2 * n - 1, 64}, W.rel_h) &&
             vec32(p + ".attn.rel_pos_w", {2 * n - 1, 64}, W.rel_w) && mk_linear(p + ".attn.proj", E, E, true, W.proj) && mk_norm(p + ".norm2", E, W.ln2) &&
             mk_linear(p + ".mlp.lin1", c.mlp_dim, E, true, W.lin1) && mk_linear(p + ".mlp.lin2", E, c.mlp_dim, true, W.lin2);
    }
    ok = ok && mk_linear("neck.0", C, E, false, sam_neck0, true) && mk_norm("neck.1", C, sam_neck1);
    if (ok) {
        const HostTensor* w = get("neck.2.weight", {C, C, 3, 3});
        ok = w != nullptr;
        if (ok) {
            sam_neck2.N = C; sam_neck2.K = 9 * C; sam_neck2.b = nullptr;
            sam_neck2.w = pack16(C, (size_t)9 * C, {conv_piece(w, C, C, C)});
            ok = sam_neck2.w != nullptr;
        }
    }
    ok = ok && mk_norm("neck.3", C, sam_neck3);
    if (!ok) return weights_failed();
    host.clear();
    finalized = true;
    return LDX_OK;
}

int SamEngine::plan(int B) {
    const ldx_sam_config& c = cfg;
    const int E = c.embed_dim, H = c.num_heads, F = c.mlp_dim, C = c.out_chans, S = c.image_size / 16, win = c.window_size;
    const int M = B * S * S, nw = (S + win - 1) / win, Mw = B * nw * nw * win * win;
    return build_plan(PlanKey{B}, [&]() -> int {
        auto ln = [&](const char* name, Act X, Act Y, const NormW& w) { op_ln(name, X, Y, w, [](LayerNormArgs& l) { l.eps = 1e-6f; }); };
        auto rowvec = [&](const char* name, Act X, const float* vec, int period, int act) {
            Op& o = emit(OP_SAM_ROWVEC, name);
            o.srv.X = ptr(X); o.srv.ld = X.ld; o.srv.rows = X.rows; o.srv.C = X.C; o.srv.vec = vec; o.srv.period = period; o.srv.act = act;
            o.bytes = 2.0 * 2.0 * (double)X.rows * X.C;
            snprintf(o.klabel, sizeof(o.klabel), "sam_rowvec_kernel<%s>", dt_name());
        };
        auto window = [&](const char* name, Act src, Act dst, bool scatter) {
            Op& o = emit(OP_SAM_WINDOW, name);
            o.swin.src = ptr(src); o.swin.dst = ptr(dst); o.swin.R = scatter ? ptr(dst) : nullptr; o.swin.B = B; o.swin.S = S; o.swin.win = win; o.swin.C = E; o.swin.scatter = scatter ? 1 : 0;
            o.bytes = 2.0 * (double)E * (scatter ? 3.0 * M : (double)M + Mw);
            snprintf(o.klabel, sizeof(o.klabel), "sam_window_kernel<%s>", dt_name());
        };
        Act patches = new_act(M, 768);
        {
            Op& o = emit(OP_SAM_PATCH, "sam.patch");          // the image is the call's
            o.spatch.out = ptr(patches); o.spatch.B = B; o.spatch.S = S;
            o.bytes = (double)M * 768 * 6;
            snprintf(o.klabel, sizeof(o.klabel), "sam_patch_kernel<%s>", dt_name());
        }
        Act x = new_act(M, E);
        op_gemm("sam.patch_embed", patches, sam_patch, x, Act{});
        release(patches);
        rowvec("sam.pos_embed", x, sam_pos, S * S, 0);
        Act nrm = new_act(M, E), f = new_act(M, F);
        for (int i = 0; i < c.depth; ++i) {
            const SamBlockW& W = sam_blocks[i];
            const int n = W.global ? S : win, N = n * n, BW = W.global ? B : B * nw * nw, rows = BW * N;
            ln("sam.ln1", x, nrm, W.ln1);
            Act src = nrm;
            if (!W.global) { src = new_act(Mw, E); window("sam.window_gather", nrm, src, false); }
            Act qkv = new_act(rows, 3 * E);
            op_gemm("sam.qkv", src, W.qkv, qkv, Act{});
            if (!W.global) release(src);
            const size_t rel_off = a_alloc((size_t)BW * H * N * 2 * n * 4);
            float* const rel = (float*)((uintptr_t)cur.arena + rel_off);
            const char* const q = (const char*)ptr(qkv);
            {
                Op& o = emit(OP_SAM_RELPOS, "sam.relpos");
                o.srel.Q = q; o.srel.ldq = 3 * E; o.srel.th = W.rel_h; o.srel.tw = W.rel_w; o.srel.out = rel; o.srel.BW = BW; o.srel.H = H; o.srel.n = n;
                o.flops = 2.0 * BW * H * (double)N * 2 * n * 64;
                o.bytes = 4.0 * BW * H * (double)N * 2 * n + 2.0 * (double)rows * E;
                snprintf(o.klabel, sizeof(o.klabel), "sam_relpos_kernel<%s>", dt_name());
                cur.flops += o.flops;
            }
            Act att = new_act(rows, E);
            {
                Op& o = emit(OP_SAM_ATTN, W.global ? "sam.attn_global" : "sam.attn_window");
                SamAttnArgs& a = o.sattn;
                a.Q = q; a.K = q + (size_t)E * 2; a.V = q + (size_t)2 * E * 2; a.ld = 3 * E; a.rel = rel; a.O = ptr(att); a.ldo = E; a.BW = BW; a.H = H; a.n = n; a.scale = 0.125f;
                if (!sam_attn_ok(a) && cur.arena) { set_error("SAM plan: attention shape outside the kernel's limits (batch * windows * heads <= 65535)"); plan_rc = LDX_EINVAL; }
                o.flops = 4.0 * BW * H * (double)N * N * 64;
                o.bytes = 2.0 * 4.0 * (double)rows * E + 4.0 * BW * H * (double)N * 2 * n;
                snprintf(o.klabel, sizeof(o.klabel), "sam_attn_kernel<%s>%s", dt_name(), W.global ? "global" : "window");
                cur.flops += o.flops;
            }
            a_free(rel_off);
            release(qkv);
            if (W.global) op_gemm("sam.proj", att, W.proj, x, x);                 // x += attention output
            else {
                Act pj = new_act(rows, E);
                op_gemm("sam.proj", att, W.proj, pj, Act{});
                window("sam.window_scatter", pj, x, true);                        // x += the cropped windows
                release(pj);
            }
            release(att);
            ln("sam.ln2", x, nrm, W.ln2);
            op_gemm("sam.lin1", nrm, W.lin1, f, Act{}, 0, [](GemmArgs& g) { g.bias = nullptr; });      // the bias goes in with the activation
            rowvec("sam.gelu", f, W.lin1.b, 1, 1);
            op_gemm("sam.lin2", f, W.lin2, x, x);                                  // x += MLP output
        }
        release(nrm); release(f);
        Act y0 = new_act(M, C), y1 = new_act(M, C);
        op_gemm("sam.neck0", x, sam_neck0, y0, Act{});
        ln("sam.neck1", y0, y1, sam_neck1);
        op_conv("sam.neck2", y1, B, S, S, C, sam_neck2, 1, S, S, y0, Act{});
        ln("sam.neck3", y0, y1, sam_neck3);
        {
            Op& o = emit(OP_SAM_OUT, "sam.out");          // the output is the call's
            o.sout.X = ptr(y1); o.sout.ld = C; o.sout.B = B; o.sout.C = C; o.sout.HW = S * S;
            o.bytes = 6.0 * (double)M * C;
            snprintf(o.klabel, sizeof(o.klabel), "sam_out_kernel<%s>", dt_name());
        }
        release(y0); release(y1); release(x);
        return LDX_OK;
    });
}

int SamEngine::run(const float* x, int B, float* out, hipStream_t st) {
    if (!finalized) { set_error("ldx_sam_encode: not a finalized SAM engine"); return LDX_ESTATE; }
    // rows of the widest activations: the MLP's on the S x S grid, the window blocks' q | k | v on the grid padded to whole windows
    const long S = cfg.image_size / 16, nw = (S + cfg.window_size - 1) / cfg.window_size, Sp = nw * cfg.window_size;
    if (!x || !out || B <= 0 || (long)B * S * S * cfg.mlp_dim >= (1L << 31) || (long)B * Sp * Sp * 3 * cfg.embed_dim >= (1L << 31) || (long)B * nw * nw * cfg.num_heads > 65535) {
        set_error("ldx_sam_encode: bad argument (null pointer, B <= 0, an activation of 2^31 elements or more, or more than 65535 windows x heads)"); return LDX_EINVAL; }
    HIP_OK(hipSetDevice(device));
    // the two pointers are what a captured graph has baked in (Engine::run_bound): a caller that wants replays keeps its buffers
    Bindings b; b.x = x; b.out = out;
    return run_planned(PlanKey{B}, [&] { return plan(B); }, b, st);
}

}  // namespace ldx
