// CLIP text encoder on the same planner / kernels as the UNet (engine.cpp).
//
//   CLIPTextModel_.forward     src/clip/CLIPTextModel.py:51-107
//   CLIPLayer / CLIPAttention / CLIPMLP / CLIPEmbeddings   src/clip/Clip.py:14-294
#include <algorithm>
#include <cmath>
#include <cstring>

#include "engine.h"

namespace ldx {

int ClipEngine::finalize() {
    if (finalized) return LDX_OK;
    const ldx_clip_config& c = cfg;
    auto bad = [&](const char* m) { set_error(std::string("unsupported CLIP config: ") + m); return LDX_EINVAL; };
    if (c.hidden_size % 64 || c.intermediate_size % 64) return bad("hidden/intermediate size must be multiples of 64");
    if (c.hidden_size % c.num_heads || (c.hidden_size / c.num_heads) % 8 || c.hidden_size / c.num_heads > 160) return bad("head dim");
    HIP_OK(hipSetDevice(device));
    const int E = c.hidden_size;
    bool ok = true;
    const HostTensor* tok = get("embeddings.token_embedding.weight", {c.vocab_size, E});
    const HostTensor* pos = get("embeddings.position_embedding.weight", {c.max_positions, E});
    ok = tok && pos;
    if (ok) {
        clip_tok = pack32((size_t)c.vocab_size * E, {{tok, nullptr, 0, c.vocab_size * E, 0}});
        clip_pos = pack32((size_t)c.max_positions * E, {{pos, nullptr, 0, c.max_positions * E, 0}});
        ok = clip_tok && clip_pos;
    }
    clip_layers.resize(c.num_layers);
    for (int l = 0; ok && l < c.num_layers; ++l) {
        ClipLayerW& L = clip_layers[l];
        const std::string p = "encoder.layers." + std::to_string(l);
        ok = mk_norm(p + ".layer_norm1", E, L.ln1) && mk_norm(p + ".layer_norm2", E, L.ln2);
        const HostTensor *qw = get(p + ".self_attn.q_proj.weight", {E, E}), *kw = get(p + ".self_attn.k_proj.weight", {E, E}),
                         *vw = get(p + ".self_attn.v_proj.weight", {E, E}), *qb = get(p + ".self_attn.q_proj.bias", {E}),
                         *kb = get(p + ".self_attn.k_proj.bias", {E}), *vb = get(p + ".self_attn.v_proj.bias", {E});
        ok = ok && qw && kw && vw && qb && kb && vb;
        if (ok) {
            L.qkv.N = 3 * E; L.qkv.K = E;
            L.qkv.w = pack16((size_t)3 * E, E, {rows_piece(qw, 0, E, E), rows_piece(kw, E, E, E), rows_piece(vw, (size_t)2 * E, E, E)});
            L.qkv.b = pack32((size_t)3 * E, {{qb, nullptr, 0, E, 0}, {kb, nullptr, (size_t)E, E, 0}, {vb, nullptr, (size_t)2 * E, E, 0}});
            ok = L.qkv.w && L.qkv.b;
        }
        ok = ok && mk_linear(p + ".self_attn.out_proj", E, E, true, L.out) && mk_linear(p + ".mlp.fc1", c.intermediate_size, E, true, L.fc1) &&
             mk_linear(p + ".mlp.fc2", E, c.intermediate_size, true, L.fc2);
    }
    ok = ok && mk_norm("final_layer_norm", E, clip_final_ln);
    if (ok && host.count("text_projection.weight")) {          // optional: the pooled output's projection (bias-free Linear)
        const HostTensor* tp = get("text_projection.weight", {E, E});
        ok = tp != nullptr;
        if (ok) { clip_proj = pack32((size_t)E * E, {{tp, nullptr, 0, E * E, 0}}); ok = clip_proj != nullptr; }
    }
    if (!ok) return weights_failed();
    host.clear();
    finalized = true;
    return LDX_OK;
}

int ClipEngine::plan(int B, int T, int inter) {
    const ldx_clip_config& c = cfg;
    const int E = c.hidden_size, M = B * T, heads = c.num_heads, D = E / heads;
    return build_plan(PlanKey{B, T, 0, inter}, [&]() -> int {
        Act x = new_act(M, E);
        emit(OP_EMBED, "clip.embed").emb = ClipEmbedArgs{nullptr, clip_tok, clip_pos, ptr(x), B, T, E, c.vocab_size, nullptr, 0};      // ids and the textual-inversion rows are the call's
        Act n = new_act(M, E), qkv = new_act(M, 3 * E), a = new_act(M, E), f = new_act(M, c.intermediate_size);
        Act xi = new_act(M, E);
        for (int l = 0; l < c.num_layers; ++l) {
            const ClipLayerW& L = clip_layers[l];
            op_ln("clip.ln1", x, n, L.ln1);
            op_gemm("clip.qkv", n, L.qkv, qkv, Act{});
            const char* base = (const char*)ptr(qkv);
            op_attn("clip.attn", base, 3 * E, base + (size_t)E * 2, 3 * E, base + (size_t)2 * E * 2, 3 * E, a, B, heads, T, T, D, [](AttnArgs& at) { at.causal = 1; });
            op_gemm("clip.out", a, L.out, x, x);                 // x += self_attn(ln1(x))
            op_ln("clip.ln2", x, n, L.ln2);
            op_gemm("clip.fc1", n, L.fc1, f, Act{}, 0, [](GemmArgs& g) { g.act = 1; });      // quick-GELU
            op_gemm("clip.fc2", f, L.fc2, x, x);                 // x += mlp(ln2(x))
            if (l == inter) {                                    // intermediate = x.clone(); final LN applied to it
                op_ln("clip.final_ln.inter", x, xi, clip_final_ln);
                { Op& o = emit(OP_CVT_OUT, "clip.out_inter"); o.out = CvtOutArgs{ptr(xi), nullptr, (size_t)(M * E)}; o.second_output = true; }
            }
        }
        op_ln("clip.final_ln", x, n, clip_final_ln);
        emit(OP_CVT_OUT, "clip.out_last").out = CvtOutArgs{ptr(n), nullptr, (size_t)(M * E)};
        return LDX_OK;
    });
}

// Textual-inversion vectors for the next ldx_clip_encode calls: the reference extends the token table by one row per vector
// and gives those rows the ids vocab_size, vocab_size + 1, ... (SDClipModel.set_up_textual_embeddings, SD15/SDClip.py:213-267).
// Host rows [n][hidden] fp32; n = 0 removes them.  Synchronous (cudaMemcpy); the buffer grows, never shrinks.
int ClipEngine::set_clip_extra(const float* rows_host, int n) {
    if (!finalized) { set_error("ldx_clip_set_extra_embeddings: not a finalized CLIP engine"); return LDX_ESTATE; }
    if (n < 0 || (n > 0 && !rows_host)) { set_error("ldx_clip_set_extra_embeddings: bad argument"); return LDX_EINVAL; }
    HIP_OK(hipSetDevice(device));
    HIP_OK(hipDeviceSynchronize());                    // a previous encode may still read the old rows
    const size_t E = (size_t)cfg.hidden_size;
    if (n > clip_extra_cap) {
        float* p = nullptr;
        HIP_OK(hipMalloc((void**)&p, (size_t)n * E * sizeof(float)));
        dev_allocs.push_back(p);                       // the old (smaller) buffer stays owned by the engine until it is destroyed
        clip_extra = p; clip_extra_cap = n;
    }
    if (n > 0) HIP_OK(hipMemcpy(clip_extra, rows_host, (size_t)n * E * sizeof(float), hipMemcpyHostToDevice));
    clip_extra_n = n;
    return LDX_OK;
}

int ClipEngine::clip_pooled(const float* last, const int* ids, int B, int T, int eos_id, float* out, hipStream_t st) {
    if (!finalized) { set_error("ldx_clip_pooled: not a finalized CLIP engine"); return LDX_ESTATE; }
    if (!last || !ids || !out || B <= 0 || T <= 0) { set_error("ldx_clip_pooled: bad argument"); return LDX_EINVAL; }
    HIP_OK(hipSetDevice(device));
    launch_clip_pooled(last, ids, B, T, cfg.hidden_size, eos_id, clip_proj, out, st);
    return launch_status();
}

int ClipEngine::run(const int* ids, int B, int T, int inter_layer, float* out_last, float* out_inter, hipStream_t st) {
    if (!finalized) { set_error("ldx_clip_encode: not a finalized CLIP engine"); return LDX_ESTATE; }
    if (!ids || !out_last || B <= 0 || T <= 0 || T > cfg.max_positions) { set_error("ldx_clip_encode: bad argument"); return LDX_EINVAL; }
    HIP_OK(hipSetDevice(device));
    int inter = -1;
    if (out_inter) {
        inter = inter_layer < 0 ? cfg.num_layers + inter_layer : inter_layer;
        if (inter < 0 || inter >= cfg.num_layers) { set_error("ldx_clip_encode: inter_layer out of range"); return LDX_EINVAL; }
    }
    Bindings b; b.ids = ids; b.out = out_last; b.out2 = out_inter; b.extra = clip_extra; b.n_extra = clip_extra_n;      // the textual-inversion rows change between calls
    return run_planned(PlanKey{B, T, 0, inter}, [&] { return plan(B, T, inter); }, b, st);
}

}  // namespace ldx
