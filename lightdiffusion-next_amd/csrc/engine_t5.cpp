// T5 encoder stack (T5-XXL for Flux conditioning) as a static launch plan over the shared GEMM / attention / norm
// kernels.  Reference: src/clip/FluxClip.py — T5 :476-519, T5Stack :386-474, T5Block :325-384, T5LayerSelfAttention
// :268-323, T5Attention :72-266, T5LayerFF / T5DenseGatedActDense :15-70, T5LayerNorm :565-582.
//
// Per block:  x += o( attn( q(n), k(n), v(n) ; + relative-position bias ) ),  n = rms_norm(x)
//             x += wo( gelu_tanh(wi_0(m)) * wi_1(m) ),                          m = rms_norm(x)
// q|k|v are one fused GEMM; wi_0|wi_1 are one GEMM whose rows are slab-interleaved so that the gated activation is
// the GEMM epilogue (value = wi_1, gate = wi_0).  Attention is unscaled: the reference multiplies k by sqrt(d) to cancel
// SDPA's 1/sqrt(d) (:265-268).  The bias table comes from the host per call (same for every block, :316-321 / :453-456).
#include "engine.h"

namespace ldx {

int T5Engine::finalize() {
    if (finalized) return LDX_OK;
    const ldx_t5_config& c = cfg;
    auto bad = [&](const char* m) { set_error(std::string("unsupported T5 config: ") + m); return LDX_EINVAL; };
    if (c.d_model <= 0 || c.d_model % 64 || c.d_ff % 64 || c.d_model > 4096) return bad("d_model / d_ff must be multiples of 64, d_model <= 4096");
    if (c.num_heads <= 0 || c.d_model % c.num_heads || (c.d_model / c.num_heads) % 8 || c.d_model / c.num_heads > 160) return bad("head dim");
    if (c.num_layers <= 0 || c.vocab_size <= 0) return bad("num_layers / vocab_size");
    HIP_OK(hipSetDevice(device));
    const int E = c.d_model, F = c.d_ff;
    bool ok = true;
    const HostTensor* tok = get("shared.weight", {c.vocab_size, E});
    ok = tok != nullptr;
    if (ok) { t5_tok = pack32((size_t)c.vocab_size * E, {{tok, nullptr, 0, c.vocab_size * E, 0}}); ok = t5_tok != nullptr; }
    auto rms = [&](const std::string& name, NormW& n) {
        const HostTensor* w = get(name + ".weight", {E});
        if (!w) return false;
        n.C = E; n.b = nullptr;
        n.g = pack32(E, {{w, nullptr, 0, E, 0}});
        return n.g != nullptr;
    };
    t5_layers.resize(c.num_layers);
    for (int l = 0; ok && l < c.num_layers; ++l) {
        T5LayerW& L = t5_layers[l];
        const std::string a = "encoder.block." + std::to_string(l) + ".layer.0", f = "encoder.block." + std::to_string(l) + ".layer.1";
        ok = rms(a + ".layer_norm", L.ln1) && rms(f + ".layer_norm", L.ln2);
        const HostTensor *qw = get(a + ".SelfAttention.q.weight", {E, E}), *kw = get(a + ".SelfAttention.k.weight", {E, E}),
                         *vw = get(a + ".SelfAttention.v.weight", {E, E});
        ok = ok && qw && kw && vw;
        if (ok) {
            L.qkv.N = 3 * E; L.qkv.K = E; L.qkv.b = nullptr;
            L.qkv.w = pack16((size_t)3 * E, E, {rows_piece(qw, 0, E, E), rows_piece(kw, E, E, E), rows_piece(vw, (size_t)2 * E, E, E)});
            ok = L.qkv.w != nullptr;
        }
        ok = ok && mk_linear(a + ".SelfAttention.o", E, E, false, L.o);
        const HostTensor *w0 = get(f + ".DenseReluDense.wi_0.weight", {F, E}), *w1 = get(f + ".DenseReluDense.wi_1.weight", {F, E});
        ok = ok && w0 && w1;
        if (ok) {
            // 64-row slabs: 32 value rows (wi_1) then their 32 gate rows (wi_0, through tanh-GELU).  As pieces: the packed matrix read as [F / 32][64 E], a slab
            // per row, whose left half is 32 consecutive rows of wi_1 and whose right half the same rows of wi_0
            L.wi.N = 2 * F; L.wi.K = E; L.wi.b = nullptr;
            L.wi.w = pack16((size_t)F / 32, (size_t)64 * E, {Piece{w1, 0, 0, F / 32, 32 * E, 1.0f, 0, 0, 0}, Piece{w0, 0, (size_t)32 * E, F / 32, 32 * E, 1.0f, 0, 0, 0}});
            ok = L.wi.w != nullptr;
        }
        ok = ok && mk_linear(f + ".DenseReluDense.wo", E, F, false, L.wo);
    }
    ok = ok && rms("encoder.final_layer_norm", t5_final_ln);
    // device-resident sources (ldx_load_tensor_dev, ldx_load_tensor_q8_0) were packed by launches on the null stream: they and the staged copies are read until it drains
    const hipError_t sync = hipDeviceSynchronize();
    drop_staged();
    if (!ok) return weights_failed();
    if (sync != hipSuccess) { set_error(std::string("weight packing failed: ") + hipGetErrorString(sync)); return LDX_EHIP; }
    host.clear();
    finalized = true;
    return LDX_OK;
}

int T5Engine::plan(int B, int L) {
    const ldx_t5_config& c = cfg;
    const int E = c.d_model, F = c.d_ff, M = B * L, heads = c.num_heads, D = E / heads;
    const int Lp = ((L + 63) / 64) * 64;
    return build_plan(PlanKey{B, L}, [&]() -> int {
        Act x = new_act(M, E);
        emit(OP_EMBED, "t5.embed").emb = ClipEmbedArgs{nullptr, t5_tok, nullptr, ptr(x), B, L, E, c.vocab_size, nullptr, 0};      // the ids are the call's
        Act n = new_act(M, E), qkv = new_act(M, 3 * E), a = new_act(M, E), f = new_act(M, F);
        auto rms = [&](const char* name, Act X, Act Y, const NormW& w) { op_ln(name, X, Y, w, [](LayerNormArgs& l) { l.eps = 1e-6f; l.rms = 1; }); };
        for (int l = 0; l < c.num_layers; ++l) {
            const T5LayerW& W = t5_layers[l];
            rms("t5.ln1", x, n, W.ln1);
            op_gemm("t5.qkv", n, W.qkv, qkv, Act{});
            const char* base = (const char*)ptr(qkv);
            op_attn("t5.attn", base, 3 * E, base + (size_t)E * 2, 3 * E, base + (size_t)2 * E * 2, 3 * E, a, B, heads, L, L, D,
                    [&](Op& o) { o.at.scale = 1.0f; o.at.bias_ld = Lp; o.at.bias_hs = (long)L * Lp; o.bias_from_call = true; });      // the relative-position table is the call's
            op_gemm("t5.o", a, W.o, x, x);                        // x += attention output
            rms("t5.ln2", x, n, W.ln2);
            op_gemm("t5.wi", n, W.wi, f, Act{}, 2);               // gelu_tanh(wi_0 n) * (wi_1 n)
            op_gemm("t5.wo", f, W.wo, x, x);                      // x += FF output
        }
        rms("t5.final_ln", x, n, t5_final_ln);
        emit(OP_CVT_OUT, "t5.out").out = CvtOutArgs{ptr(n), nullptr, (size_t)(M * E)};
        return LDX_OK;
    });
}

int T5Engine::run(const int* ids, int B, int L, const float* bias, float* out, hipStream_t st) {
    if (!finalized) { set_error("ldx_t5_encode: not a finalized T5 engine"); return LDX_ESTATE; }
    if (!ids || !bias || !out || B <= 0 || L <= 0) { set_error("ldx_t5_encode: bad argument"); return LDX_EINVAL; }
    HIP_OK(hipSetDevice(device));
    Bindings b; b.ids = ids; b.bias = bias; b.out = out;
    return run_planned(PlanKey{B, L}, [&] { return plan(B, L); }, b, st);
}

}  // namespace ldx
