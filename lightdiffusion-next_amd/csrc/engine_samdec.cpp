// SAM prompt encoder + mask decoder (segment_anything's PromptEncoder and MaskDecoder: what SamPredictor.predict runs per prompt behind the image encoder;
// src/AutoDetailer/SAM.py:10-53 calls it once per detected segment) as a fixed launch sequence over samdec.hip, fp32 throughout.  Keys are segment_anything's own.
//
//   per image (set_image):  rows = embedding^T + no_mask_embed; layer 0's k | v of the tokens' attention and q of the rows' attention (they do not depend on the prompt)
//   per call (predict), P prompts as one batch of P * T token rows and P * g * g image rows:
//     tokens = iou_token | mask_tokens | prompt encodings                     T = 5 + ns <= 15
//     layer i:  tokens  = norm1(self_attn(tokens))                            layer 0 without the positional term and without the residual (skip_first_layer_pe)
//               tokens  = norm2(tokens + attn(tokens + pe_t, rows + pe, rows))
//               tokens  = norm3(tokens + lin2(relu(lin1(tokens))))
//               rows    = norm4(rows + attn(rows + pe, tokens + pe_t, tokens))
//     tokens = norm_final(tokens + attn(tokens + pe_t, rows + pe, rows))
//     hyper = the four 3-layer MLPs on tokens 1 .. 4, iou = the 3-layer head on token 0
//     logits = hyper . gelu(convT2(gelu(LayerNorm2d(convT1(rows)))))           the transposed convolutions are GEMMs over the rows: kernel 2, stride 2
// The cross-attentions' inner width is C / 2, the self-attention's C.  LayerNorm eps 1e-5 in the transformer, 1e-6 in LayerNorm2d.
#include "engine.h"

#include <cmath>

namespace ldx {

SamDecoderEngine::~SamDecoderEngine() {
    for (DecPlan& p : plans) {
        if (p.exec) (void)hipGraphExecDestroy(p.exec);
        if (p.ws) (void)hipFree(p.ws);
    }
}

int SamDecoderEngine::validate() const {
    const ldx_samdec_config& c = cfg;
    auto bad = [&](const char* m) { set_error(std::string("unsupported SAM decoder config: ") + m); return LDX_EINVAL; };
    if (c.hidden <= 0 || c.hidden % 64 || c.hidden > 256) return bad("hidden must be a multiple of 64, at most 256 (a LayerNorm row is held by one workgroup)");
    if (c.num_heads <= 0 || (c.hidden / 2) % c.num_heads) return bad("hidden / 2 must be divisible by num_heads");
    const int hd = c.hidden / 2 / c.num_heads;
    if (hd != 8 && hd != 16 && hd != 32) return bad("the cross-attention head dimension hidden / 2 / num_heads must be 8, 16 or 32");
    if (c.depth != 2 || c.num_multimask != 3) return bad("depth must be 2 and num_multimask 3");
    if (c.mlp_dim <= 0 || c.mlp_dim % 4 || c.iou_head_hidden <= 0 || c.iou_head_hidden % 4) return bad("mlp_dim and iou_head_hidden must be positive multiples of 4");
    if (c.image_size <= 0 || c.image_size % 16 || c.image_size > 4096) return bad("image_size must be a multiple of 16, at most 4096");
    return LDX_OK;
}

// the tensors `keys` (each of `shape`, or any shape when it is empty) one after the other
float* SamDecoderEngine::stack32(const std::vector<std::string>& keys, std::initializer_list<int64_t> shape) {
    std::vector<VecPiece> pieces;
    size_t off = 0;
    for (const std::string& k : keys) {
        const HostTensor* t = get(k, shape);
        if (!t) return nullptr;
        pieces.push_back(VecPiece{t, nullptr, off, (int)t->numel, 0});
        off += t->numel;
    }
    return pack32(off, pieces);
}

bool SamDecoderEngine::mk_attn(const std::string& pre, int inner, SamDecAttnW& w) {
    const int C = cfg.hidden;
    w.wq = stack32({pre + ".q_proj.weight"}, {inner, C});
    w.bq = stack32({pre + ".q_proj.bias"}, {inner});
    w.wkv = stack32({pre + ".k_proj.weight", pre + ".v_proj.weight"}, {inner, C});
    w.bkv = stack32({pre + ".k_proj.bias", pre + ".v_proj.bias"}, {inner});
    w.wo = stack32({pre + ".out_proj.weight"}, {C, inner});
    w.bo = stack32({pre + ".out_proj.bias"}, {C});
    return w.wq && w.bq && w.wkv && w.bkv && w.wo && w.bo;
}

int SamDecoderEngine::finalize() {
    if (finalized) return LDX_OK;
    HIP_OK(hipSetDevice(device));
    const int C = cfg.hidden, C2 = C / 2, C4 = C / 4, C8 = C / 8, F = cfg.mlp_dim, Hh = cfg.iou_head_hidden, g = cfg.image_size / 16, M = g * g;
    const std::string pe = "prompt_encoder.", md = "mask_decoder.", tr = "mask_decoder.transformer.";
    bool ok = true;
    ok = ok && (gauss = stack32({pe + "pe_layer.positional_encoding_gaussian_matrix"}, {2, C2}));
    ok = ok && (point_emb = stack32({pe + "point_embeddings.0.weight", pe + "point_embeddings.1.weight", pe + "point_embeddings.2.weight", pe + "point_embeddings.3.weight"}, {1, C}));
    ok = ok && (not_a_point = stack32({pe + "not_a_point_embed.weight"}, {1, C}));
    ok = ok && (no_mask = stack32({pe + "no_mask_embed.weight"}, {1, C}));
    ok = ok && (iou_token = stack32({md + "iou_token.weight"}, {1, C}));
    ok = ok && (mask_tokens = stack32({md + "mask_tokens.weight"}, {4, C}));
    for (int i = 0; ok && i < 2; ++i) {
        SamDecLayerW& L = layers[i];
        const std::string p = tr + "layers." + std::to_string(i);
        const std::string sa = p + ".self_attn";
        L.wqkv = stack32({sa + ".q_proj.weight", sa + ".k_proj.weight", sa + ".v_proj.weight"}, {C, C});
        L.bqkv = stack32({sa + ".q_proj.bias", sa + ".k_proj.bias", sa + ".v_proj.bias"}, {C});
        L.wo = stack32({sa + ".out_proj.weight"}, {C, C});
        L.bo = stack32({sa + ".out_proj.bias"}, {C});
        L.w1 = stack32({p + ".mlp.lin1.weight"}, {F, C}); L.b1 = stack32({p + ".mlp.lin1.bias"}, {F});
        L.w2 = stack32({p + ".mlp.lin2.weight"}, {C, F}); L.b2 = stack32({p + ".mlp.lin2.bias"}, {C});
        ok = L.wqkv && L.bqkv && L.wo && L.bo && L.w1 && L.b1 && L.w2 && L.b2 && mk_norm(p + ".norm1", C, L.n1) && mk_norm(p + ".norm2", C, L.n2) && mk_norm(p + ".norm3", C, L.n3) &&
             mk_norm(p + ".norm4", C, L.n4) && mk_attn(p + ".cross_attn_token_to_image", C2, L.t2i) && mk_attn(p + ".cross_attn_image_to_token", C2, L.i2t);
    }
    ok = ok && mk_attn(tr + "final_attn_token_to_image", C2, fin) && mk_norm(tr + "norm_final_attn", C, nfin) && mk_norm(md + "output_upscaling.1", C4, up_ln);
    // ConvTranspose2d(kernel 2, stride 2) as a GEMM over the pixels: W'[(dy * 2 + dx) * Cout + co][ci] = w[ci][co][dy][dx], the bias once per (dy, dx)
    auto convT = [&](const std::string& key, int Cin, int Cout, float*& w, float*& b) {
        const HostTensor* wt = get(key + ".weight", {Cin, Cout, 2, 2});
        const HostTensor* bt = get(key + ".bias", {Cout});
        if (!wt || !bt) return false;
        w = upload32((size_t)4 * Cout * Cin, [&](size_t i) { const size_t n = i / Cin, ci = i % Cin, d = n / Cout, co = n % Cout; return wt->at((ci * Cout + co) * 4 + d); });
        b = upload32((size_t)4 * Cout, [&](size_t i) { return bt->at(i % Cout); });
        return w && b;
    };
    ok = ok && convT(md + "output_upscaling.0", C, C4, up1_w, up1_b) && convT(md + "output_upscaling.3", C4, C8, up2_w, up2_b);
    const int hyp_n[3] = {C, C, C8}, iou_n[3] = {Hh, Hh, 4}, iou_k[3] = {C, Hh, Hh};
    for (int l = 0; ok && l < 3; ++l) {
        std::vector<std::string> wk, bk;
        for (int i = 0; i < 4; ++i) {
            const std::string p = md + "output_hypernetworks_mlps." + std::to_string(i) + ".layers." + std::to_string(l);
            wk.push_back(p + ".weight"); bk.push_back(p + ".bias");
        }
        hyp_w[l] = stack32(wk, {hyp_n[l], C}); hyp_b[l] = stack32(bk, {hyp_n[l]});
        const std::string p = md + "iou_prediction_head.layers." + std::to_string(l);
        iou_w[l] = stack32({p + ".weight"}, {iou_n[l], iou_k[l]}); iou_b[l] = stack32({p + ".bias"}, {iou_n[l]});
        ok = hyp_w[l] && hyp_b[l] && iou_w[l] && iou_b[l];
    }
    if (ok) {
        // PromptEncoder.get_dense_pe as rows [g * g][C]: the random-Fourier encoding of the cell centres, evaluated in double
        const HostTensor* gm = get(pe + "pe_layer.positional_encoding_gaussian_matrix", {2, C2});
        dense_pe = upload32((size_t)M * C, [&](size_t i) {
            const size_t m = i / C, c = i % C, f = c < (size_t)C2 ? c : c - C2;
            const double cx = 2.0 * (((double)(m % g) + 0.5) / g) - 1.0, cy = 2.0 * (((double)(m / g) + 0.5) / g) - 1.0;
            const double ang = 2.0 * M_PI * (cx * (double)gm->at(f) + cy * (double)gm->at(C2 + f));
            return (float)(c < (size_t)C2 ? std::sin(ang) : std::cos(ang));
        });
        ok = dense_pe != nullptr;
    }
    if (ok) {
        src0 = (float*)weight_buf((size_t)M * C * 4); k0v0 = (float*)weight_buf((size_t)M * C * 4); q0 = (float*)weight_buf((size_t)M * C2 * 4);
        ok = src0 && k0v0 && q0;
    }
    if (!ok) return weights_failed();
    host.clear();
    finalized = true;
    return LDX_OK;
}

static SamDecGemmArgs gemm_args(const float* X, int ldx, const float* W, const float* bias, float* Y, int ldy, long M, int N, int K, int nb) {
    SamDecGemmArgs a; memset(&a, 0, sizeof(a));
    a.X = X; a.ldx = ldx; a.W = W; a.bias = bias; a.Y = Y; a.ldy = ldy; a.M = M; a.N = N; a.K = K; a.nb = nb; a.nz = 1;
    return a;
}

int SamDecoderEngine::set_image(const float* emb, hipStream_t st) {
    if (!finalized) { set_error("ldx_samdec_set_image: not a finalized SAM decoder engine"); return LDX_ESTATE; }
    if (!emb) { set_error("ldx_samdec_set_image: null embedding"); return LDX_EINVAL; }
    HIP_OK(hipSetDevice(device));
    const int C = cfg.hidden, C2 = C / 2, g = cfg.image_size / 16, M = g * g;
    launch_samdec_transpose(emb, no_mask, src0, C, M, st);
    SamDecGemmArgs kv = gemm_args(src0, C, layers[0].t2i.wkv, layers[0].t2i.bkv, k0v0, C, M, C, C, C2);
    kv.PE = dense_pe; kv.ldpe = C; kv.pe_period = M; kv.pe_cols = C2;
    SamDecGemmArgs q = gemm_args(src0, C, layers[0].i2t.wq, layers[0].i2t.bq, q0, C2, M, C2, C, C2);
    q.PE = dense_pe; q.ldpe = C; q.pe_period = M; q.pe_cols = C2;
    if (!samdec_gemm_ok(kv) || !samdec_gemm_ok(q)) { set_error("ldx_samdec_set_image: internal error (GEMM arguments)"); return LDX_EINVAL; }
    launch_samdec_gemm(kv, st);
    launch_samdec_gemm(q, st);
    have_image = true;
    return launch_status();
}

// The launch sequence of one call.  A plan without a workspace: only the workspace size is computed.
int SamDecoderEngine::run_ops(DecPlan& pl, const Call& c, float* tokens_out, hipStream_t st) {
    const bool dry = pl.ws == nullptr;
    const int C = cfg.hidden, C2 = C / 2, C4 = C / 4, C8 = C / 8, F = cfg.mlp_dim, Hh = cfg.iou_head_hidden, H = cfg.num_heads, g = cfg.image_size / 16, M = g * g;
    const int P = pl.P, n = pl.n, ns = n + (pl.box ? 2 : 1), T = 5 + ns, R = P * T;
    const long PM = (long)P * M;
    const int S = samdec_t2i_ranges(M), chunk = (M + S - 1) / S, hd2 = C2 / H, hds = C / H;
    // workspace
    size_t top = 0;
    auto take = [&](size_t floats) { float* p = pl.ws ? pl.ws + top : nullptr; top += (floats + 63) & ~(size_t)63; return p; };
    float* const tok0 = take((size_t)R * C); float* const qry = take((size_t)R * C); float* const qkv = take((size_t)R * 3 * C); float* const att = take((size_t)R * C);
    float* const tq = take((size_t)R * C2); float* const mlp = take((size_t)R * F); float* const tkv = take((size_t)R * C);
    float* const part = take((size_t)P * H * S * 16 * (hd2 + 2));
    float* const h1 = take((size_t)4 * P * C); float* const h2 = take((size_t)4 * P * C); float* const hyper = take((size_t)P * 4 * C8);
    float* const i1 = take((size_t)P * Hh); float* const i2 = take((size_t)P * Hh);
    float* const keys = take((size_t)PM * C); float* const ikv = take((size_t)PM * C); float* const iq = take((size_t)PM * C2); float* const ia = take((size_t)PM * C2);
    if (dry) { pl.ws_floats = top; return LDX_OK; }

    int64_t count = 0; bool bad = false;
    // ldx_profile: a pair of events around every launch (never while capturing), summed per label when the call has run
    const bool prof_on = profiling && !capturing;
    std::vector<std::pair<const char*, size_t>> marks;
    auto ev = [&]() { if (prof_events.size() <= 2 * marks.size() + 1) { hipEvent_t a = nullptr, b = nullptr; (void)hipEventCreate(&a); (void)hipEventCreate(&b); prof_events.push_back(a); prof_events.push_back(b); } };
    auto begin = [&](const char* name) { if (!prof_on) return; ev(); (void)hipEventRecord(prof_events[2 * marks.size()], st); marks.push_back({name, marks.size()}); };
    auto end = [&]() { if (prof_on) (void)hipEventRecord(prof_events[2 * marks.back().second + 1], st); };
    auto flush = [&]() {
        if (!prof_on || marks.empty()) return;
        (void)hipStreamSynchronize(st);
        for (auto& m : marks) { float ms = 0.f; if (hipEventElapsedTime(&ms, prof_events[2 * m.second], prof_events[2 * m.second + 1]) == hipSuccess) { ProfEntry& pe = prof[m.first]; pe.count += 1; pe.ms += ms; } }
    };
    auto gemm = [&](const char* name, SamDecGemmArgs a) { if (!samdec_gemm_ok(a)) { bad = true; return; } begin(name); launch_samdec_gemm(a, st); end(); ++count; };
    auto with_pe = [&](SamDecGemmArgs a, const float* PE, long period, int cols) { a.PE = PE; a.ldpe = C; a.pe_period = period; a.pe_cols = cols; return a; };
    auto with_ln = [&](SamDecGemmArgs a, const float* Rp, long r_period, const NormW& nw, int group, float eps) {
        a.R = Rp; a.ldr = C; a.r_period = r_period; a.gamma = nw.g; a.beta = nw.b; a.ln_group = group; a.eps = eps; return a; };
    auto with_act = [&](SamDecGemmArgs a, int act) { a.act = act; return a; };
    auto t2i = [&](const SamDecAttnW& w, const NormW& nw, const float* K, const float* V, int shared) {
        gemm("samdec.t2i_q", with_pe(gemm_args(qry, C, w.wq, w.bq, tq, C2, R, C2, C, C2), tok0, R, C2));
        SamDecAttnT2IArgs a; memset(&a, 0, sizeof(a));
        a.Q = tq; a.ldq = C2; a.K = K; a.ldk = C; a.V = V; a.ldv = C; a.kv_shared = shared; a.part = part; a.O = att; a.ldo = C2; a.B = P; a.T = T; a.M = M; a.H = H; a.hd = hd2; a.S = S; a.chunk = chunk;
        a.scale = 1.0f / sqrtf((float)hd2);
        if (!samdec_attn_t2i_ok(a)) bad = true; else { begin("samdec.t2i_attn+merge"); launch_samdec_attn_t2i(a, st); end(); count += 2; }
        gemm("samdec.t2i_out+ln", with_ln(gemm_args(att, C2, w.wo, w.bo, qry, C, R, C, C2, C), qry, 0, nw, C, 1e-5f));
    };
    auto small = [&](const char* name, const float* Q, int ldq, int q_shared, const float* K, const float* V, int ldkv, float* O, int ldo, long Tq, int hd) {
        SamDecAttnSmallArgs a; memset(&a, 0, sizeof(a));
        a.Q = Q; a.ldq = ldq; a.q_shared = q_shared; a.K = K; a.ldk = ldkv; a.V = V; a.ldv = ldkv; a.O = O; a.ldo = ldo; a.B = P; a.Tq = Tq; a.Tk = T; a.H = H; a.hd = hd; a.scale = 1.0f / sqrtf((float)hd);
        if (!samdec_attn_small_ok(a)) bad = true; else { begin(name); launch_samdec_attn_small(a, st); end(); ++count; }
    };

    {
        SamDecPromptArgs a; memset(&a, 0, sizeof(a));
        a.points = c.points; a.labels = c.labels; a.boxes = c.boxes; a.P = P; a.n = n; a.ns = ns; a.C = C; a.size = (float)cfg.image_size; a.gauss = gauss; a.point_emb = point_emb;
        a.not_a_point = not_a_point; a.iou_token = iou_token; a.mask_tokens = mask_tokens; a.out = tokens_out ? tokens_out : tok0;
        begin("samdec.prompt"); launch_samdec_prompt(a, st); end(); ++count;
        if (tokens_out) { flush(); last_launches = count; return launch_status(); }
    }
    for (int i = 0; i < 2; ++i) {
        const SamDecLayerW& L = layers[i];
        const float* const tin = i ? qry : tok0;
        // self-attention of the tokens; layer 0: no positional term, no residual
        SamDecGemmArgs a = gemm_args(tin, C, L.wqkv, L.bqkv, qkv, 3 * C, R, 3 * C, C, C);
        gemm("samdec.self_qkv", i ? with_pe(a, tok0, R, 2 * C) : a);
        small("samdec.self_attn", qkv, 3 * C, 0, qkv + C, qkv + 2 * C, 3 * C, att, C, T, hds);
        gemm("samdec.self_out+ln", with_ln(gemm_args(att, C, L.wo, L.bo, qry, C, R, C, C, C), i ? qry : nullptr, 0, L.n1, C, 1e-5f));
        // tokens attend to the image rows
        if (i) gemm("samdec.t2i_kv", with_pe(gemm_args(keys, C, L.t2i.wkv, L.t2i.bkv, ikv, C, PM, C, C, C2), dense_pe, M, C2));
        t2i(L.t2i, L.n2, i ? ikv : k0v0, (i ? ikv : k0v0) + C2, i ? 0 : 1);
        // MLP
        gemm("samdec.mlp1", with_act(gemm_args(qry, C, L.w1, L.b1, mlp, F, R, F, C, 256), 1));
        gemm("samdec.mlp2+ln", with_ln(gemm_args(mlp, F, L.w2, L.b2, qry, C, R, C, F, C), qry, 0, L.n3, C, 1e-5f));
        // image rows attend to the tokens
        gemm("samdec.i2t_kv", with_pe(gemm_args(qry, C, L.i2t.wkv, L.i2t.bkv, tkv, C, R, C, C, C2), tok0, R, C2));
        if (i) gemm("samdec.i2t_q", with_pe(gemm_args(keys, C, L.i2t.wq, L.i2t.bq, iq, C2, PM, C2, C, C2), dense_pe, M, C2));
        small("samdec.i2t_attn", i ? iq : q0, C2, i ? 0 : 1, tkv, tkv + C2, C, ia, C2, M, hd2);
        gemm("samdec.i2t_out+ln", with_ln(gemm_args(ia, C2, L.i2t.wo, L.i2t.bo, keys, C, PM, C, C2, C), i ? keys : src0, i ? 0 : M, L.n4, C, 1e-5f));
    }
    gemm("samdec.t2i_kv", with_pe(gemm_args(keys, C, fin.wkv, fin.bkv, ikv, C, PM, C, C, C2), dense_pe, M, C2));
    t2i(fin, nfin, ikv, ikv + C2, 0);
    // the four hypernetwork MLPs (grid.z) on tokens 1 .. 4, the IoU head on token 0
    for (int l = 0; l < 3; ++l) {
        const int N = l < 2 ? C : C8;
        SamDecGemmArgs a = gemm_args(l == 0 ? qry + C : l == 1 ? h1 : h2, l == 0 ? T * C : C, hyp_w[l], hyp_b[l], l == 0 ? h1 : l == 1 ? h2 : hyper, l < 2 ? C : 4 * C8, P, N, C, N);
        a.nz = 4; a.xz = l == 0 ? C : (long)P * C; a.wz = (long)N * C; a.bz = N; a.yz = l < 2 ? (long)P * C : C8; a.act = l < 2 ? 1 : 0;
        gemm("samdec.hyper_mlp", a);
    }
    gemm("samdec.iou_head", with_act(gemm_args(qry, T * C, iou_w[0], iou_b[0], i1, Hh, P, Hh, C, 256), 1));
    gemm("samdec.iou_head", with_act(gemm_args(i1, Hh, iou_w[1], iou_b[1], i2, Hh, P, Hh, Hh, 256), 1));
    gemm("samdec.iou_head", gemm_args(i2, Hh, iou_w[2], iou_b[2], c.iou, 4, P, 4, Hh, 4));
    // upscaling: convT1 + LayerNorm2d + GELU -> [P * M][2 x 2][C / 4] (in the k | v buffer, free by now), then convT2 + GELU + the hypernetwork product
    gemm("samdec.up1+ln2d+gelu", with_act(with_ln(gemm_args(keys, C, up1_w, up1_b, ikv, C, PM, C, C, C), nullptr, 0, up_ln, C4, 1e-6f), 2));
    {
        SamDecGemmArgs a = gemm_args(ikv, C4, up2_w, up2_b, nullptr, 0, 4 * PM, C2, C4, C2);
        a.act = 2; a.hyper = hyper; a.g = g; a.logits = c.lowres;
        gemm("samdec.up2+gelu+hyper", a);
    }
    flush();
    last_launches = count;
    if (bad) { set_error("ldx_samdec_predict: internal error (a launch's arguments were refused; the call is incomplete)"); return LDX_EINVAL; }
    return launch_status();
}

int SamDecoderEngine::predict(const float* points, const int* labels, int n, const float* boxes, int P, float* lowres, float* iou, float* tokens_out, hipStream_t st) {
    const char* fn = tokens_out ? "ldx_samdec_prompt_tokens" : "ldx_samdec_predict";
    if (!finalized) { set_error(std::string(fn) + ": not a finalized SAM decoder engine"); return LDX_ESTATE; }
    if (n < 0 || n > 8 || (n > 0 && (!points || !labels)) || (n == 0 && !boxes) || P < 1 || P > 64 || (!tokens_out && (!lowres || !iou))) {
        set_error(std::string(fn) + ": bad argument (n outside 0 .. 8, points without labels, neither points nor boxes, P outside 1 .. 64, null output)"); return LDX_EINVAL; }
    if (!tokens_out && !have_image) { set_error(std::string(fn) + ": no image set (ldx_samdec_set_image)"); return LDX_ESTATE; }
    HIP_OK(hipSetDevice(device));
    DecPlan* pl = nullptr;
    for (DecPlan& p : plans) if (p.P == P && p.n == n && p.box == (boxes ? 1 : 0)) pl = &p;
    if (!pl) {
        DecPlan p; p.P = P; p.n = n; p.box = boxes ? 1 : 0;
        (void)run_ops(p, Call{}, nullptr, st);                  // dry: the workspace size
        HIP_OK(hipMalloc((void**)&p.ws, p.ws_floats * 4));
        plans.push_back(p);
        pl = &plans.back();
    }
    const Call c{n ? points : nullptr, n ? labels : nullptr, boxes, lowres, iou};
    if (tokens_out) return run_ops(*pl, c, tokens_out, st);
    // as Engine::run_bound: a graph is captured once the same buffers have run eagerly, and replayed only for the buffers it was captured with
    const bool same = memcmp(&pl->c, &c, sizeof(Call)) == 0;
    if (!same) pl->valid = false;
    if (graph_mode && pl->valid) {
        HIP_OK(hipGraphLaunch(pl->exec, st));
        ++n_graph_replays;
        return LDX_OK;
    }
    const bool capture = graph_mode && pl->warm && same;
    pl->c = c; pl->warm = true;
    if (!capture) return run_ops(*pl, c, nullptr, st);
    if (pl->exec) { (void)hipGraphExecDestroy(pl->exec); pl->exec = nullptr; }
    if (!cap_stream) HIP_OK(hipStreamCreateWithFlags(&cap_stream, hipStreamNonBlocking));
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipStreamBeginCapture(cap_stream, hipStreamCaptureModeThreadLocal));
    capturing = true;
    int rc = run_ops(*pl, c, nullptr, cap_stream);
    capturing = false;
    hipGraph_t graph = nullptr;
    const char* what = "hipStreamEndCapture";
    hipError_t err = hipStreamEndCapture(cap_stream, &graph);
    if (!rc && err == hipSuccess) { what = "hipGraphInstantiate"; err = hipGraphInstantiate(&pl->exec, graph, nullptr, nullptr, 0); }
    if (graph) (void)hipGraphDestroy(graph);
    if (!rc && err == hipSuccess) { what = "hipGraphLaunch"; err = hipGraphLaunch(pl->exec, st); }
    if (!rc && err != hipSuccess) { set_error(std::string(what) + ": " + hipGetErrorString(err)); rc = LDX_EHIP; }
    if (rc) { if (pl->exec) { (void)hipGraphExecDestroy(pl->exec); pl->exec = nullptr; } return rc; }
    pl->valid = true;
    ++n_graph_captures;
    return launch_status();
}

}  // namespace ldx
