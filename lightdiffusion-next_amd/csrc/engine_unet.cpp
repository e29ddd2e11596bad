// SD1.5 UNet on the shared planner / kernels (engine.cpp).
//
// Mirrors, for the accelerated path only, what the reference spreads over
//   UNetModel1.__init__/forward          src/NeuralNetwork/unet.py:208-770
//   ResBlock1 / Downsample1 / Upsample1  src/AutoEncoders/ResBlock.py:75-335
//   SpatialTransformer / BasicTransformerBlock / FeedForward   src/NeuralNetwork/transformer.py:19-377
//   CrossAttention                       src/Attention/Attention.py:53-124
//   BaseModel.apply_model                src/Model/ModelBase.py:72-133
#include "engine.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

namespace ldx {

UNetEngine::UNetEngine(const ldx_unet_config& c, int dev) : Engine(dev, c.compute_dtype, true, true), cfg(c) {
    const UNetSwitches sw;          // the environment as it is now, not as it was at load (ldx_switches.h)
    cfg_share = sw.cfg_share;
    upconv_phase = sw.upconv_phase;
}
UNetEngine::~UNetEngine() {
    (void)hipSetDevice(device);
    if (d_sigma_cfg) (void)hipFree(d_sigma_cfg);
}

int UNetEngine::validate() const {
    auto bad = [&](const char* m) { set_error(std::string("unsupported UNet config: ") + m); return LDX_EINVAL; };
    if (cfg.model_channels <= 0 || cfg.model_channels % 64) return bad("model_channels must be a multiple of 64");
    if (cfg.context_dim <= 0 || cfg.context_dim % 64) return bad("context_dim must be a multiple of 64");
    // these two (every level's channels = model_channels * channel_mult) are also what the pack kernels' 16-byte stores need (Engine::pack16)
    if (cfg.num_levels < 1 || cfg.num_levels > 8) return bad("num_levels out of range");
    if (cfg.num_heads < 1) return bad("num_heads");
    if (cfg.in_channels < 1 || cfg.in_channels > 64 || cfg.out_channels < 1 || cfg.out_channels > 128) return bad("in/out channels");
    for (int l = 0; l < cfg.num_levels; ++l) {
        const int ch = cfg.model_channels * cfg.channel_mult[l];
        if (ch % cfg.num_heads || (ch / cfg.num_heads) % 8 || ch / cfg.num_heads > 160) return bad("head dim must be a multiple of 8 and <= 160");
        if (ch % 32) return bad("channels not divisible by 32 groups");
    }
    return LDX_OK;
}

int UNetEngine::set_tables(const float* ls, int n, const float* temb, int dim) {
    // after finalize the per-timestep emb_layers table (build_emb_table) and every cached plan depend on these tables
    if (finalized) { set_error("ldx_set_tables after ldx_finalize"); return LDX_ESTATE; }
    if (!ls || !temb || n <= 0 || dim != cfg.model_channels) { set_error("ldx_set_tables: bad argument (temb_dim must equal model_channels)"); return LDX_EINVAL; }
    HIP_OK(hipSetDevice(device));
    void* p = nullptr;
    HIP_OK(hipMalloc(&p, (size_t)n * 4)); dev_allocs.push_back(p);
    HIP_OK(hipMemcpy(p, ls, (size_t)n * 4, hipMemcpyHostToDevice));
    d_log_sigmas = (float*)p; n_sigmas = n;
    HIP_OK(hipMalloc(&p, (size_t)n * dim * 4)); dev_allocs.push_back(p);
    HIP_OK(hipMemcpy(p, temb, (size_t)n * dim * 4, hipMemcpyHostToDevice));
    d_temb = (float*)p;
    return LDX_OK;
}

static int stacked_rows(const std::vector<EmbSrc>& srcs) { int n = 0; for (const EmbSrc& s : srcs) n += s.n; return n; }
bool UNetEngine::mk_res(const std::string& pre, int Cin, int Cout, ResW& r) {
    r.Cin = Cin; r.Cout = Cout;
    if (!mk_norm(pre + ".in_layers.0", Cin, r.gn1)) return false;
    if (!mk_conv3(pre + ".in_layers.2", Cout, Cin, Cin, r.conv1)) return false;
    // emb_layers.1 is batched with every other ResBlock's projection (one skinny GEMM per forward)
    const HostTensor* ew = get(pre + ".emb_layers.1.weight", {Cout, 4 * cfg.model_channels});
    const HostTensor* eb = get(pre + ".emb_layers.1.bias", {Cout});
    if (!ew || !eb) return false;
    r.emb_off = stacked_rows(emb_srcs);
    emb_srcs.push_back({ew, eb, Cout});
    if (!mk_norm(pre + ".out_layers.0", Cout, r.gn2)) return false;
    r.has_skip = Cin != Cout;
    if (r.has_skip && Cin % 64 == 0 && g_plan_sw.fused_skip) return mk_fused_skip(pre + ".out_layers.3", pre + ".skip_connection", Cin, Cout, r);
    if (!mk_conv3(pre + ".out_layers.3", Cout, Cout, Cout, r.conv2)) return false;
    return !r.has_skip || mk_linear(pre + ".skip_connection", Cout, Cin, true, r.skip, true);
}

static inline bool q_prescale() { return g_plan_sw.q_prescale; }

bool UNetEngine::mk_xf(const std::string& pre, int C, int depth, XfW& x) {
    x.C = C; x.depth = depth;
    const int ctx = cfg.context_dim;
    if (!mk_norm(pre + ".norm", C, x.gn)) return false;
    if (!mk_linear(pre + ".proj_in", C, C, true, x.proj_in, true)) return false;
    if (!mk_linear(pre + ".proj_out", C, C, true, x.proj_out, true)) return false;
    x.blocks.resize(depth);
    for (int d = 0; d < depth; ++d) {
        XfBlockW& b = x.blocks[d];
        const std::string bp = pre + ".transformer_blocks." + std::to_string(d);
        if (!mk_norm(bp + ".norm1", C, b.ln1) || !mk_norm(bp + ".norm2", C, b.ln2) || !mk_norm(bp + ".norm3", C, b.ln3)) return false;
        // fused q|k|v for self attention
        const HostTensor* q = get(bp + ".attn1.to_q.weight", {C, C});
        const HostTensor* k = get(bp + ".attn1.to_k.weight", {C, C});
        const HostTensor* v = get(bp + ".attn1.to_v.weight", {C, C});
        if (!q || !k || !v) return false;
        // LDX_LNFOLD=1: fold norm1/2/3 into the q|k|v / q / GEGLU projections (48 launches and the normalised copies of h less per step).
        // Correct and tested, but measured neutral on MI355X (17.26 vs 17.14 ms per step): with every part of the fold switched off the
        // consuming GEMM is still 16 us slower at level 0 when it follows the GEMM that wrote h than when a LayerNorm launch sits between
        // them (50 -> 66 us; the statistics MFMAs, the LDS exchange and the epilogue add 8 more) - profiles/ubench/README.md.  Off by default.
        // Round 4: it does pay where the row-block kernels are not taken (512^2 step 6.01 -> 5.87 ms) and loses where they are (1024^2: 14.31 -> 15.04 with
        // the fold everywhere), so both copies of the three weights are kept (+0.3 GB for SD1.5) and the planner decides per input shape
        // (emit_xf: LDX_LNFOLD_MAXROWS); LDX_LNFOLD=0: plain weights only.
        b.ln_fold = g_plan_sw.lnfold;
        // softmax_scale * log2(e) folded into the q projections at load time (one rounding of c * Wq instead of rounding q and multiplying
        // every score): the attention ops then run with scale = 1 / log2(e), i.e. exp2(q.k - m) as before; LDX_NO_QPRESCALE=1 keeps the plain weights
        const float cq = q_prescale() ? (1.0f / std::sqrt((float)(C / cfg.num_heads))) * 1.44269504088896340736f : 1.0f;
        const HostTensor* q2w = get(bp + ".attn2.to_q.weight", {C, C});
        if (!q2w) return false;
        const std::vector<Piece> qkv_p{rows_piece(q, 0, C, C, cq), rows_piece(k, C, C, C), rows_piece(v, (size_t)2 * C, C, C)}, q2_p{rows_piece(q2w, 0, C, C, cq)};
        if (b.ln_fold) {
            if (!mk_ln_folded(3 * C, C, qkv_p, nullptr, bp + ".norm1", b.qkv_f, b.c1_qkv)) return false;
            if (!mk_ln_folded(C, C, q2_p, nullptr, bp + ".norm2", b.q2_f, b.c1_q2)) return false;
        }
        b.qkv.N = 3 * C; b.qkv.K = C; b.qkv.b = nullptr;
        b.qkv.w = pack16((size_t)3 * C, C, qkv_p);
        b.q2.N = C; b.q2.K = C; b.q2.b = nullptr;
        b.q2.w = pack16(C, C, q2_p);
        if (!b.qkv.w || !b.q2.w) return false;
        if (!mk_linear(bp + ".attn1.to_out.0", C, C, true, b.o1)) return false;
        const HostTensor* k2 = get(bp + ".attn2.to_k.weight", {C, ctx});
        const HostTensor* v2 = get(bp + ".attn2.to_v.weight", {C, ctx});
        if (!k2 || !v2) return false;
        b.kv2.N = 2 * C; b.kv2.K = ctx; b.kv2.b = nullptr; b.kv2.w = nullptr;
        b.kv_off = stacked_rows(kv_srcs);          // columns [kv_off, kv_off + 2C) of the batched k|v projection
        kv_srcs.push_back({k2, nullptr, C}); kv_srcs.push_back({v2, nullptr, C});
        if (!mk_linear(bp + ".attn2.to_out.0", C, C, true, b.o2)) return false;
        // GEGLU projection: rows permuted so each 64-column slab holds 32 value rows then their 32 gate rows (geglu_src_row)
        const int inner = 4 * C;
        const HostTensor* fw = get(bp + ".ff.net.0.proj.weight", {2 * inner, C});
        const HostTensor* fb = get(bp + ".ff.net.0.proj.bias", {2 * inner});
        if (!fw || !fb) return false;
        const std::vector<Piece> ff1_p{rows_piece(fw, 0, 2 * inner, C, 1.0f, inner)};
        if (b.ln_fold && !mk_ln_folded(2 * inner, C, ff1_p, fb, bp + ".norm3", b.ff1_f, b.c1_ff1)) return false;
        b.ff1.N = 2 * inner; b.ff1.K = C;
        b.ff1.w = pack16((size_t)2 * inner, C, ff1_p);
        b.ff1.b = pack32((size_t)2 * inner, {{fb, nullptr, 0, 2 * inner, inner}});
        if (!b.ff1.w || !b.ff1.b) return false;
        if (!mk_linear(bp + ".ff.net.2", C, inner, true, b.ff2)) return false;
    }
    return true;
}

// The structure walk: every packed weight buffer of the UNet from the registered tensors, in one fixed order.  walk_mode says what a buffer is:
// a new allocation (finalize), nothing (refresh: keys and shapes only) or the allocation finalize made (refresh: refill).  Whatever the mode, the
// walk builds a fresh UNetW which, when it succeeds, holds the same pointers as the one before; only then does it replace `un`.
int UNetEngine::walk_weights() {
    UNetW w;
    emb_srcs.clear(); kv_srcs.clear();
    missing.clear(); walk_err.clear(); walk_next = 0;
    const int mc = cfg.model_channels, ted = 4 * mc;
    bool ok = true;
    // --- structure walk, identical in order to UNetModel1.__init__ (unet.py:344-677) ---
    ok = ok && mk_linear("time_embed.0", ted, mc, true, w.te0) && mk_linear("time_embed.2", ted, ted, true, w.te2);
    ok = ok && mk_conv3("input_blocks.0.0", mc, cfg.in_channels, 64, w.conv_in);
    int ch = mc, td_i = 0, ib = 1;
    std::vector<int> chans{mc};
    for (int level = 0; ok && level < cfg.num_levels; ++level) {
        for (int nr = 0; ok && nr < cfg.num_res_blocks[level]; ++nr) {
            BlockW blk;
            const std::string pre = "input_blocks." + std::to_string(ib);
            const int co = cfg.channel_mult[level] * mc;
            blk.has_res = true;
            ok = ok && mk_res(pre + ".0", ch, co, blk.res);
            ch = co;
            const int depth = cfg.transformer_depth[td_i++];
            if (ok && depth > 0) { blk.has_xf = true; ok = mk_xf(pre + ".1", ch, depth, blk.xf); }
            blk.level = level; blk.ch = ch;
            w.in_blocks.push_back(std::move(blk)); chans.push_back(ch); ++ib;
        }
        if (ok && level != cfg.num_levels - 1) {
            BlockW blk; blk.has_down = true;
            ok = mk_conv3("input_blocks." + std::to_string(ib) + ".0.op", ch, ch, ch, blk.down);
            blk.level = level + 1; blk.ch = ch;
            w.in_blocks.push_back(std::move(blk)); chans.push_back(ch); ++ib;
        }
    }
    if (ok && cfg.transformer_depth_middle >= -1) {
        w.has_middle = true;
        ok = mk_res("middle_block.0", ch, ch, w.mid_res0);
        if (ok && cfg.transformer_depth_middle >= 0) {
            w.mid_has_xf = true;
            ok = mk_xf("middle_block.1", ch, std::max(1, (int)cfg.transformer_depth_middle), w.mid_xf) && mk_res("middle_block.2", ch, ch, w.mid_res1);
            if (cfg.transformer_depth_middle == 0) { set_error("transformer_depth_middle == 0 unsupported"); return LDX_EINVAL; }
        }
    }
    int n_out = 0;
    for (int l = 0; l < cfg.num_levels; ++l) n_out += cfg.num_res_blocks[l] + 1;
    int td_o = n_out, ob = 0;
    for (int level = cfg.num_levels - 1; ok && level >= 0; --level) {
        for (int i = 0; ok && i <= cfg.num_res_blocks[level]; ++i) {
            BlockW blk;
            const std::string pre = "output_blocks." + std::to_string(ob);
            const int ich = chans.back(); chans.pop_back();
            const int co = mc * cfg.channel_mult[level];
            blk.has_res = true; blk.skip_ch = ich; blk.level = level; blk.ch = ch;
            ok = mk_res(pre + ".0", ch + ich, co, blk.res);
            ch = co;
            int sub = 1;
            const int depth = cfg.transformer_depth_output[--td_o];
            if (ok && depth > 0) { blk.has_xf = true; ok = mk_xf(pre + ".1", ch, depth, blk.xf); ++sub; }
            if (ok && level && i == cfg.num_res_blocks[level]) {
                blk.has_up = true;
                ok = mk_conv3(pre + "." + std::to_string(sub) + ".conv", ch, ch, ch, blk.up);
            }
            w.out_blocks.push_back(std::move(blk)); ++ob;
        }
    }
    ok = ok && mk_norm("out.0", ch, w.out_gn) && mk_conv3("out.2", cfg.out_channels, mc, mc, w.conv_out);
    ok = ok && mk_stacked(emb_srcs, ted, w.emb_all) && (kv_srcs.empty() || mk_stacked(kv_srcs, cfg.context_dim, w.kv_all));
    w.emb_total = w.emb_all.N; w.kv_total = w.kv_all.N;
    emb_srcs.clear(); kv_srcs.clear();
    if (ok && walk_mode != WALK_ALLOC && walk_next != weight_allocs.size()) { ok = false; walk_err = "the weight layout differs from the one ldx_finalize built (plan switches changed since?)"; }
    // the device packers run on the null stream, in order behind the host path's copies: one wait for all of them, then the staged copies can go
    hipError_t sync = ok && walk_mode != WALK_CHECK ? hipDeviceSynchronize() : hipSuccess;
    if (sync == hipSuccess && walk_mode != WALK_CHECK) sync = hipGetLastError();
    drop_staged();
    if (!ok) return weights_failed();
    if (sync != hipSuccess) { set_error(std::string("weight packing failed: ") + hipGetErrorString(sync)); return LDX_EHIP; }
    un = std::move(w);
    return LDX_OK;
}

int UNetEngine::finalize() {
    if (finalized) return LDX_OK;
    int rc = validate();
    if (rc) return rc;
    HIP_OK(hipSetDevice(device));
    if (!d_log_sigmas) { set_error("ldx_finalize: call ldx_set_tables first"); return LDX_ESTATE; }
    walk_mode = WALK_ALLOC;
    if ((rc = walk_weights())) return rc;
    host.clear();
    { const int rc2 = build_emb_table(); if (rc2) return rc2; }
    finalized = true;
    return LDX_OK;
}

int UNetEngine::refresh_begin() {
    if (!finalized) { set_error("ldx_unet_refresh_begin: not a finalized UNet engine"); return LDX_ESTATE; }
    host.clear();                          // a second begin starts over
    refreshing = true;
    return LDX_OK;
}

int UNetEngine::refresh_abort() {
    if (!finalized) { set_error("ldx_unet_refresh_abort: not a finalized UNet engine"); return LDX_ESTATE; }
    host.clear();
    refreshing = false;
    return LDX_OK;
}

int UNetEngine::refresh_commit() {
    if (!finalized || !refreshing) { set_error("ldx_unet_refresh_commit: call ldx_unet_refresh_begin first"); return LDX_ESTATE; }
    HIP_OK(hipSetDevice(device));
    HIP_OK(hipDeviceSynchronize());        // no forward still reads the buffers about to be rewritten
    // every key and shape first, with nothing written (a failing walk leaves `un` as it is)
    walk_mode = WALK_CHECK;
    int rc = walk_weights();
    if (rc == LDX_OK) {
        walk_mode = WALK_REFILL;
        rc = walk_weights();               // an error from here on (a HIP failure) leaves the weights partly rewritten
    }
    walk_mode = WALK_ALLOC;
    host.clear();
    refreshing = false;                    // either way the refresh is over: the engine holds the new weights, or (validation failed) still the old ones
    if (rc) return rc;
    ++ctx_epoch;                           // cached k|v projections of the context were made with the old weights
    if ((rc = derive_up_phase())) return rc;
    return build_emb_table();
}

// rows [0, rows) of the view -> rows [rows, 2 * rows): the second half of a CFG batch takes over what was computed once for both (plan(): share)
void UNetEngine::op_dup(const Act& a, int rows) {
    Op& o = emit(OP_DUP, "cfg.dup");
    o.dup = DupRowsArgs{ptr(a), cur.arena ? (char*)ptr(a) + (size_t)rows * a.ld * 2 : nullptr, rows, a.C, a.ld};
    o.bytes = 2.0 * 2.0 * (double)rows * a.C;
    snprintf(o.klabel, sizeof(o.klabel), "dup_rows");
}

void UNetEngine::dup_second_half(const DupReq& d) {
    if (!g_plan_sw.cfg_share_copy && d.producer < cur.ops.size()) {
        Op& o = cur.ops[d.producer];
        if (o.kind == OP_GEMM && o.g.C == ptr(d.a) && o.g.ldc == d.a.ld && o.g.M == d.rows && !o.g.geglu && !o.g.C8) { o.g.dup_rows = d.rows; return; }
        if (o.kind == OP_ROWGEMM && o.rg.Y == ptr(d.a) && o.rg.ldy == d.a.ld && o.rg.M == d.rows) { o.rg.dup_rows = d.rows; return; }
    }
    op_dup(d.a, d.rows);
}

// SpatialTransformer.forward (transformer.py:342-377) + BasicTransformerBlock._forward (:186-245)
void UNetEngine::emit_xf(const XfW& x, Act X, Act OUT, int B, int H, int W, Act ctx16, int Mc, int Bshare, const std::vector<DupReq>* dups) {
    const int M = B * H * W, C = x.C, heads = cfg.num_heads, D = C / heads;
    // Shared CFG prefix (plan(): share): up to the first cross-attention both halves of the batch hold the same values, so norm / proj_in / norm1 / q|k|v /
    // self-attention / to_out of the FIRST transformer block run on the first Bq samples (rows [0, Mq)) only
    int Bq = Bshare > 0 ? Bshare : B, Mq = Bq * H * W;
    // which launches the level's stages run as; norm + proj_in become one rowgemm launch in fuse_gn_rowgemm, once norm's statistics come from its producer
    const XfPick pick = xf_pick(XfShape{C, heads, B, H * W, Mc, Bshare, x.blocks[0].ln_fold, 0});
    auto head = [&](const Act& a) { return rows(a, 0, Mq); };      // the first Mq rows of a buffer
    Act t1 = new_act(M, C);
    op_gn("xf.norm", X, t1, Bq, H * W, x.gn, 1e-6f, false);
    Act h = new_act(M, C);
    op_gemm("xf.proj_in", head(t1), x.proj_in, head(h), Act{});
    release(t1);
    Act n{};
    // LayerNorm + projection of the first Mq rows of h, by stage: `w` behind a LayerNorm (its own launch or rowgemm's prologue), the folded copy `wf` otherwise
    auto norm_gemm = [&](XfStage st, const char* rowgemm_name, const char* ln_name, const char* name, const NormW& ln, const LinearW& w, const LinearW& wf, const float* c1, Act Cc, bool geglu) {
        if (st == XS_ROWBLOCK) { op_rowgemm(rowgemm_name, head(h), w, head(Cc), Act{}, 1, &ln); return; }
        if (st == XS_FOLDED) {
            op_gemm(name, head(h), wf, head(Cc), Act{}, geglu, [&](GemmArgs& g) { g.ln_c1 = c1; g.ln_eps = 1e-5f; });
            return;
        }
        if (!n.valid) n = new_act(M, C);
        NormW plain = ln;
        if (st == XS_LN_FOLDED) { plain.g = nullptr; plain.b = nullptr; }     // gamma / beta already live in the folded weights / bias
        op_ln(ln_name, head(h), head(n), plain);
        op_gemm(name, head(n), st == XS_LN_FOLDED ? wf : w, head(Cc), Act{}, geglu);
    };
    const AttnEdit prescaled = [](AttnArgs& a) { if (q_prescale()) a.scale = 1.0f / 1.44269504088896340736f; };      // the q rows of the projections already carry scale * log2(e) (mk_xf)
    // projection + residual into h, in place: x += W . a + b
    auto out_gemm = [&](XfStage st, const char* name, Act a, const LinearW& w) {
        if (st == XS_ROWBLOCK) op_rowgemm(name, a, w, head(h), head(h), 0, nullptr); else op_gemm(name, a, w, head(h), head(h));
    };
    for (int d = 0; d < x.depth; ++d) {
        const XfBlockW& b = x.blocks[d];
        const XfBlockPick& bp = d == 0 ? pick.first : pick.rest;
        Act qkv = new_act(M, 3 * C);
        norm_gemm(bp.qkv, "xf.ln1+qkv", "xf.ln1", "xf.qkv", b.ln1, b.qkv, b.qkv_f, b.c1_qkv, qkv, false);
        Act a = new_act(M, C);
        const char* base = (const char*)ptr(qkv);
        op_attn("xf.attn1", base, 3 * C, base + (size_t)C * 2, 3 * C, base + (size_t)2 * C * 2, 3 * C, a, Bq, heads, H * W, H * W, D, prescaled);
        release(qkv);
        out_gemm(bp.o1, "xf.o1", head(a), b.o1);                   // x += attn1(norm1(x))
        if (Bq != B) {
            // the context enters here: from now on the halves differ.  The second half's rows take over the shared results that full-batch ops still read.
            cur.prefix_end = cur.ops.size();                               // every op so far ran on one half of the batch
            if (dups) for (const DupReq& dq : *dups) dup_second_half(dq);
            dup_second_half(DupReq{h, Mq, cur.ops.size() - 1});       // the op just emitted (to_out + residual) wrote h
            Bq = B; Mq = M;
        }
        // k|v of the context come from the one batched projection emitted at the start of the forward
        const char* kvb = (const char*)((uintptr_t)cur.arena + cur.kv_all_off) + (size_t)b.kv_off * 2;
        if (bp.xattn) {
            // LayerNorm + q projection + attention over the context + out projection + residual as ONE launch (xattn_block.hip)
            Op& o = emit(OP_XATTN, "xf.xattn2");
            XAttnArgs& xa = o.xa;
            xa.H = ptr(h); xa.ldh = h.ld; xa.M = M; xa.N = H * W; xa.C = C; xa.heads = heads; xa.ln_g = b.ln2.g; xa.ln_b = b.ln2.b; xa.eps = 1e-5f;
            xa.Wq = b.q2.w; xa.Wo = b.o2.w; xa.bo = b.o2.b; xa.K = kvb; xa.ldk = un.kv_total; xa.V = kvb + (size_t)C * 2; xa.ldv = un.kv_total; xa.Mk = Mc;
            xa.scale = q_prescale() ? 1.0f / 1.44269504088896340736f : 1.0f / std::sqrt((float)D);
            o.flops = 2.0 * 2.0 * M * (double)C * C + 4.0 * B * heads * (double)(H * W) * Mc * D;
            o.bytes = 2.0 * 2.0 * (double)M * C;
            snprintf(o.klabel, sizeof(o.klabel), "xattn_block<%s>", dt_name());
            cur.flops += o.flops;
        } else {
            Act q = new_act(M, C);
            norm_gemm(bp.q2, "xf.ln2+q2", "xf.ln2", "xf.q2", b.ln2, b.q2, b.q2_f, b.c1_q2, q, false);
            op_attn("xf.attn2", ptr(q), C, kvb, un.kv_total, kvb + (size_t)C * 2, un.kv_total, a, B, heads, H * W, Mc, D, prescaled);
            release(q);
            out_gemm(bp.o2, "xf.o2", a, b.o2);                     // x += attn2(norm2(x), ctx)
        }
        release(a);
        if (bp.ffblock) {
            // LayerNorm + GEGLU projection + down projection + residual as ONE launch (ff_block.hip): the [M][4C] activation never leaves the CUs
            Op& o = emit(OP_FFBLOCK, "xf.ffblock");
            FFBlockArgs& fa = o.fb;
            fa.H = ptr(h); fa.ldh = h.ld; fa.M = M; fa.C = C; fa.inner = 4 * C; fa.ln_g = b.ln3.g; fa.ln_b = b.ln3.b; fa.eps = 1e-5f;
            fa.W1 = b.ff1.w; fa.b1 = b.ff1.b; fa.W2 = b.ff2.w; fa.b2 = b.ff2.b;
            o.flops = 2.0 * M * (double)C * (8.0 * C) + 2.0 * M * (double)C * (4.0 * C);
            o.bytes = 2.0 * 2.0 * (double)M * C;
            snprintf(o.klabel, sizeof(o.klabel), "ff_block<%s>", dt_name());
            cur.flops += o.flops;
        } else {
            Act f = new_act(M, 4 * C);
            norm_gemm(bp.ff1, "", "xf.ln3", "xf.ff1", b.ln3, b.ff1, b.ff1_f, b.c1_ff1, f, true);        // GEGLU
            op_gemm("xf.ff2", f, b.ff2, h, h);                     // x = ff(norm3(x)) + x
            release(f);
        }
    }
    if (n.valid) release(n);
    if (pick.proj_out == XS_ROWBLOCK) op_rowgemm("xf.proj_out", h, x.proj_out, OUT, X, 0, nullptr);
    else op_gemm("xf.proj_out", h, x.proj_out, OUT, X);         // + x_in
    release(h);
}

// The batch of the shared CFG prefix for an evaluation (0 = every op on the full batch): a CFG evaluation over ONE latent batch (xB > 0, B2 == 2 xB, no
// c_concat), a model with a cross-attention for the prefix to end at, and enough rows per half that the prefix ops still fill the chip — below
// LDX_CFG_SHARE_MINROWS (default 8192: 512^2 at bs = 1 has 4096 and measured 5.73 against 5.69 ms per step shared) nothing is shared.
int UNetEngine::share_for(int B2, int h, int w, int xB, bool denoise, bool concat) const {
    const long share_minrows = g_plan_sw.cfg_share_minrows;
    if (!cfg_share || !denoise || concat || xB <= 0 || B2 != 2 * xB || (cfg_share == 1 && (long)xB * h * w < share_minrows)) return 0;
    for (auto& blk : un.in_blocks) if (blk.has_xf) return xB;
    return 0;
}

int UNetEngine::plan(int B2, int h, int w, int Mc, int share) {
    return build_plan(PlanKey{B2, h, w, Mc, share}, [&]() -> int {
        const int mc = cfg.model_channels, ted = 4 * mc;
        // fixed small buffers
        auto f32buf = [&](size_t n) { float* p = arena_ptr<float>(n * 4); return cur.arena ? p : nullptr; };      // null in the dry pass: emit_res and the prep op test them
        cur.d_temb_out = f32buf((size_t)B2 * mc); cur.d_e1 = f32buf((size_t)B2 * ted); cur.d_e2 = f32buf((size_t)B2 * ted); cur.d_emb_all = f32buf((size_t)B2 * un.emb_total);
        cur.gn_ws_off = a_alloc(gn_ws_bytes(B2, (long)h * w));
        cur.d_eps = f32buf((size_t)B2 * h * w * cfg.out_channels);

        // ---- level geometry & concat buffers (so skips are written in place, no torch.cat copy) ----
        struct Skip { Act act; int H, W; };
        std::vector<int> Hs{h}, Ws{w};
        for (int l = 1; l < cfg.num_levels; ++l) { Hs.push_back((Hs.back() + 1) / 2); Ws.push_back((Ws.back() + 1) / 2); }
        // the walk's bookkeeping (BlockW::level, ch) sizes the concat buffers of the output blocks: skip s is conv_in's output (s = 0) or input block s - 1's;
        // output block k consumes skip (n_skips - 1 - k) beside its own h channels
        std::vector<int> in_ch{mc}, in_lv{0}, out_hch;
        for (const BlockW& blk : un.in_blocks) { in_ch.push_back(blk.ch); in_lv.push_back(blk.level); }
        for (const BlockW& blk : un.out_blocks) out_hch.push_back(blk.ch);
        const int n_skips = (int)in_ch.size();
        std::vector<Act> cat(n_skips);
        for (int k = 0; k < n_skips; ++k) {
            const int s = n_skips - 1 - k, lv = in_lv[s];
            cat[k] = new_act(B2 * Hs[lv] * Ws[lv], out_hch[k] + in_ch[s]);
        }
        auto skip_view = [&](int s) { const int k = n_skips - 1 - s; return view(cat[k], out_hch[k], in_ch[s]); };

        // ---- ops ----
        auto res = [&](const ResW& r, Act X, Act OUT, int B, int H, int W) { emit_res(r, X, OUT, B, H, W, cur.d_emb_all, un.emb_total); };      // with its columns of the batched emb_layers output
        Act xin = new_act(B2 * h * w, 64);
        cur.prep_xc_off = xin.off;
        {
            PrepArgs& p = emit(OP_PREP, "prep").prep;          // x, sigma / timesteps and c_concat are the call's
            p.B = B2; p.C = cfg.in_channels; p.H = h; p.W = w; p.Cpad = 64; p.xc = ptr(xin);
            p.log_sigmas = d_log_sigmas; p.n_sigmas = n_sigmas; p.temb_table = d_temb; p.temb_dim = mc; p.temb_out = cur.d_temb_out;
            if (d_emb_table) { p.emb_table = d_emb_table; p.emb_n = un.emb_total; p.emb_out = cur.d_emb_all; }
        }
        Act ctx16 = new_act(B2 * Mc, cfg.context_dim);
        { Op& o = emit(OP_CVT, "ctx.cvt"); o.cvt = CvtArgs{nullptr, ptr(ctx16), (size_t)B2 * Mc * cfg.context_dim}; o.ctx_only = true; }
        if (!d_emb_table) {       // per-step time-embedding MLP (LDX_EMB_TABLE=0); otherwise the prep kernel gathers the timestep's row of the table
            emit(OP_SKINNY, "time_embed.0").sk = skinny_args(cur.d_temb_out, mc, un.te0.w, un.te0.b, cur.d_e1, ted, B2, ted, mc, 0, 1);
            emit(OP_SKINNY, "time_embed.2").sk = skinny_args(cur.d_e1, ted, un.te2.w, un.te2.b, cur.d_e2, ted, B2, ted, ted, 0, 1);
            emit(OP_SKINNY, "emb_layers").sk = skinny_args(cur.d_e2, ted, un.emb_all.w, un.emb_all.b, cur.d_emb_all, un.emb_total, B2, un.emb_total, ted, 0, 0);
            cur.flops += 2.0 * B2 * ((double)ted * mc + (double)ted * ted + (double)un.emb_total * ted);
        }
        Act kvall = new_act(B2 * Mc, un.kv_total);
        cur.kv_all_off = kvall.off;
        op_gemm("xf.kv2_all", ctx16, un.kv_all, kvall, Act{}, 0, [](Op& o) { o.ctx_only = true; });

        int lv = 0, s = 0;
        Act hcur = skip_view(0);
        // Bp: batch of the ops in front of the first cross-attention (share > 0: one half of the CFG batch stands for both); `pend` = what they produce
        // that later full-batch ops read (the skip connections), duplicated into the second half's rows when the prefix ends (emit_xf)
        int Bp = share > 0 ? share : B2;
        std::vector<DupReq> pend;
        op_conv("conv_in", xin, Bp, h, w, 64, un.conv_in, 1, h, w, hcur, Act{});
        cur.flops -= 2.0 * Bp * h * w * (double)mc * 9.0 * (64 - cfg.in_channels);   // padded channels are not algorithmic work
        release(xin);
        if (Bp != B2) pend.push_back({hcur, Bp * h * w, cur.ops.size() - 1});
        for (auto& blk : un.in_blocks) {
            ++s;
            Act dst = skip_view(s);
            if (blk.has_down) {
                op_conv("down", hcur, Bp, Hs[lv], Ws[lv], in_ch[s - 1], blk.down, 2, Hs[lv + 1], Ws[lv + 1], dst, Act{});
                ++lv;
                if (Bp != B2) pend.push_back({dst, Bp * Hs[lv] * Ws[lv], cur.ops.size() - 1});
            } else if (blk.has_xf) {
                Act mid = new_act(B2 * Hs[lv] * Ws[lv], blk.res.Cout);
                res(blk.res, hcur, mid, Bp, Hs[lv], Ws[lv]);
                if (Bp != B2) {
                    pend.push_back({mid, Bp * Hs[lv] * Ws[lv], cur.ops.size() - 1});          // proj_out's residual reads it for every sample (emit_res ends with the conv that writes it)
                    emit_xf(blk.xf, mid, dst, B2, Hs[lv], Ws[lv], ctx16, Mc, Bp, &pend);
                    Bp = B2; pend.clear();
                } else {
                    emit_xf(blk.xf, mid, dst, B2, Hs[lv], Ws[lv], ctx16, Mc);
                }
                release(mid);
            } else {
                res(blk.res, hcur, dst, Bp, Hs[lv], Ws[lv]);
                if (Bp != B2) pend.push_back({dst, Bp * Hs[lv] * Ws[lv], cur.ops.size() - 1});
            }
            hcur = dst;
        }
        // middle block (unet.py:537-584); its last op writes column 0 of the first concat buffer
        {
            const int Mm = B2 * Hs[lv] * Ws[lv];
            Act dst = view(cat[0], 0, out_hch[0]);
            if (!un.has_middle) { set_error("UNet config without a middle block is not supported by the planner"); return LDX_EINVAL; }
            if (un.mid_has_xf) {
                Act m0 = new_act(Mm, un.mid_res0.Cout);
                res(un.mid_res0, hcur, m0, B2, Hs[lv], Ws[lv]);
                Act m1 = new_act(Mm, un.mid_res0.Cout);
                emit_xf(un.mid_xf, m0, m1, B2, Hs[lv], Ws[lv], ctx16, Mc);
                release(m0);
                res(un.mid_res1, m1, dst, B2, Hs[lv], Ws[lv]);
                release(m1);
            } else {
                res(un.mid_res0, hcur, dst, B2, Hs[lv], Ws[lv]);
            }
        }
        // output blocks: input of block k is the whole concat buffer cat[k]
        int k = 0;
        Act final_h{};
        for (auto& blk : un.out_blocks) {
            const bool last = (k == n_skips - 1);
            const int Hc = Hs[lv], Wc = Ws[lv], Mrows = B2 * Hc * Wc;
            // where does this block's result go?  column 0 of the next concat buffer (at the next block's resolution)
            const int co = blk.res.Cout;
            int nsub = 1 + (blk.has_xf ? 1 : 0) + (blk.has_up ? 1 : 0);
            auto target = [&](bool is_final_sub, int rows) -> Act {
                if (is_final_sub && !last) return view(cat[k + 1], 0, out_hch[k + 1]);
                return new_act(rows, co);
            };
            int sub = 0;
            Act x = cat[k];
            Act r_out = target(++sub == nsub, Mrows);
            res(blk.res, x, r_out, B2, Hc, Wc);
            release(cat[k]);
            x = r_out;
            if (blk.has_xf) {
                Act x_out = target(++sub == nsub, Mrows);
                emit_xf(blk.xf, x, x_out, B2, Hc, Wc, ctx16, Mc);
                release(x);
                x = x_out;
            }
            if (blk.has_up) {
                const int Hn = Hs[lv - 1], Wn = Ws[lv - 1];       // output_shape = hs[-1].shape (unet.py:754)
                Act u_out = target(++sub == nsub, B2 * Hn * Wn);
                op_conv("up", x, B2, Hc, Wc, co, blk.up, 1, Hn, Wn, u_out, Act{});
                if (int rc = up_to_phase(blk.up)) return rc;
                release(x);
                x = u_out; --lv;
            }
            final_h = x;
            ++k;
        }
        // out: GroupNorm -> SiLU -> conv3x3 (unet.py:663-677), fp32 NHWC eps
        {
            const int Mrows = B2 * h * w;
            Act t = new_act(Mrows, mc);
            op_gn("out.gn", final_h, t, B2, h * w, un.out_gn, 1e-5f, true);
            release(final_h);
            op_conv("out.conv", t, B2, h, w, mc, un.conv_out, 1, h, w, Act{}, Act{}, nullptr, 0, cur.d_eps, cfg.out_channels);
            release(t);
        }
        { FinishArgs& f = emit(OP_FINISH, "finish").fin; f.eps = cur.d_eps; f.ld = cfg.out_channels; f.B = B2; f.C = cfg.out_channels; f.HW = h * w; }          // x, sigma and out are the call's
        release(ctx16); release(kvall);
        // what the shared prefix saves: every op in front of the first hand-over copy ran on half the batch (the context-only ops are not part of it)
        if (share > 0) {
            for (size_t i = 0; i < cur.prefix_end && i < cur.ops.size(); ++i) if (!cur.ops[i].ctx_only) cur.flops_shared += cur.ops[i].flops;
            cur.flops_shared -= 2.0 * share * h * w * (double)mc * 9.0 * (64 - cfg.in_channels);        // conv_in's padded channels are not algorithmic work (see above)
        }
        fuse_gn_stats();
        fuse_gn_rowgemm();
        return LDX_OK;
    });
}

// Upsample1 (ResBlock.py:75-138) as four 2 x 2 convs, one per output parity, over the stored image: 4/9 of the 9-tap op's MFMA work (GemmArgs::up2x).  Taken where
// gemm_upconv_phase says the form exists and the planner may take it; everything else — odd sizes, where output_shape is no exact double, small levels that need split-K — keeps the op.
int UNetEngine::up_to_phase(const LinearW& w) {
    Op& o = cur.ops.back();
    GemmArgs ph;
    if (!upconv_phase || !gemm_upconv_phase(o.g, true, &ph)) return LDX_OK;
    UpPhase* u = nullptr;
    for (UpPhase& e : up_phase) if (e.w9 == w.w) u = &e;
    if (!u) {
        const size_t bytes = (size_t)16 * w.N * ph.Cin * 2;
        void* p = nullptr;
        HIP_OK(hipMalloc(&p, bytes));
        dev_allocs.push_back(p);
        weight_bytes += bytes;
        up_phase.push_back({w.w, p, w.N, ph.Cin});
        u = &up_phase.back();
        launch_up_phase(up_phase_args(u->w9, u->wp, u->N, u->Cin, dt), nullptr);
        HIP_OK(hipStreamSynchronize(nullptr));
        HIP_OK(hipGetLastError());
    }
    ph.W = u->wp;
    ph.up2x = upconv_phase >= 2 ? 1 : 2;         // the tile order: phase-major unless LDX_UPCONV_PHASE=2 asks for band-major (GemmArgs::up2x)
    const double full = o.flops;
    o.g = ph;
    o.flops = full * 4.0 / 9.0;
    o.bytes = 2.0 * ((double)(ph.M / 4) * ph.Cin + 16.0 * ph.N * ph.Cin + (double)ph.M * ph.N);
    cur.flops -= full - o.flops;
    cur.flops_up2x += full - o.flops;
    return LDX_OK;
}
int UNetEngine::derive_up_phase() {
    if (up_phase.empty()) return LDX_OK;
    for (const UpPhase& u : up_phase) launch_up_phase(up_phase_args(u.w9, u.wp, u.N, u.Cin, dt), nullptr);
    HIP_OK(hipStreamSynchronize(nullptr));
    HIP_OK(hipGetLastError());
    return LDX_OK;
}

// The 22 emb_layers outputs for EVERY timestep of the table (ldx_set_tables), by the same three skinny launches a forward would run on its B2 rows:
// row t of d_emb_table is bit-identical to what those launches write for a sample whose timestep index is t (the skinny kernel's rows are independent).
int UNetEngine::build_emb_table() {
    if (!g_plan_sw.emb_table || !d_temb || n_sigmas <= 0 || un.emb_total <= 0 || un.emb_total % 4) return LDX_OK;
    if (finalized && !d_emb_table) return LDX_OK;        // a refresh rebuilds the table finalize() built, in place (the plans hold its address); it never adds one
    const bool refill = d_emb_table != nullptr;
    const int mc = cfg.model_channels, ted = 4 * mc, n = n_sigmas;
    float *e1 = nullptr, *e2 = nullptr, *tab = d_emb_table;
    auto fail = [&](hipError_t err, const char* what) {       // nothing of a half-built table survives an error
        if (e1) (void)hipFree(e1);
        if (e2) (void)hipFree(e2);
        if (tab && !refill) (void)hipFree(tab);
        set_error(std::string(what) + ": " + hipGetErrorString(err));
        return LDX_EHIP;
    };
    hipError_t err;
    if ((err = hipMalloc((void**)&e1, (size_t)n * ted * 4)) != hipSuccess) return fail(err, "build_emb_table: hipMalloc");
    if ((err = hipMalloc((void**)&e2, (size_t)n * ted * 4)) != hipSuccess) return fail(err, "build_emb_table: hipMalloc");
    if (!refill && (err = hipMalloc((void**)&tab, (size_t)n * un.emb_total * 4)) != hipSuccess) return fail(err, "build_emb_table: hipMalloc");
    launch_skinny(skinny_args(d_temb, mc, un.te0.w, un.te0.b, e1, ted, n, ted, mc, 0, 1), dt, nullptr);
    launch_skinny(skinny_args(e1, ted, un.te2.w, un.te2.b, e2, ted, n, ted, ted, 0, 1), dt, nullptr);
    launch_skinny(skinny_args(e2, ted, un.emb_all.w, un.emb_all.b, tab, un.emb_total, n, un.emb_total, ted, 0, 0), dt, nullptr);
    if ((err = hipStreamSynchronize(nullptr)) != hipSuccess) return fail(err, "build_emb_table: hipStreamSynchronize");
    if ((err = hipGetLastError()) != hipSuccess) return fail(err, "build_emb_table: kernel launch");
    (void)hipFree(e1); (void)hipFree(e2);
    if (refill) return LDX_OK;
    dev_allocs.push_back(tab);
    d_emb_table = tab;
    weight_bytes += (size_t)n * un.emb_total * 4;
    return LDX_OK;
}

int UNetEngine::run_cfg(const float* x, float sigma, const float* ctx, int B, int h, int w, int Mc, float* out, hipStream_t st, int t_index) {
    if (B <= 0) { set_error("ldx_unet_denoise_cfg: bad argument"); return LDX_EINVAL; }
    if (t_index >= n_sigmas) { set_error("ldx_unet_denoise_cfg_t: t_index outside the sigma table"); return LDX_EINVAL; }
    HIP_OK(hipSetDevice(device));
    if (sigma_cfg_cap < 2 * B) {
        HIP_OK(hipStreamSynchronize(st));
        if (d_sigma_cfg) (void)hipFree(d_sigma_cfg);
        d_sigma_cfg = nullptr; sigma_cfg_cap = 0;
        HIP_OK(hipMalloc((void**)&d_sigma_cfg, sizeof(float) * 4 * B));
        sigma_cfg_cap = 2 * B;
    }
    float* d_t = d_sigma_cfg + sigma_cfg_cap;
    if (t_index >= 0) launch_fill2_f32(d_sigma_cfg, sigma, d_t, (float)t_index, 2 * B, st);          // outside the captured graph: the values change every step
    else launch_fill_f32(d_sigma_cfg, sigma, 2 * B, st);
    return run(x, d_sigma_cfg, ctx, 2 * B, h, w, Mc, out, true, st, B, nullptr, 0, t_index >= 0 ? d_t : nullptr);
}
int UNetEngine::timestep_lookup(const float* sigma_dev, int n, int* out_dev, hipStream_t st) {
    if (!d_log_sigmas) { set_error("ldx_unet_timestep: needs a UNet engine with its sigma table (ldx_set_tables)"); return LDX_ESTATE; }
    if (!sigma_dev || !out_dev || n < 0) { set_error("ldx_unet_timestep: bad argument"); return LDX_EINVAL; }
    HIP_OK(hipSetDevice(device));
    launch_timestep(sigma_dev, d_log_sigmas, n_sigmas, n, out_dev, st);
    HIP_OK(hipGetLastError());
    return LDX_OK;
}

int UNetEngine::run(const float* x, const float* sigma_or_t, const float* ctx, int B2, int h, int w, int Mc, float* out, bool denoise, hipStream_t st, int xB,
                const float* c_concat, int cc_channels, const float* t_idx) {
    if (!denoise) t_idx = nullptr;            // forward mode: sigma_or_t already carries the indices
    if (c_concat && (cc_channels <= 0 || cc_channels >= cfg.in_channels || (denoise && cfg.in_channels - cc_channels != cfg.out_channels))) {
        set_error("ldx_unet_denoise_concat: c_concat channels must leave the latent's channels (in_channels - cc_channels == out_channels)"); return LDX_EINVAL;
    }
    if (!c_concat) cc_channels = 0;
    if (xB < 0 || (xB > 0 && B2 % xB != 0)) { set_error("ldx_unet_*: the batch of x must divide the evaluation batch"); return LDX_EINVAL; }
    if (!finalized) { set_error("ldx_unet_*: engine not finalized"); return LDX_ESTATE; }
    if (!x || !sigma_or_t || !ctx || !out || B2 <= 0 || h <= 0 || w <= 0 || Mc <= 0) { set_error("ldx_unet_*: bad argument"); return LDX_EINVAL; }
    HIP_OK(hipSetDevice(device));
    // CFG evaluation over one latent batch (ldx_unet_denoise_cfg*: xB > 0 and B2 == 2 xB): the two halves are identical up to the first cross-attention, which
    // the plan then computes once (plan(): share).  LDX_CFG_SHARE=0: every op on the full batch, as the concatenated ldx_unet_denoise call runs it.
    const int share = share_for(B2, h, w, xB, denoise, c_concat != nullptr);
    if (int rc = select_plan(PlanKey{B2, h, w, Mc, share}, st, [&] { return plan(B2, h, w, Mc, share); })) return rc;
    bind = Bindings{};
    bind.x = x; bind.s = sigma_or_t; bind.ctx = ctx; bind.out = out; bind.den = denoise; bind.xB = xB; bind.cc = c_concat; bind.ccn = cc_channels; bind.t = t_idx;
    bind.ctxc = ctx_cache;
    // context cache: the ctx_only ops run here, eagerly, only when this plan's buffers do not hold the projections of (ctx, epoch) yet; every
    // other op (and the captured graph) then leaves them out
    if (bind.ctxc && !(cur.kv_ptr == ctx && cur.kv_epoch == ctx_epoch && cur.kv_stream == st)) {
        prof_graph = false;
        if (int rc = exec_ops(st, 0, (size_t)-1, 2)) return rc;
        cur.kv_ptr = ctx; cur.kv_epoch = ctx_epoch; cur.kv_stream = st;
    }
    return run_bound(st, bind.ctxc ? 1 : 0);
}

}  // namespace ldx
