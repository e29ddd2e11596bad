"""SAM image encoder, host side: Sam.preprocess and ResizeLongestSide's shape rule, and the network itself stated in torch (segment_anything's
ImageEncoderViT, restated from the published architecture; tests/tools/capture_sam.py checks it against transformers' SamVisionEncoder).

  preprocess_shape(h, w)            ResizeLongestSide.get_preprocess_shape
  preprocess_host(img, size)        Sam.preprocess of a uint8 [h][w][3] image: what ldx_sam_preprocess computes, float for float
  sam_encoder_host(sd, x)           the encoder in fp32: the statement SAMImageEncoderEngine is held to
  sam_encoder_host16(sd, x, dtype)  the same with the engine's number formats: GEMM weights and every stored activation rounded to bf16 / f16, sums in
                                    fp32, biases, norm parameters, pos_embed and the rel_pos tables in fp32.  The tests' tolerances come from it.
Both run on the device of `x` (the CPU in the tests).  The configuration is read off the state dict's shapes.
"""
import torch
import torch.nn.functional as F

PIXEL_MEAN = (123.675, 116.28, 103.53)
PIXEL_STD = (58.395, 57.12, 57.375)
ABLATIONS = ("no_relpos", "no_rel_w", "mask_pad", "scaled_q")      # the four mistakes the fixture must tell from the network (tests/tools/capture_sam.py)


def preprocess_shape(h: int, w: int, size: int = 1024):
    """(new_h, new_w) of ResizeLongestSide.get_preprocess_shape: the longest side becomes `size`."""
    scale = size * 1.0 / max(h, w)
    return int(h * scale + 0.5), int(w * scale + 0.5)


def preprocess_host(img, size: int = 1024) -> torch.Tensor:
    """uint8 [h][w][3] -> fp32 [3][size][size]: (x - pixel_mean) / pixel_std, zero-padded at the bottom and the right (Sam.preprocess)."""
    x = torch.as_tensor(img)
    assert x.dtype == torch.uint8 and x.dim() == 3 and x.shape[2] == 3 and x.shape[0] <= size and x.shape[1] <= size
    x = x.permute(2, 0, 1).float()
    x = (x - torch.tensor(PIXEL_MEAN).view(-1, 1, 1)) / torch.tensor(PIXEL_STD).view(-1, 1, 1)
    return F.pad(x, (0, size - x.shape[2], 0, size - x.shape[1]))


def config_of(sd):
    """SAMConfig read off an encoder state dict's shapes."""
    from .weights import SAMConfig
    _, S, _, E = sd["pos_embed"].shape
    depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    D = sd["blocks.0.attn.rel_pos_h"].shape[1]
    sides = [(sd[f"blocks.{i}.attn.rel_pos_h"].shape[0] + 1) // 2 for i in range(depth)]
    window = min(sides)
    return SAMConfig(image_size=16 * S, embed_dim=E, depth=depth, num_heads=E // D, mlp_dim=sd["blocks.0.mlp.lin1.weight"].shape[0],
                     out_chans=sd["neck.0.weight"].shape[0], window_size=window,
                     global_attn_indexes=tuple(i for i in range(depth) if sides[i] == S and S != window))      # one window of the whole grid is a global block


def _encoder(sd, x, r, ablate=None):
    assert ablate is None or ablate in ABLATIONS
    cfg = config_of(sd)
    E, H, S, C, win = cfg.embed_dim, cfg.num_heads, cfg.grid, cfg.out_chans, cfg.window_size
    dev = x.device
    w16 = lambda k: r(sd[k].float().to(dev))          # noqa: E731  a GEMM operand: stored in the compute type
    w32 = lambda k: sd[k].float().to(dev)             # noqa: E731
    B = x.shape[0]
    M = B * S * S

    def ln(t, pre):
        return F.layer_norm(t, (t.shape[-1],), w32(pre + ".weight"), w32(pre + ".bias"), 1e-6)

    p = r(x.float()).reshape(B, 3, S, 16, S, 16).permute(0, 2, 4, 1, 3, 5).reshape(M, 768)
    t = r(p @ w16("patch_embed.proj.weight").reshape(E, 768).T + w32("patch_embed.proj.bias"))
    t = r((t.view(B, S * S, E) + w32("pos_embed").view(1, S * S, E)).view(M, E))
    for i in range(cfg.depth):
        pre = f"blocks.{i}"
        glob = i in cfg.global_attn_indexes
        n = S if glob else win
        n1 = r(ln(t, pre + ".norm1"))
        if glob:
            src, BW, nw = n1, B, 1
        else:
            nw = -(-S // win)
            Sp = nw * win
            g = F.pad(n1.view(B, S, S, E), (0, 0, 0, Sp - S, 0, Sp - S))
            src = g.view(B, nw, win, nw, win, E).permute(0, 1, 3, 2, 4, 5).reshape(-1, E)
            BW = B * nw * nw
        N = n * n
        qkv = r(src @ w16(pre + ".attn.qkv.weight").T + w32(pre + ".attn.qkv.bias")).view(BW, N, 3, H, 64).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]                                                   # [BW][H][N][64]
        scores = 0.125 * (q @ k.transpose(-1, -2))
        if ablate != "no_relpos":
            idx = torch.arange(n, device=dev)[:, None] - torch.arange(n, device=dev)[None, :] + (n - 1)
            qq = (q * 0.125 if ablate == "scaled_q" else q).reshape(BW, H, n, n, 64)
            rel_h = torch.einsum("bhxyc,xkc->bhxyk", qq, w32(pre + ".attn.rel_pos_h")[idx])
            bias = rel_h[..., :, None]
            if ablate != "no_rel_w":
                bias = bias + torch.einsum("bhxyc,ykc->bhxyk", qq, w32(pre + ".attn.rel_pos_w")[idx])[..., None, :]
            scores = scores + bias.expand(BW, H, n, n, n, n).reshape(BW, H, N, N)
        if ablate == "mask_pad" and not glob:
            yy = (torch.arange(nw, device=dev)[:, None] * win + torch.arange(win, device=dev)[None, :])          # [nw][win] grid coordinate
            real = ((yy < S)[:, None, :, None] & (yy < S)[None, :, None, :]).reshape(nw * nw, N)              # [window][key]
            scores = scores.masked_fill(~real.repeat(B, 1)[:, None, None, :], float("-inf"))
        att = r(r(torch.softmax(scores, dim=-1)) @ v).permute(0, 2, 1, 3).reshape(BW * N, E)
        if glob:
            t = r(att @ w16(pre + ".attn.proj.weight").T + w32(pre + ".attn.proj.bias") + t)
        else:
            pj = r(att @ w16(pre + ".attn.proj.weight").T + w32(pre + ".attn.proj.bias"))
            pj = pj.view(B, nw, nw, win, win, E).permute(0, 1, 3, 2, 4, 5).reshape(B, nw * win, nw * win, E)[:, :S, :S]
            t = r(t + pj.reshape(M, E))
        n2 = r(ln(t, pre + ".norm2"))
        f = r(n2 @ w16(pre + ".mlp.lin1.weight").T)
        f = r(F.gelu(f + w32(pre + ".mlp.lin1.bias")))
        t = r(f @ w16(pre + ".mlp.lin2.weight").T + w32(pre + ".mlp.lin2.bias") + t)
    y = r(t @ w16("neck.0.weight").view(C, E).T)
    y = r(ln(y, "neck.1"))
    y = F.conv2d(y.view(B, S, S, C).permute(0, 3, 1, 2), w16("neck.2.weight"), padding=1)
    y = r(y.permute(0, 2, 3, 1).reshape(M, C))
    y = r(ln(y, "neck.3"))
    return y.view(B, S, S, C).permute(0, 3, 1, 2).contiguous()


@torch.no_grad()
def sam_encoder_host(sd, x, ablate=None) -> torch.Tensor:
    """ImageEncoderViT.forward in fp32: x [B][3][size][size] (preprocessed) -> [B][out_chans][size / 16][size / 16].
    ablate: one of ABLATIONS, a deliberately wrong network for the fixture's condition check."""
    return _encoder(sd, x, lambda t: t, ablate)


@torch.no_grad()
def sam_encoder_host16(sd, x, dtype=torch.bfloat16) -> torch.Tensor:
    """The engine's arithmetic on the host: see the module docstring."""
    return _encoder(sd, x, lambda t: t.to(dtype).float())


# ---- prompt encoder + mask decoder + post-processing (segment_anything PromptEncoder, MaskDecoder, Sam.postprocess_masks; restated from the published
# architecture, tests/tools/capture_samdec.py checks it against transformers' SamPromptEncoder + SamMaskDecoder in fp64) -------------------------------------
#   sam_prompt_host(sd, points, labels, boxes, image_size)   the sparse prompt encodings [P][ns][C]
#   sam_decoder_host(sd, emb, points, labels, boxes)          (low-res logits [P][4][4g][4g], IoU predictions [P][4]); index 0 is the single-mask output
#   postprocess_host(lowres, image_size, input_hw, out_hw)    Sam.postprocess_masks + threshold in numpy fp32: what ldx_samdec_postprocess computes, float for float
#   apply_coords_host / apply_boxes_host                       ResizeLongestSide.apply_coords / apply_boxes
#   select_masks_host(scores, threshold)                       sam_predict's selection rule (src/AutoDetailer/SAM.py:34-53)
#   detector_prompts_host(bboxes, hw, bbox_expansion)          make_sam_mask's centre points and expanded, clamped boxes (SAM.py:230-241)
DECODER_ABLATIONS = ("no_half_pixel", "eps_1e-6", "pe_in_layer0", "swap_corners", "no_ln2d")      # the five mistakes the fixture must tell from the network


def _posenc(coords01, gauss):
    """PositionEmbeddingRandom._pe_encoding: coordinates in [0, 1] -> [.., C]."""
    import math
    c = (2 * coords01 - 1) @ gauss
    c = 2 * math.pi * c
    return torch.cat([torch.sin(c), torch.cos(c)], dim=-1)


@torch.no_grad()
def sam_prompt_host(sd, points, labels, boxes, image_size, dtype=torch.float64, ablate=None, device="cpu"):
    """PromptEncoder's sparse embeddings: points [P][n][2] with labels [P][n] (1 foreground, 0 background, -1 not a point) and / or boxes [P][4], in the
    resized frame -> [P][ns][C].  A padding point with label -1 is appended exactly when there is no box; the box corners come last."""
    w = lambda k: sd["prompt_encoder." + k].to(device, dtype)          # noqa: E731
    gauss = w("pe_layer.positional_encoding_gaussian_matrix")
    shift = 0.0 if ablate == "no_half_pixel" else 0.5
    out = []
    if points is not None:
        pts = torch.as_tensor(points).to(device, dtype) + shift
        lab = torch.as_tensor(labels).to(device, torch.int64)
        if boxes is None:
            pts = torch.cat([pts, torch.zeros((pts.shape[0], 1, 2), dtype=dtype, device=device)], dim=1)
            lab = torch.cat([lab, -torch.ones((lab.shape[0], 1), dtype=torch.int64, device=device)], dim=1)
        e = _posenc(pts / image_size, gauss)
        e = torch.where((lab == -1)[..., None], w("not_a_point_embed.weight").expand_as(e), e)
        e = torch.where((lab == 0)[..., None], e + w("point_embeddings.0.weight"), e)
        e = torch.where((lab == 1)[..., None], e + w("point_embeddings.1.weight"), e)
        out.append(e)
    if boxes is not None:
        b = (torch.as_tensor(boxes).to(device, dtype) + shift).reshape(-1, 2, 2)
        e = _posenc(b / image_size, gauss)
        first, second = (3, 2) if ablate == "swap_corners" else (2, 3)
        e = torch.stack([e[:, 0] + w(f"point_embeddings.{first}.weight")[0], e[:, 1] + w(f"point_embeddings.{second}.weight")[0]], dim=1)
        out.append(e)
    assert out, "neither points nor boxes"
    return torch.cat(out, dim=1)


@torch.no_grad()
def sam_decoder_host(sd, emb, points, labels, boxes, dtype=torch.float32, ablate=None, num_heads=8):
    """PromptEncoder + MaskDecoder.predict_masks for P prompts on one image embedding emb [C][g][g] -> (logits [P][4][4g][4g], iou [P][4]) in `dtype`
    (fp32: the statement SAMMaskDecoderEngine is held to; fp64: compared with the golden).  ablate: one of DECODER_ABLATIONS."""
    assert ablate is None or ablate in DECODER_ABLATIONS
    emb = torch.as_tensor(emb).to(dtype)
    dev = emb.device          # the statement runs where the embedding lies (the CPU in the tests)
    C, g = emb.shape[0], emb.shape[1]
    M, H = g * g, num_heads
    wt = lambda k: sd[k].to(dev, dtype)          # noqa: E731
    eps = 1e-6 if ablate == "eps_1e-6" else 1e-5

    def lin(x, p):
        return x @ wt(p + ".weight").T + wt(p + ".bias")

    def ln(x, p, e=None):
        return F.layer_norm(x, (x.shape[-1],), wt(p + ".weight"), wt(p + ".bias"), eps if e is None else e)

    def attn(p, q, k, v):
        q, k, v = lin(q, p + ".q_proj"), lin(k, p + ".k_proj"), lin(v, p + ".v_proj")
        B, hd = q.shape[0], q.shape[-1] // H
        sp = lambda t: t.reshape(B, t.shape[1], H, hd).transpose(1, 2)          # noqa: E731
        q, k, v = sp(q), sp(k), sp(v)
        a = torch.softmax((q @ k.transpose(-1, -2)) / (hd ** 0.5), dim=-1) @ v
        return lin(a.transpose(1, 2).reshape(B, -1, H * hd), p + ".out_proj")

    sparse = sam_prompt_host(sd, points, labels, boxes, 16 * g, dtype, ablate, dev)
    P = sparse.shape[0]
    tokens = torch.cat([wt("mask_decoder.iou_token.weight"), wt("mask_decoder.mask_tokens.weight")], dim=0)[None].expand(P, -1, -1)
    tokens = torch.cat([tokens, sparse], dim=1)
    src = (emb + wt("prompt_encoder.no_mask_embed.weight").reshape(C, 1, 1)).reshape(C, M).T[None].expand(P, -1, -1)
    cell = (torch.arange(g, dtype=dtype, device=dev) + 0.5) / g
    grid = torch.stack([cell[None, :].expand(g, g), cell[:, None].expand(g, g)], dim=-1)          # (x, y) of every cell centre
    pos = _posenc(grid, wt("prompt_encoder.pe_layer.positional_encoding_gaussian_matrix")).reshape(1, M, C)

    t = "mask_decoder.transformer"
    queries, keys, qpe = tokens, src, tokens
    for i in range(2):
        p = f"{t}.layers.{i}"
        if i == 0 and ablate != "pe_in_layer0":
            queries = attn(p + ".self_attn", queries, queries, queries)
        else:
            q = queries + qpe
            queries = queries + attn(p + ".self_attn", q, q, queries)
        queries = ln(queries, p + ".norm1")
        queries = ln(queries + attn(p + ".cross_attn_token_to_image", queries + qpe, keys + pos, keys), p + ".norm2")
        queries = ln(queries + lin(torch.relu(lin(queries, p + ".mlp.lin1")), p + ".mlp.lin2"), p + ".norm3")
        keys = ln(keys + attn(p + ".cross_attn_image_to_token", keys + pos, queries + qpe, queries), p + ".norm4")
    queries = ln(queries + attn(t + ".final_attn_token_to_image", queries + qpe, keys + pos, keys), t + ".norm_final_attn", 1e-5)

    def mlp3(x, p):
        return lin(torch.relu(lin(torch.relu(lin(x, p + ".layers.0")), p + ".layers.1")), p + ".layers.2")

    u = "mask_decoder.output_upscaling"
    x = keys.transpose(1, 2).reshape(P, C, g, g)
    x = F.conv_transpose2d(x, wt(u + ".0.weight"), wt(u + ".0.bias"), stride=2)
    if ablate != "no_ln2d":
        x = F.layer_norm(x.permute(0, 2, 3, 1), (C // 4,), wt(u + ".1.weight"), wt(u + ".1.bias"), 1e-6).permute(0, 3, 1, 2)
    x = F.gelu(x)
    x = F.gelu(F.conv_transpose2d(x, wt(u + ".3.weight"), wt(u + ".3.bias"), stride=2))
    hyper = torch.stack([mlp3(queries[:, 1 + i], f"mask_decoder.output_hypernetworks_mlps.{i}") for i in range(4)], dim=1)          # [P][4][C / 8]
    logits = (hyper @ x.reshape(P, C // 8, 16 * M)).reshape(P, 4, 4 * g, 4 * g)
    iou = mlp3(queries[:, 0], "mask_decoder.iou_prediction_head")
    return logits, iou


def _bilinear_taps(out: int, inp: int):
    """F.interpolate(mode="bilinear", align_corners=False) along one axis in fp32: (i0, i1, lambda) of every destination index."""
    import numpy as np
    scale = np.float32(inp) / np.float32(out)
    s = scale * (np.arange(out, dtype=np.float32) + np.float32(0.5)) - np.float32(0.5)
    s = np.maximum(s, np.float32(0.0))
    i0 = np.minimum(s.astype(np.int64), inp - 1)
    i1 = i0 + (i0 < inp - 1)
    return i0, i1, (s - i0.astype(np.float32)).astype(np.float32)


def _bilinear_host(v, oh: int, ow: int):
    """v fp32 [n][h][w] -> [n][oh][ow]: (v00 (1 - lx) + v01 lx) (1 - ly) + (v10 (1 - lx) + v11 lx) ly, every product and sum rounded to fp32."""
    import numpy as np
    y0, y1, ly = _bilinear_taps(oh, v.shape[1])
    x0, x1, lx = _bilinear_taps(ow, v.shape[2])
    wx, wy = (np.float32(1.0) - lx)[None, None, :], (np.float32(1.0) - ly)[None, :, None]
    lx, ly = lx[None, None, :], ly[None, :, None]
    top = v[:, y0][:, :, x0] * wx + v[:, y0][:, :, x1] * lx
    bot = v[:, y1][:, :, x0] * wx + v[:, y1][:, :, x1] * lx
    out = top * wy + bot * ly
    assert out.dtype == np.float32
    return out


def postprocess_host(lowres, image_size: int, input_hw, out_hw):
    """Sam.postprocess_masks and the threshold (SamPredictor: masks > mask_threshold = 0) in numpy fp32: lowres [n][L][L] -> bilinear to image_size a side ->
    crop to input_hw (the resized image inside the padded square) -> bilinear to out_hw.  Returns (uint8 [n][H][W], fp32 logits [n][H][W])."""
    import numpy as np
    v = np.ascontiguousarray(np.asarray(lowres, dtype=np.float32))
    full = _bilinear_host(v, image_size, image_size)[:, :input_hw[0], :input_hw[1]]
    out = _bilinear_host(full, out_hw[0], out_hw[1])
    return (out > np.float32(0.0)).astype(np.uint8), out


def apply_coords_host(coords, original_hw, image_size: int = 1024):
    """ResizeLongestSide.apply_coords: (x, y) coordinates [..][2] of the original image -> the resized frame, in float64 as numpy does it."""
    import numpy as np
    nh, nw = preprocess_shape(original_hw[0], original_hw[1], image_size)
    c = np.array(coords, dtype=np.float64, copy=True)
    c[..., 0] = c[..., 0] * (nw / original_hw[1])
    c[..., 1] = c[..., 1] * (nh / original_hw[0])
    return c


def apply_boxes_host(boxes, original_hw, image_size: int = 1024):
    """ResizeLongestSide.apply_boxes: [..][4] boxes (x1, y1, x2, y2)."""
    import numpy as np
    return apply_coords_host(np.asarray(boxes, dtype=np.float64).reshape(-1, 2, 2), original_hw, image_size).reshape(-1, 4)


def select_masks_host(scores, threshold):
    """sam_predict's rule (src/AutoDetailer/SAM.py:34-53) on one prompt's scores: the indices with score >= threshold, in order; if there is none, the first
    index of the largest score, but only if that score is > 0; else nothing.  A score is a numpy float32 and the threshold a Python float, compared as numpy
    compares them."""
    import numpy as np
    scores = np.asarray(scores, dtype=np.float32)
    picked, best, best_score = [], None, 0
    for i in range(len(scores)):
        if scores[i] > best_score:
            best_score, best = scores[i], i
        if scores[i] >= threshold:
            picked.append(i)
    if not picked and best is not None:
        picked.append(best)
    return picked


def detector_prompts_host(bboxes, hw, bbox_expansion):
    """make_sam_mask's prompts (SAM.py:230-241), in the original image's frame: per segment bbox (x1, y1, x2, y2) the centre point and the box expanded by
    bbox_expansion and clamped to the image.  Returns (points [P][1][2], boxes [P][4]) as float64 numpy arrays."""
    import numpy as np
    pts, boxes = [], []
    for b in bboxes:
        w, h = b[2] - b[0], b[3] - b[1]
        pts.append([[b[0] + w / 2, b[1] + h / 2]])
        boxes.append([max(b[0] - bbox_expansion, 0), max(b[1] - bbox_expansion, 0), min(b[2] + bbox_expansion, hw[1]), min(b[3] + bbox_expansion, hw[0])])
    return np.array(pts, dtype=np.float64).reshape(-1, 1, 2), np.array(boxes, dtype=np.float64).reshape(-1, 4)


def detector_selection_host(scores, threshold, combine="first"):
    """Which masks make_sam_mask keeps: scores [P][3] of the segments in order -> the list of (segment, mask index) that end up in the result.
    combine="first": the reference as written, mask_util.combine_masks2 keeps the first collected mask alone; "or": every selected mask of every segment."""
    assert combine in ("first", "or")
    picked = [(p, k) for p in range(len(scores)) for k in select_masks_host(scores[p], threshold)]
    return picked[:1] if combine == "first" else picked


class SAMDetector:
    """SAMDetectorCombined (src/AutoDetailer/SAM.py:185-309) on the device: from the image the pipeline holds and the detector's segments to the mask that
    segs_bitwise_and_mask consumes, without segment_anything.  Per image: one encoder.set_image, one decoder.set_image, one predict over all segments (the
    centre point with label 1 plus the box expanded by bbox_expansion and clamped), one copy of the [P][3] scores to the host for the selection, and one
    post-processing launch for the selected masks alone.

    combine="first" is the reference as written: mask_util.combine_masks2 keeps masks[0] of everything sam_predict collected, so the result is the first
    selected mask of the first segment that selects one; and dilate_mask ignores its dilation.  combine="or" ORs every selected mask of every segment, which
    is what the Impact Pack code the reference was cut from does.  detection_hint, mask_hint_threshold, mask_hint_use_negative and dilation are accepted and
    unused, as in the reference."""

    def __init__(self, encoder_engine, decoder_engine):
        assert encoder_engine.cfg.image_size == decoder_engine.cfg.image_size and encoder_engine.cfg.out_chans == decoder_engine.cfg.hidden
        self.encoder, self.decoder = encoder_engine, decoder_engine

    def detect(self, image, segs, threshold, bbox_expansion, combine="first"):
        """image: fp32 [1,H,W,3] or [H,W,3] in [0, 1] (or uint8); segs: (shape, [segments with .bbox = (x1, y1, x2, y2)]).  Returns the fp32 0/1 mask
        [1,H,W] on the device, or None where the reference returns None (no segment, or no score above 0 and none at the threshold)."""
        assert combine in ("first", "or")
        seg_list = segs[1]
        if len(seg_list) == 0:
            return None
        img = image[0] if image.dim() == 4 else image
        H, W = int(img.shape[0]), int(img.shape[1])
        self.decoder.set_image(self.encoder.set_image(image))
        points, boxes = detector_prompts_host([s.bbox for s in seg_list], (H, W), bbox_expansion)
        out = None
        for p0 in range(0, len(seg_list), 64):          # the decoder takes 64 prompts a call
            p1 = min(p0 + 64, len(seg_list))
            lowres, iou = self.decoder.predict(points[p0:p1], [[1]] * (p1 - p0), boxes[p0:p1], (H, W))
            picked = detector_selection_host(iou.cpu().numpy(), threshold, combine)
            if not picked:
                continue
            idx = torch.tensor([p * 3 + k for p, k in picked], device=lowres.device)
            m = self.decoder.masks(lowres.reshape(-1, lowres.shape[-2], lowres.shape[-1]).index_select(0, idx), (H, W))
            m = m.amax(dim=0, keepdim=True)
            if combine == "first":
                return m.float()
            out = m if out is None else torch.maximum(out, m)
        return None if out is None else out.float()

    def doit(self, sam_model=None, segs=None, image=None, detection_hint=None, dilation=0, threshold=0.93, bbox_expansion=0, mask_hint_threshold=0.7,
             mask_hint_use_negative=False, combine="first"):
        """SAMDetectorCombined.doit's keyword names; sam_model is unused (the engines are this object's).  Returns (mask,) or None."""
        m = self.detect(image, segs, threshold, bbox_expansion, combine)
        return None if m is None else (m,)
