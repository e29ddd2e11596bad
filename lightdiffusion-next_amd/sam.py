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
