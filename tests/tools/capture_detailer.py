"""Golden capture for the ADetailer path (DetailerForEachTest.doit): writes tests/golden/detailer.npz and tests/golden/detailer.META.txt.  Build
container only (needs Pillow and the reference; see oracle/ref_capture.py for how the reference is entered).

  host functions      the reference's make_crop_region, enhance_detail's sample size, ksampler_wrapper's sigma selection and segs_bitwise_and_mask on
                      the argument lists of tests/_detailer_ref.py
  stand-in runs       doit with VAEEncode.encode / ksampler_wrapper / vae.decode replaced by (the pixels, the latent, the byte table 255 - v)
  tiny-network run    the same call on synthetic tiny networks, and its distance to five perturbed runs ("wiring distances")

src.AutoDetailer imports torchvision, cv2 and ultralytics, which are absent here: three stand-in modules go into sys.modules first (META says what
each is).  WildcardChooser.get is replaced for the multi-segment runs only (META says why).

    python tests/tools/capture_detailer.py [--skip-real]      # --skip-real keeps the tiny-network keys of the existing file
"""
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import ref_capture  # noqa: E402
import _detailer_ref as D  # noqa: E402


def install_standins():
    """cv2 (only cv2.dilate is used, by the detectors), ultralytics.YOLO (the detector), torchvision.transforms.GaussianBlur (the mask feather)."""
    sys.modules["cv2"] = types.ModuleType("cv2")
    ul = types.ModuleType("ultralytics")
    ul.YOLO = object
    sys.modules["ultralytics"] = ul

    class GaussianBlur:
        """torchvision's published rule (transforms/_functional_tensor.py: _get_gaussian_kernel1d / 2d, gaussian_blur) for one kernel size and one
        sigma on a float [N][C][H][W] tensor: reflect padding by k // 2, then a k x k correlation per channel."""

        def __init__(self, kernel_size, sigma):
            self.k, self.sigma = int(kernel_size), float(sigma)

        def __call__(self, img):
            k = self.k
            half = (k - 1) * 0.5
            x = torch.linspace(-half, half, steps=k)
            pdf = torch.exp(-0.5 * (x / self.sigma).pow(2))
            k1 = pdf / pdf.sum()
            k2 = torch.mm(k1[:, None], k1[None, :]).to(img.dtype)
            c = img.shape[1]
            padded = torch.nn.functional.pad(img, [k // 2] * 4, mode="reflect")
            return torch.nn.functional.conv2d(padded, k2.expand(c, 1, k, k), groups=c)

    tv, tr = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
    tr.GaussianBlur = GaussianBlur
    tv.transforms = tr
    sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tr


class Patched:
    """the three network calls of a segment replaced; log rows = [pixel height, pixel width, seed]"""

    def __init__(self, cycle_chooser):
        from src.AutoDetailer import ADetailer, bbox
        from src.AutoEncoders import VariationalAE
        self.A, self.B, self.V = ADetailer, bbox, VariationalAE
        self.cycle_chooser, self.log, self.sigmas = cycle_chooser, [], []

    def __enter__(self):
        self.orig = (self.V.VAEEncode.encode, self.A.ksampler_wrapper, self.B.WildcardChooser.get)
        me = self

        def encode(self, vae, pixels, flux=False):
            me.log.append([pixels.shape[1], pixels.shape[2]])
            return ({"samples": pixels},)

        def ksampler_wrapper(model, seed, steps, cfg, sampler_name, scheduler, positive, negative, latent_image, denoise, *a, **k):
            me.log[-1].append(seed)
            return latent_image
        self.V.VAEEncode.encode, self.A.ksampler_wrapper = encode, ksampler_wrapper
        if self.cycle_chooser:
            self.B.WildcardChooser.get = lambda self, seg: self.items[0]        # "return the only item"
        return self

    def __exit__(self, *a):
        self.V.VAEEncode.encode, self.A.ksampler_wrapper, self.B.WildcardChooser.get = self.orig


class TableVAE:
    def __init__(self):
        self.table = torch.from_numpy(D.standin_decode_table())

    def decode(self, samples):
        return self.table[torch.round(samples * 255.0).long()]


def _doit(image, segs, model, vae, positive, negative, **kw):
    from src.AutoDetailer import ADetailer
    a = dict(guide_size_for=False, noise_mask=True, force_inpaint=True, wildcard="", inpaint_model=False, noise_mask_feather=0, pipeline=True)
    a.update(kw)
    with torch.no_grad():
        return ADetailer.DetailerForEachTest().doit(image=image, segs=segs, model=model, clip=None, vae=vae, positive=positive, negative=negative, **a)[0]


def host_functions(g, mp):
    from src.AutoDetailer import AD_util, ADetailer, SEGS
    g["crop_regions"] = np.array([AD_util.make_crop_region(w, h, bbox, f) for w, h, bbox, f in D.CROP_CASES], np.int64)
    sizes = []
    for w, h, guide, mx in D.SIZE_CASES:                 # enhance_detail's sizes, read off the pixels it hands to the encoder
        with Patched(False) as p:
            ADetailer.enhance_detail(torch.zeros(1, h, w, 3), None, None, TableVAE(), guide, False, mx, [0, 0, w, h], 0, 1, 1.0, "euler", "karras", [], [],
                                     1.0, None, True)
        sizes.append([p.log[0][1], p.log[0][0]])
    g["detail_sizes"] = np.array(sizes, np.int64)
    orig = ADetailer.sample_with_custom_noise
    got = []
    ADetailer.sample_with_custom_noise = lambda model, add_noise, seed, cfg, pos, neg, sampler, sigmas, latent, **k: (got.append(sigmas), (latent, latent))[1]
    try:
        for i, (sched, steps, den) in enumerate(D.SIGMA_CASES):
            ADetailer.ksampler_wrapper(mp, 0, steps, 1.0, "dpmpp_2m_cfgpp", sched, [], [], {"samples": torch.zeros(1, 4, 8, 8)}, den)
            g[f"sigmas_{i}"] = got[-1].numpy()
    finally:
        ADetailer.sample_with_custom_noise = orig
    shape, items, full = D.and_mask_case()
    segs = (shape, [SEGS.SEG(None, m, 1.0, region, region, "seg", None) for m, region in items])
    out = SEGS.segs_bitwise_and_mask(segs, torch.from_numpy(full)[None])
    for i, s in enumerate(out[1]):
        g[f"and_mask_{i}"] = s.cropped_mask


def standin_runs(g, meta):
    from src.AutoDetailer import AD_util, SEGS
    import ldx_amd as ldx
    img = D.image(D.STANDIN_IMAGE)
    _, h, w, _ = img.shape
    kw = dict(D.STANDIN)
    table = D.standin_decode_table()
    for name, boxes in D.STANDIN_CASES.items():
        segs = D.make_segs(h, w, boxes, AD_util.make_crop_region, SEGS.SEG)
        with Patched(name != "one") as p:
            out = _doit(torch.from_numpy(img), segs, None, TableVAE(), [], [], **kw)
        g[f"standin_{name}"], g[f"standin_{name}_log"] = out.numpy(), np.array(p.log, np.int64)
        # the package's fp32 statement on the same job: how far its fixed summation order is from torch's conv2d
        log = []
        host = ldx.detailer.detailer_host(img, D.make_segs(h, w, boxes, ldx.detailer.make_crop_region, ldx.SEG), kw["guide_size"], kw["max_size"], kw["seed"],
                                          kw["steps"], kw["cfg"], kw["sampler_name"], kw["scheduler"], None, None, kw["denoise"], kw["feather"], kw["cycle"],
                                          encode=lambda px: (log.append([px.shape[1], px.shape[2]]), px)[1],
                                          sample=lambda lat, seed, *a: (log[-1].append(seed), lat)[1],
                                          decode=lambda lat: table[np.round(lat * np.float32(255.0)).astype(np.int64)])
        d = np.abs(host - out.numpy())
        tol = 128 * 2.0 ** -24
        line = (f"stand-in {name}: crops {[tuple(r[:2][::-1]) for r in p.log]} (w, h at the sample size), seeds {[r[2] for r in p.log]}; detailer_host vs the reference: "
                f"max |difference| {d.max():.3e}, share of values above 128 * 2^-24: {100.0 * (d > tol).mean():.3f} %")
        print(line)
        meta.append(line)
        assert log == p.log, (log, p.log)


def real_runs(g, meta, mp):
    from src.AutoDetailer import AD_util, SEGS
    from src.AutoEncoders import VariationalAE
    import ldx_amd as ldx
    vcfg = ldx.VAEConfig(ch=64)
    vsd = ldx.weights.synth_state_dict(ldx.weights.vae_state_dict_spec(vcfg), seed=4321, dtype=torch.float32)
    enc, dec = VariationalAE.Encoder, VariationalAE.Decoder          # the reference's VAE class only knows ch = 128: narrow its two halves
    VariationalAE.Encoder, VariationalAE.Decoder = (lambda **dd: enc(**dict(dd, ch=64))), (lambda **dd: dec(**dict(dd, ch=64)))
    try:
        vae = VariationalAE.VAE(sd=vsd, device=torch.device("cpu"), dtype=torch.float32)
    finally:
        VariationalAE.Encoder, VariationalAE.Decoder = enc, dec
    assert set(vae.get_sd().keys()) == set(vsd.keys())
    g7 = torch.Generator().manual_seed(7)
    P, N = torch.randn([1, 77, 128], generator=g7), torch.randn([1, 77, 128], generator=g7)
    z = torch.zeros(1, 128)
    g["real_P"], g["real_N"] = P.numpy(), N.numpy()
    img = D.image(D.TINY_IMAGE)
    _, h, w, _ = img.shape

    def run(boxes, **over):
        kw = dict(D.TINY, **over)
        segs = D.make_segs(h, w, boxes, AD_util.make_crop_region, SEGS.SEG)
        torch.manual_seed(11)
        # noise_mask_feather = 20 is the pipeline's value: it must not change a pixel (the package computes nothing for it)
        with PatchedChooser():
            out = _doit(torch.from_numpy(img), segs, mp, vae, [[P, {"pooled_output": z}]], [[N, {"pooled_output": z}]], noise_mask_feather=20, **kw)
        return torch.clamp(torch.round(out[0] * 255.0), 0, 255).to(torch.uint8).numpy()
    base = run(D.TINY_BOXES)
    g["real_out"] = base
    union = D.union_mask(h, w, D.make_segs(h, w, D.TINY_BOXES, AD_util.make_crop_region, SEGS.SEG))
    dist = []
    for name in D.TINY_PERTURBED:
        over, boxes = D.tiny_variant(name)
        r = run(boxes, **over)
        dist.append(np.abs(r.astype(np.int64) - base.astype(np.int64))[union].mean())
    d = np.array(dist)
    line = f"tiny-network wiring distances (mean |byte difference| to the base run over the union of the crop regions): {dict(zip(D.TINY_PERTURBED, d.round(3).tolist()))}"
    print(line)
    meta.append(line)
    # a perturbation the test could not tell from rounding would make the parity bound meaningless
    assert d.min() >= 2.0, d
    g["real_wiring"], g["real_wiring_names"] = d, np.array(D.TINY_PERTURBED)


class PatchedChooser:
    def __enter__(self):
        from src.AutoDetailer import bbox
        self.bbox, self.orig = bbox, bbox.WildcardChooser.get
        bbox.WildcardChooser.get = lambda self, seg: self.items[0]

    def __exit__(self, *a):
        self.bbox.WildcardChooser.get = self.orig


META_HEAD = """tests/golden/detailer.npz: generated by tests/tools/capture_detailer.py from the reference snapshot, torch {torch} on the CPU in fp32.
Stand-in modules installed before importing src.AutoDetailer (the packages are not in the build container):
  cv2                  empty (only the detectors use it);
  ultralytics          YOLO = object (the detector, not run);
  torchvision          transforms.GaussianBlur written out from torchvision's published rule (1-D kernel exp(-0.5 (x / sigma)^2) on linspace, normalised,
                       outer product, reflect padding by k // 2, k x k correlation through torch's conv2d).  The mask feather is therefore pinned to the
                       published rule, not to torchvision's binary.
More than one non-empty segment: the reference's WildcardChooser holds one item and raises IndexError at the second non-empty segment.  The golden "one"
is captured from the unmodified reference; "disjoint", "overlap", "empty" and the tiny-network runs are captured with WildcardChooser.get replaced, in the
capture tool only, by "return the only item".  The package processes every segment.
Stand-in runs: VAEEncode.encode returns the pixels, ksampler_wrapper returns the latent, vae.decode is the byte table 255 - v; image smooth_image{simg},
{standin}.
Tiny-network run: tiny UNet (64, 128) seed 1234, VAE ch = 64 seed 4321, image smooth_image{timg}, boxes {tboxes}, {tiny}, noise_mask_feather = 20,
torch.manual_seed(11) before the call; stored as bytes.
"""


def main():
    sys.path.insert(0, REPO)
    import ldx_amd as ldx
    torch.set_num_threads(8)
    ref_capture.enter_reference()
    path = os.path.join(ref_capture.OUT, "detailer.npz")
    meta_path = os.path.join(ref_capture.OUT, "detailer.META.txt")
    ucfg = ldx.UNetConfig.tiny(64, 128)
    _, mp = ref_capture.build_reference_model(ucfg, ldx.weights.synth_state_dict(ldx.weights.unet_state_dict_spec(ucfg), seed=1234))
    install_standins()               # after the model: transformers, imported on the way, probes for a real torchvision and must not find the stand-in
    g, meta = {}, []
    host_functions(g, mp)
    standin_runs(g, meta)
    old_meta = open(meta_path).read().splitlines() if os.path.exists(meta_path) else []
    if "--skip-real" in sys.argv:
        old = np.load(path)
        g.update({k: old[k] for k in old.files if k.startswith("real_")})
        meta += [ln for ln in old_meta if ln.startswith("tiny-network")]
    else:
        real_runs(g, meta, mp)
    meta += [ln for ln in old_meta if ln.startswith("MI355X")]          # what the GPU tests measured against these goldens, added by hand
    np.savez_compressed(path, **g)
    with open(meta_path, "w") as f:
        f.write(META_HEAD.format(torch=torch.__version__, simg=D.STANDIN_IMAGE, standin=D.STANDIN, timg=D.TINY_IMAGE, tboxes=D.TINY_BOXES, tiny=D.TINY))
        f.write("\n".join(meta) + "\n")
    print("detailer.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
