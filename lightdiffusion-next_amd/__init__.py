"""ldx — MI355X-native engine for LightDiffusion-Next's denoising hot path.

The package directory is named ``lightdiffusion-next_amd`` (not a Python identifier); import it as
``import ldx_amd`` (shim at the repository root) or ``importlib.import_module("lightdiffusion-next_amd")``.

Layout:
  csrc/        hand-written HIP kernels for gfx950 + the C ABI (include/ldx.h) -> libldx.so
  lib.py       ctypes binding of libldx.so (fails loudly if the library or a GPU is missing)
  engine.py    UNetEngine: weights in, denoise out (device pointers through the C ABI)
  hook.py      LdxUNetPatch / LdxFluxPatch: drop-ins for model_options["model_function_wrapper"] (cond.py:254-263); LdxSAMPatch: Sam.image_encoder
  sampling.py  host mirror of src/sample (schedulers, CFG batching, Euler / DPM++ loops, the TAESD preview hook: LatentPreviewer)
  parallel.py  batch shard + single all-gather across the GPUs of a node (RCCL / gloo)
  weights.py   SD1.5 state-dict layout + seeded synthetic weights (no checkpoints offline)
  checkpoint.py  load-time ingestion: checkpoint split, UNet layout sniffing, LoRA key maps + merge
  usdu.py      UltimateSDUpscale: the img2img tile redraw / seam fix, canvas on the device (ldx_image_* kernels -> libldx_image.so)
  hdr.py       AutoHDR: the default post-effect after the VAE (LittleCMS Lab round trip as two 33^3 tables, luminance table, Pillow's contrast / colour
               blends) on device images (ldx_hdr_* kernels -> libldx_hdr.so); autohdr_host is the same in numpy
  png.py       PNGEncoder / SaveImage: the finished PNG file of a device image (row filters, chunked deflate, CRC-32 / Adler-32: ldx_png_* kernels
               -> libldx_png.so) and the reference's file placement around it; png_host is the same in numpy
  gguf.py      GGUF v2 / v3 container reader (F32, F16, BF16, Q8_0): the reference's Flux and T5 files as {key: GGUFTensor}, nothing expanded;
               FluxEngine.from_gguf / T5Engine.from_gguf expand Q8_0 once at load time (ldx_load_tensor_q8_0 -> libldx_q8.so, or the host)
  detailer.py  Detailer: ADetailer's per-segment redraw (crop, LANCZOS, encode, sample, decode, feathered fp32 paste) with the canvas on the device
               (ldx_detail_* kernels -> libldx_detail.so, ldx_image_* for the 8-bit steps); detailer_host is the same in numpy
  sam.py       SAM image encoder, host side: Sam.preprocess, ResizeLongestSide's shape rule and the network in torch (sam_encoder_host / _host16);
               SAMImageEncoderEngine runs it on the device (the shared GEMM / norm kernels + ldx_sam_* kernels -> libldx_sam.so), LdxSAMPatch binds it
               into segment_anything's Sam; the prompt encoder, mask decoder and post-processing likewise (sam_decoder_host, postprocess_host; SAMMaskDecoderEngine
               on the fp32 kernels of libldx_samdec.so), and SAMDetector: SAMDetectorCombined from the device image and the detector's boxes to the mask
"""
from . import lib, weights  # noqa: F401
from .engine import UNetEngine, UNetConfig, VAEDecoderEngine, CLIPTextEngine, FluxEngine, T5Engine, ESRGANEngine, TAESDEngine, SAMImageEncoderEngine, SAMMaskDecoderEngine, bislerp, latent_upscale  # noqa: F401
VAEEngine = VAEDecoderEngine      # the same engine encodes when encoder.* weights are loaded
from .weights import VAEConfig, CLIPConfig, FluxConfig, T5Config, ESRGANConfig, TAESDConfig, SAMConfig, SAMDecoderConfig  # noqa: F401
from .hook import LdxUNetPatch, LdxFluxPatch, LdxSAMPatch  # noqa: F401
from .sam import SAMDetector  # noqa: F401
from . import prompt  # noqa: F401
from . import sampling, parallel, checkpoint, usdu, hdr, png, detailer, gguf, sam  # noqa: F401
from .detailer import Detailer, SEG  # noqa: F401
from .sampling import LatentPreviewer  # noqa: F401
from .usdu import UltimateSDUpscale  # noqa: F401
from .hdr import AutoHDR  # noqa: F401
from .png import PNGEncoder, SaveImage  # noqa: F401
