#!/usr/bin/env python
"""Latents -> 8-bit image + safety verdict, on the host route (sd_vae_decode -> numpy -> PIL -> CLIPImageProcessor -> upload ->
sd_safety_checker_run: the pipeline without device_postprocess) and on the device route (sd_vae_decode_images), at SD2.1-base's decoder
(64 x 64 latents, 512 x 512 images) with the full ViT-L/14 checker, random weights.  Wall time per call in one session, both routes
interleaved, plus the two kernels' HIP-event time as operators.
usage (from the repository root): tools/image_post_bench.py [calls]      prints one JSON line"""
import json
import sys
import time

sys.path[:0] = [".", "ml-stable-diffusion_amd", "tests"]
import numpy as np

from oracle import vae_ref, weights
from python_hip_stable_diffusion import HipSafetyChecker, HipVaeDecoder, _lib, pipeline as P, safety_checker as sc
from test_safety_checker import CONFIGS, make_checkpoint

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 20
from transformers import CLIPImageProcessor

fe = CLIPImageProcessor(size={"shortest_edge": 224}, crop_size={"height": 224, "width": 224})
vcfg = vae_ref.VAE_CONFIGS["sd"]
vae = HipVaeDecoder(vcfg, weights.make_state_dict(vae_ref.vae_decoder_param_shapes(vcfg), seed=61, dtype=np.float16), batch=1,
                    latent_height=64, latent_width=64)
ccfg = dict(CONFIGS["vit-l-2"], num_hidden_layers=24)
ckpt = make_checkpoint(ccfg, seed=3)
ckpt["concept_embeds_weights"][:] = 2.0          # nothing fires: neither route zeroes an image
ckpt["special_care_embeds_weights"][:] = 2.0
chk = HipSafetyChecker(ccfg, ckpt, batch=1)
post = sc.image_post(fe, 512, 512, 224)
z = weights.seeded_normal((1, 4, 64, 64), 9).astype(np.float16)
numpy_to_pil = P.HipStableDiffusionPipeline.numpy_to_pil


def host(parts=None):
    t0 = time.perf_counter()
    image = vae(z=z)["image"]
    t1 = time.perf_counter()
    image = np.clip(image / 2 + 0.5, 0, 1).transpose((0, 2, 3, 1))                                  # decode_latents
    pil = numpy_to_pil(image)
    clip_input = fe(pil, return_tensors="np").pixel_values.astype(np.float16)                      # run_safety_checker
    t2 = time.perf_counter()
    flags, scores, _ = chk.run(clip_input)
    t3 = time.perf_counter()
    if parts is not None:
        parts.append((t1 - t0, t2 - t1, t3 - t2))
    return pil, flags, scores


def device():
    out = vae.decode_images(z, chk, post, want_image=False)
    from PIL import Image
    return [Image.fromarray(im) for im in out["rgb8"]], out["has_nsfw_concepts"], out["concept_scores"]


for _ in range(3):
    a, b = host(), device()
assert np.array_equal(np.asarray(a[0][0]), np.asarray(b[0][0])) and np.array_equal(a[2], b[2]), "the two routes disagree"
wall = {"host": [], "device": []}
parts = []
for _ in range(calls):
    t = time.perf_counter(); host(parts); wall["host"].append((time.perf_counter() - t) * 1e3)
    t = time.perf_counter(); device(); wall["device"].append((time.perf_counter() - t) * 1e3)
image = vae(z=z)["image"]
rgb8, ms_rgb8 = _lib.image_rgb8(image, iters=200)
_, ms_clip = _lib.clip_input(rgb8, 224, 224, 224, post.image_mean, post.image_std, iters=200)
_, ms_clip4 = _lib.clip_input(np.repeat(rgb8, 4, axis=0), 224, 224, 224, post.image_mean, post.image_std, iters=200)
parts = np.array(parts) * 1e3
print(json.dumps({
    "calls": calls,
    "host_wall_ms": {"median": round(float(np.median(wall["host"])), 3), "min": round(min(wall["host"]), 3)},
    "device_wall_ms": {"median": round(float(np.median(wall["device"])), 3), "min": round(min(wall["device"]), 3)},
    "host_parts_ms_median": {"sd_vae_decode": round(float(np.median(parts[:, 0])), 3),
                             "numpy_pil_clip_image_processor": round(float(np.median(parts[:, 1])), 3),
                             "sd_safety_checker_run": round(float(np.median(parts[:, 2])), 3)},
    "vae_forward_ms": round(vae.time_forward(), 3), "checker_last_ms": round(chk.last_ms(), 3),
    "image_rgb8_kernel_us": round(ms_rgb8 * 1e3, 2), "clip_input_kernel_us": round(ms_clip * 1e3, 2),
    "clip_input_kernel_batch4_us": round(ms_clip4 * 1e3, 2)}))
vae.close(), chk.close()
