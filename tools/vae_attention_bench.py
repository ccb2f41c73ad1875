#!/usr/bin/env python
"""Timing of the VAE's mid-block attention, both routes, and of whole decodes at the sizes only the streaming kernel reaches (random
weights, batch 1, operands warm, HIP events; medians of REPS).
usage (from the repository root): tools/vae_attention_bench.py [out.json]
  streaming kernel   sd_op_vae_attention's ms at (1, 4096, 512), (1, 9216, 512), (1, 16384, 512)
  materialised op    the `sd` decoder at 64 x 64 latents, the attention row of its per-op profile (QK^T GEMM + row softmax + PV GEMM)
  whole decodes      sd_vae_decode's launch list at 96 x 96 and 128 x 128 latents (sd_unet_time_forward, HIP events)"""
import json
import sys

sys.path[:0] = [".", "ml-stable-diffusion_amd"]
import numpy as np
from oracle import vae_ref, weights
from python_hip_stable_diffusion import HipVaeDecoder, _lib

REPS = 31
res = {"reps": REPS}
rs = np.random.RandomState(0)
for S in (4096, 9216, 16384):
    q, k, v = (rs.randn(1, S, 512).astype(np.float16) for _ in range(3))
    _lib.vae_attention(q, k, v, iters=3)
    ms = [_lib.vae_attention(q, k, v, iters=4)[1] for _ in range(REPS)]           # each figure: the mean of 4 back-to-back launches
    res["stream_S%d_ms" % S] = float(np.median(ms))
    print("streaming kernel (1, %d, 512): median %.3f ms (min %.3f, max %.3f) = %.0f TFLOP/s" %
          (S, np.median(ms), min(ms), max(ms), 4.0 * S * S * 512 / np.median(ms) * 1e-9), flush=True)

SD = vae_ref.VAE_CONFIGS["sd"]
sd16 = weights.make_state_dict(vae_ref.vae_decoder_param_shapes(SD), seed=61, dtype=np.float16, gain=1.6)
for hw in (64, 96, 128):
    vae = HipVaeDecoder(SD, sd16, batch=1, latent_height=hw, latent_width=hw)
    z = (weights.seeded_normal((1, 4, hw, hw), 62) / 0.18215).astype(np.float16)
    image = vae(z=z)["image"]
    assert np.isfinite(image).all()
    att = []
    for _ in range(REPS if hw == 64 else 5):
        rows = [r for r in vae.profile(iters=1) if r[0].startswith("VAE attention")]
        assert len(rows) == 1, rows
        att.append(rows[0][2])
    total = [vae.time_forward(warmup=1, iters=1) for _ in range(REPS)]
    res["decoder_%dx%d" % (hw, hw)] = {"attention_label": rows[0][0], "attention_op_ms": float(np.median(att)), "decode_ms": float(np.median(total)),
                                       "arena_used_MB": _lib.lib().sd_unet_arena_used_bytes(vae._h) / 2 ** 20}
    print("sd decoder %dx%d latents: whole launch list median %.2f ms | %s: median %.3f ms | arena %.0f MB" %
          (hw, hw, np.median(total), rows[0][0], np.median(att), res["decoder_%dx%d" % (hw, hw)]["arena_used_MB"]), flush=True)
    vae.close()
print(json.dumps(res))
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
