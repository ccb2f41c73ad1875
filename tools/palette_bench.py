#!/usr/bin/env python3
"""Times of the kernels that read palettized weights against the fp16 kernels they mirror, and of an SD2.1-base handle with and without
palettes - the measurements LAB_NOTES rounds 15, 16 and 20 ask for.  One process, one session; prints one JSON line per measurement.

    python tools/palette_bench.py ops              # operator times: tile 16 vs 13, 15 vs 12, 14 vs 9 (HIP events, --iters launches)
    python tools/palette_bench.py handle           # arena_used_bytes and sd_unet_time_forward, fp16 against quantize_nbits=6

Operator times are back-to-back launches on hot caches: ratios between kernels, not step times."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ml-stable-diffusion_amd")]

from python_hip_stable_diffusion import HipModel, _lib  # noqa: E402


def h16(a):
    return np.asarray(a, np.float32).astype(np.float16)


def palette(rs, nbits, k, shape):
    lut = np.sort(h16(rs.randn(1 << nbits) / np.sqrt(k)))
    return lut, rs.randint(0, 1 << nbits, size=shape).astype(np.uint8)


def ops(iters):
    rs = np.random.RandomState(7)
    print(json.dumps({"calibration": _lib.calibrate() if hasattr(_lib, "calibrate") else None}))
    for M, K, N2 in ((512, 1280, 10240), (2048, 640, 5120)):           # ff.net.0.proj of SD2.1-base at CFG batch 2
        x = h16(rs.randn(M, K) + 0.5)
        g, b, bias = (1 + 0.2 * rs.randn(K)).astype(np.float32), (0.1 * rs.randn(K)).astype(np.float32), (0.1 * rs.randn(N2)).astype(np.float32)
        for nbits in (4, 6, 8):
            lut, idx = palette(rs, nbits, K, (N2, K))
            _, ms13 = _lib.geglu_ln(x, lut[idx], bias, g, b, kernel=100, iters=iters)
            rec = {"op": "geglu", "M": M, "K": K, "N2": N2, "bits": nbits, "tile13_us": round(1e3 * ms13, 2)}
            try:
                _, _, ms16 = _lib.geglu_palettized(x, lut, idx, nbits, bias=bias, ln_weight=g, ln_bias=b, iters=iters)
                rec["tile16_us"] = round(1e3 * ms16, 2)
            except ValueError:
                rec["tile16_us"] = None                                  # 256-row tiles: not built
            print(json.dumps(rec), flush=True)
    for B, HW, C in ((2, 16, 1280), (2, 32, 640)):                       # proj_in / to_out.0
        x = h16(rs.randn(B, C, HW, HW))
        bias = (0.1 * rs.randn(C)).astype(np.float32)
        for nbits in (4, 6, 8):
            lut, idx = palette(rs, nbits, C, (C, C))
            _, ms12 = _lib.conv2d(x, lut[idx][..., None, None], bias, tile=140, iters=iters)
            _, _, ms15 = _lib.gemm_palettized(x, lut, idx, nbits, bias=bias, iters=iters)
            print(json.dumps({"op": "gemm1x1", "M": B * HW * HW, "K": C, "N": C, "bits": nbits, "tile12_us": round(1e3 * ms12, 2),
                              "tile15_us": round(1e3 * ms15, 2)}), flush=True)
    x = h16(rs.randn(2, 1280, 8, 8))                                     # 3x3 conv of the 8x8 level
    bias = (0.1 * rs.randn(1280)).astype(np.float32)
    for nbits in (4, 6, 8):
        lut, idx = palette(rs, nbits, 9 * 1280, (1280, 1280, 3, 3))
        _, _, _, ms9 = _lib.conv2d_ex(x, lut[idx], bias, tile=9, iters=iters)
        _, _, ms14 = _lib.conv2d_palettized(x, lut, idx, nbits, bias=bias, iters=iters)
        print(json.dumps({"op": "conv3x3", "M": 128, "K": 9 * 1280, "N": 1280, "bits": nbits, "tile9_us": round(1e3 * ms9, 2),
                          "tile14_us": round(1e3 * ms14, 2)}), flush=True)


def handle(iters):
    from oracle import unet_ref, weights
    cfg = unet_ref.CONFIGS["sd21-base"]
    sd16 = weights.make_state_dict(unet_ref.unet_param_shapes(cfg), seed=21, dtype=np.float16)
    hw = cfg["sample_size"]
    inputs = dict(sample=weights.seeded_normal((2, 4, hw, hw), 1).astype(np.float16), timestep=np.array([981, 981], np.float16),
                  encoder_hidden_states=weights.seeded_normal((2, cfg["cross_attention_dim"], 1, 77), 2).astype(np.float16))
    for q in (None, 6):
        t0 = time.time()
        m = HipModel(cfg, sd16, batch=2, quantize_nbits=q)
        m(**inputs)
        ms = [m.time_forward(warmup=3, iters=iters) for _ in range(3)]
        print(json.dumps({"handle": "sd21-base", "quantize_nbits": q, "arena_used_bytes": m.arena_used_bytes, "palette_info": list(m.palette_info()),
                          "step_ms": [round(v, 4) for v in ms], "build_s": round(time.time() - t0, 1)}), flush=True)
        m.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["ops", "handle"])
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    {"ops": ops, "handle": handle}[a.what](a.iters)
