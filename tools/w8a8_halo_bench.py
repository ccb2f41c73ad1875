#!/usr/bin/env python3
"""The W8A8 halo conv (plan tile 18) against the fp16 halo conv (plan tile 7): the measurements of LAB_NOTES round 25.  One process, one
session; prints one JSON line per measurement.

    python tools/w8a8_halo_bench.py ops      # the 3x3 / stride-1 shapes of SD2.1-base at CFG batch 2 above the 8x8 level: tile 18 vs
                                             # tile 7 on the library's plan codes for the shape (ring, split-K), alternating back to
                                             # back, HIP events around --iters launches, median and range over --rounds rounds
    python tools/w8a8_halo_bench.py handle   # SD2.1-base on random weights, calibrated on one forward: the fp16 handle, the handle with
                                             # the weight-stream layers alone (plan tile 17) and the handle with every eligible layer
                                             # (tiles 17 + 18), alternating: step time, sd_unet_device_bytes, arena_used_bytes, applied
                                             # layers per kernel, PSNR of the noise prediction against the fp16 handle's

Operator times are back-to-back launches of one conv on hot caches: ratios between kernels, not step times."""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ml-stable-diffusion_amd")]

from python_hip_stable_diffusion import HipModel, _lib, activation_quantization as aq  # noqa: E402

# (C0, C1, Cout, H, W of the source, upsample)
OP_SHAPES = [(1280, 0, 1280, 16, 16, False), (1280, 1280, 1280, 16, 16, False), (1280, 0, 1280, 8, 8, True), (640, 0, 640, 32, 32, False),
             (640, 640, 640, 32, 32, False), (320, 0, 320, 64, 64, False)]


def h16(a):
    return np.asarray(a, np.float32).astype(np.float16)


def med(v):
    return float(np.median(np.asarray(v, np.float64)))


def ops(iters, rounds):
    rs = np.random.RandomState(25)
    for C0, C1, N, H, W, ups in OP_SHAPES:
        ctot, up = C0 + C1, 2 if ups else 1
        x = h16(rs.randn(2, C0, H, W))
        x1 = h16(rs.randn(2, C1, H, W)) if C1 else None
        w = (rs.randn(N, ctot, 3, 3) / np.sqrt(9 * ctot)).astype(np.float32)
        bias = (0.1 * rs.randn(N)).astype(np.float32)
        wq, ws, _ = _lib.quantize_weight(w)
        absmax = float(max(np.abs(x.astype(np.float32)).max(), np.abs(x1.astype(np.float32)).max() if C1 else 0.0))
        lib_plan = _lib.conv_plan(3, 1, up, C0, C1, N, 2, H * up, W * up, flags=16)
        forced = lib_plan["tile"] != 7                                            # (a shape whose own plan is another kernel: tile 7's default ring)
        p7 = _lib.conv_plan(3, 1, up, C0, C1, N, 2, H * up, W * up, flags=16, tile=7, staging=3) if forced else lib_plan
        t7, t18 = [], []
        for _ in range(rounds):                                                  # alternating, back to back
            t7.append(_lib.conv2d_ex(x, h16(w), bias, x1=x1, upsample=ups, tile=10 * p7["staging"] + 7, splitk=p7["splitk"], iters=iters)[3])
            t18.append(_lib.conv2d_w8a8_halo(x, wq, ws, absmax, bias=bias, x1=x1, upsample=ups, staging=p7["staging"], splitk=p7["splitk"], iters=iters)[2])
        p18 = _lib.conv_plan(3, 1, up, C0, C1, N, 2, H * up, W * up, flags=16, tile=18, staging=p7["staging"], splitk=p7["splitk"])
        print(json.dumps({"op": "conv3x3", "shape": f"{ctot}->{N} @{H * up}x{W * up} B=2" + (" x2 upsample" if ups else ""),
                          "library_plan_is_tile7": not forced, "tile7_kernel": p7["kernel"], "tile18_kernel": p18["kernel"], "splitk": p7["splitk"],
                          "weight_MB_fp16": round(2e-6 * w.size, 1), "weight_MB_int8": round(1e-6 * w.size, 1),
                          "tile7_us_median": round(1e3 * med(t7), 2), "tile18_us_median": round(1e3 * med(t18), 2),
                          "tile18_over_tile7": round(med(t18) / med(t7), 3),
                          "tile7_us_min_max": [round(1e3 * min(t7), 2), round(1e3 * max(t7), 2)],
                          "tile18_us_min_max": [round(1e3 * min(t18), 2), round(1e3 * max(t18), 2)], "rounds": rounds, "iters": iters}), flush=True)


def handle(iters, rounds):
    from oracle import psnr, unet_ref, weights
    cfg = unet_ref.CONFIGS["sd21-base"]
    sd16 = weights.make_state_dict(unet_ref.unet_param_shapes(cfg), seed=21, dtype=np.float16)
    hw = cfg["sample_size"]
    inputs = dict(sample=weights.seeded_normal((2, 4, hw, hw), 1).astype(np.float16), timestep=np.array([981, 981], np.float16),
                  encoder_hidden_states=weights.seeded_normal((2, cfg["cross_attention_dim"], 1, 77), 2).astype(np.float16))
    t0 = time.time()
    recipes = {}
    for scope, level in (("stream", True), ("all", "all")):
        obs = HipModel(cfg, sd16, batch=2, observe_activations=level)
        obs(**inputs)
        recipes[scope] = aq.recipe_from_ranges(obs.activation_ranges())
        obs.close()
    halo_layers = set(recipes["all"]) - set(recipes["stream"])
    halo_weights = sum(int(np.prod(sd16[k + ".weight"].shape)) for k in halo_layers)
    print(json.dumps({"calibration": "one forward per scope", "layers": {k: len(v) for k, v in recipes.items()},
                      "halo_layers_fp16_weight_MB": round(2e-6 * halo_weights, 1), "s": round(time.time() - t0, 1)}), flush=True)
    models = {"fp16": HipModel(cfg, sd16, batch=2), "stream": HipModel(cfg, sd16, batch=2, activation_quantization=recipes["stream"]),
              "all": HipModel(cfg, sd16, batch=2, activation_quantization=recipes["all"])}
    outs = {k: m(**inputs)["noise_pred"] for k, m in models.items()}
    steps = {k: [] for k in models}
    for _ in range(rounds):                                                      # the three handles alternating
        for k, m in models.items():
            steps[k].append(m.time_forward(warmup=3, iters=iters))

    def layer_us(model, layers):
        t = {}
        for lab, _, ms in model.profile(7):
            m = re.search(r" K=\d+ (\S+) #", lab)
            if m and m.group(1) in layers:
                t[m.group(1)] = 1e3 * ms
        return t

    u = {k: layer_us(m, halo_layers) for k, m in models.items()}
    print(json.dumps({"handle": "sd21-base random weights", "w8a8_info": {k: list(m.w8a8_info()) for k, m in models.items()},
                      "applied_per_kernel": {"tile17": len(recipes["stream"]), "tile18": len(set(models["all"].w8a8_layers()) - set(recipes["stream"]))},
                      "step_ms_median": {k: round(med(v), 4) for k, v in steps.items()},
                      "step_ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in steps.items()},
                      "device_bytes": {k: m.device_bytes for k, m in models.items()},
                      "arena_used_bytes": {k: m.arena_used_bytes for k, m in models.items()},
                      "halo_layers_profile_us_sum": {k: round(sum(v.values()), 1) for k, v in u.items()},
                      "psnr_db_vs_fp16_handle": {k: round(psnr.compute_psnr(outs[k], outs["fp16"]), 2) for k in ("stream", "all")}}), flush=True)
    for name in sorted(halo_layers):
        print(json.dumps({"layer": name, "fp16_us": round(u["fp16"].get(name, float("nan")), 2), "w8a8_us": round(u["all"].get(name, float("nan")), 2)}), flush=True)
    for m in models.values():
        m.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["ops", "handle"])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    {"ops": ops, "handle": handle}[a.what](a.iters, a.rounds)
