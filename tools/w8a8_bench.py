#!/usr/bin/env python3
"""W8A8 (plan tile 17) against the fp16 weight stream (plan tile 9): the measurements of LAB_NOTES round 23.  One process, one session;
prints one JSON line per measurement.

    python tools/w8a8_bench.py ops      # 1280->1280 and 2560->1280 @8x8 at batch 2: tile 17 vs tile 9, alternating back to back,
                                        # HIP events around --iters launches, median over --rounds rounds
    python tools/w8a8_bench.py handle   # SD2.1-base on random weights, every eligible layer quantized (calibrated on one forward)
                                        # against the fp16 handle: step time with the two handles alternating, sd_unet_device_bytes,
                                        # arena_used_bytes, the per-op times of the quantized layers in both, PSNR of the noise
                                        # prediction against the fp16 handle's

Operator times are back-to-back launches of one conv: its weights stay in the Infinity Cache, so they are ratios between kernels on
hot caches, not step times; the per-op profile of the handles (eager launches in step order) is the figure nearer to the step."""
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


def h16(a):
    return np.asarray(a, np.float32).astype(np.float16)


def med(v):
    return float(np.median(np.asarray(v, np.float64)))


def ops(iters, rounds):
    rs = np.random.RandomState(23)
    for C0, C1 in ((1280, 0), (1280, 1280)):
        ctot, N = C0 + C1, 1280
        x = h16(rs.randn(2, C0, 8, 8))
        x1 = h16(rs.randn(2, C1, 8, 8)) if C1 else None
        w = (rs.randn(N, ctot, 3, 3) / np.sqrt(9 * ctot)).astype(np.float32)
        bias = (0.1 * rs.randn(N)).astype(np.float32)
        wq, ws, _ = _lib.quantize_weight(w)
        absmax = float(max(np.abs(x.astype(np.float32)).max(), np.abs(x1.astype(np.float32)).max() if C1 else 0.0))
        for nw, code in ((8, 9), (4, 49)):
            t9, t17 = [], []
            for _ in range(rounds):                                              # alternating, back to back
                t9.append(_lib.conv2d_ex(x, h16(w), bias, x1=x1, tile=code, iters=iters)[3])
                t17.append(_lib.conv2d_w8a8(x, wq, ws, absmax, bias=bias, x1=x1, nw=nw, iters=iters)[2])
            print(json.dumps({"op": "conv3x3", "shape": f"{ctot}->{N} @8x8 B=2", "waves": nw, "weight_MB_fp16": round(2e-6 * w.size, 1),
                              "weight_MB_int8": round(1e-6 * w.size, 1), "tile9_us_median": round(1e3 * med(t9), 2),
                              "tile17_us_median": round(1e3 * med(t17), 2), "tile9_us_min_max": [round(1e3 * min(t9), 2), round(1e3 * max(t9), 2)],
                              "tile17_us_min_max": [round(1e3 * min(t17), 2), round(1e3 * max(t17), 2)], "rounds": rounds, "iters": iters}), flush=True)


def handle(iters, rounds):
    from oracle import psnr, unet_ref, weights
    cfg = unet_ref.CONFIGS["sd21-base"]
    sd16 = weights.make_state_dict(unet_ref.unet_param_shapes(cfg), seed=21, dtype=np.float16)
    hw = cfg["sample_size"]
    inputs = dict(sample=weights.seeded_normal((2, 4, hw, hw), 1).astype(np.float16), timestep=np.array([981, 981], np.float16),
                  encoder_hidden_states=weights.seeded_normal((2, cfg["cross_attention_dim"], 1, 77), 2).astype(np.float16))
    t0 = time.time()
    obs = HipModel(cfg, sd16, batch=2, observe_activations=True)
    obs(**inputs)
    recipe = aq.recipe_from_ranges(obs.activation_ranges())
    obs.close()
    print(json.dumps({"calibration": "one forward", "layers": len(recipe), "absmax_min_max": [min(recipe.values()), max(recipe.values())],
                      "s": round(time.time() - t0, 1)}), flush=True)
    fp16 = HipModel(cfg, sd16, batch=2)
    w8a8 = HipModel(cfg, sd16, batch=2, activation_quantization=recipe)
    a, b = fp16(**inputs)["noise_pred"], w8a8(**inputs)["noise_pred"]
    steps = {"fp16": [], "w8a8": []}
    for _ in range(rounds):                                                      # the two routes alternating
        steps["fp16"].append(fp16.time_forward(warmup=3, iters=iters))
        steps["w8a8"].append(w8a8.time_forward(warmup=3, iters=iters))
    layers = set(w8a8.w8a8_layers())

    def layer_us(model):
        t = {}
        for lab, _, ms in model.profile(7):
            m = re.search(r" K=\d+ (\S+) #", lab)
            if m and m.group(1) in layers:
                t[m.group(1)] = 1e3 * ms
        return t

    u16, u8 = layer_us(fp16), layer_us(w8a8)
    print(json.dumps({"handle": "sd21-base random weights", "w8a8_info": list(w8a8.w8a8_info()),
                      "step_ms_median": {k: round(med(v), 4) for k, v in steps.items()},
                      "step_ms_all": {k: [round(x, 4) for x in v] for k, v in steps.items()},
                      "device_bytes": {"fp16": fp16.device_bytes, "w8a8": w8a8.device_bytes},
                      "arena_used_bytes": {"fp16": fp16.arena_used_bytes, "w8a8": w8a8.arena_used_bytes},
                      "quantized_layers_profile_us_sum": {"fp16": round(sum(u16.values()), 1), "w8a8": round(sum(u8.values()), 1)},
                      "psnr_db_vs_fp16_handle": round(psnr.compute_psnr(b, a), 2)}), flush=True)
    for name in sorted(layers):
        print(json.dumps({"layer": name, "fp16_us": round(u16.get(name, float("nan")), 2), "w8a8_us": round(u8.get(name, float("nan")), 2)}), flush=True)
    fp16.close()
    w8a8.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["ops", "handle"])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    {"ops": ops, "handle": handle}[a.what](a.iters, a.rounds)
