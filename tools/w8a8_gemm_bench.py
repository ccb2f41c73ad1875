#!/usr/bin/env python3
"""The W8A8 small-M 1x1 GEMM (plan tile 19) against the fp16 small-M GEMM (plan tile 12): the measurements of LAB_NOTES round 26.  One
process, one session; prints one JSON line per measurement.

    python tools/w8a8_gemm_bench.py box      # the box's calibration figures (cold_code_us among them)
    python tools/w8a8_gemm_bench.py ops      # the two plain projection shapes of SD2.1-base at CFG batch 2 (1280 -> 1280 at M = 512,
                                             # 640 -> 640 at M = 2048, bias + residual): tile 19 vs tile 12 on the same tile height,
                                             # alternating back to back, HIP events around --iters launches, median and range over
                                             # --rounds rounds
    python tools/w8a8_gemm_bench.py handle   # SD2.1-base on random weights, calibrated on one forward: the fp16 handle, the handle with
                                             # every eligible conv (plan tiles 17 + 18) and the handle with the projections added (tile
                                             # 19), alternating: step time, sd_unet_device_bytes, arena_used_bytes, applied layers, PSNR
                                             # of the noise prediction against the fp16 handle's

Operator times are back-to-back launches of one GEMM on hot caches: ratios between kernels, not step times."""
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

# (K, N, H, W) at B = 2
OP_SHAPES = [(1280, 1280, 16, 16), (640, 640, 32, 32)]


def h16(a):
    return np.asarray(a, np.float32).astype(np.float16)


def med(v):
    return float(np.median(np.asarray(v, np.float64)))


def box(iters, rounds):
    print(json.dumps({"calibration": _lib.calibrate(0)}), flush=True)


def ops(iters, rounds):
    rs = np.random.RandomState(26)
    for K, N, H, W in OP_SHAPES:
        x = h16(rs.randn(2, K, H, W))
        w = (rs.randn(N, K) / np.sqrt(K)).astype(np.float32)
        bias = (0.1 * rs.randn(N)).astype(np.float32)
        res = h16(rs.randn(2, N, H, W))
        wq, ws, _ = _lib.quantize_weight(w)
        absmax = float(np.abs(x.astype(np.float32)).max())
        p12 = _lib.conv_plan(1, 1, 1, K, 0, N, 2, H, W, flags=4 | 16)
        assert p12["tile"] == 12, p12
        bm = int(p12["kernel"].split("bm")[1])
        t12, t19 = [], []
        for _ in range(rounds):                                                  # alternating, back to back
            t12.append(_lib.conv2d(x, h16(w)[..., None, None], bias, res, tile=141 if bm == 32 else 142, iters=iters)[1])
            t19.append(_lib.gemm_w8a8(x, wq, ws, absmax, bias=bias, res=res, bm=bm, iters=iters)[2])
        p19 = _lib.conv_plan(1, 1, 1, K, 0, N, 2, H, W, flags=4 | 16, tile=19)
        print(json.dumps({"op": "gemm1x1", "shape": f"{K}->{N} M={2 * H * W}", "tile12_kernel": p12["kernel"], "tile19_kernel": p19["kernel"],
                          "weight_MB_fp16": round(2e-6 * w.size, 2), "weight_MB_int8": round(1e-6 * w.size, 2),
                          "tile12_us_median": round(1e3 * med(t12), 2), "tile19_us_median": round(1e3 * med(t19), 2),
                          "tile19_over_tile12": round(med(t19) / med(t12), 3),
                          "tile12_us_min_max": [round(1e3 * min(t12), 2), round(1e3 * max(t12), 2)],
                          "tile19_us_min_max": [round(1e3 * min(t19), 2), round(1e3 * max(t19), 2)], "rounds": rounds, "iters": iters}), flush=True)


def handle(iters, rounds):
    from oracle import psnr, unet_ref, weights
    cfg = unet_ref.CONFIGS["sd21-base"]
    sd16 = weights.make_state_dict(unet_ref.unet_param_shapes(cfg), seed=21, dtype=np.float16)
    hw = cfg["sample_size"]
    inputs = dict(sample=weights.seeded_normal((2, 4, hw, hw), 1).astype(np.float16), timestep=np.array([981, 981], np.float16),
                  encoder_hidden_states=weights.seeded_normal((2, cfg["cross_attention_dim"], 1, 77), 2).astype(np.float16))
    t0 = time.time()
    recipes = {}
    for scope in ("all", "gemm"):
        obs = HipModel(cfg, sd16, batch=2, observe_activations=scope)
        obs(**inputs)
        recipes[scope] = aq.recipe_from_ranges(obs.activation_ranges())
        obs.close()
    gemm_layers = set(recipes["gemm"]) - set(recipes["all"])
    gemm_weights = sum(int(np.prod(sd16[k + ".weight"].shape)) for k in gemm_layers)
    print(json.dumps({"calibration": "one forward per scope", "layers": {k: len(v) for k, v in recipes.items()},
                      "gemm_layers_fp16_weight_MB": round(2e-6 * gemm_weights, 1), "s": round(time.time() - t0, 1)}), flush=True)
    models = {"fp16": HipModel(cfg, sd16, batch=2), "all": HipModel(cfg, sd16, batch=2, activation_quantization=recipes["all"]),
              "gemm": HipModel(cfg, sd16, batch=2, activation_quantization=recipes["gemm"])}
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

    u = {k: layer_us(m, gemm_layers) for k, m in models.items()}
    print(json.dumps({"handle": "sd21-base random weights", "w8a8_info": {k: list(m.w8a8_info()) for k, m in models.items()},
                      "applied_tile19": len(set(models["gemm"].w8a8_layers()) - set(recipes["all"])),
                      "step_ms_median": {k: round(med(v), 4) for k, v in steps.items()},
                      "step_ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in steps.items()},
                      "device_bytes": {k: m.device_bytes for k, m in models.items()},
                      "arena_used_bytes": {k: m.arena_used_bytes for k, m in models.items()},
                      "gemm_layers_profile_us_sum": {k: round(sum(v.values()), 1) for k, v in u.items()},
                      "psnr_db_vs_fp16_handle": {k: round(psnr.compute_psnr(outs[k], outs["fp16"]), 2) for k in ("all", "gemm")}}), flush=True)
    for m in models.values():
        m.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["box", "ops", "handle"])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    {"box": box, "ops": ops, "handle": handle}[a.what](a.iters, a.rounds)
