#!/usr/bin/env python3
"""The W8A8 GEGLU projection (plan tile 20) and the LayerNorm that writes its int8 activations against the fp16 GEGLU with the LayerNorm
folded in (plan tile 13): the measurements of LAB_NOTES round 27.  One process, one session; prints one JSON line per measurement.

    python tools/w8a8_geglu_bench.py box      # the box's calibration figures (cold_code_us among them)
    python tools/w8a8_geglu_bench.py ops      # the two GEGLU shapes of SD2.1-base at CFG batch 2 (1280 -> 10240 at M = 512, 640 -> 5120
                                              # at M = 2048): tile 13 with the fold (the one launch being replaced), tile 20 alone and
                                              # layernorm_q8, alternating, HIP events around --iters launches, median and range over
                                              # --rounds rounds.  The pair's figure is the SUM of the two separately timed launches
    python tools/w8a8_geglu_bench.py handle   # SD2.1-base on random weights, calibrated on one forward per scope: the fp16 handle, the
                                              # handle with every eligible conv (plan tiles 17 + 18), that one with the GEGLUs added
                                              # (tile 20) and the handle with every layer (tiles 17 - 20), alternating: step time,
                                              # sd_unet_device_bytes, arena_used_bytes, applied layers, PSNR of the noise prediction
                                              # against the fp16 handle's

Operator times are back-to-back launches of one kernel on hot caches: ratios between kernels, not step times."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ml-stable-diffusion_amd")]

from python_hip_stable_diffusion import HipModel, _lib, activation_quantization as aq  # noqa: E402

# (M, K, N2) at CFG batch 2
OP_SHAPES = [(512, 1280, 10240), (2048, 640, 5120)]


def h16(a):
    return np.asarray(a, np.float32).astype(np.float16)


def med(v):
    return float(np.median(np.asarray(v, np.float64)))


def box(iters, rounds):
    print(json.dumps({"calibration": _lib.calibrate(0)}), flush=True)


def ops(iters, rounds):
    rs = np.random.RandomState(27)
    for M, K, N2 in OP_SHAPES:
        x = h16(rs.randn(M, K) * (1.0 + rs.rand(M, 1)) + 0.5)
        w = (rs.randn(N2, K) / np.sqrt(K)).astype(np.float32)
        bias = (0.1 * rs.randn(N2)).astype(np.float32)
        ln_w, ln_b = (1.0 + 0.2 * rs.randn(K)).astype(np.float32), (0.1 * rs.randn(K)).astype(np.float32)
        wq, ws, _ = _lib.quantize_weight(w)
        hw = M // 2
        p13 = _lib.conv_plan(1, 1, 1, K, 0, N2, 2, 1, hw, out_mode=2, flags=1 | 16)
        assert p13["tile"] == 13, p13
        bm = int(p13["kernel"].split("bm")[1])
        xq, _ = _lib.layernorm_q8(x, ln_w, ln_b, 6.0)
        t13, t20, tln = [], [], []
        for _ in range(rounds):                                                  # alternating, back to back
            t13.append(_lib.geglu_ln(x, h16(w), bias=bias, ln_weight=ln_w, ln_bias=ln_b, kernel=101 if bm == 128 else 102, iters=iters)[1])
            t20.append(_lib.geglu_w8a8(xq, wq, ws, 6.0, bias=bias, bm=bm, iters=iters)[2])
            tln.append(_lib.layernorm_q8(x, ln_w, ln_b, 6.0, iters=iters)[1])
        p20 = _lib.conv_plan(1, 1, 1, K, 0, N2, 2, 1, hw, out_mode=2, flags=16, tile=20)
        pair = [a + b for a, b in zip(t20, tln)]
        print(json.dumps({"op": "geglu", "shape": f"{K}->{N2} M={M}", "tile13_kernel": p13["kernel"], "tile20_kernel": p20["kernel"],
                          "weight_MB_fp16": round(2e-6 * w.size, 2), "weight_MB_int8": round(1e-6 * w.size, 2),
                          "tile13_folded_us_median": round(1e3 * med(t13), 2), "tile20_us_median": round(1e3 * med(t20), 2),
                          "layernorm_q8_us_median": round(1e3 * med(tln), 2), "pair_us_median": round(1e3 * med(pair), 2),
                          "tile20_over_tile13": round(med(t20) / med(t13), 3), "pair_over_tile13": round(med(pair) / med(t13), 3),
                          "tile13_us_min_max": [round(1e3 * min(t13), 2), round(1e3 * max(t13), 2)],
                          "tile20_us_min_max": [round(1e3 * min(t20), 2), round(1e3 * max(t20), 2)],
                          "layernorm_q8_us_min_max": [round(1e3 * min(tln), 2), round(1e3 * max(tln), 2)], "rounds": rounds, "iters": iters}), flush=True)


def handle(iters, rounds):
    from oracle import psnr, unet_ref, weights
    cfg = unet_ref.CONFIGS["sd21-base"]
    sd16 = weights.make_state_dict(unet_ref.unet_param_shapes(cfg), seed=21, dtype=np.float16)
    hw = cfg["sample_size"]
    inputs = dict(sample=weights.seeded_normal((2, 4, hw, hw), 1).astype(np.float16), timestep=np.array([981, 981], np.float16),
                  encoder_hidden_states=weights.seeded_normal((2, cfg["cross_attention_dim"], 1, 77), 2).astype(np.float16))
    t0 = time.time()
    ranges = {}
    for scope in ("all", "gemm", "geglu"):
        obs = HipModel(cfg, sd16, batch=2, observe_activations=scope)
        obs(**inputs)
        ranges[scope] = aq.recipe_from_ranges(obs.activation_ranges())
        obs.close()
    geglus = {k: v for k, v in ranges["geglu"].items() if k not in ranges["gemm"]}
    recipes = {"convs": ranges["all"], "convs+geglus": dict(ranges["all"], **geglus), "every layer": ranges["geglu"]}
    geglu_weights = sum(int(np.prod(sd16[k + ".weight"].shape)) for k in geglus)
    print(json.dumps({"calibration": "one forward per scope", "layers": {k: len(v) for k, v in recipes.items()}, "geglu_layers": len(geglus),
                      "geglu_layers_fp16_weight_MB": round(2e-6 * geglu_weights, 1), "s": round(time.time() - t0, 1)}), flush=True)
    models = {"fp16": HipModel(cfg, sd16, batch=2)}
    for k, r in recipes.items():
        models[k] = HipModel(cfg, sd16, batch=2, activation_quantization=r)
    outs = {k: m(**inputs)["noise_pred"] for k, m in models.items()}
    steps = {k: [] for k in models}
    for _ in range(rounds):                                                      # the handles alternating
        for k, m in models.items():
            steps[k].append(m.time_forward(warmup=3, iters=iters))
    print(json.dumps({"handle": "sd21-base random weights", "w8a8_info": {k: list(m.w8a8_info()) for k, m in models.items()},
                      "applied_tile20": len(set(models["every layer"].w8a8_layers()) & set(geglus)),
                      "step_ms_median": {k: round(med(v), 4) for k, v in steps.items()},
                      "step_ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in steps.items()},
                      "device_bytes": {k: m.device_bytes for k, m in models.items()},
                      "arena_used_bytes": {k: m.arena_used_bytes for k, m in models.items()},
                      "psnr_db_vs_fp16_handle": {k: round(psnr.compute_psnr(outs[k], outs["fp16"]), 2) for k in recipes}}), flush=True)
    for m in models.values():
        m.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["box", "ops", "handle"])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    {"box": box, "ops": ops, "handle": handle}[a.what](a.iters, a.rounds)
