#!/usr/bin/env python3
"""The W8A8 self-attention q|k|v projection (plan tile 22) and the LayerNorm that writes its int8 activations against the fp16 fused
q|k|v launch with the LayerNorm folded in: the measurements of LAB_NOTES round 29.  One process, one session; prints one JSON line per
measurement.

    python tools/w8a8_qkv_bench.py box      # the box's calibration figures (cold_code_us among them)
    python tools/w8a8_qkv_bench.py ops      # the two q|k|v shapes of SD2.1-base at CFG batch 2 (640 -> 1920 at M = 2048, 1280 -> 3840 at
                                            # M = 512): the folded fp16 launch by the library's plan (the one launch being replaced), tile
                                            # 22 alone and layernorm_q8, alternating, HIP events around --iters launches, median and
                                            # range over --rounds rounds.  The pair's figure is the SUM of the two separately timed launches
    python tools/w8a8_qkv_bench.py handle   # SD2.1-base on random weights, calibrated on one forward per scope: the fp16 handle, the
                                            # handle with every layer of the geglu scope (plan tiles 17 - 20) and that one with the ten
                                            # q|k|v launches added (tile 22), alternating: step time, sd_unet_device_bytes,
                                            # arena_used_bytes, applied layers, PSNR of the noise prediction against the fp16 handle's

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

# (B, HW, C) at CFG batch 2
OP_SHAPES = [(2, 1024, 640), (2, 256, 1280)]
Q_PRE = float(np.float32(1.4426950408889634) / np.float32(8.0))                  # attention_q_prescale(64)
PARTS = ("attn1.to_q", "attn1.to_k", "attn1.to_v")


def h16(a):
    return np.asarray(a, np.float32).astype(np.float16)


def med(v):
    return float(np.median(np.asarray(v, np.float64)))


def box(iters, rounds):
    print(json.dumps({"calibration": _lib.calibrate(0)}), flush=True)


def ops(iters, rounds):
    rs = np.random.RandomState(29)
    for B, HW, C in OP_SHAPES:
        M = B * HW
        x = h16(rs.randn(M, C) * (1.0 + rs.rand(M, 1)) + 0.5)
        w = (rs.randn(3 * C, C) / np.sqrt(C)).astype(np.float32)
        ln_w, ln_b = (1.0 + 0.2 * rs.randn(C)).astype(np.float32), (0.1 * rs.randn(C)).astype(np.float32)
        wq, ws, _ = _lib.quantize_weight(w)
        side = int(round(HW ** 0.5))
        p16 = _lib.conv_plan(1, 1, 1, C, 0, 3 * C, B, side, side, flags=1 | 16, n_trans=2 * C)
        p22 = _lib.conv_plan(1, 1, 1, C, 0, 3 * C, B, side, side, n_trans=2 * C, tile=22)
        xq, _ = _lib.layernorm_q8(x, ln_w, ln_b, 6.0)
        t16, t22, tln = [], [], []
        for _ in range(rounds):                                                  # alternating, back to back
            t16.append(_lib.qkv_ln(x, ln_w, ln_b, h16(w), B, q_scale=Q_PRE, vt_perm=True, iters=iters)[2])
            t22.append(_lib.qkv_w8a8(xq, wq, ws, 6.0, B, q_scale=Q_PRE, vt_perm=True, iters=iters)[3])
            tln.append(_lib.layernorm_q8(x, ln_w, ln_b, 6.0, iters=iters)[1])
        pair = [a + b for a, b in zip(t22, tln)]
        print(json.dumps({"op": "qkv", "shape": f"{C}->{3 * C} M={M}", "fp16_kernel": p16["kernel"], "tile22_kernel": p22["kernel"],
                          "weight_MB_fp16": round(2e-6 * w.size, 2), "weight_MB_int8": round(1e-6 * w.size, 2),
                          "fp16_folded_us_median": round(1e3 * med(t16), 2), "tile22_us_median": round(1e3 * med(t22), 2),
                          "layernorm_q8_us_median": round(1e3 * med(tln), 2), "pair_us_median": round(1e3 * med(pair), 2),
                          "tile22_over_fp16": round(med(t22) / med(t16), 3), "pair_over_fp16": round(med(pair) / med(t16), 3),
                          "fp16_us_min_max": [round(1e3 * min(t16), 2), round(1e3 * max(t16), 2)],
                          "tile22_us_min_max": [round(1e3 * min(t22), 2), round(1e3 * max(t22), 2)],
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
    for scope in ("geglu", "attn"):
        obs = HipModel(cfg, sd16, batch=2, observe_activations=scope)
        obs(**inputs)
        ranges[scope] = aq.recipe_from_ranges(obs.activation_ranges())
        obs.close()
    qkv = {k: v for k, v in ranges["attn"].items() if k not in ranges["geglu"]}
    assert all(k.endswith(PARTS) for k in qkv)
    recipes = {"geglu scope": ranges["geglu"], "attn scope": ranges["attn"]}
    qkv_weights = sum(int(np.prod(sd16[k + ".weight"].shape)) for k in qkv)
    print(json.dumps({"calibration": "one forward per scope", "layers": {k: len(v) for k, v in recipes.items()}, "qkv_tensors": len(qkv),
                      "qkv_fp16_weight_MB": round(2e-6 * qkv_weights, 1), "s": round(time.time() - t0, 1)}), flush=True)
    models = {"fp16": HipModel(cfg, sd16, batch=2)}
    for k, r in recipes.items():
        models[k] = HipModel(cfg, sd16, batch=2, activation_quantization=r)
    outs = {k: m(**inputs)["noise_pred"] for k, m in models.items()}
    steps = {k: [] for k in models}
    for _ in range(rounds):                                                      # the handles alternating
        for k, m in models.items():
            steps[k].append(m.time_forward(warmup=3, iters=iters))
    print(json.dumps({"handle": "sd21-base random weights", "w8a8_info": {k: list(m.w8a8_info()) for k, m in models.items()},
                      "applied_tile22_tensors": len(set(models["attn scope"].w8a8_layers()) & set(qkv)),
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
