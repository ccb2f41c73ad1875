#!/usr/bin/env python3
"""The W8A8 self-attention einsums (attention_i8.hip: int8 Q.K^T and P.V, two passes over the keys) and the quantizer launch in front of
them against the fp16 head-dim-64 attention kernel (attention8.hip).  One process, one session; prints one JSON line per measurement.

    python tools/w8a8_einsum_bench.py box      # the box's calibration figures (cold_code_us among them)
    python tools/w8a8_einsum_bench.py ops      # SD2.1-base's four self-attention shapes at CFG batch 2 (heads x S = 5 x 4096, 10 x 1024,
                                               # 20 x 256, 20 x 64): the fp16 attention by the library's dispatch with pre-scaled queries
                                               # (what a handle runs), the int8 attention and the einsum_q8 quantizer launch on its own,
                                               # alternating, HIP events around --iters launches, median and range over --rounds rounds.
                                               # The pair's figure is the SUM of the two separately timed launches
    python tools/w8a8_einsum_bench.py handle   # SD2.1-base on random weights, calibrated on one forward per scope: the fp16 handle, the
                                               # handle with every layer of the tail scope and that one with the einsums added,
                                               # alternating: step time, arena bytes, applied einsums, PSNR against the fp16 handle's

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

# (B, heads, S) at CFG batch 2
OP_SHAPES = [(2, 5, 4096), (2, 10, 1024), (2, 20, 256), (2, 20, 64)]
Q_PRE = float(np.float32(1.4426950408889634) / np.float32(8.0))                  # attention_q_prescale(64)


def med(v):
    return float(np.median(np.asarray(v, np.float64)))


def box(iters, rounds):
    print(json.dumps({"calibration": _lib.calibrate(0)}), flush=True)


def ops(iters, rounds):
    rs = np.random.RandomState(31)
    for B, heads, S in OP_SHAPES:
        C = heads * 64
        q, k, v = ((rs.randn(B, C, 1, S) * 1.5).astype(np.float16) for _ in range(3))
        tok = lambda t: np.ascontiguousarray(t.reshape(B, C, S).transpose(0, 2, 1).reshape(B * S, C))   # noqa: E731
        r_q, r_k, r_v = (float(np.abs(t.astype(np.float32)).max()) for t in (q, k, v))
        qq, kq, vq = ((np.clip(np.rint(tok(t).astype(np.float32) * (127.0 / r)), -127, 127)).astype(np.int8) for t, r in ((q, r_q), (k, r_k), (v, r_v)))
        qk = np.concatenate([(tok(q).astype(np.float32) * Q_PRE).astype(np.float16), tok(k)], axis=1)
        vt = np.ascontiguousarray(v.reshape(B, C, S))
        t16, ti8, tq8 = [], [], []
        for _ in range(rounds):                                                  # alternating, back to back
            t16.append(_lib.attention("SPLIT_EINSUM", (q.astype(np.float32) * Q_PRE).astype(np.float16), k, v, heads, 64, variant=2, iters=iters)[1])
            ti8.append(_lib.attention_w8a8(qq, kq, vq, r_q, r_k, r_v, B, heads, iters=iters)[1])
            tq8.append(_lib.einsum_quantize(qk, vt, r_q * Q_PRE, r_k, r_v, vt_perm_in=0, iters=iters)[2])
        pair = [a + b for a, b in zip(ti8, tq8)]
        print(json.dumps({"op": "attention", "shape": f"B={B} h={heads} S={S}", "fp16_us_median": round(1e3 * med(t16), 2),
                          "int8_us_median": round(1e3 * med(ti8), 2), "einsum_q8_us_median": round(1e3 * med(tq8), 2),
                          "pair_us_median": round(1e3 * med(pair), 2), "int8_over_fp16": round(med(ti8) / med(t16), 3),
                          "pair_over_fp16": round(med(pair) / med(t16), 3), "fp16_us_min_max": [round(1e3 * min(t16), 2), round(1e3 * max(t16), 2)],
                          "int8_us_min_max": [round(1e3 * min(ti8), 2), round(1e3 * max(ti8), 2)],
                          "einsum_q8_us_min_max": [round(1e3 * min(tq8), 2), round(1e3 * max(tq8), 2)], "rounds": rounds, "iters": iters}), flush=True)


def handle(iters, rounds):
    from oracle import psnr, unet_ref, weights
    cfg = unet_ref.CONFIGS["sd21-base"]
    sd16 = weights.make_state_dict(unet_ref.unet_param_shapes(cfg), seed=21, dtype=np.float16)
    hw = cfg["sample_size"]
    inputs = dict(sample=weights.seeded_normal((2, 4, hw, hw), 1).astype(np.float16), timestep=np.array([981, 981], np.float16),
                  encoder_hidden_states=weights.seeded_normal((2, cfg["cross_attention_dim"], 1, 77), 2).astype(np.float16))
    t0 = time.time()
    recipes = {}
    for scope in ("tail", "einsum"):
        obs = HipModel(cfg, sd16, batch=2, observe_activations=scope)
        obs(**inputs)
        recipes[scope + " scope"] = aq.recipe_from_ranges(obs.activation_ranges())
        obs.close()
    einsums = [k for k in recipes["einsum scope"] if aq.is_einsum(k)]
    print(json.dumps({"calibration": "one forward per scope", "layers": {k: len(v) for k, v in recipes.items()}, "einsums": len(einsums),
                      "s": round(time.time() - t0, 1)}), flush=True)
    models = {"fp16": HipModel(cfg, sd16, batch=2)}
    for k, r in recipes.items():
        models[k] = HipModel(cfg, sd16, batch=2, activation_quantization=r)
    outs = {k: m(**inputs)["noise_pred"] for k, m in models.items()}
    steps = {k: [] for k in models}
    for _ in range(rounds):                                                      # the handles alternating
        for k, m in models.items():
            steps[k].append(m.time_forward(warmup=3, iters=iters))
    print(json.dumps({"handle": "sd21-base random weights", "w8a8_info": {k: list(m.w8a8_info()) for k, m in models.items()},
                      "einsum_info": {k: list(m.einsum_info()) for k, m in models.items()},
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
