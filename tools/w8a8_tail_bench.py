#!/usr/bin/env python3
"""The W8A8 transformer tail - the GEGLU with an int8 output (plan tile 20), ff.net.2 from int8 activations (plan tile 24) and proj_out
(plan tile 19) - against the fp16 GEGLU and the merged fp16 tail launch it replaces: the measurements of LAB_NOTES round 31.  One
process, one session; prints one JSON line per measurement.

    python tools/w8a8_tail_bench.py box      # the box's calibration figures (cold_code_us among them)
    python tools/w8a8_tail_bench.py ops      # ff.net.2 of SD2.1-base at CFG batch 2 (2560 -> 640 at M = 2048, 5120 -> 1280 at M = 512):
                                             # tile 24, tile 19 and the fp16 single-source launch under the library's own plan, then
                                             # the triple GEGLU-q8out + tile 24 + proj_out (tile 19) against fp16 GEGLU (tile 13,
                                             # folded) + the merged two-source launch - sums of separately timed launches -
                                             # alternating, HIP events around --iters launches, median and range over --rounds rounds
    python tools/w8a8_tail_bench.py handle   # SD2.1-base on random weights, calibrated on one forward per scope: the fp16 handle and
                                             # the handles of the scopes "attn" and "tail", alternating: step time,
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

# (M, C) at CFG batch 2: ff.net.2 is 4C -> C, proj_out C -> C, ff.net.0.proj C -> 8C
OP_SHAPES = [(2048, 640), (512, 1280)]


def h16(a):
    return np.asarray(a, np.float32).astype(np.float16)


def med(v):
    return float(np.median(np.asarray(v, np.float64)))


def us(v):
    return {"median": round(1e3 * med(v), 2), "min_max": [round(1e3 * min(v), 2), round(1e3 * max(v), 2)]}


def box(iters, rounds):
    print(json.dumps({"calibration": _lib.calibrate(0)}), flush=True)


def ops(iters, rounds):
    rs = np.random.RandomState(31)
    nchw = lambda a: np.ascontiguousarray(a.T)[None, :, None, :]   # noqa: E731  (M, C) token-major -> (1, C, 1, M)
    for M, C in OP_SHAPES:
        K1 = 4 * C
        x = h16(rs.randn(M, C) * (1.0 + rs.rand(M, 1)) + 0.5)
        ln_w, ln_b = (1.0 + 0.2 * rs.randn(C)).astype(np.float32), (0.1 * rs.randn(C)).astype(np.float32)
        w0 = (rs.randn(8 * C, C) / np.sqrt(C)).astype(np.float32)
        b0 = (0.1 * rs.randn(8 * C)).astype(np.float32)
        w2 = (rs.randn(C, K1) / np.sqrt(K1)).astype(np.float32)
        wp = (rs.randn(C, C) / np.sqrt(C)).astype(np.float32)
        b2, bp = (0.1 * rs.randn(C)).astype(np.float32), (0.1 * rs.randn(C)).astype(np.float32)
        h2, tres = h16(rs.randn(M, C)), h16(rs.randn(M, C))
        w0q, w0s, _ = _lib.quantize_weight(w0)
        w2q, w2s, _ = _lib.quantize_weight(w2)
        wpq, wps, _ = _lib.quantize_weight(wp)
        bm13 = int(_lib.conv_plan(1, 1, 1, C, 0, 8 * C, 2, 1, M // 2, out_mode=2, flags=1 | 16)["kernel"].split("bm")[1])
        xq, _ = _lib.layernorm_q8(x, ln_w, ln_b, 6.0)
        g16, _, _ = _lib.geglu_w8a8(xq, w0q, w0s, 6.0, bias=b0, bm=bm13)
        a_g = float(np.abs(g16.astype(np.float32)).max())
        gq, _, _ = _lib.geglu_w8a8(xq, w0q, w0s, 6.0, bias=b0, bm=bm13, out_absmax=a_g)
        h3, p24, _ = _lib.gemm_q8(gq, w2q, w2s, a_g, bias=b2, res=h2)
        a_h = float(np.abs(h3.astype(np.float32)).max())
        merged_w = np.concatenate([wp @ w2, wp], axis=1)[:, :, None, None]       # [Wp W2 | Wp] over [g | h2]
        merged_b = wp @ b2 + bp
        p_fp16 = _lib.conv_plan(1, 1, 1, K1, 0, C, 2, 1, M // 2, flags=4 | 16)
        p_merged = _lib.conv_plan(1, 1, 1, K1, C, C, 2, 1, M // 2, flags=4 | 16)
        t = {k: [] for k in ("tile24", "tile19_ffn2", "fp16_ffn2", "geglu_q8out", "geglu_i8_fp16out", "proj_out_tile19", "geglu_fp16_folded", "merged_fp16")}
        for _ in range(rounds):                                                  # alternating, back to back
            t["tile24"].append(_lib.gemm_q8(gq, w2q, w2s, a_g, bias=b2, res=h2, iters=iters)[2])
            t["tile19_ffn2"].append(_lib.gemm_w8a8(nchw(g16), w2q, w2s, a_g, bias=b2, res=nchw(h2), iters=iters)[2])
            t["fp16_ffn2"].append(_lib.conv2d(nchw(g16), h16(w2)[:, :, None, None], bias=b2, res=nchw(h2), iters=iters)[1])
            t["geglu_q8out"].append(_lib.geglu_w8a8(xq, w0q, w0s, 6.0, bias=b0, bm=bm13, out_absmax=a_g, iters=iters)[2])
            t["geglu_i8_fp16out"].append(_lib.geglu_w8a8(xq, w0q, w0s, 6.0, bias=b0, bm=bm13, iters=iters)[2])
            t["proj_out_tile19"].append(_lib.gemm_w8a8(nchw(h3), wpq, wps, a_h, bias=bp, res=nchw(tres), iters=iters)[2])
            t["geglu_fp16_folded"].append(_lib.geglu_ln(x, h16(w0), bias=b0, ln_weight=ln_w, ln_bias=ln_b, kernel=101 if bm13 == 128 else 102, iters=iters)[1])
            t["merged_fp16"].append(_lib.conv2d_ex(nchw(g16), h16(merged_w), bias=merged_b, res=nchw(tres), x1=nchw(h2), iters=iters)[3])
        triple = [a + b + c for a, b, c in zip(t["geglu_q8out"], t["tile24"], t["proj_out_tile19"])]
        pair = [a + b for a, b in zip(t["geglu_fp16_folded"], t["merged_fp16"])]
        i8_pair = [a + b for a, b in zip(t["geglu_i8_fp16out"], t["merged_fp16"])]
        print(json.dumps({"op": "tail", "shape": f"ff.net.2 {K1}->{C} M={M}", "tile24_kernel": "smgemm_q8 bm%d" % (32 if p24[1] == 1 else 64),
                          "fp16_ffn2_plan": p_fp16["kernel"], "merged_plan": p_merged["kernel"],
                          "ffn2_weight_MB_fp16": round(2e-6 * w2.size, 2), "ffn2_weight_MB_int8": round(1e-6 * w2.size, 2),
                          "us": {k: us(v) for k, v in t.items()},
                          "tile24_over_fp16_ffn2": round(med(t["tile24"]) / med(t["fp16_ffn2"]), 3),
                          "tile24_over_tile19": round(med(t["tile24"]) / med(t["tile19_ffn2"]), 3),
                          "triple_us": us(triple), "fp16_geglu_plus_merged_us": us(pair), "int8_geglu_plus_merged_us": us(i8_pair),
                          "triple_over_fp16_pair": round(med(triple) / med(pair), 3), "triple_over_int8_geglu_pair": round(med(triple) / med(i8_pair), 3),
                          "rounds": rounds, "iters": iters}), flush=True)


def handle(iters, rounds):
    from oracle import psnr, unet_ref, weights
    cfg = unet_ref.CONFIGS["sd21-base"]
    sd16 = weights.make_state_dict(unet_ref.unet_param_shapes(cfg), seed=21, dtype=np.float16)
    hw = cfg["sample_size"]
    inputs = dict(sample=weights.seeded_normal((2, 4, hw, hw), 1).astype(np.float16), timestep=np.array([981, 981], np.float16),
                  encoder_hidden_states=weights.seeded_normal((2, cfg["cross_attention_dim"], 1, 77), 2).astype(np.float16))
    t0 = time.time()
    recipes = {}
    for scope in ("attn", "tail"):
        obs = HipModel(cfg, sd16, batch=2, observe_activations=scope)
        obs(**inputs)
        recipes[scope] = aq.recipe_from_ranges(obs.activation_ranges())
        obs.close()
    tails = {k: v for k, v in recipes["tail"].items() if k not in recipes["attn"]}
    tail_weights = sum(int(np.prod(sd16[k + ".weight"].shape)) for k in tails)
    print(json.dumps({"calibration": "one forward per scope", "layers": {k: len(v) for k, v in recipes.items()},
                      "tail_layers": {"ff.net.2": sum(k.endswith("ff.net.2") for k in tails), "proj_out": sum(k.endswith("proj_out") for k in tails)},
                      "tail_layers_fp16_weight_MB": round(2e-6 * tail_weights, 1), "s": round(time.time() - t0, 1)}), flush=True)
    models = {"fp16": HipModel(cfg, sd16, batch=2)}
    for k, r in recipes.items():
        models[k] = HipModel(cfg, sd16, batch=2, activation_quantization=r)
    outs = {k: m(**inputs)["noise_pred"] for k, m in models.items()}
    steps = {k: [] for k in models}
    for _ in range(rounds):                                                      # the handles alternating
        for k, m in models.items():
            steps[k].append(m.time_forward(warmup=3, iters=iters))
    labels = [lab for lab, _, _ in models["tail"].profile(1)]
    print(json.dumps({"handle": "sd21-base random weights", "w8a8_info": {k: list(m.w8a8_info()) for k, m in models.items()},
                      "applied_tail_layers": len(set(models["tail"].w8a8_layers()) & set(tails)),
                      "launches": {"geglu_q8out": sum("+q8out+w8a8" in lab for lab in labels), "quantize_q8": sum(lab.startswith("quantize_q8") for lab in labels),
                                   "merged_tails_left": sum("ff.net.2 + residual + proj_out" in lab for lab in labels)},
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
