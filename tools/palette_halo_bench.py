#!/usr/bin/env python3
"""The palettized halo conv (plan tile 25) against the fp16 halo conv (plan tile 7), and an SD2.1-base handle with the store's halo
switch off and on: the measurements of LAB_NOTES round 34.  One process, one session; prints one JSON line per measurement, the box's
calibration (`cold_code_us`) first.

    python tools/palette_halo_bench.py ops      # the 3x3 / stride-1 shapes of SD2.1-base at CFG batch 2 above the 8x8 level: tile 25 at 4,
                                                # 6 and 8 bits vs tile 7 on the library's plan codes for the shape (ring, split-K),
                                                # alternating back to back, HIP events around --iters launches, median and range over
                                                # --rounds rounds
    python tools/palette_halo_bench.py handle   # SD2.1-base on random weights: the fp16 handle, the 6-bit palettized handle with the halo
                                                # switch off and the one with it on, alternating: step time, sd_unet_device_bytes,
                                                # arena_used_bytes, palette_info, PSNR of switch-on against switch-off (identical bits: inf)

Operator times are back-to-back launches of one conv on hot caches: ratios between kernels, not step times."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ml-stable-diffusion_amd")]

from python_hip_stable_diffusion import HipModel, _lib, hip_model, palettize  # noqa: E402

# (C0, C1, Cout, H, W of the source, upsample)
OP_SHAPES = [(1280, 0, 1280, 16, 16, False), (1280, 1280, 1280, 16, 16, False), (640, 0, 640, 32, 32, False), (640, 640, 640, 32, 32, False),
             (320, 0, 320, 64, 64, False), (1280, 0, 1280, 16, 16, True)]
OP_BITS = (4, 6, 8)


def h16(a):
    return np.asarray(a, np.float32).astype(np.float16)


def med(v):
    return float(np.median(np.asarray(v, np.float64)))


def ops(iters, rounds):
    rs = np.random.RandomState(33)
    for C0, C1, N, H, W, ups in OP_SHAPES:
        ctot, up = C0 + C1, 2 if ups else 1
        x = h16(rs.randn(2, C0, H, W))
        x1 = h16(rs.randn(2, C1, H, W)) if C1 else None
        bias = (0.1 * rs.randn(N)).astype(np.float32)
        pal = {}
        for nbits in OP_BITS:
            lut = h16(np.sort(rs.randn(1 << nbits)) / np.sqrt(9 * ctot))
            pal[nbits] = (lut, rs.randint(0, 1 << nbits, size=(N, ctot, 3, 3)).astype(np.uint8))
        w = {nbits: h16(lut[idx]) for nbits, (lut, idx) in pal.items()}
        lib_plan = _lib.conv_plan(3, 1, up, C0, C1, N, 2, H * up, W * up, flags=16)
        forced = lib_plan["tile"] != 7                                            # (a shape whose own plan is another kernel: tile 7's default ring)
        p7 = _lib.conv_plan(3, 1, up, C0, C1, N, 2, H * up, W * up, flags=16, tile=7, staging=3) if forced else lib_plan
        t7, t25 = [], {nbits: [] for nbits in OP_BITS}
        same = {}
        for r in range(rounds):                                                  # alternating, back to back
            o7, _, _, ms = _lib.conv2d_ex(x, w[6], bias, x1=x1, upsample=ups, tile=10 * p7["staging"] + 7, splitk=p7["splitk"], iters=iters)
            t7.append(ms)
            for nbits, (lut, idx) in pal.items():
                o25, _, ms = _lib.conv2d_palettized_halo(x, lut, idx, nbits, bias=bias, x1=x1, upsample=ups, staging=p7["staging"], splitk=p7["splitk"],
                                                         iters=iters)
                t25[nbits].append(ms)
                if r == 0 and nbits == 6:
                    same[nbits] = bool(np.array_equal(o7.view(np.uint16), o25.view(np.uint16)))
        p25 = _lib.conv_plan(3, 1, up, C0, C1, N, 2, H * up, W * up, flags=16, tile=25, staging=p7["staging"], splitk=p7["splitk"])
        print(json.dumps({"op": "conv3x3", "shape": f"{ctot}->{N} @{H * up}x{W * up} B=2" + (" x2 upsample" if ups else ""),
                          "library_plan_is_tile7": not forced, "library_plan_tile": lib_plan["tile"], "tile7_kernel": p7["kernel"], "tile25_kernel": p25["kernel"],
                          "splitk": p7["splitk"], "weight_MB_fp16": round(2e-6 * N * ctot * 9, 1),
                          "stream_MB": {str(b): round(1e-6 * -(-N // 64) * 64 * 9 * ctot * b / 8, 1) for b in OP_BITS},
                          "bit_identical_at_6_bits": same.get(6), "tile7_us_median": round(1e3 * med(t7), 2),
                          "tile25_us_median": {str(b): round(1e3 * med(v), 2) for b, v in t25.items()},
                          "tile25_over_tile7": {str(b): round(med(v) / med(t7), 3) for b, v in t25.items()},
                          "tile7_us_min_max": [round(1e3 * min(t7), 2), round(1e3 * max(t7), 2)],
                          "tile25_us_min_max": {str(b): [round(1e3 * min(v), 2), round(1e3 * max(v), 2)] for b, v in t25.items()},
                          "rounds": rounds, "iters": iters}), flush=True)


def handle(iters, rounds):
    from oracle import psnr, unet_ref, weights
    cfg = unet_ref.CONFIGS["sd21-base"]
    sd16 = weights.make_state_dict(unet_ref.unet_param_shapes(cfg), seed=21, dtype=np.float16)
    hw = cfg["sample_size"]
    inputs = dict(sample=weights.seeded_normal((2, 4, hw, hw), 1).astype(np.float16), timestep=np.array([981, 981], np.float16),
                  encoder_hidden_states=weights.seeded_normal((2, cfg["cross_attention_dim"], 1, 77), 2).astype(np.float16))
    t0 = time.time()
    store = hip_model.Weights(sd16)
    palettize.apply(store, nbits=6)
    print(json.dumps({"palettize": "sd21-base random weights, 6 bits", "s": round(time.time() - t0, 1)}), flush=True)
    models = {"fp16": HipModel(cfg, sd16, batch=2), "pal6": HipModel(cfg, store, batch=2), "pal6_halo": HipModel(cfg, store, batch=2, palette_halo=True)}
    store.close()
    outs = {k: m(**inputs)["noise_pred"].copy() for k, m in models.items()}
    steps = {k: [] for k in models}
    for _ in range(rounds):                                                      # the three handles alternating
        for k, m in models.items():
            steps[k].append(m.time_forward(warmup=3, iters=iters))
    labels = [lab for lab, _, _ in models["pal6_halo"].profile(1)]
    halo = [lab for lab in labels if lab.startswith("conv3x3+pal") and " @8x8 " not in lab]
    identical = bool(np.array_equal(outs["pal6"].view(np.uint16), outs["pal6_halo"].view(np.uint16)))
    p = psnr.compute_psnr(outs["pal6_halo"], outs["pal6"])
    print(json.dumps({"handle": "sd21-base random weights", "palette_info": {k: list(m.palette_info()) for k, m in models.items()},
                      "tile25_convs": len(halo), "step_ms_median": {k: round(med(v), 4) for k, v in steps.items()},
                      "step_ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in steps.items()},
                      "device_bytes": {k: m.device_bytes for k, m in models.items()},
                      "arena_used_bytes": {k: m.arena_used_bytes for k, m in models.items()},
                      "halo_on_vs_off_identical_bits": identical, "halo_on_vs_off_psnr_db": "inf" if np.isinf(p) else round(float(p), 2),
                      "psnr_db_pal6_vs_fp16": round(float(psnr.compute_psnr(outs["pal6"], outs["fp16"])), 2), "rounds": rounds, "iters": iters}), flush=True)
    for m in models.values():
        m.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["ops", "handle"])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    print(json.dumps({"calibration": _lib.calibrate()}), flush=True)
    {"ops": ops, "handle": handle}[a.what](a.iters, a.rounds)
