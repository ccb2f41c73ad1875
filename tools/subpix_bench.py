#!/usr/bin/env python3
"""The sub-pixel upsampler conv (plan tile 21) against the halo conv with the upsample in its gather (plan tile 7): the measurements
of LAB_NOTES round 28.  One session; prints one JSON line per measurement.

    python tools/subpix_bench.py ops      # the upsampler shapes of SD2.1-base at CFG batch 2: tile 7 on the library's plan for the
                                          # shape and tile 21 (each built ring, both phase orders where asked) alternating back to back,
                                          # HIP events around --iters launches, median and range over --rounds rounds
    python tools/subpix_bench.py handle   # the step: bench.py children, one per configuration of --configs, interleaved --rounds times,
                                          # each under its own timeout; a failing child ends the run.  A configuration is the value of
                                          # SD_UP_SUBPIX, optionally ":<M>" for SD_UP_SUBPIX_M (mode 2 on the one shape with M output
                                          # pixels), e.g.  --configs 0 2 2:2048 2:8192 2:512

Operator times are back-to-back launches of one conv on hot caches: ratios between kernels, not step times.  The phase order of the
grid (SD_SUBPIX_PHASE_OUTER) is read once per process: `ops` reports the order of its own process."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ml-stable-diffusion_amd")]

# (C, Hi, Wi): C -> C at batch 2, Hi x Wi -> 2Hi x 2Wi
OP_SHAPES = [(1280, 16, 16), (640, 32, 32), (1280, 8, 8)]


def h16(a):
    return np.asarray(a, np.float32).astype(np.float16)


def med(v):
    return float(np.median(np.asarray(v, np.float64)))


def ops(iters, rounds):
    from python_hip_stable_diffusion import _lib
    rs = np.random.RandomState(28)
    for C, H, W in OP_SHAPES:
        x = h16(rs.randn(2, C, H, W))
        w = h16(rs.randn(C, C, 3, 3) / np.sqrt(9 * C))
        bias = (0.1 * rs.randn(C)).astype(np.float32)
        p7 = _lib.conv_plan(3, 1, 2, C, 0, C, 2, 2 * H, 2 * W, flags=16)
        forced = p7["tile"] != 7
        if forced:
            p7 = _lib.conv_plan(3, 1, 2, C, 0, C, 2, 2 * H, 2 * W, flags=16, tile=7, staging=3)
        t = {"tile7": [], "tile21_ring3": [], "tile21_ring4": []}
        plans = {}
        for _ in range(rounds):                                                  # alternating, back to back
            t["tile7"].append(_lib.conv2d_ex(x, w, bias, upsample=True, tile=10 * p7["staging"] + 7, splitk=p7["splitk"], iters=iters)[3])
            for code, key in ((2, "tile21_ring3"), (3, "tile21_ring4")):
                _, plans[key], ms = _lib.conv2d_subpixel(x, w, bias, staging=code, iters=iters)
                t[key].append(ms)
        row = {"op": "conv3x3 x2 upsample", "shape": f"{C}->{C} @{2 * H}x{2 * W} B=2", "library_plan_is_tile7": not forced, "tile7_kernel": p7["kernel"],
               "tile7_splitk": p7["splitk"], "tile21_splitk": plans["tile21_ring4"][2], "weight_MB_3x3": round(2e-6 * w.size, 1),
               "weight_MB_folded": round(2e-6 * w.size * 16 / 9, 1), "phase_outer": os.environ.get("SD_SUBPIX_PHASE_OUTER", "0"),
               "rounds": rounds, "iters": iters}
        for k, v in t.items():
            row[k + "_us_median"] = round(1e3 * med(v), 2)
            row[k + "_us_min_max"] = [round(1e3 * min(v), 2), round(1e3 * max(v), 2)]
        row["ring4_over_tile7"] = round(med(t["tile21_ring4"]) / med(t["tile7"]), 3)
        print(json.dumps(row), flush=True)


def handle(configs, rounds, steps, warmup, timeout):
    results = {c: [] for c in configs}
    for r in range(rounds):
        for c in configs:                                                        # interleaved: one child per configuration and round
            mode, _, only_m = c.partition(":")
            env = dict(os.environ, SD_TUNE="1", SD_UP_SUBPIX=mode)
            env.pop("SD_UP_SUBPIX_M", None)
            if only_m:
                env["SD_UP_SUBPIX_M"] = only_m
            p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--cpu-steps", "0"],
                               env=env, capture_output=True, text=True, timeout=timeout)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
            if p.returncode != 0 or not line:
                print(json.dumps({"config": c, "round": r, "failed": p.returncode, "stderr_tail": p.stderr[-1500:]}), flush=True)
                sys.exit(1)                                                      # nothing more is started behind a failed child
            j = json.loads(line[-1])
            results[c].append(j["ms_per_step"])
            print(json.dumps({"config": c, "round": r, "ms_per_step": j["ms_per_step"], "repeats_ms_per_step": j.get("repeats_ms_per_step"),
                              "cold_code_us": j.get("calibration", {}).get("cold_code_us")}), flush=True)
    print(json.dumps({"step_ms_median": {c: round(med(v), 4) for c, v in results.items()},
                      "step_ms_min_max": {c: [min(v), max(v)] for c, v in results.items()}, "rounds": rounds}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["ops", "handle"])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--configs", nargs="+", default=["0", "1"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per bench.py child")
    a = ap.parse_args()
    if a.what == "ops":
        ops(a.iters, a.rounds)
    else:
        handle(a.configs, a.rounds, a.steps, a.warmup, a.timeout)
