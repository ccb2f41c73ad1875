#!/usr/bin/env python
"""What a progress handler costs the device-resident loop: SD2.1-base at 512 x 512 (64 x 64 latents, CFG batch 2), 20 DDIM steps,
a no-op handler after every step (sd_unet_denoise_loop_progress: one snapshot copy + one stream drain per step) against no handler,
and the same with the de-noised tap (`pred`: one more 64-KB store per step plus its copy).  A handle keeps ONE captured step graph,
keyed among others on the tap but not on the handler: "no_handler" and "handler" share a key and run on one handle, the tap variant
runs on a second handle of its own, so no timed call captures a graph.  The three variants alternate inside one process, round after
round, behind a warm-up round; a number is the host wall clock around the whole call, which ends in a stream synchronise, over the
steps, next to the median of the per-step device events (which exclude the copy and the handler by construction).  Prints one JSON
line.  Random weights: the time does not depend on them."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ml-stable-diffusion_amd")):
    sys.path.insert(0, p)
from python_hip_stable_diffusion import HipModel, checkpoint, schedulers  # noqa: E402

MODEL = "stabilityai/stable-diffusion-2-1-base"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--attention-implementation", default="ORIGINAL")
    a = ap.parse_args()
    ck = checkpoint.random_checkpoint(checkpoint.unet_param_shapes(MODEL), seed=0)
    m = HipModel(MODEL, ck, batch=2, attention_implementation=a.attention_implementation, device=0)
    m_tap = HipModel(MODEL, ck, batch=2, attention_implementation=a.attention_implementation, device=0)
    ehs = np.random.RandomState(94).randn(2, 1024, 1, 77).astype(np.float16)
    lat = np.random.RandomState(93).randn(1, 4, 64, 64).astype(np.float32)
    sch = schedulers.DDIMScheduler()
    sch.set_timesteps(a.steps)
    ts, coef, hist = sch.device_tables()
    pred = sch.denoised_table()
    noop = lambda step, n, latents, denoised: True   # noqa: E731
    variants = {"no_handler": (m, {}), "handler": (m, dict(progress=noop)), "handler_denoised": (m_tap, dict(progress=noop, pred=pred))}
    wall = {k: [] for k in variants}
    event = {k: [] for k in variants}
    outs = {}
    for r in range(a.rounds + 1):                    # round 0 warms both handles up (graph capture, code objects) and is not timed
        for name, (model, kw) in variants.items():
            t0 = time.perf_counter()
            out, ms = model.denoise_loop(lat, ts, coef, 7.5, history=hist, encoder_hidden_states=ehs, **kw)
            dt = time.perf_counter() - t0
            outs[name] = out
            if r:
                wall[name].append(dt / a.steps * 1e3)
                event[name].append(float(np.median(ms)))
    same = all(np.array_equal(outs["no_handler"], o) for o in outs.values())
    res = {"model": MODEL, "steps": a.steps, "rounds": a.rounds, "attention": a.attention_implementation, "identical_latents": same}
    for name in variants:
        res[name] = {"wall_ms_per_step_median": round(float(np.median(wall[name])), 4),
                     "wall_ms_per_step_min_max": [round(min(wall[name]), 4), round(max(wall[name]), 4)],
                     "event_ms_per_step_median": round(float(np.median(event[name])), 4)}
    print(json.dumps(res))
    m.close()
    m_tap.close()
    if not same:
        sys.exit("the variants' final latents differ")


if __name__ == "__main__":
    main()
