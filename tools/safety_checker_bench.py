#!/usr/bin/env python
"""Timing of the full ViT-L/14 safety checker (24 layers, random weights, batch 1) and of its attention kernel next to sd_op_attention.
usage (from the repository root): tools/safety_checker_bench.py time     HIP-event time per image (graph replay / eager), attention operators
                                  tools/safety_checker_bench.py trace    six eager runs, to be wrapped in rocprofv3 --kernel-trace
                                                                          (summarise the database with tools/rocpd_stats.py)"""
import sys, time, json
sys.path[:0] = [".", "ml-stable-diffusion_amd", "tests"]
import numpy as np
from oracle import weights
from python_hip_stable_diffusion import HipSafetyChecker, _lib
from test_safety_checker import make_checkpoint, CONFIGS

mode = sys.argv[1]
cfg = dict(CONFIGS["vit-l-2"], num_hidden_layers=24)
sd = make_checkpoint(cfg, seed=3)
x = weights.seeded_normal((1, 3, 224, 224), 5).astype(np.float16)
if mode == "time":
    chk = HipSafetyChecker(cfg, sd, batch=1, use_graph=True)
    print("device MB", chk.device_bytes() / 2**20)
    for _ in range(3):
        chk.run(x)
    ms, wall = [], []
    for _ in range(40):
        t = time.perf_counter(); chk.run(x); wall.append((time.perf_counter() - t) * 1e3); ms.append(chk.last_ms())
    print("GRAPH replay last_ms: median %.3f min %.3f max %.3f | wall per call median %.3f" % (np.median(ms), min(ms), max(ms), np.median(wall)))
    chk.close()
    chk = HipSafetyChecker(cfg, sd, batch=1, use_graph=False)
    for _ in range(3):
        chk.run(x)
    ms = []
    for _ in range(20):
        chk.run(x); ms.append(chk.last_ms())
    print("EAGER launches last_ms: median %.3f min %.3f" % (np.median(ms), min(ms)))
    chk.close()
    rs = np.random.RandomState(0)
    for B, S, H in ((1, 257, 16), (2, 257, 16), (1, 256, 16)):
        qkv = rs.randn(B, S, 3 * H * 64).astype(np.float16)
        _, t_new = _lib.vit_attention(qkv, H, iters=200)
        q, k, v = (np.ascontiguousarray(qkv[:, :, i * H * 64:(i + 1) * H * 64].transpose(0, 2, 1)[:, :, None, :]) for i in range(3))
        _, t_old = _lib.attention("ORIGINAL", q, k, v, H, 64, iters=200)
        _, t_old1 = _lib.attention("ORIGINAL", q, k, v, H, 64, variant=1, iters=200)
        print("ATTN B%d S%d heads%d: vit_attention %.2f us | sd_op_attention ORIGINAL %.2f us (variant 1: %.2f us)" % (B, S, H, t_new * 1e3, t_old * 1e3, t_old1 * 1e3))
else:
    chk = HipSafetyChecker(cfg, sd, batch=1, use_graph=False)
    for _ in range(6):
        chk.run(x)
    print("eager last_ms", chk.last_ms())
    chk.close()
