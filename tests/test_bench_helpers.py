"""CPU suite: the host-side bookkeeping of bench.py - kernel-family attribution of the per-op profile, the dominant
kernel by TIME share, and the rule that `roofline.traffic` is only reported from a PMC file measured on this very library
and workload (a committed file from another build must not pass as this run's traffic); --dump-outputs and
--full.  One GPU test at the end: a plain run on the real model stays lean."""
import argparse
import json
import os

import pytest

import bench
from conftest import ROOT

OPS = [
    ("conv3x3 320->320 @64x64 M=8192 K=2880 down_blocks.0.resnets.0.conv1 #0,3,1,1,320,320,8192", 15.1e9, 0.028),
    ("conv3x3 4->320 @64x64 M=8192 K=36 conv_in #0,3,1,1,4,320,8192", 0.2e9, 0.009),
    ("gemm1x1 320->320 @64x64 M=8192 K=320 x.proj_in #0,1,1,1,320,320,8192", 1.7e9, 0.012),
    ("geglu1x1+ln 320->2560 @64x64 M=8192 K=320 x.ff.net.0.proj #2,1,1,1,320,2560,8192", 13.4e9, 0.048),
    ("attention h=5 d=64 Sq=4096 Sk=4096", 43e9, 0.112),
    ("xattn+ln q-proj 320->320 + attention h=5 d=64 Sq=4096 Sk=77 x.attn2", 2.1e9, 0.022),
    ("groupnorm C=320 @64x64 x.norm1", 0.0, 0.010),
    ("conv3x3 small-N conv_out -> fp32 NCHW", 0.19e9, 0.035),
    ("boundary: timestep f16->f32, sample NCHW->NHWC", 0.0, 0.011),
]


def test_kernel_families_and_dominant_kernel_by_time_share():
    fam = {bench.op_family(lbl) for lbl, _, _ in OPS}
    assert len(fam) == 6
    assert bench.op_family(OPS[1][0]).startswith("other") and bench.op_family(OPS[7][0]).startswith("other")
    r = bench.kernel_families(OPS, graph_ms=0.25)
    rows = r["kernel_families"]
    assert [x["family"] for x in rows][0].startswith("self-attention")            # 0.112 ms: the largest TIME share
    assert r["dominant_kernel"]["kernel"] == rows[0]["family"] and abs(sum(x["share"] for x in rows) - 1.0) < 1e-3
    att = rows[0]
    assert att["launches"] == 1 and abs(att["achieved"] - 43e9 / 0.112e-3 / 1e12) < 0.1 and abs(att["frac"] - att["achieved"] / 2500) < 1e-3
    gemm = next(x for x in rows if x["family"].startswith("1x1 GEMMs"))
    assert gemm["launches"] == 2 and abs(gemm["ms"] - 0.060) < 1e-6
    assert r["step_ops"] == len(OPS)


def test_traffic_is_reported_only_for_the_profiled_build_and_workload():
    path = os.path.join(ROOT, "profiles", bench.HBM_TRAFFIC_FILE)
    if not os.path.exists(path):   # no PMC pass committed (yet) for this round's library: nothing may be reported
        args = argparse.Namespace(model="sd21-base", prompts_per_gpu=1, attention="ORIGINAL")
        got = bench.hbm_traffic(5.0, args, 64)
        assert got["traffic"] is None and got["traffic_source"] is None
        return
    t = json.load(open(path))
    for key in ("build_id", "model", "latent", "prompts_per_gpu", "attention", "bytes_per_step", "read_bytes_per_step"):
        assert key in t, key
    args = argparse.Namespace(model=t["model"], prompts_per_gpu=t["prompts_per_gpu"], attention=t["attention"])
    got = bench.hbm_traffic(5.0, args, t["latent"])
    if bench.build_id() == t["build_id"]:            # the committed file belongs to the committed source
        assert got["traffic"] == t["bytes_per_step"] and 0.1 < got["traffic_detail"]["hbm_frac"] < 1.0
        assert "replayed from profiles/" in got["traffic_source"] and "NOT measured by this run" in got["traffic_source"]
    else:
        assert got["traffic"] is None
    for other in (argparse.Namespace(model="sdxl-base", prompts_per_gpu=1, attention="ORIGINAL"),
                  argparse.Namespace(model=t["model"], prompts_per_gpu=2, attention=t["attention"]),
                  argparse.Namespace(model=t["model"], prompts_per_gpu=1, attention="SPLIT_EINSUM")):
        miss = bench.hbm_traffic(5.0, other, t["latent"])
        assert miss["traffic"] is None and "another build / workload" in miss["traffic_detail"]["note"]
    assert bench.hbm_traffic(5.0, args, 96)["traffic"] is None


def test_bench_models_cover_the_baseline_configs():
    assert set(bench.MODELS) == {"sd21-base", "sdxl-base", "sdxl-refiner", "sd15-control"}
    assert bench.MODELS["sd21-base"]["latent"] == 64 and bench.MODELS["sdxl-base"]["latent"] == 96
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    assert "SD2.1-base 512" in base["configs"][1] and "config 2" in bench.MODELS["sd21-base"]["config"]


def _stub_bench(tmp_path, steps, tag):
    import subprocess
    import sys
    out = tmp_path / tag
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--prompts-per-gpu", "2", "--stub-model", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), out


def test_dump_outputs_writes_the_timed_loops_final_latents_deterministically(tmp_path):
    """--dump-outputs DIR: the gathered final latents of the last timed loop as DIR/latents.npy (float32), identical from run
    to run with the same arguments; --steps sets the timed steps, the line carries ms_per_step (bench.py's own plumbing,
    StubModel in the UNet's place)."""
    import numpy as np
    a, da = _stub_bench(tmp_path, 3, "a")
    b, db = _stub_bench(tmp_path, 3, "b")
    c, dc = _stub_bench(tmp_path, 4, "c")
    assert sorted(os.listdir(da)) == ["latents.npy"]
    la, lb, lc = (np.load(d / "latents.npy") for d in (da, db, dc))
    assert la.dtype == np.float32 and la.shape == (2, 4, 64, 64) and np.isfinite(la).all()
    assert np.array_equal(la, lb) and not np.array_equal(la, lc)
    assert a["steps"] == 3 and c["steps"] == 4 and a["ms_per_step"] > 0
    assert abs(float(np.asarray(la, np.float64).sum()) - a["checksum"]) <= 1e-6 * max(1.0, abs(a["checksum"]))


def test_full_and_dump_outputs_are_options_and_streams_requires_full():
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120,
                       cwd=ROOT)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--streams", "2", "--stub-model"], capture_output=True,
                       text=True, timeout=120, cwd=ROOT)
    assert r.returncode != 0 and "--full" in r.stderr


@pytest.mark.gpu
def test_plain_bench_run_is_lean(tmp_path):
    """A plain `bench.py --gpus 1 --steps N --warmup W` on the real model: one timed repeat of exactly N steps, the dump of
    the final latents, none of the --full records (calibration, rocm-smi state, sustained leg, roofline / profile, end-to-end
    latency, CPU baseline), and at most 30 s of the whole run - a fresh process, start to exit - outside its N + W steps."""
    import subprocess
    import sys
    import time

    import numpy as np
    steps, warmup = 10, 2
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                        str(warmup), "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, timeout=300, cwd=ROOT)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["unit"] == "it/s" and d["higher_is_better"] is True and d["dtype"] == "fp16" and "SD2.1-base 512x512" in d["metric"]
    assert d["steps"] == steps and d["warmup"] == warmup and d["repeats"] == 1 and len(d["repeats_ms_per_step"]) == 1
    assert d["ms_per_step"] > 0 and abs(d["value"] - 1e3 / d["ms_per_step"]) <= 1e-3 * d["value"] + 0.01
    assert not {"roofline", "gpu_state", "calibration", "cpu_baseline", "concurrent_prompts"} & set(d), sorted(d)
    assert d["sustained_leg"] is None and "latency_prompt_to_image_s" not in d["e2e"]
    lat = np.load(tmp_path / "out" / "latents.npy")
    assert lat.dtype == np.float32 and lat.shape == (1, 4, 64, 64) and np.isfinite(lat).all()
    outside = wall - (steps + warmup) * d["ms_per_step"] * 1e-3
    print(f"plain bench run: {wall:.1f} s start to exit, {outside:.1f} s outside its steps")
    assert outside <= 30.0, outside
