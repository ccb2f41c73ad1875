"""CPU suite: the sub-pixel form of the upsampler conv (plan tile 21, csrc/conv3x3_halo_sp.hip) - the host fold of its weights
(weight_prep.h subpixel_fold through sd_op_subpixel_fold), the planner's case for it and the stand-alone sanitizer program.  No GPU."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from python_hip_stable_diffusion import _lib

FOLD_SHAPES = [(4, 64), (72, 192), (64, 128)]      # (Cout, Cin)
# ky (or kx) taps that land on fold position d of phase bit a: the low-res row floor((a + k - 1) / 2) = a + d - 1
SRC = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}


def numpy_fold(w, acc):
    """(Cout, Cin, 3, 3) -> (4, Cout, 4, Cin) in dtype `acc`: sequential sums in (ky, kx) order, no rounding besides acc's own."""
    cout, cin = w.shape[:2]
    out = np.zeros((4, cout, 4, cin), acc)
    for p in range(4):
        a, b = p >> 1, p & 1
        for t in range(4):
            dy, dx = t >> 1, t & 1
            s = np.zeros((cout, cin), acc)
            for ky in SRC[(a, dy)]:
                for kx in SRC[(b, dx)]:
                    s = (s + w[:, :, ky, kx].astype(acc)).astype(acc)
            out[p, :, t, :] = s
    return out


@pytest.mark.parametrize("cout,cin", FOLD_SHAPES)
@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_fold_equals_numpy_bit_for_bit(sdlib, cout, cin, dtype):
    """fp32 sums of the store's values, ONE rounding to fp16 - from fp32 and from fp16 source values."""
    rs = np.random.RandomState(cout * 1000 + cin)
    w = (rs.randn(cout, cin, 3, 3) / np.sqrt(9 * cin)).astype(dtype)
    got = _lib.subpixel_fold(w)
    want = numpy_fold(w, np.float32).astype(np.float16)
    assert got.shape == (4, cout, 4, cin) and got.dtype == np.float16
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16))


def _upsample_conv64(x, w):
    """float64 reference: nearest x2, zero pad 1, 3x3 conv; also the same sums over |x| |w| (the bound's scale)."""
    up = x.repeat(2, axis=2).repeat(2, axis=3)
    B, C, H, W = up.shape
    pad = np.zeros((B, C, H + 2, W + 2))
    pad[:, :, 1:-1, 1:-1] = up
    out = np.zeros((B, w.shape[0], H, W))
    for ky in range(3):
        for kx in range(3):
            out += np.einsum("bchw,nc->bnhw", pad[:, :, ky:ky + H, kx:kx + W], w[:, :, ky, kx])
    return out


def _phase_convs64(x, f):
    """the four 2x2 convs on the low-res image with folded weights f (4, N, 4, C): tap (dy, dx) of phase (a, b) at offset (a + dy - 1, b + dx - 1)"""
    B, C, H, W = x.shape
    pad = np.zeros((B, C, H + 2, W + 2))
    pad[:, :, 1:-1, 1:-1] = x
    out = np.zeros((B, f.shape[1], 2 * H, 2 * W))
    for p in range(4):
        a, b = p >> 1, p & 1
        for t in range(4):
            dy, dx = t >> 1, t & 1
            out[:, :, a::2, b::2] += np.einsum("bchw,nc->bnhw", pad[:, :, a + dy:a + dy + H, b + dx:b + dx + W], f[p, :, t, :])
    return out


@pytest.mark.parametrize("B,C,H,W,N", [(2, 8, 8, 8, 4), (1, 6, 8, 12, 5), (1, 4, 3, 5, 2)])
def test_phase_convs_equal_upsample_conv_in_float64(B, C, H, W, N):
    """The identity, borders included.  Both sides are float64 sums of the same real number, of at most 9 C products each (the fold adds
    at most 3 roundings of partial sums of the same terms): each is within gamma_n sum |x||w| of it, n = 9 C + 4, so they differ by at
    most 2 n eps sum |x||w| - the float64 bound of the sum, no free constant."""
    rs = np.random.RandomState(B * 100 + C)
    x = rs.randn(B, C, H, W)
    w = rs.randn(N, C, 3, 3)
    ref = _upsample_conv64(x, w)
    got = _phase_convs64(x, numpy_fold(w, np.float64))
    scale = _upsample_conv64(np.abs(x), np.abs(w))
    n = 9 * C + 4
    bound = 2 * n * np.finfo(np.float64).eps * scale
    diff = np.abs(got - ref)
    print(f"worst |phase convs - upsample conv| = {diff.max():.3e} (bound at that element {bound.flat[diff.argmax()]:.3e})")
    assert np.all(diff <= bound)


# ---- planner ----
SD21_UPSAMPLERS = [(1280, 1280, 2, 8, 8), (1280, 1280, 2, 16, 16), (640, 640, 2, 32, 32)]     # (C0, N, B, Hi, Wi): up_blocks.{0,1,2}
SMALL_SHAPES = [(128, 64, 2, 8, 8), (192, 72, 1, 8, 12), (64, 64, 1, 16, 16), (256, 128, 2, 24, 16), (1280, 8, 1, 8, 8)]


def _plan(c0, n, b, hi, wi, **kw):
    return _lib.conv_plan(3, 1, 2, c0, 0, n, b, 2 * hi, 2 * wi, **kw)


@pytest.mark.parametrize("c0,n,b,hi,wi", SD21_UPSAMPLERS + SMALL_SHAPES)
def test_flagged_upsamplers_answer_tile_21(sdlib, c0, n, b, hi, wi):
    p = _plan(c0, n, b, hi, wi, flags=16 | 64)
    assert p["tile"] == 21 and p["kernel"] == "conv3x3_halo_sp ring4" and p["copies"] == (False, False, False)
    assert p["splitk"] >= 1 and p["slab"] == (p["splitk"] > 1)
    assert p["workspace_bytes"] == (p["splitk"] * b * 4 * hi * wi * n * 4 if p["slab"] else 0)      # tile 7's slab arithmetic
    p3 = _plan(c0, n, b, hi, wi, flags=16 | 64, staging=2, splitk=2)
    assert p3["tile"] == 21 and p3["kernel"] == "conv3x3_halo_sp ring3" and p3["splitk"] == min(2, c0 // 64)
    # without the flag nothing moves: the library's own answer is not tile 21, and a pinned tile 7 is tile 7
    plain = _plan(c0, n, b, hi, wi, flags=16)
    assert plain["tile"] != 21 and "halo_sp" not in plain["kernel"]
    assert _plan(c0, n, b, hi, wi, flags=16, tile=7, staging=3)["kernel"] == "halo_ks ring4"


def test_unflagged_upsampler_rows_answer_what_the_golden_holds(sdlib):
    """every recorded up = 2 3x3 row of tests/golden/conv_plans.json, the three SD2.1-base upsamplers among them"""
    with open(os.path.join(GOLDEN, "conv_plans.json")) as f:
        g = json.load(f)
    fields = g["desc_fields"]
    n = len(fields)
    rows = [r for r in g["launch_rows"] + g["extra_launch_rows"] if r[0] == 3 and r[fields.index("up")] == 2]
    keys = {(r[fields.index("C0")], r[fields.index("N")], r[fields.index("B")], r[fields.index("Ho")]) for r in rows}
    assert {(1280, 1280, 2, 16), (1280, 1280, 2, 32), (640, 640, 2, 64)} <= keys, sorted(keys)
    for r in rows:
        p = _lib.conv_plan(**dict(zip(fields, r[:n])))
        assert [p["tile"], p["staging"], p["splitk"], int(p["slab"]), p["workspace_bytes"]] == r[n:n + 5], r


@pytest.mark.parametrize("kw,why", [
    (dict(C1=64), "second source"),
    (dict(stride=2), "stride"),
    (dict(up=1), "up is not 2"),
    (dict(Wi=4), "Wi < 8"),
    (dict(Hi=4), "Hi < 8"),
    (dict(C0=96), "C0 is no multiple of 64"),
    (dict(out_mode=2), "GEGLU"),
    (dict(out_mode=1), "transposed"),
    (dict(ksize=1), "not a 3x3"),
])
def test_halo_sp_ok_refuses_and_names_the_reason(sdlib, kw, why):
    base = dict(C0=128, N=64, B=1, Hi=8, Wi=8)
    assert _lib.subpixel_refusal(**base) == ""
    args = dict(base, **kw)
    assert why in _lib.subpixel_refusal(**args)
    # the planner refuses the flagged descriptor with the same words
    up, stride = args.get("up", 2), args.get("stride", 1)
    with pytest.raises(ValueError, match="plan tile 21"):
        _lib.conv_plan(args.get("ksize", 3), stride, up, args["C0"], args.get("C1", 0), args["N"], args["B"], args["Hi"] * up // stride,
                       args["Wi"] * up // stride, out_mode=args.get("out_mode", 0), flags=64)


# ---- sanitizer ----
def test_fold_runs_clean_under_the_sanitizers(tmp_path):
    """weight_prep.h's fold and its refusals in a stand-alone program (tools/subpixel_host_check.cpp) under -fsanitize=address,undefined."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "subpixel_host_check")
    build = subprocess.run([hipcc, "--offload-arch=gfx950", "-x", "hip", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                            "-Xarch_host", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "ml-stable-diffusion_amd", "csrc"),
                            os.path.join(ROOT, "tools", "subpixel_host_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "subpixel host check OK" in run.stdout, run.stdout[-2000:] + run.stderr[-3000:]
