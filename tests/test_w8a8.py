"""CPU suite: the host side of W8A8 (activation_quantization.py:141-203 of the reference: symmetric int8, per-output-channel weights,
per-tensor activations; parity with coremltools' quantizer unpinned).  The weight quantizer and the packer of the int8 weight stream
against numpy restatements bit for bit, the store's marks, the recipe files, the plan tile and its name - nothing here needs a GPU."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from python_hip_stable_diffusion import HipModel, _lib, activation_quantization as aq, hip_model


# ---- quantizer ----
def quantize_ref(w):
    """s_w[n] = absmax_n / 127 (an all-zero row: 1), q = clip(rint(w / s_w[n]), -127, 127): fp32 division, ties to even"""
    w = np.asarray(w, np.float32)
    rows = w.reshape(w.shape[0], -1)
    amax = np.abs(rows).max(axis=1).astype(np.float32)
    s = np.where(amax > 0, amax / np.float32(127.0), np.float32(1.0)).astype(np.float32)
    q = np.clip(np.rint(rows / s[:, None]), -127, 127).astype(np.int8)
    return q.reshape(w.shape), s


def test_quantizer_equals_the_numpy_restatement_bit_for_bit():
    rs = np.random.RandomState(5)
    w = rs.randn(12, 4, 3, 3).astype(np.float32)
    w[0] = 0.0                                                                   # an all-zero row: scale 1, all zeros
    w[1] = np.abs(w[1]) * 0.5
    w[1, 2, 1, 1] = -3.0                                                         # a row whose absmax is a negative element
    w[2] = 0.0                                                                   # exact .5 ties of both parities: absmax 127 -> scale 1
    w[2].reshape(-1)[:8] = [127.0, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 126.5]
    w[3].reshape(-1)[:2] = [65504.0, -65504.0]                                   # +-65504
    w[4] = 0.0
    w[4].reshape(-1)[:3] = [-65504.0, 65504.0 / 254.0, 3 * 65504.0 / 254.0]      # ties at a scale that is no power of two
    q, s, err = _lib.quantize_weight(w)
    qr, sr = quantize_ref(w)
    assert q.dtype == np.int8 and s.dtype == np.float32
    assert np.array_equal(s.view(np.uint32), sr.view(np.uint32))
    assert np.array_equal(q, qr)
    assert s[0] == 1.0 and not q[0].any()
    assert q[1, 2, 1, 1] == -127 and q[1].max() < 127
    assert list(q[2].reshape(-1)[:8]) == [127, 0, 2, 2, 0, -2, -2, 126]          # round half to even
    assert list(q[3].reshape(-1)[:2]) == [127, -127] and q.min() >= -127
    want = float(((w.astype(np.float64) - qr.astype(np.float64) * sr.astype(np.float64).reshape(-1, 1, 1, 1)) ** 2).sum())
    assert abs(err - want) <= 1e-9 * max(1.0, want)
    with pytest.raises(ValueError):
        bad = w.copy()
        bad[5, 0, 0, 0] = np.inf
        _lib.quantize_weight(bad)


# ---- packer ----
def pack_ref(q):
    """[Cout / 32][Ctot / 32][taps][64 lanes][16]: lane l of (strip, slice, tap) holds row strip * 32 + (l & 31), channels
    slice * 32 + (l >> 5) * 16 + (0 .. 15)"""
    Cout, Ctot, k, _ = q.shape
    out = np.zeros((Cout // 32, Ctot // 32, k * k, 64, 16), np.int8)
    flat = q.reshape(Cout, Ctot, k * k)
    for strip in range(Cout // 32):
        for sl in range(Ctot // 32):
            for lane in range(64):
                n, c0 = strip * 32 + (lane & 31), sl * 32 + (lane >> 5) * 16
                out[strip, sl, :, lane, :] = flat[n, c0:c0 + 16, :].T
    return out


@pytest.mark.parametrize("shape", [(32, 64, 3), (64, 192, 3), (32, 64, 1)])
def test_packer_equals_the_numpy_restatement(shape):
    Cout, Ctot, k = shape
    q = np.random.RandomState(Cout + Ctot + k).randint(-127, 128, size=(Cout, Ctot, k, k)).astype(np.int8)
    got = _lib.w8a8_pack(q)
    assert got.shape == (Cout // 32, Ctot // 32, k * k, 64, 16) and got.dtype == np.int8
    assert np.array_equal(got, pack_ref(q))
    with pytest.raises(ValueError):
        _lib.w8a8_pack(q[:, :48])                                                # 48 channels: no whole slices


# ---- store ----
def small_store():
    rs = np.random.RandomState(1)
    return hip_model.Weights({"a.weight": rs.randn(32, 64, 3, 3).astype(np.float16), "a.bias": rs.randn(32).astype(np.float32),
                              "lin.weight": rs.randn(32, 64).astype(np.float16), "b.weight": rs.randn(32, 64, 1, 1).astype(np.float16)})


def test_store_marks_and_refusals():
    w = small_store()
    assert w.w8a8_info("a.weight") is None
    with pytest.raises(KeyError):
        w.quantize_w8a8("missing.weight", 1.0)
    for name in ("a.bias", "lin.weight"):                                        # not a conv weight
        with pytest.raises(ValueError, match="not a conv weight"):
            w.quantize_w8a8(name, 1.0)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="act_absmax"):
            w.quantize_w8a8("a.weight", bad)
    assert w.w8a8_info("a.weight") is None                                       # a refused call marks nothing
    err = w.quantize_w8a8("a.weight", 6.35)
    q, s = quantize_ref(w.read("a.weight"))
    want = float(((w.read("a.weight").astype(np.float64) - q * s.astype(np.float64).reshape(-1, 1, 1, 1)) ** 2).sum())
    assert err > 0 and abs(err - want) <= 1e-9 * want
    assert w.w8a8_info("a.weight") == float(np.float32(6.35) / np.float32(127.0))   # round trip: s_a
    assert w.w8a8_info("b.weight") is None
    with pytest.raises(ValueError, match="W8A8"):                                # W8A8 + palette on one tensor, either order
        w.palettize("a.weight", 4)
    w.palettize("b.weight", 4)
    with pytest.raises(ValueError, match="palette"):
        w.quantize_w8a8("b.weight", 1.0)
    assert np.array_equal(w.read("a.weight"), small_store().read("a.weight"))   # the mark leaves the fp16 values alone
    w.add("a.weight", np.zeros((32, 64, 3, 3), np.float16))                      # new values: the mark is gone
    assert w.w8a8_info("a.weight") is None
    w.close()


# ---- recipe ----
def test_recipe_round_trip_and_checks(tmp_path):
    ranges = {"mid.conv1": 3.25, "mid.conv2.weight": 0.125, "up.conv": 7.0}
    recipe = aq.recipe_from_ranges(ranges, skip=("up.conv",))
    assert recipe == {"mid.conv1": 3.25, "mid.conv2": 0.125}
    path = tmp_path / "recipe.json"
    aq.save_recipe(recipe, path)
    assert json.load(open(path)) == recipe and aq.load_recipe(str(path)) == recipe and aq.load_recipe(recipe) == recipe
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            aq.recipe_from_ranges({"x": bad})
        with pytest.raises(ValueError):
            aq.load_recipe({"x": bad})
    w = small_store()
    with pytest.raises(KeyError, match="nope"):
        aq.apply(w, {"a": 1.0, "nope": 1.0})
    assert w.w8a8_info("a.weight") is None                                       # nothing marked by the refused recipe
    errs = aq.apply(w, {"a": 2.0})
    assert list(errs) == ["a"] and w.w8a8_info("a.weight") is not None
    w.close()


TINY = dict(block_out_channels=(32, 64), down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"), up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"),
            layers_per_block=1, attention_head_dim=(2, 4), cross_attention_dim=48, sample_size=16)


def test_hip_model_argument_conflicts_raise_without_a_gpu():
    w = small_store()
    with pytest.raises(ValueError, match="not both"):
        HipModel(TINY, w, activation_quantization={"a": 1.0}, observe_activations=True)
    with pytest.raises(ValueError, match="UNet only"):
        HipModel(TINY, w, kind="controlnet", activation_quantization={"a": 1.0})
    with pytest.raises(KeyError, match="nope"):                                  # a tensor the model does not have
        HipModel(TINY, w, activation_quantization={"nope": 1.0})
    with pytest.raises(ValueError, match="palettized"):                          # the palettization recipe covers the same tensor
        HipModel(TINY, w, palettization_recipe={"a": 4}, activation_quantization={"a": 1.0})
    w.close()
    big = {"a.weight": np.zeros((128, 128, 3, 3), np.float16)}
    with pytest.raises(ValueError, match="palettized"):                          # quantize_nbits covers it (every tensor > 1e5 elements)
        HipModel(TINY, big, quantize_nbits=4, activation_quantization={"a": 1.0})


# ---- plan ----
def test_plan_tile_17_and_its_kernel_name():
    for staging, waves, splits in ((0, 8, 5), (4, 4, 10)):
        p = _lib.conv_plan(3, 1, 1, 1280, 0, 1280, 2, 8, 8, flags=2 | 16, tile=17, staging=staging)
        assert (p["tile"], p["staging"], p["splitk"], p["slab"]) == (17, staging, splits, True), p
        assert p["kernel"] == f"wstream_i8 waves{waves}"
        assert p["workspace_bytes"] == splits * 128 * 1280 * 4
    assert _lib.conv_plan(1, 1, 1, 64, 0, 32, 1, 8, 9, tile=17)["kernel"] == "wstream_i8 waves8"       # the 1x1 form
    assert _lib.conv_plan(3, 1, 2, 64, 0, 32, 2, 8, 8, tile=17)["tile"] == 17                          # the folded upsample
    for desc in ((3, 1, 1, 64, 0, 32, 1, 8, 12), (3, 1, 1, 64, 0, 48, 1, 8, 8), (3, 2, 1, 64, 0, 32, 1, 8, 8), (3, 1, 1, 64, 0, 32, 1, 32, 32)):
        with pytest.raises(ValueError, match="plan tile 17"):                    # off the weight-stream shapes
            _lib.conv_plan(*desc, tile=17)
    # the tile is never the library's own answer: it takes a W8A8 descriptor
    assert _lib.conv_plan(3, 1, 1, 1280, 0, 1280, 2, 8, 8, flags=2 | 16)["tile"] == 9


# ---- sanitizer ----
def test_quantizer_and_packer_run_clean_under_the_sanitizers(tmp_path):
    """weight_prep.h's W8A8 host code in a stand-alone program (tools/w8a8_host_check.cpp) under -fsanitize=address,undefined."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "w8a8_host_check")
    build = subprocess.run([hipcc, "--offload-arch=gfx950", "-x", "hip", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                            "-Xarch_host", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "ml-stable-diffusion_amd", "csrc"), os.path.join(ROOT, "tools", "w8a8_host_check.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "w8a8 host check OK" in run.stdout, run.stdout[-2000:] + run.stderr[-3000:]
