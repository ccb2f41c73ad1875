"""GPU suite: the upsampler conv as four 2x2 phase convs on the low-res image (plan tile 21, conv3x3_halo_sp.hip) through
sd_op_conv2d_subpixel, against plan tile 7 (the same conv with the upsample folded into the halo gather) and the float64 reference,
then a handle whose upsampler takes the new path (SD_UP_SUBPIX=2 in a child process) beside the same handle without it.

Exact family: integer activations in [-4, 4], weights and bias multiples of 2^-6 in [-1, 1) - the folded weights are exact in fp16 and
every fp32 partial sum is exact up to Cin = 1280, so tile 21, tile 7 and the rounded float64 reference agree bit for bit.
General family: N(0, 1) inputs, weights / sqrt(9 Cin), bias and residual, PSNR >= 60 dB against the float64 reference (the gate of the
3x3 operator tests of tests/test_ops_gpu.py).  Measured on the MI355X (LAB_NOTES.md round 28), tile 21 / tile 7 on the same inputs:
see GENERAL_PSNR_MEASURED below."""
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle import psnr, unet_ref, weights
from python_hip_stable_diffusion import HipModel, _lib, activation_quantization as aq

pytestmark = pytest.mark.gpu

# (B, Cin, Hi, Wi, N): the smallest shapes that reach each thing that can go wrong
SHAPES = {
    "half-empty tile, chunk boundary": (2, 128, 8, 8, 64),
    "ragged columns, N no multiple of 64: the weight-row clamp": (1, 192, 8, 12, 72),
    "one chunk only: the final-chunk instantiation alone": (1, 64, 16, 16, 64),
    "several tiles in y, ragged last; two n-tiles": (2, 256, 24, 16, 128),
    "longest K": (1, 1280, 8, 8, 8),
}
RINGS = {2: 3, 3: 4}      # plan tile 7's ring code -> stages of the sub-pixel kernel (every depth that is built)

# PSNR (dB) against the float64 reference on the general family, (tile 21, tile 7) per shape in the order of SHAPES, measured on the MI355X
GENERAL_PSNR_MEASURED = [(83.71, 84.79), (84.41, 85.50), (83.05, 84.21), (85.64, 87.39), (83.81, 85.60)]


def h16(a):
    return np.asarray(a, np.float32).astype(np.float16)


def upsample_conv64(x, w, bias=None, res=None):
    """float64: nearest x2, zero pad 1, 3x3 conv (+ bias, + residual)"""
    up = np.asarray(x, np.float64).repeat(2, axis=2).repeat(2, axis=3)
    B, C, H, W = up.shape
    pad = np.zeros((B, H + 2, W + 2, C))
    pad[:, 1:-1, 1:-1, :] = up.transpose(0, 2, 3, 1)
    w = np.asarray(w, np.float64)
    out = np.zeros((B, H, W, w.shape[0]))
    for ky in range(3):
        for kx in range(3):
            out += pad[:, ky:ky + H, kx:kx + W, :] @ w[:, :, ky, kx].T
    out = out.transpose(0, 3, 1, 2)
    if bias is not None:
        out = out + np.asarray(bias, np.float64)[None, :, None, None]
    if res is not None:
        out = out + np.asarray(res, np.float64)
    return out


@functools.lru_cache(maxsize=None)
def exact_case(name):
    """inputs, the float64 reference rounded to fp16 and tile 7's output: computed once per shape, shared by every ring / split-K case"""
    B, C, H, W, N = SHAPES[name]
    rs = np.random.RandomState(C * 31 + N)
    x = h16(rs.randint(-4, 5, (B, C, H, W)))
    w = h16(rs.randint(-64, 64, (N, C, 3, 3)) / 64.0)
    bias = (rs.randint(-64, 64, N) / 64.0).astype(np.float32)
    want = upsample_conv64(x, w, bias).astype(np.float16)
    tile7, _ = _lib.conv2d(x, w, bias, None, upsample=True, tile=37)
    for a in (x, w, bias, want, tile7):
        a.setflags(write=False)
    return x, w, bias, want, tile7


@pytest.mark.parametrize("splitk", [1, 2])
@pytest.mark.parametrize("staging", list(RINGS))
@pytest.mark.parametrize("name", list(SHAPES))
def test_exact_family_is_bit_identical_to_tile_7_and_the_float64_reference(name, staging, splitk):
    B, C, H, W, N = SHAPES[name]
    x, w, bias, want, tile7 = exact_case(name)
    assert np.array_equal(tile7.view(np.uint16), want.view(np.uint16)), "tile 7 against the rounded float64 reference"
    outs = []
    for _ in range(2):
        out, plan, _ = _lib.conv2d_subpixel(x, w, bias, None, splitk=splitk, staging=staging)
        assert plan[:3] == [21, staging, min(splitk, C // 64)] and plan[3] == int(plan[2] > 1), plan
        outs.append(out)
    # (the entry prefills the device output with NaN patterns and fails when the guard behind it was written)
    assert np.isfinite(outs[0]).all(), "an output element was not written"
    assert np.array_equal(outs[0].view(np.uint16), outs[1].view(np.uint16)), "two runs differ"
    assert np.array_equal(outs[0].view(np.uint16), tile7.view(np.uint16)), "tile 21 against tile 7"
    assert np.array_equal(outs[0].view(np.uint16), want.view(np.uint16)), "tile 21 against the rounded float64 reference"
    p = _lib.conv_plan(3, 1, 2, C, 0, N, B, 2 * H, 2 * W, flags=16 | 64, staging=staging, splitk=splitk)
    assert p["kernel"] == f"conv3x3_halo_sp ring{RINGS[staging]}"


def test_the_plans_own_split_k_and_ring():
    """staging 0 / splitk 0: four stages and tile 7's split rule over the phase grid (the longest-K shape has 4 workgroups: it splits)"""
    name = "longest K"
    x, w, bias, want, _ = exact_case(name)
    out, plan, _ = _lib.conv2d_subpixel(x, w, bias, None)
    assert plan[0] == 21 and plan[1] == 3 and plan[2] > 1 and plan[3] == 1, plan
    assert np.array_equal(out.view(np.uint16), want.view(np.uint16))


@pytest.mark.parametrize("idx,name", list(enumerate(SHAPES)))
def test_general_family_against_the_float64_reference(idx, name):
    B, C, H, W, N = SHAPES[name]
    rs = np.random.RandomState(C * 7 + N)
    x = h16(rs.randn(B, C, H, W))
    w = h16(rs.randn(N, C, 3, 3) / np.sqrt(9 * C))
    bias = (0.1 * rs.randn(N)).astype(np.float32)
    res = h16(rs.randn(B, N, 2 * H, 2 * W))
    ref = upsample_conv64(x, w, bias, res)
    out, plan, _ = _lib.conv2d_subpixel(x, w, bias, res)
    t7, _ = _lib.conv2d(x, w, bias, res, upsample=True, tile=37)
    p21, p7 = psnr.compute_psnr(out.astype(np.float64), ref), psnr.compute_psnr(t7.astype(np.float64), ref)
    print(f"general family {SHAPES[name]}: PSNR tile 21 {p21:.2f} dB, tile 7 {p7:.2f} dB, plan {plan}")
    assert plan[0] == 21 and np.isfinite(out).all()
    assert p21 >= 60.0      # (tile 7 beside it: GENERAL_PSNR_MEASURED[idx] - the folded weights carry one more fp16 rounding, 1.1 - 1.8 dB)


def test_operator_refusals_and_a_valid_call_right_after():
    x, w, bias, want, _ = exact_case("half-empty tile, chunk boundary")
    with pytest.raises(ValueError, match="Wi < 8"):
        _lib.conv2d_subpixel(x[:, :, :, :4], w)
    with pytest.raises(ValueError, match="C0 is no multiple of 64"):
        _lib.conv2d_subpixel(x[:, :96], w[:, :96])
    with pytest.raises(ValueError, match="staging"):
        _lib.conv2d_subpixel(x, w, staging=1)
    out, _, _ = _lib.conv2d_subpixel(x, w, bias)
    assert np.array_equal(out.view(np.uint16), want.view(np.uint16))


# ---- handle ----
# the two-level (64, 640) UNet of tests/test_palettize_gemm_gpu.py at batch 2: its one upsampler is 640 -> 640, 16x16 -> 32x32
CFG = unet_ref.make_config(sample_size=32, block_out_channels=(64, 640), down_block_types=(unet_ref.DN, unet_ref.CA),
                           up_block_types=(unet_ref.CAUP, unet_ref.UP), layers_per_block=1, attention_head_dim=(1, 10),
                           cross_attention_dim=128)
UPSAMPLER = "up_blocks.0.upsamplers.0.conv"
# PSNR of one forward against oracle/unet_ref.py, measured on the MI355X in two children of one run (LAB_NOTES.md round 28): the handle
# whose upsampler runs tile 21 (SD_UP_SUBPIX=2) and the same handle under SD_UP_SUBPIX=0.  Gate: measured - 6 dB, floor 60 dB.
HANDLE_PSNR_MEASURED = (69.21, 69.32)       # (SD_UP_SUBPIX=2, SD_UP_SUBPIX=0)


def handle_report():
    """runs inside a child process (the switch is read once per process): everything the handle test asserts, as JSON"""
    import torch
    sd16 = weights.make_state_dict(unet_ref.unet_param_shapes(CFG), seed=44, dtype=np.float16)
    hw = CFG["sample_size"]
    inp = dict(sample=weights.seeded_normal((2, 4, hw, hw), 1).astype(np.float16), timestep=np.array([981, 981], np.float16),
               encoder_hidden_states=weights.seeded_normal((2, CFG["cross_attention_dim"], 1, 77), 2).astype(np.float16))
    r = {}
    outs = []
    for use_graph in (False, True):
        m = HipModel(CFG, sd16, batch=2, use_graph=use_graph)
        outs += [m(**inp)["noise_pred"].copy() for _ in range(2)]
        r["labels"] = [lab for lab, _, _ in m.profile(1)]
        r["device_bytes"], r["used"] = m.device_bytes, m.arena_used_bytes
        m.close()
    r["replay_equals_eager"] = bool(all(np.isfinite(o).all() and np.array_equal(o, outs[0]) for o in outs))
    sd_t = weights.to_torch({k: v.astype(np.float32) for k, v in sd16.items()})
    ref = unet_ref.unet_forward(sd_t, CFG, torch.from_numpy(inp["sample"].astype(np.float32)), torch.from_numpy(inp["timestep"].astype(np.float32)),
                                torch.from_numpy(inp["encoder_hidden_states"].astype(np.float32))).numpy()
    r["psnr"] = float(psnr.compute_psnr(outs[0], ref))
    # an observing handle: the conv itself stays fp16, so its output is the plain handle's
    obs = HipModel(CFG, sd16, batch=2, observe_activations="all")
    r["observing_equals_plain"] = bool(np.array_equal(obs(**inp)["noise_pred"], outs[0]))
    r["observing_labels"] = [lab for lab, _, _ in obs.profile(1)]
    ranges = obs.activation_ranges()
    obs.close()
    # a W8A8-marked upsampler runs what it ran before: the int8 halo conv (plan tile 18)
    key = [k for k in ranges if UPSAMPLER in k]
    r["upsampler_observed"] = bool(key)
    if key:
        q = HipModel(CFG, sd16, batch=2, activation_quantization={aq.layer_of(key[0]): float(ranges[key[0]])})
        oq = q(**inp)["noise_pred"]
        r["w8a8_labels"] = [lab for lab, _, _ in q.profile(1) if UPSAMPLER in lab]
        r["w8a8_layers"] = list(q.w8a8_layers())
        r["w8a8_finite"] = bool(np.isfinite(oq).all())
        q.close()
    return r


def _child(mode):
    env = dict(os.environ, SD_TUNE="1", SD_UP_SUBPIX=str(mode))
    head = "import sys, json; sys.path[:0] = [%r, %r, %r]\n" % (ROOT, os.path.join(ROOT, "ml-stable-diffusion_amd"), os.path.join(ROOT, "tests"))
    code = "import test_subpixel_gpu as t\nprint('RESULT ' + json.dumps(t.handle_report()))\n"
    p = subprocess.run([sys.executable, "-c", head + code], env=env, capture_output=True, text=True, timeout=900)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert p.returncode == 0 and line, p.stdout[-2000:] + p.stderr[-2000:]
    return json.loads(line[0][len("RESULT "):])


def _upsampler_label(labels):
    labs = [lab for lab in labels if lab.startswith("conv3x3") and UPSAMPLER in lab]
    assert len(labs) == 1, labs
    return labs[0]


def test_handle_takes_the_sub_pixel_path_on_its_upsampler_only():
    new, old = _child(2), _child(0)
    lab_new, lab_old = _upsampler_label(new["labels"]), _upsampler_label(old["labels"])
    assert re.match(r"^conv3x3\+subpix 640->640 @32x32 M=2048 K=5760 \S+ #0,3,1,2,640,640,2048$", lab_new), lab_new
    assert "+subpix" not in lab_old and lab_old == lab_new.replace("+subpix", "")
    assert [lab for lab in new["labels"] if "+subpix" in lab] == [lab_new]              # nothing else moved
    assert [lab.replace("+subpix", "") for lab in new["labels"]] == old["labels"]
    assert not [lab for lab in old["observing_labels"] + old.get("w8a8_labels", []) if "+subpix" in lab]
    assert new["replay_equals_eager"] and old["replay_equals_eager"]
    assert new["observing_equals_plain"] and old["observing_equals_plain"]
    assert "+subpix" in _upsampler_label(new["observing_labels"])
    # a W8A8-marked upsampler still runs tile 18 under either mode
    for r in (new, old):
        assert r["upsampler_observed"] and r["w8a8_finite"] and len(r["w8a8_labels"]) == 1 and r["w8a8_labels"][0].startswith("conv3x3+w8a8 "), r.get("w8a8_labels")
        assert any(UPSAMPLER in n for n in r["w8a8_layers"])
    # (the folded matrix is 16/9 of the 3x3 one; under SD_TUNE the arena also reserves split-K slabs for a plan sweep of every conv a
    # candidate can move, which tile 21 is not - the two figures are reported, not compared)
    print(f"handle PSNR vs oracle/unet_ref.py: SD_UP_SUBPIX=2 {new['psnr']:.2f} dB, SD_UP_SUBPIX=0 {old['psnr']:.2f} dB; "
          f"arena used {new['used']} vs {old['used']} B, device_bytes {new['device_bytes']} vs {old['device_bytes']}")
    assert new["psnr"] >= 60.0
    if HANDLE_PSNR_MEASURED is not None:
        assert new["psnr"] >= max(HANDLE_PSNR_MEASURED[0] - 6.0, 60.0)
