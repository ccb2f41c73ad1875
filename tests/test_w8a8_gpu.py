"""GPU suite: W8A8 on the device (activation_quantization.py:141-203 of the reference: symmetric int8, per-output-channel weights,
per-tensor activations; parity with coremltools' quantizer unpinned).  The int8 weight-stream conv (plan tile 17) sums exact
integers, so with power-of-two scales the whole operator is exact and compared bit for bit; with random scales it is gated against a
float64 fake-quant reference whose integer part is the kernel's by construction.  Then the absmax observers, a calibrated handle
against a fake-quantizing oracle, and the two CLI flags.

Shapes: the geometries of tests/test_palettize_gpu.py (the forms of wstream_kernel: dead waves, a ragged last workgroup of
slices, three K splits, a second source, the upsample gather, the 16-pixel-wide form, ragged and multi-block M of the 1x1 form, and
the H != W images 16x8, 24x8 at batch 3 and 8x16)."""
import json
import os
import re

import numpy as np
import pytest

from oracle import psnr, unet_ref, weights
from python_hip_stable_diffusion import HipModel, _lib, activation_quantization as aq, hip_model
from test_palettize_gpu import CASES, TINY, gate, h16, tiny_inputs

pytestmark = pytest.mark.gpu


def conv_f64(xq, wq, ups):
    """exact integer convolution (float64 holds every sum: < 2^53) of (B, C, H, W) by (Cout, C, k, k), nearest x2 upsample first"""
    import torch
    import torch.nn.functional as F
    xt = torch.from_numpy(np.asarray(xq, np.float64))
    if ups:
        xt = F.interpolate(xt, scale_factor=2.0, mode="nearest")
    return F.conv2d(xt, torch.from_numpy(np.asarray(wq, np.float64)), padding=wq.shape[2] // 2).numpy()


def quantize_act(x, act_absmax):
    """the kernel's x_q, restated: clip(rint(fp32(x) * fp32(1 / s_a)), -127, 127), NaN -> 0, +-inf -> +-127"""
    s_a = np.float32(act_absmax) / np.float32(127.0)
    inv_s = np.float32(1.0) / s_a
    with np.errstate(invalid="ignore"):
        v = np.rint(x.astype(np.float32) * inv_s)
    return np.where(np.isnan(v), np.float32(0), np.clip(v, -127, 127)).astype(np.float64), s_a


def run_op(c, **kw):
    n = int(np.prod(c["shape"]))
    guard = 4 * c["shape"][3] * c["shape"][1]
    buf = np.full(n + guard, np.nan, np.float16)
    out, plan, _ = _lib.conv2d_w8a8(c["x"], c["wq"], c["w_scale"], c["act_absmax"], bias=c["bias"], res=c["res"], x1=c["x1"], upsample=c["ups"],
                                    nw=c["nw"], out=buf, **kw)
    out = out.copy()
    assert np.isnan(buf[n:]).all(), "the guard behind the output was written"
    assert not np.isnan(buf[:n]).any(), "the NaN prefill was not fully overwritten"
    nslices = c["wq"].shape[1] // 32
    assert plan == [17, 4 if c["nw"] == 4 else 0, -(-nslices // c["nw"]), 1], plan
    again, plan2, _ = _lib.conv2d_w8a8(c["x"], c["wq"], c["w_scale"], c["act_absmax"], bias=c["bias"], res=c["res"], x1=c["x1"],
                                       upsample=c["ups"], nw=c["nw"], iters=3)
    assert plan2 == plan and np.array_equal(out.view(np.uint16), again.view(np.uint16)), "two runs differ"
    return out


def reference(c):
    xs = c["x"] if c["x1"] is None else np.concatenate([c["x"], c["x1"]], axis=1)
    xq, s_a = quantize_act(xs, c["act_absmax"])
    acc = conv_f64(xq, c["wq"], c["ups"])
    cs = (s_a * c["w_scale"].astype(np.float32)).astype(np.float32)               # cs[n] = fp32(s_a * s_w[n]), as the host computes it
    return acc * cs.astype(np.float64).reshape(1, -1, 1, 1) + c["bias"].astype(np.float64).reshape(1, -1, 1, 1) + c["res"].astype(np.float64)


# ---- exact family ----
def make_exact_case(name):
    """s_a = 2^-3 and s_w[n] in {2^-4, 2^-5, 2^-6}: every activation is a multiple (or an exact .5 tie) of s_a, every slab element an
    integer times the output quantum cs[n] >= 2^-9, bias and residual multiples of 2^-7, every magnitude far below 2^14: all fp32 sums
    are exact whatever their order, and the output is float16(exact value)."""
    B, C0, C1, H, W, Cout, k, ups, nw = CASES[name]
    rs = np.random.RandomState(7000 + list(CASES).index(name))
    ctot = C0 + C1
    wq = rs.randint(-3, 4, size=(Cout, ctot, k, k)).astype(np.int8)              # random: no symmetry under n <-> c or tap flips
    wq.reshape(-1)[rs.choice(wq.size, 24, replace=False)] = np.array([-127, 127] * 12, np.int8)
    w_scale = (2.0 ** -rs.randint(4, 7, size=Cout)).astype(np.float32)
    ks = rs.randint(-8, 9, size=(B, ctot, H, W)).astype(np.float64)
    flat = ks.reshape(-1)
    pick = rs.choice(flat.size, 64, replace=False)
    flat[pick[:8]] = 127                                                         # the ends of the range
    flat[pick[8:16]] = -127
    flat[pick[16:24]] = [200, -200, 128, -128, 127.5, -127.5, 1000, -1000]       # values that clamp
    flat[pick[24:40]] = np.array([0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, -3.5, 126.5, -126.5, 125.5, -125.5, 6.5, 7.5, -6.5, -7.5])  # exact ties
    xs = h16(ks * 0.125)
    assert np.array_equal(xs.astype(np.float64), ks * 0.125)                     # all exactly representable in fp16
    flat16 = xs.reshape(-1)
    flat16[pick[40:44]] = np.float16(np.inf)                                     # saturate to +127
    flat16[pick[44:48]] = -np.float16(np.inf)                                    # ... and -127
    flat16[pick[48:56]] = np.float16(np.nan)                                     # become 0
    up = 2 if ups else 1
    bias = (rs.randint(-64, 65, size=Cout) * 2.0 ** -7).astype(np.float32)
    res = h16(rs.randint(-256, 257, size=(B, Cout, H * up, W * up)) * 2.0 ** -7)
    return dict(x=xs[:, :C0].copy(), x1=xs[:, C0:].copy() if C1 else None, wq=wq, w_scale=w_scale, act_absmax=np.float32(127 * 0.125), bias=bias,
                res=res, ups=ups, nw=nw, shape=(B, Cout, H * up, W * up))


@pytest.mark.parametrize("name", list(CASES))
def test_operator_exact_family_is_bit_identical_to_the_integer_convolution(name):
    c = make_exact_case(name)
    assert np.float32(c["act_absmax"]) / np.float32(127) == np.float32(0.125)
    out = run_op(c)
    want = reference(c)
    assert np.abs(want).max() < 2.0 ** 14 and np.array_equal(want * 512, np.rint(want * 512))   # what makes every fp32 sum exact
    want16 = want.astype(np.float16)
    assert np.array_equal(out.view(np.uint16), want16.view(np.uint16)), f"{name}: {np.count_nonzero(out != want16)} elements differ"


def test_special_values_saturate_or_vanish():
    """+-inf -> +-127, NaN -> 0, stated in wstream.hip (ws_quantize8): one channel of ones against each special input"""
    x = np.zeros((1, 64, 8, 8), np.float16)
    x[0, 0, 2, 3], x[0, 1, 4, 4], x[0, 2, 6, 1] = np.inf, -np.inf, np.nan
    wq = np.zeros((32, 64, 1, 1), np.int8)
    wq[:, :3, 0, 0] = 1
    out, _, _ = _lib.conv2d_w8a8(x, wq, np.ones(32, np.float32), 127.0)
    want = np.zeros((1, 32, 8, 8), np.float16)
    want[0, :, 2, 3], want[0, :, 4, 4] = 127, -127
    assert np.array_equal(out, want)


# ---- general family ----
def make_general_case(name):
    B, C0, C1, H, W, Cout, k, ups, nw = CASES[name]
    rs = np.random.RandomState(9000 + list(CASES).index(name))
    ctot = C0 + C1
    w = (rs.randn(Cout, ctot, k, k) / np.sqrt(ctot * k * k)).astype(np.float32)
    wq, w_scale, _ = _lib.quantize_weight(w)
    xs = h16(rs.randn(B, ctot, H, W) * (1 + rs.rand(1, ctot, 1, 1)))
    up = 2 if ups else 1
    return dict(x=xs[:, :C0].copy(), x1=xs[:, C0:].copy() if C1 else None, wq=wq, w_scale=w_scale,
                act_absmax=np.float32(np.abs(xs.astype(np.float32)).max()), bias=(0.1 * rs.randn(Cout)).astype(np.float32),
                res=h16(rs.randn(B, Cout, H * up, W * up)), ups=ups, nw=nw, shape=(B, Cout, H * up, W * up))


@pytest.mark.parametrize("name", list(CASES))
def test_operator_general_family_against_the_float64_fake_quant_reference(name):
    c = make_general_case(name)
    out = run_op(c)
    gate(out, reference(c), f"W8A8 {name}")


def test_operator_refusals():
    rs = np.random.RandomState(0)
    ok = rs.randint(-127, 128, size=(32, 64, 3, 3)).astype(np.int8)
    sc = np.full(32, 0.01, np.float32)
    x = h16(rs.randn(1, 64, 8, 8))
    _lib.conv2d_w8a8(x, ok, sc, 4.0)
    with pytest.raises(ValueError):                                             # 12-pixel-wide image: not a weight-stream shape
        _lib.conv2d_w8a8(h16(rs.randn(1, 64, 8, 12)), ok, sc, 4.0)
    with pytest.raises(ValueError):                                             # 32 input channels: off the MFMA path
        _lib.conv2d_w8a8(h16(rs.randn(1, 32, 8, 8)), ok[:, :32], sc, 4.0)
    with pytest.raises(ValueError):                                             # 48 output channels
        _lib.conv2d_w8a8(x, rs.randint(-127, 128, size=(48, 64, 3, 3)).astype(np.int8), np.full(48, 0.01, np.float32), 4.0)
    with pytest.raises(ValueError):
        _lib.conv2d_w8a8(x, ok, sc, 4.0, nw=2)
    bad = ok.copy()
    bad[5, 7, 1, 1] = -128
    with pytest.raises(ValueError, match="-128"):                                # outside the symmetric range
        _lib.conv2d_w8a8(x, bad, sc, 4.0)
    for absmax in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="act_absmax"):
            _lib.conv2d_w8a8(x, ok, sc, absmax)
    with pytest.raises(ValueError, match="w_scale"):
        _lib.conv2d_w8a8(x, ok, np.zeros(32, np.float32), 4.0)


# ---- absmax ----
@pytest.mark.parametrize("n", [1, 63, 64, 65, 8 * 8 * 64])
def test_absmax_is_numpys(n):
    rs = np.random.RandomState(n)
    for where in sorted({0, n - 1, n // 2}):
        x = h16(rs.randn(n))
        x[where] = np.float16(-9.25 if where % 2 else 9.25)                      # the maximum at the first, last and a middle position
        got = _lib.absmax(x)
        assert got.dtype == np.float32 and got == np.abs(x.astype(np.float32)).max() == np.float32(9.25)
    x = h16(rs.randn(n))
    assert _lib.absmax(x) == np.abs(x.astype(np.float32)).max()
    assert _lib.absmax(np.zeros(n, np.float16)) == 0.0


def test_selftest_passes_with_the_int8_case():
    assert _lib.lib().sd_selftest_mfma() == 0


# ---- handles ----
def tiny_state():
    sd16 = weights.make_state_dict(unet_ref.unet_param_shapes(TINY), seed=33, dtype=np.float16)
    return sd16, weights.to_torch({k: v.astype(np.float32) for k, v in sd16.items()})


def oracle_forward(sd_t, hook=None):
    """unet_ref.unet_forward on the tiny inputs; hook(sd, name, x, orig, **kw) replaces unet_ref.conv for the call"""
    import torch
    inp = tiny_inputs()
    orig = unet_ref.conv
    if hook is not None:
        unet_ref.conv = lambda sd, name, x, stride=1, padding=0: hook(sd, name, x, orig, stride=stride, padding=padding)
    try:
        return unet_ref.unet_forward(sd_t, TINY, torch.from_numpy(inp["sample"].astype(np.float32)), torch.from_numpy(inp["timestep"].astype(np.float32)),
                                     torch.from_numpy(inp["encoder_hidden_states"].astype(np.float32))).numpy()
    finally:
        unet_ref.conv = orig


def forward_twice(model):
    inp = tiny_inputs()
    return [model(**inp)["noise_pred"].copy() for _ in range(2)]


@pytest.fixture(scope="module")
def calibration():
    """One observing handle and one plain handle, eager and graph, and the oracle's ranges of the same conv inputs."""
    sd16, sd_t = tiny_state()
    r = {"outs": {}, "ranges": {}}
    for use_graph in (False, True):
        obs = HipModel(TINY, sd16, batch=2, use_graph=use_graph, observe_activations=True)
        plain = HipModel(TINY, sd16, batch=2, use_graph=use_graph)
        r["outs"][use_graph] = (forward_twice(obs), forward_twice(plain))
        r["ranges"][use_graph] = obs.activation_ranges()
        r["plain_ranges"] = plain.activation_ranges()
        r["labels"] = [lab for lab, _, _ in obs.profile(1)]
        obs.close()
        plain.close()
    seen = {}

    def spy(sd, name, x, orig, **kw):
        seen[name] = max(seen.get(name, 0.0), float(x.abs().max()))
        return orig(sd, name, x, **kw)

    r["oracle_out"] = oracle_forward(sd_t, spy)
    r["oracle_ranges"] = seen
    r["sd16"], r["sd_t"] = sd16, sd_t
    return r


# the largest relative deviation of an observed range from the oracle's, measured on the MI355X (LAB_NOTES.md round 23): the handle
# stores fp16 activations of a model that matches the oracle to ~60 dB.  Gate: four times that, and never above 5 %
RANGE_DEV_MEASURED = 1.06e-3    # mid_block.resnets.0.conv2: 4.2227 observed, 4.2182 in the oracle; the other seven layers 3e-5 .. 7e-4
RANGE_DEV_GATE = 0.05


def test_observing_handle_sees_the_oracles_ranges_and_changes_nothing(calibration):
    r = calibration
    for use_graph in (False, True):
        obs, plain = r["outs"][use_graph]
        assert np.isfinite(obs[0]).all()
        for a in obs + plain[1:]:                                                # the observers write nothing the model reads; replay == eager
            assert np.array_equal(a, plain[0])
    assert np.array_equal(r["outs"][False][0][0], r["outs"][True][0][0])
    ranges = r["ranges"][False]
    assert len(ranges) >= 1 and ranges == r["ranges"][True] and r["plain_ranges"] == {}
    assert sum(1 for lab in r["labels"] if lab.startswith("absmax ")) == len(ranges)
    devs = {k: abs(v - r["oracle_ranges"][k]) / r["oracle_ranges"][k] for k, v in ranges.items()}
    print("observed ranges vs oracle:", {k: (round(v, 4), round(r["oracle_ranges"][k], 4), f"{devs[k]:.2e}") for k, v in ranges.items()})
    gate_ = RANGE_DEV_GATE if RANGE_DEV_MEASURED is None else min(RANGE_DEV_GATE, 4 * RANGE_DEV_MEASURED)
    assert max(devs.values()) <= gate_, devs


def fake_quant_hook(recipe, sd16):
    """unet_ref.conv with input and weight of the recipe's layers fake-quantized (the W8A8 scheme in float)"""
    import torch
    wfq = {}
    for layer in recipe:
        q, s, _ = _lib.quantize_weight(sd16[layer + ".weight"].astype(np.float32))
        wfq[layer] = torch.from_numpy(q.astype(np.float32) * s.reshape(-1, 1, 1, 1))

    def hook(sd, name, x, orig, **kw):
        if name not in recipe:
            return orig(sd, name, x, **kw)
        s_a = np.float32(recipe[name]) / np.float32(127.0)
        xq = torch.clamp(torch.round(x * float(np.float32(1.0) / s_a)), -127, 127) * float(s_a)
        return orig({name + ".weight": wfq[name], name + ".bias": sd[name + ".bias"]}, name, xq, **kw)

    return hook


# PSNR of the W8A8 handle against the fake-quantizing oracle measured on the MI355X (LAB_NOTES.md round 23); the gate is the project's
# rule, measured - 6 dB
W8A8_PSNR_MEASURED = 51.44      # (the fp16 handle against the same oracle: 49.86 dB; against the plain fp32 oracle: 67.35 dB)


def test_w8a8_handle_follows_the_fake_quant_oracle(calibration):
    r = calibration
    sd16 = r["sd16"]
    recipe = aq.recipe_from_ranges(r["ranges"][False])
    outs, info = {}, {}
    for use_graph in (False, True):
        m = HipModel(TINY, sd16, batch=2, use_graph=use_graph, activation_quantization=recipe)
        outs[use_graph] = forward_twice(m)
        info[use_graph] = (m.w8a8_info(), m.w8a8_layers(), m.arena_used_bytes, [lab for lab, _, _ in m.profile(1)])
        m.close()
    plain_model = HipModel(TINY, sd16, batch=2)
    plain_used = plain_model.arena_used_bytes
    plain_model.close()
    (n_marked, n_applied, nbytes), layers, used, labels = info[True]
    assert info[False][0] == info[True][0] and n_applied >= 1 and n_applied == n_marked == len(recipe) and sorted(layers) == sorted(recipe)
    for a in outs[False] + outs[True]:                                           # eager twice, graph capture + replay: bit for bit
        assert np.isfinite(a).all() and np.array_equal(a, outs[False][0])
    marked = [re.search(r"^\S+\+w8a8 \d+->(\d+) .* K=(\d+) (\S+) ", lab) for lab in labels]
    applied_weights = [int(m.group(1)) * int(m.group(2)) for m in marked if m]
    assert len(applied_weights) == n_applied and sorted(m.group(3) for m in marked if m) == sorted(recipe)
    # an applied conv dropped both fp16 copies (4 B per weight) and holds 1 B per weight plus 4 B per output channel: `nbytes`;
    # four allocations per layer, each rounded up to the arena's 256 bytes
    assert nbytes == sum(applied_weights) + 4 * sum(int(m.group(1)) for m in marked if m)
    assert abs((plain_used - used) - (4 * sum(applied_weights) - nbytes)) <= 512 * n_applied, (plain_used, used, nbytes)
    # parity, free of parameters: the handle is closer to the fake-quantizing oracle than the fp16 handle is
    w8a8, plain = outs[True][0], r["outs"][True][1][0]
    assert not np.array_equal(w8a8, plain)
    fq = oracle_forward(r["sd_t"], fake_quant_hook(recipe, sd16))
    p_w8a8, p_plain = psnr.compute_psnr(w8a8, fq), psnr.compute_psnr(plain, fq)
    print(f"tiny UNet, {n_applied} W8A8 layers: PSNR vs the fake-quant oracle {p_w8a8:.2f} dB (the fp16 handle: {p_plain:.2f} dB); "
          f"fp16 handle vs the fp32 oracle {psnr.compute_psnr(plain, r['oracle_out']):.2f} dB")
    assert p_w8a8 > p_plain
    if W8A8_PSNR_MEASURED is not None:
        assert p_w8a8 >= W8A8_PSNR_MEASURED - 6.0


def test_recipe_with_an_ineligible_conv_leaves_it_fp16(calibration):
    recipe = dict(aq.recipe_from_ranges(calibration["ranges"][False]))
    skipped = "down_blocks.0.resnets.0.conv1"                                    # 32 channels at 16x16: not a weight-stream conv
    assert skipped not in recipe
    recipe[skipped] = 5.0
    m = HipModel(TINY, calibration["sd16"], batch=2, activation_quantization=recipe)
    out = forward_twice(m)[0]
    n_marked, n_applied, _ = m.w8a8_info()
    labels = [lab for lab, _, _ in m.profile(1)]
    m.close()
    assert np.isfinite(out).all() and n_marked == len(recipe) and n_applied == n_marked - 1
    lab = [x for x in labels if f" {skipped} " in x]
    assert len(lab) == 1 and "+w8a8" not in lab[0] and sum("+w8a8" in x for x in labels) == n_applied


# ---- pipeline ----
def test_cli_calibrates_then_applies_the_recipe(tmp_path, monkeypatch):
    from PIL import Image
    from python_hip_stable_diffusion import pipeline as P
    from test_text_encoder_gpu import write_checkpoint_dir
    root = str(tmp_path / "mini-sd")
    os.makedirs(root)
    write_checkpoint_dir(root)
    recipe_path = str(tmp_path / "w8a8.json")
    pipes = []
    real = P.get_hip_pipe
    monkeypatch.setattr(P, "get_hip_pipe", lambda *a, **kw: pipes.append(real(*a, **kw)) or pipes[-1])

    def generate(tag, *flags):
        args = P.build_parser().parse_args(["--prompt", "a photo of an astronaut riding a horse", "-i", root, "-o", str(tmp_path / tag), "--seed", "93",
                                            "--model-version", "mini/stable-diffusion", "--scheduler", "DDIM", "--num-inference-steps", "2",
                                            "--attention-implementation", "ORIGINAL", *flags])
        return np.array(Image.open(P.main(args)))

    plain = generate("plain")
    assert pipes[-1].unet.w8a8_info() == (0, 0, 0) and pipes[-1].unet.activation_ranges() == {}
    calibrated = generate("calib", "--calibrate-activations", recipe_path)
    assert np.array_equal(calibrated, plain)                                     # observing changes no image
    recipe = json.load(open(recipe_path))
    assert len(recipe) >= 1 and recipe == aq.recipe_from_ranges(pipes[-1].unet.activation_ranges())
    quant = generate("w8a8", "--activation-quantization-recipe", recipe_path)
    n_marked, n_applied, nbytes = pipes[-1].unet.w8a8_info()
    assert n_marked == len(recipe) and n_applied == n_marked and nbytes > 0 and sorted(pipes[-1].unet.w8a8_layers()) == sorted(recipe)
    assert quant.shape == plain.shape and not np.array_equal(quant, plain)       # the recipe really is applied
    print(f"mini pipeline, {n_applied} W8A8 layers: image PSNR vs fp16 {psnr.compute_psnr(quant.astype(np.float64), plain.astype(np.float64)):.1f} dB")
    with pytest.raises(ValueError):
        generate("both", "--calibrate-activations", recipe_path, "--activation-quantization-recipe", recipe_path)
