"""GPU suite: the W8A8 halo conv (plan tile 18, conv3x3_halo_i8.hip) - the int8 form of the 3x3 / stride-1 halo kernel (plan tile 7)
with the semantics of the int8 weight stream (plan tile 17; tests/test_w8a8_gpu.py): exact int32 sums, so with power-of-two scales the
whole operator is exact and compared bit for bit; with random scales it is gated against the float64 fake-quant reference whose
integer part is the kernel's by construction.  Then handles whose recipes name convs of both int8 kernels, and the CLI's calibrate scope.

Shapes (B, C0, C1, H, W, Cout, upsample, split-K): one per mechanism of the kernel, named in SHAPES."""
import json
import os
import re

import numpy as np
import pytest

from oracle import psnr, unet_ref, weights
from python_hip_stable_diffusion import HipModel, _lib, activation_quantization as aq
from test_palettize_gpu import TINY, gate, h16
from test_w8a8_gpu import fake_quant_hook, reference

pytestmark = pytest.mark.gpu

SHAPES = {
    "one workgroup, one chunk: the last-chunk path alone": (1, 64, 0, 8, 16, 64, False, 1),
    "first + last chunk": (1, 128, 0, 8, 16, 64, False, 1),
    "steady state, both register parities, two samples": (2, 192, 0, 8, 16, 64, False, 1),
    "ragged tiles both ways, H != W": (1, 64, 0, 12, 24, 64, False, 1),
    "an image narrower than the tile": (1, 64, 0, 16, 8, 64, False, 1),
    "ragged last n-tile, clamped weight rows": (1, 64, 0, 8, 16, 96, False, 1),
    "N % 8 != 0: the element-wise store tail": (1, 64, 0, 8, 16, 68, False, 1),
    "second source 64 | 128": (1, 64, 128, 8, 16, 64, False, 1),
    "second source 128 | 64": (1, 128, 64, 8, 16, 64, False, 1),
    "upsample gather to 16x16": (2, 64, 0, 8, 8, 64, True, 1),
    "split-K through the slabs, even": (1, 256, 0, 8, 16, 64, False, 2),
    "split-K through the slabs, uneven, batch 3": (3, 320, 0, 8, 16, 64, False, 3),
}
STEADY = "steady state, both register parities, two samples"
RING_CODES = {0: 2, 2: 3, 3: 4}      # plan tile 7's ring code -> weight stages of the int8 kernel


def run_op(c, staging=3, plain=False):
    """the operator on case c (plain: no bias, no time embedding, no residual): NaN-prefilled output with a guard behind it, the plan,
    and a second run that must be bit-identical"""
    n = int(np.prod(c["shape"]))
    guard = 4 * c["shape"][3] * c["shape"][1]
    buf = np.full(n + guard, np.nan, np.float16)
    kw = dict(x1=c["x1"], upsample=c["ups"], staging=staging, splitk=c["splitk"])
    if not plain:
        kw.update(bias=c["bias"], temb=c["temb"], res=c["res"])
    out, plan, _ = _lib.conv2d_w8a8_halo(c["x"], c["wq"], c["w_scale"], c["act_absmax"], out=buf, **kw)
    out = out.copy()
    assert np.isnan(buf[n:]).all(), "the guard behind the output was written"
    assert not np.isnan(buf[:n]).any(), "the NaN prefill was not fully overwritten"
    nch = c["wq"].shape[1] // 64
    splits = -(-nch // -(-nch // c["splitk"]))
    assert plan == [18, staging, splits, int(splits > 1)], plan
    again, plan2, _ = _lib.conv2d_w8a8_halo(c["x"], c["wq"], c["w_scale"], c["act_absmax"], iters=3, **kw)
    assert plan2 == plan and np.array_equal(out.view(np.uint16), again.view(np.uint16)), "two runs differ"
    return out


def want_of(c, plain=False):
    """tests/test_w8a8_gpu.py reference (+ the time-embedding row); plain: the scaled integer convolution alone"""
    if plain:
        z = dict(c, bias=np.zeros_like(c["bias"]), res=np.zeros_like(c["res"]))
        return reference(z)
    return reference(c) + c["temb"].astype(np.float64)[:, :, None, None]


# ---- exact family ----
def make_exact_case(name):
    """The recipe of tests/test_w8a8_gpu.py make_exact_case on this file's shapes: s_a = 2^-3, s_w[n] in {2^-4, 2^-5, 2^-6}, activations
    multiples (or exact .5 ties) of s_a with +-127, clamping values, +-inf and NaN among them, weights in [-3, 3] with a few +-127, bias,
    time embedding and residual multiples of 2^-7: every fp32 sum is exact whatever its order."""
    B, C0, C1, H, W, Cout, ups, splitk = SHAPES[name]
    rs = np.random.RandomState(18000 + list(SHAPES).index(name))
    ctot = C0 + C1
    wq = rs.randint(-3, 4, size=(Cout, ctot, 3, 3)).astype(np.int8)
    wq.reshape(-1)[rs.choice(wq.size, 24, replace=False)] = np.array([-127, 127] * 12, np.int8)
    w_scale = (2.0 ** -rs.randint(4, 7, size=Cout)).astype(np.float32)
    ks = rs.randint(-8, 9, size=(B, ctot, H, W)).astype(np.float64)
    flat = ks.reshape(-1)
    pick = rs.choice(flat.size, 64, replace=False)
    flat[pick[:8]] = 127
    flat[pick[8:16]] = -127
    flat[pick[16:24]] = [200, -200, 128, -128, 127.5, -127.5, 1000, -1000]
    flat[pick[24:40]] = np.array([0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, -3.5, 126.5, -126.5, 125.5, -125.5, 6.5, 7.5, -6.5, -7.5])
    xs = h16(ks * 0.125)
    assert np.array_equal(xs.astype(np.float64), ks * 0.125)
    flat16 = xs.reshape(-1)
    flat16[pick[40:44]] = np.float16(np.inf)
    flat16[pick[44:48]] = -np.float16(np.inf)
    flat16[pick[48:56]] = np.float16(np.nan)
    up = 2 if ups else 1
    bias = (rs.randint(-64, 65, size=Cout) * 2.0 ** -7).astype(np.float32)
    temb = (rs.randint(-64, 65, size=(B, Cout)) * 2.0 ** -7).astype(np.float32)
    res = h16(rs.randint(-256, 257, size=(B, Cout, H * up, W * up)) * 2.0 ** -7)
    return dict(x=xs[:, :C0].copy(), x1=xs[:, C0:].copy() if C1 else None, wq=wq, w_scale=w_scale, act_absmax=np.float32(127 * 0.125), bias=bias,
                temb=temb, res=res, ups=ups, splitk=splitk, shape=(B, Cout, H * up, W * up))


def assert_exact(out, want, what):
    assert np.abs(want).max() < 2.0 ** 14 and np.array_equal(want * 512, np.rint(want * 512))   # what makes every fp32 sum exact
    want16 = want.astype(np.float16)
    assert np.array_equal(out.view(np.uint16), want16.view(np.uint16)), f"{what}: {np.count_nonzero(out != want16)} elements differ"


@pytest.mark.parametrize("name", list(SHAPES))
def test_operator_exact_family_is_bit_identical_to_the_integer_convolution(name):
    c = make_exact_case(name)
    assert np.float32(c["act_absmax"]) / np.float32(127) == np.float32(0.125)
    assert_exact(run_op(c), want_of(c), name)


@pytest.mark.parametrize("staging", list(RING_CODES))
def test_every_ring_depth_is_exact(staging):
    c = make_exact_case(STEADY)
    assert _lib.conv_plan(3, 1, 1, 192, 0, 64, 2, 8, 16, tile=18, staging=staging, splitk=1)["kernel"] == f"halo_i8 ring{RING_CODES[staging]}"
    assert_exact(run_op(c, staging=staging), want_of(c), f"ring code {staging}")


def test_without_bias_time_embedding_and_residual():
    c = make_exact_case(STEADY)
    assert_exact(run_op(c, plain=True), want_of(c, plain=True), "plain epilogue")
    c = make_exact_case("split-K through the slabs, even")
    assert_exact(run_op(c, plain=True), want_of(c, plain=True), "plain epilogue, slabs")


def test_the_librarys_split_k_rule_runs_too():
    c = dict(make_exact_case("split-K through the slabs, uneven, batch 3"), splitk=0)
    want = _lib.conv_plan(3, 1, 1, 320, 0, 64, 3, 8, 16, flags=2 | 4 | 16, tile=7, staging=3)
    out, plan, _ = _lib.conv2d_w8a8_halo(c["x"], c["wq"], c["w_scale"], c["act_absmax"], bias=c["bias"], temb=c["temb"], res=c["res"], staging=3, splitk=0)
    assert plan == [18, 3, want["splitk"], int(want["slab"])]
    assert_exact(out, want_of(c), "library split-K")


# ---- general family ----
def make_general_case(name):
    B, C0, C1, H, W, Cout, ups, splitk = SHAPES[name]
    rs = np.random.RandomState(19000 + list(SHAPES).index(name))
    ctot = C0 + C1
    w = (rs.randn(Cout, ctot, 3, 3) / np.sqrt(ctot * 9)).astype(np.float32)
    wq, w_scale, _ = _lib.quantize_weight(w)
    xs = h16(rs.randn(B, ctot, H, W) * (1 + rs.rand(1, ctot, 1, 1)))
    up = 2 if ups else 1
    return dict(x=xs[:, :C0].copy(), x1=xs[:, C0:].copy() if C1 else None, wq=wq, w_scale=w_scale,
                act_absmax=np.float32(np.abs(xs.astype(np.float32)).max()), bias=(0.1 * rs.randn(Cout)).astype(np.float32),
                temb=(0.1 * rs.randn(B, Cout)).astype(np.float32), res=h16(rs.randn(B, Cout, H * up, W * up)), ups=ups, splitk=splitk,
                shape=(B, Cout, H * up, W * up))


@pytest.mark.parametrize("name", list(SHAPES))
def test_operator_general_family_against_the_float64_fake_quant_reference(name):
    c = make_general_case(name)
    gate(run_op(c), want_of(c), f"W8A8 halo {name}")


def test_tile_18_is_the_same_function_as_tile_17():
    """a 16-pixel-wide shape both int8 kernels take: the same integers, the same scale, and the residual added to the fp32 value in front
    of the one rounding - in tile 17's slab combine and in tile 18's epilogue alike"""
    c = make_general_case(STEADY)
    o18 = run_op(dict(c, temb=np.zeros_like(c["temb"])))
    o17, plan, _ = _lib.conv2d_w8a8(c["x"], c["wq"], c["w_scale"], c["act_absmax"], bias=c["bias"], res=c["res"])
    assert plan[0] == 17 and np.array_equal(o18.view(np.uint16), o17.view(np.uint16))


# ---- refusals, in the order of the header ----
def test_operator_refusals():
    rs = np.random.RandomState(0)
    ok = rs.randint(-127, 128, size=(64, 64, 3, 3)).astype(np.int8)
    sc = np.full(64, 0.01, np.float32)
    x = h16(rs.randn(1, 64, 8, 16))
    _lib.conv2d_w8a8_halo(x, ok, sc, 4.0)
    lib = _lib.lib()
    out = np.empty(64 * 128, np.float16)
    args = lambda **kw: [kw.get("x", _lib.ptr(x)), None, kw.get("wq", _lib.ptr(ok)), kw.get("sc", _lib.fptr(sc)), 4.0, None, None, None,   # noqa: E731
                         kw.get("out", _lib.ptr(out)), kw.get("B", 1), 64, 0, 8, 16, 64, kw.get("up", 0), kw.get("staging", 3), 0, None, 1, None]
    assert lib.sd_op_conv2d_w8a8_halo(*args()) == 0
    for kw in (dict(x=None), dict(wq=None), dict(sc=None), dict(out=None), dict(B=0), dict(up=2), dict(staging=1), dict(staging=6)):
        assert lib.sd_op_conv2d_w8a8_halo(*args(**kw)) == -1, kw                 # SD_ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError, match="plan tile 18"):                        # 32 input channels: off the 64-channel chunks
        _lib.conv2d_w8a8_halo(h16(rs.randn(1, 32, 8, 16)), ok[:, :32], sc, 4.0)
    with pytest.raises(ValueError, match="plan tile 18"):                        # 66 output channels
        _lib.conv2d_w8a8_halo(x, rs.randint(-127, 128, size=(66, 64, 3, 3)).astype(np.int8), np.full(66, 0.01, np.float32), 4.0)
    with pytest.raises(ValueError, match="plan tile 18"):                        # a 4-row image
        _lib.conv2d_w8a8_halo(h16(rs.randn(1, 64, 4, 16)), ok, sc, 4.0)
    # the int32 bound comes before the values: an absurd act_absmax does not get a word in
    big = np.zeros((4, 14848, 3, 3), np.int8)
    with pytest.raises(ValueError, match="14784"):
        _lib.conv2d_w8a8_halo(np.zeros((1, 14848, 8, 8), np.float16), big, np.ones(4, np.float32), float("nan"))
    for absmax in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="act_absmax"):
            _lib.conv2d_w8a8_halo(x, ok, np.zeros(64, np.float32), absmax)        # ... and act_absmax before w_scale
    bad = ok.copy()
    bad[5, 7, 1, 1] = -128
    with pytest.raises(ValueError, match="w_scale"):
        _lib.conv2d_w8a8_halo(x, bad, np.zeros(64, np.float32), 4.0)             # ... and w_scale before the weight values
    with pytest.raises(ValueError, match="-128"):
        _lib.conv2d_w8a8_halo(x, bad, sc, 4.0)


# ---- handles ----
# a UNet whose fp16 plan holds plain, two-source and upsampling halo convs (the 64-channel 16x16 level) beside weight-stream convs
# (the 128-channel 8x8 level)
CFG = unet_ref.make_config(sample_size=16, block_out_channels=(64, 128), down_block_types=(unet_ref.CA, unet_ref.DN),
                           up_block_types=(unet_ref.UP, unet_ref.CAUP), layers_per_block=1, attention_head_dim=(2, 4), cross_attention_dim=48)


def cfg_inputs(cfg):
    hw = cfg["sample_size"]
    return dict(sample=weights.seeded_normal((2, 4, hw, hw), 1).astype(np.float16), timestep=np.array([981, 981], np.float16),
                encoder_hidden_states=weights.seeded_normal((2, cfg["cross_attention_dim"], 1, 77), 2).astype(np.float16))


def oracle_forward(cfg, sd_t, hook=None):
    import torch
    inp = cfg_inputs(cfg)
    orig = unet_ref.conv
    if hook is not None:
        unet_ref.conv = lambda sd, name, x, stride=1, padding=0: hook(sd, name, x, orig, stride=stride, padding=padding)
    try:
        return unet_ref.unet_forward(sd_t, cfg, torch.from_numpy(inp["sample"].astype(np.float32)), torch.from_numpy(inp["timestep"].astype(np.float32)),
                                     torch.from_numpy(inp["encoder_hidden_states"].astype(np.float32))).numpy()
    finally:
        unet_ref.conv = orig


def forward_twice(model, cfg):
    inp = cfg_inputs(cfg)
    return [model(**inp)["noise_pred"].copy() for _ in range(2)]


def conv_labels(labels):
    """{layer: (has the +w8a8 mark, the library's fp16 plan tile for the label's shape key, Cout, weights)} of the 3x3 conv labels"""
    r = {}
    for lab in labels:
        m = re.search(r"^conv3x3(\S*) (\d+)->(\d+) @(\d+)x(\d+) M=\d+ K=(\d+) (\S+) #0,3,(\d+),(\d+),(\d+),", lab)
        if m:
            mark, cin, cout, ho, wo, k, name, stride, up, ctot = m.groups()
            tile = _lib.conv_plan(3, int(stride), int(up), int(ctot), 0, int(cout), 2, int(ho), int(wo), flags=16)["tile"]
            r[name] = ("+w8a8" in mark, tile, int(cout), int(cout) * int(k))
    return r


@pytest.fixture(scope="module")
def calibrated():
    sd16 = weights.make_state_dict(unet_ref.unet_param_shapes(CFG), seed=35, dtype=np.float16)
    sd_t = weights.to_torch({k: v.astype(np.float32) for k, v in sd16.items()})
    r = {"sd16": sd16, "sd_t": sd_t, "outs": {}, "ranges": {}}
    for level in (True, "all"):
        m = HipModel(CFG, sd16, batch=2, observe_activations=level)
        r["outs"][level] = forward_twice(m, CFG)
        r["ranges"][level] = m.activation_ranges()
        m.close()
    plain = HipModel(CFG, sd16, batch=2)
    r["plain"] = forward_twice(plain, CFG)
    r["plain_used"] = plain.arena_used_bytes
    r["plain_labels"] = [lab for lab, _, _ in plain.profile(1)]
    plain.close()
    return r


def test_the_fp16_plan_has_every_kind_of_halo_conv(calibrated):
    convs = conv_labels(calibrated["plain_labels"])
    halo = {n for n, (_, tile, _, _) in convs.items() if tile == 7}
    labels = {n: lab for lab in calibrated["plain_labels"] for n in halo if f" {n} " in lab}
    assert any(re.search(r"#0,3,1,2,", lab) for lab in labels.values()), "no upsampling halo conv"
    assert any("up_blocks.1.resnets" in n and n.endswith("conv1") for n in halo), "no two-source halo conv"
    assert any(n.endswith("conv2") for n in halo) and any(tile == 9 for _, tile, _, _ in convs.values())


def test_observing_all_is_a_strict_superset_and_changes_nothing(calibrated):
    r = calibrated
    one, both = r["ranges"][True], r["ranges"]["all"]
    assert len(one) >= 1 and set(one) < set(both) and all(both[k] == one[k] for k in one)
    convs = conv_labels(r["plain_labels"])
    assert {k for k in both if k not in one} == {n for n, (_, tile, _, _) in convs.items() if tile == 7}
    assert set(one) == {n for n, (_, tile, _, _) in convs.items() if tile == 9}
    for a in r["outs"][True] + r["outs"]["all"] + r["plain"][1:]:
        assert np.array_equal(a, r["plain"][0])


# PSNR of the W8A8 handle (every eligible conv) against the fake-quantizing oracle, measured on the MI355X (LAB_NOTES.md round 25); the
# gate is the project's rule, measured - 6 dB, beside the parameter-free one.
W8A8_HALO_PSNR_MEASURED = 44.46      # 10 weight-stream + 7 halo layers (the fp16 handle against the same oracle: 43.69 dB; against the fp32 oracle: 68.77 dB)


def test_handle_runs_both_int8_kernels_and_follows_the_fake_quant_oracle(calibrated):
    r = calibrated
    sd16 = r["sd16"]
    recipe = aq.recipe_from_ranges(r["ranges"]["all"])
    stream_layers = set(r["ranges"][True])
    outs, info = {}, {}
    for use_graph in (False, True):
        m = HipModel(CFG, sd16, batch=2, use_graph=use_graph, activation_quantization=recipe)
        outs[use_graph] = forward_twice(m, CFG)
        info[use_graph] = (m.w8a8_info(), m.w8a8_layers(), m.arena_used_bytes, [lab for lab, _, _ in m.profile(1)])
        m.close()
    (n_marked, n_applied, nbytes), layers, used, labels = info[True]
    assert info[False][0] == info[True][0] and n_applied == n_marked == len(recipe) and sorted(layers) == sorted(recipe)
    for a in outs[False] + outs[True]:                                           # eager twice, graph capture + replay: bit for bit
        assert np.isfinite(a).all() and np.array_equal(a, outs[False][0])
    convs = conv_labels(labels)
    marked = {n for n, (mark, _, _, _) in convs.items() if mark}
    assert marked == set(recipe)
    t17 = {n for n in marked if convs[n][1] == 9}
    t18 = {n for n in marked if convs[n][1] == 7}
    assert t17 == stream_layers and t18 == marked - stream_layers and len(t17) >= 1 and len(t18) >= 3
    # an applied conv holds 1 B per weight + 4 B per output channel (two allocations: weights, scales).  The fp16 handle held the
    # [N][K] matrix (one allocation) and, for a weight-stream conv, its fragment-major copy (a second one).  Every allocation is rounded
    # up to the arena's 256 bytes: at most 255 B each way per allocation, so within 512 B per layer (tests/test_w8a8_gpu.py's bound).
    assert nbytes == sum(convs[n][3] + 4 * convs[n][2] for n in marked)
    saved = sum(4 * convs[n][3] - (convs[n][3] + 4 * convs[n][2]) for n in t17) + sum(2 * convs[n][3] - (convs[n][3] + 4 * convs[n][2]) for n in t18)
    assert abs((r["plain_used"] - used) - saved) <= 512 * n_applied, (r["plain_used"], used, saved)
    # parity, free of parameters: the handle is closer to the fake-quantizing oracle than the fp16 handle is
    w8a8, plain = outs[True][0], r["plain"][0]
    assert not np.array_equal(w8a8, plain)
    fq = oracle_forward(CFG, r["sd_t"], fake_quant_hook(recipe, sd16))
    p_w8a8, p_plain = psnr.compute_psnr(w8a8, fq), psnr.compute_psnr(plain, fq)
    print(f"W8A8 handle, {len(t17)} weight-stream + {len(t18)} halo layers: PSNR vs the fake-quant oracle {p_w8a8:.2f} dB "
          f"(the fp16 handle: {p_plain:.2f} dB); fp16 handle vs the fp32 oracle {psnr.compute_psnr(plain, oracle_forward(CFG, r['sd_t'])):.2f} dB")
    assert p_w8a8 > p_plain
    if W8A8_HALO_PSNR_MEASURED is not None:
        assert p_w8a8 >= W8A8_HALO_PSNR_MEASURED - 6.0


def test_stream_only_recipe_is_what_it_was(calibrated):
    """a recipe that names weight-stream layers alone: the halo convs stay fp16, their labels carry no mark"""
    r = calibrated
    recipe = aq.recipe_from_ranges(r["ranges"][True])
    m = HipModel(CFG, r["sd16"], batch=2, activation_quantization=recipe)
    out = forward_twice(m, CFG)[0]
    convs = conv_labels([lab for lab, _, _ in m.profile(1)])
    n_marked, n_applied, _ = m.w8a8_info()
    m.close()
    assert n_marked == n_applied == len(recipe) and {n for n, (mark, _, _, _) in convs.items() if mark} == set(recipe)
    assert all(convs[n][1] == 9 for n in recipe) and np.isfinite(out).all()


def test_recipe_naming_a_32_channel_conv_leaves_that_one_fp16():
    sd16 = weights.make_state_dict(unet_ref.unet_param_shapes(TINY), seed=33, dtype=np.float16)
    obs = HipModel(TINY, sd16, batch=2, observe_activations="all")
    forward_twice(obs, TINY)
    recipe = dict(aq.recipe_from_ranges(obs.activation_ranges()))
    obs.close()
    skipped = "down_blocks.0.resnets.0.conv1"                                    # 32 channels at 16x16: neither int8 kernel takes it
    assert skipped not in recipe and any("upsamplers" in k for k in recipe)      # (the 64-channel upsampler is a halo conv)
    recipe[skipped] = 5.0
    m = HipModel(TINY, sd16, batch=2, activation_quantization=recipe)
    out = forward_twice(m, TINY)[0]
    n_marked, n_applied, _ = m.w8a8_info()
    labels = [lab for lab, _, _ in m.profile(1)]
    m.close()
    assert np.isfinite(out).all() and n_marked == len(recipe) and n_applied == n_marked - 1
    lab = [x for x in labels if f" {skipped} " in x]
    assert len(lab) == 1 and "+w8a8" not in lab[0] and sum("+w8a8" in x for x in labels) == n_applied


# ---- pipeline ----
def test_cli_calibrates_every_eligible_conv_then_applies_the_recipe(tmp_path, monkeypatch):
    from PIL import Image
    from python_hip_stable_diffusion import pipeline as P
    from test_text_encoder_gpu import write_checkpoint_dir
    root = str(tmp_path / "mini-sd")
    os.makedirs(root)
    write_checkpoint_dir(root)
    paths = {scope: str(tmp_path / f"w8a8-{scope}.json") for scope in ("stream", "all")}
    pipes = []
    real = P.get_hip_pipe
    monkeypatch.setattr(P, "get_hip_pipe", lambda *a, **kw: pipes.append(real(*a, **kw)) or pipes[-1])

    def generate(tag, *flags):
        args = P.build_parser().parse_args(["--prompt", "a photo of an astronaut riding a horse", "-i", root, "-o", str(tmp_path / tag), "--seed", "93",
                                            "--model-version", "mini/stable-diffusion", "--scheduler", "DDIM", "--num-inference-steps", "2",
                                            "--attention-implementation", "ORIGINAL", *flags])
        return np.array(Image.open(P.main(args)))

    plain = generate("plain")
    recipes = {}
    for scope in ("stream", "all"):
        calibrated_image = generate("calib-" + scope, "--calibrate-activations", paths[scope], "--calibrate-scope", scope)
        assert np.array_equal(calibrated_image, plain)                           # observing changes no image
        recipes[scope] = json.load(open(paths[scope]))
        assert recipes[scope] == aq.recipe_from_ranges(pipes[-1].unet.activation_ranges())
    assert len(recipes["stream"]) >= 1 and set(recipes["stream"]) < set(recipes["all"])
    quant = generate("w8a8", "--activation-quantization-recipe", paths["all"])
    n_marked, n_applied, nbytes = pipes[-1].unet.w8a8_info()
    assert n_marked == len(recipes["all"]) and n_applied == n_marked and nbytes > 0 and sorted(pipes[-1].unet.w8a8_layers()) == sorted(recipes["all"])
    assert quant.shape == plain.shape and not np.array_equal(quant, plain)       # the recipe really is applied
    print(f"mini pipeline, {n_applied} W8A8 layers: image PSNR vs fp16 {psnr.compute_psnr(quant.astype(np.float64), plain.astype(np.float64)):.1f} dB")
