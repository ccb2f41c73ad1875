"""GPU suite of the W8A8 small-M 1x1 GEMM (plan tile 19, smgemm_i8.hip smgemm_i8_kernel): tile 12's tiles from int8 weights and int8
activations on v_mfma_i32_16x16x64_i8, with the semantics of the int8 weight stream (plan tile 17) - exact int32 sums over the whole K,
one scale per column, bias and residual added in fp32, ONE rounding to fp16.  With power-of-two scales the whole operator is exact and
compared bit for bit with the float64 integer product; with random scales it is gated against the float64 fake-quant reference of
tests/test_w8a8_gpu.py.  Then the third calibration scope, handles whose plain projections run from int8, and the CLI flag.

Shapes are those of tests/test_palettize_gemm_gpu.py - the smallest at which each mechanism of the shared geometry exists: 8 tiles in
all, 3 tiles per XCD, the n-fast order, M = 1280 over five samples, N = 1280, both tile heights - plus one H != W image.  The K walk
covers one stage, a K shorter than the prologue and every ring position twice around (a ring within 160 KB has at most 16 stages)."""
import functools
import json
import os
import re

import numpy as np
import pytest

from oracle import psnr, unet_ref, weights
from python_hip_stable_diffusion import HipModel, _lib, activation_quantization as aq
from test_palettize_gemm_gpu import BATCH, CFG, K_SHAPES, SHAPES as PAL_SHAPES, _child
from test_palettize_gpu import gate, h16
from test_w8a8_gpu import fake_quant_hook, reference

pytestmark = pytest.mark.gpu

# name -> (B, H, W, N, bm); M = B * H * W
SHAPES = dict(PAL_SHAPES)
SHAPES["bm32 M=128 N=160 (8x16 image)"] = (1, 8, 16, 160, 32)
K_WALK = tuple(64 * s for s in range(1, 35)) + (1280, 2560)


def run_op(c, what=""):
    """every operator call: NaN-prefilled output with a guard behind it, the plan, a second call with iters = 3"""
    n = int(np.prod(c["shape"]))
    guard = 4 * c["shape"][1] * c["shape"][3]
    buf = np.full(n + guard, np.nan, np.float16)
    args = (c["x"], c["wq"][:, :, 0, 0], c["w_scale"], c["act_absmax"])
    out, plan, _ = _lib.gemm_w8a8(*args, bias=c["bias"], res=c["res"], bm=c["bm"], out=buf)
    out = out.copy()
    assert np.isnan(buf[n:]).all(), f"{what}: the guard behind the output was written"
    assert not np.isnan(buf[:n]).any(), f"{what}: the NaN prefill was not fully overwritten"
    assert plan == [19, 1 if c["bm"] == 32 else 2, 1, 0], plan
    again, plan2, _ = _lib.gemm_w8a8(*args, bias=c["bias"], res=c["res"], bm=c["bm"], iters=3)
    assert plan2 == plan and np.array_equal(out.view(np.uint16), again.view(np.uint16)), f"{what}: two runs differ"
    return out


def want_of(c):
    """test_w8a8_gpu.reference (float64: exact integer product, cs[n] as the host computes it, bias, residual); an absent bias or
    residual adds nothing"""
    B, N, H, W = c["shape"]
    full = dict(c, x1=None, ups=False, bias=np.zeros(N, np.float32) if c["bias"] is None else c["bias"],
                res=np.zeros((B, N, H, W), np.float16) if c["res"] is None else c["res"])
    return reference(full)


# ---- exact family ----
def make_exact_case(shape, K, with_bias=True, with_res=True):
    """the recipe of test_w8a8_gpu.make_exact_case for a (N, K) weight: s_a = 2^-3 and s_w[n] in {2^-4, 2^-5, 2^-6}, every activation a
    multiple (or an exact .5 tie) of s_a, +-127, clamping values, +-inf and NaN among them, weights in [-3, 3] with a few +-127, bias and
    residual multiples of 2^-7: every fp32 value of the epilogue is exact, and the output is float16(exact value)."""
    B, H, W, N, bm = SHAPES[shape]
    rs = np.random.RandomState(19000 + 100 * list(SHAPES).index(shape) + K // 64)
    wq = rs.randint(-3, 4, size=(N, K, 1, 1)).astype(np.int8)                    # random: no symmetry under n <-> k
    wq.reshape(-1)[rs.choice(wq.size, 24, replace=False)] = np.array([-127, 127] * 12, np.int8)
    w_scale = (2.0 ** -rs.randint(4, 7, size=N)).astype(np.float32)
    ks = rs.randint(-8, 9, size=(B, K, H, W)).astype(np.float64)
    flat = ks.reshape(-1)
    pick = rs.choice(flat.size, 64, replace=False)
    flat[pick[:8]] = 127                                                         # the ends of the range
    flat[pick[8:16]] = -127
    flat[pick[16:24]] = [200, -200, 128, -128, 127.5, -127.5, 1000, -1000]       # values that clamp
    flat[pick[24:40]] = np.array([0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, -3.5, 126.5, -126.5, 125.5, -125.5, 6.5, 7.5, -6.5, -7.5])  # exact ties
    x = h16(ks * 0.125)
    assert np.array_equal(x.astype(np.float64), ks * 0.125)                      # all exactly representable in fp16
    flat16 = x.reshape(-1)
    flat16[pick[40:44]] = np.float16(np.inf)                                     # saturate to +127
    flat16[pick[44:48]] = -np.float16(np.inf)                                    # ... and -127
    flat16[pick[48:56]] = np.float16(np.nan)                                     # become 0
    bias = (rs.randint(-64, 65, size=N) * 2.0 ** -7).astype(np.float32) if with_bias else None
    res = h16(rs.randint(-256, 257, size=(B, N, H, W)) * 2.0 ** -7) if with_res else None
    return dict(x=x, wq=wq, w_scale=w_scale, act_absmax=np.float32(127 * 0.125), bias=bias, res=res, bm=bm, shape=(B, N, H, W))


def check_exact(c, what):
    assert np.float32(c["act_absmax"]) / np.float32(127) == np.float32(0.125)
    out = run_op(c, what)
    want = want_of(c)
    assert np.abs(want).max() < 2.0 ** 14 and np.array_equal(want * 512, np.rint(want * 512))   # what makes every fp32 value exact
    want16 = want.astype(np.float16)
    assert np.array_equal(out.view(np.uint16), want16.view(np.uint16)), f"{what}: {np.count_nonzero(out != want16)} of {out.size} elements differ"


@pytest.mark.parametrize("shape", list(SHAPES))
def test_operator_exact_family_is_bit_identical_to_the_integer_product(shape):
    check_exact(make_exact_case(shape, 192), f"{shape} K=192")


@pytest.mark.parametrize("K", K_WALK)
@pytest.mark.parametrize("shape", K_SHAPES)
def test_k_walk_covers_every_ring_position(shape, K):
    check_exact(make_exact_case(shape, K), f"{shape} K={K}")


@pytest.mark.parametrize("with_bias,with_res", [(False, True), (True, False), (False, False)])
@pytest.mark.parametrize("shape", K_SHAPES)
def test_bias_and_residual_absent(shape, with_bias, with_res):
    check_exact(make_exact_case(shape, 576, with_bias, with_res), f"{shape} K=576 bias={with_bias} res={with_res}")


def test_special_values_saturate_or_vanish():
    """+-inf -> +-127, NaN -> 0 (quantize8.h ws_quantize8): one channel of ones against each special input"""
    x = np.zeros((1, 64, 8, 8), np.float16)
    x[0, 0, 2, 3], x[0, 1, 4, 4], x[0, 2, 6, 1] = np.inf, -np.inf, np.nan
    wq = np.zeros((320, 64), np.int8)
    wq[:, :3] = 1
    out, plan, _ = _lib.gemm_w8a8(x, wq, np.ones(320, np.float32), 127.0)
    want = np.zeros((1, 320, 8, 8), np.float16)
    want[0, :, 2, 3], want[0, :, 4, 4] = 127, -127
    assert plan[0] == 19 and np.array_equal(out, want)


# ---- general family ----
def make_general_case(shape, K=192):
    B, H, W, N, bm = SHAPES[shape]
    rs = np.random.RandomState(29000 + list(SHAPES).index(shape))
    w = (rs.randn(N, K, 1, 1) / np.sqrt(K)).astype(np.float32)
    wq, w_scale, _ = _lib.quantize_weight(w)
    x = h16(rs.randn(B, K, H, W) * (1 + rs.rand(1, K, 1, 1)))
    return dict(x=x, wq=wq, w_scale=w_scale, act_absmax=np.float32(np.abs(x.astype(np.float32)).max()), bias=(0.1 * rs.randn(N)).astype(np.float32),
                res=h16(rs.randn(B, N, H, W)), bm=bm, shape=(B, N, H, W))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_operator_general_family_against_the_float64_fake_quant_reference(shape):
    c = make_general_case(shape)
    gate(run_op(c, shape), want_of(c), f"W8A8 gemm {shape}")


def test_tile_19_is_the_same_function_as_tile_17():
    """B = 2, 8x8, K = 192, N = 160 is a shape both int8 kernels take (tile 17 in one slab of eight waves): the same integers, the same
    scale, and the residual added to the fp32 value in front of the one rounding - in tile 17's slab combine and in tile 19's epilogue"""
    c = make_general_case("bm32 M=128 N=160")
    o19 = run_op(c)
    o17, plan, _ = _lib.conv2d_w8a8(c["x"], c["wq"], c["w_scale"], c["act_absmax"], bias=c["bias"], res=c["res"], nw=8)
    assert plan[0] == 17 and plan[2] == 1 and np.array_equal(o19.view(np.uint16), o17.view(np.uint16))


# ---- refusals, in the order of the header, each followed by a valid call ----
def test_operator_refusals_and_a_valid_call_right_after():
    c = make_exact_case("bm32 M=64 N=320 (8 tiles)", 128)
    x, wq, sc = c["x"], c["wq"][:, :, 0, 0], c["w_scale"]
    valid = lambda: check_exact(c, "a valid call right after a refused one")      # noqa: E731
    valid()
    lib = _lib.lib()
    out = np.empty(320 * 64, np.float16)
    plan = (_lib.C.c_int * 4)()
    args = lambda **kw: [kw.get("x", _lib.ptr(x)), kw.get("wq", _lib.ptr(wq)), kw.get("sc", _lib.fptr(sc)), 15.875, None, None,   # noqa: E731
                         kw.get("out", _lib.ptr(out)), kw.get("B", 1), 128, 8, 8, 320, kw.get("bm", 0), kw.get("plan", plan), 1, None]
    assert lib.sd_op_gemm_w8a8(*args()) == 0 and list(plan) == [19, 1, 1, 0]
    for kw in (dict(x=None), dict(wq=None), dict(sc=None), dict(out=None), dict(plan=None), dict(B=0)):
        assert lib.sd_op_gemm_w8a8(*args(**kw)) == -1, kw                        # SD_ERR_INVALID_ARGUMENT
        valid()
    assert lib.sd_op_gemm_w8a8(*args(bm=48, x=None)) == -1                       # (bm is looked at first; either way refused)
    with pytest.raises(ValueError, match="bm = 48"):
        _lib.gemm_w8a8(x, wq, sc, 15.875, bm=48)
    valid()
    with pytest.raises(ValueError, match="plan tile 19"):                        # N = 96
        _lib.gemm_w8a8(x, wq[:96], sc[:96], 15.875)
    valid()
    with pytest.raises(ValueError, match="plan tile 19"):                        # K = 96
        _lib.gemm_w8a8(x[:, :96], wq[:, :96], sc, 15.875)
    valid()
    # the int32 bound comes before the values: an absurd act_absmax does not get a word in
    with pytest.raises(ValueError, match="133120"):
        _lib.gemm_w8a8(np.zeros((1, 133184, 8, 8), np.float16), np.zeros((320, 133184), np.int8), np.ones(320, np.float32), float("nan"))
    valid()
    bad = wq.copy()
    bad[5, 7] = -128
    for absmax in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="act_absmax"):
            _lib.gemm_w8a8(x, bad, np.zeros(320, np.float32), absmax)              # ... and act_absmax before w_scale
        valid()
    with pytest.raises(ValueError, match="w_scale"):
        _lib.gemm_w8a8(x, bad, np.zeros(320, np.float32), 15.875)                  # ... and w_scale before the weight values
    valid()
    with pytest.raises(ValueError, match="-128"):
        _lib.gemm_w8a8(x, bad, sc, 15.875)
    valid()


def test_selftest_passes_with_the_16x16x64_int8_case():
    assert _lib.lib().sd_selftest_mfma() == 0


# ---- handles: block channels (64, 640) at 32x32, batch 4 - the twelve 640 -> 640 projections at M = 1024 ----
PROJECTIONS = ("proj_in", "attn1.to_out.0", "attn2.to_out.0")
SKIPPED = "up_blocks.1.resnets.0.conv_shortcut"           # a 64-channel 1x1 (it rides in norm1's launch): off the tiles


def cfg_inputs():
    hw = CFG["sample_size"]
    return dict(sample=weights.seeded_normal((BATCH, 4, hw, hw), 1).astype(np.float16), timestep=np.full(BATCH, 981, np.float16),
                encoder_hidden_states=weights.seeded_normal((BATCH, CFG["cross_attention_dim"], 1, 77), 2).astype(np.float16))


@functools.lru_cache(maxsize=None)
def state_dict():
    return weights.make_state_dict(unet_ref.unet_param_shapes(CFG), seed=44, dtype=np.float16)


def oracle_forward(sd_t, hook=None):
    import torch
    inp = cfg_inputs()
    orig = unet_ref.conv
    if hook is not None:
        unet_ref.conv = lambda sd, name, x, stride=1, padding=0: hook(sd, name, x, orig, stride=stride, padding=padding)
    try:
        return unet_ref.unet_forward(sd_t, CFG, torch.from_numpy(inp["sample"].astype(np.float32)), torch.from_numpy(inp["timestep"].astype(np.float32)),
                                     torch.from_numpy(inp["encoder_hidden_states"].astype(np.float32))).numpy()
    finally:
        unet_ref.conv = orig


def forward_twice(model):
    inp = cfg_inputs()
    return [model(**inp)["noise_pred"].copy() for _ in range(2)]


def gemm_labels(labels):
    """{layer: (has the +w8a8 mark, Cin, Cout, Ho, Wo, M)} of the plain 1x1 labels"""
    r = {}
    for lab in labels:
        m = re.search(r"^gemm1x1(\S*) (\d+)->(\d+) @(\d+)x(\d+) M=(\d+) K=(\d+) (\S+) #0,1,", lab)
        if m:
            mark, cin, cout, ho, wo, M, k, name = m.groups()
            r[name] = ("+w8a8" in mark, int(cin), int(cout), int(ho), int(wo), int(M))
    return r


def marked_labels(labels):
    return sorted(m.group(1) for m in (re.search(r"^\S+\+w8a8 .* K=\d+ (\S+) ", lab) for lab in labels) if m)


def run_recipe(recipe, graphs=(False, True)):
    """a handle per graph mode from the recipe: outputs of two forwards each, w8a8_info, applied layers, arena, labels"""
    outs, r = [], {}
    for use_graph in graphs:
        m = HipModel(CFG, state_dict(), batch=BATCH, use_graph=use_graph, activation_quantization=recipe)
        outs += forward_twice(m)
        r = dict(info=list(m.w8a8_info()), layers=sorted(m.w8a8_layers()), used=m.arena_used_bytes, labels=[lab for lab, _, _ in m.profile(1)])
        m.close()
    r["outs"] = outs
    return r


def plain_handle():
    m = HipModel(CFG, state_dict(), batch=BATCH)
    r = dict(outs=forward_twice(m), used=m.arena_used_bytes, labels=[lab for lab, _, _ in m.profile(1)])
    m.close()
    return r


def fixed_recipe(labels):
    """the twelve projections by name with a fixed range - for a process whose observers cannot see them (SD_SMGEMM=0)"""
    return {n: 6.0 for n in gemm_labels(labels) if n.endswith(PROJECTIONS)}


def switched_off():
    """what the child process of test_handle_with_the_small_m_gemm_switched_off reports"""
    plain = plain_handle()
    recipe = fixed_recipe(plain["labels"])
    r = run_recipe(recipe)
    return dict(n_recipe=len(recipe), info=r["info"], used=[r["used"], plain["used"]], marked=marked_labels(r["labels"]),
                finite=bool(all(np.isfinite(a).all() for a in r["outs"])), equal=bool(all(np.array_equal(a, plain["outs"][0]) for a in r["outs"])))


@pytest.fixture(scope="module")
def calibrated():
    r = {"outs": {}, "ranges": {}}
    for scope in ("all", "gemm"):
        m = HipModel(CFG, state_dict(), batch=BATCH, observe_activations=scope)
        r["outs"][scope] = forward_twice(m)
        r["ranges"][scope] = m.activation_ranges()
        m.close()
    r["plain"] = plain_handle()
    return r


def test_gemm_scope_adds_exactly_the_twelve_projections_and_changes_nothing(calibrated):
    r = calibrated
    both, three = r["ranges"]["all"], r["ranges"]["gemm"]
    assert len(both) >= 1 and set(both) < set(three) and all(three[k] == both[k] for k in both)
    extra = {k for k in three if k not in both}
    gemms = gemm_labels(r["plain"]["labels"])
    assert extra == {n for n in gemms if n.endswith(PROJECTIONS)} and len(extra) == 12
    for n in extra:                                                              # the 640-channel level: tile 12's by the library's own rule
        _, cin, cout, ho, wo, M = gemms[n]
        assert (cin, cout, ho, wo, M) == (640, 640, 16, 16, 1024)
        res = 0 if n.endswith("proj_in") else 4
        assert _lib.conv_plan(1, 1, 1, cin, 0, cout, BATCH, ho, wo, flags=16 | res)["tile"] == 12
    for a in r["outs"]["all"] + r["outs"]["gemm"] + r["plain"]["outs"][1:]:
        assert np.array_equal(a, r["plain"]["outs"][0])


# PSNR of the handle with the twelve int8 projections against the fake-quantizing oracle, measured on the MI355X (LAB_NOTES.md round
# 26); the gate is the project's rule, measured - 6 dB, beside the parameter-free one.
W8A8_GEMM_PSNR_MEASURED = 48.89      # 12 int8 projections (the fp16 handle against the same oracle: 47.48 dB; against the fp32 oracle: 70.10 dB)


def test_projections_run_from_int8_and_follow_the_fake_quant_oracle(calibrated):
    r = calibrated
    twelve = {k: v for k, v in r["ranges"]["gemm"].items() if k not in r["ranges"]["all"]}
    recipe = aq.recipe_from_ranges(twelve)
    assert len(recipe) == 12
    q = run_recipe(recipe)
    assert len(q["outs"]) == 4
    for a in q["outs"]:                                                          # eager twice, graph capture + replay: bit for bit
        assert np.isfinite(a).all() and np.array_equal(a, q["outs"][0])
    marked = [lab for lab in q["labels"] if "+w8a8" in lab]
    assert marked_labels(q["labels"]) == sorted(recipe) == q["layers"] and all(lab.startswith("gemm1x1+w8a8 640->640 @16x16 M=1024 K=640 ") for lab in marked)
    n_marked, n_applied, nbytes = q["info"]
    K = N = 640
    assert (n_marked, n_applied) == (12, 12) and nbytes == 12 * (K * N + 4 * N)
    # an applied projection holds 1 B per weight + 4 B per output channel (two allocations) instead of the fp16 [N][K] matrix (one):
    # every allocation is rounded up to the arena's 256 bytes, so within 512 B per layer (tests/test_w8a8_gpu.py's bound)
    saved = 12 * (2 * K * N - (K * N + 4 * N))
    assert abs((r["plain"]["used"] - q["used"]) - saved) <= 512 * 12, (r["plain"]["used"], q["used"], saved)
    # parity, free of parameters: the handle is closer to the fake-quantizing oracle than the fp16 handle is
    w8a8, plain = q["outs"][0], r["plain"]["outs"][0]
    assert not np.array_equal(w8a8, plain)
    sd16 = state_dict()
    sd_t = weights.to_torch({k: v.astype(np.float32) for k, v in sd16.items()})
    fq = oracle_forward(sd_t, fake_quant_hook(recipe, sd16))
    p_w8a8, p_plain = psnr.compute_psnr(w8a8, fq), psnr.compute_psnr(plain, fq)
    print(f"W8A8 handle, 12 int8 projections: PSNR vs the fake-quant oracle {p_w8a8:.2f} dB (the fp16 handle: {p_plain:.2f} dB); "
          f"fp16 handle vs the fp32 oracle {psnr.compute_psnr(plain, oracle_forward(sd_t)):.2f} dB")
    assert p_w8a8 > p_plain
    if W8A8_GEMM_PSNR_MEASURED is not None:
        assert p_w8a8 >= W8A8_GEMM_PSNR_MEASURED - 6.0


def test_both_families_in_one_handle(calibrated):
    """the whole gemm scope: halo convs, any weight-stream convs and the projections"""
    recipe = aq.recipe_from_ranges(calibrated["ranges"]["gemm"])
    q = run_recipe(recipe)
    n_marked, n_applied, _ = q["info"]
    assert n_marked == n_applied == len(recipe) and q["layers"] == sorted(recipe) == marked_labels(q["labels"])
    kinds = {lab.split("+w8a8")[0] for lab in q["labels"] if "+w8a8" in lab}
    assert kinds == {"conv3x3", "gemm1x1"}, kinds
    for a in q["outs"]:                                                          # graph replay == eager
        assert np.isfinite(a).all() and np.array_equal(a, q["outs"][0])
    assert not np.array_equal(q["outs"][0], calibrated["plain"]["outs"][0])


def test_handle_with_the_small_m_gemm_switched_off():
    """SD_SMGEMM=0 (an A/B switch, read once per process under SD_TUNE): the fp16 plan of the projections is no longer tile 12, so none
    runs from int8 - the reference's skipped layers: marked, not applied, fp16 arena, no mark in a label, the fp16 handle's output"""
    code = ("import test_w8a8_gemm_gpu as t\n"
            "print('RESULT ' + json.dumps(t.switched_off()))\n")
    r, _ = _child(code, dict(SD_TUNE="1", SD_SMGEMM="0"))
    assert r["n_recipe"] == 12 and r["info"] == [12, 0, 0]
    assert r["used"][0] == r["used"][1] and r["marked"] == [] and r["finite"] and r["equal"]


def test_recipe_naming_a_64_channel_projection_leaves_that_one_fp16(calibrated):
    labels = calibrated["plain"]["labels"]
    recipe = fixed_recipe(labels)
    assert len(recipe) == 12 and SKIPPED not in recipe and any(SKIPPED in lab for lab in labels)
    recipe[SKIPPED] = 5.0
    q = run_recipe(recipe, graphs=(False,))
    n_marked, n_applied, _ = q["info"]
    assert np.isfinite(q["outs"][0]).all() and n_marked == 13 and n_applied == n_marked - 1
    lab = [x for x in q["labels"] if SKIPPED in x]
    assert len(lab) == 1 and "+w8a8" not in lab[0] and sum("+w8a8" in x for x in q["labels"]) == n_applied


# ---- pipeline ----
def test_cli_calibrates_with_the_gemm_scope(tmp_path, monkeypatch):
    """the mini checkpoint has no projection tile 19 takes: the gemm scope observes what the all scope observes, and changes no image"""
    from PIL import Image
    from python_hip_stable_diffusion import pipeline as P
    from test_text_encoder_gpu import write_checkpoint_dir
    root = str(tmp_path / "mini-sd")
    os.makedirs(root)
    write_checkpoint_dir(root)
    paths = {scope: str(tmp_path / f"w8a8-{scope}.json") for scope in ("all", "gemm")}
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
    for scope in ("all", "gemm"):
        image = generate("calib-" + scope, "--calibrate-activations", paths[scope], "--calibrate-scope", scope)
        assert np.array_equal(image, plain)                                      # observing changes no image
        recipes[scope] = json.load(open(paths[scope]))
        assert recipes[scope] == aq.recipe_from_ranges(pipes[-1].unet.activation_ranges())
    assert len(recipes["gemm"]) >= 1 and recipes["gemm"] == recipes["all"]
