"""GPU suite of the W8A8 GEGLU projection (plan tile 20, smgeglu_i8.hip smgeglu_i8_kernel) and of the LayerNorm that writes its int8
activations (norm.hip layernorm_q8_kernel).  The LayerNorm is compared bit for bit with numpy's quantizer applied to the output of the
existing LayerNorm operator.  With power-of-two scales the GEGLU is compared bit for bit with plan tile 13 in plain form on fp16 operands
whose products and fp32 sums are exact; with random scales it is gated against a float64 fake-quant reference.  Then the fourth
calibration scope, handles whose GEGLU projections run from int8, and the CLI flag.

Shapes (M, N2) are those of tests/test_palettize_geglu_gpu.py on 128-row tiles - 2 x 4 = 8 tiles, 4 x 2, 3 x 8 = 24 (three per XCD) -
and two on 256-row tiles.  A ring stage is K64; the K walk covers every stage count from one up to twice around the deeper ring (8
stages at 128 rows, 6 at 256) plus two, then the 640-, 1280- and 2560-deep projections."""
import json
import os
import re

import numpy as np
import pytest

from oracle import psnr, weights
from python_hip_stable_diffusion import HipModel, _lib, activation_quantization as aq
from test_palettize_gemm_gpu import BATCH, CFG, _child
from test_palettize_geglu_gpu import SHAPES as SHAPES_128
from test_palettize_gpu import gate, h16
from test_w8a8_gemm_gpu import forward_twice, marked_labels, oracle_forward, plain_handle, run_recipe, state_dict
from test_w8a8_gpu import RANGE_DEV_GATE, fake_quant_hook, quantize_act

pytestmark = pytest.mark.gpu

SHAPES = [(m, n2, 128) for m, n2 in SHAPES_128] + [(512, 640, 256), (768, 1280, 256)]
assert [s[:2] for s in SHAPES[:3]] == [(256, 640), (512, 320), (384, 1280)]
ids3 = lambda s: "x".join(map(str, s))   # noqa: E731
K_WALK = tuple(64 * s for s in range(1, 2 * 8 + 3)) + (1280, 2560)
assert 640 in K_WALK
S_A = np.float32(0.125)


def run_op(c, what=""):
    """every GEGLU call: NaN-prefilled output with a guard behind it, the plan, a second call with iters = 3"""
    M, n = c["xq"].shape[0], c["xq"].shape[0] * c["wq"].shape[0] // 2
    buf = np.full(n + 4 * c["wq"].shape[0], np.nan, np.float16)
    args = (c["xq"], c["wq"], c["w_scale"], c["act_absmax"])
    out, plan, _ = _lib.geglu_w8a8(*args, bias=c["bias"], bm=c["bm"], out=buf)
    out = out.copy()
    assert out.shape == (M, c["wq"].shape[0] // 2)
    assert np.isnan(buf[n:]).all(), f"{what}: the guard behind the output was written"
    assert not np.isnan(buf[:n]).any(), f"{what}: the NaN prefill was not fully overwritten"
    assert plan == [20, 1 if c["bm"] == 128 else 2, 1, 0], plan
    again, plan2, _ = _lib.geglu_w8a8(*args, bias=c["bias"], bm=c["bm"], iters=3)
    assert plan2 == plan and np.array_equal(out.view(np.uint16), again.view(np.uint16)), f"{what}: two runs differ"
    return out


def run_ln(x, ln_w, ln_b, act_absmax):
    """every layernorm_q8 call: the output prefilled with -128 (a value the quantizer never writes), guard bytes behind it"""
    n = x.size
    buf = np.full(n + 4096, -128, np.int8)
    xq, _ = _lib.layernorm_q8(x, ln_w, ln_b, act_absmax, out=buf)
    xq = xq.copy()
    assert (buf[n:] == -128).all(), "the guard behind xq was written"
    assert (buf[:n] != -128).all(), "the prefill was not fully overwritten"
    again, _ = _lib.layernorm_q8(x, ln_w, ln_b, act_absmax, iters=3)
    assert np.array_equal(xq, again)
    return xq


def gelu64(g):
    import torch
    g = torch.from_numpy(np.asarray(g, np.float64))
    return (0.5 * g * (1.0 + torch.erf(g / np.sqrt(2.0)))).numpy()


def reference(xq, c):
    """float64: the exact integer product, cs[n] as the host computes it, the bias, v * gelu(g)"""
    half = c["wq"].shape[0] // 2
    s_a = np.float32(c["act_absmax"]) / np.float32(127.0)
    cs = (s_a * c["w_scale"].astype(np.float32)).astype(np.float32).astype(np.float64)
    y = (xq.astype(np.float64) @ c["wq"].astype(np.float64).T) * cs
    if c["bias"] is not None:
        y = y + c["bias"].astype(np.float64)
    return y[:, :half] * gelu64(y[:, half:])


# ---- layernorm_q8 ----
def ln_case(M, C, seed):
    rs = np.random.RandomState(seed)
    x = h16(rs.randn(M, C) * (1.0 + rs.rand(M, 1)) + 0.5 + 0.5 * rs.rand(M, 1))   # test_smgeglu_gpu.make_case's rows
    return x, (1.0 + 0.2 * rs.randn(C)).astype(np.float32), (0.1 * rs.randn(C)).astype(np.float32)


@pytest.mark.parametrize("M", [1, 5, 256])
@pytest.mark.parametrize("C", [64, 640, 1280, 2048])
def test_layernorm_q8_is_the_quantizer_over_the_layernorm_operator(C, M):
    x, ln_w, ln_b = ln_case(M, C, 100 * C + M)
    y, _ = _lib.layernorm(np.ascontiguousarray(x.T)[None, :, None, :], ln_w, ln_b)
    y = np.ascontiguousarray(y[0, :, 0, :].T)                                    # (M, C) fp16: the tensor an observer sees
    for absmax in (np.float32(np.abs(y.astype(np.float32)).max()), np.float32(1.5)):   # the calibrated range, and one that clamps
        want = quantize_act(y, absmax)[0].astype(np.int8)
        assert np.abs(want).max() == 127
        got = run_ln(x, ln_w, ln_b, absmax)
        assert np.array_equal(got, want), f"C={C} M={M} absmax={absmax}: {np.count_nonzero(got != want)} of {got.size} differ"


def test_layernorm_q8_plain_form_special_values_ties_and_clamps():
    """no affine: xq = quantize(x).  +-inf -> +-127, NaN -> 0, exact .5 ties to even, values past the range clamp"""
    rs = np.random.RandomState(5)
    ks = rs.randint(-8, 9, size=(5, 640)).astype(np.float64)
    flat = ks.reshape(-1)
    flat[:24] = [127, -127, 200, -200, 128, -128, 127.5, -127.5, 1000, -1000, 0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, -3.5, 126.5, -126.5, 125.5, -125.5, 6.5, -7.5]
    x = h16(ks * 0.125)
    assert np.array_equal(x.astype(np.float64), ks * 0.125)
    x.reshape(-1)[700:703] = [np.inf, -np.inf, np.nan]
    got = run_ln(x, None, None, np.float32(127 * 0.125))
    want = quantize_act(x, np.float32(127 * 0.125))[0].astype(np.int8)
    assert np.array_equal(got, want)
    assert list(got.reshape(-1)[:24]) == [127, -127, 127, -127, 127, -127, 127, -127, 127, -127, 0, 2, 2, 4, 0, -2, -2, -4, 126, -126, 126, -126, 6, -8]
    assert list(got.reshape(-1)[700:703]) == [127, -127, 0]


# ---- exact family ----
def make_exact_case(shape, K, with_bias=True):
    """s_a = 2^-3, s_w[n] in {2^-4, 2^-5, 2^-6}, xq mostly in [-8, 8] and wq mostly in [-3, 3] with a few +-127 each, bias multiples
    of 2^-7: xq * s_a and wq * s_w are exact fp16 values, their products and every partial sum exact fp32 values (asserted below), so
    tile 13 on them and tile 20 on the integers compute the same v and g in front of the same ending."""
    M, N2, bm = shape
    rs = np.random.RandomState(20000 + 100 * SHAPES.index(shape) + K // 64)
    wq = rs.randint(-3, 4, size=(N2, K)).astype(np.int8)                         # random: no symmetry under n <-> k
    wq.reshape(-1)[rs.choice(wq.size, 24, replace=False)] = np.array([-127, 127] * 12, np.int8)
    w_scale = (2.0 ** -rs.randint(4, 7, size=N2)).astype(np.float32)
    xq = rs.randint(-8, 9, size=(M, K)).astype(np.int8)
    xq.reshape(-1)[rs.choice(xq.size, 24, replace=False)] = np.array([-127, 127] * 12, np.int8)
    bias = (rs.randint(-64, 65, size=N2) * 2.0 ** -7).astype(np.float32) if with_bias else None
    return dict(xq=xq, wq=wq, w_scale=w_scale, act_absmax=np.float32(127) * S_A, bias=bias, bm=bm)


def check_exact(c, what):
    assert np.float32(c["act_absmax"]) / np.float32(127) == S_A
    # the condition of exactness, on the CPU before the launch: for every output the sum of |xq * wq| over K is below 2^24
    mag = np.abs(c["xq"].astype(np.int64)) @ np.abs(c["wq"].astype(np.int64)).T
    assert mag.max() < 2 ** 24, mag.max()
    x16, w16 = h16(c["xq"].astype(np.float32) * S_A), h16(c["wq"].astype(np.float32) * c["w_scale"][:, None])
    assert np.array_equal(x16.astype(np.float64), c["xq"] * 0.125) and np.array_equal(w16.astype(np.float64), c["wq"] * c["w_scale"][:, None].astype(np.float64))
    want, _ = _lib.geglu_ln(x16, w16, bias=c["bias"], kernel=101 if c["bm"] == 128 else 102)   # tile 13, plain form, the same tile height
    out = run_op(c, what)
    assert np.isfinite(want).all() and np.abs(want).max() > 1
    assert np.array_equal(out.view(np.uint16), want.view(np.uint16)), f"{what}: {np.count_nonzero(out != want)} of {out.size} elements differ"


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("shape", SHAPES, ids=ids3)
def test_exact_family_is_bit_identical_to_tile_13_in_plain_form(shape, with_bias):
    check_exact(make_exact_case(shape, 192, with_bias), f"{shape} K=192 bias={with_bias}")


@pytest.mark.parametrize("K", K_WALK)
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]], ids=ids3)
def test_k_walk_covers_every_ring_position(shape, K):
    check_exact(make_exact_case(shape, K), f"{shape} K={K}")


# ---- general family and composition ----
def make_general_case(shape, K=192):
    M, N2, bm = shape
    rs = np.random.RandomState(30000 + SHAPES.index(shape))
    w = (rs.randn(N2, K) / np.sqrt(K)).astype(np.float32)
    wq, w_scale, _ = _lib.quantize_weight(w)
    x, ln_w, ln_b = ln_case(M, K, 31000 + SHAPES.index(shape))
    return dict(x=x, ln_w=ln_w, ln_b=ln_b, wq=wq, w_scale=w_scale, bias=(0.1 * rs.randn(N2)).astype(np.float32), bm=bm)


def layernorm64(x, ln_w, ln_b, eps=1e-5):
    x = x.astype(np.float64)
    mu = x.mean(axis=1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * ln_w.astype(np.float64) + ln_b.astype(np.float64)


@pytest.mark.parametrize("shape", SHAPES, ids=ids3)
def test_general_family_and_composition_against_the_float64_fake_quant_reference(shape):
    c = make_general_case(shape)
    y16 = layernorm64(c["x"], c["ln_w"], c["ln_b"]).astype(np.float16)            # the reference quantizes float16(LayerNorm)
    c["act_absmax"] = np.float32(np.abs(y16.astype(np.float32)).max())
    c["xq"] = run_ln(c["x"], c["ln_w"], c["ln_b"], c["act_absmax"])              # activations through layernorm_q8 with an affine
    out = run_op(c, str(shape))
    gate(out, reference(c["xq"], c), f"W8A8 geglu {shape}: the operator on the device's int8 activations")
    xq64 = quantize_act(y16, c["act_absmax"])[0]
    print(f"{shape}: {np.count_nonzero(xq64 != c['xq'])} of {xq64.size} int8 activations differ from the float64 LayerNorm's")
    gate(out, reference(xq64, c), f"W8A8 geglu {shape}: layernorm_q8 + geglu_w8a8 against the float64 composition")


# ---- refusals that need the device for the valid call in between, in the header's order ----
def test_operator_refusals_and_a_valid_call_right_after():
    c = make_exact_case(SHAPES[0], 128)
    xq, wq, sc = c["xq"], c["wq"], c["w_scale"]
    valid = lambda: check_exact(c, "a valid call right after a refused one")      # noqa: E731
    valid()
    bad_w, bad_x = wq.copy(), xq.copy()
    bad_w[5, 7] = bad_x[3, 9] = -128
    refused = [
        dict(args=(xq, wq, sc, 15.875), bm=64, match="bm = 64"),
        dict(args=(xq[:0], wq, sc, 15.875), match="empty"),
        dict(args=(xq, wq[:320], sc[:320], 15.875), match="plan tile 20"),       # 2 x 2 tiles
        dict(args=(xq[:, :96], wq[:, :96], sc, 15.875), match="plan tile 20"),
        dict(args=(xq, wq, sc, 15.875), bm=256, match="plan tile 20"),           # one row of 256-row tiles
        dict(args=(bad_x, bad_w, np.zeros(640, np.float32), float("nan")), match="act_absmax"),
        dict(args=(bad_x, bad_w, np.zeros(640, np.float32), 15.875), match="w_scale"),
        dict(args=(bad_x, bad_w, sc, 15.875), match="weight value -128"),
        dict(args=(bad_x, wq, sc, 15.875), match="activation value -128"),
    ]
    for r in refused:
        with pytest.raises(ValueError, match=r["match"]):
            _lib.geglu_w8a8(*r["args"], bm=r.get("bm", 0))
        valid()


# ---- handles: block channels (64, 640) at 32x32, batch 4 - the GEGLU projections 640 -> 5120 at M = 1024 ----
def geglu_labels(labels):
    """{layer: (mark, Cin, Cout, Ho, Wo, M)} of the GEGLU labels"""
    r = {}
    for lab in labels:
        m = re.search(r"^geglu1x1(\S*) (\d+)->(\d+) @(\d+)x(\d+) M=(\d+) K=(\d+) (\S+) #2,1,", lab)
        if m:
            mark, cin, cout, ho, wo, M, k, name = m.groups()
            r[name] = (mark, int(cin), int(cout), int(ho), int(wo), int(M))
    return r


@pytest.fixture(scope="module")
def calibrated():
    r = {"outs": {}, "ranges": {}, "labels": {}}
    for scope in ("gemm", "geglu"):
        m = HipModel(CFG, state_dict(), batch=BATCH, observe_activations=scope)
        r["outs"][scope] = forward_twice(m)
        r["ranges"][scope] = m.activation_ranges()
        r["labels"][scope] = [lab for lab, _, _ in m.profile(1)]
        m.close()
    r["plain"] = plain_handle()
    return r


def test_geglu_scope_adds_exactly_the_geglu_projections_and_changes_nothing(calibrated):
    r = calibrated
    three, four = r["ranges"]["gemm"], r["ranges"]["geglu"]
    assert len(three) >= 1 and set(three) < set(four) and all(four[k] == three[k] for k in three)
    extra = {k for k in four if k not in three}
    geglus = geglu_labels(r["plain"]["labels"])
    at_1024 = {n for n, v in geglus.items() if v[5] == 1024}
    assert len(at_1024) >= 1 and all(n.endswith("ff.net.0.proj") for n in at_1024)
    assert extra == at_1024
    for n in extra:                                                              # tile 13 by the library's own rule, folded
        mark, cin, cout, ho, wo, M = geglus[n]
        assert (mark, cin, cout) == ("+ln", 640, 5120)
        p = _lib.conv_plan(1, 1, 1, cin, 0, cout, BATCH, ho, wo, out_mode=2, flags=1 | 16)
        assert p["tile"] == 13 and p["kernel"] == "smgeglu bm128"
    # two ordinary launches per observed GEGLU, in front of the GEGLU, which still runs folded
    labs = r["labels"]["geglu"]
    for n in extra:
        i = next(k for k, lab in enumerate(labs) if lab == "absmax " + n)
        assert labs[i - 1].startswith("layernorm ") and labs[i - 1].endswith(n.replace("ff.net.0.proj", "norm3"))
        assert labs[i + 1].startswith("geglu1x1+ln ") and f" {n} " in labs[i + 1]
    assert len(labs) == len(r["labels"]["gemm"]) + 2 * len(extra) and not any("layernorm_q8" in lab for lab in labs)
    for a in r["outs"]["gemm"] + r["outs"]["geglu"] + r["plain"]["outs"][1:]:
        assert np.array_equal(a, r["plain"]["outs"][0])
    # each new range against the oracle's max |layer_norm_ane(...)| at that layer
    seen = {}

    def spy(sd, name, x, orig, **kw):
        seen[name] = max(seen.get(name, 0.0), float(x.abs().max()))
        return orig(sd, name, x, **kw)

    sd_t = weights.to_torch({k: v.astype(np.float32) for k, v in state_dict().items()})
    oracle_forward(sd_t, spy)
    devs = {n: abs(four[n] - seen[n]) / seen[n] for n in extra}
    print("observed norm3 ranges vs oracle:", {n: (round(four[n], 4), round(seen[n], 4), f"{devs[n]:.2e}") for n in extra})
    assert max(devs.values()) <= RANGE_DEV_GATE, devs


# PSNR of the handle with the int8 GEGLU projections against the fake-quantizing oracle, measured on the MI355X (LAB_NOTES.md round
# 27); the gate is the project's rule, measured - 6 dB, beside the parameter-free one.
W8A8_GEGLU_PSNR_MEASURED = 55.63     # 4 int8 GEGLU projections (the fp16 handle against the same oracle: 52.23 dB; against the fp32 oracle: 70.10 dB)


def test_geglus_run_from_int8_and_follow_the_fake_quant_oracle(calibrated):
    r = calibrated
    new = {k: v for k, v in r["ranges"]["geglu"].items() if k not in r["ranges"]["gemm"]}
    recipe = aq.recipe_from_ranges(new)
    n = len(recipe)
    assert n >= 1 and all(k.endswith("ff.net.0.proj") for k in recipe)
    q = run_recipe(recipe)
    assert len(q["outs"]) == 4
    for a in q["outs"]:                                                          # eager twice, graph capture + replay: bit for bit
        assert np.isfinite(a).all() and np.array_equal(a, q["outs"][0])
    labs = q["labels"]
    marked = [k for k, lab in enumerate(labs) if "+w8a8" in lab]
    assert marked_labels(labs) == sorted(recipe) == q["layers"]
    for k in marked:                                                             # a layernorm_q8 launch sits in front of each marked launch
        assert labs[k].startswith("geglu1x1+w8a8 640->5120 @16x16 M=1024 K=640 ")
        name = re.search(r"K=640 (\S+) ", labs[k]).group(1)
        assert labs[k - 1] == "layernorm_q8 " + name.replace("ff.net.0.proj", "norm3")
    assert sum("layernorm_q8" in lab for lab in labs) == n and len(labs) == len(r["plain"]["labels"]) + n
    n_marked, n_applied, nbytes = q["info"]
    K, N2, M = 640, 5120, 1024
    assert (n_marked, n_applied) == (n, n) and nbytes == n * (K * N2 + 4 * N2)
    # fp16: the folded matrix, colsum, bias.  int8: the stream, cs, bias, norm3's weight and bias, the int8 activations.  Nine
    # allocations, each rounded up to the arena's 256 bytes
    saved = n * ((2 * K * N2 + 8 * N2) - (K * N2 + 8 * N2 + 8 * K + M * K))
    assert abs((r["plain"]["used"] - q["used"]) - saved) <= 256 * 9 * n, (r["plain"]["used"], q["used"], saved)
    # parity, free of parameters: the handle is closer to the fake-quantizing oracle than the fp16 handle is
    w8a8, plain = q["outs"][0], r["plain"]["outs"][0]
    assert not np.array_equal(w8a8, plain)
    sd16 = state_dict()
    sd_t = weights.to_torch({k: v.astype(np.float32) for k, v in sd16.items()})
    fq = oracle_forward(sd_t, fake_quant_hook(recipe, sd16))
    p_w8a8, p_plain = psnr.compute_psnr(w8a8, fq), psnr.compute_psnr(plain, fq)
    print(f"W8A8 handle, {n} int8 GEGLU projections: PSNR vs the fake-quant oracle {p_w8a8:.2f} dB (the fp16 handle: {p_plain:.2f} dB); "
          f"fp16 handle vs the fp32 oracle {psnr.compute_psnr(plain, oracle_forward(sd_t)):.2f} dB")
    assert p_w8a8 > p_plain
    if W8A8_GEGLU_PSNR_MEASURED is not None:
        assert p_w8a8 >= W8A8_GEGLU_PSNR_MEASURED - 6.0


def switched_off():
    """what the child process of test_handle_with_the_geglu_kernel_switched_off reports"""
    plain = plain_handle()
    recipe = {n: 6.0 for n, v in geglu_labels(plain["labels"]).items() if v[5] == 1024}
    r = run_recipe(recipe)
    return dict(n_recipe=len(recipe), info=r["info"], used=[r["used"], plain["used"]], marked=marked_labels(r["labels"]),
                q8=sum("layernorm_q8" in lab for lab in r["labels"]), finite=bool(all(np.isfinite(a).all() for a in r["outs"])),
                equal=bool(all(np.array_equal(a, plain["outs"][0]) for a in r["outs"])))


def test_handle_with_the_geglu_kernel_switched_off():
    """SD_SMGEGLU=0 (an A/B switch, read once per process under SD_TUNE): the fp16 plan of the GEGLUs is no longer tile 13, so none runs
    from int8 - the reference's skipped layers: marked, not applied, fp16 arena, no mark in a label, the fp16 handle's output"""
    code = ("import test_w8a8_geglu_gpu as t\n"
            "print('RESULT ' + json.dumps(t.switched_off()))\n")
    r, _ = _child(code, dict(SD_TUNE="1", SD_SMGEGLU="0"))
    assert r["n_recipe"] >= 1 and r["info"] == [r["n_recipe"], 0, 0]
    assert r["used"][0] == r["used"][1] and r["marked"] == [] and r["q8"] == 0 and r["finite"] and r["equal"]


# ---- pipeline ----
def test_cli_calibrates_with_the_geglu_scope_then_applies_the_recipe(tmp_path, monkeypatch):
    """the mini checkpoint has no GEGLU tile 20 takes: the geglu scope observes what the gemm scope observes and changes no image, and
    its recipe is applied"""
    from PIL import Image
    from python_hip_stable_diffusion import pipeline as P
    from test_text_encoder_gpu import write_checkpoint_dir
    root = str(tmp_path / "mini-sd")
    os.makedirs(root)
    write_checkpoint_dir(root)
    paths = {scope: str(tmp_path / f"w8a8-{scope}.json") for scope in ("gemm", "geglu")}
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
    for scope in ("gemm", "geglu"):
        image = generate("calib-" + scope, "--calibrate-activations", paths[scope], "--calibrate-scope", scope)
        assert np.array_equal(image, plain)                                      # observing changes no image
        recipes[scope] = json.load(open(paths[scope]))
        assert recipes[scope] == aq.recipe_from_ranges(pipes[-1].unet.activation_ranges())
    assert len(recipes["geglu"]) >= 1 and recipes["geglu"] == recipes["gemm"]
    quant = generate("w8a8", "--activation-quantization-recipe", paths["geglu"])
    n_marked, n_applied, nbytes = pipes[-1].unet.w8a8_info()
    assert n_marked == len(recipes["geglu"]) and n_applied == n_marked and nbytes > 0
    assert quant.shape == plain.shape and not np.array_equal(quant, plain)       # the recipe really is applied
