"""GPU suite of the W8A8 transformer tail's two kernels: the small-M 1x1 GEMM from int8 weights and int8 activations (plan tile 24,
smgemm_q8.hip smgemm_q8_kernel) and the GEGLU projection that writes those activations itself (plan tile 20 with an int8 output,
smgeglu_i8.hip smgeglu_i8_kernel<BM, true>).

Tile 24 is tile 19 (smgemm_i8.hip) behind its quantizer - the same tiles, the same integers, the same epilogue - so with activations
that are exact multiples of s_a = 2^-3 the two operators must agree bit for bit, with no tolerance and with random scales, bias and
residual; the same output is restated in numpy: the int64 product, then the epilogue's fp32 operations one by one.  With random
weights the operator is gated against the float64 reference on the int8 activations the device wrote.  The GEGLU's int8 output is
compared bit for bit with numpy's quantizer over the fp16 output of the plain call.

Shapes (M, N, bm) are the smallest the tiles admit: 8 / 8 / 24 tiles at 32 rows, 8 / 8 at 64.  A ring stage is K64; the K walk covers
every stage count from one up to twice around the deeper ring (22 stages at 32 rows, 17 at 64) plus two, then K = 2560 and 5120.

Then the calibration scope ``tail``, handles whose transformer tails run un-merged from int8 - block channels (64, 640) at 32x32, batch
4: four blocks of 2560 -> 640 at M = 1024 - and the CLI flag."""
import json
import os
import re

import numpy as np
import pytest

from oracle import psnr, weights
from python_hip_stable_diffusion import HipModel, _lib, activation_quantization as aq
from test_palettize_gemm_gpu import BATCH, CFG, _child
from test_palettize_gpu import gate, h16
from test_w8a8_geglu_gpu import make_exact_case as geglu_exact_case, make_general_case as geglu_general_case, layernorm64, reference as geglu_reference
from test_w8a8_geglu_gpu import run_ln, run_op as run_geglu
from test_w8a8_gemm_gpu import forward_twice, marked_labels, oracle_forward, plain_handle, state_dict
from test_w8a8_gpu import RANGE_DEV_GATE, quantize_act
from test_w8a8_qkv_gpu import fake_quant_hook, run_recipe

pytestmark = pytest.mark.gpu

SHAPES = [(128, 160, 32), (64, 320, 32), (96, 640, 32), (256, 160, 64), (128, 320, 64)]
ids3 = lambda s: "x".join(map(str, s))   # noqa: E731
NST_DEEPER = 22                                           # SmQ8Cfg<32>::NST: 160 KB / 7 KB
K_WALK = tuple(64 * s for s in range(1, 2 * NST_DEEPER + 3)) + (2560, 5120)
S_A = np.float32(0.125)
ABSMAX_EXACT = np.float32(127) * S_A


def run_q8(c, what=""):
    """every gemm_q8 call: NaN-prefilled output with a guard behind it, the plan, a second call with iters = 3"""
    M, N = c["xq"].shape[0], c["wq"].shape[0]
    n = M * N
    buf = np.full(n + 4 * N, np.nan, np.float16)
    args = (c["xq"], c["wq"], c["w_scale"], c["act_absmax"])
    out, plan, _ = _lib.gemm_q8(*args, bias=c["bias"], res=c["res"], bm=c["bm"], out=buf)
    out = out.copy()
    assert out.shape == (M, N)
    assert np.isnan(buf[n:]).all(), f"{what}: the guard behind the output was written"
    assert not np.isnan(buf[:n]).any(), f"{what}: the NaN prefill was not fully overwritten"
    assert plan == [24, 1 if c["bm"] == 32 else 2, 1, 0], plan
    again, plan2, _ = _lib.gemm_q8(*args, bias=c["bias"], res=c["res"], bm=c["bm"], iters=3)
    assert plan2 == plan and np.array_equal(out.view(np.uint16), again.view(np.uint16)), f"{what}: two runs differ"
    return out


def run_geglu_q8(c, out_absmax, what=""):
    """every geglu_w8a8(out_absmax) call: the output prefilled with -128 (a value the quantizer never writes), guard bytes behind it"""
    M, half = c["xq"].shape[0], c["wq"].shape[0] // 2
    n = M * half
    buf = np.full(n + 4096, -128, np.int8)
    args = (c["xq"], c["wq"], c["w_scale"], c["act_absmax"])
    gq, plan, _ = _lib.geglu_w8a8(*args, bias=c["bias"], bm=c["bm"], out=buf, out_absmax=out_absmax)
    gq = gq.copy()
    assert gq.shape == (M, half) and gq.dtype == np.int8
    assert (buf[n:] == -128).all(), f"{what}: the guard behind out_q was written"
    assert (buf[:n] != -128).all(), f"{what}: the prefill was not fully overwritten"
    assert plan == [20, 1 if c["bm"] == 128 else 2, 1, 0], plan
    again, plan2, _ = _lib.geglu_w8a8(*args, bias=c["bias"], bm=c["bm"], iters=3, out_absmax=out_absmax)
    assert plan2 == plan and np.array_equal(gq, again), f"{what}: two runs differ"
    return gq


def cs_of(c):
    """cs[n] = fp32(s_a * s_w[n]) with s_a = fp32(act_absmax / 127), as the host computes it"""
    s_a = np.float32(c["act_absmax"]) / np.float32(127.0)
    return (s_a * c["w_scale"].astype(np.float32)).astype(np.float32)


def reference64(xq, c):
    """float64: the exact integer product, cs[n], the bias, the residual; an absent one adds nothing"""
    y = (xq.astype(np.float64) @ c["wq"].astype(np.float64).T) * cs_of(c).astype(np.float64)
    if c["bias"] is not None:
        y = y + c["bias"].astype(np.float64)
    if c["res"] is not None:
        y = y + c["res"].astype(np.float64)
    return y


def epilogue32(c):
    """the operator restated: the int64 product, one conversion, one product, bias and residual added in fp32 - every operation rounded
    on its own - and ONE rounding to fp16"""
    acc = c["xq"].astype(np.int64) @ c["wq"].astype(np.int64).T
    assert np.abs(acc).max() < 2 ** 24                                           # the conversion to fp32 is exact
    v = acc.astype(np.float32) * cs_of(c)[None, :]
    if c["bias"] is not None:
        v = v + c["bias"][None, :]
    if c["res"] is not None:
        v = v + c["res"].astype(np.float32)
    assert v.dtype == np.float32
    return v.astype(np.float16)


def tile_19(c):
    """sd_op_gemm_w8a8 on x16 = xq * s_a (exact in fp16) at the same tile height; its layout is (B, C, H, W): one sample, one row of M pixels"""
    x16 = h16(c["xq"].astype(np.float32) * S_A)
    assert np.array_equal(x16.astype(np.float64), c["xq"] * 0.125)
    assert np.array_equal(quantize_act(x16, c["act_absmax"])[0], c["xq"])        # ws_quantize8(x16) == xq: the issue's condition
    nchw = lambda a: None if a is None else np.ascontiguousarray(a.T)[None, :, None, :]   # noqa: E731
    out, plan, _ = _lib.gemm_w8a8(nchw(x16), c["wq"], c["w_scale"], c["act_absmax"], bias=c["bias"], res=nchw(c["res"]), bm=c["bm"])
    assert plan == [19, 1 if c["bm"] == 32 else 2, 1, 0], plan
    return np.ascontiguousarray(out[0, :, 0, :].T)


# ---- exact family ----
def make_exact_case(shape, K, with_bias=True, with_res=True):
    """xq mostly in [-8, 8] and wq mostly in [-3, 3] with a few +-127 each, s_a = 2^-3, RANDOM w_scale, bias and residual: nothing about
    the epilogue is exact - tiles 19 and 24 must run the same fp32 operations in the same order to agree"""
    M, N, bm = shape
    rs = np.random.RandomState(24000 + 100 * SHAPES.index(shape) + K // 64)
    wq = rs.randint(-3, 4, size=(N, K)).astype(np.int8)                          # random: no symmetry under n <-> k
    wq.reshape(-1)[rs.choice(wq.size, 24, replace=False)] = np.array([-127, 127] * 12, np.int8)
    xq = rs.randint(-8, 9, size=(M, K)).astype(np.int8)
    xq.reshape(-1)[rs.choice(xq.size, 24, replace=False)] = np.array([-127, 127] * 12, np.int8)
    w_scale = (2.0 ** -5 * (0.5 + 1.5 * rs.rand(N))).astype(np.float32)
    bias = (0.1 * rs.randn(N)).astype(np.float32) if with_bias else None
    res = h16(rs.randn(M, N)) if with_res else None
    return dict(xq=xq, wq=wq, w_scale=w_scale, act_absmax=ABSMAX_EXACT, bias=bias, res=res, bm=bm)


def check_exact(c, what):
    assert np.float32(c["act_absmax"]) / np.float32(127) == S_A
    out = run_q8(c, what)
    want19 = tile_19(c)
    assert np.isfinite(want19).all() and np.abs(want19).max() > 1
    assert np.array_equal(out.view(np.uint16), want19.view(np.uint16)), f"{what}: {np.count_nonzero(out != want19)} of {out.size} elements differ from tile 19"
    want = epilogue32(c)
    assert np.array_equal(out.view(np.uint16), want.view(np.uint16)), f"{what}: {np.count_nonzero(out != want)} of {out.size} elements differ from numpy"


@pytest.mark.parametrize("shape", SHAPES, ids=ids3)
def test_exact_family_is_bit_identical_to_tile_19_and_to_the_integer_product(shape):
    check_exact(make_exact_case(shape, 192), f"{shape} K=192")


@pytest.mark.parametrize("K", K_WALK)
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]], ids=ids3)
def test_k_walk_covers_every_ring_position(shape, K):
    check_exact(make_exact_case(shape, K), f"{shape} K={K}")


@pytest.mark.parametrize("with_bias,with_res", [(False, True), (True, False), (False, False)])
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]], ids=ids3)
def test_bias_and_residual_absent(shape, with_bias, with_res):
    check_exact(make_exact_case(shape, 576, with_bias, with_res), f"{shape} K=576 bias={with_bias} res={with_res}")


# ---- general family ----
def make_general_case(shape, K=192):
    M, N, bm = shape
    rs = np.random.RandomState(34000 + SHAPES.index(shape))
    w = (rs.randn(N, K) / np.sqrt(K)).astype(np.float32)
    wq, w_scale, _ = _lib.quantize_weight(w)
    x = h16(rs.randn(M, K) * (1 + rs.rand(1, K)))
    return dict(x=x, wq=wq, w_scale=w_scale, act_absmax=np.float32(np.abs(x.astype(np.float32)).max()), bias=(0.1 * rs.randn(N)).astype(np.float32),
                res=h16(rs.randn(M, N)), bm=bm)


@pytest.mark.parametrize("shape", SHAPES, ids=ids3)
def test_general_family_against_the_float64_reference_on_the_devices_activations(shape):
    c = make_general_case(shape)
    c["xq"] = run_ln(c["x"], None, None, c["act_absmax"])                        # the plain-form quantizer launch: the fallback producer
    assert np.array_equal(c["xq"], quantize_act(c["x"], c["act_absmax"])[0])
    gate(run_q8(c, str(shape)), reference64(c["xq"], c), f"W8A8 gemm_q8 {shape}")


# ---- the producer: tile 20 with an int8 output ----
GEGLU_SHAPES = [(256, 640, 128), (512, 640, 256)]                      # one per tile height, both in test_w8a8_geglu_gpu.SHAPES


def make_geglu_general_case(shape):
    """test_w8a8_geglu_gpu.make_general_case with its activations: the range of float16(LayerNorm), int8 through layernorm_q8"""
    c = geglu_general_case(shape)
    y16 = layernorm64(c["x"], c["ln_w"], c["ln_b"]).astype(np.float16)
    c["act_absmax"] = np.float32(np.abs(y16.astype(np.float32)).max())
    c["xq"] = run_ln(c["x"], c["ln_w"], c["ln_b"], c["act_absmax"])
    return c


@pytest.mark.parametrize("shape", GEGLU_SHAPES, ids=ids3)
def test_geglu_int8_output_is_the_quantizer_over_the_fp16_output(shape):
    c = make_geglu_general_case(shape)
    g16 = run_geglu(c, str(shape))                                               # the fp16 instantiation, with its own guard and repeat
    gate(g16, geglu_reference(c["xq"], c), f"W8A8 geglu {shape}: the fp16 output beside the int8 one")
    observed = np.float32(np.abs(g16.astype(np.float32)).max())
    for absmax in (observed, np.float32(0.25) * observed):                       # the calibrated range, and one that clamps
        want = quantize_act(g16, absmax)[0].astype(np.int8)
        assert np.abs(want).max() == 127 and (absmax == observed or np.count_nonzero(np.abs(want) == 127) > 8)
        got = run_geglu_q8(c, absmax, f"{shape} out_absmax={absmax}")
        assert np.array_equal(got, want), f"{shape} out_absmax={absmax}: {np.count_nonzero(got != want)} of {got.size} differ"
    again = run_geglu(c, str(shape))                                             # ... and the fp16 launch behind the int8 ones: the same bits
    assert np.array_equal(again.view(np.uint16), g16.view(np.uint16))


@pytest.mark.parametrize("shape", GEGLU_SHAPES, ids=ids3)
def test_geglu_exact_family_int8_output(shape):
    """the exact family of tile 20's own suite (power-of-two scales: its fp16 output is tile 13's bit for bit, asserted there)"""
    c = geglu_exact_case(shape, 192)
    g16 = run_geglu(c, str(shape))
    absmax = np.float32(np.abs(g16.astype(np.float32)).max())
    assert np.array_equal(run_geglu_q8(c, absmax, str(shape)), quantize_act(g16, absmax)[0].astype(np.int8))


# ---- composition: ff.net.0.proj -> ff.net.2 with no fp16 tensor in between ----
@pytest.mark.parametrize("shape,n_out,bm2", [((256, 640, 128), 320, 32), ((256, 640, 128), 160, 64), ((512, 640, 256), 160, 64)], ids=str)
def test_composition_against_the_float64_fake_quant_composition(shape, n_out, bm2):
    c = make_geglu_general_case(shape)
    M, K2 = shape[0], shape[1] // 2
    g64 = geglu_reference(c["xq"], c)                                            # float64 on the device's int8 LayerNorm output
    g16 = g64.astype(np.float16)
    a2 = np.float32(np.abs(g16.astype(np.float32)).max())                        # the range a calibration pass would observe
    rs = np.random.RandomState(38000 + n_out + bm2)
    wq2, w_scale2, _ = _lib.quantize_weight((rs.randn(n_out, K2) / np.sqrt(K2)).astype(np.float32))
    tail = dict(wq=wq2, w_scale=w_scale2, act_absmax=a2, bias=(0.1 * rs.randn(n_out)).astype(np.float32), res=h16(rs.randn(M, n_out)), bm=bm2)
    tail["xq"] = run_geglu_q8(c, a2, f"{shape} -> {n_out}")
    out = run_q8(tail, f"{shape} -> {n_out}")
    gate(out, reference64(tail["xq"], tail), f"gemm_q8 on the GEGLU's int8 output {shape} -> {n_out}")
    gq64 = quantize_act(g16, a2)[0]
    print(f"{shape} -> {n_out}: {np.count_nonzero(gq64 != tail['xq'])} of {gq64.size} int8 activations differ from the float64 GEGLU's")
    gate(out, reference64(gq64, tail), f"geglu_w8a8(out_absmax) + gemm_q8 against the float64 composition {shape} -> {n_out}")


# ---- refusals that need the device for the valid call in between, in the header's order ----
def test_gemm_q8_refusals_and_a_valid_call_right_after():
    c = make_exact_case(SHAPES[1], 128)
    xq, wq, sc = c["xq"], c["wq"], c["w_scale"]
    valid = lambda: check_exact(c, "a valid call right after a refused one")      # noqa: E731
    valid()
    bad_w, bad_x = wq.copy(), xq.copy()
    bad_w[5, 7] = bad_x[3, 9] = -128
    zeros = np.zeros(320, np.float32)
    refused = [
        dict(args=(xq, wq, sc, 15.875), bm=48, match="bm = 48"),
        dict(args=(xq[:0], wq, sc, 15.875), match="empty"),
        dict(args=(xq, wq[:96], sc[:96], 15.875), match="plan tile 24"),         # N = 96
        dict(args=(xq[:, :96], wq[:, :96], sc, 15.875), match="plan tile 24"),   # K = 96
        dict(args=(xq, wq, sc, 15.875), bm=64, match="plan tile 24"),            # one row of 64-row tiles
        dict(args=(bad_x, bad_w, zeros, float("nan")), match="act_absmax"),
        dict(args=(bad_x, bad_w, zeros, 0.0), match="act_absmax"),
        dict(args=(bad_x, bad_w, zeros, 15.875), match="w_scale"),
        dict(args=(bad_x, bad_w, sc, 15.875), match="weight value -128"),
        dict(args=(bad_x, wq, sc, 15.875), match="activation value -128"),
    ]
    for r in refused:
        with pytest.raises(ValueError, match=r["match"]):
            _lib.gemm_q8(*r["args"], bm=r.get("bm", 0))
        valid()


def test_geglu_q8_refusals_and_a_valid_call_right_after():
    c = geglu_exact_case((256, 640, 128), 128)
    xq, wq, sc = c["xq"], c["wq"], c["w_scale"]
    g16 = run_geglu(c)
    absmax = np.float32(np.abs(g16.astype(np.float32)).max())
    want = quantize_act(g16, absmax)[0].astype(np.int8)
    valid = lambda: np.testing.assert_array_equal(run_geglu_q8(c, absmax), want)  # noqa: E731
    valid()
    bad_w = wq.copy()
    bad_w[5, 7] = -128
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="out_absmax"):                      # beside act_absmax: before w_scale and the values
            _lib.geglu_w8a8(xq, bad_w, np.zeros(640, np.float32), 15.875, out_absmax=bad)
        valid()
    with pytest.raises(ValueError, match="act_absmax"):                          # ... and act_absmax in front of it
        _lib.geglu_w8a8(xq, wq, sc, float("nan"), out_absmax=float("nan"))
    valid()
    with pytest.raises(ValueError, match="bm = 64"):
        _lib.geglu_w8a8(xq, wq, sc, 15.875, bm=64, out_absmax=1.0)
    valid()
    with pytest.raises(ValueError, match="int8"):                                # a float16 buffer for the int8 output
        _lib.geglu_w8a8(xq, wq, sc, 15.875, out=np.empty(256 * 320, np.float16), out_absmax=1.0)
    valid()


# ---- handles: block channels (64, 640) at 32x32, batch 4 - four tails ff.net.2 2560 -> 640 + proj_out 640 -> 640 at M = 1024 ----
C_, K1_, M_ = 640, 2560, 1024


def tail_blocks(labels):
    """the transformer blocks whose tail the plain handle runs as the merged launch, in launch order"""
    return [m.group(1) for m in (re.search(r"^gemm1x1 3200->640 @16x16 M=1024 K=3200 (\S+)\.ff\.net\.2 \+ residual \+ proj_out \+ residual ", lab)
                                 for lab in labels) if m]


def names_of(block):
    """ff.net.2 of the block and proj_out of its SpatialTransformer"""
    return [block + ".ff.net.2", block.rsplit(".transformer_blocks.", 1)[0] + ".proj_out"]


@pytest.fixture(scope="module")
def calibrated():
    r = {"outs": {}, "ranges": {}, "labels": {}}
    for scope in ("attn", "tail"):
        for use_graph in (False, True):
            m = HipModel(CFG, state_dict(), batch=BATCH, use_graph=use_graph, observe_activations=scope)
            r["outs"].setdefault(scope, []).extend(forward_twice(m))
            if not use_graph:
                r["ranges"][scope] = m.activation_ranges()
                r["labels"][scope] = [lab for lab, _, _ in m.profile(1)]
            m.close()
    r["plain"] = plain_handle()
    r["blocks"] = tail_blocks(r["plain"]["labels"])
    return r


def test_tail_scope_adds_exactly_the_tails_and_changes_nothing(calibrated):
    r = calibrated
    five, six = r["ranges"]["attn"], r["ranges"]["tail"]
    assert len(five) >= 1 and set(five) < set(six) and all(six[k] == five[k] for k in five)
    blocks = r["blocks"]
    assert len(blocks) == 4
    extra = {k for k in six if k not in five}
    assert extra == {n for b in blocks for n in names_of(b)} and len(extra) == 8
    assert all(six[n] > 0 for n in extra)
    for K, N in ((K1_, C_), (C_, C_)):                                           # both layers are on their kernels' tiles
        assert _lib.conv_plan(1, 1, 1, K, 0, N, BATCH, 16, 16, tile=24 if K == K1_ else 19, flags=4 | 16)["staging"] == 1
    # three ordinary launches per block - absmax over g, a scratch ff.net.2, absmax over its result - in front of the merged launch
    labs = r["labels"]["tail"]
    for b in blocks:
        f2, po = names_of(b)
        i = next(k for k, lab in enumerate(labs) if lab == "absmax " + f2)
        assert labs[i + 1].startswith("gemm1x1 2560->640 @16x16 M=1024 K=2560 " + f2 + " ")
        assert labs[i + 2] == "absmax " + po
        assert labs[i + 3].startswith("gemm1x1 3200->640 ") and f" {f2} + residual + proj_out + residual " in labs[i + 3]
    assert len(labs) == len(r["labels"]["attn"]) + 3 * len(blocks) and not any("_q8" in lab or "+w8a8" in lab for lab in labs)
    assert len(r["outs"]["tail"]) == 4                                           # eager twice, capture + replay
    for a in r["outs"]["attn"] + r["outs"]["tail"] + r["plain"]["outs"][1:]:
        assert np.array_equal(a, r["plain"]["outs"][0])
    # each new range against the oracle's max |x| at that conv
    seen = {}

    def spy(sd, name, x, orig, **kw):
        seen[name] = max(seen.get(name, 0.0), float(x.abs().max()))
        return orig(sd, name, x, **kw)

    sd_t = weights.to_torch({k: v.astype(np.float32) for k, v in state_dict().items()})
    oracle_forward(sd_t, spy)
    devs = {n: abs(six[n] - seen[n]) / seen[n] for n in extra}
    print("observed tail ranges vs oracle:", {n: (round(six[n], 4), round(seen[n], 4), f"{devs[n]:.2e}") for n in sorted(extra)})
    assert max(devs.values()) <= RANGE_DEV_GATE, devs


def check_outputs(q):
    assert len(q["outs"]) == 4
    for a in q["outs"]:                                                          # eager twice, graph capture + replay: bit for bit
        assert np.isfinite(a).all() and np.array_equal(a, q["outs"][0])


def psnr_against_the_fake_quant_oracle(q, plain, recipe, what):
    w8a8 = q["outs"][0]
    assert not np.array_equal(w8a8, plain)
    sd16 = state_dict()
    sd_t = weights.to_torch({k: v.astype(np.float32) for k, v in sd16.items()})
    fq = oracle_forward(sd_t, fake_quant_hook(recipe, sd16))
    p_w8a8, p_plain = psnr.compute_psnr(w8a8, fq), psnr.compute_psnr(plain, fq)
    print(f"W8A8 handle, {what}: PSNR vs the fake-quant oracle {p_w8a8:.2f} dB (the fp16 handle: {p_plain:.2f} dB); "
          f"fp16 handle vs the fp32 oracle {psnr.compute_psnr(plain, oracle_forward(sd_t)):.2f} dB")
    return p_w8a8, p_plain


# PSNR of the handles against the fake-quantizing oracle, measured on the MI355X (LAB_NOTES.md round 31); the gate is the project's
# rule, measured - 6 dB, beside the parameter-free one.
W8A8_TAIL_PSNR_MEASURED = 45.19      # 4 int8 tails, 8 layers (the fp16 handle against the same oracle: 42.70 dB; against the fp32 oracle: 70.10 dB)
W8A8_TAIL_SCOPE_PSNR_MEASURED = 37.67   # all 53 layers of the "tail" scope (the fp16 handle against that oracle: 38.66 dB)


def test_tails_alone_run_from_int8_behind_a_quantizer_launch(calibrated):
    r = calibrated
    blocks = r["blocks"]
    new = {k: v for k, v in r["ranges"]["tail"].items() if k not in r["ranges"]["attn"]}
    recipe = aq.recipe_from_ranges(new)
    assert sorted(recipe) == sorted(n for b in blocks for n in names_of(b))
    q = run_recipe(recipe)
    check_outputs(q)
    labs = q["labels"]
    for b in blocks:                                                             # quantize_q8, ff.net.2 from int8, proj_out from int8, in a row
        f2, po = names_of(b)
        i = next(k for k, lab in enumerate(labs) if lab == "quantize_q8 " + f2)
        assert labs[i - 1].startswith("geglu1x1+ln 640->5120 ")                  # the fp16 GEGLU, folded as ever
        assert labs[i + 1].startswith(f"gemm1x1+w8a8 2560->640 @16x16 M=1024 K=2560 {f2} ")
        assert labs[i + 2].startswith(f"gemm1x1+w8a8 640->640 @16x16 M=1024 K=640 {po} ")
    assert marked_labels(labs) == sorted(recipe) and not any("ff.net.2 + residual + proj_out" in lab for lab in labs)
    assert sum(lab.startswith("quantize_q8 ") for lab in labs) == 4 and len(labs) == len(r["plain"]["labels"]) + 2 * 4
    assert q["info"] == [8, 8, 4 * ((K1_ * C_ + 4 * C_) + (C_ * C_ + 4 * C_))]
    assert q["layers"] == [n for b in blocks for n in names_of(b)]               # build order
    p_w8a8, p_plain = psnr_against_the_fake_quant_oracle(q, r["plain"]["outs"][0], recipe, "4 int8 tails (ff.net.2 + proj_out)")
    assert p_w8a8 > p_plain
    if W8A8_TAIL_PSNR_MEASURED is not None:
        assert p_w8a8 >= W8A8_TAIL_PSNR_MEASURED - 6.0


def test_ff_net_2_alone_and_proj_out_alone(calibrated):
    r = calibrated
    b = r["blocks"][1]
    f2, po = names_of(b)
    rng = r["ranges"]["tail"]
    # proj_out alone stays inside the merged fp16 launch: marked, not applied, the fp16 handle bit for bit
    q = run_recipe({po: rng[po]}, graphs=(False,))
    assert q["info"] == [1, 0, 0] and q["layers"] == [] and q["labels"] == r["plain"]["labels"] and q["used"] == r["plain"]["used"]
    assert all(np.array_equal(a, r["plain"]["outs"][0]) for a in q["outs"])
    # ff.net.2 alone: un-merged from int8, its proj_out an fp16 launch of its own; the other three blocks keep the merged launch
    q = run_recipe({f2: rng[f2]}, graphs=(False,))
    assert q["info"] == [1, 1, K1_ * C_ + 4 * C_] and q["layers"] == [f2]
    labs = q["labels"]
    i = labs.index("quantize_q8 " + f2)
    assert labs[i + 1].startswith(f"gemm1x1+w8a8 2560->640 @16x16 M=1024 K=2560 {f2} ") and labs[i + 2].startswith(f"gemm1x1 640->640 @16x16 M=1024 K=640 {po} ")
    assert sum("ff.net.2 + residual + proj_out" in lab for lab in labs) == 3 and len(labs) == len(r["plain"]["labels"]) + 2
    assert np.isfinite(q["outs"][0]).all() and not np.array_equal(q["outs"][0], r["plain"]["outs"][0])


def test_the_whole_tail_scope_the_geglu_writes_int8_itself(calibrated):
    """The parameter-free gate - closer to the fake-quantizing oracle than the fp16 handle is - is asserted on the recipe of the new
    layers alone (above), as the suites of tiles 19, 20 and 22 do.  A recipe of a whole scope misses it on this model whatever the tails
    do: with dozens of quantizers in a row the handle's and the oracle's rounding decisions stop being the same decisions, and the
    handle ends as far from the oracle as two independent quantizations are.  Measured on the MI355X in one session: the parent's
    whole "attn" scope (45 layers, tails merged in fp16) 40.00 dB against the fp16 handle's 40.92 dB to that oracle; the whole "tail"
    scope (53 layers) 37.67 dB against 38.66 dB; the two handles against each other 39.12 dB.  So the figures are printed, and the
    project's rule - measured - 6 dB - is what gates this recipe."""
    r = calibrated
    blocks = r["blocks"]
    recipe = aq.recipe_from_ranges(r["ranges"]["tail"])
    base = run_recipe(aq.recipe_from_ranges(r["ranges"]["attn"]), graphs=(False,))   # the same handle with the tails merged in fp16
    q = run_recipe(recipe)
    check_outputs(q)
    n_marked, n_applied, nbytes = q["info"]
    assert n_marked == n_applied == len(recipe) and sorted(q["layers"]) == sorted(recipe)
    labs = q["labels"]
    for b in blocks:                                                             # GEGLU with an int8 output, ff.net.2, proj_out, in a row
        f2, po = names_of(b)
        i = next(k for k, lab in enumerate(labs) if lab.startswith(f"gemm1x1+w8a8 2560->640 @16x16 M=1024 K=2560 {f2} "))
        assert labs[i - 1].startswith(f"geglu1x1+q8out+w8a8 640->5120 @16x16 M=1024 K=640 {b}.ff.net.0.proj ")
        assert labs[i + 1].startswith(f"gemm1x1+w8a8 640->640 @16x16 M=1024 K=640 {po} ")
    assert not any(lab.startswith("quantize_q8 ") for lab in labs) and len(labs) == len(base["labels"]) + 4
    assert nbytes == base["info"][2] + 4 * ((K1_ * C_ + 4 * C_) + (C_ * C_ + 4 * C_)) and n_applied == base["info"][1] + 8
    # per block, merged: [Wp W2 | Wp] fp16, its bias, the fp16 product g, the output.  un-merged: ff.net.2's stream, cs and bias, the
    # int8 product - NO fp16 one - and h3; proj_out's stream, cs and bias and the output.  Thirteen allocations, each rounded up to the
    # arena's 256 bytes
    merged = 2 * C_ * (K1_ + C_) + 4 * C_ + 2 * M_ * K1_ + 2 * M_ * C_
    unmerged = (K1_ * C_ + 8 * C_ + M_ * K1_ + 2 * M_ * C_) + (C_ * C_ + 8 * C_ + 2 * M_ * C_)
    assert abs((base["used"] - q["used"]) - 4 * (merged - unmerged)) <= 256 * 13 * 4, (base["used"], q["used"], 4 * (merged - unmerged))
    base_recipe = aq.recipe_from_ranges(r["ranges"]["attn"])
    psnr_against_the_fake_quant_oracle(base, r["plain"]["outs"][0], base_recipe, f'the whole "attn" scope, {len(base_recipe)} layers')
    print(f'the "tail" handle against the "attn" handle: {psnr.compute_psnr(q["outs"][0], base["outs"][0]):.2f} dB')
    p_w8a8, p_plain = psnr_against_the_fake_quant_oracle(q, r["plain"]["outs"][0], recipe, f'the whole "tail" scope, {len(recipe)} layers')
    if W8A8_TAIL_SCOPE_PSNR_MEASURED is not None:
        assert p_w8a8 >= W8A8_TAIL_SCOPE_PSNR_MEASURED - 6.0


def switched_off():
    """what the child process of test_handle_with_the_small_m_gemm_switched_off reports"""
    plain = plain_handle()
    recipe = {n: 6.0 for b in tail_blocks(plain["labels"]) for n in names_of(b)}
    r = run_recipe(recipe)
    return dict(n_recipe=len(recipe), info=r["info"], used=[r["used"], plain["used"]], marked=marked_labels(r["labels"]),
                q8=sum("_q8" in lab for lab in r["labels"]), finite=bool(all(np.isfinite(a).all() for a in r["outs"])),
                equal=bool(all(np.array_equal(a, plain["outs"][0]) for a in r["outs"])))


def test_handle_with_the_small_m_gemm_switched_off():
    """SD_SMGEMM=0 (an A/B switch, read once per process under SD_TUNE) takes tile 12 - and with it tiles 19 and 24 - out of a handle's
    plans: marked, not applied, fp16 arena, no mark in a label, the fp16 handle's output"""
    code = ("import test_w8a8_tail_gpu as t\n"
            "print('RESULT ' + json.dumps(t.switched_off()))\n")
    r, _ = _child(code, dict(SD_TUNE="1", SD_SMGEMM="0"))
    assert r["n_recipe"] == 8 and r["info"] == [8, 0, 0]
    assert r["used"][0] == r["used"][1] and r["marked"] == [] and r["q8"] == 0 and r["finite"] and r["equal"]


# ---- pipeline ----
def test_cli_calibrates_with_the_tail_scope_then_applies_the_recipe(tmp_path, monkeypatch):
    """the mini checkpoint has no tail tile 24 takes: the tail scope observes what the attn scope observes and changes no image, and its
    recipe is applied"""
    from PIL import Image
    from python_hip_stable_diffusion import pipeline as P
    from test_text_encoder_gpu import write_checkpoint_dir
    root = str(tmp_path / "mini-sd")
    os.makedirs(root)
    write_checkpoint_dir(root)
    paths = {scope: str(tmp_path / f"w8a8-{scope}.json") for scope in ("attn", "tail")}
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
    for scope in ("attn", "tail"):
        image = generate("calib-" + scope, "--calibrate-activations", paths[scope], "--calibrate-scope", scope)
        assert np.array_equal(image, plain)                                      # observing changes no image
        recipes[scope] = json.load(open(paths[scope]))
        assert recipes[scope] == aq.recipe_from_ranges(pipes[-1].unet.activation_ranges())
    assert len(recipes["tail"]) >= 1 and set(recipes["attn"]) <= set(recipes["tail"])
    quant = generate("w8a8", "--activation-quantization-recipe", paths["tail"])
    n_marked, n_applied, nbytes = pipes[-1].unet.w8a8_info()
    assert n_marked == len(recipes["tail"]) and n_applied == n_marked and nbytes > 0
    assert quant.shape == plain.shape and not np.array_equal(quant, plain)       # the recipe really is applied
