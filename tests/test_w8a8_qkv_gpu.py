"""GPU suite of the W8A8 self-attention q|k|v projection (plan tile 22, smqkv_i8.hip smqkv_i8_kernel): the operator bit for bit against
a numpy float32 restatement of its arithmetic - every step of it is one correctly rounded IEEE operation, so the restatement is exact
for ALL inputs - then the composition behind layernorm_q8 against a float64 fake-quant reference, the calibration scope ``attn``,
handles whose q|k|v launches run from int8, partial marks, the A/B switch and the CLI flag.

Shapes (B, HW, C, bm) are the smallest the rule admits (C a multiple of 320 from 640 up, HW of 16, an even number of tile rows): 2 x 12 =
24 tiles (three per XCD) at either height, with one sample, with samples smaller than a tile (four of 64 tokens in 128 rows, eight in
256) and with several tile rows per sample (B = 2 at HW = 256).

THE K WALK.  K of this operator IS C, and the rule refuses every C that is not a multiple of 320 from 640 up (C = 320 by name), so the
walk K = 64 s, s = 1 .. 2 * ring + 2, cannot be run through it: there is no launch with fewer than ten K64 stages.  The walk here is every
K the rule admits up to 2880 - 10, 15, 20, 25, 30, 35, 40, 45 stages, which end on every residue of the 8-stage ring (2, 7, 4, 1, 6, 3, 0,
5) and of the 6-stage ring (4, 3, 2, 1, 0, 5, 4, 3) - and includes 640, 1280 and 2560."""
import json
import os
import re

import numpy as np
import pytest

from oracle import psnr, weights
from python_hip_stable_diffusion import HipModel, _lib, activation_quantization as aq
from test_palettize_gemm_gpu import BATCH, CFG, _child
from test_palettize_gpu import gate, h16
from test_w8a8_geglu_gpu import layernorm64, ln_case, run_ln
from test_w8a8_gemm_gpu import forward_twice, marked_labels, oracle_forward, plain_handle, state_dict
from test_w8a8_gpu import RANGE_DEV_GATE, quantize_act

pytestmark = pytest.mark.gpu

SHAPES = [(1, 256, 640, 128), (4, 64, 640, 128), (2, 256, 640, 128), (2, 256, 640, 256), (8, 64, 640, 256)]
ids4 = lambda s: "x".join(map(str, s))   # noqa: E731
K_WALK = tuple(range(640, 2881, 320))
assert {k // 64 % 8 for k in K_WALK} == set(range(8)) and {k // 64 % 6 for k in K_WALK} == set(range(6)) and {640, 1280, 2560} <= set(K_WALK)
Q_PRE = np.float32(1.4426950408889634) / np.float32(8.0)                         # attention_q_prescale(64)
ACT_ABSMAX = np.float32(7.3)


def key_order(S):
    """position p of a V^T row holds token key_order(S)[p]: the two middle 4-token blocks of every 16 tokens swapped (an involution)"""
    return np.arange(S).reshape(-1, 4, 4)[:, [0, 2, 1, 3], :].reshape(-1)


def make_case(shape, seed, with_bias=False, q_scale=1.0, vt_perm=True):
    """random int8 operands over the whole symmetric range with +-127 planted, scales that are no powers of two.  |out| is bounded by
    127^2 * K * s_a * max(s_w) + |bias| < 65504 by construction (asserted in restate)"""
    B, HW, C, bm = shape
    rs = np.random.RandomState(seed)
    wq = rs.randint(-127, 128, size=(3 * C, C)).astype(np.int8)
    xq = rs.randint(-127, 128, size=(B * HW, C)).astype(np.int8)
    for a in (wq, xq):
        a.reshape(-1)[rs.choice(a.size, 24, replace=False)] = np.array([-127, 127] * 12, np.int8)
    w_scale = (1e-3 * (0.8 + 0.4 * rs.rand(3 * C))).astype(np.float32)
    bias = (0.5 * rs.randn(3 * C)).astype(np.float32) if with_bias else None
    return dict(B=B, HW=HW, C=C, bm=bm, xq=xq, wq=wq, w_scale=w_scale, act_absmax=ACT_ABSMAX, bias=bias, q_scale=np.float32(q_scale), vt_perm=vt_perm)


def restate(c, xq=None, dtype=np.float32):
    """the header's arithmetic, one numpy operation per rounded step (dtype float32), or the same formula in float64"""
    xq = c["xq"] if xq is None else xq
    B, HW, C = c["B"], c["HW"], c["C"]
    acc = xq.astype(np.float64) @ c["wq"].astype(np.float64).T                   # exact: |sum| <= 127^2 * K < 2^53
    assert np.array_equal(acc, np.rint(acc)) and np.abs(acc).max() < 2 ** 31
    s_a = np.float32(c["act_absmax"]) / np.float32(127.0)
    cs = (s_a * c["w_scale"].astype(np.float32)).astype(np.float32)              # the host's fp32 product
    v = acc.astype(dtype) * cs.astype(dtype)[None, :]
    if c["bias"] is not None:
        v = v + c["bias"].astype(dtype)[None, :]
    if c["q_scale"] != 1.0:
        v[:, :C] = v[:, :C] * dtype(c["q_scale"])
    assert v.dtype == dtype and np.abs(v).max() < 65504.0                        # no fp16 overflow, checked on the CPU before the launch
    out = v.astype(np.float16) if dtype is np.float32 else v
    vt = np.ascontiguousarray(out[:, 2 * C:].reshape(B, HW, C).transpose(0, 2, 1))
    if c["vt_perm"]:
        vt = np.ascontiguousarray(vt[..., key_order(HW)])
    return np.ascontiguousarray(out[:, :2 * C]), vt


def run_op(c, what="", xq=None):
    """every call: NaN-prefilled outputs with guards behind both (and the library's own poisoned guards on the device), the plan, a second
    call with iters = 3"""
    xq = c["xq"] if xq is None else xq
    B, HW, C = c["B"], c["HW"], c["C"]
    n_qk, n_vt = B * HW * 2 * C, B * C * HW
    bqk, bvt = np.full(n_qk + 4096, np.nan, np.float16), np.full(n_vt + 4096, np.nan, np.float16)
    kw = dict(q_scale=float(c["q_scale"]), vt_perm=c["vt_perm"], bias=c["bias"], bm=c["bm"])
    qk, vt, plan, _ = _lib.qkv_w8a8(xq, c["wq"], c["w_scale"], c["act_absmax"], B, out_qk=bqk, out_vt=bvt, **kw)
    qk, vt = qk.copy(), vt.copy()
    assert qk.shape == (B * HW, 2 * C) and vt.shape == (B, C, HW)
    assert np.isnan(bqk[n_qk:]).all() and np.isnan(bvt[n_vt:]).all(), f"{what}: a guard behind an output was written"
    assert not np.isnan(bqk[:n_qk]).any() and not np.isnan(bvt[:n_vt]).any(), f"{what}: the NaN prefill was not fully overwritten"
    assert plan == [22, 1 if c["bm"] == 128 else 2, 1, 0], plan
    qk2, vt2, plan2, _ = _lib.qkv_w8a8(xq, c["wq"], c["w_scale"], c["act_absmax"], B, iters=3, **kw)
    assert plan2 == plan and np.array_equal(qk.view(np.uint16), qk2.view(np.uint16)) and np.array_equal(vt.view(np.uint16), vt2.view(np.uint16)), \
        f"{what}: two runs differ"
    return qk, vt


def check_exact(c, what):
    want_qk, want_vt = restate(c)
    qk, vt = run_op(c, what)
    assert np.abs(want_qk.astype(np.float32)).max() > 1 and np.abs(want_vt.astype(np.float32)).max() > 1
    assert np.array_equal(qk.view(np.uint16), want_qk.view(np.uint16)), f"{what}: {np.count_nonzero(qk != want_qk)} of {qk.size} q | k elements differ"
    assert np.array_equal(vt.view(np.uint16), want_vt.view(np.uint16)), f"{what}: {np.count_nonzero(vt != want_vt)} of {vt.size} V^T elements differ"


# ---- the operator against the numpy restatement, bit for bit ----
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("q_scale", [1.0, Q_PRE], ids=["q1", "qpre"])
@pytest.mark.parametrize("vt_perm", [False, True], ids=["plain", "perm"])
@pytest.mark.parametrize("shape", SHAPES, ids=ids4)
def test_operator_is_the_numpy_restatement_bit_for_bit(shape, vt_perm, q_scale, with_bias):
    seed = 22000 + 16 * SHAPES.index(shape) + 4 * vt_perm + 2 * (q_scale != 1.0) + with_bias
    check_exact(make_case(shape, seed, with_bias, q_scale, vt_perm), f"{shape} perm={vt_perm} q_scale={q_scale} bias={with_bias}")


@pytest.mark.parametrize("K", K_WALK)
@pytest.mark.parametrize("bm", [128, 256])
def test_k_walk_covers_every_ring_position_the_rule_admits(bm, K):
    """four tile rows at each height: an odd multiple of 320 has 3 K / 160 = 2 (mod 4) tile columns, and the tile count must be a
    multiple of 8"""
    check_exact(make_case((2, 2 * bm, K, bm), 23000 + K + bm, True, Q_PRE, True), f"bm={bm} K={K}")


def test_the_grid_rule_picks_the_tile_height():
    """bm = 0: 128 rows while that grid stays within 256 workgroups"""
    c = make_case((1, 256, 640, 0), 24000)
    want_qk, want_vt = restate(c)
    qk, vt, plan, _ = _lib.qkv_w8a8(c["xq"], c["wq"], c["w_scale"], c["act_absmax"], 1, vt_perm=True)
    assert plan == [22, 1, 1, 0] and np.array_equal(qk.view(np.uint16), want_qk.view(np.uint16)) and np.array_equal(vt.view(np.uint16), want_vt.view(np.uint16))


# ---- composition: layernorm_q8, then the projection ----
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]], ids=ids4)
def test_composition_against_the_float64_fake_quant_reference(shape):
    B, HW, C, bm = shape
    rs = np.random.RandomState(25000 + SHAPES.index(shape))
    w = (rs.randn(3 * C, C) / np.sqrt(C)).astype(np.float32)
    wq, w_scale, _ = _lib.quantize_weight(w)
    x, ln_w, ln_b = ln_case(B * HW, C, 25500 + SHAPES.index(shape))
    y16 = layernorm64(x, ln_w, ln_b).astype(np.float16)                          # the reference quantizes float16(LayerNorm)
    absmax = np.float32(np.abs(y16.astype(np.float32)).max())
    c = dict(B=B, HW=HW, C=C, bm=bm, wq=wq, w_scale=w_scale, act_absmax=absmax, bias=None, q_scale=Q_PRE, vt_perm=True)
    c["xq"] = run_ln(x, ln_w, ln_b, absmax)                                      # activations through layernorm_q8 with an affine
    qk, vt = run_op(c, str(shape))
    ref_qk, ref_vt = restate(c, dtype=np.float64)
    gate(qk, ref_qk, f"W8A8 q|k {shape}: the operator on the device's int8 activations")
    gate(vt, ref_vt, f"W8A8 V^T {shape}: the operator on the device's int8 activations")
    xq64 = quantize_act(y16, absmax)[0]
    print(f"{shape}: {np.count_nonzero(xq64 != c['xq'])} of {xq64.size} int8 activations differ from the float64 LayerNorm's")
    ref_qk, ref_vt = restate(c, xq=xq64, dtype=np.float64)
    gate(qk, ref_qk, f"W8A8 q|k {shape}: layernorm_q8 + qkv_w8a8 against the float64 composition")
    gate(vt, ref_vt, f"W8A8 V^T {shape}: layernorm_q8 + qkv_w8a8 against the float64 composition")
    # sanity, printed and not gated: the folded fp16 launch on the de-quantized weights (its activations are NOT quantized)
    w16 = h16(wq.astype(np.float32) * w_scale[:, None])
    f_qk, f_vt, _ = _lib.qkv_ln(x, ln_w, ln_b, w16, B, q_scale=float(Q_PRE), vt_perm=True)
    print(f"{shape}: PSNR against qkv_ln on the de-quantized weights: q|k {psnr.compute_psnr(qk, f_qk):.1f} dB, V^T {psnr.compute_psnr(vt, f_vt):.1f} dB")
    assert psnr.compute_psnr(qk, f_qk) > 30.0 and psnr.compute_psnr(vt, f_vt) > 30.0     # a transposed or permuted output would be near 0 dB


# ---- refusals that need the device for the valid call in between, in the header's order ----
def test_operator_refusals_and_a_valid_call_right_after():
    c = make_case(SHAPES[0], 26000, True, Q_PRE, True)
    xq, wq, sc = c["xq"], c["wq"], c["w_scale"]
    valid = lambda: check_exact(c, "a valid call right after a refused one")      # noqa: E731
    valid()
    bad_w, bad_x = wq.copy(), xq.copy()
    bad_w[5, 7] = bad_x[3, 9] = -128
    zeros = np.zeros(1920, np.float32)
    refused = [
        dict(args=(xq, wq, sc, 7.3, 1), bm=64, match="bm = 64"),
        dict(args=(xq[:0], wq, sc, 7.3, 1), match="empty"),
        dict(args=(xq, wq, sc, 7.3, 1), bm=256, match="plan tile 22"),           # one row of 256-row tiles
        dict(args=(xq, wq, sc, 7.3, 32), match="plan tile 22"),                  # samples of 8 tokens
        dict(args=(xq[:, :320], wq[:960, :320], sc[:960], 7.3, 1), match="plan tile 22"),
        dict(args=(bad_x, bad_w, zeros, float("nan"), 1), match="act_absmax"),
        dict(args=(bad_x, bad_w, zeros, 7.3, 1), q_scale=float("inf"), match="q_scale"),
        dict(args=(bad_x, bad_w, zeros, 7.3, 1), match="w_scale"),
        dict(args=(bad_x, bad_w, sc, 7.3, 1), match="weight value -128"),
        dict(args=(bad_x, wq, sc, 7.3, 1), match="activation value -128"),
    ]
    for r in refused:
        with pytest.raises(ValueError, match=r["match"]):
            _lib.qkv_w8a8(*r["args"], bm=r.get("bm", 0), q_scale=r.get("q_scale", 1.0))
        valid()


# ---- handles: block channels (64, 640) at 32x32, batch 4 - four self-attentions 640 -> 1920 at M = 1024 ----
C_, N3, M_ = 640, 1920, 1024
PARTS = ("to_q", "to_k", "to_v")


def qkv_blocks(labels):
    """{transformer block: mark} of the fused q|k|v launches 640 -> 1920 at M = 1024, in launch order"""
    r = {}
    for lab in labels:
        m = re.search(r"^gemm1x1(\S*) 640->1920 @16x16 M=1024 K=640 (\S+)\.attn1\.to_qkv #3,1,1,1,640,1920,1024", lab)
        if m:
            r[m.group(2)] = m.group(1)
    return r


def names_of(block):
    return [f"{block}.attn1.{p}" for p in PARTS]


def run_recipe(recipe, graphs=(False, True)):
    """test_w8a8_gemm_gpu.run_recipe with the applied layers in the library's own order"""
    outs, r = [], {}
    for use_graph in graphs:
        m = HipModel(CFG, state_dict(), batch=BATCH, use_graph=use_graph, activation_quantization=recipe)
        outs += forward_twice(m)
        r = dict(info=list(m.w8a8_info()), layers=list(m.w8a8_layers()), used=m.arena_used_bytes, labels=[lab for lab, _, _ in m.profile(1)])
        m.close()
    r["outs"] = outs
    return r


@pytest.fixture(scope="module")
def calibrated():
    r = {"outs": {}, "ranges": {}, "labels": {}}
    for scope in ("geglu", "attn"):
        for use_graph in (False, True):
            m = HipModel(CFG, state_dict(), batch=BATCH, use_graph=use_graph, observe_activations=scope)
            r["outs"].setdefault(scope, []).extend(forward_twice(m))
            if not use_graph:
                r["ranges"][scope] = m.activation_ranges()
                r["labels"][scope] = [lab for lab, _, _ in m.profile(1)]
            m.close()
    r["plain"] = plain_handle()
    r["blocks"] = qkv_blocks(r["plain"]["labels"])
    return r


def test_attn_scope_adds_exactly_the_qkv_projections_and_changes_nothing(calibrated):
    r = calibrated
    four, five = r["ranges"]["geglu"], r["ranges"]["attn"]
    assert len(four) >= 1 and set(four) < set(five) and all(five[k] == four[k] for k in four)
    blocks = r["blocks"]
    assert len(blocks) == 4 and set(blocks.values()) == {"+ln"}                  # the folded fp16 launches
    extra = {k for k in five if k not in four}
    assert extra == {n for b in blocks for n in names_of(b)}
    for b in blocks:                                                             # one observation, three names
        q, k, v = (five[n] for n in names_of(b))
        assert q == k == v and q > 0
    # two ordinary launches per block - LayerNorm + absmax - in front of the launch, which still runs folded
    labs = r["labels"]["attn"]
    for b in blocks:
        i = next(k for k, lab in enumerate(labs) if lab == f"absmax {b}.attn1.to_qkv")
        assert labs[i - 1].startswith("layernorm ") and labs[i - 1].endswith(f" {b}.norm1")
        assert labs[i + 1].startswith("gemm1x1+ln 640->1920 ") and f" {b}.attn1.to_qkv " in labs[i + 1]
    assert len(labs) == len(r["labels"]["geglu"]) + 2 * len(blocks) and not any("layernorm_q8" in lab or "+w8a8" in lab for lab in labs)
    assert len(r["outs"]["attn"]) == 4                                           # eager twice, capture + replay
    for a in r["outs"]["geglu"] + r["outs"]["attn"] + r["plain"]["outs"][1:]:
        assert np.array_equal(a, r["plain"]["outs"][0])
    # each range against the oracle's max |layer_norm_ane(...)| in front of attn1
    seen = {}

    def spy(sd, name, x, orig, **kw):
        seen[name] = max(seen.get(name, 0.0), float(x.abs().max()))
        return orig(sd, name, x, **kw)

    sd_t = weights.to_torch({k: v.astype(np.float32) for k, v in state_dict().items()})
    oracle_forward(sd_t, spy)
    devs = {n: abs(five[n] - seen[n]) / seen[n] for n in extra}
    print("observed norm1 ranges vs oracle:", {n: (round(five[n], 4), round(seen[n], 4), f"{devs[n]:.2e}") for n in sorted(extra)})
    assert max(devs.values()) <= RANGE_DEV_GATE, devs


def fake_quant_hook(recipe, sd16):
    """unet_ref.conv with input and weight of the recipe's layers fake-quantized (the W8A8 scheme in float); a layer without a bias
    (to_q / to_k / to_v) stays without one"""
    import torch
    wfq = {}
    for layer in recipe:
        w = sd16[layer + ".weight"].astype(np.float32)
        q, s, _ = _lib.quantize_weight(w)
        wfq[layer] = torch.from_numpy((q.astype(np.float32) * s.reshape((-1,) + (1,) * (w.ndim - 1))).reshape(w.shape))

    def hook(sd, name, x, orig, **kw):
        if name not in recipe:
            return orig(sd, name, x, **kw)
        s_a = np.float32(recipe[name]) / np.float32(127.0)
        xq = torch.clamp(torch.round(x * float(np.float32(1.0) / s_a)), -127, 127) * float(s_a)
        sub = {name + ".weight": wfq[name]}
        if name + ".bias" in sd:
            sub[name + ".bias"] = sd[name + ".bias"]
        return orig(sub, name, xq, **kw)

    return hook


# PSNR of the handle with the four int8 q|k|v launches against the fake-quantizing oracle, measured on the MI355X (LAB_NOTES.md round
# 29); the gate is the project's rule, measured - 6 dB, beside the parameter-free one.
W8A8_QKV_PSNR_MEASURED = 67.30       # 4 int8 q|k|v launches (the fp16 handle against the same oracle: 61.46 dB; against the fp32 oracle: 70.10 dB)


def test_qkv_launches_run_from_int8_and_follow_the_fake_quant_oracle(calibrated):
    r = calibrated
    blocks = list(r["blocks"])
    new = {k: v for k, v in r["ranges"]["attn"].items() if k not in r["ranges"]["geglu"]}
    recipe = aq.recipe_from_ranges(new)
    assert len(recipe) == 12 and all(k.endswith(PARTS) for k in recipe)
    q = run_recipe(recipe)
    assert len(q["outs"]) == 4
    for a in q["outs"]:                                                          # eager twice, graph capture + replay: bit for bit
        assert np.isfinite(a).all() and np.array_equal(a, q["outs"][0])
    labs = q["labels"]
    assert qkv_blocks(labs) == {b: "+w8a8" for b in blocks}
    assert marked_labels(labs) == sorted(b + ".attn1.to_qkv" for b in blocks)
    for k, lab in enumerate(labs):                                               # a layernorm_q8 launch sits right in front of each marked launch
        if "+w8a8" in lab:
            b = re.search(r"K=640 (\S+)\.attn1\.to_qkv ", lab).group(1)
            assert labs[k - 1] == f"layernorm_q8 {b}.norm1"
    assert sum("layernorm_q8" in lab for lab in labs) == 4 and len(labs) == len(r["plain"]["labels"]) + 4
    assert q["info"] == [12, 12, 4 * (3 * C_ * C_ + 4 * N3)]
    assert q["layers"] == [n for b in blocks for n in names_of(b)]               # to_q, to_k, to_v of each launch, in build order
    # fp16: the folded matrix, colsum, bias.  int8: the stream, cs, norm1's weight and bias, the int8 activations.  Eight allocations,
    # each rounded up to the arena's 256 bytes
    saved = 4 * ((2 * N3 * C_ + 8 * N3) - (N3 * C_ + 4 * N3 + 8 * C_ + M_ * C_))
    assert abs((r["plain"]["used"] - q["used"]) - saved) <= 256 * 8 * 4, (r["plain"]["used"], q["used"], saved)
    # parity, free of parameters: the handle is closer to the fake-quantizing oracle than the fp16 handle is
    w8a8, plain = q["outs"][0], r["plain"]["outs"][0]
    assert not np.array_equal(w8a8, plain)
    sd16 = state_dict()
    sd_t = weights.to_torch({k: v.astype(np.float32) for k, v in sd16.items()})
    fq = oracle_forward(sd_t, fake_quant_hook(recipe, sd16))
    p_w8a8, p_plain = psnr.compute_psnr(w8a8, fq), psnr.compute_psnr(plain, fq)
    print(f"W8A8 handle, 4 int8 q|k|v launches: PSNR vs the fake-quant oracle {p_w8a8:.2f} dB (the fp16 handle: {p_plain:.2f} dB); "
          f"fp16 handle vs the fp32 oracle {psnr.compute_psnr(plain, oracle_forward(sd_t)):.2f} dB")
    assert p_w8a8 > p_plain
    if W8A8_QKV_PSNR_MEASURED is not None:
        assert p_w8a8 >= W8A8_QKV_PSNR_MEASURED - 6.0


def test_partial_marks_keep_the_fp16_launch(calibrated):
    r = calibrated
    blocks = list(r["blocks"])
    rng = {b: r["ranges"]["attn"][names_of(b)[0]] for b in blocks}
    only_q = {names_of(blocks[1])[0]: rng[blocks[1]]}
    three_ranges = {n: rng[blocks[2]] * f for n, f in zip(names_of(blocks[2]), (1.0, 1.0, 1.25))}
    # nothing but partial marks: four marked, none applied, the fp16 handle bit for bit
    q = run_recipe({**only_q, **three_ranges}, graphs=(False,))
    assert q["info"] == [4, 0, 0] and q["layers"] == [] and q["labels"] == r["plain"]["labels"] and q["used"] == r["plain"]["used"]
    for a in q["outs"]:
        assert np.array_equal(a, r["plain"]["outs"][0])
    # beside a block with all three under one range: that block alone runs from int8
    full = {n: rng[blocks[0]] for n in names_of(blocks[0])}
    q = run_recipe({**full, **only_q, **three_ranges}, graphs=(False,))
    assert q["info"] == [7, 3, 3 * C_ * C_ + 4 * N3] and q["layers"] == names_of(blocks[0])
    marks = qkv_blocks(q["labels"])
    assert marks == {b: ("+w8a8" if b == blocks[0] else "+ln") for b in blocks}
    assert [lab for lab in q["labels"] if "layernorm_q8" in lab] == [f"layernorm_q8 {blocks[0]}.norm1"]
    assert np.isfinite(q["outs"][0]).all() and not np.array_equal(q["outs"][0], r["plain"]["outs"][0])


def switched_off():
    """what the child process of test_handle_with_the_qkv_kernel_switched_off reports"""
    plain = plain_handle()
    recipe = {n: 6.0 for b in qkv_blocks(plain["labels"]) for n in names_of(b)}
    r = run_recipe(recipe)
    return dict(n_recipe=len(recipe), info=r["info"], used=[r["used"], plain["used"]], marked=marked_labels(r["labels"]),
                q8=sum("layernorm_q8" in lab for lab in r["labels"]), finite=bool(all(np.isfinite(a).all() for a in r["outs"])),
                equal=bool(all(np.array_equal(a, plain["outs"][0]) for a in r["outs"])))


def test_handle_with_the_qkv_kernel_switched_off():
    """SD_QKV_I8=0 (an A/B switch, read once per process under SD_TUNE) takes plan tile 22 out of every plan: marked, not applied, fp16
    arena, no mark in a label, the fp16 handle's output"""
    code = ("import test_w8a8_qkv_gpu as t\n"
            "print('RESULT ' + json.dumps(t.switched_off()))\n")
    r, _ = _child(code, dict(SD_TUNE="1", SD_QKV_I8="0"))
    assert r["n_recipe"] == 12 and r["info"] == [12, 0, 0]
    assert r["used"][0] == r["used"][1] and r["marked"] == [] and r["q8"] == 0 and r["finite"] and r["equal"]


# ---- pipeline ----
def test_cli_calibrates_with_the_attn_scope_then_applies_the_recipe(tmp_path, monkeypatch):
    """the mini checkpoint has no self-attention tile 22 takes: the attn scope observes what the geglu scope observes and changes no
    image, and its recipe is applied"""
    from PIL import Image
    from python_hip_stable_diffusion import pipeline as P
    from test_text_encoder_gpu import write_checkpoint_dir
    root = str(tmp_path / "mini-sd")
    os.makedirs(root)
    write_checkpoint_dir(root)
    paths = {scope: str(tmp_path / f"w8a8-{scope}.json") for scope in ("geglu", "attn")}
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
    for scope in ("geglu", "attn"):
        image = generate("calib-" + scope, "--calibrate-activations", paths[scope], "--calibrate-scope", scope)
        assert np.array_equal(image, plain)                                      # observing changes no image
        recipes[scope] = json.load(open(paths[scope]))
        assert recipes[scope] == aq.recipe_from_ranges(pipes[-1].unet.activation_ranges())
    assert len(recipes["attn"]) >= 1 and set(recipes["geglu"]) <= set(recipes["attn"])
    for b in {k.rsplit(".", 1)[0] for k in recipes["attn"] if k.endswith(PARTS) and ".attn1." in k}:   # where it names one, it names three, equal
        assert len({recipes["attn"][f"{b}.{p}"] for p in PARTS}) == 1
    quant = generate("w8a8", "--activation-quantization-recipe", paths["attn"])
    n_marked, n_applied, nbytes = pipes[-1].unet.w8a8_info()
    assert n_marked == len(recipes["attn"]) and n_applied == n_marked and nbytes > 0
    assert quant.shape == plain.shape and not np.array_equal(quant, plain)       # the recipe really is applied
