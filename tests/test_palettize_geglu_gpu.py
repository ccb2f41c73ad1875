"""GPU suite of the palettized GEGLU projection (plan tile 16, smgeglu.hip smgeglu_pal_kernel): it decodes its indices, looks them up
in the LUT and - with the LayerNorm fold - multiplies by norm3's weight in front of the MFMAs of smgeglu_kernel, in the same order, with
the same statistics and epilogue, so every comparison against plan tile 13 on the folded lut[indices] is an equality of bits - at the
operator and on a whole handle.

Only 128-row tiles are built (smgeglu.hip says why), so the shapes are the 128-row ones: 8 tiles (one per XCD) up to three per XCD,
both tile orders, and K values that walk the kernel's index half-groups (4 stages of K64) and groups (8) past every slot of its
3-stage ring."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from python_hip_stable_diffusion import HipModel, _lib, hip_model, palettize
from oracle import weights
from test_palettize_gemm_gpu import BATCH, CFG, _state_dict
from test_palettize_gpu import h16, make_palette
from test_smgeglu_gpu import close, geglu_ln_ref

pytestmark = pytest.mark.gpu

NBITS = (1, 2, 4, 6, 8)
SHAPES = [(256, 640), (512, 320), (384, 1280)]        # (M, N2) on 128-row tiles: 2 x 4 = 8 tiles, 4 x 2, 3 x 8 = 24 (three per XCD)
ids2 = lambda s: "x".join(map(str, s))
# K / 64 stages: 1 - one stage, fewer than the two the prologue issues; 2 - exactly the prologue; 3 - the ring once; 4 - the ring
# wraps, exactly one half-group; 5 - the second half-group is read (the first refill of the transit buffer); 7 / 8 / 9 - a group
# boundary (the register words' fragment counter wraps, the stream's second group begins) minus one, on it, plus one; 13 - half-group
# boundaries have met every ring slot (stage 4 in slot 1, 8 in slot 2, 12 in slot 0), 13 stages is no multiple of the ring or a
# half-group; 20 / 40 - the 1280- and 2560-deep projections (2560: the most gamma the LDS holds)
K_SWEEP = (64, 128, 192, 256, 320, 448, 512, 576, 832, 1280, 2560)


def make_case(M, K, N2, nbits, ln=True, with_bias=True, case_no=0):
    """test_smgeglu_gpu.make_case's inputs (rows of different scale around a non-zero mean) over a palette of
    test_palettize_gpu.make_palette: -0, +0, a subnormal, +-65504 and NaN entries no index uses.  The +-65504 entries go only against
    input channel 0, whose activations are small, whose norm weight is 2^-10 and whose norm bias is 0."""
    rs = np.random.RandomState(100000 * nbits + 10 * K + N2 + case_no)
    lut, ordinary, big = make_palette(rs, nbits, K, case_no)
    idx = ordinary[rs.randint(0, len(ordinary), size=(N2, K))].astype(np.uint8)
    if len(big):
        sel = rs.rand(N2) < 0.5
        idx[sel, 0] = big[rs.randint(0, len(big), size=int(sel.sum()))]
    x = h16(rs.randn(M, K) * (1.0 + rs.rand(M, 1)) + 0.5 + 0.5 * rs.rand(M, 1))
    x[:, 0] = h16(np.sign(rs.randn(M)) * 2.0 ** -10 * (1 + rs.rand(M)))          # 65504 x these: at most 128 per product
    bias = (0.1 * rs.randn(N2)).astype(np.float32) if with_bias else None
    ln_w = (1.0 + 0.2 * rs.randn(K)).astype(np.float32) if ln else None
    ln_b = (0.1 * rs.randn(K)).astype(np.float32) if ln else None
    if ln:
        ln_w[0] = 2.0 ** -10                                                      # 65504 x this = 64 (minus an ulp) in the folded weights
        ln_b[0] = 0.0                                                             # ... and 65504 x the norm bias would leave fp16 in the folded bias
    return dict(x=x, lut=lut, idx=idx, bias=bias, ln_w=ln_w, ln_b=ln_b, shape=(M, N2 // 2))


def check_case(c, nbits, what):
    M, half_n = c["shape"]
    n = M * half_n
    buf = np.full(n + 4 * half_n, np.nan, np.float16)
    out, plan, _ = _lib.geglu_palettized(c["x"], c["lut"], c["idx"], nbits, bias=c["bias"], ln_weight=c["ln_w"], ln_bias=c["ln_b"],
                                         bm=128, out=buf)
    out = out.copy()
    assert np.isnan(buf[n:]).all() and not np.isnan(buf[:n]).any(), what
    assert plan == [16, 1, 1, 0], plan
    w = c["lut"][c["idx"]]
    assert np.isfinite(w).all()                                                   # no index reaches a NaN entry
    if c["ln_w"] is not None:                                                     # ... and the folded fp16 weights are finite too
        assert np.isfinite((w.astype(np.float32) * c["ln_w"][None, :]).astype(np.float16)).all()
    ref, _ = _lib.geglu_ln(c["x"], w, c["bias"], c["ln_w"], c["ln_b"], kernel=101)
    ndiff = np.count_nonzero(out.view(np.uint16) != ref.view(np.uint16))
    print(f"{what}: {ndiff} of {n} elements differ from plan tile 13")
    assert ndiff == 0, f"{what}: {ndiff} of {n} elements differ from plan tile 13 on lut[indices]"
    again, _, _ = _lib.geglu_palettized(c["x"], c["lut"], c["idx"], nbits, bias=c["bias"], ln_weight=c["ln_w"], ln_bias=c["ln_b"], bm=0,
                                        iters=3)
    assert np.array_equal(out.view(np.uint16), again.view(np.uint16)), what
    want = geglu_ln_ref(c["x"], w, c["bias"], c["ln_w"], c["ln_b"])
    close(out, want, f"palettized {what}")
    close(ref, want, f"tile 13 {what}")


@pytest.mark.parametrize("nbits", NBITS)
@pytest.mark.parametrize("ln", [True, False], ids=["ln-fold", "plain"])
@pytest.mark.parametrize("shape", SHAPES, ids=ids2)
def test_operator_is_bit_identical_to_the_fp16_geglu_kernel(shape, ln, nbits):
    M, N2 = shape
    check_case(make_case(M, 192, N2, nbits, ln, case_no=SHAPES.index(shape)), nbits, f"M={M} N2={N2} K=192 ln={ln} at {nbits} bits")


@pytest.mark.parametrize("nbits", NBITS)
def test_gamma_product_is_the_host_folds(nbits):
    """norm weights 0, -1, 2^-14 (products in the fp16 subnormal range), 1 + 2^-10 (products on rounding ties: a LUT value
    1.5 * 2^e times it lies exactly between two fp16 numbers) and 8, taking turns over the channels."""
    c = make_case(256, 192, 640, nbits, True, case_no=3)
    rs = np.random.RandomState(nbits)
    lut, ordinary, _ = make_palette(rs, nbits, 192, 3)
    if len(ordinary) >= 3:
        lut[ordinary[-1]] = np.float16(0.046875)                                  # 1.5 * 2^-5
    c["lut"] = lut
    c["idx"] = ordinary[rs.randint(0, len(ordinary), size=c["idx"].shape)].astype(np.uint8)
    gamma = np.array([0.0, -1.0, 2.0 ** -14, 1.0 + 2.0 ** -10, 8.0], np.float32)
    c["ln_w"] = gamma[np.arange(192) % 5].copy()
    folded = (lut[c["idx"]].astype(np.float32) * c["ln_w"][None, :]).astype(np.float16)
    assert np.isfinite(folded).all()
    tiny = np.abs(folded.astype(np.float32))
    assert ((tiny > 0) & (tiny < 2.0 ** -14)).any()                               # subnormal products do occur
    if len(ordinary) >= 3:
        exact = lut[c["idx"]].astype(np.float64) * c["ln_w"][None, :].astype(np.float64)
        assert (np.abs(exact - 0.046875 * (1.0 + 2.0 ** -10)) == 0).any()         # ... and so does the tie
    check_case(c, nbits, f"gamma arithmetic at {nbits} bits")


@pytest.mark.parametrize("nbits", NBITS)
@pytest.mark.parametrize("K", K_SWEEP)
def test_index_half_groups_walk_past_every_ring_slot(K, nbits):
    """K_SWEEP (above) says which K does what."""
    check_case(make_case(256, K, 640, nbits, True), nbits, f"M=256 N2=640 K={K} at {nbits} bits")


@pytest.mark.parametrize("nbits", NBITS)
@pytest.mark.parametrize("ln,with_bias", [(True, False), (False, True), (False, False)], ids=["no-bias", "no-fold", "neither"])
def test_bias_and_fold_absent(ln, with_bias, nbits):
    check_case(make_case(256, 576, 640, nbits, ln, with_bias), nbits, f"K=576 ln={ln} bias={with_bias} at {nbits} bits")


def _child(code, env_extra):
    env = dict(os.environ, **env_extra)
    head = "import sys, json; sys.path[:0] = [%r, %r, %r]\n" % (ROOT, os.path.join(ROOT, "ml-stable-diffusion_amd"), os.path.join(ROOT, "tests"))
    p = subprocess.run([sys.executable, "-c", head + code], env=env, capture_output=True, text=True, timeout=900)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert p.returncode == 0 and line, p.stdout[-2000:] + p.stderr[-2000:]
    return json.loads(line[0][len("RESULT "):]), p.stderr


def n_fast_by_the_rule(M, N2, K, bm=128):
    """conv_plan.cpp choose_tile_order on the fp16 operand sizes (both fit an L2 here)"""
    a, w, nbm, nbn = 2.0 * M * K, 2.0 * N2 * K, M // bm, N2 // 160
    assert a <= 3.5e6 and w <= 3.5e6
    return int(nbn > 1 and a + w * min(8, nbm) < w + a * min(8, nbn))


def test_tile_16_takes_the_tile_order_of_tile_13():
    want = {(M, N2): n_fast_by_the_rule(M, N2, 192) for M, N2 in SHAPES}
    assert set(want.values()) == {0, 1}, want                                     # both orders are on the table
    code = ("import test_palettize_geglu_gpu as t\n"
            "for M, N2 in t.SHAPES:\n"
            "    t.check_case(t.make_case(M, 192, N2, 6), 6, str((M, N2)))\n"
            "print('RESULT ' + json.dumps(True))\n")
    _, err = _child(code, dict(SD_TUNE="1", SD_LOG_CONVS="1"))
    orders = {}
    for m in re.finditer(r"M=(\d+) N=(\d+) K=192 mode=2 tile=(\d+) bm=128 n_fast=(\d)( bits=6)?", err):
        orders.setdefault(int(m.group(3)), {})[(int(m.group(1)), int(m.group(2)))] = int(m.group(4))
        assert (m.group(5) is not None) == (m.group(3) == "16"), m.group(0)      # tile 16's line says bits=
    assert set(orders) == {13, 16} and orders[16] == orders[13] == want, (orders, want)


def test_operator_refusals_and_a_valid_call_right_after():
    c = make_case(256, 128, 640, 4)
    x, lut, idx = c["x"], c["lut"], c["idx"]
    g, b = c["ln_w"], c["ln_b"]
    bad = idx.copy()
    bad[5, 7] = 16
    refused = [
        dict(args=(x, lut[:8], idx % 8, 3), match="nbits"),
        dict(args=(x, lut, idx, 4), bm=64, match="bm"),
        dict(args=(x[:0], lut, idx, 4), match="empty"),
        dict(args=(x, lut, idx, 4), ln_weight=g, match="go together"),
        dict(args=(x, lut, bad, 4), match="index 16"),
        dict(args=(x, lut, idx[:480], 4), match="plan tile 16"),                 # 2 x 3 tiles
        dict(args=(x[:200], lut, idx, 4), match="plan tile 16"),                 # ragged M
        dict(args=(x[:, :32], lut, idx[:, :32], 4), match="plan tile 16"),       # C = 32
        dict(args=(np.concatenate([x, x]), lut, idx, 4), bm=256, match="256 is not built"),
    ]
    for r in refused:
        with pytest.raises(ValueError, match=r["match"]):
            _lib.geglu_palettized(*r["args"], bm=r.get("bm", 0), ln_weight=r.get("ln_weight"))
        check_case(c, 4, "a valid call right after a refused one")


# ---- handle: the two-level UNet of test_palettize_gemm_gpu; its four 640 -> 5120 GEGLUs run at M = 1024 on 128-row tiles ----
ENDINGS = ("ff.net.0.proj", "proj_in", "to_out.0", "proj_out", "ff.net.2")
RECIPES = {"6 bits": 6, "mixed 4 / 8 / 16": (4, 8, 16)}
GEGLU_N2, GEGLU_K = 5120, 640


def stores(recipe, endings=ENDINGS):
    sd16 = _state_dict()
    pal = hip_model.Weights(sd16)
    modules = [m for m in palettize.palettizable(pal, min_size=1000) if m.endswith(endings)]
    assert len(modules) == 4 * len(endings) + 4 * ("to_out.0" in endings), modules   # four transformer blocks; to_out.0 is attn1's and attn2's
    modules.sort(key=lambda m: (not m.endswith("ff.net.0.proj"), m))           # the GEGLUs first: a mixed recipe gives them every width
    bits = {m: (recipe if isinstance(recipe, int) else recipe[i % len(recipe)]) for i, m in enumerate(modules)}
    palettize.apply(pal, recipe=bits)
    plain = hip_model.Weights({k: (pal.read(k).astype(np.float16) if k.endswith(".weight") and pal.palette_bits(k) else v) for k, v in sd16.items()})
    return pal, plain, bits


def compare_handles(recipe, endings=ENDINGS):
    """the palettized and the de-palettized handle, eager twice, then graph capture + replay"""
    pal, plain, bits = stores(recipe, endings)
    hw = CFG["sample_size"]
    inputs = dict(sample=weights.seeded_normal((BATCH, 4, hw, hw), 1).astype(np.float16), timestep=np.full(BATCH, 981, np.float16),
                  encoder_hidden_states=weights.seeded_normal((BATCH, CFG["cross_attention_dim"], 1, 77), 2).astype(np.float16))
    r = {"bits": bits, "equal": []}
    for use_graph in (False, True):
        hp = HipModel(CFG, pal, batch=BATCH, use_graph=use_graph)
        hq = HipModel(CFG, plain, batch=BATCH, use_graph=use_graph)
        for _ in range(2):
            a, b = hp(**inputs)["noise_pred"], hq(**inputs)["noise_pred"]
            r["equal"].append(bool(np.isfinite(a).all() and np.array_equal(a, b)))
        r["info"], r["info_plain"] = list(hp.palette_info()), list(hq.palette_info())
        r["used"] = [hp.arena_used_bytes, hq.arena_used_bytes]
        r["labels"] = [lab for lab, _, _ in hp.profile(1)]
        hp.close()
        hq.close()
    pal.close()
    plain.close()
    return r


def streamed_geglus(r, fold=True):
    """the marked GEGLU labels, each checked against its own width: [(module, bits)]"""
    marked = [lab for lab in r["labels"] if "+pal" in lab and "ff.net.0.proj" in lab]
    out = []
    for lab in marked:
        m = re.search(r"^geglu\+pal(\d+)(\+ln)? 640->5120 @16x16 M=1024 K=640 (\S+)", lab)
        assert m and r["bits"][m.group(3)] == int(m.group(1)) and (m.group(2) is not None) == fold, lab
        out.append((m.group(3), int(m.group(1))))
    return out


@pytest.mark.parametrize("recipe", list(RECIPES))
def test_handle_from_a_palettized_store_equals_the_depalettized_one(recipe):
    r = compare_handles(RECIPES[recipe])
    n_pal, n_streamed, stream_bytes = r["info"]
    assert r["info_plain"] == [0, 0, 0]
    assert all(r["equal"]) and len(r["equal"]) == 4, r["equal"]                  # eager twice, graph capture + replay
    assert n_pal == sum(1 for b in r["bits"].values() if b != 16)
    marked = [lab for lab in r["labels"] if "+pal" in lab]
    geglus = streamed_geglus(r)
    wanted = [m for m in r["bits"] if m.endswith("ff.net.0.proj") and r["bits"][m] != 16]
    assert sorted(m for m, _ in geglus) == sorted(wanted) and len(wanted) >= 2, (geglus, wanted)
    assert len(wanted) == 4 or recipe != "6 bits"
    assert all(lab.startswith(("geglu+pal", "gemm1x1+pal")) for lab in marked), marked
    assert n_streamed == len(marked)
    # a streamed projection dropped its fp16 [N][K] upload and holds its stream and LUT (stream_bytes) instead; a streamed GEGLU
    # also holds norm3's weight as fp32.  Every allocation is a multiple of the arena's 256-byte alignment
    n_gemm = len(marked) - len(geglus)
    dropped = 2 * 640 * 640 * n_gemm + 2 * GEGLU_N2 * GEGLU_K * len(geglus)
    added = stream_bytes + 4 * GEGLU_K * len(geglus)
    for _, b in geglus:                                                          # the stream's size formula, in passing
        assert (GEGLU_N2 // 16) * 2 * b * 1024 <= stream_bytes
    used_pal, used_plain = r["used"]
    assert abs((used_plain - used_pal) - (dropped - added)) <= 256 * (2 * n_gemm + 3 * len(geglus)), (r["used"], r["info"])
    assert used_pal < used_plain


def test_handle_with_the_geglu_kernel_switched_off_uploads_fp16():
    """SD_SMGEGLU=0 (an A/B switch, read once per process under SD_TUNE): no GEGLU streams and the bits are the de-palettized
    handle's; with round 16's streaming projections left out of the recipe nothing streams at all and the arenas are equal."""
    code = ("import test_palettize_geglu_gpu as t\n"
            "r = t.compare_handles(6, ('ff.net.0.proj', 'proj_out', 'ff.net.2'))\n"
            "print('RESULT ' + json.dumps({k: r[k] for k in ('info', 'equal', 'used', 'labels')}))\n")
    r, _ = _child(code, dict(SD_TUNE="1", SD_SMGEGLU="0"))
    assert r["info"] == [12, 0, 0], r["info"]
    assert all(r["equal"]) and len(r["equal"]) == 4
    assert not [lab for lab in r["labels"] if "+pal" in lab]
    assert r["used"][0] == r["used"][1]


def test_handle_without_the_layernorm_fold_streams_the_plain_geglu():
    """SD_NO_LN_FOLD=1: the LayerNorm is a launch of its own and the plain GEGLU behind it streams, without a norm weight."""
    code = ("import test_palettize_geglu_gpu as t\n"
            "r = t.compare_handles(6)\n"
            "r['geglus'] = t.streamed_geglus(r, fold=False)\n"
            "print('RESULT ' + json.dumps({k: r[k] for k in ('info', 'equal', 'geglus')}))\n")
    r, _ = _child(code, dict(SD_TUNE="1", SD_NO_LN_FOLD="1"))
    assert len(r["geglus"]) == 4 and r["info"][1] >= 4, r
    assert all(r["equal"]) and len(r["equal"]) == 4
