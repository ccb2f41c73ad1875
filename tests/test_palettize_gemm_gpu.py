"""GPU suite of the palettized small-M 1x1 GEMM (plan tile 15, smgemm.hip smgemm_pal_kernel): it decodes its indices in front of the
MFMAs of smgemm_kernel, in the same order, with the same epilogue, so every comparison against plan tile 12 on lut[indices] is an
array_equal - at the operator and on a whole handle.

Shapes are the smallest the kernel can still go wrong at: 8 tiles (one per XCD) up to 3 and 4 per XCD, both tile heights, both tile
orders, and K values that walk the boundary of an index group (8 stages of K64) past every position of the activation ring (16
stages at 32-row tiles, 8 at 64-row tiles): one stage, exactly one group, a group plus one stage, the ring wrap, two groups, the 20
and 40 stages of the 1280- and 2560-deep projections."""
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle import unet_ref, weights
from python_hip_stable_diffusion import HipModel, _lib, hip_model, palettize
from test_palettize_gpu import gate, h16, make_palette

pytestmark = pytest.mark.gpu

NBITS = (1, 2, 4, 6, 8)

# name -> (B, H, W, N, bm); M = B * H * W
SHAPES = {
    "bm32 M=64 N=320 (8 tiles)": (1, 8, 8, 320, 32),
    "bm32 M=128 N=160": (2, 8, 8, 160, 32),
    "bm32 M=96 N=640 (3 tiles per XCD)": (1, 8, 12, 640, 32),
    "bm32 M=512 N=160": (2, 16, 16, 160, 32),
    "bm32 M=64 N=1280": (1, 8, 8, 1280, 32),
    "bm32 M=1280 N=160 (n-fast order)": (5, 16, 16, 160, 32),
    "bm64 M=128 N=320": (2, 8, 8, 320, 64),
    "bm64 M=256 N=160": (1, 16, 16, 160, 64),
}
# ring depth NST = 16 / 8 at bm 32 / 64: 64 NST and 64 (NST + 1) are 1024, 1088 / 512, 576
K_SWEEP = (64, 512, 576, 640, 704, 1024, 1088, 1280, 2560)
K_SHAPES = ("bm32 M=64 N=320 (8 tiles)", "bm64 M=128 N=320")


def make_case(shape, K, nbits, with_bias=True, with_res=True):
    B, H, W, N, bm = SHAPES[shape]
    case_no = list(SHAPES).index(shape)
    rs = np.random.RandomState(100000 * nbits + 10 * K + case_no)
    lut, ordinary, big = make_palette(rs, nbits, K, case_no)
    idx = ordinary[rs.randint(0, len(ordinary), size=(N, K))].astype(np.uint8)
    if len(big):
        sel = rs.rand(N) < 0.5
        idx[sel, 0] = big[rs.randint(0, len(big), size=int(sel.sum()))]
    x = h16(rs.randn(B, K, H, W))
    x[:, 0] = h16(np.sign(rs.randn(B, H, W)) * 2.0 ** -10 * (1 + rs.rand(B, H, W)))   # 65504 x these: at most 128 per product
    bias = (0.1 * rs.randn(N)).astype(np.float32) if with_bias else None
    res = h16(rs.randn(B, N, H, W)) if with_res else None
    return dict(x=x, lut=lut, idx=idx, bias=bias, res=res, bm=bm, shape=(B, N, H, W))


def torch_reference(c):
    import torch
    w = torch.from_numpy(c["lut"][c["idx"]].astype(np.float32))
    y = torch.einsum("bkhw,nk->bnhw", torch.from_numpy(c["x"].astype(np.float32)), w)
    if c["bias"] is not None:
        y = y + torch.from_numpy(c["bias"])[None, :, None, None]
    if c["res"] is not None:
        y = y + torch.from_numpy(c["res"].astype(np.float32))
    return y.numpy()


def check_case(c, nbits, what):
    n = int(np.prod(c["shape"]))
    guard = 4 * c["shape"][1] * c["shape"][3]
    buf = np.full(n + guard, np.nan, np.float16)
    out, plan, _ = _lib.gemm_palettized(c["x"], c["lut"], c["idx"], nbits, bias=c["bias"], res=c["res"], bm=c["bm"], out=buf)
    out = out.copy()
    assert np.isnan(buf[n:]).all() and not np.isnan(buf[:n]).any(), what
    assert plan == [15, 1 if c["bm"] == 32 else 2, 1, 0], plan
    w = c["lut"][c["idx"]]
    assert np.isfinite(w).all()                                                 # no index reaches a NaN entry
    ref, _ = _lib.conv2d(c["x"], w[..., None, None], c["bias"], c["res"], tile=141 if c["bm"] == 32 else 142)
    ndiff = np.count_nonzero(out.view(np.uint16) != ref.view(np.uint16))
    assert ndiff == 0, f"{what}: {ndiff} of {n} elements differ from plan tile 12 on lut[indices]"
    again, _, _ = _lib.gemm_palettized(c["x"], c["lut"], c["idx"], nbits, bias=c["bias"], res=c["res"], bm=c["bm"], iters=3)
    assert np.array_equal(out.view(np.uint16), again.view(np.uint16)), what
    want = torch_reference(c)
    gate(out, want, f"palettized {what}")
    gate(ref, want, f"tile 12 {what}")


@pytest.mark.parametrize("nbits", NBITS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_operator_is_bit_identical_to_the_fp16_small_m_gemm(shape, nbits):
    check_case(make_case(shape, 192, nbits), nbits, f"{shape} K=192 at {nbits} bits")


@pytest.mark.parametrize("nbits", NBITS)
@pytest.mark.parametrize("K", K_SWEEP)
@pytest.mark.parametrize("shape", K_SHAPES)
def test_index_group_boundary_walks_past_every_ring_position(shape, K, nbits):
    check_case(make_case(shape, K, nbits), nbits, f"{shape} K={K} at {nbits} bits")


@pytest.mark.parametrize("nbits", NBITS)
@pytest.mark.parametrize("with_bias,with_res", [(False, False), (True, False), (False, True)])
def test_bias_and_residual_absent(with_bias, with_res, nbits):
    for shape in K_SHAPES:
        check_case(make_case(shape, 576, nbits, with_bias, with_res), nbits, f"{shape} K=576 bias={with_bias} res={with_res} at {nbits} bits")


def _child(code, env_extra):
    env = dict(os.environ, **env_extra)
    head = "import sys, json; sys.path[:0] = [%r, %r, %r]\n" % (ROOT, os.path.join(ROOT, "ml-stable-diffusion_amd"), os.path.join(ROOT, "tests"))
    p = subprocess.run([sys.executable, "-c", head + code], env=env, capture_output=True, text=True, timeout=900)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert p.returncode == 0 and line, p.stdout[-2000:] + p.stderr[-2000:]
    return json.loads(line[0][len("RESULT "):]), p.stderr


def test_both_tile_orders_occur():
    """The launcher picks the tile order by choose_tile_order from the fp16 operand sizes, as plan tile 12 does.  By that rule both
    M = 512 / N = 160 and M = 64 / N = 1280 run m-fast (n_fast = 0); M = 1280 / N = 160 runs n-fast.  Read from the launch log."""
    code = ("import test_palettize_gemm_gpu as t\n"
            "for s in ('bm32 M=512 N=160', 'bm32 M=64 N=1280', 'bm32 M=1280 N=160 (n-fast order)'):\n"
            "    t.check_case(t.make_case(s, 192, 6), 6, s)\n"
            "print('RESULT ' + json.dumps(True))\n")
    _, err = _child(code, dict(SD_TUNE="1", SD_LOG_CONVS="1"))
    orders = {}
    for m in re.finditer(r"M=(\d+) N=(\d+) K=192 mode=0 tile=(\d+) bm=32 n_fast=(\d)", err):
        orders.setdefault(int(m.group(3)), {})[(int(m.group(1)), int(m.group(2)))] = int(m.group(4))
    assert set(orders) == {12, 15} and orders[15] == orders[12], orders           # tile 15 takes tile 12's order, case by case
    assert orders[15] == {(512, 160): 0, (64, 1280): 0, (1280, 160): 1}, orders


def test_operator_refusals_and_a_valid_call_right_after():
    c = make_case("bm32 M=64 N=320 (8 tiles)", 128, 4)
    x, lut, idx = c["x"], c["lut"], c["idx"]
    bad = idx.copy()
    bad[5, 7] = 16
    refused = [
        dict(args=(x, lut[:8], idx % 8, 3), match="nbits"),
        dict(args=(x, lut, idx, 4), bm=48, match="bm"),
        dict(args=(x, lut, bad, 4), match="index 16"),
        dict(args=(x, lut, idx[:96], 4)),                                        # N = 96
        dict(args=(h16(np.zeros((1, 128, 8, 9))), lut, idx, 4)),                 # M = 72
        dict(args=(x[:, :32], lut, idx[:, :32], 4)),                             # Cin = 32
        dict(args=(h16(np.zeros((1, 128, 8, 12))), lut, idx, 4)),                # 12 tiles
    ]
    for r in refused:
        with pytest.raises(ValueError, match=r.get("match")):
            _lib.gemm_palettized(*r["args"], bm=r.get("bm", 0))
        check_case(c, 4, "a valid call right after a refused one")


# ---- handle ----
CFG = unet_ref.make_config(sample_size=32, block_out_channels=(64, 640), down_block_types=(unet_ref.DN, unet_ref.CA),
                           up_block_types=(unet_ref.CAUP, unet_ref.UP), layers_per_block=1, attention_head_dim=(1, 10),
                           cross_attention_dim=128)
BATCH = 4
ENDINGS = ("proj_in", "to_out.0", "proj_out", "ff.net.2")
RECIPES = {"6 bits": 6, "mixed 4 / 8 / 16": (4, 8, 16)}


@functools.lru_cache(maxsize=None)
def _state_dict():
    return weights.make_state_dict(unet_ref.unet_param_shapes(CFG), seed=44, dtype=np.float16)


def stores(recipe):
    sd16 = _state_dict()
    pal = hip_model.Weights(sd16)
    modules = [m for m in palettize.palettizable(pal, min_size=1000) if m.endswith(ENDINGS)]
    assert len(modules) == 20, modules
    bits = {m: (recipe if isinstance(recipe, int) else recipe[i % len(recipe)]) for i, m in enumerate(modules)}
    palettize.apply(pal, recipe=bits)
    plain = hip_model.Weights({k: (pal.read(k).astype(np.float16) if k.endswith(".weight") and pal.palette_bits(k) else v) for k, v in sd16.items()})
    return pal, plain, bits


def compare_handles(recipe):
    """test_palettize_gpu.compare_handles over this UNet: the palettized and the de-palettized handle, eager twice, then graph
    capture + replay."""
    pal, plain, bits = stores(recipe)
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
        r["device_bytes"] = [hp.device_bytes, hq.device_bytes]
        r["labels"] = [lab for lab, _, _ in hp.profile(1)]
        hp.close()
        hq.close()
    pal.close()
    plain.close()
    return r


@pytest.mark.parametrize("recipe", list(RECIPES))
def test_handle_from_a_palettized_store_equals_the_depalettized_one(recipe):
    r = compare_handles(RECIPES[recipe])
    n_pal, n_streamed, stream_bytes = r["info"]
    assert r["info_plain"] == [0, 0, 0]
    assert all(r["equal"]) and len(r["equal"]) == 4, r["equal"]                 # eager twice, graph capture + replay
    assert n_pal == sum(1 for b in r["bits"].values() if b != 16)
    marked = [lab for lab in r["labels"] if "+pal" in lab]
    assert all(lab.startswith("gemm1x1+pal") for lab in marked), marked
    # the twelve 640 -> 640 projections proj_in / attn1.to_out.0 / attn2.to_out.0 stream, less those the recipe left at 16 bits
    eligible = [m for m in r["bits"] if m.endswith(("proj_in", "to_out.0"))]
    assert len(eligible) == 12
    assert n_streamed == len(marked) == sum(1 for m in eligible if r["bits"][m] != 16)
    assert n_streamed == (12 if recipe == "6 bits" else 12 - sum(1 for m in eligible if r["bits"][m] == 16)) and n_streamed >= 6
    for lab in marked:                                                          # ... each at its own width
        m = re.search(r"^gemm1x1\+pal(\d+) 640->640 @16x16 M=1024 K=640 (\S+)", lab)
        assert m and r["bits"][m.group(2)] == int(m.group(1)), lab
    # proj_out and ff.net.2 are palettized in the store but folded into the merged tail on fp16
    assert not [lab for lab in marked if "proj_out" in lab or "ff.net.2" in lab]
    assert [lab for lab in r["labels"] if "ff.net.2" in lab and "proj_out" in lab]
    used_pal, used_plain = r["used"]
    # a streamed op dropped its fp16 [N][K] upload - 2 bytes per weight - and holds stream_bytes instead; every allocation is a
    # multiple of the arena's 256-byte alignment
    assert abs((used_plain - used_pal) - (2 * 640 * 640 * n_streamed - stream_bytes)) <= 256 * n_streamed, (r["used"], r["info"])
    assert used_pal < used_plain and r["device_bytes"][0] <= r["device_bytes"][1]


def test_handle_with_the_small_m_gemm_switched_off_uploads_fp16():
    """SD_SMGEMM=0 (an A/B switch, read once per process under SD_TUNE): no projection streams, the bits and the arena are the
    de-palettized handle's."""
    code = ("import test_palettize_gemm_gpu as t\n"
            "r = t.compare_handles(6)\n"
            "print('RESULT ' + json.dumps({k: r[k] for k in ('info', 'equal', 'used')}))\n")
    r, _ = _child(code, dict(SD_TUNE="1", SD_SMGEMM="0"))
    assert r["info"][0] == 20 and r["info"][1] == 0 and r["info"][2] == 0
    assert all(r["equal"]) and len(r["equal"]) == 4
    assert r["used"][0] == r["used"][1]
