"""Operator tests of the three ConvDesc fields the UNet / VAE builders set and sd_op_conv2d never does, through sd_op_conv2d_ex:
  * temb / temb_stride - the per-sample time-embedding row of every resnet conv1 (unet.py:477), through each kernel family's own
    epilogue: tile_epilogue (block-uniform constant, or per-row sample index when a tile straddles samples), the halo kernel,
    splitk_reduce_kernel, reduce_twin_kernel and the direct kernels;
  * x1 / C1 - the K order k = tap * (C0 + C1) + c of a two-source conv (the up blocks' torch.cat, unet.py:213-216) on the im2col
    tiles, the rings, the halo kernel and the weight-streaming kernel;
  * pad = 0 with stride 2 - the VAE encoder's F.pad(x, (0, 1, 0, 1)) downsample.
Reference: torch in fp64 on the fp16-rounded inputs.  Tolerance: the operator bar of tests/test_ops_gpu.py (`close` is copied from
there): PSNR >= 60 dB and max |err| <= 4e-3 * max|ref| + 1e-3.  The twin output uses the four comparisons and bounds of
tests/test_round5_gpu.py::test_groupnorm_twin_of_the_slab_combine.

The inputs make a wrong index visible: temb[b][n] = 1.5 b + 0.3 randn, every (b, n) at least 0.5 away from every other sample's value
at n (asserted; a column that misses the distance is drawn again - at 1280 columns no seed gives a draw without one), x0 ~ randn,
x1 ~ 0.5 randn + 1, batch 3.  The library keeps the temb rows inside a wider buffer poisoned with 1e30, so a neighbouring column or
row is garbage.  test_close_rejects_the_mutants (CPU) shows that each wrong index is far outside the tolerance.

Every test asserts on the plan the launch reports (plan = [tile, staging, splitk, slab], -1 = direct kernels), and the last test
checks that every epilogue family was reached by a passing case."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import psnr
from python_hip_stable_diffusion import _lib

gpu = pytest.mark.gpu


def close(got, ref, what, min_psnr=60.0, rel=4e-3):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    p = psnr.compute_psnr(got, ref)
    err = np.abs(got - ref).max()
    bound = rel * np.abs(ref).max() + 1e-3
    print(f"{what}: PSNR {p:.1f} dB, max|err| {err:.3e} (bound {bound:.3e})")
    assert p >= min_psnr and err <= bound, f"{what}: PSNR {p:.1f} dB, max|err| {err:.3e} (bound {bound:.3e})"


def h16(a):
    return np.asarray(a, np.float32).astype(np.float16)


def separated_temb(rs, b, n):
    """temb[b][n] = 1.5 b + 0.3 randn with every column's samples >= 0.5 apart (columns that miss it are drawn again)."""
    t = 1.5 * np.arange(b)[:, None] + 0.3 * rs.randn(b, n)
    for _ in range(1000):
        d = np.abs(t[:, None, :] - t[None, :, :]) + 1e9 * np.eye(b)[:, :, None]
        bad = np.nonzero(d.min(axis=(0, 1)) < 0.5)[0]
        if bad.size == 0:
            break
        t[:, bad] = 1.5 * np.arange(b)[:, None] + 0.3 * rs.randn(b, bad.size)
    t = t.astype(np.float32)
    for i in range(b):
        for j in range(b):
            assert i == j or (np.abs(t[i] - t[j]) >= 0.5).all(), "temb rows of two samples are too close to tell a wrong index"
    return t


def out_size(h, w, k, stride, up, pad_mode):
    f = 2 if up else 1
    extra = 1 if pad_mode else 2 * (k // 2)
    return (h * f + extra - k) // stride + 1, (w * f + extra - k) // stride + 1


@functools.lru_cache(maxsize=None)
def inputs(b, c0, c1, h, w, cout, k, stride=1, up=False, pad_mode=0):
    """The tensors of one case, fp16-rounded where the library takes fp16; built once and shared (never modified)."""
    rs = np.random.RandomState(1000 * b + 100 * k + c0 + 3 * c1 + 7 * h + 11 * w + cout + 13 * stride + 17 * int(up) + 19 * pad_mode)
    ho, wo = out_size(h, w, k, stride, up, pad_mode)
    t = {"x0": h16(rs.randn(b, c0, h, w)),
         "x1": h16(0.5 * rs.randn(b, c1, h, w) + 1.0) if c1 else None,
         "w": h16(rs.randn(cout, c0 + c1, k, k) / np.sqrt((c0 + c1) * k * k)),
         "bias": (0.1 * rs.randn(cout)).astype(np.float32),
         "temb": separated_temb(rs, b, cout),
         "res": h16(rs.randn(b, cout, ho, wo)),
         "geom": (k, stride, up, pad_mode)}
    for v in t.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return t


def conv_ref64(t, w=None, symmetric_pad=False):
    """fp64 conv of the (concatenated, upsampled, padded) input, without the epilogue terms."""
    k, stride, up, pad_mode = t["geom"]
    x = torch.from_numpy(t["x0"].astype(np.float64))
    if t["x1"] is not None:
        x = torch.cat([x, torch.from_numpy(t["x1"].astype(np.float64))], dim=1)
    if up:
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    pad = k // 2
    if pad_mode and not symmetric_pad:
        x = F.pad(x, (0, 1, 0, 1))
        pad = 0
    return F.conv2d(x, torch.from_numpy((t["w"] if w is None else w).astype(np.float64)), None, stride=stride, padding=pad)


@functools.lru_cache(maxsize=None)
def _conv_ref64_cached(key):
    return conv_ref64(inputs(*key))


def ref64(key, bias, temb, res, temb_rows=None):
    t = inputs(*key)
    y = _conv_ref64_cached(key).clone()
    if bias:
        y += torch.from_numpy(t["bias"].astype(np.float64))[None, :, None, None]
    if temb:
        y += torch.from_numpy((t["temb"] if temb_rows is None else temb_rows).astype(np.float64))[:, :, None, None]
    if res:
        y += torch.from_numpy(t["res"].astype(np.float64))
    return y.numpy()


# ------------------------------------------------------------------ coverage of the epilogue families
PASSED = []   # (plan, facts) of every launch whose result passed `close`


def bm_of(tile):
    return 128 if tile in (1, 2) else 64


COVERAGE = {
    "tile_epilogue, HoWo % BM == 0": lambda p, f: f["temb"] and p[0] in (1, 2, 3, 4) and not p[3] and f["howo"] % bm_of(p[0]) == 0,
    "tile_epilogue, HoWo % BM != 0": lambda p, f: f["temb"] and p[0] in (1, 2, 3, 4) and not p[3] and f["howo"] % bm_of(p[0]) != 0,
    "halo kernel (tile 7)": lambda p, f: f["temb"] and p[0] == 7 and not p[3],
    "splitk_reduce_kernel (slab, no twin)": lambda p, f: f["temb"] and p[3] == 1 and not f["twin"],
    "reduce_twin_kernel behind tile 9": lambda p, f: f["temb"] and p[0] == 9 and f["twin"],
    "reduce_twin_kernel behind another tile": lambda p, f: f["temb"] and p[0] not in (9, -1) and f["twin"],
    "direct kernels": lambda p, f: f["temb"] and p[0] == -1,
    "two sources on tiles 1-4": lambda p, f: f["c1"] and p[0] in (1, 2, 3, 4),
    "two sources on the halo kernel": lambda p, f: f["c1"] and p[0] == 7,
    "two sources on the weight stream": lambda p, f: f["c1"] and p[0] == 9,
    "encoder padding on tiles 1-4": lambda p, f: f["pad_mode"] and p[0] in (1, 2, 3, 4),
}


def run(key, what, bias=True, temb=False, res=False, tile=0, splitk=0, force_generic=False, twin=None, iters=1):
    """One sd_op_conv2d_ex launch of the case `key` against the fp64 reference.  Returns (out, twin output, plan)."""
    b, c0, c1, h, w, cout, k, stride, up, pad_mode = key
    t = inputs(*key)
    out, out_twin, plan, _ = _lib.conv2d_ex(t["x0"], t["w"], t["bias"] if bias else None, t["res"] if res else None, x1=t["x1"],
                                            temb=t["temb"] if temb else None, stride=stride, upsample=up, pad_mode=pad_mode, twin=twin,
                                            tile=tile, splitk=splitk, force_generic=force_generic, iters=iters)
    what = f"{what} {key} code {tile} splitk {splitk} generic {int(force_generic)} bias {int(bias)} temb {int(temb)} res {int(res)} -> plan {plan}"
    close(out, ref64(key, bias, temb, res), what)
    ho, wo = out_size(h, w, k, stride, up, pad_mode)
    PASSED.append((plan, {"temb": temb, "c1": c1, "pad_mode": pad_mode, "twin": twin is not None, "howo": ho * wo}))
    return out, out_twin, plan


def case(b, c0, c1, h, w, cout, k, stride=1, up=False, pad_mode=0):
    return (b, c0, c1, h, w, cout, k, stride, up, pad_mode)


def ident(v):
    return "x".join(str(int(e)) if isinstance(e, bool) else str(e) for e in v) if isinstance(v, tuple) else str(v)


# ------------------------------------------------------------------ A. time embedding through every epilogue
TILE_CODES = [1, 2, 3, 4] + [10 * s + t for s in range(1, 9) for t in range(1, 5)]   # those of test_conv2d_every_tile_and_splitk
A_SIZES = [(8, 8), (9, 11), (16, 16)]   # HoWo 64: BM 128 straddles two samples; 99: the boundary falls mid-tile and mid-quad; 256: uniform


@gpu
@pytest.mark.parametrize("hw", A_SIZES, ids=ident)
@pytest.mark.parametrize("k", [3, 1])
@pytest.mark.parametrize("tile", TILE_CODES)
def test_temb_on_every_tile_and_ring(tile, k, hw):
    key = case(3, 64, 0, hw[0], hw[1], 100, k)
    for splitk in (1, 2):
        _, _, plan = run(key, "temb, all terms", temb=True, res=True, tile=tile, splitk=splitk)
        assert plan[0] == tile % 10 and plan[1] == tile // 10, plan
        assert plan[2] == (splitk if k == 3 else 1) and plan[3] == int(plan[2] > 1), plan   # (64 channels of a 1x1: one K step, no split)
        _, _, plan = run(key, "temb alone", bias=False, temb=True, tile=tile, splitk=splitk)
        assert plan[0] == tile % 10, plan


HALO_CASES = [case(3, 64, 0, 8, 8, 96, 3), case(2, 128, 0, 9, 17, 68, 3), case(3, 64, 0, 8, 8, 64, 3, up=True)]


@gpu
@pytest.mark.parametrize("key", HALO_CASES, ids=ident)
@pytest.mark.parametrize("splitk", [1, 2, 3])
@pytest.mark.parametrize("tile", [7, 27, 37, 47])
def test_temb_on_the_halo_kernel(tile, splitk, key):
    chunks = key[1] // 64   # the halo kernel splits whole 64-channel chunks
    for terms in (dict(temb=True, res=True), dict(bias=False, temb=True)):
        _, _, plan = run(key, "halo temb", tile=tile, splitk=splitk, **terms)
        assert plan[0] == 7 and plan[1] == tile // 10 and plan[2] == min(splitk, chunks) and plan[3] == int(plan[2] > 1), plan


WS_CASES = [case(3, 128, 0, 8, 8, 320, 3), case(2, 64, 0, 16, 16, 320, 3), case(3, 64, 0, 8, 8, 320, 1)]


@gpu
@pytest.mark.parametrize("key", WS_CASES, ids=ident)
@pytest.mark.parametrize("tile", [9, 49], ids=["8waves", "4waves"])
def test_temb_behind_the_weight_stream(tile, key):
    for terms in (dict(temb=True, res=True), dict(bias=False, temb=True)):
        _, _, plan = run(key, "wstream temb", tile=tile, **terms)
        assert plan[0] == 9 and plan[3] == 1, plan


DIRECT_CASES = [case(3, 64, 0, 9, 11, 100, 3), case(3, 64, 0, 9, 11, 100, 1),   # conv_generic_kernel
                case(3, 4, 0, 16, 16, 64, 3),                                    # conv_small_cin_kernel (K = 36)
                case(3, 32, 0, 8, 8, 48, 3)]                                     # conv_generic_kernel off the MFMA shapes


@gpu
@pytest.mark.parametrize("key", DIRECT_CASES, ids=ident)
def test_temb_on_the_direct_kernels(key):
    for terms in (dict(temb=True, res=True), dict(bias=False, temb=True)):
        _, _, plan = run(key, "direct temb", force_generic=True, **terms)
        assert plan == [-1, -1, -1, -1], plan


@gpu
@pytest.mark.parametrize("tile,splitk", [(0, 0), (1, 1), (3, 2), (24, 1)])
def test_temb_on_a_stride_2_conv(tile, splitk):
    key = case(3, 64, 0, 9, 11, 100, 3, stride=2)   # 5x6 outputs per sample: every tile straddles samples
    for terms in (dict(temb=True, res=True), dict(bias=False, temb=True)):
        _, _, plan = run(key, "stride-2 temb", tile=tile, splitk=splitk, **terms)
        assert plan[0] in (1, 2, 3, 4), plan   # the im2col kernel


# ------------------------------------------------------------------ B. twin + temb (the low-res conv1 -> norm2 path)
TWIN_CASES = [case(3, 128, 0, 8, 8, 1280, 3), case(3, 64, 0, 16, 16, 640, 3), case(3, 64, 0, 4, 4, 256, 3)]   # the 3x3 rows of test_round5_gpu


def group_norm64(y, gw, gb, eps, silu):
    z = F.group_norm(torch.from_numpy(np.asarray(y, np.float64)), 32, torch.from_numpy(gw.astype(np.float64)),
                     torch.from_numpy(gb.astype(np.float64)), eps)
    return (F.silu(z) if silu else z).numpy()


@gpu
@pytest.mark.parametrize("key", TWIN_CASES, ids=ident)
@pytest.mark.parametrize("tile", [0, 9])
def test_twin_with_temb(tile, key):
    cout = key[5]
    rs = np.random.RandomState(cout + tile)
    gw = (1.0 + 0.2 * rs.randn(cout)).astype(np.float32)
    gb = (0.2 * rs.randn(cout)).astype(np.float32)
    eps, silu = 1e-5, True
    twin = (32, gw, gb, eps, silu)
    if tile == 9 and key[3] == 4:   # a 4x4 image is not the weight stream's 8- / 16-pixel-wide form
        with pytest.raises(ValueError):
            run(key, "twin + temb", temb=True, res=True, tile=tile, twin=twin)
        return
    conv_t, out_t, plan = run(key, "twin + temb", temb=True, res=True, tile=tile, twin=twin)
    assert plan[3] == 1 and (tile != 9 or plan[0] == 9), plan
    # against the GroupNorm of OUR conv output (isolates the twin from the conv's rounding) and against the launch it replaces
    close(out_t, group_norm64(conv_t, gw, gb, eps, silu), f"GroupNorm twin {key} tile {tile}")
    conv_b, _, _ = run(key, "no twin", temb=True, res=True)
    out_b, _ = _lib.groupnorm(conv_b, gw, gb, 32, eps, silu)
    close(out_t, out_b.astype(np.float64), f"twin vs GroupNorm launch {key} tile {tile}", min_psnr=58.0, rel=1e-2)
    ref_conv = ref64(key, True, True, True)
    close(out_t, group_norm64(h16(ref_conv), gw, gb, eps, silu), f"conv -> GroupNorm {key} tile {tile}", min_psnr=55.0, rel=1e-2)


@gpu
def test_twin_with_temb_is_bit_reproducible():
    key = TWIN_CASES[0]
    rs = np.random.RandomState(5)
    twin = (32, (1.0 + 0.2 * rs.randn(1280)).astype(np.float32), (0.2 * rs.randn(1280)).astype(np.float32), 1e-5, True)
    conv_a, out_a, _ = run(key, "twin + temb", temb=True, res=True, tile=9, twin=twin)
    conv_b, out_b, _ = run(key, "twin + temb, 3 launches", temb=True, res=True, tile=9, twin=twin, iters=3)
    assert np.array_equal(conv_a, conv_b) and np.array_equal(out_a, out_b)


@gpu
def test_twin_is_refused_where_the_combine_cannot_hold_it():
    key = case(1, 64, 0, 32, 32, 192, 3)   # 1024 pixels x 24 channels per (sample, group) slice: more than a workgroup keeps in registers
    g = np.ones(192, np.float32)
    with pytest.raises(ValueError):
        run(key, "twin", temb=True, twin=(8, g, g, 1e-5, True))
    with pytest.raises(ValueError):       # no twin behind the direct kernels
        run(case(1, 64, 0, 8, 8, 64, 3), "twin", temb=True, twin=(16, g, g, 1e-5, True), force_generic=True)


# ------------------------------------------------------------------ C. two sources
SOURCES = [(128, 64), (64, 192)]
C_CODES = [1, 2, 3, 4, 11, 22, 33, 44, 51, 62, 73, 84]   # tiles 1-4 and one code of every staging family


@gpu
@pytest.mark.parametrize("geom", [(3, 8, 8), (3, 9, 11), (1, 16, 16)], ids=ident)
@pytest.mark.parametrize("src", SOURCES, ids=ident)
@pytest.mark.parametrize("tile", C_CODES + [7, 37])
def test_two_sources_on_tiles_rings_and_halo(tile, src, geom):
    k, h, w = geom
    key = case(3, src[0], src[1], h, w, 100, k)
    for splitk in (1, 2):
        _, _, plan = run(key, "two sources", res=True, tile=tile, splitk=splitk)
        if tile % 10 == 7 and k == 1:
            assert plan[0] in (1, 2, 3, 4), plan   # no halo kernel for a 1x1: the planner's own tile
        else:
            assert plan[0] == tile % 10 and plan[1] == tile // 10, plan
        assert plan[2] == splitk and plan[3] == int(splitk > 1), plan


@gpu
@pytest.mark.parametrize("src", SOURCES + [(96, 32)], ids=ident)
@pytest.mark.parametrize("tile", [9, 49], ids=["8waves", "4waves"])
def test_two_sources_on_the_weight_stream(tile, src):
    key = case(3, src[0], src[1], 8, 8, 320, 3)
    _, _, plan = run(key, "two sources, wstream", res=True, tile=tile)
    if src == (96, 32):   # wstream_shape_ok admits 32-channel sources, conv_fast_path_ok (64-channel K steps) does not: the direct kernel
        assert plan[0] == -1, plan
    else:
        assert plan[0] == 9 and plan[3] == 1, plan


@gpu
@pytest.mark.parametrize("hw,tile", [(8, 0), (8, 9), (16, 0), (16, 37), (16, 3), (16, 23)])
def test_up_block_resnet_conv1(hw, tile):
    """Both sources + time embedding + residual, no upsample: conv1 of an up-block resnet."""
    key = case(3, 128, 64, hw, hw, 320, 3)
    for splitk in (0, 2) if tile % 10 != 9 else (0,):
        _, _, plan = run(key, "up-block conv1", temb=True, res=True, tile=tile, splitk=splitk)
        assert plan[0] == (tile % 10 if tile else (9 if hw == 8 and splitk == 0 else 7)), plan   # (the library's own plan at 8x8: wstream)


@gpu
def test_two_sources_on_the_direct_kernel():
    for k in (3, 1):
        _, _, plan = run(case(3, 32, 16, 9, 11, 100, k), "two sources, direct", temb=True, res=True, force_generic=True)
        assert plan[0] == -1, plan


# ------------------------------------------------------------------ D. encoder padding
PAD_CASES = [case(2, 128, 0, 16, 16, 128, 3, stride=2, pad_mode=1), case(1, 64, 0, 9, 11, 64, 3, stride=2, pad_mode=1),   # odd: 4x5 out
             case(2, 64, 0, 8, 8, 256, 3, stride=2, pad_mode=1)]


@gpu
@pytest.mark.parametrize("key", PAD_CASES, ids=ident)
@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4])
def test_encoder_padding(tile, key):
    for splitk in (1, 2) if tile else (0,):
        out, _, plan = run(key, "encoder padding", res=True, tile=tile, splitk=splitk)
        assert out.shape[2:] == out_size(key[3], key[4], 3, 2, False, 1)
        assert plan[0] in (1, 2, 3, 4) and (tile == 0 or (plan[0] == tile and plan[2] == splitk)), plan
    if tile == 0:
        _, _, plan = run(key, "encoder padding, direct", res=True, force_generic=True)
        assert plan[0] == -1, plan


@gpu
def test_encoder_padding_refusals():
    key = PAD_CASES[2]
    t = inputs(*key)
    with pytest.raises(ValueError):   # the weight stream has no explicit padding (and no stride 2)
        _lib.conv2d_ex(t["x0"], t["w"], t["bias"], stride=2, pad_mode=1, tile=9)
    with pytest.raises(ValueError):   # the (0,1,0,1) padding belongs to the stride-2 downsample
        _lib.conv2d_ex(t["x0"], t["w"], t["bias"], stride=1, pad_mode=1)
    with pytest.raises(ValueError):
        _lib.conv2d_ex(t["x0"], t["w"], t["bias"], stride=2, pad_mode=2)


# ------------------------------------------------------------------ coverage: asserted, not assumed
COVERAGE_CASES = {   # one representative per family, run here when the tests above were deselected
    "tile_epilogue, HoWo % BM == 0": lambda: run(case(3, 64, 0, 16, 16, 100, 3), "coverage", temb=True, tile=1, splitk=1),
    "tile_epilogue, HoWo % BM != 0": lambda: run(case(3, 64, 0, 9, 11, 100, 3), "coverage", temb=True, tile=1, splitk=1),
    "halo kernel (tile 7)": lambda: run(HALO_CASES[0], "coverage", temb=True, tile=7, splitk=1),
    "splitk_reduce_kernel (slab, no twin)": lambda: run(case(3, 64, 0, 9, 11, 100, 3), "coverage", temb=True, tile=3, splitk=2),
    "reduce_twin_kernel behind tile 9": lambda: test_twin_with_temb(9, TWIN_CASES[0]),
    "reduce_twin_kernel behind another tile": lambda: test_twin_with_temb(0, TWIN_CASES[1]),
    "direct kernels": lambda: run(DIRECT_CASES[0], "coverage", temb=True, force_generic=True),
    "two sources on tiles 1-4": lambda: run(case(3, 128, 64, 9, 11, 100, 3), "coverage", tile=3, splitk=1),
    "two sources on the halo kernel": lambda: run(case(3, 128, 64, 9, 11, 100, 3), "coverage", tile=7, splitk=1),
    "two sources on the weight stream": lambda: run(case(3, 128, 64, 8, 8, 320, 3), "coverage", tile=9),
    "encoder padding on tiles 1-4": lambda: run(PAD_CASES[0], "coverage", tile=3, splitk=1),
}


@gpu
def test_every_epilogue_family_was_reached_by_a_passing_case():
    """Over the plans the launches of this module REPORTED (not the codes they asked for).  Must stay the last GPU test of the file."""
    for name, hit in COVERAGE.items():
        if not any(hit(p, f) for p, f in PASSED):
            COVERAGE_CASES[name]()
        n = sum(1 for p, f in PASSED if hit(p, f))
        print(f"coverage: {name}: {n} passing launches")
        assert n >= 1, f"no passing launch reached: {name}"


# ------------------------------------------------------------------ the guard on the test itself (CPU)
def test_close_rejects_the_mutants():
    """torch only: for the inputs of one case per group, each wrong index this module is after lies far outside `close`, and the
    fp16-rounded reference itself lies inside."""
    def rejected(mutant, ref, what):
        with pytest.raises(AssertionError):
            close(mutant, ref, what)

    for key in (case(3, 64, 0, 9, 11, 100, 3), TWIN_CASES[2]):   # A, B: the time embedding
        t = inputs(*key)
        ref = ref64(key, True, True, True)
        close(h16(ref), ref, f"fp16-rounded reference {key}")
        rejected(ref64(key, True, True, True, temb_rows=np.roll(t["temb"], 1, axis=0)), ref, "temb rolled by one sample")
        cut = t["temb"].copy()
        cut[:, -4:] = 0.0
        rejected(ref64(key, True, True, True, temb_rows=cut), ref, "temb of the last 4 channels dropped")
    for src in SOURCES:   # C: the weight blocks of the two sources swapped
        key = case(3, src[0], src[1], 9, 11, 100, 3)
        t = inputs(*key)
        ref = ref64(key, True, False, True)
        close(h16(ref), ref, f"fp16-rounded reference {key}")
        swapped = np.concatenate([t["w"][:, src[0]:], t["w"][:, :src[0]]], axis=1)
        mutant = conv_ref64(t, w=swapped).numpy() + (ref - _conv_ref64_cached(key).numpy())
        rejected(mutant, ref, "weight blocks of x0 and x1 swapped")
    for key in (PAD_CASES[0], PAD_CASES[2]):   # D: symmetric padding 1 (the same output size at even images)
        t = inputs(*key)
        ref = ref64(key, True, False, True)
        close(h16(ref), ref, f"fp16-rounded reference {key}")
        mutant = conv_ref64(t, symmetric_pad=True).numpy() + (ref - _conv_ref64_cached(key).numpy())
        rejected(mutant, ref, "padding 1 on every side")
