"""CPU suite of the palettized small-M 1x1 GEMM (plan tile 15): the index bit stream against a numpy restatement of the layout the
header describes, the refusals of the operator entry (all made on the host, in front of any device work), and the planner's answers
for the fp16 descriptors of the shapes the GPU suite uses."""
import numpy as np
import pytest

from python_hip_stable_diffusion import _lib

NBITS = (1, 2, 4, 6, 8)
GROUP = 8            # K64 stages per group of the stream


def pack_reference(idx, nbits):
    """include/sd_mi355x.h, sd_op_palette_pack_gemm: lane l = 16 g + r16 of strip n / 16 owns, per stage s and sub-step kk, the indices
    of W[16 strip + r16][64 s + 32 kk + 8 g + e]; its 128 indices of a group of 8 stages in the order (s, kk, e) are little-endian
    nbits-wide fields in nbits 16-byte words; word q at [strip][group][q][lane][16 B]; stages beyond K / 64 are zero fields."""
    n, k = idx.shape
    groups = -(-(k // 64) // GROUP)
    padded = np.zeros((n, groups * GROUP * 64), np.uint8)
    padded[:, :k] = idx
    lane = np.arange(64)
    f = np.arange(GROUP * 16)
    s, kk, e = f >> 4, (f >> 3) & 1, f & 7
    col = (64 * s + 32 * kk + e)[None, :] + 8 * (lane >> 4)[:, None]                 # [lane][field] inside a group
    row = lane & 15
    fields = np.empty((n // 16, groups, 64, GROUP * 16), np.uint8)
    for strip in range(n // 16):
        for grp in range(groups):
            fields[strip, grp] = padded[(16 * strip + row)[:, None], grp * GROUP * 64 + col]
    bits = (fields[..., None] >> np.arange(nbits, dtype=np.uint8)) & 1               # little-endian inside a field
    by = np.packbits(bits.reshape(n // 16, groups, 64, GROUP * 16 * nbits), axis=-1, bitorder="little")
    return by.reshape(n // 16, groups, 64, nbits, 16).transpose(0, 1, 3, 2, 4)


def unpack(stream, n, k, nbits):
    """the inverse, written on its own: (indices the stream holds, the padding fields)"""
    strips, groups = stream.shape[:2]
    by = stream.transpose(0, 1, 3, 2, 4).reshape(strips, groups, 64, nbits * 16)
    bits = np.unpackbits(by, axis=-1, bitorder="little").reshape(strips, groups, 64, GROUP * 16, nbits)
    fields = (bits.astype(np.uint32) << np.arange(nbits, dtype=np.uint32)).sum(-1)
    out = np.full((n, groups * GROUP * 64), 255, np.uint32)
    for strip in range(strips):
        for grp in range(groups):
            for lane in range(64):
                for st in range(GROUP):
                    for kk in range(2):
                        c0 = grp * GROUP * 64 + 64 * st + 32 * kk + 8 * (lane >> 4)
                        out[16 * strip + (lane & 15), c0:c0 + 8] = fields[strip, grp, lane, (2 * st + kk) * 8:(2 * st + kk) * 8 + 8]
    return out[:, :k], out[:, k:]


@pytest.mark.parametrize("nbits", NBITS)
@pytest.mark.parametrize("cout,k", [(16 * 2, 64), (80, 576), (160, 704), (80, 1280)])
def test_palette_pack_gemm_against_the_documented_layout(cout, k, nbits):
    rs = np.random.RandomState(cout + k + nbits)
    idx = rs.randint(0, 1 << nbits, size=(cout, k)).astype(np.uint8)
    idx[0, 0], idx[-1, -1] = (1 << nbits) - 1, (1 << nbits) - 1                     # both ends of the tensor carry all-ones fields
    got = _lib.palette_pack_gemm(idx, nbits)
    groups = -(-(k // 64) // GROUP)
    assert got.shape == (cout // 16, groups, nbits, 64, 16) and got.dtype == np.uint8
    assert got.size == (cout // 16) * groups * nbits * 1024                         # the size formula
    want = pack_reference(idx, nbits)
    assert np.array_equal(got, want), f"{np.count_nonzero(got != want)} bytes differ"
    back, padding = unpack(got, cout, k, nbits)
    assert np.array_equal(back, idx)
    assert padding.size == cout * (groups * GROUP * 64 - k) and not padding.any()


def test_palette_pack_gemm_refusals():
    ok = np.zeros((32, 64), np.uint8)
    for bad_shape in ((24, 64), (32, 96)):
        with pytest.raises(ValueError):
            _lib.palette_pack_gemm(np.zeros(bad_shape, np.uint8), 4)
    with pytest.raises(ValueError):
        _lib.palette_pack_gemm(ok, 3)
    with pytest.raises(ValueError):
        _lib.palette_pack_gemm(np.zeros((32, 64, 1, 1), np.uint8), 4)


def _problem(B=1, Cin=64, H=8, W=8, Cout=320, nbits=4):
    rs = np.random.RandomState(5)
    lut = rs.randn(1 << nbits).astype(np.float16)
    idx = rs.randint(0, 1 << nbits, size=(Cout, Cin)).astype(np.uint8)
    x = rs.randn(B, Cin, H, W).astype(np.float16)
    return x, lut, idx


def test_refusals_need_no_gpu():
    """Validation precedes device work: every one of these is a ValueError on a box without a GPU (where a valid call is a
    RuntimeError: no HIP device)."""
    x, lut, idx = _problem()
    with pytest.raises(ValueError, match="nbits"):
        _lib.gemm_palettized(x, lut[:8], idx % 8, 3)
    with pytest.raises(ValueError, match="bm"):
        _lib.gemm_palettized(x, lut, idx, 4, bm=48)
    bad = idx.copy()
    bad[7, 9] = 16
    with pytest.raises(ValueError, match="index 16"):
        _lib.gemm_palettized(x, lut, bad, 4)
    with pytest.raises(ValueError):                                                 # N = 96: not a multiple of the 80-column tile
        _lib.gemm_palettized(*_problem(Cout=96), 4)
    with pytest.raises(ValueError):                                                 # M = 72: ragged
        _lib.gemm_palettized(*_problem(H=8, W=9), 4)
    with pytest.raises(ValueError):                                                 # Cin = 32: off the MFMA path
        _lib.gemm_palettized(*_problem(Cin=32), 4)
    with pytest.raises(ValueError):                                                 # 3 x 4 = 12 tiles: not a multiple of 8
        _lib.gemm_palettized(*_problem(H=8, W=12), 4)
    with pytest.raises(ValueError):                                                 # the same M with 64-row tiles: one row of tiles
        _lib.gemm_palettized(x, lut, idx, 4, bm=64)
    # the order of the checks: nbits before bm before the index range before the shape
    with pytest.raises(ValueError, match="nbits"):
        _lib.gemm_palettized(x, lut[:8], idx % 8, 3, bm=48)
    with pytest.raises(ValueError, match="bm"):
        _lib.gemm_palettized(*_problem(Cout=96)[:2], bad[:96], 4, bm=48)
    with pytest.raises(ValueError, match="index 16"):
        _lib.gemm_palettized(*_problem(Cout=96)[:2], bad[:96], 4)


# (B, H, W, Cin, Cout, flags: 16 bias, 4 residual) -> plan tile of the fp16 descriptor
FP16_PLANS = [
    ((4, 16, 16, 640, 640, 16), 12),          # the handle test's projections: proj_in (bias)
    ((4, 16, 16, 640, 640, 16 | 4), 12),      # ... and to_out.0 (bias + residual)
    ((2, 16, 16, 1280, 1280, 16 | 4), 12),    # SD2.1-base at CFG batch 2
    ((2, 32, 32, 640, 640, 16 | 4), 12),
]


@pytest.mark.parametrize("desc,tile", FP16_PLANS)
def test_fp16_plans_are_unchanged_and_tile_15_takes_what_tile_12_takes(desc, tile):
    """A palette never changes a plan of a handle without palettes: the planner's answers for the fp16 descriptors stay what they
    were, no answer is ever tile 14 / 15, and the shapes it sends to tile 12 pass the host validation of the palettized entry (on a
    box without a GPU the call then stops at the device: RuntimeError, not ValueError)."""
    B, H, W, cin, cout, flags = desc
    p = _lib.conv_plan(1, 1, 1, cin, 0, cout, B, H, W, flags=flags)
    assert p["tile"] == tile and p["splitk"] == 1 and not p["slab"] and p["workspace_bytes"] == 0, p
    assert _lib.conv_plan(1, 1, 1, cin, 0, cout, B, H, W, flags=flags | 8)["tile"] not in (12, 14, 15)   # GroupNorm statistics asked
    x, lut, idx = _problem(B=B, Cin=cin, H=H, W=W, Cout=cout)
    try:
        out, plan, _ = _lib.gemm_palettized(x, lut, idx, 4)
    except RuntimeError:
        return
    assert plan == [15, 1 if B * H * W <= 1024 else 2, 1, 0]
