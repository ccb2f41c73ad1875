"""The merged tail of a SpatialTransformer: ff.net.2 + residual -> proj_out + residual as ONE GEMM over [g | h2] with the folded
weights [Wp W2 | Wp] and bias Wp b2 + bp (wfold.hip, the two-source form of smgemm.hip, igemm.hip's two-source split-K), through the
C ABI.  Reference: the two-step formula in fp64 from the fp16 inputs, no intermediate rounding.  Tolerances as
tests/test_smgemm_gpu.py: PSNR >= 60 dB, max |err| <= 4e-3 * max|ref| + 1e-3 (fp16 I/O, fp32 accumulate).

Shapes: the smallest that cross the source switch inside a running ring and wrap it (C = 320: 20 + 5 K stages against the 10-stage
ring of the 32-row tile; C = 640: 40 + 10 stages on both tile heights, the 64-row tile's ring being 8 deep), a split-K boundary on the
source boundary (C = 640 / 1280 on the tiled kernels), the step's own 8x8 shape (C = 1280: 80 + 20 stages) and a ragged M that only
the tiled kernels take."""
import functools

import numpy as np
import pytest

from oracle import psnr
from python_hip_stable_diffusion import _lib

pytestmark = pytest.mark.gpu


def h16(a):
    return np.asarray(a, np.float32).astype(np.float16)


def close(got, ref, what, min_psnr=60.0, rel=4e-3):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    p = psnr.compute_psnr(got, ref)
    err = np.abs(got - ref).max()
    bound = rel * np.abs(ref).max() + 1e-3
    print(f"{what}: PSNR {p:.1f} dB, max|err| {err:.3e} (bound {bound:.3e})")
    assert p >= min_psnr and err <= bound, f"{what}: PSNR {p:.1f} dB, max|err| {err:.3e} (bound {bound:.3e})"


# ---------------------------------------------------------------- the fold kernel on its own
FOLD_SHAPES = [(64, 64, 256), (80, 144, 208), (320, 320, 1280)]   # (N, J, K): whole tiles, ragged in all three, more than one tile


@pytest.mark.parametrize("shape", FOLD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fold_kernel_matches_fp64(shape):
    n, j, k = shape
    rs = np.random.RandomState(n + j + k)
    wp = h16(rs.randn(n, j) / np.sqrt(j))
    w2 = h16(rs.randn(j, k) / np.sqrt(k))
    bp = (0.1 * rs.randn(n)).astype(np.float32)
    b2 = (0.1 * rs.randn(j)).astype(np.float32)
    wm, bm = _lib.fold_linear(wp, bp, w2, b2)
    ref = (wp.astype(np.float64) @ w2.astype(np.float64)).astype(np.float16)
    # fp16 bit patterns one apart are neighbours of the same sign (0x0000 / 0x8000 are 32768 apart)
    d = np.abs(wm.view(np.uint16).astype(np.int32) - ref.view(np.uint16).astype(np.int32))
    frac = float((d != 0).mean())
    print(f"fold {shape}: max ulp distance {d.max()}, {100 * frac:.3f} % of elements differ")
    assert d.max() <= 1, f"fold {shape}: {d.max()} ulp"
    assert frac <= 0.005, f"fold {shape}: {100 * frac:.3f} % of elements differ from the rounded fp64 product"
    bref = bp.astype(np.float64) + wp.astype(np.float64) @ b2.astype(np.float64)
    berr = np.abs(bm.astype(np.float64) - bref) / np.abs(bref)
    print(f"fold {shape}: bias max relative error {berr.max():.3e}")
    assert berr.max() <= 1e-6, f"fold {shape}: bias relative error {berr.max():.3e}"
    wm2, bm2 = _lib.fold_linear(wp, bp, w2, b2)
    assert np.array_equal(wm.view(np.uint16), wm2.view(np.uint16)) and np.array_equal(bm.view(np.uint32), bm2.view(np.uint32))


# ---------------------------------------------------------------- the merged tail
TAIL_CASES = {  # (B, C, S): the fused codes that take the shape
    (2, 320, 64): (2, 3, 4),
    (2, 640, 64): (2, 3, 4, 5),
    (2, 1280, 64): (2, 3, 4),      # the step's own 8x8 shape
    (1, 320, 40): (2, 3),          # ragged M = 40
}


@functools.lru_cache(maxsize=None)
def tail_inputs(case, wscale=1.0):
    """inputs and the fp64 two-step reference of one case, computed once and shared (read-only) by the tests"""
    b, c, s_ = case
    rs = np.random.RandomState(7 * c + s_ + b)
    g = h16(rs.randn(b, 4 * c, 1, s_))
    w1 = h16(wscale * rs.randn(c, 4 * c) / np.sqrt(4 * c))
    b1 = (0.1 * rs.randn(c)).astype(np.float32)
    res1 = h16(rs.randn(b, c, 1, s_))
    w2 = h16(wscale * rs.randn(c, c) / np.sqrt(c))
    b2 = (0.1 * rs.randn(c)).astype(np.float32)
    res2 = h16(rs.randn(b, c, 1, s_))
    f = lambda a: np.asarray(a, np.float64)
    h3 = f(res1)[:, :, 0, :] + np.einsum("nk,bks->bns", f(w1), f(g)[:, :, 0, :]) + f(b1)[None, :, None]
    ref = f(res2)[:, :, 0, :] + np.einsum("nk,bks->bns", f(w2), h3) + f(b2)[None, :, None]
    args = (g, w1, b1, res1, w2, b2, res2)
    for a in args:
        a.setflags(write=False)
    ref = ref[:, :, None, :]
    ref.setflags(write=False)
    return args, ref


def gn_want(out, groups):
    b, c, _, s_ = out.shape
    o = out.astype(np.float64).reshape(b, groups, c // groups, s_)
    return np.stack([o.sum(axis=(2, 3)), (o ** 2).sum(axis=(2, 3))], axis=-1)


def gn_ok(sums, out, groups=32):   # the bound tests/test_round5_gpu.py asks of the one-launch tail's statistics
    want = gn_want(out, groups)
    return np.isfinite(sums).all() and np.abs(sums - want).max() <= 2e-4 * np.abs(want).max() + 1e-3


@pytest.mark.parametrize("case,fused", [(c, f) for c, codes in TAIL_CASES.items() for f in codes],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"fused{v}")
def test_merged_tail_matches_fp64(case, fused):
    args, ref = tail_inputs(case)
    out, _, _ = _lib.ffn_out_proj(*args, fused=fused)
    close(out, ref, f"merged tail {case} fused={fused}")


@pytest.mark.parametrize("fused", [4, 5])
def test_smgemm_refuses_the_ragged_tail(fused):
    args, _ = tail_inputs((1, 320, 40))
    with pytest.raises(ValueError):
        _lib.ffn_out_proj(*args, fused=fused)


# which form leaves the consumer GroupNorm's statistics at each shape: (two launches, merged).  A launch leaves them only from an
# unsplit K loop over whole 64-row tiles of one sample: (2, 320, 64) neither form splits K (5 / 25 K steps); (2, 640, 64) proj_out's 10
# steps run unsplit, the merged 50 steps are split in two; (2, 1280, 64) both run their split-K plans of the 8x8 level; S = 40 is ragged
GN_STATS_LEFT = {(2, 320, 64): (True, True), (2, 640, 64): (True, False), (2, 1280, 64): (False, False), (1, 320, 40): (False, False)}


@pytest.mark.parametrize("case", list(TAIL_CASES), ids=lambda c: "x".join(map(str, c)))
def test_merged_against_two_launches(case):
    """fused=2 against fused=0 on the same inputs (the CPU emulation of both roundings puts them 81-82 dB apart), and the GroupNorm
    statistics either form leaves for its consumer: where a form leaves them (GN_STATS_LEFT) they match the sums of its own fp16 output
    within the bound of tests/test_round5_gpu.py; where it leaves none it reports NaN everywhere (sd_mi355x.h) and the consumer runs its
    own statistics pass - a form that silently stops leaving them, or starts to, fails here."""
    args, _ = tail_inputs(case)
    two, sums_two, _ = _lib.ffn_out_proj(*args, groups=32, fused=0)
    one, sums_one, _ = _lib.ffn_out_proj(*args, groups=32, fused=2)
    close(one, two.astype(np.float32), f"merged vs two launches {case}")
    for what, sums, out, left in zip(("two launches", "merged"), (sums_two, sums_one), (two, one), GN_STATS_LEFT[case]):
        if left:
            assert gn_ok(sums, out), f"GroupNorm statistics, {what} {case}"
        else:
            assert np.isnan(sums).all(), f"GroupNorm statistics, {what} {case}: expected none"


def test_merged_tail_with_small_weights():
    """Both weight matrices scaled by 0.1: about a quarter of the folded matrix is fp16-subnormal.  Emulated on the CPU the merged tail
    gives 87 dB with subnormals honoured and 57.7 dB with them flushed to zero, so the 60 dB gate says what the conversion and the
    MFMA do with them."""
    case = (2, 640, 64)
    args, ref = tail_inputs(case, 0.1)
    wm, _ = _lib.fold_linear(args[4], args[5], args[1], args[2])
    a = np.abs(wm.astype(np.float32))
    print(f"small weights: {100 * float(((a > 0) & (a < 2.0 ** -14)).mean()):.1f} % of the folded matrix is subnormal")
    for fused in TAIL_CASES[case]:
        out, _, _ = _lib.ffn_out_proj(*args, fused=fused)
        close(out, ref, f"merged tail, weights x 0.1, fused={fused}")


@pytest.mark.parametrize("case", list(TAIL_CASES), ids=lambda c: "x".join(map(str, c)))
def test_merged_tail_bit_reproducible(case):
    args, _ = tail_inputs(case)
    a, _, _ = _lib.ffn_out_proj(*args, fused=2)
    b, _, _ = _lib.ffn_out_proj(*args, fused=2, iters=3)
    assert np.array_equal(a.view(np.uint16), b.view(np.uint16))
