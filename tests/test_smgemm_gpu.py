"""smgemm.hip (plan tile 12): small-M single-source 1x1 GEMMs of the 640- / 1280-channel levels through the C ABI against fp32
torch: every shape the kernel takes in the SD2.1-base step (and the M = 128 shapes of the 8x8 level, forced), with and without
residual, both tile heights, bias absent, bit-reproducibility, the tiled kernel it replaces, and the shapes it refuses.
Tolerances as tests/test_ops_gpu.py: PSNR >= 60 dB, max |err| <= 4e-3 * max|ref| + 1e-3 (fp16 I/O, fp32 accumulate)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

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
    assert p >= min_psnr and err <= bound, f"{what}: PSNR {p:.1f} dB, max|err| {err:.3e} (bound {bound:.3e})"


def conv1x1_ref(x, w, bias, res):
    y = F.conv2d(torch.from_numpy(x.astype(np.float32)), torch.from_numpy(w.astype(np.float32)), None if bias is None else torch.from_numpy(bias))
    if res is not None:
        y = y + torch.from_numpy(res.astype(np.float32))
    return y.numpy()


def make(case, seed, with_res, with_bias=True):
    b, cin, hh, ww, cout = case
    rs = np.random.RandomState(seed)
    x = h16(rs.randn(b, cin, hh, ww))
    w = h16(rs.randn(cout, cin, 1, 1) / np.sqrt(cin))
    bias = (0.1 * rs.randn(cout)).astype(np.float32) if with_bias else None
    res = h16(rs.randn(b, cout, hh, ww)) if with_res else None
    return x, w, bias, res


SM_CASES = [  # (B, Cin, H, W, Cout) at CFG batch 2
    (2, 1280, 16, 16, 1280),   # proj_in / to_out / proj_out of the 16x16 level: M = 512, 20 K stages (10-stage ring, tail)
    (2, 2560, 16, 16, 1280),   # M = 512, 40 K stages
    (2, 5120, 16, 16, 1280),   # ff.net.2 of the 16x16 level: 80 K stages
    (2, 640, 32, 32, 640),     # proj_in / to_out / proj_out of the 32x32 level: M = 2048, 10 K stages (8-stage ring)
    (2, 2560, 32, 32, 640),    # ff.net.2 of the 32x32 level
    (2, 1280, 8, 8, 1280),     # the 8x8 level (M = 128), forced: 64 workgroups
    (2, 2560, 8, 8, 1280),
    (2, 5120, 8, 8, 1280),
]


@pytest.mark.parametrize("case", SM_CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("tile", [140, 141, 142], ids=["auto", "bm32", "bm64"])
@pytest.mark.parametrize("with_res", [True, False], ids=["res", "nores"])
def test_smgemm_matches_torch(case, tile, with_res):
    x, w, bias, res = make(case, sum(case) + tile, with_res)
    out, _ = _lib.conv2d(x, w, bias, res, tile=tile)
    close(out, conv1x1_ref(x, w, bias, res), f"smgemm {case} tile {tile} res={with_res}")


def test_smgemm_without_bias():
    case = (2, 1280, 16, 16, 1280)
    x, w, _, res = make(case, 5, True, with_bias=False)
    out, _ = _lib.conv2d(x, w, None, res, tile=140)
    close(out, conv1x1_ref(x, w, None, res), "smgemm without bias")


@pytest.mark.parametrize("case", SM_CASES[:5], ids=lambda c: "x".join(map(str, c)))
def test_smgemm_bit_reproducible_and_matches_the_tiled_kernel(case):
    x, w, bias, res = make(case, 11, True)
    a, _ = _lib.conv2d(x, w, bias, res, tile=140)
    b, _ = _lib.conv2d(x, w, bias, res, tile=140)
    assert np.array_equal(a.view(np.uint16), b.view(np.uint16))
    t, _ = _lib.conv2d(x, w, bias, res, tile=33)   # igemm_kernel 64 x 64, 4-stage ring: the plan these shapes had
    close(a, t.astype(np.float32), f"smgemm vs igemm {case}", min_psnr=60.0)


@pytest.mark.parametrize("case", [(2, 1280, 16, 16, 1000), (2, 1280, 3, 5, 1280), (2, 1280, 16, 16, 1280)],
                         ids=["n_not_80", "ragged_m", "3x3"])
def test_smgemm_refuses_other_shapes(case):
    b, cin, hh, ww, cout = case
    rs = np.random.RandomState(3)
    x = h16(rs.randn(b, cin, hh, ww))
    k = 3 if case == (2, 1280, 16, 16, 1280) else 1
    w = h16(rs.randn(cout, cin, k, k) / np.sqrt(cin * k * k))
    with pytest.raises(ValueError):
        _lib.conv2d(x, w, None, None, tile=140)
