"""smgeglu.hip (plan tile 13): the GEGLU projections of the 640- / 1280-channel levels in one chip-filling round, through the C ABI
against fp32 torch (LayerNorm -> Linear -> v * gelu(g), erf form): both shapes of the SD2.1-base step with the LayerNorm fold and
without, with and without bias, both tile heights, a ring tail and the smallest K per tile height, the tiled kernel it replaces,
bit-reproducibility, and the shapes it refuses.
Tolerances as tests/test_ops_gpu.py and tests/test_smgemm_gpu.py: PSNR >= 60 dB, max |err| <= 4e-3 * max|ref| + 1e-3 (fp16 I/O,
fp32 accumulate)."""
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
    print(f"{what}: PSNR {p:.1f} dB, max|err| {err:.3e} (bound {bound:.3e})")
    assert p >= min_psnr and err <= bound, f"{what}: PSNR {p:.1f} dB, max|err| {err:.3e} (bound {bound:.3e})"


def geglu_ln_ref(x, w, bias, ln_w, ln_b, eps=1e-5):
    xt = torch.from_numpy(x.astype(np.float32))
    if ln_w is not None:
        xt = F.layer_norm(xt, (xt.shape[1],), torch.from_numpy(ln_w), torch.from_numpy(ln_b), eps)   # unet.py:583-591 norm3
    h = xt @ torch.from_numpy(w.astype(np.float32)).T
    if bias is not None:
        h = h + torch.from_numpy(bias)
    val, gate = h.chunk(2, dim=1)                                                                   # unet.py:616-617
    return (val * F.gelu(gate)).numpy()


def make_case(shape, seed, ln=True, with_bias=True):
    m, c, n2 = shape
    rs = np.random.RandomState(seed)
    # rows of different scale around a non-zero mean: the fold's statistics and its ln_b * colsum term matter
    x = h16(rs.randn(m, c) * (1.0 + rs.rand(m, 1)) + 0.5 + 0.5 * rs.rand(m, 1))
    w = h16(rs.randn(n2, c) / np.sqrt(c))
    bias = (0.1 * rs.randn(n2)).astype(np.float32) if with_bias else None
    ln_w = (1.0 + 0.2 * rs.randn(c)).astype(np.float32) if ln else None
    ln_b = (0.1 * rs.randn(c)).astype(np.float32) if ln else None
    return x, w, bias, ln_w, ln_b


STEP_SHAPES = [  # (M, K, N2) at CFG batch 2
    (512, 1280, 10240),   # ff.net.0.proj of the 16x16 level: 4 x 64 tiles of 128 rows, 20 K stages
    (2048, 640, 5120),    # ff.net.0.proj of the 32x32 level: 8 x 32 tiles of 256 rows, 10 K stages (3-stage ring: a tail)
]
TAIL_SHAPES = [
    (512, 832, 1280),     # 13 K stages: not a multiple of either ring depth (4 at 128 rows, 3 at 256 rows)
    (512, 64, 1280),      # the smallest K: one stage, fewer than the ring's prologue issues
]
ids3 = lambda s: "x".join(map(str, s))


@pytest.mark.parametrize("shape", STEP_SHAPES, ids=ids3)
@pytest.mark.parametrize("kernel", [100, 101, 102], ids=["auto", "bm128", "bm256"])
@pytest.mark.parametrize("ln", [True, False], ids=["ln-fold", "plain"])
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
def test_smgeglu_matches_torch(shape, kernel, ln, with_bias):
    x, w, bias, ln_w, ln_b = make_case(shape, sum(shape) + kernel, ln, with_bias)
    out, _ = _lib.geglu_ln(x, w, bias, ln_w, ln_b, kernel=kernel)
    close(out, geglu_ln_ref(x, w, bias, ln_w, ln_b), f"smgeglu {shape} kernel {kernel} ln={ln} bias={with_bias}")


@pytest.mark.parametrize("shape", TAIL_SHAPES, ids=ids3)
@pytest.mark.parametrize("kernel", [101, 102], ids=["bm128", "bm256"])
@pytest.mark.parametrize("ln", [True, False], ids=["ln-fold", "plain"])
def test_smgeglu_ring_tail_and_smallest_k(shape, kernel, ln):
    x, w, bias, ln_w, ln_b = make_case(shape, sum(shape) + kernel, ln)
    out, _ = _lib.geglu_ln(x, w, bias, ln_w, ln_b, kernel=kernel)
    close(out, geglu_ln_ref(x, w, bias, ln_w, ln_b), f"smgeglu {shape} kernel {kernel} ln={ln}")


@pytest.mark.parametrize("shape", STEP_SHAPES, ids=ids3)
@pytest.mark.parametrize("ln", [True, False], ids=["ln-fold", "plain"])
def test_smgeglu_bit_reproducible_and_matches_the_tiled_kernel(shape, ln):
    x, w, bias, ln_w, ln_b = make_case(shape, 11, ln)
    a, _ = _lib.geglu_ln(x, w, bias, ln_w, ln_b, kernel=100)
    b, _ = _lib.geglu_ln(x, w, bias, ln_w, ln_b, kernel=100)
    assert np.array_equal(a.view(np.uint16), b.view(np.uint16))
    t, _ = _lib.geglu_ln(x, w, bias, ln_w, ln_b, kernel=1)   # igemm_kernel 64 x 128: the plan these shapes had
    close(a, t.astype(np.float32), f"smgeglu vs igemm {shape} ln={ln}")
    d, _ = _lib.geglu_ln(x, w, bias, ln_w, ln_b, kernel=0)
    assert np.array_equal(d.view(np.uint16), a.view(np.uint16)), "the library's own plan for this shape is plan tile 13"


@pytest.mark.parametrize("shape,kernel", [((512, 1280, 1024), 100), ((500, 1280, 10240), 100), ((512, 1312, 10240), 100), ((384, 1280, 10240), 102)],
                         ids=["n_not_160", "ragged_m", "k_not_64", "m_not_256"])
def test_smgeglu_refuses_other_shapes(shape, kernel):
    m, c, n2 = shape
    rs = np.random.RandomState(3)
    x = h16(rs.randn(m, c))
    w = h16(rs.randn(n2, c) / np.sqrt(c))
    with pytest.raises(ValueError):
        _lib.geglu_ln(x, w, None, None, None, kernel=kernel)
