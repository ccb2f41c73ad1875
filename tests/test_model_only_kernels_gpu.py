"""Operator tests of the kernels that otherwise run only inside whole models, each through its own sd_op_* entry point:
vae_f32.hip (conv_f32, groupnorm_f32, row_softmax_f32, the fp32 layout kernels), norm.hip row_softmax, misc.hip (gemv, the layout
and conversion kernels, add_half / sum_half), clip.hip (attention, embed, act) and vit.hip (patch rows, tokens).

References are float64 on the inputs as they cross the ABI; the comparators and their bounds are in model_only_ref.py, derived
from the number formats and operation counts, and test_model_only_kernels.py (CPU) shows that each rejects the defects these
cases are after.  The copy, conversion and fp16-sum kernels are compared bit for bit: numpy's float32 arithmetic and its casts
round to nearest even exactly like the kernels' single operations.  The library keeps every device output in front of a guard of
NaN patterns, and poisons the output itself: an element a launch skipped reads back as NaN, a write behind the end fails the call."""
import numpy as np
import pytest

import model_only_ref as R
from python_hip_stable_diffusion import _lib

pytestmark = pytest.mark.gpu

HALF_GRID = 2048 * 256          # threads of the fp16 copy kernels' largest grid
F32_GRID = 65535 * 256          # ... of the fp32 copy kernels'


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16 if a.dtype == np.float16 else np.uint32)


def same_bits(got, ref, what):
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, got.shape, ref.dtype, ref.shape)
    assert np.array_equal(bits(got), bits(ref)), f"{what}: {int((bits(got) != bits(ref)).sum())} of {ref.size} elements differ"


# ------------------------------------------------------------------------------------------------ bit-exact kernels
LAYOUT_SHAPES = [(2, 3, 5, 7), (1, 4, 8, 8), (3, 320, 1, 2)]


def ramp(shape, dtype, seed):
    """Distinct-looking values that are exact in fp16, so that every conversion in the chain is exact and a misplaced element shows."""
    rs = np.random.RandomState(seed)
    return (rs.randint(-2048, 2048, size=shape) / 8.0).astype(dtype)


@pytest.mark.parametrize("shape", LAYOUT_SHAPES + [(1, 4, 363, 363)])   # the last: past the fp16 kernels' grid of 2048 x 256 threads
def test_layout_kernels_to_and_from_half(shape):
    assert (np.prod(shape) > HALF_GRID) == (shape == (1, 4, 363, 363))
    for src_dt in (np.float16, np.float32):
        x = ramp(shape, src_dt, 1)
        same_bits(_lib.layout("nchw_to_nhwc", x, np.float16), np.ascontiguousarray(x.transpose(0, 2, 3, 1)).astype(np.float16),
                  f"nchw_to_nhwc {src_dt.__name__} -> fp16 {shape}")
    x = ramp(shape, np.float32, 2) + np.float32(2.0 ** -13)      # not fp16-representable: the cast rounds
    same_bits(_lib.layout("nchw_to_nhwc", x, np.float16), np.ascontiguousarray(x.transpose(0, 2, 3, 1)).astype(np.float16),
              f"nchw_to_nhwc fp32 -> fp16 (rounding) {shape}")
    B, C, H, W = shape
    t = ramp((B, H, W, C), np.float16, 3)
    same_bits(_lib.layout("nhwc_to_nchw", t, np.float32), np.ascontiguousarray(t.transpose(0, 3, 1, 2)).astype(np.float32),
              f"nhwc_to_nchw fp16 -> fp32 {shape}")


@pytest.mark.parametrize("shape", LAYOUT_SHAPES)
def test_layout_kernels_fp32(shape):
    for src_dt in (np.float16, np.float32):
        x = ramp(shape, src_dt, 4) if src_dt == np.float16 else np.random.RandomState(5).randn(*shape).astype(np.float32)
        same_bits(_lib.layout("nchw_to_nhwc", x, np.float32), np.ascontiguousarray(x.transpose(0, 2, 3, 1)).astype(np.float32),
                  f"nchw_to_nhwc {src_dt.__name__} -> fp32 {shape}")
    B, C, H, W = shape
    t = np.random.RandomState(6).randn(B, H, W, C).astype(np.float32)
    same_bits(_lib.layout("nhwc_to_nchw", t, np.float32), np.ascontiguousarray(t.transpose(0, 3, 1, 2)), f"nhwc_to_nchw fp32 {shape}")


def test_layout_kernels_fp32_past_their_grid():
    """More elements than the 65535 x 256 threads of the fp32 copy kernels' largest grid: the grid-stride loop takes a second trip.
    The values repeat with a period co-prime to every dimension, so a misplaced element differs from its neighbours."""
    shape = (1, 3, 2365, 2365)
    n = int(np.prod(shape))
    assert n > F32_GRID
    x = (np.arange(n, dtype=np.int64) % 2039 - 1000).astype(np.float16).reshape(shape)
    ref = np.ascontiguousarray(x.transpose(0, 2, 3, 1)).astype(np.float32)
    same_bits(_lib.layout("nchw_to_nhwc", x, np.float32), ref, "nchw_to_nhwc fp16 -> fp32 past the grid")
    same_bits(_lib.layout("nhwc_to_nchw", ref, np.float32), x.astype(np.float32), "nhwc_to_nchw fp32 past the grid")


def test_bc1s_to_tokens_and_conversions():
    x = ramp((2, 48, 1, 77), np.float16, 7)
    same_bits(_lib.layout("bc1s_to_tokens", x, np.float16), np.ascontiguousarray(x[:, :, 0, :].transpose(0, 2, 1)), "bc1s_to_tokens (2,48,77)")
    rs = np.random.RandomState(8)
    for n in (1, 1000, HALF_GRID + 1):
        special = np.array([0.0, -0.0, 6e-8, -6e-8, 65504.0, -65504.0, np.inf, -np.inf], np.float32)
        f = np.concatenate([special, (rs.randn(n) * 10.0 ** rs.uniform(-9, 5, n)).astype(np.float32)])[:max(n, 1)]
        with np.errstate(over="ignore"):
            fh = f.astype(np.float16)
        same_bits(_lib.layout("convert", f, np.float16), fh, f"float_to_half n={n}")
        hsrc = fh if n > 1 else np.array([-0.0], np.float16)
        same_bits(_lib.layout("convert", hsrc, np.float32), hsrc.astype(np.float32), f"half_to_float n={n}")


@pytest.mark.parametrize("n", [8, 8 * (HALF_GRID + 1)])
def test_sum_half_and_add_half(n):
    """Values whose fp32 sum is not fp16-representable: 2048 + 1.5 -> 2049.5 rounds to 2050 in one rounding, while rounding after
    each addition (2048 + 1 = 2049 -> 2048 (tie to even), + 0.5 -> 2048) or a different source order gives something else."""
    rs = np.random.RandomState(n % 1000)
    srcs = [(rs.randn(n) * 10.0 ** rs.uniform(-3, 3, n)).astype(np.float16) for _ in range(4)]
    for s, v in zip(srcs, (2048.0, 1.0, 0.5, 0.25)):
        s[:8] = v
    acc = srcs[0].astype(np.float32)
    for k in range(1, 5):
        same_bits(_lib.sum_half(srcs[:k]), acc.astype(np.float16), f"sum_half of {k}, n={n}")
        if k < 4:
            acc = acc + srcs[k].astype(np.float32)
    same_bits(_lib.sum_half(srcs[:2], add=True), (srcs[0].astype(np.float32) + srcs[1].astype(np.float32)).astype(np.float16), f"add_half n={n}")
    assert float(_lib.sum_half(srcs[:3])[0]) == 2050.0


@pytest.mark.parametrize("D", [8, 1032])   # 1032: the second trip of the 128-thread x 8 loop is partial
def test_clip_embed(D):
    rs = np.random.RandomState(D)
    S, vocab = 77, 50
    tok, pos = rs.randn(vocab, D).astype(np.float16), rs.randn(S, D).astype(np.float16)
    ids = rs.randint(0, vocab, S).astype(np.int32)
    ids[:4] = [-1, vocab, vocab - 1, 0]
    ref = (tok[np.clip(ids, 0, vocab - 1)].astype(np.float32) + pos.astype(np.float32)).astype(np.float16)
    same_bits(_lib.clip_embed(ids, tok, pos), ref, f"clip_embed D={D}")


def test_vit_patch_rows_and_tokens():
    rs = np.random.RandomState(11)
    B, I, p = 2, 28, 14
    img = rs.randn(B, 3, I, I).astype(np.float16)
    G = I // p
    rows = img.reshape(B, 3, G, p, G, p).transpose(0, 2, 4, 1, 3, 5).reshape(B * G * G, 3 * p * p)
    for Kp in (3 * p * p, 3 * p * p + 20):
        ref = np.zeros((B * G * G, Kp), np.float16)
        ref[:, :3 * p * p] = rows
        same_bits(_lib.vit_patch_rows(img, p, Kp), ref, f"vit_patch_rows Kp={Kp}")
    for D in (40, 1032):
        S = 5
        patch, cls, pos = rs.randn(B, S - 1, D).astype(np.float16), rs.randn(D).astype(np.float16), rs.randn(S, D).astype(np.float16)
        x = np.concatenate([np.broadcast_to(cls, (B, 1, D)), patch], axis=1)
        same_bits(_lib.vit_tokens(patch, cls, pos), (x.astype(np.float32) + pos.astype(np.float32)[None]).astype(np.float16), f"vit_tokens D={D}")


# ------------------------------------------------------------------------------------------------ conv_f32
def run_conv(case, with_bias_res, magnitude=1.0):
    B, Cin, H, W, N, k, stride, up, pad_mode, w_kind = case
    x, w, bias, res = R.conv_inputs(case, magnitude)
    if not with_bias_res:
        bias = res = None
    got = _lib.conv_f32(x, w, bias, res, stride=stride, upsample=up == 2, pad_mode=pad_mode, w_kind=w_kind)
    ref = R.conv_ref(x, w, bias, res, stride, up, pad_mode, w_kind)
    mag = R.conv_ref(x, w, bias, res, stride, up, pad_mode, w_kind, absolute=True)
    R.conv_close(got, ref, mag, k * k * Cin, f"conv_f32 {case} bias/res={with_bias_res} x{magnitude:g}")


@pytest.mark.parametrize("with_bias_res", [False, True])
@pytest.mark.parametrize("case", R.CONV_CASES)
def test_conv_f32(case, with_bias_res):
    run_conv(case, with_bias_res)


@pytest.mark.parametrize("case", [R.CONV_CASES[2], R.CONV_CASES[5]])
def test_conv_f32_at_magnitude_1e6(case):
    """The reason the path exists: activations, bias and residual of magnitude 1e6, far outside fp16, under the same relative bound."""
    run_conv(case, True, magnitude=1.0e6)


# ------------------------------------------------------------------------------------------------ groupnorm_f32
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("case", R.GN_CASES)
def test_groupnorm_f32(case, silu):
    x, gamma, beta = R.gn_inputs(case)
    ref, bound = R.groupnorm_ref(x, gamma, beta, case[4], 1e-6, silu)
    R.bounded_close(_lib.groupnorm_f32(x, gamma, beta, case[4], eps=1e-6, silu=silu), ref, bound, f"groupnorm_f32 {case} silu={silu}")


# ------------------------------------------------------------------------------------------------ row_softmax
@pytest.mark.parametrize("cols", [8, 264, 2048, 2056, 8192])   # 2048: exactly 256 chunks of 8, one per thread
def test_row_softmax_fp16(cols):
    for name, x, scale in R.softmax_rows(cols, False):
        got = _lib.row_softmax(x, scale)
        assert got.dtype == np.float16
        R.softmax_close(got, R.softmax_ref(x, scale), False, f"row_softmax fp16 cols={cols} {name}")


@pytest.mark.parametrize("cols", [1, 7, 256, 257, 1000])
def test_row_softmax_fp32(cols):
    for name, x, scale in R.softmax_rows(cols, True):
        got = _lib.row_softmax(x, scale)
        assert got.dtype == np.float32
        R.softmax_close(got, R.softmax_ref(x, scale), True, f"row_softmax fp32 cols={cols} {name}")


# ------------------------------------------------------------------------------------------------ gemv
def gemv_inputs(B, N, K):
    rs = np.random.RandomState(100000 * B + 1000 * N + K)
    w = (rs.randn(N, K) / np.sqrt(K)).astype(np.float16)
    x = np.clip(1.5 * rs.randn(B, K), -4.0, 4.0).astype(np.float32)
    return w, rs.randn(N).astype(np.float32), x, rs.randn(B, N).astype(np.float32)


@pytest.mark.parametrize("K", [8, 320, 1536, 1544, 3072])   # 1536 / 1544: the last K of the 3-chunk kernels, the first of <4,6,4>
def test_gemv(K):
    """Every N of {1, 31, 33, 100} with every B of {1, 2, 3, 4, 5, 9} (<2,3,8> / <4,3,8> by the batch, <4,6,4> by K, the 4 + 1 and
    4 + 4 + 1 splits); the 16 combinations of silu_in, silu_out, accumulate and bias walk through the 24 shapes, so that every K
    sees each of them at least once."""
    combo, seen = 0, set()
    for N in (1, 31, 33, 100):
        for B in (1, 2, 3, 4, 5, 9):
            silu_in, silu_out, acc, has_bias = (combo >> 0) & 1, (combo >> 1) & 1, (combo >> 2) & 1, (combo >> 3) & 1
            seen.add(combo % 16)
            combo += 5          # co-prime to 16: all 16 combinations within 16 consecutive shapes
            w, bias, x, init = gemv_inputs(B, N, K)
            bias, init = (bias if has_bias else None), (init if acc else None)
            got = _lib.gemv(w, bias, x, init=init, silu_in=silu_in, silu_out=silu_out)
            ref, bound = R.gemv_ref(w, bias, x, init, silu_in, silu_out)
            R.bounded_close(got, ref, bound, f"gemv K={K} N={N} B={B} silu_in={silu_in} silu_out={silu_out} accumulate={acc} bias={has_bias}")
    assert len(seen) == 16


# ------------------------------------------------------------------------------------------------ clip_attention
ATTN_CASES = [(1, 1, 8, None), (2, 3, 40, None), (64, 2, 64, None), (65, 2, 64, None), (77, 2, 64, None), (77, 2, 80, None),
              (80, 1, 128, None), (77, 2, 64, 60.0)]


@pytest.mark.parametrize("S,heads,d,score", ATTN_CASES)
def test_clip_attention(S, heads, d, score):
    qkv = R.attention_inputs(S, heads, d, score)
    D = heads * d
    got = _lib.clip_attention(qkv, heads)
    ref, bound = R.clip_attention_ref(qkv, heads)
    if score is not None:
        s = np.einsum("ihc,jhc->hij", qkv[:, :D].astype(np.float64).reshape(S, heads, d), qkv[:, D:2 * D].astype(np.float64).reshape(S, heads, d))
        assert 50.0 <= np.abs(s).max() * d ** -0.5 <= 70.0
    R.bounded_close(got, ref, bound, f"clip_attention {(S, heads, d, score)}")
    R.close(got, ref, f"clip_attention {(S, heads, d, score)}")
    # row 0 sees key 0 alone: its weight is exp(0) / 1, the output v[0] bit for bit
    same_bits(got[0], qkv[0, 2 * D:], "clip_attention row 0")
    # causality: other keys and values behind position i leave rows <= i bit-identical
    if S > 1:
        i = S // 2 - 1 if S > 2 else 0
        other = qkv.copy()
        other[i + 1:, D:] = R.attention_inputs(S, heads, d, score)[::-1][:S - i - 1, D:] * np.float16(1.5)
        assert not np.array_equal(bits(other[i + 1:, D:]), bits(qkv[i + 1:, D:]))
        again = _lib.clip_attention(other, heads)
        same_bits(again[:i + 1], got[:i + 1], f"clip_attention rows <= {i} with k, v rewritten behind them")
        assert not np.array_equal(bits(again[i + 1:]), bits(got[i + 1:]))


# ------------------------------------------------------------------------------------------------ clip_act
@pytest.mark.parametrize("n", [8, 8 * (HALF_GRID + 1)])
@pytest.mark.parametrize("act", ["quick_gelu", "gelu"])
def test_clip_act(act, n):
    rs = np.random.RandomState(n % 997)
    x = (3.0 * rs.randn(n)).astype(np.float16)
    special = np.array([0.0, -0.0, 6e-8, -6e-8, 3e-5, -3e-5, 65504.0, -65504.0], np.float16)
    if n > 8:
        x[:8] = special
        x[8:4009] = np.linspace(-12, 12, 4001).astype(np.float16)
        got = _lib.clip_act(x, act)
    else:
        x, got = special, _lib.clip_act(special, act)
    assert got.dtype == np.float16 and got.shape == x.shape
    R.clip_act_close(got, R.clip_act_ref(x, act), f"clip_act {act} n={n}")
