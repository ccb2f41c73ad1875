"""CPU part of the operator tests of the kernels that otherwise run only inside whole models (the GPU part:
test_model_only_kernels_gpu.py; references and comparators: model_only_ref.py).

  * the _lib wrappers refuse arrays that do not fit together with ValueError before the library is called;
  * the library refuses what a kernel cannot do before any device work - on a box without a GPU the refusal arrives instead of the
    "no HIP device" error every launch would end in;
  * every toleranced comparator rejects its mutants: the reference with one defect of the kind the GPU cases are there to find,
    built from the reference alone, while the reference rounded to the output type passes."""
import numpy as np
import pytest

import model_only_ref as R
from python_hip_stable_diffusion import _lib


def rejected(fn, *args):
    with pytest.raises(AssertionError):
        fn(*args)


# ------------------------------------------------------------------------------------------------ wrappers and refusals
def test_wrappers_refuse_inconsistent_arrays_before_the_library_is_called(monkeypatch):
    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "lib", no_library)
    f4 = lambda *s: np.zeros(s, np.float32)   # noqa: E731
    h = lambda *s: np.zeros(s, np.float16)    # noqa: E731
    bad = [
        lambda: _lib.conv_f32(f4(1, 4, 5), f4(3, 4, 3, 3)),                          # x not 4-d
        lambda: _lib.conv_f32(f4(1, 4, 5, 7), f4(3, 5, 3, 3)),                       # Cin mismatch
        lambda: _lib.conv_f32(f4(1, 4, 5, 7), f4(3, 4, 5, 5)),                       # ksize 5
        lambda: _lib.conv_f32(f4(1, 4, 5, 7), f4(3, 4, 3, 3), bias=f4(4)),           # bias length
        lambda: _lib.conv_f32(f4(1, 4, 5, 7), f4(3, 4, 3, 3), res=f4(1, 3, 5, 6)),   # residual shape
        lambda: _lib.conv_f32(f4(1, 4, 5, 7), f4(3, 4, 3, 3), w_kind=3),
        lambda: _lib.conv_f32(f4(1, 4, 5, 7), f4(5, 3), w_kind=2),                   # [K][N] with K != Cin
        lambda: _lib.conv_f32(f4(1, 4, 5, 7), f4(3, 4, 3, 3), pad_mode=1),           # the encoder padding on a stride-1 conv
        lambda: _lib.conv_f32(f4(1, 4, 5, 7), f4(3, 4, 3, 3), stride=3),
        lambda: _lib.groupnorm_f32(f4(1, 32, 2, 3), f4(31), f4(32), 8),
        lambda: _lib.groupnorm_f32(f4(1, 32, 2), f4(32), f4(32), 8),
        lambda: _lib.row_softmax(np.zeros((3, 8), np.float64)),
        lambda: _lib.row_softmax(h(3, 2, 8)),
        lambda: _lib.row_softmax(h(0, 8)),
        lambda: _lib.gemv(h(5, 8), None, f4(2, 16)),
        lambda: _lib.gemv(h(5, 8), f4(4), f4(2, 8)),
        lambda: _lib.gemv(h(5, 8), None, f4(2, 8), init=f4(2, 4)),
        lambda: _lib.clip_attention(h(4, 50), 2),
        lambda: _lib.clip_attention(h(4, 48), 3),                                     # D = 16 over 3 heads
        lambda: _lib.clip_embed(np.zeros(5, np.int32), h(10, 8), h(4, 8)),
        lambda: _lib.clip_embed(np.zeros(5, np.int32), h(10, 8), h(5, 16)),
        lambda: _lib.clip_act(h(8), "relu"),
        lambda: _lib.layout("nhwc_to_nchw", h(1, 2, 3, 4), np.float16),               # no kernel writes NCHW fp16
        lambda: _lib.layout("bc1s_to_tokens", h(1, 2, 3, 4), np.float16),             # H != 1
        lambda: _lib.layout("nchw_to_nhwc", h(2, 3, 4), np.float16),
        lambda: _lib.layout("transpose", h(1, 2, 3, 4), np.float16),
        lambda: _lib.sum_half([]),
        lambda: _lib.sum_half([h(8), h(16)]),
        lambda: _lib.sum_half([h(8)] * 3, add=True),
        lambda: _lib.vit_patch_rows(h(2, 3, 28, 28), 14, 3 * 14 * 14 - 1),
        lambda: _lib.vit_patch_rows(h(2, 3, 28, 28), 12, 1024),
        lambda: _lib.vit_patch_rows(h(2, 4, 28, 28), 14, 1024),
        lambda: _lib.vit_tokens(h(2, 4, 40), h(40), h(4, 40)),
        lambda: _lib.vit_tokens(h(2, 4, 40), h(32), h(5, 40)),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {i} was accepted")


def test_the_library_refuses_before_any_device_work(sdlib):
    """What a kernel cannot do is SD_ERR_UNSUPPORTED / SD_ERR_INVALID_ARGUMENT from the entry point, raised in front of the first
    HIP call: without a GPU the same calls would otherwise end in RuntimeError (no HIP device)."""
    h = lambda *s: np.zeros(s, np.float16)    # noqa: E731
    f4 = lambda *s: np.zeros(s, np.float32)   # noqa: E731
    for K in (12, 3080):
        with pytest.raises(NotImplementedError, match="gemv"):
            _lib.gemv(h(4, K), None, f4(1, K))
    for cols in (12, 8200):
        with pytest.raises(NotImplementedError, match="row_softmax"):
            _lib.row_softmax(h(3, cols))
    for S, heads, d in ((81, 1, 64), (4, 1, 136), (4, 2, 12)):
        with pytest.raises(NotImplementedError, match="clip_attention"):
            _lib.clip_attention(h(S, 3 * heads * d), heads)
    with pytest.raises(NotImplementedError, match="clip_embed"):
        _lib.clip_embed(np.zeros(77, np.int32), h(10, 12), h(77, 12))
    with pytest.raises(NotImplementedError, match="groupnorm_f32"):
        _lib.groupnorm_f32(f4(1, 33, 2, 3), f4(33), f4(33), 32)
    with pytest.raises(NotImplementedError, match="vit_tokens"):
        _lib.vit_tokens(h(2, 4, 12), h(12), h(5, 12))
    with pytest.raises(ValueError, match="sum_half"):
        _lib.sum_half([h(12)])
    with pytest.raises(ValueError, match="sum_half"):
        _lib.sum_half([h(8)] * 5)
    with pytest.raises(ValueError, match="sum_half"):
        _lib.sum_half([h(12), h(12)], add=True)
    with pytest.raises(ValueError, match="clip_act"):
        _lib.clip_act(h(12), "gelu")
    with pytest.raises(ValueError, match="conv_f32"):
        _lib.conv_f32(f4(1, 4, 1, 1), f4(3, 4, 3, 3), stride=2, pad_mode=1)           # empty output


# ------------------------------------------------------------------------------------------------ mutants
def conv_refs(case, magnitude=1.0, mutant=None):
    B, Cin, H, W, N, k, stride, up, pad_mode, w_kind = case
    x, w, bias, res = R.conv_inputs(case, magnitude)
    ref = R.conv_ref(x, w, bias, res, stride, up, pad_mode, w_kind, mutant=mutant)
    mag = R.conv_ref(x, w, bias, res, stride, up, pad_mode, w_kind, absolute=True)
    return ref, mag, k * k * Cin


def test_conv_comparator_rejects_the_mutants():
    for case in R.CONV_CASES:
        ref, mag, K = conv_refs(case)
        R.conv_close(ref.astype(np.float32), ref, mag, K, f"fp32-rounded reference {case}")
    for case in [c for c in R.CONV_CASES if c[5] == 3]:
        ref, mag, K = conv_refs(case)
        rejected(R.conv_close, conv_refs(case, mutant="drop_tap")[0], ref, mag, K, f"one tap dropped at pixel (0, 0) {case}")
        if case != (2, 8, 9, 11, 70, 3, 2, 1, 1, 1):   # (0,1,0,1) padding at an odd image: no output reads it
            rejected(R.conv_close, conv_refs(case, mutant="edge_clamp")[0], ref, mag, K, f"edge clamp instead of zero padding {case}")
    up_case = R.CONV_CASES[5]
    assert up_case[7] == 2
    ref, mag, K = conv_refs(up_case)
    rejected(R.conv_close, conv_refs(up_case, mutant="up_shift")[0], ref, mag, K, "upsample shifted by one")
    ref, mag, K = conv_refs(R.CONV_CASES[2], magnitude=1.0e6)   # the bound scales with the data: still tight at 1e6
    R.conv_close(ref.astype(np.float32), ref, mag, K, "fp32-rounded reference at 1e6")
    rejected(R.conv_close, conv_refs(R.CONV_CASES[2], 1.0e6, "drop_tap")[0], ref, mag, K, "one tap dropped at 1e6")


def test_groupnorm_comparator_rejects_the_mutants():
    for case in R.GN_CASES:
        x, gamma, beta = R.gn_inputs(case)
        for silu in (False, True):
            ref, bound = R.groupnorm_ref(x, gamma, beta, case[4], 1e-6, silu)
            R.bounded_close(ref.astype(np.float32), ref, bound, f"fp32-rounded reference {case} silu={silu}")
            for mutant in ("neighbour", "unbiased"):
                rejected(R.bounded_close, R.groupnorm_ref(x, gamma, beta, case[4], 1e-6, silu, mutant=mutant)[0], ref, bound,
                         f"{mutant} {case} silu={silu}")


def test_softmax_comparator_rejects_the_mutant():
    for fp32, cols in ((False, 264), (True, 257)):
        out = np.float32 if fp32 else np.float16
        seen = 0
        for name, x, scale in R.softmax_rows(cols, fp32):
            ref = R.softmax_ref(x, scale)
            R.softmax_close(ref.astype(out), ref, fp32, f"rounded reference, {name}")
            if scale < 0:   # the maximum taken before scaling is the minimum of the scores: the exponentials overflow
                rejected(R.softmax_close, R.softmax_ref(x, scale, mutant="max_before_scale"), ref, fp32, f"max before scale, {name}")
                seen += 1
        assert seen == 1


def gemv_inputs(B, N, K, seed=0):
    rs = np.random.RandomState(seed + 100000 * B + 1000 * N + K)
    w = (rs.randn(N, K) / np.sqrt(K)).astype(np.float16)
    x = np.clip(1.5 * rs.randn(B, K), -4.0, 4.0).astype(np.float32)
    bias = rs.randn(N).astype(np.float32)
    init = rs.randn(B, N).astype(np.float32)
    return w, bias, x, init


def test_gemv_comparator_rejects_the_mutants():
    for K in (8, 320, 3072):
        w, bias, x, init = gemv_inputs(3, 33, K)
        for silu_in, silu_out, acc in ((0, 0, 0), (1, 0, 1), (0, 1, 0), (1, 1, 1)):
            i = init if acc else None
            ref, bound = R.gemv_ref(w, bias, x, i, silu_in, silu_out)
            R.bounded_close(ref.astype(np.float32), ref, bound, f"fp32-rounded reference K={K}")
            for mutant in ("drop_chunk", "no_bias", "swap_rows"):
                rejected(R.bounded_close, R.gemv_ref(w, bias, x, i, silu_in, silu_out, mutant=mutant)[0], ref, bound,
                         f"{mutant} K={K} silu_in={silu_in} silu_out={silu_out} accumulate={acc}")


def test_clip_attention_comparator_rejects_the_mutants():
    for S, heads, d, score in ((2, 3, 40, None), (77, 2, 64, None), (77, 2, 64, 60.0)):
        qkv = R.attention_inputs(S, heads, d, score)
        ref, bound = R.clip_attention_ref(qkv, heads)
        R.bounded_close(ref.astype(np.float16), ref, bound, f"fp16-rounded reference {(S, heads, d, score)}")
        for mutant in ("strict", "ahead"):
            rejected(R.bounded_close, R.clip_attention_ref(qkv, heads, mutant=mutant)[0], ref, bound, f"{mutant} {(S, heads, d, score)}")


def test_clip_act_comparator():
    x = np.concatenate([np.linspace(-12, 12, 4001), [0.0, -0.0, 6e-8, -6e-8, 3e-5, -3e-5, 65504.0, -65504.0]]).astype(np.float16)
    for act in ("quick_gelu", "gelu"):
        ref = R.clip_act_ref(x, act)
        with np.errstate(over="ignore"):
            R.clip_act_close(ref.astype(np.float16), ref, f"fp16-rounded reference {act}")
        rejected(R.clip_act_close, R.clip_act_ref(x, "gelu" if act == "quick_gelu" else "quick_gelu"), ref, f"the other activation for {act}")
