"""CPU suite of sd_op_attention_kernel (``_lib.attention_kernel``): which kernel the three attention launchers choose, asked of the
choice functions the launchers themselves call.  Without a device the compute-unit count the rules read is 256 (an MI355X has 256
too), so every line below is what the GPU suites must see: the cases of test_attention_forms_gpu.py and test_w8a8_einsum_gpu.py are
pinned here, beside the UNet's own shapes, both sides of every threshold, and the refusals.

Last, the check the docstring of test_w8a8_einsum_gpu.py used to report only: the numpy restatement of the int8 einsums against
itself, its exp2 moved by one fp32 ulp (alternating sign per element) from a float64 exp2, stays inside criteria (a), (b) and (c) of
that file on every shape of that file - so the 2 % cap of (b) is met by the reference alone on those inputs."""
import ctypes as C

import numpy as np
import pytest

import test_attention_forms_gpu as forms
import test_w8a8_einsum_gpu as einsum
import w8a8_einsum_ref as ref
from python_hip_stable_diffusion import _lib

k = _lib.attention_kernel


def i8(B, heads, S):
    return k(None, B, heads, 64, S, int8=True)


def test_the_gpu_cases_reach_the_forms_they_are_there_for():
    for shape in einsum.SHAPES:
        assert i8(*shape) == einsum.KERNEL[shape], shape
        assert i8(1, 1, shape[2]) == "attn_i8 w4"                                # the sub-problem of the bit-equality check
    assert [einsum.KERNEL[s] for s in einsum.SHAPES] == ["attn_i8 w4"] * 4 + ["attn_i8 w8"] * 3
    for impl in forms.IMPLS:
        for B, heads, Sq, Sk in forms.CLASSIC + [forms.PATTERN_SHAPE]:
            assert k(impl, B, heads, 64, Sq, Sk) == "attn8 w8 classic", (impl, B, heads, Sq, Sk)
            assert k(impl, B, heads, 64, Sq, Sk, 1) == forms.GENERAL_W4[impl]
            assert k(impl, 1, 1, 64, Sq, Sk) == "attn8 w4 classic"
        assert k(impl, *forms.PATTERN_SHAPE[:2], 64, 256, 397) == forms.GENERAL_W4[impl]          # ragged keys: never attention8
        for variant in (0, 2, 3):
            assert k(impl, 4, 16, 64, 320, 320, variant) == "attn8 w8 classic"
    for (B, heads, Sq, Sk, upw), want in forms.BALANCED:
        assert k("ORIGINAL", B, heads, 64, Sq, Sk, 100 + upw) == want
        assert k("ORIGINAL", B, heads, 64, Sq, Sk) == want[:9] + "classic"      # explicit splits only: the launch's own rule keeps the classic grid
    assert [w for _, w in forms.BALANCED] == ["attn8 w8 balanced upw=3 seg=2", "attn8 w8 balanced upw=1 seg=1", "attn8 w8 balanced upw=7 seg=3",
                                              "attn8 w8 balanced upw=5 seg=3", "attn8 w4 balanced upw=3 seg=2"]
    for (B, heads, d, Sq, Sk), variant, want in forms.V2:
        assert k("SPLIT_EINSUM_V2", B, heads, d, Sq, Sk, variant) == want, (B, heads, d, Sq, Sk)
    assert [w for _, _, w in forms.V2] == ["attn d16 split w8 qt2", "attn d40 split w8 qt2", "attn d64 split w8 qt2", "attn d64 split w8 qt2",
                                           "attn d64 split w8 qt1", "attn d80 split w8 qt1", "attn d160 split w8 qt1", "attn d64 split w8 qt2",
                                           "attn d40 split w4 qt1"]


def test_the_unets_own_self_attentions():
    """SD2.1 at 64 x 64 latents, batch 2 (160 eight-wave workgroups: the balanced form, 40 units each) and a 40 x 72 latent at batch 4 run
    eight waves; the 32 x 32 and 16 x 16 levels four"""
    assert k("ORIGINAL", 2, 5, 64, 4096, 4096) == "attn8 w8 balanced upw=40 seg=2" and i8(2, 5, 4096) == "attn_i8 w8"
    assert k("ORIGINAL", 4, 5, 64, 2880, 2880) == "attn8 w8 classic" and i8(4, 5, 2880) == "attn_i8 w8"          # a tail query tile: no balanced form
    assert k("ORIGINAL", 2, 10, 64, 1024, 1024) == "attn8 w4 classic" and i8(2, 10, 1024) == "attn_i8 w4"
    assert k("ORIGINAL", 2, 20, 64, 256, 256) == "attn8 w4 classic" and i8(2, 20, 256) == "attn_i8 w4"
    for impl in ("SPLIT_EINSUM", "SPLIT_EINSUM_V2"):                              # attention8 has one schedule
        assert k(impl, 2, 5, 64, 4096, 4096) == "attn8 w8 balanced upw=40 seg=2"
    assert k("ORIGINAL", 2, 5, 64, 4096, 77) == "attn d64 original w4 qt1" and k("SPLIT_EINSUM", 2, 5, 64, 4096, 77) == "attn d64 split w4 qt1"
    assert k("SPLIT_EINSUM_V2", 2, 8, 40, 4096, 4096) == "attn d40 split w8 qt1"  # SD1.5 at batch 2: 128 chunks


def test_thresholds_on_both_sides():
    """one waves rule for attention8.hip and attention_i8.hip: eight where B * heads * ceil(Sq / 256) >= CUs / 2 = 128"""
    for Sq in (64, 256):
        assert k("ORIGINAL", 127, 1, 64, Sq, 64) == "attn8 w4 classic" and k("ORIGINAL", 128, 1, 64, Sq, 64) == "attn8 w8 classic"
        assert k("ORIGINAL", 1, 127, 64, Sq, 64) == "attn8 w4 classic" and k("ORIGINAL", 1, 128, 64, Sq, 64) == "attn8 w8 classic"
        assert i8(127, 1, Sq) == "attn_i8 w4" and i8(128, 1, Sq) == "attn_i8 w8" and i8(1, 128, Sq) == "attn_i8 w8"
    assert k("ORIGINAL", 1, 63, 64, 512, 64) == "attn8 w4 classic" and k("ORIGINAL", 1, 64, 64, 512, 64) == "attn8 w8 classic"   # ceil(Sq / 256) = 2
    assert k("ORIGINAL", 1, 64, 64, 257, 64) == "attn8 w8 classic" and k("ORIGINAL", 1, 64, 64, 256, 64) == "attn8 w4 classic"
    assert i8(1, 63, 512) == "attn_i8 w4" and i8(1, 64, 512) == "attn_i8 w8" and i8(1, 64, 320) == "attn_i8 w8"
    assert k("ORIGINAL", 127, 1, 64, 256, 256, 103) == "attn8 w4 balanced upw=3 seg=2"            # the balanced form follows the same rule
    assert k("ORIGINAL", 128, 1, 64, 256, 256, 103) == "attn8 w8 balanced upw=3 seg=2"
    # SPLIT_EINSUM_V2 chunks of 512 queries: 96 -> eight waves, 192 -> two query tiles per wave
    for d in (16, 40, 64):
        assert k("SPLIT_EINSUM_V2", 95, 1, d, 512, 77) == f"attn d{d} split w4 qt1" and k("SPLIT_EINSUM_V2", 96, 1, d, 512, 77) == f"attn d{d} split w8 qt1"
        assert k("SPLIT_EINSUM_V2", 191, 1, d, 512, 77) == f"attn d{d} split w8 qt1" and k("SPLIT_EINSUM_V2", 192, 1, d, 512, 77) == f"attn d{d} split w8 qt2"
        assert k("SPLIT_EINSUM_V2", 1, 48, d, 1024, 77) == f"attn d{d} split w8 qt1" and k("SPLIT_EINSUM_V2", 1, 96, d, 1024, 77) == f"attn d{d} split w8 qt2"
        assert k("SPLIT_EINSUM_V2", 500, 1, d, 256, 77) == f"attn d{d} split w4 qt1"              # below one chunk: SPLIT_EINSUM's launch
        assert k("SPLIT_EINSUM", 500, 1, d, 512, 77) == f"attn d{d} split w4 qt1" and k("ORIGINAL", 500, 1, d, 512, 77) == f"attn d{d} original w4 qt1"


def test_head_dims_above_64_never_get_two_query_tiles_per_wave():
    for d in range(8, 161, 8):
        for chunks in (95, 96, 191, 192, 193, 4096):
            line = k("SPLIT_EINSUM_V2", chunks, 1, d, 512, 77)
            waves, qt = (8, 2 if d <= 64 else 1) if chunks >= 192 else (8, 1) if chunks >= 96 else (4, 1)
            assert line == f"attn d{d} split w{waves} qt{qt}", (d, chunks, line)


def test_refusals_are_those_of_the_entries():
    refused = [
        (lambda: k("ORIGINAL", 0, 1, 64, 64, 64), ValueError, "empty attention problem"),
        (lambda: k("ORIGINAL", 1, 1, 64, 64, 0), ValueError, "empty attention problem"),
        (lambda: k("ORIGINAL", 1, 1, 64, 64, 77, 3), ValueError, "Sq == Sk"),
        (lambda: k("ORIGINAL", 1, 1, 40, 64, 64, 2), ValueError, "variant 2"),
        (lambda: k("ORIGINAL", 1, 1, 64, 64, 77, 100), ValueError, "variant 100 .balanced form. needs attention8's shape"),
        (lambda: k("ORIGINAL", 1, 1, 64, 33, 64, 103), ValueError, "variant 103: the balanced form cannot run this shape"),
        (lambda: k("ORIGINAL", 1, 1, 12, 64, 64), NotImplementedError, "head dim 12"),
        (lambda: k("ORIGINAL", 1, 1, 168, 64, 64), NotImplementedError, "head dim 168"),
        (lambda: k("SPLIT_EINSUM_V2", 1, 1, 64, 576, 77), ValueError, "512"),
        (lambda: k("FLASH", 1, 1, 64, 64, 64), ValueError, "unknown attention implementation"),
        (lambda: i8(0, 1, 64), ValueError, "empty problem"),
        (lambda: i8(1, 1, 100), ValueError, "off the shape rule"),
        (lambda: i8(1, 1, 32), ValueError, "off the shape rule"),
        (lambda: i8(1, 1, ref.MAX_S + 64), ValueError, "133120"),
    ]
    for call, error, match in refused:
        with pytest.raises(error, match=match):
            call()
        assert i8(1, 1, ref.MAX_S) == "attn_i8 w8" and k("ORIGINAL", 1, 1, 64, 64, 64) == "attn8 w4 classic"   # a valid question right after
    lib = _lib.lib()
    with pytest.raises(ValueError, match="unknown attention implementation 3"):
        _lib.check(lib.sd_op_attention_kernel(0, 3, 1, 1, 64, 64, 64, 0, C.create_string_buffer(96), 96))
    with pytest.raises(ValueError, match="bad attention_kernel arguments"):
        _lib.check(lib.sd_op_attention_kernel(0, 0, 1, 1, 64, 64, 64, 0, None, 96))
    small = C.create_string_buffer(8)
    with pytest.raises(ValueError, match="the text buffer holds 8 bytes"):
        _lib.check(lib.sd_op_attention_kernel(0, 0, 1, 1, 64, 64, 64, 0, small, 8))


def exp2_f64(x):
    return np.exp2(x.astype(np.float64)).astype(np.float32)


@pytest.mark.parametrize("shape", einsum.SHAPES, ids=einsum.ids3)
def test_restatement_with_exp2_one_ulp_off_stays_inside_the_criteria(shape):
    c = einsum.case_of(shape)
    einsum.check_inputs(c)
    moved = [0, 0]

    def exp2_off(x):
        e = exp2_f64(x)
        up = (np.indices(e.shape).sum(axis=0) & 1).astype(bool)                   # alternating sign per element
        off = np.where(up, np.nextafter(e, np.float32(np.inf)), np.nextafter(e, np.float32(-np.inf)))
        moved[0] += np.count_nonzero(np.rint(np.float32(127.0) * off) != np.rint(np.float32(127.0) * e))
        moved[1] += e.size
        return off

    args = (c["q"], c["k"], c["v"], einsum.R_QK, einsum.R_QK, einsum.R_V, c["B"], c["heads"])
    want = ref.attention(*args, exp2=exp2_f64)
    got = ref.attention(*args, exp2=exp2_off)
    print(f"{shape}: {moved[0]} of {moved[1]} probabilities moved")
    einsum.criteria(got, want, c, f"{shape} restatement, exp2 one ulp off")
