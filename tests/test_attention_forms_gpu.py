"""GPU suite of the launch forms of the attention kernels that only a chip-filling grid selects: attn8_kernel<8, ...> classic and
balanced (attention8.hip), and the eight-wave SPLIT_EINSUM_V2 forms of the general kernel (attention.hip), one and two query tiles
per wave.  (attn_i8_kernel<8, 4> is in test_w8a8_einsum_gpu.py, whose criteria it shares.)  The launchers pick these by the number of
workgroups a problem makes, so the shapes have many samples and heads and few tokens: a few MB each.

Every case first asks ``_lib.attention_kernel`` - the launcher's own choice function - which kernel the call will run and compares the
line with the one written beside the case (pinned for 256 compute units by test_attention_kernel.py, without a GPU): on a device
with another CU count the case fails there, it does not pass on another kernel.

Gates: ``close`` of test_ops_gpu.py (60 dB, 4e-3 max|ref| + 1e-3) against oracle/attention_ref.py; test_round4_gpu.py's comparison with
the general kernel (55 dB); test_round6_gpu.py's three assertions for the balanced form.  Bit equalities: variant 3 against variant 0,
and every (sample, head) of an eight-wave attention8 launch against the four-wave launch of that (1, 1, Sq, Sk) problem alone - a wave
holds the same 32-aligned queries, walks the same key tiles and takes the same refresh vote in both."""
import re

import numpy as np
import pytest

from oracle import attention_ref
from python_hip_stable_diffusion import _lib
from test_ops_gpu import IMPLS, close, h16

gpu = pytest.mark.gpu
PASSED = []                                                                      # the query's line of every launch whose result passed its gate

ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)   # noqa: E731


def f32(*a):
    return [x.astype(np.float32) for x in a]


def ask(impl, B, heads, d, Sq, Sk, variant, want):
    line = _lib.attention_kernel(impl, B, heads, d, Sq, Sk, variant)
    assert line == want, f"{impl} {(B, heads, d, Sq, Sk)} variant {variant} is here for '{want}', this device would run '{line}'"
    return line


def randn_qkv(seed, B, heads, d, Sq, Sk):
    rs = np.random.RandomState(seed)
    return [rs.randn(B, heads * d, 1, n).astype(np.float32) for n in (Sq, Sk, Sk)]


def alone(t, b, h, d=64):
    return np.ascontiguousarray(t[b:b + 1, h * d:(h + 1) * d])


def assert_heads_equal_four_waves(impl, q, k, v, heads, got, what, variant=0):
    """samples 0 and B - 1, heads 0 and heads - 1 of the eight-wave result ``got``: bit for bit the four-wave launch of that head alone"""
    B, Sq, Sk = q.shape[0], q.shape[3], k.shape[3]
    for b in sorted({0, B - 1}):
        for h in sorted({0, heads - 1}):
            line = ask(impl, 1, 1, 64, Sq, Sk, variant, "attn8 w4 classic")
            sub, _ = _lib.attention(impl, alone(q, b, h), alone(k, b, h), alone(v, b, h), 1, 64, variant=variant)
            n = np.count_nonzero(sub.view(np.uint16) != alone(got, b, h).view(np.uint16))
            print(f"{what} sample {b} head {h}: {n} of {sub.size} values differ between eight and four waves")
            assert n == 0, f"{what} sample {b} head {h}: {n} of {sub.size} values differ between the eight- and the four-wave kernel"
            PASSED.append(line)


# ------------------------------------------------------------------ attention8, eight waves, classic grid
CLASSIC = [  # (B, heads, Sq, Sk): one key tile, six waves of eight without a query | a tail query tile of two waves | Sq != Sk | queries ragged inside a wave
    (8, 16, 64, 64), (4, 16, 320, 320), (4, 16, 320, 128), (4, 16, 300, 192),
]
GENERAL_W4 = {"ORIGINAL": "attn d64 original w4 qt1", "SPLIT_EINSUM": "attn d64 split w4 qt1", "SPLIT_EINSUM_V2": "attn d64 split w4 qt1"}   # Sq < 512


@gpu
@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("shape", CLASSIC, ids=ids)
def test_attention8_eight_waves_against_oracle_general_kernel_and_four_waves(impl, shape):
    B, heads, Sq, Sk = shape
    line = ask(impl, B, heads, 64, Sq, Sk, 0, "attn8 w8 classic")
    line1 = ask(impl, B, heads, 64, Sq, Sk, 1, GENERAL_W4[impl])
    q, k, v = (h16(t) for t in randn_qkv(4000 + Sq + Sk, B, heads, 64, Sq, Sk))
    ref = attention_ref.IMPLS[impl](*f32(q, k, v), heads, 64)
    new, _ = _lib.attention(impl, q, k, v, heads, 64, variant=0)
    old, _ = _lib.attention(impl, q, k, v, heads, 64, variant=1)
    close(new, ref, f"{line} {impl} {shape}")
    close(old, ref, f"{line1} {impl} {shape}")
    close(new, old.astype(np.float32), f"{line} vs {line1} {impl} {shape}", min_psnr=55)
    PASSED.extend([line, line1])
    assert_heads_equal_four_waves(impl, q, k, v, heads, new, f"{impl} {shape}")


PATTERN_SHAPE = (8, 16, 256, 448)


def pattern_inputs(pattern):
    """test_attention_lazy_running_max_patterns of test_ops_gpu.py at PATTERN_SHAPE (ragged_rising keeps that test's 397 keys, which no
    attention8 form can run: the query names the general kernel for it)"""
    B, heads, Sq, Sk = PATTERN_SHAPE
    if pattern == "ragged_rising":
        Sk = 397
    q, k, v = randn_qkv(11, B, heads, 64, Sq, Sk)
    tile = np.arange(Sk) // 64
    if pattern in ("rising", "ragged_rising"):
        k *= (1.0 + 0.9 * tile)[None, None, None, :]          # every 64-key tile raises the max
    elif pattern == "falling":
        k *= (6.0 / (1.0 + tile))[None, None, None, :]        # the first tile dominates
    elif pattern == "outlier_query":
        q[:, :, :, 37] *= 12.0                                # one row keeps triggering the wave-wide vote
        k *= (1.0 + 0.4 * tile)[None, None, None, :]
    elif pattern == "flat":
        q[:] = 0.0                                            # all scores 0 -> uniform weights
    return h16(q), h16(k), h16(v)


PATTERN_REFS = {}


def pattern_case(pattern):
    if pattern not in PATTERN_REFS:
        q, k, v = pattern_inputs(pattern)
        PATTERN_REFS[pattern] = (q, k, v, attention_ref.original(*f32(q, k, v), PATTERN_SHAPE[1], 64))
    return PATTERN_REFS[pattern]


@gpu
@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("pattern", ["rising", "falling", "outlier_query", "flat", "ragged_rising"])
def test_attention8_eight_waves_lazy_running_max_patterns(impl, pattern):
    B, heads, Sq, _ = PATTERN_SHAPE
    q, k, v, ref = pattern_case(pattern)
    line = ask(impl, B, heads, 64, Sq, k.shape[3], 0, GENERAL_W4[impl] if pattern == "ragged_rising" else "attn8 w8 classic")
    out, _ = _lib.attention(impl, q, k, v, heads, 64)
    close(out, ref, f"{line} {impl} lazy-max {pattern}")
    PASSED.append(line)
    if line.startswith("attn8"):
        assert_heads_equal_four_waves(impl, q, k, v, heads, out, f"{impl} lazy-max {pattern}")


@gpu
@pytest.mark.parametrize("impl", IMPLS)
def test_attention8_eight_waves_running_max_rescale_branch(impl):
    """test_attention_running_max_rescale_branch at PATTERN_SHAPE: late key tiles carry much larger scores than early ones, and one key
    of the last tile dominates query 7"""
    B, heads, Sq, Sk = PATTERN_SHAPE
    line = ask(impl, B, heads, 64, Sq, Sk, 0, "attn8 w8 classic")
    q, k, v = randn_qkv(5, B, heads, 64, Sq, Sk)
    k[:, :, :, 300:] *= 6.0                  # scores jump inside tile 4
    k[:, :, :, 430] = 3.0 * q[:, :, :, 7]    # one key dominates query 7
    q, k, v = h16(q), h16(k), h16(v)
    out, _ = _lib.attention(impl, q, k, v, heads, 64)
    close(out, attention_ref.original(*f32(q, k, v), heads, 64), f"{line} {impl} rescale")
    PASSED.append(line)
    assert_heads_equal_four_waves(impl, q, k, v, heads, out, f"{impl} rescale")


@gpu
def test_attention8_eight_waves_first_key_tile_far_below_zero():
    """test_attention8_first_key_tile_far_below_zero of test_round5_gpu.py at PATTERN_SHAPE, the construction applied to heads 0 and 15:
    the first 64 keys of those heads score below -128 in log2 units for a query, so the seed of the running max must only set the max"""
    B, heads, Sq, Sk = PATTERN_SHAPE
    rs = np.random.RandomState(11)
    q = rs.randn(B, heads, 64, Sq).astype(np.float32)
    k = rs.randn(B, heads, 64, Sk).astype(np.float32)
    v = rs.randn(B, heads * 64, 1, Sk).astype(np.float32)
    for h in (0, heads - 1):
        q[:, h] *= 3.0
        qm = q[:, h].mean(axis=2, keepdims=True)                             # a direction every query of the head shares
        q[:, h] += 6.0 * np.sign(qm)
        k[:, h, :, :64] = -8.0 * np.sign(qm) + 0.1 * k[:, h, :, :64]          # first key tile: q.k / 8 * log2(e) far below -128
    q, k, v = h16(q.reshape(B, heads * 64, 1, Sq)), h16(k.reshape(B, heads * 64, 1, Sk)), h16(v)
    qf, kf = q.astype(np.float32).reshape(B, heads, 64, Sq), k.astype(np.float32).reshape(B, heads, 64, Sk)
    for h in (0, heads - 1):
        s0 = np.einsum("bcq,bck->bqk", qf[:, h], kf[:, h, :, :64])
        assert (s0.max(axis=2) / 8 * 1.4427 < -128).any(), f"head {h}: the case must reach the overflow range"
    ref = attention_ref.original(*f32(q, k, v), heads, 64)
    for impl in ("ORIGINAL", "SPLIT_EINSUM"):
        line = ask(impl, B, heads, 64, Sq, Sk, 0, "attn8 w8 classic")
        out, _ = _lib.attention(impl, q, k, v, heads, 64)
        close(out, ref, f"{line} {impl}, first tile below -128")
        PASSED.append(line)
        assert_heads_equal_four_waves(impl, q, k, v, heads, out, f"{impl} first tile below -128")


@gpu
@pytest.mark.parametrize("impl", IMPLS)
def test_attention8_eight_waves_strided_qk_and_prescaled_q(impl):
    """variant 3 (q and k rows of ONE [B][S][2C] buffer): other addresses, same arithmetic - bit-equal to variant 0.  variant 2 (q arrives
    multiplied by d^-0.5 * log2(e), rounded once): inside the gate against the oracle on the un-scaled q."""
    B, heads, S = 4, 16, 320
    for variant in (0, 2, 3):
        line = ask(impl, B, heads, 64, S, S, variant, "attn8 w8 classic")
    q, k, v = (h16(t) for t in randn_qkv(4321, B, heads, 64, S, S))
    ref = attention_ref.IMPLS[impl](*f32(q, k, v), heads, 64)
    plain, _ = _lib.attention(impl, q, k, v, heads, 64, variant=0)
    strided, _ = _lib.attention(impl, q, k, v, heads, 64, variant=3)
    close(strided, ref, f"{line} {impl} q|k interleaved")
    n = np.count_nonzero(strided.view(np.uint16) != plain.view(np.uint16))
    assert n == 0, f"{impl}: {n} of {plain.size} values differ between ldq = C and ldq = 2C"
    c = np.float32(1.4426950408889634 / 8.0)
    scaled, _ = _lib.attention(impl, h16(q.astype(np.float32) * c), k, v, heads, 64, variant=2)
    close(scaled, ref, f"{line} {impl} pre-scaled q")
    PASSED.extend([line] * 3)


# ------------------------------------------------------------------ attention8, balanced form, explicit splits
BALANCED = [  # (B, heads, Sq, Sk, upw), the query's line
    ((8, 16, 256, 256, 3), "attn8 w8 balanced upw=3 seg=2"),      # an explicit split
    ((8, 16, 256, 256, 1), "attn8 w8 balanced upw=1 seg=1"),      # one key tile per workgroup
    ((4, 16, 512, 320, 7), "attn8 w8 balanced upw=7 seg=3"),      # crosses into the next query tile
    ((8, 16, 256, 128, 5), "attn8 w8 balanced upw=5 seg=3"),      # more units than a query tile has
    ((1, 2, 256, 256, 3), "attn8 w4 balanced upw=3 seg=2"),       # (the four-wave form, for the coverage list)
]
CLASSIC_OF = {8: "attn8 w8 classic", 4: "attn8 w4 classic"}


@gpu
@pytest.mark.parametrize("case,want", BALANCED, ids=ids)
def test_attention8_balanced_form_eight_waves(case, want):
    """the three assertions of test_attention8_balanced_form (test_round6_gpu.py) on its inputs: oracle, classic grid, bit-reproducible"""
    from test_round6_gpu import attn_ref
    B, heads, Sq, Sk, upw = case
    line = ask("ORIGINAL", B, heads, 64, Sq, Sk, 100 + upw, want)
    line0 = ask("ORIGINAL", B, heads, 64, Sq, Sk, 0, CLASSIC_OF[int(want[7])])
    rs = np.random.RandomState(Sq + Sk + upw)
    c = heads * 64
    q = h16(rs.randn(B, c, 1, Sq) * 1.5)
    k = h16(rs.randn(B, c, 1, Sk) * 1.5)
    k[:, :, :, Sk // 2:] *= 1.8                                  # the later keys carry the larger scores: the running max moves between segments
    v = h16(rs.randn(B, c, 1, Sk))
    got, _ = _lib.attention("ORIGINAL", q, k, v, heads, 64, variant=100 + upw)
    classic, _ = _lib.attention("ORIGINAL", q, k, v, heads, 64, variant=0)
    close(got, attn_ref(q, k, v, heads), f"{line} B={B} h={heads} {Sq}x{Sk}", min_psnr=60.0, rel=6e-3)
    close(got, classic.astype(np.float32), f"{line} vs {line0}", min_psnr=66.0, rel=4e-3)
    again, _ = _lib.attention("ORIGINAL", q, k, v, heads, 64, variant=100 + upw, iters=3)    # the counters come back to zero; arrival order does not matter
    assert np.array_equal(got.view(np.uint16), again.view(np.uint16)), "bit-reproducible"
    PASSED.extend([line, line0])


# ------------------------------------------------------------------ the general kernel, SPLIT_EINSUM_V2 on whole 512-query chunks, keys ragged
V2 = [  # (B, heads, d, Sq, Sk), variant, the query's line
    ((12, 16, 16, 512, 77), 0, "attn d16 split w8 qt2"),
    ((12, 16, 40, 512, 77), 0, "attn d40 split w8 qt2"),
    ((12, 16, 64, 512, 77), 0, "attn d64 split w8 qt2"),
    ((6, 16, 64, 1024, 129), 0, "attn d64 split w8 qt2"),         # two chunks per head, a third key tile of one key
    ((6, 16, 64, 512, 77), 0, "attn d64 split w8 qt1"),           # 96 chunks
    ((12, 16, 80, 512, 77), 0, "attn d80 split w8 qt1"),          # d > 64 at 192 chunks
    ((6, 16, 160, 512, 65), 0, "attn d160 split w8 qt1"),
    ((12, 16, 64, 512, 128), 1, "attn d64 split w8 qt2"),         # the general kernel at a shape attention8 would otherwise take
    ((1, 8, 40, 256, 77), 0, "attn d40 split w4 qt1"),            # (the four-wave form, for the coverage list)
]


@gpu
@pytest.mark.parametrize("shape,variant,want", V2, ids=ids)
def test_split_einsum_v2_eight_wave_forms(shape, variant, want):
    B, heads, d, Sq, Sk = shape
    line = ask("SPLIT_EINSUM_V2", B, heads, d, Sq, Sk, variant, want)
    q, k, v = (h16(t) for t in randn_qkv(7000 + d + Sq + Sk, B, heads, d, Sq, Sk))
    out, _ = _lib.attention("SPLIT_EINSUM_V2", q, k, v, heads, d, variant=variant)
    close(out, attention_ref.IMPLS["SPLIT_EINSUM_V2"](*f32(q, k, v), heads, d), f"{line} {shape}")
    PASSED.append(line)


# ------------------------------------------------------------------ coverage: asserted, not assumed
COVERAGE = [  # every form a launcher can choose, as a pattern over the query's line
    r"attn_i8 w4", r"attn_i8 w8",
    r"attn8 w4 classic", r"attn8 w8 classic", r"attn8 w4 balanced upw=\d+ seg=\d+", r"attn8 w8 balanced upw=\d+ seg=\d+",
    r"attn d\d+ split w4 qt1", r"attn d\d+ split w8 qt1", r"attn d\d+ split w8 qt2", r"attn d\d+ original w4 qt1",
]
COVERAGE_CASES = {   # one representative per form, run here when the tests above were deselected
    r"attn8 w4 classic": lambda: test_attention8_eight_waves_against_oracle_general_kernel_and_four_waves("ORIGINAL", CLASSIC[0]),
    r"attn8 w8 classic": lambda: test_attention8_eight_waves_against_oracle_general_kernel_and_four_waves("ORIGINAL", CLASSIC[0]),
    r"attn d\d+ split w4 qt1": lambda: test_attention8_eight_waves_against_oracle_general_kernel_and_four_waves("SPLIT_EINSUM", CLASSIC[0]),
    r"attn d\d+ original w4 qt1": lambda: test_attention8_eight_waves_against_oracle_general_kernel_and_four_waves("ORIGINAL", CLASSIC[0]),
    r"attn8 w4 balanced upw=\d+ seg=\d+": lambda: test_attention8_balanced_form_eight_waves(*BALANCED[4]),
    r"attn8 w8 balanced upw=\d+ seg=\d+": lambda: test_attention8_balanced_form_eight_waves(*BALANCED[0]),
    r"attn d\d+ split w8 qt1": lambda: test_split_einsum_v2_eight_wave_forms(*V2[4]),
    r"attn d\d+ split w8 qt2": lambda: test_split_einsum_v2_eight_wave_forms(*V2[2]),
}


@gpu
def test_every_attention_form_was_reached_by_a_passing_case():
    """Over the lines the query REPORTED for launches whose results passed their gates, here and in test_w8a8_einsum_gpu.py (the int8
    kernel's cases; this module runs first, so one four- and one eight-wave case of that file run from here when it has none yet).
    Must stay the last GPU test of the file."""
    import test_w8a8_einsum_gpu as einsum
    for form in COVERAGE:
        seen = PASSED + einsum.PASSED_FORMS
        if not any(re.fullmatch(form, line) for line in seen):
            if form.startswith("attn_i8"):
                einsum.test_operator_against_the_restatement(einsum.SHAPES[0] if form.endswith("w4") else einsum.W8_SHAPES[0])
            else:
                COVERAGE_CASES[form]()
        n = sum(1 for line in PASSED + einsum.PASSED_FORMS if re.fullmatch(form, line))
        print(f"coverage: {form}: {n} passing launches")
        assert n >= 1, f"no passing launch reached: {form}"
