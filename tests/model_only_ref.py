"""Float64 references and comparators of the operator tests in test_model_only_kernels.py (CPU: the comparators reject the
mutants) and test_model_only_kernels_gpu.py (GPU: the kernels pass them).  Every reference takes the inputs as the library takes
them - already rounded to the type that crosses the ABI - and computes in float64; every bound is derived from the number formats
and the operation count, never from what a kernel returned.

u = 2^-24 is the unit roundoff of fp32, 2^-11 that of fp16."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
U16 = 2.0 ** -11
TINY32 = 2.0 ** -126          # smallest normal fp32: what one operation can lose to underflow


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def silu64(v):
    v = np.asarray(v, np.float64)
    with np.errstate(over="ignore"):
        return v / (1.0 + np.exp(-v))


# ----------------------------------------------------------------------------------------------- conv_f32
def conv_out_size(h, w, k, stride, up, pad_mode):
    extra = 1 if pad_mode else 2 * (k // 2)
    return (h * up + extra - k) // stride + 1, (w * up + extra - k) // stride + 1


def conv_weight_oihw(w, w_kind):
    """The weight as (N, Cin, k, k) float64: kind 0 rounds to fp16 first (what crosses the ABI), kind 2 is stored (K, N)."""
    if w_kind == 0:
        return t64(np.asarray(w, np.float32).astype(np.float16))
    if w_kind == 2:
        return t64(np.asarray(w, np.float32).T)[:, :, None, None]
    return t64(np.asarray(w, np.float32))


def conv_ref(x, w, bias, res, stride, up, pad_mode, w_kind, absolute=False, mutant=None):
    """out = conv(nearest_up(x), w) + bias + res in float64 (B, N, Ho, Wo).  absolute: the same sum over absolute values, the
    magnitude the running-error bound scales with.  mutant: "edge_clamp" pads with the border pixel instead of zeros,
    "up_shift" reads upsampled pixel (y + 1) >> 1, (x + 1) >> 1, "drop_tap" leaves the centre tap out at output pixel (0, 0)."""
    xt, wt = t64(x), conv_weight_oihw(w, w_kind)
    k = wt.shape[2]
    if absolute:
        xt, wt = xt.abs(), wt.abs()
    if up == 2:
        if mutant == "up_shift":
            iy = torch.clamp((torch.arange(2 * xt.shape[2]) + 1) >> 1, max=xt.shape[2] - 1)
            ix = torch.clamp((torch.arange(2 * xt.shape[3]) + 1) >> 1, max=xt.shape[3] - 1)
            xt = xt[:, :, iy][:, :, :, ix]
        else:
            xt = F.interpolate(xt, scale_factor=2, mode="nearest")
    pads = (0, 1, 0, 1) if pad_mode else (k // 2,) * 4
    xt = F.pad(xt, pads, mode="replicate" if mutant == "edge_clamp" else "constant")
    out = F.conv2d(xt, wt, stride=stride)
    if mutant == "drop_tap":   # output pixel (0, 0) reads padded pixel (k // 2, k // 2) through the centre tap
        c = k // 2
        out[:, :, 0, 0] -= torch.einsum("nc,bc->bn", wt[:, :, c, c], xt[:, :, c, c])
    if bias is not None:
        b = t64(bias)
        out = out + (b.abs() if absolute else b)[None, :, None, None]
    if res is not None:
        r = t64(res)
        out = out + (r.abs() if absolute else r)
    return out.numpy()


def conv_close(got, ref, mag, K, what):
    """|got - ref| <= (K + 2) u mag + (K + 2) 2^-126 elementwise: the running-error bound of K fp32 FMAs in any order plus the
    epilogue's two adds (Higham, Accuracy and Stability, section 3.1: |fl(sum) - sum| <= gamma_n sum |terms| for every order), mag the same
    sum over absolute values; the second term is what K + 2 operations can lose to underflow."""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    bound = (K + 2) * U32 * mag + (K + 2) * TINY32
    err = np.abs(got - ref)
    worst = float((err / bound).max())
    print(f"{what}: max |err| / bound = {worst:.3f} (max|err| {err.max():.3e}, max|ref| {np.abs(ref).max():.3e})")
    assert worst <= 1.0, f"{what}: |err| reaches {worst:.2f} x the bound at {np.unravel_index((err / bound).argmax(), err.shape)}"


# ----------------------------------------------------------------------------------------------- groupnorm_f32
def groupnorm_ref(x, gamma, beta, groups, eps, silu, mutant=None):
    """(out, bound) in float64.  v = (x - mean) * rstd * gamma + beta with the biased variance of each (sample, group).

    The bound counts roundings: mean and rstd each reach the apply kernel rounded once from fp64 to fp32 (2), then a subtraction,
    two products and an addition (4) - 6 roundings, each at most u relative to a partial result no larger than
    (|x| + |mean|) rstd |gamma| + |beta|; with the factor 2 of slack and rounded up to a power of two: 16 u.  SiLU multiplies an
    input error by at most max |silu'| < 1.1 and adds its own evaluation (expf, one add, one division: < 16 u |silu(v)|).
    mutant: "neighbour" normalises group g with the statistics of group g + 1, "unbiased" divides the variance by n - 1."""
    x = np.asarray(x, np.float64)
    B, C, H, W = x.shape
    xg = x.reshape(B, groups, -1)
    n = xg.shape[2]
    mean = xg.mean(axis=2, keepdims=True)
    var = ((xg - mean) ** 2).sum(axis=2, keepdims=True) / (n - 1 if mutant == "unbiased" else n)
    rstd = 1.0 / np.sqrt(var + eps)
    if mutant == "neighbour":
        mean, rstd = np.roll(mean, -1, axis=1), np.roll(rstd, -1, axis=1)
    g = np.asarray(gamma, np.float64).reshape(1, groups, -1, 1)
    b = np.asarray(beta, np.float64).reshape(1, groups, -1, 1)
    xc = x.reshape(B, groups, C // groups, H * W)
    mean, rstd = mean[..., None], rstd[..., None]
    v = (xc - mean) * rstd * g + b
    bound = 16 * U32 * ((np.abs(xc) + np.abs(mean)) * rstd * np.abs(g) + np.abs(b))
    if silu:
        v = silu64(v)
        bound = 1.1 * bound + 16 * U32 * np.abs(v)
    return v.reshape(x.shape), (bound + TINY32).reshape(x.shape)


def bounded_close(got, ref, bound, what):
    """|got - ref| <= bound elementwise, all finite."""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    err = np.abs(got - ref)
    worst = float((err / bound).max())
    print(f"{what}: max |err| / bound = {worst:.3f} (max|err| {err.max():.3e}, max|ref| {np.abs(ref).max():.3e})")
    assert worst <= 1.0, f"{what}: |err| reaches {worst:.2f} x the bound at {np.unravel_index((err / bound).argmax(), err.shape)}"


# ----------------------------------------------------------------------------------------------- row_softmax
def softmax_ref(x, scale, mutant=None):
    """softmax(scale * x) over the last axis in float64; x as it crosses the ABI (fp16 or fp32), scale the fp32 value.
    mutant "max_before_scale": the maximum is taken over x and scaled afterwards - the minimum of the scores when scale < 0 - and
    the exponentials are fp32 like a kernel's, so a row whose scores span more than fp32's exponent range overflows."""
    s = np.asarray(x, np.float64) * float(np.float32(scale))
    if mutant == "max_before_scale":
        m = np.asarray(x, np.float64).max(axis=-1, keepdims=True) * float(np.float32(scale))
        with np.errstate(over="ignore", invalid="ignore"):
            e = np.exp((s - m).astype(np.float32))
            return (e / e.sum(axis=-1, keepdims=True, dtype=np.float32)).astype(np.float64)
    e = np.exp(s - s.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def softmax_close(got, ref, fp32, what):
    """fp16 kernel: |got - ref| <= 2^-10 ref + 2^-24 - one fp16 rounding (2^-11 ref; 2^-24 is the smallest fp16 subnormal) plus an
    equal budget for the fp32 exp2 and the sum.  fp32 kernel: 64 u ref + 1e-38.  Every row sums to 1 within cols 2^-11 (cols 2^-23)."""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    bound = 64 * U32 * ref + 1e-38 if fp32 else 2.0 ** -10 * ref + 2.0 ** -24
    err = np.abs(got - ref)
    worst = float((err / bound).max())
    cols = ref.shape[-1]
    sum_err = float(np.abs(got.sum(axis=-1) - 1.0).max())
    sum_bound = cols * (2.0 ** -23 if fp32 else 2.0 ** -11)
    print(f"{what}: max |err| / bound = {worst:.3f}, max |row sum - 1| = {sum_err:.3e} (bound {sum_bound:.3e})")
    assert worst <= 1.0, f"{what}: |err| reaches {worst:.2f} x the bound at {np.unravel_index((err / bound).argmax(), err.shape)}"
    assert sum_err <= sum_bound, f"{what}: a row sums to 1 +- {sum_err:.3e} (bound {sum_bound:.3e})"


# ----------------------------------------------------------------------------------------------- gemv
def gemv_ref(w, bias, x, init, silu_in, silu_out, mutant=None):
    """(out, bound) in float64: out = act_out(act_in(x) @ w.T + bias) + init.

    Bound (K + 16) u (sum_k |w| |act(x)| + |bias| + |init|): K FMAs and adds in any order, and 16 for the SiLU of the input - the
    hardware exp2 and rcp at 1 ulp each, the rounding of its argument and of the product at |x| <= 4 - and the epilogue's adds.
    With silu_out the part in front of the SiLU passes through |silu'| < 1.1 and the SiLU's own evaluation adds 16 u |silu(v)|.
    mutant: "drop_chunk" leaves columns [8, 16) (K = 8: [0, 8)) out, "no_bias" skips the bias, "swap_rows" swaps batch rows 0 and 1."""
    w = np.asarray(w, np.float64)
    x = np.asarray(x, np.float64)
    N, K = w.shape
    a = silu64(x) if silu_in else x
    if mutant == "swap_rows":
        a = a[[1, 0] + list(range(2, a.shape[0]))]
    if mutant == "drop_chunk":
        a = a.copy()
        a[:, (8 if K > 8 else 0):(16 if K > 8 else 8)] = 0.0
    b = np.zeros(N) if bias is None or mutant == "no_bias" else np.asarray(bias, np.float64)
    v = a @ w.T + b
    bound = (K + 16) * U32 * (np.abs(a) @ np.abs(w).T + np.abs(b))
    if silu_out:
        v = silu64(v)
        bound = 1.1 * bound + 16 * U32 * np.abs(v)
    if init is not None:
        i = np.asarray(init, np.float64)
        v = v + i
        bound = bound + (K + 16) * U32 * np.abs(i)
    return v, bound + TINY32


# ----------------------------------------------------------------------------------------------- clip_attention
def clip_attention_ref(qkv, heads, mutant=None):
    """(out, bound) in float64 from qkv (S, 3 D) fp16: per head softmax(q k^T d^-0.5 + causal mask) v.

    Bound of row i, column c: (2^-11 + 2 (d + 4) u max_{j<=i} sum_c' |q_c' k_jc'| d^-0.5) max_{j<=i} |v_jc| + 2^-24.  The output is a
    convex combination of the v_jc, so the fp16 rounding of the result is at most 2^-11 max_j |v_jc|; a score carries the
    running error of d products and adds plus the scale and the subtraction of the maximum ((d + 4) u of its magnitude), which
    the exponential turns into that relative error of a weight, and numerator and denominator both carry it (factor 2).
    mutant: "strict" masks j < i only (row 0 sees nothing and is zero), "ahead" lets row i see key i + 1."""
    qkv = np.asarray(qkv, np.float64)
    S, D3 = qkv.shape
    D = D3 // 3
    d = D // heads
    out, bound = np.zeros((S, D)), np.zeros((S, D))
    off = {None: 0, "strict": -1, "ahead": 1}[mutant]
    for h in range(heads):
        q, k, v = (qkv[:, i * D + h * d:i * D + (h + 1) * d] for i in range(3))
        s = q @ k.T * d ** -0.5
        smag = np.abs(q) @ np.abs(k).T * d ** -0.5
        for i in range(S):
            hi = min(max(i + 1 + off, 0), S)
            if hi == 0:
                continue
            e = np.exp(s[i, :hi] - s[i, :hi].max())
            out[i, h * d:(h + 1) * d] = (e / e.sum()) @ v[:hi]
            vmax = np.abs(v[:i + 1]).max(axis=0)
            bound[i, h * d:(h + 1) * d] = (U16 + 2 * (d + 4) * U32 * smag[i, :i + 1].max()) * vmax + 2.0 ** -24
    return out, bound


# ----------------------------------------------------------------------------------------------- clip_act
def clip_act_ref(x, act):
    """quick_gelu x sigmoid(1.702 x) / exact-erf gelu x Phi(x) in float64 (Phi through erfc: no cancellation in the tail)."""
    x = np.asarray(x, np.float64)
    if act == "quick_gelu":
        with np.errstate(over="ignore"):
            return x / (1.0 + np.exp(-1.702 * x))
    return 0.5 * x * torch.erfc(t64(-x / np.sqrt(2.0))).numpy()


def clip_act_close(got, ref, what):
    """|got - ref| <= 2^-10 |ref| + 2^-24: one fp16 rounding (2^-11 |ref|, 2^-25 in the subnormal range) and as much again for the
    fp32 evaluation."""
    bounded_close(got, ref, 2.0 ** -10 * np.abs(ref) + 2.0 ** -24, what)


# ----------------------------------------------------------------------------------------------- the project's operator bar
def close(got, ref, what, min_psnr=60.0, rel=4e-3):
    """tests/test_ops_gpu.py's `close`: PSNR >= 60 dB and max |err| <= 4e-3 max|ref| + 1e-3."""
    from oracle import psnr
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    p = psnr.compute_psnr(got, ref)
    err = np.abs(got - ref).max()
    bound = rel * np.abs(ref).max() + 1e-3
    assert p >= min_psnr and err <= bound, f"{what}: PSNR {p:.1f} dB, max|err| {err:.3e} (bound {bound:.3e})"


# ----------------------------------------------------------------------------------------------- shared inputs
# conv cases (B, Cin, H, W, N, k, stride, up, pad_mode, w_kind); up is the factor of the nearest upsample in front (1 or 2)
CONV_CASES = [
    (1, 4, 5, 7, 3, 3, 1, 1, 0, 0),      # K = 36, M = 35, N = 3: every tile ragged
    (1, 4, 5, 7, 3, 3, 1, 1, 0, 1),
    (2, 8, 9, 11, 70, 3, 2, 1, 0, 1),    # two n-blocks, the second ragged; one m-block spanning both images
    (2, 8, 9, 11, 70, 3, 2, 1, 1, 1),    # ... with the encoder's (0,1,0,1) padding
    (2, 8, 8, 10, 70, 3, 2, 1, 1, 1),    # ... at an even image, where the last output row and column read the padding (at 9x11 none does)
    (2, 16, 4, 3, 64, 3, 1, 2, 0, 0),    # the upsample gather, M = 96
    (1, 16, 1, 65, 65, 1, 1, 1, 0, 1),   # K = 16 is a single K step; one live row and one live column in the second blocks
    (1, 17, 3, 3, 8, 1, 1, 1, 0, 1),     # K = 17
    (1, 24, 1, 70, 70, 1, 1, 1, 0, 1),   # attention q k^T: 70 tokens of width 24 against 70 keys [N][K]
    (1, 70, 1, 70, 24, 1, 1, 1, 0, 2),   # attention p v: V stored [K][N], N = 24
    (1, 70, 1, 70, 100, 1, 1, 1, 0, 2),  # ... N = 100: two n-blocks of the [K][N] loader
]


@functools.lru_cache(maxsize=None)
def conv_inputs(case, magnitude=1.0):
    """x, w (in the layout of its kind), bias, res of one case, float32 (kind 0: w fp16-representable); built once, never modified."""
    B, Cin, H, W, N, k, stride, up, pad_mode, w_kind = case
    rs = np.random.RandomState(hash(case) % (2 ** 31))
    ho, wo = conv_out_size(H, W, k, stride, up, pad_mode)
    x = (magnitude * rs.randn(B, Cin, H, W)).astype(np.float32)
    w = (rs.randn(N, Cin, k, k) / np.sqrt(Cin * k * k)).astype(np.float32)
    if w_kind == 0:
        w = w.astype(np.float16).astype(np.float32)
    if w_kind == 2:
        w = np.ascontiguousarray(w[:, :, 0, 0].T)
    bias = (magnitude * rs.randn(N)).astype(np.float32)
    res = (magnitude * rs.randn(B, N, ho, wo)).astype(np.float32)
    for a in (x, w, bias, res):
        a.setflags(write=False)
    return x, w, bias, res


GN_CASES = [   # (B, C, H, W, G, offset of the group means, magnitude)
    (1, 32, 2, 3, 32, 0.0, 1.0),        # HW = 6, one slab, one channel per group
    (2, 64, 8, 8, 32, 0.0, 1.0),
    (1, 96, 10, 13, 32, 0.0, 1.0),      # HW = 130: two slabs of 65, three channels per group
    (1, 32, 65, 64, 8, 0.0, 1.0),       # HW = 4160: 64 slabs of 65
    (2, 64, 9, 9, 32, 1.0e3, 1.0),      # group means near 1e3 at unit spread
    (2, 64, 8, 8, 32, 0.0, 1.0e6),      # magnitude 1e6
]


@functools.lru_cache(maxsize=None)
def gn_inputs(case):
    B, C, H, W, G, offset, magnitude = case
    rs = np.random.RandomState(hash(case) % (2 ** 31))
    x = rs.randn(B, C, H, W)
    if offset:
        x = x + offset * (1.0 + 0.1 * rs.randn(B, G, 1, 1)).repeat(C // G, axis=1)
    x = (magnitude * x).astype(np.float32)
    gamma = (1.0 + 0.3 * rs.randn(C)).astype(np.float32)
    beta = (0.2 * rs.randn(C)).astype(np.float32)
    for a in (x, gamma, beta):
        a.setflags(write=False)
    return x, gamma, beta


def softmax_rows(cols, fp32):
    """(x (rows, cols), scale) pairs of one width, in the type that crosses the ABI."""
    rs = np.random.RandomState(cols + 7 * int(fp32))
    dt = np.float32 if fp32 else np.float16
    dom = np.full((3, cols), -30.0)
    dom[np.arange(3), rs.randint(0, cols, 3)] = 30.0          # e^-60 = 9e-27: zero in fp16, a normal number in fp32
    wide = rs.choice([-6.0e4, 6.0e4], size=(3, cols)) * (1.0 - 2.0 ** -8 * rs.rand(3, cols))   # fp16 inputs near +-6e4
    wide[:, 0] = 6.0e4
    rows = [("random", (3.0 * rs.randn(3, cols)).astype(dt), 0.37),
            ("constant", np.full((3, cols), 1.25, dt), 1.0),
            ("dominant", dom.astype(dt), 1.0),
            ("near +-6e4", wide.astype(np.float16).astype(dt), 512.0 ** -0.5),
            ("near +-6e4, negative scale", wide.astype(np.float16).astype(dt), -(512.0 ** -0.5))]
    if fp32:   # scores of magnitude 1e6 a few units apart; the scale a power of two, so that scale * x is exact in fp32 as it is in
        # the reference (with any other scale the product itself rounds at 0.03: no fp32 evaluation, torch's included, gets closer)
        rows.append(("1e6-scale", (1.0e6 + 8.0 * rs.randn(3, cols)).astype(np.float32), 0.5))
    return rows


def attention_inputs(S, heads, d, score=None):
    """qkv (S, 3 D) fp16; score: q and k scaled so that the largest |q k^T| d^-0.5 is about that."""
    rs = np.random.RandomState(1000 * S + 10 * heads + d)
    qkv = rs.randn(S, 3 * heads * d)
    if score is not None:
        D = heads * d
        q, k = qkv[:, :D].reshape(S, heads, d), qkv[:, D:2 * D].reshape(S, heads, d)
        peak = np.abs(np.einsum("ihc,jhc->hij", q, k)).max() * d ** -0.5
        qkv[:, :2 * D] *= np.sqrt(score / peak)
    return qkv.astype(np.float16)
