"""The W8A8 self-attention einsums restated in numpy (include/sd_mi355x.h at sd_op_attention_w8a8, steps 1-5): float32 for every
product stated as fp32, ``np.exp2`` on float32, int64 for the integer sums.  Head dim 64."""
import numpy as np

D = 64
LOG2E = np.float64(1.4426950408889634)
MAX_S = 133120
F32 = np.float32


def vt_key(p):
    """position p (0 .. 31) of every 32-key group of the int8 V^T holds this key of the group"""
    return (p & 3) + 8 * ((p >> 2) & 3) + 4 * (p >> 4)


def quantize(x, r_eff):
    """step 1 on float16 values: clip(rint(fp32(x) * fp32(127 / r)), -127, 127), NaN -> 0, +-inf -> +-127"""
    inv = F32(127.0) / F32(r_eff)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.rint(np.asarray(x, np.float16).astype(F32) * inv)
    v = np.where(np.isnan(v), F32(0), np.clip(v, -127, 127))
    return v.astype(np.int8)


def scale(r):
    return F32(r) / F32(127.0)


def score_scale(r_q, r_k):
    """c = fp32(s_q * s_k * d^-0.5 * log2 e): the product formed in float64, rounded once"""
    return F32(((np.float64(scale(r_q)) * np.float64(scale(r_k))) * (1.0 / np.sqrt(np.float64(D)))) * LOG2E)


def probabilities(q_q, k_q, c, exp2=None):
    """steps 2-3 for one head: q_q (S, 64), k_q (S, 64) int8 -> p_q (S, S) int64 in 0 .. 127 (row = query)"""
    s = q_q.astype(np.int64) @ k_q.astype(np.int64).T
    t = s.astype(F32) * F32(c)
    m = t.max(axis=1, keepdims=True)
    x = t - m
    e = np.exp2(x) if exp2 is None else exp2(x)
    return np.rint(F32(127.0) * e.astype(F32)).astype(np.int64)


def attention(q_q, k_q, v_q, r_q, r_k, r_v, batch, heads, exp2=None):
    """q_q, k_q, v_q (batch * S, heads * 64) int8 token-major -> out (batch * S, heads * 64) float16"""
    q_q, k_q, v_q = (np.asarray(a, np.int8) for a in (q_q, k_q, v_q))
    S = q_q.shape[0] // batch
    c, s_v = score_scale(r_q, r_k), scale(r_v)
    out = np.empty(q_q.shape, np.float16)
    for b in range(batch):
        rows = slice(b * S, (b + 1) * S)
        for h in range(heads):
            cols = slice(h * D, (h + 1) * D)
            p = probabilities(q_q[rows, cols], k_q[rows, cols], c, exp2)
            n = p @ v_q[rows, cols].astype(np.int64)
            l = p.sum(axis=1, keepdims=True)
            out[rows, cols] = (n.astype(F32) * (s_v / l.astype(F32))).astype(np.float16)
    return out
