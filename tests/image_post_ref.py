"""numpy restatement of the image post-processing between the VAE decoder and the safety checker: the 8-bit quantisation of
``numpy_to_pil``, Pillow's 8-bit ``Image.resize(..., BICUBIC)`` and CLIPImageProcessor's centre crop / rescale / normalise
(python_coreml_stable_diffusion/pipeline.py:286-320).  The kernels of csrc/imgpost.hip and ``sd_op_resample_coeffs`` are pinned
against this module bit for bit; tests/test_image_post.py pins this module against Pillow and transformers themselves."""
import math

import numpy as np

PRECISION_BITS = 22
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def quantise(x):
    """decoder output in [-1, 1] (any shape, float32) -> uint8, ``(np.clip(x / 2 + 0.5, 0, 1) * 255).round().astype("uint8")`` spelled
    as the kernel computes it: fp32 throughout, the multiply by 255 rounded on its own, round-half-to-even."""
    x = np.asarray(x, np.float32)
    v = np.minimum(np.maximum(x * np.float32(0.5) + np.float32(0.5), np.float32(0)), np.float32(1))
    return np.rint(v * np.float32(255.0)).astype(np.uint8)


def _bicubic(t, a=-0.5):
    t = abs(t)
    if t < 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1
    if t < 2.0:
        return (((t - 5) * t + 8) * t - 4) * a
    return 0.0


def resample_coeffs(in_size, out_size):
    """Pillow's 8-bit bicubic coefficients of one axis: (ksize, bounds (out, 2) int32 = [xmin, n], coeffs (out, ksize) int32, zeros
    behind the n taps of a row).  All in double (Python floats), C truncation for the integer conversions."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    coeffs = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - xmin
        w = [_bicubic((x + xmin - center + 0.5) / fs) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = (xmin, n)
        for x, v in enumerate(w):
            coeffs[xx, x] = int(v * (1 << PRECISION_BITS) - 0.5) if v < 0 else int(v * (1 << PRECISION_BITS) + 0.5)
    return ksize, bounds, coeffs


def _resample_axis0(src, out_size):
    """one pass along axis 0 of a uint8 array (in, ...) -> (out, ...) uint8"""
    in_size = src.shape[0]
    _, bounds, coeffs = resample_coeffs(in_size, out_size)
    out = np.empty((out_size,) + src.shape[1:], np.uint8)
    s = src.astype(np.int64)
    for xx in range(out_size):
        xmin, n = bounds[xx]
        ss = (1 << (PRECISION_BITS - 1)) + np.tensordot(coeffs[xx, :n].astype(np.int64), s[xmin:xmin + n], axes=(0, 0))
        assert np.abs(ss).max() < 2 ** 31, "the int32 accumulation the kernel relies on"
        out[xx] = np.clip(ss >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return out


def resize_u8(image, rh, rw):
    """Pillow's ``Image.fromarray(image).resize((rw, rh), BICUBIC)`` for a (H, W, 3) uint8 array: the horizontal pass, the
    intermediate image rounded to uint8, the vertical pass; a pass whose size does not change is skipped."""
    image = np.asarray(image, np.uint8)
    H, W, _ = image.shape
    if rw != W:
        image = _resample_axis0(image.transpose(1, 0, 2), rw).transpose(1, 0, 2)
    if rh != H:
        image = _resample_axis0(image, rh)
    return np.ascontiguousarray(image)


def clip_input(images, rh, rw, S, mean=CLIP_MEAN, std=CLIP_STD):
    """(B, H, W, 3) uint8 -> the checker's ``clip_input`` (B, 3, S, S) float16: resize to (rh, rw), centre crop to S x S, then
    ``((float)u / 255.0f - mean[c]) / std[c]`` in fp32 with both divisions rounded, then round to fp16."""
    mean, std = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    out = []
    for im in np.asarray(images, np.uint8):
        r = resize_u8(im, rh, rw)
        top, left = (rh - S) // 2, (rw - S) // 2
        c = r[top:top + S, left:left + S].astype(np.float32)
        v = (c / np.float32(255.0) - mean) / std
        assert v.dtype == np.float32
        out.append(v.transpose(2, 0, 1))
    return np.stack(out).astype(np.float16)


def tie_sweep():
    """The inputs of the quantisation test: for every k in 0..254 the fp32 x = 2 (k + 0.5) / 255 - 1 whose image lands on (or beside)
    the tie k + 0.5, its +-1, +-2, +-3 ulp neighbours, and the values +-1, +-1.5, +-0, +-3e38, +-inf."""
    xs = []
    for k in range(255):
        x = np.float32(np.float32(2.0) * (np.float32(k) + np.float32(0.5)) / np.float32(255.0) - np.float32(1.0))
        xs.append(x)
        lo = hi = x
        for _ in range(3):
            lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
            xs += [lo, hi]
    xs += [1.0, -1.0, 1.5, -1.5, 0.0, -0.0, 3e38, -3e38, np.inf, -np.inf]
    return np.array(xs, np.float32)


def contents(kind, H, W, seed=0):
    """Test images (H, W, 3) uint8: "noise", a "ramp" (a different direction per channel), "checker" = 0 / 255 noise, whose
    overshoots through the filter's negative lobes reach both clamps."""
    rs = np.random.RandomState(seed + 1000 * H + W)
    if kind == "noise":
        return rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    if kind == "checker":
        return (rs.randint(0, 2, (H, W, 3)) * 255).astype(np.uint8)
    if kind == "ramp":
        y, x = np.mgrid[0:H, 0:W]
        return np.stack([x * 255 // max(W - 1, 1), y * 255 // max(H - 1, 1), (x + y) * 255 // max(H + W - 2, 1)], axis=-1).astype(np.uint8)
    raise ValueError(kind)
