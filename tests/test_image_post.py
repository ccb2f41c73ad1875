"""CPU suite of the device image post-processing (csrc/imgpost.hip behind sd_vae_decode_images): the numpy restatement
(tests/image_post_ref.py) against the authorities it restates - Pillow's 8-bit bicubic resize and transformers' CLIPImageProcessor,
bit for bit - the library's host-side coefficient tables against the restatement, the quantisation against the numpy expression of
``numpy_to_pil``, the refusals of ``safety_checker.image_post``, the ABI mirrors and the CLI flag.  No test here needs a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import image_post_ref as R
from conftest import ROOT
from python_hip_stable_diffusion import _lib, pipeline as P, safety_checker as sc
from test_build_isa import CSRC, HIPCC, kernel_resources
from test_library_abi import _header_struct_fields

# (H, W) -> (rh, rw) as CLIPImageProcessor resolves {"shortest_edge": 224}; the last one skips both passes
GEOMETRIES = [((512, 512), (224, 224)), ((64, 64), (224, 224)), ((768, 512), (336, 224)), ((72, 40), (403, 224)),
              ((200, 296), (224, 331)), ((224, 224), (224, 224))]
CONTENTS = ("noise", "ramp", "checker")


def _processor(**kw):
    from transformers import CLIPImageProcessor
    cfg = dict(size={"shortest_edge": 224}, crop_size={"height": 224, "width": 224}, image_mean=list(R.CLIP_MEAN),
               image_std=list(R.CLIP_STD))
    cfg.update(kw)
    return CLIPImageProcessor(**cfg)


@pytest.mark.parametrize("geometry", GEOMETRIES, ids=lambda g: "%dx%d-%dx%d" % (g[0] + g[1]))
def test_restatement_equals_pillow_and_clip_image_processor(geometry):
    from PIL import Image
    (H, W), (rh, rw) = geometry
    fe = _processor()
    post = sc.image_post(fe, H, W, 224)
    assert (post.resize_h, post.resize_w) == (rh, rw), "the wrapper resolves the resized size as CLIPImageProcessor does"
    reached = set()
    for kind in CONTENTS:
        im = R.contents(kind, H, W)
        want = np.asarray(Image.fromarray(im).resize((rw, rh), Image.BICUBIC))
        got = R.resize_u8(im, rh, rw)
        assert got.shape == want.shape == (rh, rw, 3)
        assert np.array_equal(got, want), f"{kind}: {(got != want).sum()} resized bytes differ from Pillow's"
        reached |= {int(got.min()), int(got.max())}
        pixel_values = fe([Image.fromarray(im)], return_tensors="np").pixel_values
        top, left = (rh - 224) // 2, (rw - 224) // 2
        crop = got[top:top + 224, left:left + 224].astype(np.float32)
        mine = ((crop / np.float32(255.0) - np.asarray(post.image_mean, np.float32)) / np.asarray(post.image_std, np.float32)).transpose(2, 0, 1)[None]
        assert pixel_values.dtype == np.float32 and pixel_values.shape == mine.shape
        assert np.array_equal(mine.view(np.uint32), pixel_values.view(np.uint32)), f"{kind}: fp32 bit patterns differ from pixel_values"
        assert np.array_equal(R.clip_input(im[None], rh, rw, 224).view(np.uint16), pixel_values.astype(np.float16).view(np.uint16))
    if (H, W) != (rh, rw):
        assert {0, 255} <= reached, "the 0 / 255 content reaches both clamps through the filter's negative lobes"


@pytest.mark.parametrize("sizes", [(512, 224), (64, 224), (128, 56), (96, 84), (331, 224), (224, 224)], ids=lambda s: "%d-%d" % s)
def test_library_coefficient_tables_equal_the_restatement(sdlib, sizes):
    ksize, bounds, coeffs = _lib.resample_coeffs(*sizes)
    want_ksize, want_bounds, want_coeffs = R.resample_coeffs(*sizes)
    assert ksize == want_ksize
    assert np.array_equal(bounds, want_bounds)
    assert np.array_equal(coeffs, want_coeffs), f"{(coeffs != want_coeffs).sum()} coefficients differ"
    assert (bounds[:, 1] <= ksize).all() and (bounds[:, 0] + bounds[:, 1] <= sizes[0]).all()
    assert np.abs(coeffs).max() < 2 ** 23, "uint8 x coefficient fits the 24-bit multiply"
    n = C.c_int(0)                                                       # the size query writes *ksize alone
    _lib.check(sdlib.sd_op_resample_coeffs(sizes[0], sizes[1], C.byref(n), None, None))
    assert n.value == ksize
    with pytest.raises(ValueError):
        _lib.resample_coeffs(0, 5)


def test_quantise_restatement_equals_the_numpy_expression_on_the_tie_sweep():
    x = R.tie_sweep()
    assert x.size == 255 * 7 + 10
    with np.errstate(invalid="ignore", over="ignore"):
        want = (np.clip(x / 2 + 0.5, 0, 1) * 255).round().astype("uint8")
        v = np.clip(x / 2 + 0.5, 0, 1) * 255
    assert np.array_equal(R.quantise(x), want)
    ties = v[v - np.floor(v) == 0.5]
    assert ties.size >= 255, "the sweep holds exact .5 ties"
    assert (np.floor(ties) % 2 == 0).any() and (np.floor(ties) % 2 == 1).any(), "ties that round down and ties that round up"
    assert list(R.quantise(np.array([np.inf, -np.inf, 3e38, -3e38, 1.5, -1.5, 0.0, -0.0], np.float32))) == [255, 0, 255, 0, 255, 0, 128, 128]


def test_image_post_resolves_sizes_and_refuses_what_the_kernels_do_not_express():
    post = sc.image_post(_processor(), 512, 768, 224)
    assert (post.resize_h, post.resize_w) == (224, 336)
    assert np.array_equal(np.asarray(post.image_mean, np.float32), np.asarray(R.CLIP_MEAN, np.float32))
    assert np.array_equal(np.asarray(post.image_std, np.float32), np.asarray(R.CLIP_STD, np.float32))
    post = sc.image_post(_processor(size={"height": 240, "width": 300}), 512, 512, 224)       # explicit sizes: those
    assert (post.resize_h, post.resize_w) == (240, 300)
    post = sc.image_post(_processor(size=56, crop_size=56), 128, 96, 56)                  # legacy integers
    assert (post.resize_h, post.resize_w) == (74, 56)
    for bad, match in ((dict(resample=2), "BICUBIC"), (dict(do_resize=False), "do_resize"), (dict(do_center_crop=False), "do_center_crop"),
                       (dict(do_rescale=False), "do_rescale"), (dict(do_normalize=False), "do_normalize"),
                       (dict(rescale_factor=1 / 256), "1/255"), (dict(size={"height": 200, "width": 300}), "zero-pad"),
                       (dict(size={"height": 300, "width": 200}), "zero-pad"), (dict(crop_size={"height": 112, "width": 112}), "crops to")):
        with pytest.raises(ValueError, match=match):
            sc.image_post(_processor(**bad), 512, 512, 224)


def test_pipeline_refuses_device_postprocess_without_library_handles():
    class Stub:
        expected_inputs = {"sample": {"shape": (2, 4, 8, 8)}, "z": {"shape": (1, 4, 8, 8), "dtype": np.dtype(np.float16)}}

    with pytest.raises(ValueError, match="HipVaeDecoder"):
        P.HipStableDiffusionPipeline(None, Stub(), Stub(), None, None, device_postprocess=True)
    pipe = P.HipStableDiffusionPipeline(None, Stub(), Stub(), None, None)      # off by default: any model runner, as before
    assert pipe.device_postprocess is False


def test_struct_and_symbol_mirrors(sdlib):
    assert [f[0] for f in _lib.ImagePost._fields_] == _header_struct_fields("sd_image_post")
    assert C.sizeof(_lib.ImagePost) == 4 * 8                                   # all members 4 bytes wide: no padding
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for name in ("sd_vae_decode_images", "sd_op_resample_coeffs", "sd_op_image_rgb8", "sd_op_clip_input"):
        assert name in bound and hasattr(sdlib, name), name
    header = open(os.path.join(ROOT, "include", "sd_mi355x.h")).read()
    for cite in ("pipeline.py:286-320", "Decoder.swift:40-68", "SafetyChecker.swift:55-99", "torch2coreml.py:1203-1207"):
        assert cite in header.split("Image post-processing on the device")[1], cite


def test_geometry_is_refused_on_the_host_before_any_device_work(sdlib):
    """The same answers with and without a GPU: the library checks the geometry before it asks for a device."""
    rgb = np.zeros((1, 32, 32, 3), np.uint8)
    with pytest.raises(ValueError, match="smaller than"):
        _lib.clip_input(rgb, 40, 56, 56, R.CLIP_MEAN, R.CLIP_STD)
    with pytest.raises(NotImplementedError, match="odd crop"):
        _lib.clip_input(rgb, 57, 57, 55, R.CLIP_MEAN, R.CLIP_STD)
    with pytest.raises(NotImplementedError, match="LDS"):
        _lib.clip_input(np.zeros((1, 4096, 8, 3), np.uint8), 224, 224, 224, R.CLIP_MEAN, R.CLIP_STD)
    with pytest.raises(ValueError, match="std"):
        _lib.clip_input(rgb, 56, 56, 56, R.CLIP_MEAN, (0.0, 1.0, 1.0))


def test_device_postprocess_flag_parses():
    common = ["--prompt", "a", "-i", "in", "-o", "out"]
    assert P.build_parser().parse_args(common).device_postprocess is False
    assert P.build_parser().parse_args(common + ["--device-postprocess"]).device_postprocess is True


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_imgpost_kernels_compile_for_gfx950_without_scratch(tmp_path):
    res = kernel_resources(os.path.join(CSRC, "imgpost.hip"), tmp_path)
    assert any("image_rgb8_kernel" in k for k in res) and any("clip_input_kernel" in k for k in res), sorted(res)
    spilled = {k: v for k, v in res.items() if v[1] != 0}
    assert not spilled, f"kernels with scratch: {spilled}"
    asm = kernel_resources.last_asm
    assert "v_div_fixup_f32" in asm, "the normalisation divides with IEEE rounding (no fast-math reciprocal)"
    assert "global_store_dwordx3" in asm or asm.count("global_store_dword ") >= 3, "the 8-bit image leaves as dword stores"
