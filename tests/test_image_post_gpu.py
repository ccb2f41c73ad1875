"""GPU suite of the device image post-processing: the two kernels of csrc/imgpost.hip as operators against the numpy restatement
(tests/image_post_ref.py, itself pinned against Pillow and transformers in tests/test_image_post.py), sd_vae_decode_images against
the host route it replaces (sd_vae_decode -> numpy_to_pil -> CLIPImageProcessor -> sd_safety_checker_run), and the pipeline with
and without ``device_postprocess``.  Everything is compared bit for bit: there is no tolerance in this file."""
import ctypes as C
import os

import numpy as np
import pytest

import image_post_ref as R
from oracle import vae_ref, weights
from python_hip_stable_diffusion import HipSafetyChecker, HipVaeDecoder, _lib, pipeline as P, safety_checker as sc
from test_safety_checker import CONFIGS, make_checkpoint
from test_safety_checker_gpu import _add_safety_checker, _close

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ image_rgb8 operator
def _numpy_rgb8(image):
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.clip(image / 2 + 0.5, 0, 1) * 255).round().astype("uint8").transpose(0, 2, 3, 1)


@pytest.mark.parametrize("shape", [(2, 3, 8, 4), (2, 3, 8, 7), (2, 3, 8, 64), (1, 3, 3, 7)], ids=lambda s: "x".join(map(str, s)))
def test_image_rgb8_equals_numpy_on_the_tie_sweep(shape):
    """(1, 3, 3, 7): 21 pixels per plane, no multiple of 4 - the planes do not start on 16-byte boundaries, the one-pixel-per-lane form."""
    sweep = R.tie_sweep()
    image = np.resize(np.roll(sweep, -37 * shape[3]), shape).astype(np.float32)
    got, _ = _lib.image_rgb8(image)
    want = _numpy_rgb8(image)
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want), f"{(got != want).sum()} bytes differ"
    if image.size >= sweep.size:
        v = np.clip(image / 2 + 0.5, 0, 1) * 255
        assert (v - np.floor(v) == 0.5).sum() >= 255, "the image holds the sweep's exact ties"


def test_image_rgb8_equals_numpy_on_noise():
    image = (weights.seeded_normal((2, 3, 128, 128), 31) * 0.8).astype(np.float32)
    got, _ = _lib.image_rgb8(image)
    want = _numpy_rgb8(image)
    assert np.array_equal(got, want), f"{(got != want).sum()} bytes differ"
    assert got.min() == 0 and got.max() == 255
    again, _ = _lib.image_rgb8(image)
    assert np.array_equal(got, again), "two runs differ"


# ------------------------------------------------------------------------------------------------ clip_input operator
CLIP_CASES = {      # B, (H, W), (rh, rw), S
    "down": (1, (128, 128), (56, 56), 56),
    "up": (1, (32, 32), (56, 56), 56),
    "nonsquare-down-wide": (1, (64, 96), (56, 84), 56),
    "nonsquare-down-tall": (1, (96, 64), (84, 56), 56),
    "identity": (1, (56, 56), (56, 56), 56),
    "ragged": (1, (200, 296), (224, 331), 224),
    "real-shape": (2, (512, 512), (224, 224), 224),
}
_clip_reference = {}


def _clip_case(case, kind):
    """input and restatement of one case, computed once"""
    if (case, kind) not in _clip_reference:
        B, (H, W), (rh, rw), S = CLIP_CASES[case]
        rgb = np.stack([R.contents(kind, H, W, seed=b) for b in range(B)])
        ref = R.clip_input(rgb, rh, rw, S)
        rgb.setflags(write=False), ref.setflags(write=False)
        _clip_reference[(case, kind)] = (rgb, ref)
    return _clip_reference[(case, kind)]


@pytest.mark.parametrize("kind", ["noise", "ramp", "checker"])
@pytest.mark.parametrize("case", list(CLIP_CASES))
def test_clip_input_equals_the_restatement_bit_for_bit(case, kind):
    B, (H, W), (rh, rw), S = CLIP_CASES[case]
    rgb, ref = _clip_case(case, kind)
    n, guard = B * 3 * S * S, 4096
    buf = np.full(n + guard, np.nan, np.float16)                    # output and the guard behind it start as NaN
    got, _ = _lib.clip_input(rgb, rh, rw, S, R.CLIP_MEAN, R.CLIP_STD, out=buf)
    assert got.shape == ref.shape == (B, 3, S, S) and np.shares_memory(got, buf)
    assert not np.isnan(got).any(), "an output element was left unwritten"
    assert np.isnan(buf[n:]).all(), "the result ran past the B * 3 * S * S outputs"
    diff = got.view(np.uint16) != ref.view(np.uint16)
    assert not diff.any(), f"{diff.sum()} of {n} fp16 bit patterns differ, first at {np.argwhere(diff)[0]}"
    again, _ = _lib.clip_input(rgb, rh, rw, S, R.CLIP_MEAN, R.CLIP_STD)
    assert np.array_equal(got.view(np.uint16), again.view(np.uint16)), "two runs differ"


# ------------------------------------------------------------------------------------------------ sd_vae_decode_images
VCFG = dict(latent_channels=4, out_channels=3, block_out_channels=(64, 64), layers_per_block=1)      # two levels: image = 2 x latent
CCFG = CONFIGS["mini"]                                                                                 # S = 56


def _feature_extractor(size=56):
    from transformers import CLIPImageProcessor
    return CLIPImageProcessor(size={"shortest_edge": size}, crop_size={"height": size, "width": size}, image_mean=list(R.CLIP_MEAN),
                              image_std=list(R.CLIP_STD))


def _checkpoint(concept_w, special_w=2.0):
    """the mini checker's weights with the thresholds spelled out: score = cosine - threshold, so 2 never fires and -2 always does"""
    sd16 = make_checkpoint(CCFG, seed=13)
    sd16["concept_embeds_weights"] = np.broadcast_to(np.asarray(concept_w, np.float16), sd16["concept_embeds_weights"].shape).copy()
    sd16["special_care_embeds_weights"] = np.full_like(sd16["special_care_embeds_weights"], special_w)
    return sd16


@pytest.fixture(scope="module")
def vae_weights():
    """Seeded weights of the two-level decoder.  With them its image stays within about +-0.2 of zero (8-bit values 104 .. 140), so
    conv_out - the last, linear layer - is scaled by 16 (a power of two: exact in fp16): the images then span the 8-bit range and
    reach both clamps."""
    sd16 = weights.make_state_dict(vae_ref.vae_decoder_param_shapes(VCFG), seed=61, dtype=np.float16, gain=1.6)
    for k in ("decoder.conv_out.weight", "decoder.conv_out.bias"):
        sd16[k] = (sd16[k].astype(np.float32) * 16).astype(np.float16)
    return sd16


def _host_route(vae, chk, fe, z):
    """what the pipeline does without device_postprocess (pipeline.py:286-320): image, 8-bit image, verdicts"""
    image = vae(z=z)["image"]
    image01 = np.clip(image / 2 + 0.5, 0, 1).transpose(0, 2, 3, 1)
    pil = P.HipStableDiffusionPipeline.numpy_to_pil(image01)
    rgb8 = np.stack([np.asarray(p) for p in pil])
    clip_input = fe(pil, return_tensors="np").pixel_values.astype(np.float16)
    cb = chk.batch
    runs = [chk.run(np.ascontiguousarray(clip_input[i:i + cb])) for i in range(0, len(pil), cb)]
    return image, rgb8, np.concatenate([r[0] for r in runs]), np.concatenate([r[1] for r in runs])


@pytest.mark.parametrize("case", ["16x16-b1", "16x16-b2-slices", "16x16-b2", "8x12-f32"])
def test_decode_images_equals_the_host_route(case, vae_weights):
    lat, B, cb, dtype = {"16x16-b1": ((16, 16), 1, 1, np.float16), "16x16-b2-slices": ((16, 16), 2, 1, np.float16),
                         "16x16-b2": ((16, 16), 2, 2, np.float16), "8x12-f32": ((8, 12), 1, 1, np.float32)}[case]
    vae = HipVaeDecoder(VCFG, vae_weights, batch=B, latent_height=lat[0], latent_width=lat[1], dtype=dtype)
    H, W = 2 * lat[0], 2 * lat[1]
    assert vae.image_shape == (B, 3, H, W)
    fe = _feature_extractor()
    post = sc.image_post(fe, H, W, 56)
    assert (post.resize_h, post.resize_w) == (56, 56 * W // H)
    z = (weights.seeded_normal((B, 4) + lat, 77) * 1.5).astype(dtype)
    chk = HipSafetyChecker(CCFG, _checkpoint(2.0), batch=cb)
    image, rgb8, flags, scores = _host_route(vae, chk, fe, z)
    assert rgb8.min() < 64 and rgb8.max() > 192, "the test's own premise: the image spans the 8-bit range"
    assert np.array_equal(rgb8, _numpy_rgb8(image)) and not flags.any()

    out = vae.decode_images(z, chk, post)
    assert np.array_equal(out["image"].view(np.uint32), image.view(np.uint32)), "image differs from sd_vae_decode's"
    assert np.array_equal(out["rgb8"], rgb8), f"{(out['rgb8'] != rgb8).sum()} bytes of rgb8 differ from numpy_to_pil's"
    assert out["has_nsfw_concepts"].dtype == bool and list(out["has_nsfw_concepts"]) == list(flags)
    assert np.array_equal(out["concept_scores"].view(np.uint32), scores.view(np.uint32)), "concept_scores differ from the host route's"

    # every NULL combination
    only_image = vae.decode_images(z)
    assert only_image["has_nsfw_concepts"] is None and only_image["concept_scores"] is None
    assert np.array_equal(only_image["image"], image) and np.array_equal(only_image["rgb8"], rgb8)
    assert np.array_equal(vae.decode_images(z, want_rgb8=False)["image"], image)
    assert np.array_equal(vae.decode_images(z, want_image=False)["rgb8"], rgb8)
    verdict_only = vae.decode_images(z, chk, post, want_image=False, want_rgb8=False)
    assert verdict_only["image"] is None and verdict_only["rgb8"] is None
    assert np.array_equal(verdict_only["concept_scores"], scores)
    nothing = vae.decode_images(z, want_image=False, want_rgb8=False)
    assert nothing == {"image": None, "rgb8": None, "has_nsfw_concepts": None, "concept_scores": None}
    _lib.check(_lib.lib().sd_vae_decode_images(vae._h, _lib.ptr(z), int(dtype == np.float32), None, None, chk._h, C.byref(post), 0.0, None,
                                               None, 0))                 # a checker whose verdict nobody reads
    chk.close()

    # flagged images come back zero in both outputs: all of them, then (batch 2) exactly the one the verdict names
    cos = scores + 2.0
    always = HipSafetyChecker(CCFG, _checkpoint(-2.0), batch=cb)
    out = vae.decode_images(z, always, post)
    assert out["has_nsfw_concepts"].all() and not out["image"].any() and not out["rgb8"].any()
    always.close()
    if B == 2:
        c = int(np.abs(cos[0] - cos[1]).argmax())
        w = np.full(cos.shape[1], 2.0)
        w[c] = np.float16((cos[0, c] + cos[1, c]) / 2)
        assert min(abs(cos[0, c] - w[c]), abs(cos[1, c] - w[c])) > 1e-4, "the test's own premise: a threshold between the two images"
        mixed = HipSafetyChecker(CCFG, _checkpoint(w), batch=cb)
        want_flags = [bool(cos[0, c] > w[c]), bool(cos[1, c] > w[c])]
        assert sorted(want_flags) == [False, True]
        out = vae.decode_images(z, mixed, post)
        assert list(out["has_nsfw_concepts"]) == want_flags
        for b in range(2):
            if want_flags[b]:
                assert not out["image"][b].any() and not out["rgb8"][b].any()
            else:
                assert np.array_equal(out["image"][b], image[b]) and np.array_equal(out["rgb8"][b], rgb8[b])
        mixed.close()
    vae.close()


def test_decode_images_refuses_before_any_device_work(vae_weights):
    """A refused call must not have run the decoder: a fresh handle still answers time_forward with "forward once first"."""
    vae = HipVaeDecoder(VCFG, vae_weights, batch=1, latent_height=16, latent_width=16)
    fe = _feature_extractor()
    post = sc.image_post(fe, 32, 32, 56)
    z = weights.seeded_normal((1, 4, 16, 16), 78).astype(np.float16)
    pair = HipSafetyChecker(CCFG, _checkpoint(2.0), batch=2)
    with pytest.raises(ValueError, match="no multiple"):
        vae.decode_images(z, pair, post)
    pair.close()
    one = HipSafetyChecker(CCFG, _checkpoint(2.0), batch=1)
    with pytest.raises(ValueError, match="image_post"):
        vae.decode_images(z, one)
    rc = _lib.lib().sd_vae_decode_images(vae._h, _lib.ptr(z), 0, None, None, one._h, None, 0.0, None, None, 0)
    assert rc == -1 and b"sd_image_post" in _lib.lib().sd_last_error()
    small = _lib.ImagePost()
    small.resize_h, small.resize_w = 56, 40
    small.image_mean[:], small.image_std[:] = list(post.image_mean), list(post.image_std)
    with pytest.raises(ValueError, match="smaller than"):
        vae.decode_images(z, one, small)
    with pytest.raises(ValueError, match="flags"):
        _lib.check(_lib.lib().sd_vae_decode_images(vae._h, _lib.ptr(z), 0, None, None, None, None, 0.0, None, None, 6))
    if _lib.lib().sd_device_count() >= 2:                               # handles on two devices (boxes with one GPU cannot ask this)
        far = HipSafetyChecker(CCFG, _checkpoint(2.0), batch=1, device=1)
        with pytest.raises(ValueError, match="device"):
            vae.decode_images(z, far, post)
        far.close()
    with pytest.raises(ValueError, match="once first"):
        vae.time_forward()
    assert vae.decode_images(z, one, post)["rgb8"].any()               # and the handles are fine
    one.close(), vae.close()


# ------------------------------------------------------------------------------------------------ pipeline
def test_pipeline_with_and_without_device_postprocess_is_identical(tmp_path):
    from test_text_encoder_gpu import write_checkpoint_dir
    root = str(tmp_path / "mini-sd")
    os.makedirs(root)
    write_checkpoint_dir(root)
    run = dict(num_inference_steps=3, guidance_scale=7.5, negative_prompt="blurry", seed=93)
    prompt = "a photo of an astronaut riding a horse"

    def generate(concept_w, device):
        _add_safety_checker(root, CCFG, _checkpoint(concept_w))
        pipe = P.get_hip_pipe(root, "mini/stable-diffusion", attention_implementation="ORIGINAL", device_postprocess=device)
        assert pipe.device_postprocess is device and (pipe._image_post is not None) is device
        previews = []

        def handler(p):
            previews.append((p.step, p.current_images))
            return True

        as_np = pipe(prompt, progress_handler=handler, progress_steps=2, **run)
        as_pil = pipe(prompt, output_type="pil", **run)
        _close(pipe)
        return as_np, as_pil, previews

    for concept_w, flagged in ((2.0, False), (-2.0, True)):
        host_np, host_pil, host_previews = generate(concept_w, False)
        dev_np, dev_pil, dev_previews = generate(concept_w, True)
        assert host_np.images.shape == (1, 128, 128, 3) and host_np.images.dtype == dev_np.images.dtype
        assert np.array_equal(dev_np.images, host_np.images), "np images differ"
        assert list(dev_np.nsfw_content_detected) == list(host_np.nsfw_content_detected) == [flagged]
        assert list(dev_pil.nsfw_content_detected) == [flagged]
        assert len(dev_pil.images) == len(host_pil.images) == 1
        assert np.array_equal(np.asarray(dev_pil.images[0]), np.asarray(host_pil.images[0])), "PIL images differ"
        assert host_np.images.any() != flagged and np.asarray(dev_pil.images[0]).any() != flagged, "flagged images are black, others not"
        assert [s for s, _ in dev_previews] == [s for s, _ in host_previews] == [0, 2]
        for (_, a), (_, b) in zip(dev_previews, host_previews):
            assert np.array_equal(a, b), "a progress handler's current_images differ"
