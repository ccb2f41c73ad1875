"""``HipSafetyChecker`` - diffusers' StableDiffusionSafetyChecker behind the reference's model-runner seam.

Duck-types the ``safety_checker`` ``CoreMLModel`` the pipeline calls (python_coreml_stable_diffusion/pipeline.py:286-311):
``safety_checker(clip_input=, images=, adjustment=)`` returns ``{"filtered_images", "has_nsfw_concepts", "concept_scores"}``
(names fixed at torch2coreml.py:1119-1309).  The CLIP vision tower (ViT-L/14), ``visual_projection`` and the concept head run in
``libsdmi355.so`` (csrc/safety_checker.cpp, csrc/vit.hip).  ``filtered_images`` is made here: the images are host arrays at this
point of the pipeline, and blackening the flagged ones (torch2coreml.py:1203-1207) is a memset.
Pre-processing stays with transformers' CLIPImageProcessor exactly as in the reference (pipeline.py:288-291).
"""
import ctypes as C
import json
import os

import numpy as np

from . import _lib
from ._lib import verify_inputs  # noqa: F401  (this module's name for it)
from .hip_model import Weights

# openai/clip-vit-large-patch14's vision tower: what every Stable Diffusion 1.x safety checker is
VIT_L_14 = dict(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16, image_size=224, patch_size=14,
                projection_dim=768, hidden_act="quick_gelu", layer_norm_eps=1e-5)
NUM_CONCEPTS, NUM_SPECIAL = 17, 3     # concept_embeds / special_care_embeds rows of StableDiffusionSafetyChecker


def vision_config(config):
    """The vision tower's settings from a safety checker's ``config.json`` (``vision_config`` inside a CLIPConfig; a bare
    CLIPVisionConfig is accepted too), missing keys from ViT-L/14; ``projection_dim`` is the CLIPConfig's top-level one."""
    config = dict(config or {})
    vc = dict(VIT_L_14)
    if "projection_dim" in config:
        vc["projection_dim"] = config["projection_dim"]
    src = config.get("vision_config") or {k: v for k, v in config.items() if k in VIT_L_14}
    vc.update({k: v for k, v in dict(src).items() if k in VIT_L_14 and v is not None})
    for k in ("num_concepts", "num_special"):
        if k in config:
            vc[k] = int(config[k])
    return vc


def load_feature_extractor(folder):
    """transformers' CLIPImageProcessor from a checkpoint's ``feature_extractor/preprocessor_config.json`` (pipeline.py:644)."""
    path = os.path.join(folder, "preprocessor_config.json")
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} not found (coreml_model.py:176-178)")
    from transformers import CLIPImageProcessor
    with open(path) as f:
        cfg = json.load(f)
    keys = ("do_resize", "size", "resample", "do_center_crop", "crop_size", "do_rescale", "rescale_factor", "do_normalize",
            "image_mean", "image_std", "do_convert_rgb")
    return CLIPImageProcessor(**{k: cfg[k] for k in keys if k in cfg})


def image_post(feature_extractor, height, width, image_size):
    """``_lib.ImagePost`` for images of ``height`` x ``width`` and a checker of ``image_size``: the size CLIPImageProcessor resizes
    them to (``{"shortest_edge": s}`` or a legacy integer: the short side becomes s, the long side ``int(s * long / short)``;
    ``{"height", "width"}``: those) and the fp32 roundings of its ``image_mean`` / ``image_std``.  A processor the device kernels
    (csrc/imgpost.hip) do not express is refused with ValueError, not worked around: a resample filter other than BICUBIC, any of
    do_resize / do_center_crop / do_rescale / do_normalize off, a rescale factor other than 1 / 255, a crop size other than the
    checker's input, a resized image smaller than the crop (transformers would zero-pad)."""
    fe = feature_extractor
    for flag in ("do_resize", "do_center_crop", "do_rescale", "do_normalize"):
        if not getattr(fe, flag, False):
            raise ValueError(f"device post-processing needs a feature extractor with {flag}=True")
    if int(getattr(fe, "resample", 0) or 0) != 3:
        raise ValueError(f"device post-processing implements PIL's BICUBIC (resample=3), the feature extractor has {fe.resample!r}")
    if float(fe.rescale_factor) != 1 / 255:
        raise ValueError(f"device post-processing rescales by 1/255, the feature extractor by {fe.rescale_factor!r}")

    def size_dict(v):
        if v is None or isinstance(v, (int, np.integer)):
            return v
        return {k: v[k] for k in ("shortest_edge", "height", "width", "longest_edge", "max_height", "max_width") if v.get(k) is not None}

    S = int(image_size)
    crop = size_dict(fe.crop_size)
    if isinstance(crop, (int, np.integer)):
        crop = {"height": int(crop), "width": int(crop)}
    if crop != {"height": S, "width": S}:
        raise ValueError(f"the feature extractor crops to {crop}, the safety checker takes {S}x{S} images")
    size = size_dict(fe.size)
    height, width = int(height), int(width)
    if isinstance(size, (int, np.integer)):
        size = {"shortest_edge": int(size)}
    if set(size) == {"shortest_edge"}:
        s = int(size["shortest_edge"])
        short, long = (width, height) if width <= height else (height, width)
        new_long = int(s * long / short)
        rh, rw = (new_long, s) if width <= height else (s, new_long)
    elif set(size) == {"height", "width"}:
        rh, rw = int(size["height"]), int(size["width"])
    else:
        raise ValueError(f"device post-processing resolves size={{'shortest_edge'}} or {{'height', 'width'}}, the feature extractor has {size}")
    if rh < S or rw < S:
        raise ValueError(f"the feature extractor resizes {height}x{width} images to {rh}x{rw}, smaller than the {S}x{S} crop "
                         "(transformers would zero-pad)")
    mean, std = np.asarray(fe.image_mean, np.float32), np.asarray(fe.image_std, np.float32)
    if mean.shape != (3,) or std.shape != (3,) or not (std != 0).all():
        raise ValueError("device post-processing needs three image_mean and three non-zero image_std values")
    post = _lib.ImagePost()
    post.resize_h, post.resize_w = rh, rw
    post.image_mean[:], post.image_std[:] = [float(v) for v in mean], [float(v) for v in std]
    return post


def blacken(images, has_nsfw):
    """``filtered_images``: a copy of ``images`` (B, H, W, 3) with every flagged image zeroed (torch2coreml.py:1203-1207)."""
    images = np.asarray(images)
    flags = np.asarray(has_nsfw).astype(bool).reshape(-1)
    if flags.shape[0] != images.shape[0]:
        raise ValueError(f"{flags.shape[0]} flags for {images.shape[0]} images")
    out = images.copy()
    out[flags] = 0
    return out


def expected_inputs(batch, image_size, image_height, image_width):
    """``CoreMLModel.expected_inputs`` of the converted safety checker (torch2coreml.py:1161-1171): static shapes, float16."""
    f16 = np.dtype(np.float16)
    return {"clip_input": {"shape": (int(batch), 3, int(image_size), int(image_size)), "dtype": f16},
            "images": {"shape": (int(batch), int(image_height), int(image_width), 3), "dtype": f16},
            "adjustment": {"shape": (1,), "dtype": f16}}


class HipSafetyChecker(_lib.Model):
    _destroy = "sd_safety_checker_destroy"

    def __init__(self, config, weights, batch=1, device=0, use_graph=True, image_height=512, image_width=512):
        vc = vision_config(config)
        act = vc["hidden_act"]
        if act not in _lib.ACTS:
            raise NotImplementedError(f"hidden_act {act!r} (CLIP vision towers use quick_gelu or gelu)")
        if int(batch) < 1:
            raise ValueError(f"batch must be >= 1, got {batch}")
        if isinstance(weights, dict):                       # the head's sizes are the checkpoint's
            if "concept_embeds" in weights:
                vc.setdefault("num_concepts", int(np.asarray(weights["concept_embeds"]).shape[0]))
            if "special_care_embeds" in weights:
                vc.setdefault("num_special", int(np.asarray(weights["special_care_embeds"]).shape[0]))
        vc.setdefault("num_concepts", NUM_CONCEPTS)
        vc.setdefault("num_special", NUM_SPECIAL)
        self.config = vc
        c = _lib.SafetyCheckerConfig()
        c.batch, c.image_size, c.patch_size = int(batch), int(vc["image_size"]), int(vc["patch_size"])
        c.hidden_size, c.intermediate_size = int(vc["hidden_size"]), int(vc["intermediate_size"])
        c.num_hidden_layers, c.num_attention_heads = int(vc["num_hidden_layers"]), int(vc["num_attention_heads"])
        c.projection_dim, c.num_concepts, c.num_special = int(vc["projection_dim"]), vc["num_concepts"], vc["num_special"]
        c.hidden_act = _lib.ACTS[act]
        c.layer_norm_eps = float(vc["layer_norm_eps"])
        c.use_graph = int(bool(use_graph))
        self._cfg_struct = c
        self.batch, self.image_size = c.batch, c.image_size
        self.seq_len = (c.image_size // max(1, c.patch_size)) ** 2 + 1
        self.expected_inputs = expected_inputs(c.batch, c.image_size, image_height, image_width)
        self._h = C.c_void_p()
        with Weights.lend(weights) as store:
            _lib.check(_lib.lib().sd_safety_checker_create(C.byref(c), store._h, device, C.byref(self._h)))

    @classmethod
    def from_pretrained(cls, folder, **kw):
        path = _lib.checkpoint_file(folder)
        cfg = {}
        if os.path.exists(os.path.join(folder, "config.json")):
            with open(os.path.join(folder, "config.json")) as f:
                cfg = json.load(f)
        from safetensors import safe_open
        with safe_open(path, framework="np") as f:                      # the head's sizes are the checkpoint's
            keys = set(f.keys())
            if "concept_embeds" in keys:
                cfg.setdefault("num_concepts", f.get_slice("concept_embeds").get_shape()[0])
            if "special_care_embeds" in keys:
                cfg.setdefault("num_special", f.get_slice("special_care_embeds").get_shape()[0])
        return cls(cfg, path, **kw)

    def run(self, clip_input, adjustment=0.0, want_hidden=False):
        """The device part: (has_nsfw (B,) bool, concept_scores (B, n) f32, image_embeds (B, P) f32[, last_hidden_state
        (B, S, hidden) f32 - the encoder output BEFORE post_layernorm])."""
        c = self._cfg_struct
        x = np.ascontiguousarray(clip_input, dtype=np.float16)
        if x.shape != self.expected_inputs["clip_input"]["shape"]:
            raise TypeError(f"Expected shape {self.expected_inputs['clip_input']['shape']}, got {x.shape} for input: clip_input")
        flags = np.empty(c.batch, np.float32)
        scores = np.empty((c.batch, c.num_concepts), np.float32)
        embeds = np.empty((c.batch, c.projection_dim), np.float32)
        hidden = np.empty((c.batch, self.seq_len, c.hidden_size), np.float32) if want_hidden else None
        _lib.check(_lib.lib().sd_safety_checker_run(self._h, _lib.ptr(x), float(adjustment), _lib.fptr(flags), _lib.fptr(scores),
                                                    _lib.fptr(embeds), _lib.fptr(hidden), 0))
        out = (flags > 0.5, scores, embeds)
        return out + (hidden,) if want_hidden else out

    def __call__(self, **kwargs):
        self._verify_inputs(**kwargs)
        has_nsfw, scores, _ = self.run(kwargs["clip_input"], float(kwargs["adjustment"][0]))
        return {"filtered_images": blacken(kwargs["images"], has_nsfw), "has_nsfw_concepts": has_nsfw, "concept_scores": scores}

    def last_ms(self):
        """HIP-event milliseconds of the last run's launch list (graph replay or eager launches), copies excluded."""
        return float(_lib.lib().sd_safety_checker_last_ms(self._h))

    def device_bytes(self):
        return _lib.lib().sd_safety_checker_device_bytes(self._h)
