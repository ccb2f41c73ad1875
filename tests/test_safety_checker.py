"""CPU suite of the safety checker (csrc/safety_checker.cpp + vit.hip behind HipSafetyChecker): the public surface exists, the
ctypes mirror follows the header, everything that can be refused on the host is refused there, a GPU-less machine gets a loud
RuntimeError instead of a CPU fallback, the host-side blackening is right, and vit.hip compiles for gfx950 without scratch.

Also the helpers the GPU suite (tests/test_safety_checker_gpu.py) shares: the miniature configs, the checkpoint inventory in
diffusers' key names, and the numpy restatement of the concept head."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from oracle import weights

# name -> vision tower settings (CLIPVisionConfig names); head dim 64 everywhere, the only one the attention kernel is built for
CONFIGS = {
    "mini": dict(image_size=56, patch_size=14, hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=1,
                 projection_dim=64, hidden_act="quick_gelu", layer_norm_eps=1e-5),                     # 17 tokens
    "mini-257": dict(image_size=224, patch_size=14, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                     projection_dim=64, hidden_act="quick_gelu", layer_norm_eps=1e-5),                 # 257 tokens
    "vit-l-2": dict(image_size=224, patch_size=14, hidden_size=1024, intermediate_size=4096, num_hidden_layers=2,
                    num_attention_heads=16, projection_dim=768, hidden_act="quick_gelu", layer_norm_eps=1e-5),
}
NUM_CONCEPTS, NUM_SPECIAL = 17, 3


def param_shapes(cfg, prefix="vision_model.vision_model."):
    """Inventory of a StableDiffusionSafetyChecker checkpoint (diffusers' key names, in module order)."""
    D, I, P, p = cfg["hidden_size"], cfg["intermediate_size"], cfg["projection_dim"], cfg["patch_size"]
    S = (cfg["image_size"] // p) ** 2 + 1
    s = {prefix + "embeddings.class_embedding": (D,),
         prefix + "embeddings.patch_embedding.weight": (D, 3, p, p),
         prefix + "embeddings.position_embedding.weight": (S, D),
         prefix + "pre_layrnorm.weight": (D,), prefix + "pre_layrnorm.bias": (D,)}
    for l in range(cfg["num_hidden_layers"]):
        q = f"{prefix}encoder.layers.{l}."
        for proj in ("k_proj", "v_proj", "q_proj", "out_proj"):
            s[q + f"self_attn.{proj}.weight"] = (D, D)
            s[q + f"self_attn.{proj}.bias"] = (D,)
        s[q + "layer_norm1.weight"], s[q + "layer_norm1.bias"] = (D,), (D,)
        s[q + "mlp.fc1.weight"], s[q + "mlp.fc1.bias"] = (I, D), (I,)
        s[q + "mlp.fc2.weight"], s[q + "mlp.fc2.bias"] = (D, I), (D,)
        s[q + "layer_norm2.weight"], s[q + "layer_norm2.bias"] = (D,), (D,)
    s[prefix + "post_layernorm.weight"], s[prefix + "post_layernorm.bias"] = (D,), (D,)
    s["visual_projection.weight"] = (P, D)
    s["concept_embeds"], s["special_care_embeds"] = (NUM_CONCEPTS, P), (NUM_SPECIAL, P)
    s["concept_embeds_weights"], s["special_care_embeds_weights"] = (NUM_CONCEPTS,), (NUM_SPECIAL,)
    return s


def make_checkpoint(cfg, seed=11, prefix="vision_model.vision_model."):
    """Seeded fp16 weights (oracle.weights.make_state_dict).  Its rule draws every 1-D tensor whose name lacks ".norm" around 0,
    which for CLIP's `layer_norm1` / `pre_layrnorm` names would mean LayerNorm gains of +-0.09: they get 1 added, so the gains are
    what a trained tower has (around 1) and the attention logits are not degenerate."""
    sd = weights.make_state_dict(param_shapes(cfg, prefix), seed=seed, dtype=np.float32, gain=2.0)
    for k in sd:
        if "norm" in k and k.endswith(".weight"):
            sd[k] = sd[k] + 1.0
    return {k: v.astype(np.float16) for k, v in sd.items()}


def head_ref(image_embeds, concept_embeds, special_embeds, concept_w, special_w, adjustment=0.0):
    """The concept head in numpy float64: cosine similarities against both embedding tables, the special-care scores decide a
    0.01 lift of every concept score of that image, any positive concept score flags it."""
    def unit(a):
        a = np.asarray(a, np.float64)
        return a / np.linalg.norm(a, axis=-1, keepdims=True)
    img = unit(image_embeds)
    special = img @ unit(special_embeds).T - np.asarray(special_w, np.float64) + adjustment
    lift = 0.01 * (special > 0).any(axis=1, keepdims=True)
    concept = img @ unit(concept_embeds).T - np.asarray(concept_w, np.float64) + lift
    return (concept > 0).any(axis=1), concept


# ---------------------------------------------------------------------------------------------------------------- tests
def test_package_exports_the_safety_checker():
    import python_hip_stable_diffusion as pkg
    assert callable(pkg.HipSafetyChecker) and callable(pkg.HipSafetyChecker.from_pretrained)
    for name in ("close", "device_bytes", "__call__"):
        assert hasattr(pkg.HipSafetyChecker, name), name


def test_ctypes_config_mirrors_the_header():
    from python_hip_stable_diffusion import _lib
    text = open(os.path.join(ROOT, "include", "sd_mi355x.h")).read()
    body = re.search(r"typedef struct sd_safety_checker_config \{(.*?)\} sd_safety_checker_config;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.search(r"([A-Za-z_][A-Za-z0-9_]*)\s*$", part.strip()).group(1)
              for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert [f[0] for f in _lib.SafetyCheckerConfig._fields_] == fields
    assert len(fields) == 13 and C.sizeof(_lib.SafetyCheckerConfig) == 4 * len(fields)       # all members 4 bytes wide: no padding
    # the UNet structs keep their pinned layout: nothing was added to them
    assert _lib.UNetIO.step_noise.offset == C.sizeof(_lib.UNetIO) - 8


def test_inputs_are_validated_like_the_model_runner_seam():
    from python_hip_stable_diffusion import safety_checker as sc
    exp = sc.expected_inputs(2, 56, 128, 96)
    assert exp["clip_input"] == {"shape": (2, 3, 56, 56), "dtype": np.dtype(np.float16)}
    assert exp["images"] == {"shape": (2, 128, 96, 3), "dtype": np.dtype(np.float16)}
    assert exp["adjustment"] == {"shape": (1,), "dtype": np.dtype(np.float16)}
    good = dict(clip_input=np.zeros((2, 3, 56, 56), np.float16), images=np.zeros((2, 128, 96, 3), np.float16),
                adjustment=np.zeros(1, np.float16))
    sc.verify_inputs(exp, **good)
    with pytest.raises(TypeError, match="dtype"):
        sc.verify_inputs(exp, **dict(good, clip_input=good["clip_input"].astype(np.float32)))
    with pytest.raises(TypeError, match="shape"):
        sc.verify_inputs(exp, **dict(good, images=good["images"][:1]))
    with pytest.raises(TypeError, match="numpy"):
        sc.verify_inputs(exp, **dict(good, adjustment=0.0))
    with pytest.raises(ValueError, match="unexpected"):
        sc.verify_inputs(exp, pixel_values=good["clip_input"], **good)
    with pytest.raises(ValueError, match="Missing"):
        sc.verify_inputs(exp, clip_input=good["clip_input"], images=good["images"])


def test_vision_config_reads_the_checkpoint_layout_and_falls_back_to_vit_l_14():
    from python_hip_stable_diffusion import safety_checker as sc
    assert sc.vision_config({}) == sc.VIT_L_14
    got = sc.vision_config({"projection_dim": 512, "vision_config": {"hidden_size": 128, "num_attention_heads": 2, "dropout": 0.0}})
    assert got["hidden_size"] == 128 and got["num_attention_heads"] == 2 and got["projection_dim"] == 512
    assert got["patch_size"] == 14 and got["image_size"] == 224 and "dropout" not in got
    assert sc.vision_config(CONFIGS["mini"])["image_size"] == 56


def test_bad_configs_and_checkpoints_are_refused_before_any_device_work(sdlib):
    """Every one of these raises the same way with and without a GPU: the C side checks the config and the whole weight inventory
    on the host before it asks for a device."""
    from python_hip_stable_diffusion import HipSafetyChecker, _lib
    cfg = CONFIGS["mini"]
    sd = make_checkpoint(cfg)
    with pytest.raises(NotImplementedError, match="hidden_act"):
        HipSafetyChecker(dict(cfg, hidden_act="silu"), sd)
    with pytest.raises(ValueError, match="batch"):
        HipSafetyChecker(cfg, sd, batch=0)
    with pytest.raises(ValueError, match="patch"):
        HipSafetyChecker(dict(cfg, image_size=60), sd)                     # 60 is no multiple of 14
    with pytest.raises(NotImplementedError, match="head dim"):
        HipSafetyChecker(dict(cfg, num_attention_heads=2), sd)             # heads of 32
    missing = {k: v for k, v in sd.items() if not k.endswith("pre_layrnorm.bias")}
    with pytest.raises(FileNotFoundError, match="pre_layrnorm.bias"):
        HipSafetyChecker(cfg, missing)
    with pytest.raises(FileNotFoundError):
        HipSafetyChecker(cfg, {})
    wrong = dict(sd)
    wrong["visual_projection.weight"] = np.zeros((cfg["projection_dim"], cfg["hidden_size"] + 8), np.float16)
    with pytest.raises(ValueError, match="visual_projection"):
        HipSafetyChecker(cfg, wrong)
    with pytest.raises(ValueError, match="concept_embeds"):                # the config's head size against the checkpoint's
        HipSafetyChecker(dict(cfg, num_concepts=5), sd)
    # the operator entries check their arguments first as well
    with pytest.raises(NotImplementedError, match="head dim"):
        _lib.vit_attention(np.zeros((1, 4, 3 * 32), np.float16), heads=1, dim_head=32)
    with pytest.raises(ValueError):
        _lib.vit_attention(np.zeros((1, 4, 100), np.float16), heads=1)
    with pytest.raises(ValueError):
        _lib.safety_head(np.zeros((1, 8)), np.zeros((3, 8)), np.zeros((2, 4)), np.zeros(3), np.zeros(2))


def test_both_key_prefixes_are_accepted_and_there_is_no_cpu_fallback(sdlib):
    """A valid checkpoint passes the host checks under diffusers' double prefix and under a single `vision_model.`; what happens
    next depends on the machine alone: a handle on a GPU, RuntimeError without one - never a computation on the host."""
    from python_hip_stable_diffusion import HipSafetyChecker, _lib
    cfg = CONFIGS["mini"]
    for prefix in ("vision_model.vision_model.", "vision_model."):
        sd = make_checkpoint(cfg, prefix=prefix)
        if sdlib.sd_device_count() > 0:
            chk = HipSafetyChecker(cfg, sd)
            assert chk.device_bytes() > 0
            chk.close()
        else:
            with pytest.raises(RuntimeError, match="no HIP device"):
                HipSafetyChecker(cfg, sd)
    if sdlib.sd_device_count() <= 0:
        with pytest.raises(RuntimeError):
            _lib.vit_attention(np.zeros((1, 4, 192), np.float16), heads=1)
        with pytest.raises(RuntimeError):
            _lib.safety_head(np.ones((1, 8)), np.ones((3, 8)), np.ones((2, 8)), np.zeros(3), np.zeros(2))


def test_blackening_of_a_mixed_batch():
    from python_hip_stable_diffusion import safety_checker as sc
    rs = np.random.RandomState(0)
    images = rs.rand(3, 8, 6, 3).astype(np.float16) + np.float16(0.25)     # no zero pixel to begin with
    keep = images.copy()
    out = sc.blacken(images, np.array([False, True, False]))
    assert out.dtype == images.dtype and out.shape == images.shape
    assert np.array_equal(out[0], keep[0]) and np.array_equal(out[2], keep[2]) and not out[1].any()
    assert np.array_equal(images, keep), "the input must not be modified"
    assert not sc.blacken(images, np.array([1.0, 1.0, 1.0])).any()
    assert np.array_equal(sc.blacken(images, np.zeros(3, bool)), keep)
    with pytest.raises(ValueError):
        sc.blacken(images, np.array([True, False]))


def test_a_checker_without_a_feature_extractor_is_refused_at_construction():
    from python_hip_stable_diffusion.pipeline import HipStableDiffusionPipeline
    from python_hip_stable_diffusion import schedulers

    class UNetShape:
        expected_inputs = {"sample": {"shape": (2, 4, 8, 8)}}
    with pytest.raises(ValueError, match="feature extractor"):
        HipStableDiffusionPipeline(None, UNetShape(), None, schedulers.DDIMScheduler(), None, safety_checker=object())
    pipe = HipStableDiffusionPipeline(None, UNetShape(), None, schedulers.DDIMScheduler(), None)      # none given: as before
    img = np.ones((1, 4, 4, 3), np.float32)
    out, flags = pipe.run_safety_checker(img)
    assert out is img and flags is None


def test_cli_has_the_disable_safety_switch():
    from python_hip_stable_diffusion import pipeline as P
    base = ["--prompt", "x", "-i", "in", "-o", "out"]
    assert P.build_parser().parse_args(base).disable_safety is False
    assert P.build_parser().parse_args(base + ["--disable-safety"]).disable_safety is True


def test_vit_kernels_compile_for_gfx950_without_scratch(tmp_path):
    from test_build_isa import CSRC, HIPCC, kernel_resources
    assert os.path.exists(HIPCC), "hipcc not installed"
    res = kernel_resources(os.path.join(CSRC, "vit.hip"), tmp_path)
    names = " ".join(res)
    for k in ("vit_attention_kernel", "vit_patch_rows_kernel", "vit_tokens_kernel", "safety_head_kernel"):
        assert k in names, (k, sorted(res))
    spilled = {k: v for k, v in res.items() if v[1] != 0}
    assert not spilled, f"kernels with scratch (register spills): {spilled}"
    assert "v_mfma_f32_16x16x32_f16" in kernel_resources.last_asm, "the attention products must run on the matrix cores"
