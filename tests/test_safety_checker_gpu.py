"""GPU parity tests of the safety checker: the attention kernel of csrc/vit.hip and the concept head as operators, the whole
checker (csrc/safety_checker.cpp behind HipSafetyChecker) against transformers' CLIPVisionModelWithProjection on the CPU in fp32
with the same fp16-rounded seeded weights, graph replay, and the pipeline / CLI surface over a miniature checkpoint directory.

Gates of the whole-checker test: PSNR at (measured - 6 dB) and never below the reference's 35 dB floor (torch2coreml.py:77),
concept_scores within 2 x the measured absolute error and never above 5e-3 - half of the head's 0.01 special-care lift, the
smallest quantity a verdict can hinge on.  The measured values are in GATES below and in LAB_NOTES.md."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import psnr, weights
from python_hip_stable_diffusion import HipSafetyChecker, _lib, pipeline as P
from test_ops_gpu import close
from test_safety_checker import CONFIGS, NUM_CONCEPTS, NUM_SPECIAL, head_ref, make_checkpoint

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ attention operator
def _attention_ref(qkv, heads):
    """softmax(Q K^T / 8) V per head in fp32 on the fp16-rounded inputs; also returns the logits (B, heads, S, S)."""
    B, S, _ = qkv.shape
    t = torch.from_numpy(qkv.astype(np.float32)).reshape(B, S, 3, heads, 64).permute(2, 0, 3, 1, 4)      # (3, B, heads, S, 64)
    logits = t[0] @ t[1].transpose(-1, -2) / 8.0
    out = torch.softmax(logits, dim=-1) @ t[2]
    return out.permute(0, 2, 1, 3).reshape(B, S, heads * 64).numpy(), logits.numpy()


def _qkv(B, S, heads, regime, seed):
    rs = np.random.RandomState(seed)
    q, k, v = (rs.randn(B, S, heads, 64).astype(np.float32) for _ in range(3))
    peaked = []
    if regime == "peaked":
        # logits of +-30: q . k / 8 has unit variance for unit-variance q and k, so 8 q spreads it to a standard deviation of 8;
        # in every (batch, head) the LAST key is aligned with one query row (logit 0.6 * 8 * |q|^2 / 8 ~ 38), so that row's
        # maximum arrives in the last key tile - with S = 257 in a tile that holds this one valid key
        for b in range(B):
            for h in range(heads):
                r = (7 * h + 3 * b) % S
                k[b, S - 1, h] = 0.6 * q[b, r, h]
                peaked.append((b, h, r))
        q *= 8.0
    qkv = np.stack([q, k, v], axis=2).reshape(B, S, 3 * heads * 64).astype(np.float16)
    return qkv, peaked


ATTN_SHAPES = [(1, 17, 1), (1, 64, 2), (2, 65, 2), (1, 257, 2), (2, 257, 16)]      # (B, S, heads)


@pytest.mark.parametrize("regime", ["unit", "peaked"])
@pytest.mark.parametrize("shape", ATTN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_vit_attention_matches_fp32_softmax(shape, regime):
    B, S, heads = shape
    qkv, peaked = _qkv(B, S, heads, regime, seed=1000 + 31 * S + heads + B)
    ref, logits = _attention_ref(qkv, heads)
    if regime == "peaked":
        assert np.abs(logits).max() >= 25.0
        for b, h, r in peaked:
            assert logits[b, h, r].argmax() == S - 1, "the test's own premise: this row's largest logit sits in the last key"
    n, guard = B * S * heads * 64, 4096
    buf = np.full(n + guard, np.nan, np.float16)                    # output and the guard behind it start as NaN
    out, _ = _lib.vit_attention(qkv, heads, out=buf)
    assert out.shape == ref.shape and np.shares_memory(out, buf)
    assert np.isfinite(out).all(), "an output element was left unwritten or is not finite"
    assert np.isnan(buf[n:]).all(), "the kernel's result ran past the B * S output rows"
    close(out, ref, f"vit_attention {shape} {regime}")              # the gate of sd_op_attention ORIGINAL (tests/test_ops_gpu.py)
    again, _ = _lib.vit_attention(qkv, heads)
    assert np.array_equal(out, again), "two runs differ"


def test_vit_attention_rejects_other_head_dims():
    with pytest.raises(NotImplementedError, match="head dim"):
        _lib.vit_attention(np.zeros((1, 8, 3 * 2 * 32), np.float16), heads=2, dim_head=32)


# ------------------------------------------------------------------------------------------------ concept head operator
def _head_case(cos_concept, cos_special, P=64, seed=0):
    """Embeddings with prescribed cosines: image b points along axis b (any length), concept / special-care row i has the component
    cos[b][i] along axis b and the rest of its unit length along an axis of its own; every row is then scaled to a random length."""
    rs = np.random.RandomState(seed)
    cos_concept, cos_special = np.atleast_2d(cos_concept), np.atleast_2d(cos_special)
    B = cos_concept.shape[0]
    image = np.zeros((B, P))
    image[np.arange(B), np.arange(B)] = rs.uniform(0.5, 5.0, B)

    def table(cos, first_axis):
        n = cos.shape[1]
        t = np.zeros((n, P))
        t[:, :B] = cos.T
        t[np.arange(n), first_axis + np.arange(n)] = np.sqrt(1.0 - (cos ** 2).sum(axis=0))
        return t * rs.uniform(0.5, 5.0, (n, 1))
    return image, table(cos_concept, B), table(cos_special, B + cos_concept.shape[1])


HEAD_CASES = {      # concept score = cos - 0.5 (+ lift), special score = cos - 0.5 + adjustment: (concept cos, special cos, adjustment, want)
    "not-flagged": ([[0.45] * 17], [[0.46] * 3], 0.0, [False]),
    "flagged-outright": ([[0.45] * 5 + [0.52] + [0.45] * 11], [[0.46] * 3], 0.0, [True]),
    "flagged-through-special-care": ([[0.45] * 16 + [0.495]], [[0.46, 0.51, 0.46]], 0.0, [True]),       # -0.005 + 0.01
    "flagged-through-adjustment": ([[0.45] * 16 + [0.495]], [[0.46, 0.49, 0.46]], 0.02, [True]),         # special -0.01 + 0.02
    "same-without-adjustment": ([[0.45] * 16 + [0.495]], [[0.46, 0.49, 0.46]], 0.0, [False]),
    "batch-of-two-mixed": ([[0.45] * 17, [0.44] * 3 + [0.53] + [0.44] * 13], [[0.46] * 3, [0.40] * 3], 0.0, [False, True]),
}


@pytest.mark.parametrize("case", sorted(HEAD_CASES))
def test_safety_head_matches_numpy(case):
    cos_c, cos_s, adjustment, want = HEAD_CASES[case]
    image, concept, special = _head_case(np.array(cos_c), np.array(cos_s), seed=len(case))
    cw, sw = np.full(NUM_CONCEPTS, 0.5), np.full(NUM_SPECIAL, 0.5)
    ref_flags, ref_scores = head_ref(image.astype(np.float32), concept.astype(np.float32), special.astype(np.float32), cw, sw, adjustment)
    assert np.abs(ref_scores).min() >= 0.004, "the test's own premise: no score close enough to 0 for rounding to decide"
    assert list(ref_flags) == want
    flags, scores = _lib.safety_head(image, concept, special, cw, sw, adjustment)
    np.testing.assert_allclose(scores, ref_scores, atol=1e-5, rtol=0)
    assert list(flags) == want


# ------------------------------------------------------------------------------------------------ whole checker
def _oracle(cfg, sd16):
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    model = CLIPVisionModelWithProjection(CLIPVisionConfig(**cfg)).eval()
    state = {k.replace("vision_model.vision_model.", "vision_model."): torch.from_numpy(v.astype(np.float32))
             for k, v in sd16.items() if k.startswith("vision_model.") or k == "visual_projection.weight"}
    model.load_state_dict(state, strict=True)
    return model


def _oracle_forward(model, clip_input):
    with torch.no_grad():
        out = model(pixel_values=torch.from_numpy(clip_input.astype(np.float32)))
    return out.last_hidden_state.numpy(), out.image_embeds.numpy()


def _cosines(embeds, table):
    e = embeds.astype(np.float64) / np.linalg.norm(embeds.astype(np.float64), axis=1, keepdims=True)
    t = table.astype(np.float64) / np.linalg.norm(table.astype(np.float64), axis=1, keepdims=True)
    return e @ t.T


def _set_thresholds(sd16, embeds, hit=()):
    """Thresholds from the ORACLE's cosines, every score at least 0.02 from 0 for every image of the batch: concept i in `hit`
    fires for all of them (threshold 0.03 under the smallest cosine), every other concept and every special-care concept for none
    (0.03 above the largest)."""
    cc, cs = _cosines(embeds, sd16["concept_embeds"]), _cosines(embeds, sd16["special_care_embeds"])
    cw = cc.max(axis=0) + 0.03
    for i in hit:
        cw[i] = cc[:, i].min() - 0.03
    sd16["concept_embeds_weights"] = cw.astype(np.float16)
    sd16["special_care_embeds_weights"] = (cs.max(axis=0) + 0.03).astype(np.float16)


# (PSNR gate of last_hidden_state, PSNR gate of image_embeds, bound of max |concept_scores error|) = (measured - 6 dB, measured - 6 dB,
# 2 x measured); measured on an MI355X, in this order: mini 71.47 / 71.93 dB / 2.456e-4, 72.09 / 72.82 / 2.456e-4;
# mini-257 64.65 / 59.06 / 9.047e-4, 65.64 / 60.00 / 9.047e-4; vit-l-2 65.66 / 63.17 / 1.847e-4, 66.32 / 63.67 / 2.014e-4
GATES = {
    ("mini", 1): (65.47, 65.93, 4.92e-4), ("mini", 2): (66.09, 66.82, 4.92e-4),
    ("mini-257", 1): (58.65, 53.06, 1.81e-3), ("mini-257", 2): (59.64, 54.00, 1.81e-3),
    ("vit-l-2", 1): (59.66, 57.17, 3.70e-4), ("vit-l-2", 2): (60.32, 57.67, 4.03e-4),
}


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("name", ["mini", "mini-257", "vit-l-2"])
def test_safety_checker_matches_transformers(name, batch):
    cfg = CONFIGS[name]
    sd16 = make_checkpoint(cfg, seed=11)
    clip_input = weights.seeded_normal((batch, 3, cfg["image_size"], cfg["image_size"]), 5).astype(np.float16)
    ref_hidden, ref_embeds = _oracle_forward(_oracle(cfg, sd16), clip_input)
    _set_thresholds(sd16, ref_embeds, hit=(5,))
    ref_flags, ref_scores = head_ref(ref_embeds, sd16["concept_embeds"], sd16["special_care_embeds"], sd16["concept_embeds_weights"],
                                     sd16["special_care_embeds_weights"])
    assert np.abs(ref_scores).min() >= 0.02 and ref_flags.all()
    chk = HipSafetyChecker(cfg, sd16, batch=batch)
    flags, scores, embeds, hidden = chk.run(clip_input, 0.0, want_hidden=True)
    chk.close()
    assert hidden.shape == ref_hidden.shape and embeds.shape == ref_embeds.shape and scores.shape == (batch, NUM_CONCEPTS)
    p_hidden, p_embeds = psnr.compute_psnr(hidden, ref_hidden), psnr.compute_psnr(embeds, ref_embeds)
    err = float(np.abs(scores - ref_scores).max())
    print(f"MEASURED safety_checker {name} batch {batch}: last_hidden_state {p_hidden:.2f} dB, image_embeds {p_embeds:.2f} dB, "
          f"max |concept_scores error| {err:.3e}")
    # the class token averages the patches away: last_hidden_state is the tensor that proves the patch path, token by token
    worst_token = min(psnr.compute_psnr(hidden[:, t], ref_hidden[:, t]) for t in range(hidden.shape[1]))
    g_hidden, g_embeds, g_err = GATES[(name, batch)]
    assert g_hidden >= psnr.ABSOLUTE_MIN_PSNR and g_embeds >= psnr.ABSOLUTE_MIN_PSNR and g_err <= 5e-3
    assert p_hidden >= g_hidden, f"last_hidden_state: PSNR {p_hidden:.1f} dB"
    assert worst_token >= psnr.ABSOLUTE_MIN_PSNR, f"worst token of last_hidden_state: PSNR {worst_token:.1f} dB"
    assert p_embeds >= g_embeds, f"image_embeds: PSNR {p_embeds:.1f} dB"
    assert err <= g_err, f"concept_scores: max |error| {err:.3e}"
    assert list(flags) == list(ref_flags)


def test_graph_replay_is_bit_identical_to_eager_launches():
    cfg = CONFIGS["mini-257"]
    sd16 = make_checkpoint(cfg, seed=12)
    clip_input = weights.seeded_normal((2, 3, 224, 224), 6).astype(np.float16)
    eager = HipSafetyChecker(cfg, sd16, batch=2, use_graph=False)
    want = eager.run(clip_input, 0.0, want_hidden=True)
    eager.close()
    assert all(np.isfinite(a).all() for a in want[1:])
    graph = HipSafetyChecker(cfg, sd16, batch=2, use_graph=True)
    for i in range(11):                                   # call 0 launches eagerly and captures, calls 1-10 replay
        got = graph.run(clip_input, 0.0, want_hidden=True)
        for a, b in zip(got, want):
            assert np.array_equal(a, b), f"call {i} differs from the eager handle"
    # the adjustment is read from device memory by the captured head: a replay sees a new value
    # (-10: no special-care concept fires, +10: all do, which lifts every concept score by 0.01)
    low, high = graph.run(clip_input, -10.0), graph.run(clip_input, 10.0)
    np.testing.assert_allclose(high[1] - low[1], 0.01, atol=1e-6, rtol=0)
    graph.close()


# ------------------------------------------------------------------------------------------------ pipeline + CLI
def _add_safety_checker(root, cfg, sd16):
    from safetensors.numpy import save_file
    os.makedirs(os.path.join(root, "safety_checker"), exist_ok=True)
    os.makedirs(os.path.join(root, "feature_extractor"), exist_ok=True)
    save_file({k: np.ascontiguousarray(v) for k, v in sd16.items()}, os.path.join(root, "safety_checker", "model.safetensors"),
              metadata={"format": "pt"})
    vision = {k: v for k, v in cfg.items() if k != "projection_dim"}
    json.dump({"architectures": ["StableDiffusionSafetyChecker"], "projection_dim": cfg["projection_dim"], "vision_config": vision},
              open(os.path.join(root, "safety_checker", "config.json"), "w"))
    size = cfg["image_size"]
    json.dump({"crop_size": {"height": size, "width": size}, "do_center_crop": True, "do_convert_rgb": True, "do_normalize": True,
               "do_resize": True, "feature_extractor_type": "CLIPFeatureExtractor", "image_mean": [0.48145466, 0.4578275, 0.40821073],
               "image_std": [0.26862954, 0.26130258, 0.27577711], "resample": 3, "size": {"shortest_edge": size}},
              open(os.path.join(root, "feature_extractor", "preprocessor_config.json"), "w"))


def _close(pipe):
    for m in (pipe.unet, pipe.vae_decoder, pipe.text_encoder, pipe.safety_checker):
        if m is not None:
            m.close()


def test_pipeline_and_cli_run_the_checkpoints_safety_checker(tmp_path):
    from test_text_encoder_gpu import write_checkpoint_dir
    root = str(tmp_path / "mini-sd")
    os.makedirs(root)
    write_checkpoint_dir(root)
    cfg = CONFIGS["mini"]
    sd16 = make_checkpoint(cfg, seed=13)
    _add_safety_checker(root, cfg, sd16)
    run = dict(num_inference_steps=3, guidance_scale=7.5, negative_prompt="blurry", seed=93)
    prompt = "a photo of an astronaut riding a horse"

    plain = P.get_hip_pipe(root, "mini/stable-diffusion", attention_implementation="ORIGINAL", disable_safety=True)
    assert plain.safety_checker is None and plain.feature_extractor is None
    base = plain(prompt, **run)
    assert base.nsfw_content_detected is None and base.images.any()
    # thresholds from the oracle's view of exactly the image the checker will see
    clip_input = plain.numpy_to_pil(base.images)
    _close(plain)
    from python_hip_stable_diffusion.safety_checker import load_feature_extractor
    clip_input = load_feature_extractor(os.path.join(root, "feature_extractor"))(clip_input, return_tensors="np").pixel_values
    _, embeds = _oracle_forward(_oracle(cfg, sd16), clip_input.astype(np.float16))

    _set_thresholds(sd16, embeds)                                       # nothing fires
    _add_safety_checker(root, cfg, sd16)
    pipe = P.get_hip_pipe(root, "mini/stable-diffusion", attention_implementation="ORIGINAL")
    assert isinstance(pipe.safety_checker, HipSafetyChecker) and pipe.safety_checker.batch == 1
    assert pipe.safety_checker.expected_inputs["images"]["shape"] == (1, 128, 128, 3)
    out = pipe(prompt, **run)
    assert np.array_equal(out.images, base.images) and list(out.nsfw_content_detected) == [False]
    latent = pipe(prompt, output_type="latent", **run)                  # no image, no verdict
    assert latent.nsfw_content_detected is None
    _close(pipe)

    _set_thresholds(sd16, embeds, hit=(3,))                             # concept 3 fires
    _add_safety_checker(root, cfg, sd16)
    pipe = P.get_hip_pipe(root, "mini/stable-diffusion", attention_implementation="ORIGINAL")
    out = pipe(prompt, **run)
    assert out.images.shape == base.images.shape and not out.images.any() and list(out.nsfw_content_detected) == [True]
    _close(pipe)

    # the CLI over the same (flagging) checkpoint: black with the checker, the picture with --disable-safety
    from PIL import Image
    common = ["--prompt", prompt, "-i", root, "--seed", "93", "--model-version", "mini/stable-diffusion", "--num-inference-steps", "3",
              "--attention-implementation", "ORIGINAL", "--negative-prompt", "blurry"]
    checked = np.asarray(Image.open(P.main(P.build_parser().parse_args(common + ["-o", str(tmp_path / "checked")]))))
    free = np.asarray(Image.open(P.main(P.build_parser().parse_args(common + ["-o", str(tmp_path / "free"), "--disable-safety"]))))
    assert not checked.any() and free.any()
