"""GPU parity tests of the VAE's streaming mid-block attention (csrc/vae_attention.hip): the operator entry against fp32 torch on the
fp16-rounded inputs, and the fp16 VAE handles at the sizes that take it - a token count H*W above 8192 or no multiple of 64 -
against oracle/vae_ref.py.  Where the materialised route ran before (H*W <= 8192 and a multiple of 64) nothing may change: the
16 x 16 decoder's output is compared bit for bit with a hash recorded from the commit before this kernel existed.

Operator gate: close() of tests/test_ops_gpu.py (PSNR >= 60 dB, max error <= 4e-3 max|ref| + 1e-3), what sd_op_attention and
sd_op_vit_attention meet.  Handle gates: PSNR at (measured on an MI355X - 6 dB), rounded down, never below 60 dB; the measured
values stand beside the gates in HANDLE_GATES."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import psnr, vae_ref, weights
from python_hip_stable_diffusion import HipVaeDecoder, HipVaeEncoder, _lib
from test_ops_gpu import close

pytestmark = pytest.mark.gpu

GUARD = 4096


# ------------------------------------------------------------------------------------------------ operator
def _ref(q, k, v, rows=None):
    """softmax(q k^T / sqrt(C)) v in fp32 on the fp16-rounded inputs, for all query rows or the listed ones; also the logits."""
    q, k, v = (torch.from_numpy(a.astype(np.float32)) for a in (q, k, v))
    if rows is not None:
        q = q[:, rows]
    logits = q @ k.transpose(1, 2) / float(np.sqrt(q.shape[2]))
    assert torch.isfinite(logits).all()
    out = torch.softmax(logits, dim=-1) @ v
    assert torch.isfinite(out).all(), "the fp32 reference must stay finite on the test's inputs"
    return out.numpy(), logits.numpy()


@functools.lru_cache(maxsize=None)
def _case(B, S, Cn, regime):
    """Inputs as test_safety_checker_gpu.py::_qkv builds them, scaled for the head dim: unit-variance q, k, v give logits
    q . k / sqrt(C) of unit variance at every C.  "peaked": 8 q spreads them to a standard deviation of 8, and in every image the
    LAST key is aligned with one query row - k = (4.8 / sqrt(C)) q gives that row the logit 4.8 |q|^2 / C ~ 38 (0.6 q at C = 64) -
    so that row's maximum arrives in the last key tile.  Returns (q, k, v, reference, logits, [(b, row)])."""
    rs = np.random.RandomState(1000 + 31 * S + Cn + B)
    q, k, v = (rs.randn(B, S, Cn).astype(np.float32) for _ in range(3))
    peaked = []
    if regime == "peaked":
        for b in range(B):
            r = (7 + 3 * b) % S
            k[b, S - 1] = 4.8 / np.sqrt(Cn) * q[b, r]
            peaked.append((b, r))
        q *= 8.0
    q, k, v = (a.astype(np.float16) for a in (q, k, v))
    ref, logits = _ref(q, k, v)
    for a in (q, k, v, ref, logits):
        a.setflags(write=False)
    return q, k, v, ref, logits, peaked


def _run_guarded(q, k, v, ref, what):
    """One launch into a NaN-filled buffer with a NaN guard behind it, the gate, and a second run that must agree bit for bit."""
    n = q.size
    buf = np.full(n + GUARD, np.nan, np.float16)                    # output and the guard behind it start as NaN
    out, _ = _lib.vae_attention(q, k, v, out=buf)
    assert out.shape == q.shape and np.shares_memory(out, buf)
    assert np.isfinite(out).all(), "an output element was left unwritten or is not finite"
    assert np.isnan(buf[n:]).all(), "the kernel's result ran past the B * S output rows"
    if ref is not None:
        close(out, ref, what)
    again, _ = _lib.vae_attention(q, k, v)
    assert np.array_equal(out.view(np.uint16), again.view(np.uint16)), "two runs differ"
    return out


OP_SHAPES = [(1, 1, 64), (1, 16, 512), (1, 64, 64), (2, 65, 128), (2, 100, 64), (1, 200, 256), (1, 192, 512), (2, 331, 512)]   # (B, S, C)


@pytest.mark.parametrize("regime", ["unit", "peaked"])
@pytest.mark.parametrize("shape", OP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_vae_attention_matches_fp32_softmax(shape, regime):
    B, S, Cn = shape
    q, k, v, ref, logits, peaked = _case(B, S, Cn, regime)
    if regime == "peaked":
        assert np.abs(logits).max() >= 25.0
        for b, r in peaked:
            assert logits[b, r].argmax() == S - 1, "the test's own premise: this row's largest logit sits in the last key"
    _run_guarded(q, k, v, ref, f"vae_attention {shape} {regime}")


def test_vae_attention_rescales_when_the_maximum_arrives_late():
    """Every logit of the first 64-key tile lies at least 200 below every later logit of its row: what the first tile accumulated
    is scaled away (exp2 underflows to 0) when the second arrives.  One shared coordinate carries the offset: q0 = 40 in every
    query, k0 = -+150 sqrt(C) / 40 in the first tile / behind it; the other coordinates add unit-variance logits."""
    B, S, Cn = 1, 200, 512
    rs = np.random.RandomState(5)
    q, k, v = (rs.randn(B, S, Cn).astype(np.float32) for _ in range(3))
    q[:, :, 0] = 40.0
    k[:, :, 0] = 150.0 * np.sqrt(Cn) / 40.0
    k[:, :64, 0] *= -1.0
    q, k, v = (a.astype(np.float16) for a in (q, k, v))
    ref, logits = _ref(q, k, v)
    assert (logits[:, :, 64:].min(axis=2) - logits[:, :, :64].max(axis=2)).min() >= 200.0, "the test's own premise"
    _run_guarded(q, k, v, ref, "vae_attention late maximum")


def test_vae_attention_past_8192_tokens_at_the_production_head_dim():
    """(1, 9216, 512): a 768 x 768 image's mid-block.  The reference covers every row of the first and of the last 64-query tile
    and every 37th row between; finiteness, the guard and the second run cover all rows."""
    B, S, Cn = 1, 9216, 512
    rs = np.random.RandomState(9216)
    q, k, v = (rs.randn(B, S, Cn).astype(np.float16) for _ in range(3))
    rows = np.unique(np.concatenate([np.arange(64), np.arange(S - 64, S), np.arange(0, S, 37)]))
    ref, _ = _ref(q, k, v, rows)
    out = _run_guarded(q, k, v, None, "")
    close(out[:, rows], ref, "vae_attention (1, 9216, 512), %d reference rows" % len(rows))


# ------------------------------------------------------------------------------------------------ handles
MINI, SD = vae_ref.VAE_CONFIGS["mini"], vae_ref.VAE_CONFIGS["sd"]
TWO_LEVEL = dict(latent_channels=4, out_channels=3, block_out_channels=(64, 64), layers_per_block=1)      # mid-block width 64

HANDLE_GATES = {                      # gate (dB), measured on an MI355X (dB)
    "dec-mini-10x10-b1": (68.0, 74.79),
    "dec-mini-10x10-b2": (68.0, 74.87),
    "dec-mini-12x10-b1": (68.0, 74.41),
    "dec-mini-12x10-b2": (68.0, 74.48),
    "dec-two-level-96x96": (72.0, 78.16),
    "dec-sd-12x12": (72.0, 78.07),
    "enc-mini-80x80": (67.0, 73.57),
    "pipeline-mini-96x96": (83.0, 89.62),
}


def _gate(name, got, ref):
    p = psnr.compute_psnr(got, ref)
    print(f"{name}: PSNR {p:.2f} dB (gate {HANDLE_GATES[name][0]})")
    assert p >= HANDLE_GATES[name][0], f"{name}: PSNR {p:.1f} dB"


def _decoder_weights(cfg, seed=61):
    sd16 = weights.make_state_dict(vae_ref.vae_decoder_param_shapes(cfg), seed=seed, dtype=np.float16, gain=1.6)
    return sd16, weights.to_torch({k: v.astype(np.float32) for k, v in sd16.items()})


def _latents(B, h, w, seed=62):
    return (weights.seeded_normal((B, 4, h, w), seed) / 0.18215).astype(np.float16)     # pipeline.py:314


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("hw", [(10, 10), (12, 10)], ids=lambda s: "%dx%d" % s)
def test_decoder_at_ragged_token_counts(hw, B):
    """S = 100 and S = 120 (non-square): no multiple of 64, refused at create before.  Graph replay == eager launches."""
    h, w = hw
    sd16, sd = _decoder_weights(MINI)
    z = _latents(B, h, w)
    ref = vae_ref.vae_decode(sd, MINI, torch.from_numpy(z.astype(np.float32))).numpy()
    outs = []
    for use_graph in (True, False):
        vae = HipVaeDecoder(MINI, sd16, batch=B, latent_height=h, latent_width=w, use_graph=use_graph)
        first = vae(z=z)["image"]
        outs += [first, vae(z=z)["image"]]            # the second call replays the captured graph
        vae.close()
    assert outs[0].shape == ref.shape == (B, 3, 8 * h, 8 * w)
    _gate(f"dec-mini-{h}x{w}-b{B}", outs[0], ref)
    for o in outs[1:]:
        assert np.array_equal(_bits(o), _bits(outs[0])), "graph replay and eager launches differ"


def test_two_level_decoder_at_96x96_has_no_score_matrix_and_feeds_decode_images():
    """S = 9216 (a 768 x 768 image's mid-block size): created before, refused inside the first decode.  The handle's arena is smaller
    than one S x S fp16 matrix, and sd_vae_decode_images runs its later ops behind the same launch list.  (In the plan tuners' mode,
    SD_TUNE=1, the conv workspace alone holds room for 16 split-K slabs of any candidate plan - 228 MB in all here - so the arena
    bound is one of a production process, as the suite runs.)"""
    h = w = 96
    S = h * w
    sd16, sd = _decoder_weights(TWO_LEVEL)
    z = _latents(1, h, w)
    ref = vae_ref.vae_decode(sd, TWO_LEVEL, torch.from_numpy(z.astype(np.float32))).numpy()
    vae = HipVaeDecoder(TWO_LEVEL, sd16, batch=1, latent_height=h, latent_width=w)
    fn = _lib.lib().sd_unet_arena_used_bytes
    used = fn(vae._h)
    assert 0 < used < S * S * 2, f"the arena holds {used} bytes: room for an S x S score matrix ({S * S * 2})"
    image = vae(z=z)["image"]
    assert image.shape == ref.shape == (1, 3, 2 * h, 2 * w)
    _gate("dec-two-level-96x96", image, ref)
    out = vae.decode_images(z)
    assert np.array_equal(_bits(out["image"]), _bits(image)), "sd_vae_decode_images' image differs from sd_vae_decode's"
    rgb8 = (np.clip(image / 2 + 0.5, 0, 1) * 255).round().astype(np.uint8).transpose(0, 2, 3, 1)
    assert np.array_equal(out["rgb8"], rgb8)
    eager = HipVaeDecoder(TWO_LEVEL, sd16, batch=1, latent_height=h, latent_width=w, use_graph=False)
    assert np.array_equal(_bits(eager(z=z)["image"]), _bits(image)), "graph replay and eager launches differ"
    eager.close()
    vae.close()


def test_sd_decoder_at_12x12():
    """The production mid-block width (512) at S = 144."""
    sd16, sd = _decoder_weights(SD)
    z = _latents(1, 12, 12)
    ref = vae_ref.vae_decode(sd, SD, torch.from_numpy(z.astype(np.float32))).numpy()
    vae = HipVaeDecoder(SD, sd16, batch=1, latent_height=12, latent_width=12)
    _gate("dec-sd-12x12", vae(z=z)["image"], ref)
    vae.close()


def test_encoder_on_an_80x80_image():
    """mid-block S = 100: the same builder serves the encoder."""
    sd16 = weights.make_state_dict(vae_ref.vae_encoder_param_shapes(MINI), seed=71, dtype=np.float16, gain=1.4)
    sd = weights.to_torch({k: v.astype(np.float32) for k, v in sd16.items()})
    x = np.tanh(weights.seeded_normal((1, 3, 80, 80), 72)).astype(np.float16)
    ref = vae_ref.vae_encode(sd, MINI, torch.from_numpy(x.astype(np.float32))).numpy()
    outs = []
    for use_graph in (True, False):
        enc = HipVaeEncoder(MINI, sd16, batch=1, height=80, width=80, use_graph=use_graph)
        outs += [enc(x=x)["latent"], enc(x=x)["latent"]]
        enc.close()
    assert outs[0].shape == ref.shape == (1, 8, 10, 10)
    _gate("enc-mini-80x80", outs[0], ref)
    for o in outs[1:]:
        assert np.array_equal(_bits(o), _bits(outs[0])), "graph replay and eager launches differ"


def test_a_mid_block_width_without_a_kernel_is_refused_at_create():
    cfg = dict(latent_channels=4, out_channels=3, block_out_channels=(64, 192), layers_per_block=1)
    sd16, _ = _decoder_weights(cfg)
    with pytest.raises(NotImplementedError, match="mid-block width 192"):
        HipVaeDecoder(cfg, sd16, batch=1, latent_height=10, latent_width=10)


def test_the_materialised_route_is_unchanged_bit_for_bit():
    """The `sd` decoder at 16 x 16 latents (S = 256: the route of every earlier test, golden and benchmark) against the SHA-256 of
    its output as the commit before the streaming kernel computed it (tests/golden/vae_decoder_sd_16x16_sha256.json)."""
    g = json.load(open(os.path.join(GOLDEN, "vae_decoder_sd_16x16_sha256.json")))
    sd16, _ = _decoder_weights(SD, seed=g["weights_seed"])
    z = _latents(1, 16, 16, seed=g["latents_seed"])
    vae = HipVaeDecoder(SD, sd16, batch=1, latent_height=16, latent_width=16)
    image = vae(z=z)["image"]
    vae.close()
    assert image.shape == tuple(g["shape"]) and image.dtype == np.float32
    assert hashlib.sha256(np.ascontiguousarray(image).tobytes()).hexdigest() == g["sha256"]


def test_mini_pipeline_at_768x768(tmp_path):
    """The mini checkpoint end to end where its VAE takes the streaming kernel.  The mini UNet has three stride-2 levels and checks its
    skip connections' shapes, so it accepts latent sides that are multiples of 8 only: every token count it accepts is a multiple of
    64, and the smallest square size that leaves the materialised route is the first above 8192 tokens, 96 x 96 latents = a
    768 x 768 image (SD2.1 768, SDXL 768²).  No Python-side check stands in the way; the image is the oracle decoder's on the
    pipeline's own latents."""
    from python_hip_stable_diffusion import pipeline as P
    from test_text_encoder_gpu import write_checkpoint_dir
    root = str(tmp_path / "mini-sd")
    os.makedirs(root)
    parts, _ = write_checkpoint_dir(root)
    pipe = P.get_hip_pipe(root, "mini/stable-diffusion", attention_implementation="ORIGINAL", guidance_scale=7.5, latent_size=96)
    assert pipe.height == pipe.width == 768
    out = pipe("a photo of an astronaut riding a horse", num_inference_steps=2, guidance_scale=7.5, seed=93)
    assert out.images.shape == (1, 768, 768, 3) and np.isfinite(out.latents).all()
    z16 = (1 / 0.18215 * out.latents).astype(np.float16)                     # decode_latents' own rounding
    img = vae_ref.vae_decode(parts["vae"], MINI, torch.from_numpy(z16.astype(np.float32))).numpy()
    img = np.clip(img / 2 + 0.5, 0, 1).transpose(0, 2, 3, 1)
    _gate("pipeline-mini-96x96", out.images, img)
    pipe.unet.close(), pipe.vae_decoder.close(), pipe.text_encoder.close()
