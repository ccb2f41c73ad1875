"""fp32 compute path of the VAE graphs: the reference converts an SDXL checkpoint's own VAE with
float32 inputs and FLOAT32 compute precision because its activations leave the fp16 range (torch2coreml.py:570-578 decoder,
:726-733 encoder), and the pipeline reads the dtype off the model (pipeline.py:315).  HipVaeDecoder / HipVaeEncoder(dtype=
np.float32) run the same graph on fp32 kernels.  Oracle: oracle/vae_ref.py (torch fp32; PARITY UNPINNED - diffusers absent).
Tolerance: fp32 vs fp32, max |err| <= 2e-4 * max|ref| (summation order only)."""
import numpy as np
import pytest
import torch

from oracle import psnr, vae_ref, weights
from python_hip_stable_diffusion import HipVaeDecoder, HipVaeEncoder

pytestmark = pytest.mark.gpu


def _close32(got, ref, what, rel=2e-4):
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    err = float(np.abs(got.astype(np.float64) - ref).max())
    bound = rel * float(np.abs(ref).max()) + 1e-6
    assert err <= bound, f"{what}: max|err| {err:.3e} > {bound:.3e} (PSNR {psnr.compute_psnr(got, ref):.1f} dB)"


@pytest.mark.parametrize("name,hw", [("mini", 8), ("mini", 12), ("sd", 32)])
def test_vae_decoder_fp32_matches_oracle(name, hw):
    cfg = vae_ref.VAE_CONFIGS[name]
    sd16 = weights.make_state_dict(vae_ref.vae_decoder_param_shapes(cfg), seed=61, dtype=np.float16, gain=1.6)
    sd = weights.to_torch({k: v.astype(np.float32) for k, v in sd16.items()})
    vae = HipVaeDecoder(cfg, sd16, batch=1, latent_height=hw, latent_width=hw, dtype=np.float32)
    assert vae.expected_inputs["z"]["dtype"] == np.float32                       # what pipeline.py:315 reads
    z = (weights.seeded_normal((1, 4, hw, hw), 63) / 0.18215).astype(np.float32)
    out = vae(z=z)["image"]
    ref = vae_ref.vae_decode(sd, cfg, torch.from_numpy(z)).numpy()
    _close32(out, ref, f"fp32 VAE decoder {name} @{hw}")
    assert np.array_equal(out, vae(z=z)["image"])                                # graph replay is deterministic
    with pytest.raises(TypeError):
        vae(z=z.astype(np.float16))                                              # the declared dtype is enforced (coreml_model.py:104-108)
    vae.close()


def test_vae_decoder_fp32_survives_activations_beyond_the_fp16_range():
    """The reason the path exists: scale conv_in so that the trunk carries values ~1e6 (every GroupNorm renormalises them, so
    the image is ordinary).  The fp16-storage handle overflows to inf / NaN, the fp32 handle matches the oracle."""
    cfg = vae_ref.VAE_CONFIGS["mini"]
    sd16 = weights.make_state_dict(vae_ref.vae_decoder_param_shapes(cfg), seed=61, dtype=np.float16, gain=1.6)
    sd16 = dict(sd16)
    sd16["decoder.conv_in.weight"] = (sd16["decoder.conv_in.weight"].astype(np.float32) * 2.0e3).astype(np.float16)
    sd = weights.to_torch({k: v.astype(np.float32) for k, v in sd16.items()})
    hw = 8
    z = (weights.seeded_normal((1, 4, hw, hw), 64) * 200.0).astype(np.float32)
    ref = vae_ref.vae_decode(sd, cfg, torch.from_numpy(z)).numpy()
    assert np.isfinite(ref).all() and np.abs(ref).max() < 1e3
    f32 = HipVaeDecoder(cfg, sd16, batch=1, latent_height=hw, latent_width=hw, dtype=np.float32)
    out = f32(z=z)["image"]
    _close32(out, ref, "fp32 VAE decoder with a 1e6-scale trunk", rel=1e-3)
    f16 = HipVaeDecoder(cfg, sd16, batch=1, latent_height=hw, latent_width=hw)
    bad = f16(z=z.astype(np.float16))["image"]
    assert (not np.isfinite(bad).all()) or psnr.compute_psnr(bad, ref) < 20.0   # the fp16-storage path cannot represent the trunk
    f32.close(), f16.close()


@pytest.mark.parametrize("name,hw", [("mini", 64), ("mini", 40)])
def test_vae_encoder_fp32_matches_oracle(name, hw):
    cfg = vae_ref.VAE_CONFIGS[name]
    sd16 = weights.make_state_dict(vae_ref.vae_encoder_param_shapes(cfg), seed=71, dtype=np.float16, gain=1.4)
    sd = weights.to_torch({k: v.astype(np.float32) for k, v in sd16.items()})
    enc = HipVaeEncoder(cfg, sd16, batch=1, height=hw, width=hw, dtype=np.float32)
    x = np.tanh(weights.seeded_normal((1, 3, hw, hw), 72)).astype(np.float32)
    out = enc(x=x)["latent"]
    ref = vae_ref.vae_encode(sd, cfg, torch.from_numpy(x)).numpy()
    _close32(out, ref, f"fp32 VAE encoder {name} @{hw}")
    enc.close()


def test_vae_fp32_handle_keeps_fp32_weights():
    """An fp32 checkpoint (an SDXL VAE is shipped in fp32) must not be rounded to fp16 on upload: weights that are
    NOT fp16-representable, against the oracle on the same fp32 weights - within the fp32 tolerance, which fp16-rounded weights
    (2^-11 relative per weight) miss by an order of magnitude."""
    cfg = vae_ref.VAE_CONFIGS["mini"]
    sd32 = weights.make_state_dict(vae_ref.vae_decoder_param_shapes(cfg), seed=67, dtype=np.float32, gain=1.6)
    assert any(not np.array_equal(v, v.astype(np.float16).astype(np.float32)) for v in sd32.values())
    sd = weights.to_torch(sd32)
    hw = 8
    z = (weights.seeded_normal((1, 4, hw, hw), 68) / 0.18215).astype(np.float32)
    ref = vae_ref.vae_decode(sd, cfg, torch.from_numpy(z)).numpy()
    vae = HipVaeDecoder(cfg, sd32, batch=1, latent_height=hw, latent_width=hw, dtype=np.float32)
    _close32(vae(z=z)["image"], ref, "fp32 VAE decoder with fp32 (not fp16-representable) weights")
    vae.close()
    # the same checkpoint rounded to fp16 first is measurably further away: the test would notice a rounding upload
    sd16 = weights.to_torch({k: v.astype(np.float16).astype(np.float32) for k, v in sd32.items()})
    rounded = vae_ref.vae_decode(sd16, cfg, torch.from_numpy(z)).numpy()
    assert np.abs(rounded - ref).max() > 2e-4 * np.abs(ref).max()


def _conv_out_checkpoint(shapes, prefix, seed, gain):
    """An fp32 checkpoint whose conv_out.weight is 1e-5 * randn - fp16's subnormal range, where rounding a weight to fp16 costs
    2^-25 absolute, 1.7e-3 of the weight's scale - and (the same values) with that one tensor rounded to fp16.  conv_out.bias is
    zero and conv_norm_out's affine is scaled by 1e3, so that conv_out's own product carries the output: with the stock bias and
    unit-scale activations the output is the bias to within 1e-3, and no rounding of the weights could reach _close32's bound."""
    sd32 = dict(weights.make_state_dict(shapes, seed=seed, dtype=np.float32, gain=gain))
    key = prefix + "conv_out.weight"
    sd32[key] = (1e-5 * weights.seeded_normal(sd32[key].shape, seed + 2)).astype(np.float32)
    sd32[prefix + "conv_out.bias"] = np.zeros_like(sd32[prefix + "conv_out.bias"])
    for name in ("conv_norm_out.weight", "conv_norm_out.bias"):
        sd32[prefix + name] = (sd32[prefix + name] * np.float32(1e3)).astype(np.float32)
    rounded = dict(sd32)
    rounded[key] = sd32[key].astype(np.float16).astype(np.float32)
    assert not np.array_equal(rounded[key], sd32[key])
    return sd32, rounded


def _assert_rounding_conv_out_shows(ref, rounded, what):
    """The precondition, on the oracle itself: conv_out.weight rounded to fp16 misses the fp32 result by >= 5 x _close32's bound."""
    gap = float(np.abs(rounded - ref).max())
    bound = 2e-4 * float(np.abs(ref).max()) + 1e-6
    print(f"{what}: fp16-rounded conv_out.weight is {gap:.3e} away, {gap / bound:.1f} x the bound {bound:.3e}")
    assert gap >= 5.0 * bound, f"{what}: rounding conv_out.weight moves the oracle by {gap:.3e}, under 5 x the bound {bound:.3e}"


def test_vae_decoder_fp32_keeps_conv_out_weights_fp32():
    """decoder.conv_out runs through Net::conv_small_n, not Net::conv: an fp32 handle must give it fp32 weights like every other conv."""
    cfg = vae_ref.VAE_CONFIGS["mini"]
    sd32, rounded = _conv_out_checkpoint(vae_ref.vae_decoder_param_shapes(cfg), "decoder.", 67, 1.6)
    hw = 8
    z = (weights.seeded_normal((1, 4, hw, hw), 68) / 0.18215).astype(np.float32)
    ref = vae_ref.vae_decode(weights.to_torch(sd32), cfg, torch.from_numpy(z)).numpy()
    _assert_rounding_conv_out_shows(ref, vae_ref.vae_decode(weights.to_torch(rounded), cfg, torch.from_numpy(z)).numpy(), "mini decoder")
    vae = HipVaeDecoder(cfg, sd32, batch=1, latent_height=hw, latent_width=hw, dtype=np.float32)
    _close32(vae(z=z)["image"], ref, "fp32 VAE decoder with a conv_out.weight in fp16's subnormal range")
    vae.close()


def test_vae_encoder_fp32_keeps_conv_out_weights_fp32():
    cfg = vae_ref.VAE_CONFIGS["mini"]
    sd32, rounded = _conv_out_checkpoint(vae_ref.vae_encoder_param_shapes(cfg), "encoder.", 71, 1.4)
    hw = 40
    x = np.tanh(weights.seeded_normal((1, 3, hw, hw), 72)).astype(np.float32)
    ref = vae_ref.vae_encode(weights.to_torch(sd32), cfg, torch.from_numpy(x)).numpy()
    _assert_rounding_conv_out_shows(ref, vae_ref.vae_encode(weights.to_torch(rounded), cfg, torch.from_numpy(x)).numpy(), "mini encoder")
    enc = HipVaeEncoder(cfg, sd32, batch=1, height=hw, width=hw, dtype=np.float32)
    _close32(enc(x=x)["latent"], ref, "fp32 VAE encoder with a conv_out.weight in fp16's subnormal range")
    enc.close()
