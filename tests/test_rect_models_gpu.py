"""GPU suite: whole handles at latent sizes with H != W (torch2coreml.py --latent-h / --latent-w converts such models; a 512x1024 or
768x512 image is an ordinary request).  Every expectation is the CPU oracle (oracle/unet_ref.py, oracle/vae_ref.py,
oracle/scheduler_ref.py) on fp32 copies of the same fp16 synthetic weights, computed here: no golden files.

A UNet's latent size must divide by 2^(levels - 1): the reference's nearest-x2 followed by the skip concat cannot do otherwise.
Gates: one forward >= 60 dB (the gate of every single-forward test of this project); the others are the gates of the square tests
of the same handles and are named where they are used."""
import time

import numpy as np
import pytest
import torch

from oracle import psnr, scheduler_ref, unet_ref, vae_ref, weights
from python_hip_stable_diffusion import HipModel, HipVaeDecoder, HipVaeEncoder, _lib, schedulers

pytestmark = pytest.mark.gpu


def t32(a):
    return torch.from_numpy(np.asarray(a).astype(np.float32))


def checkpoint(shapes, seed):
    sd16 = weights.make_state_dict(shapes, seed=seed, dtype=np.float16)
    return sd16, weights.to_torch({k: v.astype(np.float32) for k, v in sd16.items()})


def unet_inputs(cfg, model, b, h, w, seed):
    """fp16 inputs of one forward; the sample carries 0.5 b + 0.1 y + 0.03 x on top of the noise, so that no two images, rows or
    columns look alike to a kernel that swaps H and W"""
    sig = 0.5 * np.arange(b).reshape(b, 1, 1, 1) + 0.1 * np.arange(h).reshape(1, 1, h, 1) + 0.03 * np.arange(w).reshape(1, 1, 1, w)
    kw = dict(sample=(weights.seeded_normal((b, cfg["in_channels"], h, w), seed) + sig).astype(np.float16),
              timestep=np.array([981] * b, np.float16),
              encoder_hidden_states=weights.seeded_normal((b, cfg["cross_attention_dim"], 1, 77), seed + 1).astype(np.float16))
    if cfg["addition_embed_type"] == "text_time":
        kw["time_ids"] = np.array([[8 * h, 8 * w, 0, 0, 8 * h, 8 * w][:model.num_time_ids]] * b, np.float16)
        kw["text_embeds"] = weights.seeded_normal((b, model.text_embed_dim), seed + 2).astype(np.float16)
    return kw


def oracle_unet(sd, cfg, kw, impl="ORIGINAL", residuals=None):
    return unet_ref.unet_forward(sd, cfg, t32(kw["sample"]), t32(kw["timestep"]), t32(kw["encoder_hidden_states"]),
                                 time_ids=t32(kw["time_ids"]) if "time_ids" in kw else None,
                                 text_embeds=t32(kw["text_embeds"]) if "text_embeds" in kw else None,
                                 additional_residuals=residuals, impl=impl).numpy()


# ---------------------------------------------------------------- UNet forward
@pytest.mark.parametrize("size", [(16, 8), (8, 16), (8, 24)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", ["mini", "mini-xl"])
def test_unet_forward_at_rectangular_latents(name, size):
    """mini (four levels) at 8x16 ends in a 1x2 mid block, at 8x24 in 1x3; mini-xl (three levels) in 2x4 / 2x6.  Batch 2, both
    attention forms the reference converts by default."""
    h, w = size
    cfg = unet_ref.CONFIGS[name]
    sd16, sd = checkpoint(unet_ref.unet_param_shapes(cfg), 21)
    model = HipModel(cfg, sd16, batch=2, latent_height=h, latent_width=w, attention_implementation="ORIGINAL")
    assert model.expected_inputs["sample"]["shape"] == (2, 4, h, w)
    kw = unet_inputs(cfg, model, 2, h, w, 300 + h)
    ref = oracle_unet(sd, cfg, kw)
    for impl in ("ORIGINAL", "SPLIT_EINSUM"):
        model.set_attention_implementation(impl)
        got = model(**kw)["noise_pred"]
        assert got.shape == ref.shape == (2, 4, h, w) and np.isfinite(got).all()
        p = psnr.compute_psnr(got, ref)
        print(f"{name} {h}x{w} {impl}: PSNR {p:.1f} dB")
        assert p >= 60.0, f"{name} {h}x{w} {impl}: PSNR {p:.1f} dB vs the oracle"
    with pytest.raises(TypeError, match="shape"):          # the transposed sample: coreml_model.py:97-116
        model(**dict(kw, sample=np.ascontiguousarray(kw["sample"].transpose(0, 1, 3, 2))))
    model.close()


# full channel widths: `mini` (64 .. 256 channels) never reaches the kernels keyed on C = 320 / 640 (gn_proj_qkv, xattn_out, ffn_proj,
# the merged tail, the planner's level-specific rows)
WIDE2 = unet_ref.make_config(sample_size=32, block_out_channels=(320, 640), down_block_types=(unet_ref.CA, unet_ref.CA),
                             up_block_types=(unet_ref.CAUP, unet_ref.CAUP), layers_per_block=1, attention_head_dim=(5, 10),
                             cross_attention_dim=1024)


@pytest.mark.parametrize("size", [(32, 16), (16, 32)], ids=lambda s: "%dx%d" % s)
def test_unet_forward_at_full_channel_widths(size):
    """Two levels of SD2.1's widths (320 with 5 heads, 640 with 10) at 32x16 and 16x32, the second level at 16x8 / 8x16.
    The level-1 resnet convs (3x3, 640 -> 640, batch 2, 16x8) run on the K-split halo kernel (`halo_ks ring4`, plan tile 7, four
    slabs), NOT on the weight-streaming kernel: this test does not cover wstream.hip in situ - tests/test_round5_gpu.py does, at
    the operator.  The planner's answer is asserted so that this sentence stays true.  109 M parameters: checkpoint, handle and oracle
    forward took 1.2 s together on the MI355X machine, so both orientations stay in one parametrised test."""
    h, w = size
    t0 = time.time()
    sd16, sd = checkpoint(unet_ref.unet_param_shapes(WIDE2), 23)
    model = HipModel(WIDE2, sd16, batch=2, latent_height=h, latent_width=w, attention_implementation="ORIGINAL")
    kw = unet_inputs(WIDE2, model, 2, h, w, 400 + h)
    ref = oracle_unet(sd, WIDE2, kw)
    print(f"wide2 {h}x{w}: checkpoint + handle + oracle forward {time.time() - t0:.1f} s")
    got = model(**kw)["noise_pred"]
    assert got.shape == ref.shape == (2, 4, h, w) and np.isfinite(got).all()
    p = psnr.compute_psnr(got, ref)
    print(f"wide2 {h}x{w} ORIGINAL: PSNR {p:.1f} dB")
    assert p >= 60.0, f"wide2 {h}x{w}: PSNR {p:.1f} dB vs the oracle"
    plan = _lib.conv_plan(3, 1, 1, 640, 0, 640, 2, h // 2, w // 2, flags=4 + 16)     # resnet conv2: bias + residual
    assert plan["kernel"] == "halo_ks ring4" and plan["tile"] == 7 and plan["slab"], plan
    model.close()


# ---------------------------------------------------------------- ControlNet
def test_controlnet_and_control_unet_at_16x8():
    """mini-control at 16x8: the ControlNet's 13 residuals (conditioning image 128x64) against the oracle, gate 55 dB as the square
    ControlNet test of tests/test_unet_gpu.py; the control-UNet with the oracle's residuals through the boundary at the single-forward
    gate, and with the ControlNet attached (residuals stay on the device) at 55 dB as tests/test_pipeline2_gpu.py."""
    h, w, b = 16, 8, 2
    cfg = unet_ref.CONFIGS["mini-control"]
    usd16, usd = checkpoint(unet_ref.unet_param_shapes(cfg), 41)
    csd16, csd = checkpoint(unet_ref.controlnet_param_shapes(cfg), 51)
    cn = HipModel(cfg, csd16, kind="controlnet", batch=b, latent_height=h, latent_width=w, attention_implementation="ORIGINAL")
    unet = HipModel(cfg, usd16, batch=b, latent_height=h, latent_width=w, attention_implementation="ORIGINAL")
    assert cn.expected_inputs["controlnet_cond"]["shape"] == (b, 3, 128, 64)
    kw = unet_inputs(cfg, unet, b, h, w, 500)
    cond = np.random.RandomState(60).rand(b, 3, 8 * h, 8 * w).astype(np.float16)
    shapes = unet_ref.residual_shapes(cfg, b, h, w)
    assert shapes[-1] == (b, 256, 2, 1) and len(shapes) == cn.num_residuals == 13
    want = unet_ref.controlnet_forward(csd, cfg, t32(kw["sample"]), t32(kw["timestep"]), t32(kw["encoder_hidden_states"]), t32(cond))
    out = cn(controlnet_cond=cond, **kw)
    for i, s_ in enumerate(shapes):
        got, ref = out[f"additional_residual_{i}"], want[i].numpy()
        assert got.shape == ref.shape == s_ == unet.expected_inputs[f"additional_residual_{i}"]["shape"]
        p = psnr.compute_psnr(got, ref)
        assert np.isfinite(got).all() and p >= 55.0, f"residual {i} {s_}: PSNR {p:.1f} dB"
    res16 = [r.half() for r in want]                                                       # fp16 hand-off (pipeline.py:284)
    ref = oracle_unet(usd, cfg, kw, residuals=[r.float() for r in res16])
    y = unet(**kw, **{f"additional_residual_{i}": r.numpy() for i, r in enumerate(res16)})["noise_pred"]
    p = psnr.compute_psnr(y, ref)
    assert y.shape == (b, 4, h, w) and p >= 60.0, f"control-UNet 16x8, residuals through the boundary: PSNR {p:.1f} dB"
    unet.attach_controlnets([cn])
    cn.set_controlnet_cond(cond)
    y = unet(**kw)["noise_pred"]
    p = psnr.compute_psnr(y, ref)
    assert p >= 55.0, f"control-UNet 16x8, ControlNet attached: PSNR {p:.1f} dB"
    unet.attach_controlnets([])
    unet.close()
    cn.close()


# ---------------------------------------------------------------- device loop
def test_device_loop_at_8x16():
    """mini at 8x16, DDIM, 4 steps, guidance 7.5: the device-resident loop against the host-stepped loop through the same handle
    (>= 45 dB, the figure of tests/test_round2_gpu.py for two HIP paths) and against the oracle loop around the oracle UNet (>= 35 dB,
    the reference's own floor, torch2coreml.py:77).  The measured values stand at the asserts."""
    h, w = 8, 16
    cfg = unet_ref.CONFIGS["mini"]
    sd16, sd = checkpoint(unet_ref.unet_param_shapes(cfg), 21)
    model = HipModel(cfg, sd16, batch=2, latent_height=h, latent_width=w, attention_implementation="SPLIT_EINSUM")
    lat0 = weights.seeded_normal((1, 4, h, w), 93)
    ehs = weights.seeded_normal((2, cfg["cross_attention_dim"], 1, 77), 94).astype(np.float16)
    n_steps, g = 4, 7.5

    def oracle_step(x, ts, e):
        return unet_ref.unet_forward(sd, cfg, t32(x), t32(ts), t32(e)).numpy()

    want = scheduler_ref.denoise_loop(oracle_step, scheduler_ref.DDIM(), lat0, ehs, n_steps, g)
    sch = schedulers.DDIMScheduler()
    sch.set_timesteps(n_steps)
    ts, coef, hist = sch.device_tables()
    lat, ms = model.denoise_loop(lat0 * np.float32(sch.init_noise_sigma), ts, coef, g, history=hist, encoder_hidden_states=ehs)
    assert lat.shape == want.shape == (1, 4, h, w) and len(ms) == n_steps and np.isfinite(lat).all()
    host = scheduler_ref.denoise_loop(lambda x, t, e: model(sample=x, timestep=t, encoder_hidden_states=e)["noise_pred"],
                                      scheduler_ref.DDIM(), lat0, ehs, n_steps, g)
    p_host, p_oracle = psnr.compute_psnr(lat, host), psnr.compute_psnr(lat, want)
    print(f"mini 8x16 device loop: {p_host:.1f} dB vs the host-stepped loop, {p_oracle:.1f} dB vs the oracle loop")
    assert p_host >= 45.0, f"device loop vs host-stepped loop: PSNR {p_host:.1f} dB"      # measured 145.6 (SD_PSNR_LOG)
    assert p_oracle >= 35.0, f"device loop vs oracle loop: PSNR {p_oracle:.1f} dB"         # measured 58.3
    model.close()


# ---------------------------------------------------------------- VAE
def _close32(got, ref, what, rel=2e-4):
    """the fp32-vs-fp32 tolerance of tests/test_vae_f32_gpu.py: summation order only"""
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    err = float(np.abs(got.astype(np.float64) - ref).max())
    bound = rel * float(np.abs(ref).max()) + 1e-6
    assert err <= bound, f"{what}: max|err| {err:.3e} > {bound:.3e} (PSNR {psnr.compute_psnr(got, ref):.1f} dB)"


VAE = vae_ref.VAE_CONFIGS["mini"]


def _vae_weights(shapes, seed, gain):
    sd16 = weights.make_state_dict(shapes, seed=seed, dtype=np.float16, gain=gain)
    return sd16, weights.to_torch({k: v.astype(np.float32) for k, v in sd16.items()})


def _image(b, h, w, seed):
    """an "image" in [-1, 1] whose two samples, rows and columns all differ"""
    sig = 0.3 * np.arange(b).reshape(b, 1, 1, 1) + 0.01 * np.arange(h).reshape(1, 1, h, 1) - 0.007 * np.arange(w).reshape(1, 1, 1, w)
    return np.tanh(weights.seeded_normal((b, 3, h, w), seed) + sig)


def test_vae_decoder_fp16_at_8x16_batch_2():
    """gate: the 68 dB of test_vae_decoder_matches_oracle (tests/test_unet_gpu.py)"""
    b, h, w = 2, 8, 16
    sd16, sd = _vae_weights(vae_ref.vae_decoder_param_shapes(VAE), 61, 1.6)
    z = (weights.seeded_normal((b, 4, h, w), 62) / 0.18215).astype(np.float16)            # pipeline.py:314
    ref = vae_ref.vae_decode(sd, VAE, t32(z)).numpy()
    vae = HipVaeDecoder(VAE, sd16, batch=b, latent_height=h, latent_width=w)
    out = vae(z=z)["image"]
    assert out.shape == ref.shape == (b, 3, 64, 128)
    p = psnr.compute_psnr(out, ref)
    assert p >= 68.0, f"fp16 VAE decoder 8x16 batch 2: PSNR {p:.1f} dB"
    with pytest.raises(TypeError, match="shape"):
        vae(z=np.ascontiguousarray(z.transpose(0, 1, 3, 2)))
    vae.close()


@pytest.mark.parametrize("size", [(64, 96), (96, 64)], ids=lambda s: "%dx%d" % s)
def test_vae_encoder_fp16_at_rectangular_images(size):
    """Three stride-2 downsamplers with the asymmetric F.pad(x, (0, 1, 0, 1)) at H != W.  Gate: the 67 dB of the square encoder test
    (tests/test_round2_gpu.py): the rectangle adds no arithmetic to a pixel's sum."""
    h, w = size
    sd16, sd = _vae_weights(vae_ref.vae_encoder_param_shapes(VAE), 71, 1.4)
    x = _image(1, h, w, 72).astype(np.float16)
    ref = vae_ref.vae_encode(sd, VAE, t32(x)).numpy()
    enc = HipVaeEncoder(VAE, sd16, height=h, width=w)
    out = enc(x=x)["latent"]
    assert out.shape == ref.shape == (1, 8, h // 8, w // 8)
    p = psnr.compute_psnr(out, ref)
    assert p >= 67.0, f"fp16 VAE encoder {h}x{w}: PSNR {p:.1f} dB"
    enc.close()


def test_vae_decoder_fp32_at_8x12_batch_2():
    """the fp32 attention's loop over the batch and the fp32 layout kernels at B > 1 and H != W"""
    b, h, w = 2, 8, 12
    sd16, sd = _vae_weights(vae_ref.vae_decoder_param_shapes(VAE), 61, 1.6)
    z = (weights.seeded_normal((b, 4, h, w), 63) / 0.18215).astype(np.float32)
    ref = vae_ref.vae_decode(sd, VAE, torch.from_numpy(z)).numpy()
    vae = HipVaeDecoder(VAE, sd16, batch=b, latent_height=h, latent_width=w, dtype=np.float32)
    out = vae(z=z)["image"]
    assert out.shape == (b, 3, 64, 96)
    _close32(out, ref, "fp32 VAE decoder 8x12 batch 2")
    assert np.array_equal(out, vae(z=z)["image"])                                         # graph replay
    vae.close()


def test_vae_encoder_fp32_at_40x64_batch_2():
    b, h, w = 2, 40, 64
    sd16, sd = _vae_weights(vae_ref.vae_encoder_param_shapes(VAE), 71, 1.4)
    x = _image(b, h, w, 72).astype(np.float32)
    ref = vae_ref.vae_encode(sd, VAE, torch.from_numpy(x)).numpy()
    enc = HipVaeEncoder(VAE, sd16, batch=b, height=h, width=w, dtype=np.float32)
    out = enc(x=x)["latent"]
    assert out.shape == (b, 8, 5, 8)
    _close32(out, ref, "fp32 VAE encoder 40x64 batch 2")
    enc.close()


# ---------------------------------------------------------------- sizes the levels do not divide
def test_unet_refuses_a_size_its_levels_do_not_divide():
    """mini has four levels: 12 does not divide by 8.  Refused at construction as an invalid argument (ValueError) that names the
    size - not as an internal "concat shape mismatch" from the middle of the build."""
    cfg = unet_ref.CONFIGS["mini"]
    sd16, _ = checkpoint(unet_ref.unet_param_shapes(cfg), 21)
    with pytest.raises(ValueError, match="12x16"):
        HipModel(cfg, sd16, batch=2, latent_height=12, latent_width=16)
    with pytest.raises(ValueError, match="16x12"):
        HipModel(cfg, sd16, batch=2, latent_height=16, latent_width=12)
    HipModel(cfg, sd16, batch=2, latent_height=8, latent_width=16).close()
