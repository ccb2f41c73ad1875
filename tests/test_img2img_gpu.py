"""Image-to-image on the GPU: the posterior-sample + add-noise kernel (csrc/misc.hip posterior_noise_kernel) against a float64
restatement of Encoder.swift:68-89 + Scheduler.swift:83-102, ``sd_vae_encode_latents`` against that kernel applied to the
handle's own moments, and the pipeline's ``starting_image`` / ``strength`` path on the mini UNet + mini VAE."""
import numpy as np
import pytest
import torch

from oracle import psnr, unet_ref, vae_ref, weights
from python_hip_stable_diffusion import HipModel, HipVaeDecoder, HipVaeEncoder, _lib, schedulers
from python_hip_stable_diffusion.pipeline import HipStableDiffusionPipeline
from test_pipeline_gpu import StubTextEncoder, StubTokenizer

pytestmark = pytest.mark.gpu


def posterior_noise_f64(moments, eps, noise, scale, sa, sb):
    """The three formula lines in float64 on the float32 inputs; also the fp32 error bound of the issue:
    1e-5 * (|sa * scale| * (|mean| + std * |eps|) + |sb * noise|) + 1e-30 - about ten times a handful of fp32 roundings plus
    a 2-ulp expf, relative to the magnitudes that enter the sums (a plain rtol is wrong where the two terms cancel)."""
    cz = moments.shape[-3] // 2
    m = moments.reshape((2 * cz,) + moments.shape[-2:]).astype(np.float64)
    mean, logvar = m[:cz], np.clip(m[cz:], -30.0, 20.0)                       # Encoder.swift:68-73
    std = np.exp(0.5 * logvar)                                                # :74-77
    scale, sa, sb = (float(np.float32(v)) for v in (scale, sa, sb))           # what crosses the ABI
    e, nz = eps.astype(np.float64), noise.astype(np.float64)
    z = (mean + std * e) * scale                                              # :78-89
    ref = sa * z[None] + sb * nz                                              # Scheduler.swift:83-102
    bound = 1e-5 * (abs(sa * scale) * (np.abs(mean) + std * np.abs(e))[None] + np.abs(sb * nz)) + 1e-30
    return ref, bound


def make_inputs(cz, h, w, n_images, seed):
    rs = np.random.RandomState(seed)
    mean = rs.randn(cz, h, w).astype(np.float32) * 3
    logvar = rs.uniform(-40.0, 25.0, (cz, h, w)).astype(np.float32)           # both clamps are hit
    logvar.reshape(-1)[:2] = (-40.0, 25.0)
    return (np.concatenate([mean, logvar]), rs.randn(cz, h, w).astype(np.float32),
            rs.randn(n_images, cz, h, w).astype(np.float32))


@pytest.mark.parametrize("cz,h,w,n_images", [(4, 2, 2, 1),      # 16 elements: below one wave, vector form
                                             (4, 5, 3, 3),      # 60 elements: ragged last wave, three images
                                             (3, 7, 5, 2),      # 105 elements: odd everything, the scalar form
                                             (4, 64, 64, 2)])   # the product size: 64 workgroups
def test_posterior_noise_kernel_matches_float64_restatement(cz, h, w, n_images):
    moments, eps, noise = make_inputs(cz, h, w, n_images, seed=cz * 1000 + h * 10 + n_images)
    assert moments[cz:].min() < -30 and moments[cz:].max() > 20
    scale, sa, sb = 0.18215, 0.6331, 0.7741
    got, _ = _lib.posterior_noise(moments, eps, noise, scale, sa, sb)
    ref, bound = posterior_noise_f64(moments, eps, noise, scale, sa, sb)
    assert got.shape == noise.shape and got.dtype == np.float32 and np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ref)
    print(f"posterior_noise {(cz, h, w, n_images)}: max err / bound = {(err / bound).max():.4f}")
    assert (err <= bound).all(), float((err / bound).max())
    again, ms = _lib.posterior_noise(moments, eps, noise, scale, sa, sb, iters=3)
    assert np.array_equal(again, got) and ms > 0                              # nothing order-dependent
    # sa = 1, sb = 0, eps = 0: the scaled mean
    got0, _ = _lib.posterior_noise(moments, np.zeros_like(eps), noise, scale, 1.0, 0.0)
    ref0, bound0 = posterior_noise_f64(moments, np.zeros_like(eps), noise, scale, 1.0, 0.0)
    want0 = moments[:cz].astype(np.float64) * float(np.float32(scale))
    assert np.array_equal(ref0, np.broadcast_to(want0, ref0.shape))
    assert (np.abs(got0.astype(np.float64) - ref0) <= bound0).all()


def test_posterior_noise_argument_checks():
    moments, eps, noise = make_inputs(4, 2, 2, 1, seed=1)
    with pytest.raises(ValueError):
        _lib.posterior_noise(moments[:6], eps, noise, 1.0, 1.0, 1.0)
    with pytest.raises(ValueError):
        _lib.posterior_noise(moments, eps, noise[0], 1.0, 1.0, 1.0)


# ---- handle level ------------------------------------------------------------------------------------------------------------
VCFG = vae_ref.VAE_CONFIGS["mini"]


def encoder_weights():
    return weights.make_state_dict(vae_ref.vae_encoder_param_shapes(VCFG), seed=71, dtype=np.float16, gain=1.4)


@pytest.mark.parametrize("use_graph", [0, 1])
@pytest.mark.parametrize("dtype,hw", [(np.float16, 64), (np.float32, 32)])
def test_encode_latents_is_the_kernel_on_the_handle_s_own_moments(dtype, hw, use_graph):
    """32x32 images on the fp32 handle; the fp16 handle's single-head attention kernel needs a multiple of 64 tokens (the library
    refuses to build it below), so its smallest image is 64x64 = 8x8 latents."""
    n_images = 3
    enc = HipVaeEncoder(VCFG, encoder_weights(), batch=1, height=hw, width=hw, use_graph=bool(use_graph), dtype=dtype)
    x = np.tanh(weights.seeded_normal((1, 3, hw, hw), 72)).astype(dtype)
    rs = np.random.RandomState(4)
    eps = rs.randn(4, hw // 8, hw // 8).astype(np.float32)
    noise = rs.randn(n_images, 4, hw // 8, hw // 8).astype(np.float32)
    scale, sa, sb = 0.18215, 0.81, 0.59
    moments = enc(x=x)["latent"]
    assert moments.shape == (1, 8, hw // 8, hw // 8)
    before = enc.device_bytes
    got = enc.encode_latents(x, eps, noise, scale, sa, sb)
    want, _ = _lib.posterior_noise(moments, eps, noise, scale, sa, sb)
    assert got.shape == (n_images, 4, hw // 8, hw // 8) and got.dtype == np.float32
    assert np.array_equal(got, want)
    ref, bound = posterior_noise_f64(moments, eps, noise, scale, sa, sb)
    assert (np.abs(got.astype(np.float64) - ref) <= bound).all()
    assert np.array_equal(enc(x=x)["latent"], moments)                        # the moments are still the encoder's output
    assert np.array_equal(enc.encode_latents(x, eps, noise, scale, sa, sb), got)
    assert np.array_equal(enc.encode_latents(x, eps, noise[:1], scale, sa, sb), got[:1])     # one image: the first of three
    assert enc.device_bytes >= before
    with pytest.raises(TypeError):
        enc.encode_latents(x, eps.astype(np.float64), noise, scale, sa, sb)
    with pytest.raises(TypeError):
        enc.encode_latents(x, eps[:2], noise, scale, sa, sb)
    with pytest.raises(TypeError):
        enc.encode_latents(x.astype(np.float64), eps, noise, scale, sa, sb)
    enc.close()


def test_encode_latents_refuses_other_handles_before_any_device_work():
    import ctypes as C
    vsd = weights.make_state_dict(vae_ref.vae_decoder_param_shapes(VCFG), seed=61, dtype=np.float16, gain=1.6)
    dec = HipVaeDecoder(VCFG, vsd, batch=1, latent_height=8, latent_width=8)
    buf = np.zeros(4 * 8 * 8, np.float32)
    lib = _lib.lib()
    x = np.zeros((1, 3, 64, 64), np.float16)
    assert lib.sd_vae_encode_latents(dec._h, _lib.ptr(x), 0, _lib.fptr(buf), _lib.fptr(buf), 1, 1.0, 1.0, 1.0, _lib.fptr(buf), 0) == -1
    assert b"not a VAE encoder" in lib.sd_last_error()
    enc = HipVaeEncoder(VCFG, encoder_weights(), batch=1, height=64, width=64)
    assert lib.sd_vae_encode_latents(enc._h, _lib.ptr(x), 0, _lib.fptr(buf), _lib.fptr(buf), 0, 1.0, 1.0, 1.0, _lib.fptr(buf), 0) == -1
    assert lib.sd_vae_encode_latents(enc._h, _lib.ptr(x), 0, None, _lib.fptr(buf), 1, 1.0, 1.0, 1.0, _lib.fptr(buf), 0) == -1
    assert lib.sd_vae_encode_latents(C.c_void_p(), _lib.ptr(x), 0, _lib.fptr(buf), _lib.fptr(buf), 1, 1.0, 1.0, 1.0, _lib.fptr(buf), 0) == -1
    dec.close(), enc.close()


# ---- pipeline ------------------------------------------------------------------------------------------------------------------
PROMPT, SEED, STEPS, STRENGTH = "a watercolour of a lighthouse", 93, 6, 0.5


@pytest.fixture(scope="module")
def pipe():
    """tests/test_pipeline_gpu.py:37-47 plus the encoder"""
    cfg = unet_ref.CONFIGS["mini"]
    sd16 = weights.make_state_dict(unet_ref.unet_param_shapes(cfg), seed=21, dtype=np.float16)
    vsd16 = weights.make_state_dict(vae_ref.vae_decoder_param_shapes(VCFG), seed=61, dtype=np.float16, gain=1.6)
    hw = cfg["sample_size"]
    unet = HipModel(cfg, sd16, batch=2, attention_implementation="SPLIT_EINSUM")
    vae = HipVaeDecoder(VCFG, vsd16, batch=1, latent_height=hw, latent_width=hw)
    enc = HipVaeEncoder(VCFG, encoder_weights(), batch=1, height=hw * 8, width=hw * 8)
    p = HipStableDiffusionPipeline(StubTextEncoder(cfg["cross_attention_dim"]), unet, vae, schedulers.DDIMScheduler(),
                                   StubTokenizer(), force_zeros_for_empty_prompt=False, vae_encoder=enc)
    yield p
    for m in (unet, vae, enc):
        m.close()


def starting_image(hw=128):
    return np.tanh(weights.seeded_normal((3, hw, hw), 73)).astype(np.float32)


@pytest.mark.parametrize("name,tail", [("DDIM", 3), ("PNDM", 4)])
def test_pipeline_image_to_image(pipe, name, tail):
    pipe.scheduler = schedulers.SCHEDULER_MAP[name]()
    kw = dict(num_inference_steps=STEPS, guidance_scale=7.5, seed=SEED, output_type="latent")
    img = starting_image()
    a = pipe(PROMPT, starting_image=img, strength=STRENGTH, **kw)
    assert a.step_ms is not None and len(a.step_ms) == tail and np.isfinite(a.images).all()      # the device loop ran the tail
    host = pipe(PROMPT, starting_image=img, strength=STRENGTH, device_loop=False, **kw)
    assert host.step_ms is None
    p = psnr.compute_psnr(host.images, a.images)
    print(f"image-to-image {name}: device loop vs host-stepped loop {p:.1f} dB")
    assert p >= 60.0                                                          # the gate of tests/test_pipeline_gpu.py:82
    assert np.array_equal(host.init_latents, a.init_latents)
    b = pipe(PROMPT, starting_image=img, strength=STRENGTH, **kw)
    assert np.array_equal(a.images, b.images)                                 # same seed: bit for bit
    c = pipe(PROMPT, starting_image=img, strength=0.7, **kw)
    assert len(c.step_ms) == tail + 1 and not np.array_equal(a.images, c.images)
    t2i = pipe(PROMPT, **kw)
    assert len(t2i.step_ms) == STEPS + (name == "PNDM") and not np.array_equal(a.images, t2i.images)
    full = pipe(PROMPT, starting_image=img, strength=1.0, **kw)               # Configuration.swift:74-80: text-to-image
    assert np.array_equal(full.images, t2i.images) and np.array_equal(full.init_latents, t2i.init_latents)


# measured on an MI355X: 108.60 dB (LAB_NOTES.md round 13; the noise term sb * noise carries the peak, the encoder's fp16 error
# enters scaled by sa * 0.18215); gate = measured - 6 dB
INIT_LATENTS_MEASURED_DB = 108.60
INIT_LATENTS_GATE_DB = 102.6


def test_pipeline_starting_latents_match_an_independent_chain(pipe):
    """The starting latents of the image-to-image call against: the oracle encoder in fp32 torch (oracle/vae_ref.py), the
    float64 restatement above, numpy's own seeded stream split [noise | posterior normals], and the add-noise coefficients
    from alphas_cumprod restated here.  Gate = measured - 6 dB; the moments alone pass >= 67 dB against the reference-block
    golden (tests/test_round5_gpu.py), the sampled latents cannot be better than they are."""
    pipe.scheduler = schedulers.DDIMScheduler()
    img = starting_image()
    out = pipe(PROMPT, starting_image=img, strength=STRENGTH, num_inference_steps=STEPS, guidance_scale=7.5, seed=SEED,
               output_type="latent")
    sd = weights.to_torch({k: v.astype(np.float32) for k, v in encoder_weights().items()})
    x16 = img[None].astype(np.float16)                                        # the encoder handle's declared input dtype
    moments = vae_ref.vae_encode(sd, VCFG, torch.from_numpy(x16.astype(np.float32))).numpy()
    np.random.seed(SEED)
    n_noise = 4 * 16 * 16
    stream = np.random.randn(2 * n_noise)
    noise, eps = stream[:n_noise].reshape(1, 4, 16, 16), stream[n_noise:].reshape(4, 16, 16)
    betas = np.linspace(np.float32(0.00085) ** 0.5, np.float32(0.012) ** 0.5, 1000, dtype=np.float32) ** 2
    acp = np.cumprod(1 - betas, dtype=np.float32).astype(np.float64)
    t_start = (np.arange(STEPS) * (1000 // STEPS))[::-1][3] + 1               # DDIM "leading", steps_offset 1; start = 6 - int(3.0)
    assert t_start == 333
    ref, _ = posterior_noise_f64(moments[0], eps.astype(np.float32), noise.astype(np.float32), 0.18215, acp[t_start] ** 0.5,
                                 (1 - acp[t_start]) ** 0.5)
    assert out.init_latents.shape == ref.shape == (1, 4, 16, 16)
    p = psnr.compute_psnr(out.init_latents, ref)
    print(f"image-to-image starting latents vs the independent chain: {p:.2f} dB (measured {INIT_LATENTS_MEASURED_DB}, "
          f"gate {INIT_LATENTS_GATE_DB})")
    assert p >= INIT_LATENTS_GATE_DB, p
