"""Progress handler on the GPU: the step kernel's de-noised tap alone (``sd_op_sched_step`` against a float64 restatement), the
handler between two replays of the device-resident loop (``sd_unet_denoise_loop_progress``: previews, stop, re-entry refused) on the
mini UNet, and the pipeline's ``progress_handler`` / ``use_denoised_intermediates`` end to end on the mini UNet and VAE."""
import itertools

import numpy as np
import pytest

from oracle import psnr, unet_ref, vae_ref, weights
from python_hip_stable_diffusion import HipModel, HipVaeDecoder, _lib, schedulers
from python_hip_stable_diffusion.pipeline import HipStableDiffusionPipeline
from test_pipeline_gpu import StubTextEncoder, StubTokenizer

pytestmark = pytest.mark.gpu


# ---- the step kernel alone ----------------------------------------------------------------------------------------------------------
# An output of cfg_sched_step_kernel passes through at most 10 fp32 roundings (guidance: 2, m: 2, the update: 2 + 3 history terms +
# the noise), each relative to a partial sum that the same expression on absolute values bounds: |got - want| <= 16 * 2^-24 * S.
# Contraction into fma only removes roundings.
BOUND = 16.0 * 2.0 ** -24


def step_reference(noise_pred, lat, hist, coef, pred, noise, g, cfg, history):
    """float64 restatement of cfg_sched_step_kernel (csrc/misc.hip): (value, the same expression on absolute values) of the
    latents, the pushed history entry m and the de-noised tap"""
    f = lambda a: np.asarray(a, np.float64)   # noqa: E731
    n_img = lat.shape[0]
    u = f(noise_pred[:n_img])
    eps, eps_s = u, np.abs(u)
    if cfg == 2:
        c = f(noise_pred[n_img:])
        eps, eps_s = u + float(g) * (c - u), np.abs(u) + abs(float(g)) * (np.abs(c) + np.abs(u))
    x = f(lat)
    cx, cm, ch, a, b = float(coef[0]), float(coef[1]), [float(v) for v in coef[2:5]], float(coef[5]), float(coef[6])
    m, m_s = a * x + b * eps, abs(a) * np.abs(x) + abs(b) * eps_s
    new, new_s = cx * x + cm * m, abs(cx) * np.abs(x) + abs(cm) * m_s
    for j in range(history):
        new, new_s = new + ch[j] * f(hist[j]), new_s + abs(ch[j]) * np.abs(f(hist[j]))
    if noise is not None:
        new, new_s = new + f(noise), new_s + np.abs(f(noise))
    den = den_s = None
    if pred is not None:
        den, den_s = float(pred[0]) * x + float(pred[1]) * eps, abs(float(pred[0])) * np.abs(x) + abs(float(pred[1])) * eps_s
        for j in range(history):
            den, den_s = den + float(pred[2 + j]) * f(hist[j]), den_s + abs(float(pred[2 + j])) * np.abs(f(hist[j]))
    return (new, new_s), (m, m_s), (den, den_s)


def within(got, want, scale, what):
    err = np.abs(np.asarray(got, np.float64) - want)
    worst = float((err / np.maximum(scale, 1e-300)).max())
    assert (err <= BOUND * scale).all(), f"{what}: |got - want| = {worst:.3g} * S, bound {BOUND:.3g} * S"


# (1, 16): one partial wave; (3, 1000): a ragged last block; (2, 9216): 18432 elements > the launch's 64 x 256 lanes - the
# grid-stride loop wraps
@pytest.mark.parametrize("n_images,n", [(1, 16), (3, 1000), (2, 9216)])
def test_sched_step_matches_float64_restatement_and_the_tap_changes_nothing(n_images, n):
    rs = np.random.RandomState(n)
    g = np.float32(7.5)
    for cfg, history, flags, with_noise in itertools.product((1, 2), (0, 1, 2, 3), (0, 1), (False, True)):
        noise_pred = rs.randn(cfg * n_images, n).astype(np.float32)
        lat = rs.randn(n_images, n).astype(np.float32)
        hist = rs.randn(history, n_images, n).astype(np.float32) if history else None
        coef = rs.randn(8).astype(np.float32)
        coef[7] = flags
        pred = np.concatenate([rs.randn(5), np.zeros(3)]).astype(np.float32)
        noise = rs.randn(n_images, n).astype(np.float32) if with_noise else None
        what = f"cfg {cfg} history {history} flags {flags} noise {with_noise}"
        plain = _lib.sched_step(noise_pred, lat, coef, g, hist=hist, step_noise=noise)
        tapped = _lib.sched_step(noise_pred, lat, coef, g, hist=hist, step_noise=noise, pred=pred)
        assert plain[3] == 1 and tapped[3] == 1, what               # the step counter; the entry itself refuses a ticket left > 0
        assert plain[2] is None and tapped[2] is not None
        # with the tap: latents, history and step counter bit for bit those without it
        assert np.array_equal(plain[0].view(np.uint32), tapped[0].view(np.uint32)), what
        assert (hist is None and tapped[1] is None) or np.array_equal(plain[1].view(np.uint32), tapped[1].view(np.uint32)), what
        (new, new_s), (m, m_s), (den, den_s) = step_reference(noise_pred, lat, hist, coef, pred, noise, g, cfg, history)
        within(tapped[0], new, new_s, what + ": latents")
        within(tapped[2], den, den_s, what + ": denoised")
        if history and flags == 0:                                  # pushed: [m, hist[0], hist[1]]
            within(tapped[1][0], m, m_s, what + ": pushed history")
            assert np.array_equal(tapped[1][1:], hist[:-1]), what
        elif history:                                               # flags != 0: the history stays as it was
            assert np.array_equal(tapped[1], hist), what


# ---- the handle's loop ----------------------------------------------------------------------------------------------------------------
CFG = unet_ref.CONFIGS["mini"]
HW = CFG["sample_size"]
G, STEPS = 7.5, 5


@pytest.fixture(scope="module")
def nets():
    """mini UNet handles (batch 2: one image under CFG) with the step graph on and off, and the mini VAE decoder; seeded weights as
    tests/test_pipeline_gpu.py build"""
    sd16 = weights.make_state_dict(unet_ref.unet_param_shapes(CFG), seed=21, dtype=np.float16)
    vcfg = vae_ref.VAE_CONFIGS["mini"]
    vsd16 = weights.make_state_dict(vae_ref.vae_decoder_param_shapes(vcfg), seed=61, dtype=np.float16, gain=1.6)
    out = {"vae": HipVaeDecoder(vcfg, vsd16, batch=1, latent_height=HW, latent_width=HW)}
    for graph in (True, False):
        out[graph] = HipModel(CFG, sd16, batch=2, attention_implementation="SPLIT_EINSUM", use_graph=graph)
    yield out
    for m in out.values():
        m.close()


EHS = weights.seeded_normal((2, CFG["cross_attention_dim"], 1, 77), 2).astype(np.float16)
LAT0 = weights.seeded_normal((1, 4, HW, HW), 93).astype(np.float32)


def tables(name):
    s = schedulers.SCHEDULER_MAP[name]()
    s.set_timesteps(STEPS)
    ts, coef, hist = s.device_tables()
    return ts, coef, hist, s.denoised_table()


def run(model, ts, coef, hist, rows=None, state=None, **kw):
    rows = len(ts) if rows is None else rows
    if "pred" in kw and kw["pred"] is not None:
        kw["pred"] = kw["pred"][:rows]
    return model.denoise_loop(LAT0, ts[:rows], coef[:rows], G, history=hist, history_state=state, encoder_hidden_states=EHS, **kw)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("graph", [True, False])
def test_ddim_loop_with_a_handler_is_the_loop_without_one(nets, graph):
    model = nets[graph]
    ts, coef, hist, pred = tables("DDIM")
    assert hist == 0
    base, ms0 = run(model, ts, coef, hist)
    prefixes = [run(model, ts, coef, hist, rows=i + 1)[0] for i in range(STEPS)]
    assert np.array_equal(bits(prefixes[-1]), bits(base))
    for p in (None, pred):
        seen = []
        lat, ms = run(model, ts, coef, hist, pred=p, progress=lambda i, n, x, d: seen.append((i, n, x, d)))
        assert np.array_equal(bits(lat), bits(base)) and len(ms) == STEPS and (ms > 0).all()
        assert [(s[0], s[1]) for s in seen] == [(i, STEPS) for i in range(STEPS)]
        for i, (_, _, x, d) in enumerate(seen):
            assert np.array_equal(bits(x), bits(prefixes[i])), f"latents at step {i}"
            assert (d is None) == (p is None) and (d is None or (d.shape == x.shape and np.isfinite(d).all()))
    thin = []
    run(model, ts, coef, hist, progress=lambda i, n, x, d: thin.append(i), progress_steps=2)
    assert thin == [0, 2, 4]


@pytest.mark.parametrize("graph", [True, False])
def test_dpm_solver_denoised_is_the_history_entry_itself(nets, graph):
    """DPM-Solver++: the de-noised estimate is the converted output m the step pushes, from the same floats"""
    model = nets[graph]
    ts, coef, hist, pred = tables("DPMSolverMultistep")
    assert hist == 1 and np.array_equal(pred[:, :2], coef[:, 5:7])
    seen = []
    full_state = np.zeros((1,) + LAT0.shape, np.float32)
    lat, _ = run(model, ts, coef, hist, pred=pred, state=full_state, progress=lambda i, n, x, d: seen.append((x, d)))
    assert len(seen) == STEPS
    for i, (x, d) in enumerate(seen):
        state = np.zeros((1,) + LAT0.shape, np.float32)
        want, _ = run(model, ts, coef, hist, rows=i + 1, state=state)
        assert np.array_equal(bits(x), bits(want)), f"latents at step {i}"
        assert np.array_equal(d, state[0]), f"denoised at step {i}"
    assert np.array_equal(bits(lat), bits(want)) and np.array_equal(full_state, state)


@pytest.mark.parametrize("graph", [True, False])
def test_stop_at_step_two_and_the_handle_starts_clean(nets, graph):
    model = nets[graph]
    ts, coef, hist, pred = tables("PNDM")                            # history 3, the warm-up row with flags != 0
    first, _ = run(model, ts, coef, hist)
    want_state = np.zeros((3,) + LAT0.shape, np.float32)
    want, _ = run(model, ts, coef, hist, rows=3, state=want_state)
    seen = []
    state = np.zeros((3,) + LAT0.shape, np.float32)

    def stop(i, n, x, d):
        seen.append((i, n, x))
        return i < 2

    lat, ms = run(model, ts, coef, hist, pred=pred, state=state, progress=stop)
    assert [s[0] for s in seen] == [0, 1, 2] and seen[0][1] == STEPS + 1         # PNDM's doubled entry counts
    assert len(ms) == 3 and (ms > 0).all()
    assert np.array_equal(bits(lat), bits(seen[-1][2])) and np.array_equal(bits(lat), bits(want))
    assert np.array_equal(bits(state), bits(want_state))
    again, ms = run(model, ts, coef, hist)
    assert np.array_equal(bits(again), bits(first)) and len(ms) == STEPS + 1


def test_the_handler_may_drive_other_handles_but_not_this_one(nets):
    model, vae = nets[True], nets["vae"]
    ts, coef, hist, pred = tables("DDIM")
    base, _ = run(model, ts, coef, hist)
    sample = np.zeros((2, 4, HW, HW), np.float16)
    images, refused = [], []

    def handler(i, n, x, d):
        with pytest.raises(ValueError, match="sd_unet_denoise_loop_progress") as e:
            model(sample=sample, timestep=np.array([1, 1], np.float16), encoder_hidden_states=EHS)
        refused.append(str(e.value))
        with pytest.raises(ValueError, match="progress handler"):
            run(model, ts, coef, hist)
        images.append(vae(z=(d / 0.18215).astype(np.float16))["image"])

    lat, ms = run(model, ts, coef, hist, pred=pred, progress=handler)
    assert len(refused) == STEPS and all("sd_unet_forward" in r for r in refused)
    assert len(images) == STEPS and all(im.shape == (1, 3, HW * 8, HW * 8) and np.isfinite(im).all() for im in images)
    assert np.array_equal(bits(lat), bits(base)) and len(ms) == STEPS
    model(sample=sample, timestep=np.array([1, 1], np.float16), encoder_hidden_states=EHS)   # behind the loop the handle is free again

    def boom(i, n, x, d):
        raise KeyError("from the handler")

    with pytest.raises(KeyError, match="from the handler"):
        run(model, ts, coef, hist, progress=boom)
    again, _ = run(model, ts, coef, hist)
    assert np.array_equal(bits(again), bits(base))


# ---- the pipeline -------------------------------------------------------------------------------------------------------------------
def test_pipeline_progress_handler_previews_and_stop(nets):
    """The de-noised intermediates of the device loop against the host-stepped loop's: gate 60 dB, the project's gate between its
    two loops (tests/test_pipeline_gpu.py:82).  The PSNR of every step is printed; no value is recorded yet (LAB_NOTES.md, round 18:
    no GPU run)."""
    pipe = HipStableDiffusionPipeline(StubTextEncoder(CFG["cross_attention_dim"]), nets[True], nets["vae"], schedulers.DDIMScheduler(),
                                      StubTokenizer(), force_zeros_for_empty_prompt=False)
    kw = dict(num_inference_steps=4, guidance_scale=G, seed=1)
    plain = pipe("a prompt", **kw)
    assert plain.images.shape == (1, HW * 8, HW * 8, 3) and plain.cancelled is False
    seen = []
    out = pipe("a prompt", progress_handler=seen.append, **kw)
    assert len(out.step_ms) == 4 and np.array_equal(out.images, plain.images) and np.array_equal(out.latents, plain.latents)
    assert [p.step for p in seen] == [0, 1, 2, 3] and {p.step_count for p in seen} == {4}
    assert np.array_equal(seen[-1].current_latent_samples, out.latents)
    assert np.array_equal(seen[-1].current_images, out.images)                  # decoded lazily, by the same decoder
    assert seen[0].current_images.shape == out.images.shape and not np.array_equal(seen[0].current_images, out.images)

    dev, host = [], []
    a = pipe("a prompt", progress_handler=dev.append, use_denoised_intermediates=True, **kw)
    b = pipe("a prompt", progress_handler=host.append, use_denoised_intermediates=True, device_loop=False, **kw)
    assert np.array_equal(a.images, plain.images) and len(a.step_ms) == 4 and b.step_ms is None
    assert len(dev) == len(host) == 4
    for d, h in zip(dev, host):
        assert not np.array_equal(d.current_latent_samples, seen[d.step].current_latent_samples)
        p = psnr.compute_psnr(d.current_latent_samples, h.current_latent_samples)
        print(f"de-noised intermediates, device loop against host-stepped loop, step {d.step}: {p:.1f} dB")
    for d, h in zip(dev, host):                                                 # the project's gate between its two loops
        assert psnr.compute_psnr(d.current_latent_samples, h.current_latent_samples) >= 60.0, d.step

    stopped = []
    c = pipe("a prompt", progress_handler=lambda p: (stopped.append(p), p.step < 1)[1], **kw)
    assert c.images == [] and c.cancelled is True and c.nsfw_content_detected is None and len(c.step_ms) == 2
    assert np.array_equal(c.latents, stopped[-1].current_latent_samples) and np.array_equal(c.latents, seen[1].current_latent_samples)
    last = []                                                                   # a stop behind the LAST step is a stop too
    e = pipe("a prompt", progress_handler=lambda p: (last.append(p), p.step < 3)[1], **kw)
    assert e.images == [] and e.cancelled is True and len(e.step_ms) == 4 and [p.step for p in last] == [0, 1, 2, 3]
    assert np.array_equal(e.latents, plain.latents)
    again = pipe("a prompt", **kw)
    assert np.array_equal(again.images, plain.images)
