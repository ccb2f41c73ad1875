"""One C handle type, three kinds (UNet / ControlNet, VAE decoder, VAE encoder): every entry point that needs one kind refuses
the others with status -1 and a fixed text, and the entry points every kind shares (profile, time_forward, device_bytes,
num_residuals, set_attention) work on a VAE handle.  Pins the behaviour of the C ABI, not of any one class behind it."""
import ctypes as C

import numpy as np
import pytest

from oracle import unet_ref, vae_ref, weights
from python_hip_stable_diffusion import HipModel, HipVaeDecoder, HipVaeEncoder, _lib

pytestmark = pytest.mark.gpu

VCFG = vae_ref.VAE_CONFIGS["mini"]


@pytest.fixture(scope="module")
def handles():
    # support_controlnet: so that attach_controlnets gets as far as looking at the handles in its list
    cfg = dict(unet_ref.CONFIGS["tiny"], support_controlnet=True)
    usd = weights.make_state_dict(unet_ref.unet_param_shapes(cfg), seed=21, dtype=np.float16)
    dsd = weights.make_state_dict(vae_ref.vae_decoder_param_shapes(VCFG), seed=61, dtype=np.float16, gain=1.6)
    esd = weights.make_state_dict(vae_ref.vae_encoder_param_shapes(VCFG), seed=71, dtype=np.float16, gain=1.4)
    h = dict(unet=HipModel(cfg, usd, batch=2),
             dec=HipVaeDecoder(VCFG, dsd, batch=1, latent_height=8, latent_width=8),
             dec32=HipVaeDecoder(VCFG, dsd, batch=1, latent_height=8, latent_width=8, dtype=np.float32),
             enc=HipVaeEncoder(VCFG, esd, batch=1, height=64, width=64))
    yield h
    for m in h.values():
        m.close()


def refused(status, text):
    assert status == -1, status
    assert text.encode() in _lib.lib().sd_last_error(), _lib.lib().sd_last_error()


BUF = np.zeros(3 * 64 * 64, np.float32)      # large enough for every argument below; a refusal touches none of them


@pytest.mark.parametrize("wrong", ["dec", "dec32", "enc"])
def test_unet_forward_refuses_vae_handles(handles, wrong):
    io = _lib.UNetIO()
    refused(_lib.lib().sd_unet_forward(handles[wrong]._h, C.byref(io)), "use sd_vae_decode")


def test_denoise_loop_refuses_a_decoder(handles):
    io = _lib.UNetIO()
    f = _lib.fptr(BUF)
    refused(_lib.lib().sd_unet_denoise_loop(handles["dec"]._h, C.byref(io), f, 1, 1, f, f, None, 0, 1.0, None, None),
            "needs a UNet handle")


def test_attach_controlnets_refuses_a_decoder_on_either_side(handles):
    lib = _lib.lib()
    refused(lib.sd_unet_attach_controlnets(handles["dec"]._h, None, 0), "needs a UNet handle")
    arr = (C.c_void_p * 1)(handles["dec"]._h)
    refused(lib.sd_unet_attach_controlnets(handles["unet"]._h, C.cast(arr, C.POINTER(C.c_void_p)), 1), "not a ControlNet")


def test_controlnet_set_cond_refuses_a_decoder(handles):
    refused(_lib.lib().sd_controlnet_set_cond(handles["dec"]._h, _lib.ptr(BUF), 0), "needs a ControlNet handle")


@pytest.mark.parametrize("wrong", ["unet", "enc"])
def test_vae_decode_refuses_other_kinds(handles, wrong):
    refused(_lib.lib().sd_vae_decode(handles[wrong]._h, _lib.ptr(BUF), 1, _lib.fptr(BUF), 0), "not a VAE decoder")


@pytest.mark.parametrize("wrong", ["unet", "dec", "dec32"])
def test_vae_encode_refuses_other_kinds(handles, wrong):
    refused(_lib.lib().sd_vae_encode(handles[wrong]._h, _lib.ptr(BUF), 1, _lib.fptr(BUF), 0), "not a VAE encoder")


@pytest.mark.parametrize("kind,dtype", [("dec", np.float16), ("dec32", np.float32)])
def test_shared_entry_points_on_a_decoder(handles, kind, dtype):
    """The handle is still fresh here (a refusal never gets as far as a decode): timing and profile need one forward first."""
    dec, lib = handles[kind], _lib.lib()
    ms, n = C.c_float(0), C.c_int(0)
    refused(lib.sd_unet_time_forward(dec._h, 1, 1, C.byref(ms)), "once first")
    refused(lib.sd_unet_profile(dec._h, 1, 0, None, None, None, 0, C.byref(n)), "once first")
    z = weights.seeded_normal((1, 4, 8, 8), 62).astype(dtype)
    first = dec(z=z)["image"]
    assert first.shape == (1, 3, 64, 64) and np.isfinite(first).all()
    ops = dec.profile(iters=1)
    assert len(ops) >= 1 and all(label for label, _, _ in ops)
    assert ops[-1][0] == "conv3x3 small-N decoder.conv_out -> fp32 NCHW"
    assert dec.time_forward(warmup=1, iters=2) > 0
    assert dec.device_bytes > 0
    assert lib.sd_unet_num_residuals(dec._h) == 0
    assert lib.sd_unet_set_attention(dec._h, 3) == -1                         # still validated ...
    assert lib.sd_unet_set_attention(dec._h, 2) == 0                          # ... accepted, and without effect on a VAE
    assert np.array_equal(dec(z=z)["image"], first)
