"""Host-side checks of the VAE's streaming mid-block attention (csrc/vae_attention.hip behind sd_op_vae_attention): the symbol, the
order of its refusals - all of them made before any device work, so they come back the same with and without a GPU - and the
kernel's register budget as the compiler reports it."""
import ctypes as C
import os

import numpy as np
import pytest

SD_ERR_INVALID_ARGUMENT, SD_ERR_UNSUPPORTED = -1, -4


def _call(sdlib, q, k, v, out, B, S, Cn):
    ms = C.c_float(0)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    st = sdlib.sd_op_vae_attention(p(q), p(k), p(v), p(out), B, S, Cn, 1, C.byref(ms))
    return st, sdlib.sd_last_error().decode()


def test_symbol_is_exported_and_declared(sdlib):
    from python_hip_stable_diffusion import _lib
    assert hasattr(sdlib, "sd_op_vae_attention")
    assert "sd_op_vae_attention" in [s[0] for s in _lib.SYMBOLS]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "sd_mi355x.h")).read()
    assert "int sd_op_vae_attention(const void* q, const void* k, const void* v, void* out, int B, int S, int C, int iters, float* ms);" in header


def test_refusals_come_in_the_stated_order_before_any_device_work(sdlib):
    a = np.zeros(2 * 4 * 64, np.float16)
    for args in ((None, a, a, a), (a, None, a, a), (a, a, None, a), (a, a, a, None)):                  # NULL
        st, _ = _call(sdlib, *args, 1, 4, 64)
        assert st == SD_ERR_INVALID_ARGUMENT
    for B, S, Cn in ((0, 4, 64), (1, 0, 64), (1, 4, 0), (-1, 4, 64), (1, -3, 64), (1, 4, -64)):       # empty
        st, _ = _call(sdlib, a, a, a, a, B, S, Cn)
        assert st == SD_ERR_INVALID_ARGUMENT, (B, S, Cn)
    for Cn in (1, 32, 96, 192, 320, 384, 1024):                                                       # a head dim the kernel is not built for
        st, msg = _call(sdlib, a, a, a, a, 1, 1, Cn)
        assert st == SD_ERR_UNSUPPORTED and "head dim %d" % Cn in msg, (Cn, st, msg)
    # the order: an invalid argument is reported before an unsupported head dim
    st, _ = _call(sdlib, None, a, a, a, 1, 4, 96)
    assert st == SD_ERR_INVALID_ARGUMENT
    st, _ = _call(sdlib, a, a, a, a, 0, 4, 96)
    assert st == SD_ERR_INVALID_ARGUMENT


def test_wrapper_checks_shapes_and_maps_the_statuses(sdlib):
    from python_hip_stable_diffusion import _lib
    z = np.zeros((1, 4, 64), np.float16)
    with pytest.raises(ValueError):
        _lib.vae_attention(z, z, np.zeros((1, 5, 64), np.float16))
    with pytest.raises(ValueError):
        _lib.vae_attention(z[0], z[0], z[0])
    with pytest.raises(ValueError):
        _lib.vae_attention(z, z, z, out=np.zeros(8, np.float16))
    with pytest.raises(NotImplementedError, match="head dim 96"):
        _lib.vae_attention(*(np.zeros((1, 4, 96), np.float16),) * 3)
    if sdlib.sd_device_count() <= 0:                     # a valid problem: only the machine decides, never a computation on the host
        with pytest.raises(RuntimeError, match="no HIP device"):
            _lib.vae_attention(z, z, z)


def test_kernel_compiles_for_gfx950_without_scratch(tmp_path):
    from test_build_isa import CSRC, HIPCC, kernel_resources
    assert os.path.exists(HIPCC), "hipcc not installed"
    res = kernel_resources(os.path.join(CSRC, "vae_attention.hip"), tmp_path)
    for d in (64, 128, 256, 512):
        assert any("vae_attention_kernelILi%dE" % d in k for k in res), (d, sorted(res))
    spilled = {k: v for k, v in res.items() if v[1] != 0}
    assert not spilled, f"kernels with scratch (register spills): {spilled}"
    assert "v_mfma_f32_16x16x32_f16" in kernel_resources.last_asm, "both products must run on the matrix cores"
