"""CPU suite: the planner's side of the W8A8 transformer tail - the small-M 1x1 GEMM from int8 weights and int8 activations (plan tile
24, smgemm_q8.hip) - the host refusals of its operator and of the int8-output GEGLU in the header's order, the fourth observe flag and
the plumbing of the calibration scope ``tail``.  Tile 24 is tile 12 / 19's geometry pinned by a descriptor that carries int8 weights and
int8 activations; it is never the library's own answer, and every shape the kernel does not take is refused by name."""
import os

import numpy as np
import pytest

from python_hip_stable_diffusion import _lib, activation_quantization as aq
from test_build_isa import CSRC, HIPCC, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES, BIAS = 4, 16
# (K, N, B, Ho, Wo) -> the tile height: ff.net.2 of SD2.1-base's 640-channel level at CFG batch 2, of the test handle (batch 4 at 16x16),
# of the 1280-channel level
ADMITTED = [(2560, 640, 2, 32, 32, 64), (2560, 640, 4, 16, 16, 32), (5120, 1280, 2, 16, 16, 32)]


def plan(K=2560, N=640, B=2, Ho=32, Wo=32, tile=24, **kw):
    kw.setdefault("flags", RES | BIAS)
    return _lib.conv_plan(kw.pop("ksize", 1), 1, 1, K, kw.pop("C1", 0), N, B, Ho, Wo, tile=tile, **kw)


def test_new_symbols_are_in_the_header_and_the_library():
    header = open(os.path.join(ROOT, "include", "sd_mi355x.h")).read()
    for sym in ("sd_op_gemm_q8", "sd_op_geglu_w8a8_q8", "sd_weights_observe_tails"):
        assert f"int {sym}(" in header and hasattr(_lib.lib(), sym), sym
    assert callable(_lib.gemm_q8)


@pytest.mark.parametrize("K, N, B, Ho, Wo, bm", ADMITTED)
def test_tile_24_answers_for_the_tails_shapes(K, N, B, Ho, Wo, bm):
    p = plan(K, N, B, Ho, Wo)
    code = 1 if bm == 32 else 2
    assert (p["tile"], p["staging"], p["kernel"]) == (24, code, f"smgemm_q8 bm{bm}")   # the resolved tile height, as tile 19 reports it
    assert (p["splitk"], p["slab"], p["workspace_bytes"], p["copies"]) == (1, False, 0, (False, False, False))
    assert plan(K, N, B, Ho, Wo, staging=code)["kernel"] == f"smgemm_q8 bm{bm}"
    p19 = plan(K, N, B, Ho, Wo, tile=19)                                         # tile 19's geometry and eligibility
    assert (p19["tile"], p19["staging"], p19["kernel"]) == (19, code, f"smgemm_i8 bm{bm}")
    assert M_of(B, Ho, Wo) // bm * (N // 80) % 8 == 0


def M_of(B, Ho, Wo):
    return B * Ho * Wo


def test_both_heights_where_both_tile():
    for staging, bm in ((1, 32), (2, 64)):
        p = plan(staging=staging)
        assert (p["tile"], p["staging"], p["kernel"]) == (24, staging, f"smgemm_q8 bm{bm}")


@pytest.mark.parametrize("kw", [
    dict(ksize=3),                                        # a 3x3 conv
    dict(K=2560, C1=640),                                 # a second source (the merged tail's [g | h2])
    dict(N=96),                                           # not whole 80-column tiles (N % 80)
    dict(K=96),                                           # not whole K64 stages (K % 64)
    dict(B=1, Ho=6, Wo=8),                                # M = 48: not whole 32-row tiles
    dict(B=2, Ho=8, Wo=8, N=160, staging=2),              # M = 128 in 64-row tiles at N = 160: 2 x 2 = 4 tiles, not a multiple of 8
    dict(B=1, Ho=4, Wo=8, N=640),                         # M = 32: one tile row - fewer than 2 x 2 tiles
    dict(B=2, Ho=8, Wo=8, N=80),                          # one tile column
    dict(out_mode=2),                                     # the GEGLU projection
    dict(K=133184),                                       # 127 * 127 * K >= 2^31
])
def test_shapes_tile_24_refuses(kw):
    with pytest.raises(ValueError, match="plan tile 24"):
        plan(tile=24, **kw)


def test_the_mid_blocks_shape_is_on_the_tiles_but_off_the_handles_rule():
    """M = 128 (the 8x8 mid block at CFG batch 2) tiles - 4 x 16 tiles of 32 rows, as for tiles 12 and 19, and the operator runs it -
    but 64 tiles are not the one round of the chip a handle takes the kernel for (smgemm_q8_wanted: 192 - 256 tiles, M >= 256), so a
    handle leaves the mid block's tail merged in fp16 (SD2.1-base: LAB_NOTES round 31 counts the six merged tails that stay)"""
    p = plan(5120, 1280, 2, 8, 8)
    assert (p["tile"], p["kernel"]) == (24, "smgemm_q8 bm32")
    assert plan(5120, 1280, 2, 8, 8, tile=19)["tile"] == 19


def test_tile_24_is_never_the_librarys_own_answer():
    for K, N, B, Ho, Wo, _ in ADMITTED:
        p = plan(K, N, B, Ho, Wo, tile=0)
        assert p["tile"] != 24 and "smgemm_q8" not in p["kernel"]


def test_the_int32_bound_is_the_last_stage_that_fits():
    p = plan(K=133120)
    assert p["tile"] == 24 and p["kernel"] == "smgemm_q8 bm64"


# ---- host refusals of the operators: everything in front of the first device call, in the header's order ----
def test_gemm_q8_host_refusals_in_the_headers_order():
    M, K, N = 64, 128, 320
    xq, wq, sc = np.ones((M, K), np.int8), np.ones((N, K), np.int8), np.ones(N, np.float32)
    lib = _lib.lib()
    out = np.empty(M * N, np.float16)
    plan_ = (_lib.C.c_int * 4)()
    nan = float("nan")
    args = lambda **kw: [kw.get("xq", _lib.ptr(xq)), kw.get("wq", _lib.ptr(wq)), kw.get("sc", _lib.fptr(sc)), kw.get("absmax", nan), None, None,   # noqa: E731
                         kw.get("out", _lib.ptr(out)), kw.get("M", M), kw.get("K", K), kw.get("N", N), kw.get("bm", 0), kw.get("plan", plan_), 1, None]
    for kw in (dict(xq=None), dict(wq=None), dict(sc=None), dict(out=None), dict(plan=None), dict(M=0), dict(K=0), dict(N=0), dict(bm=48), dict()):
        assert lib.sd_op_gemm_q8(*args(**kw)) == -1, kw                          # SD_ERR_INVALID_ARGUMENT (the last one: act_absmax)
    with pytest.raises(ValueError, match="bm = 48"):                             # (1) in front of (2): an empty problem does not get a word in
        _lib.gemm_q8(xq[:0], wq, sc, nan, bm=48)
    with pytest.raises(ValueError, match="empty"):                               # (2) in front of (3)
        _lib.gemm_q8(xq[:0], wq, sc, nan)
    with pytest.raises(ValueError, match="plan tile 24"):                        # (3) one row of 64-row tiles
        _lib.gemm_q8(xq, wq, sc, nan, bm=64)
    with pytest.raises(ValueError, match="plan tile 24"):                        # (3) N = 96
        _lib.gemm_q8(xq, wq[:96], sc[:96], nan)
    with pytest.raises(ValueError, match="plan tile 24"):                        # (3) K = 96
        _lib.gemm_q8(xq[:, :96], wq[:, :96], sc, nan)
    # (4) in front of (5): the first depth past the bound - refused before a byte of it is read
    assert lib.sd_op_gemm_q8(*args(K=133184)) == -1 and b"exact int32 sums" in lib.sd_last_error() and b"133120" in lib.sd_last_error()
    bad_w, bad_x = wq.copy(), xq.copy()
    bad_w[5, 7] = bad_x[3, 9] = -128
    zeros = np.zeros(N, np.float32)
    for absmax in (0.0, -1.0, nan, float("inf")):
        with pytest.raises(ValueError, match="act_absmax"):                      # (5) in front of (6)
            _lib.gemm_q8(bad_x, bad_w, zeros, absmax)
    with pytest.raises(ValueError, match="w_scale"):                             # (6) in front of (7)
        _lib.gemm_q8(bad_x, bad_w, zeros, 1.0)
    with pytest.raises(ValueError, match="weight value -128"):                   # (7) in front of (8)
        _lib.gemm_q8(bad_x, bad_w, sc, 1.0)
    with pytest.raises(ValueError, match="activation value -128 at element %d" % (3 * K + 9)):   # (8), the last
        _lib.gemm_q8(bad_x, wq, sc, 1.0)
    if not _lib.lib().sd_device_count() > 0:                                     # a valid call reaches the device: without one, the no-GPU error
        with pytest.raises(RuntimeError, match="no HIP device"):
            _lib.gemm_q8(xq, wq, sc, 1.0)
    with pytest.raises(ValueError):                                              # the wrapper's own shape checks
        _lib.gemm_q8(xq, wq[:, :64], sc, 1.0)
    with pytest.raises(ValueError):
        _lib.gemm_q8(xq, wq, sc, 1.0, res=np.zeros((M, N - 1), np.float16))
    with pytest.raises(ValueError):
        _lib.gemm_q8(xq, wq, sc, 1.0, out=np.empty(8, np.float16))


def test_geglu_w8a8_q8_host_refusals_in_the_headers_order():
    M, C, N2 = 256, 128, 640
    xq, wq, sc = np.ones((M, C), np.int8), np.ones((N2, C), np.int8), np.ones(N2, np.float32)
    lib = _lib.lib()
    out = np.empty(M * N2 // 2, np.int8)
    plan_ = (_lib.C.c_int * 4)()
    nan = float("nan")
    args = lambda **kw: [kw.get("xq", _lib.ptr(xq)), kw.get("wq", _lib.ptr(wq)), kw.get("sc", _lib.fptr(sc)), kw.get("absmax", 1.0), None,   # noqa: E731
                         kw.get("out_absmax", nan), kw.get("out", _lib.ptr(out)), kw.get("M", M), C, N2, kw.get("bm", 0), kw.get("plan", plan_), 1, None]
    for kw in (dict(xq=None), dict(wq=None), dict(sc=None), dict(out=None), dict(plan=None), dict(M=0), dict(bm=64), dict()):
        assert lib.sd_op_geglu_w8a8_q8(*args(**kw)) == -1, kw                    # (the last one: out_absmax)
    assert b"out_absmax" in lib.sd_last_error()
    with pytest.raises(ValueError, match="bm = 64"):                             # (1)
        _lib.geglu_w8a8(xq[:0], wq, sc, nan, bm=64, out_absmax=nan)
    with pytest.raises(ValueError, match="empty"):                               # (2)
        _lib.geglu_w8a8(xq[:0], wq, sc, nan, out_absmax=nan)
    with pytest.raises(ValueError, match="plan tile 20"):                        # (3) one row of 256-row tiles
        _lib.geglu_w8a8(xq, wq, sc, nan, bm=256, out_absmax=nan)
    bad_w, bad_x = wq.copy(), xq.copy()
    bad_w[5, 7] = bad_x[3, 9] = -128
    zeros = np.zeros(N2, np.float32)
    with pytest.raises(ValueError, match="act_absmax"):                          # (5): act_absmax, then out_absmax beside it
        _lib.geglu_w8a8(bad_x, bad_w, zeros, nan, out_absmax=nan)
    for bad in (0.0, -1.0, nan, float("inf")):
        with pytest.raises(ValueError, match="out_absmax"):                      # ... in front of (6)
            _lib.geglu_w8a8(bad_x, bad_w, zeros, 1.0, out_absmax=bad)
    with pytest.raises(ValueError, match="w_scale"):                             # (6) in front of (7)
        _lib.geglu_w8a8(bad_x, bad_w, zeros, 1.0, out_absmax=1.0)
    with pytest.raises(ValueError, match="weight value -128"):                   # (7) in front of (8)
        _lib.geglu_w8a8(bad_x, bad_w, sc, 1.0, out_absmax=1.0)
    with pytest.raises(ValueError, match="activation value -128"):               # (8)
        _lib.geglu_w8a8(bad_x, wq, sc, 1.0, out_absmax=1.0)
    with pytest.raises(ValueError, match="int8"):                                # the wrapper: an int8 output needs an int8 buffer
        _lib.geglu_w8a8(xq, wq, sc, 1.0, out=np.empty(M * N2 // 2, np.float16), out_absmax=1.0)
    with pytest.raises(ValueError, match="float16"):                             # ... and the fp16 output a float16 one, as before
        _lib.geglu_w8a8(xq, wq, sc, 1.0, out=np.empty(M * N2 // 2, np.int8))


# ---- the fourth observe flag and the scope ----
def test_observe_tails_flag_contract():
    from python_hip_stable_diffusion import hip_model
    assert hip_model.observe_level("tail") == 2                                  # level 2 with the four flags beside it
    store = hip_model.Weights(tensors={"w": np.zeros((4, 4), np.float32)})
    try:
        lib = _lib.lib()
        assert lib.sd_weights_observe_tails(store._h, 1) == 0 and lib.sd_weights_observe_tails(store._h, 0) == 0
        for bad in (2, -1, 3):
            assert lib.sd_weights_observe_tails(store._h, bad) == -1
        assert lib.sd_weights_observe_tails(None, 1) == -1
        for on in ("tail", False, "tail", "attn", "geglu", "gemm", "all", True, False):
            store.observe_activations(on)
        for bad in ("tails", "ff", "proj_out"):
            with pytest.raises(ValueError):
                store.observe_activations(bad)
        assert lib.sd_weights_observe_activations(store._h, 3) == -1             # the level entry keeps its three levels
    finally:
        store.close()


def test_scope_mapping_and_cli_choices():
    from python_hip_stable_diffusion import pipeline as P
    assert list(aq.CALIBRATION_SCOPES) == ["stream", "all", "gemm", "geglu"]     # the three pinned facts, unchanged
    assert aq.ATTENTION_SCOPES == {"attn": "attn"}
    assert list(aq.calibration_scopes()) == ["stream", "all", "gemm", "geglu", "attn"]
    assert aq.TAIL_SCOPES == {"tail": "tail"}
    assert list(aq.all_calibration_scopes()) == ["stream", "all", "gemm", "geglu", "attn", "tail"] and aq.all_calibration_scopes()["stream"] is True
    base = ["--prompt", "x", "-i", "in", "-o", "out", "--seed", "1"]
    assert P.build_parser().parse_args(base).calibrate_scope == "stream"
    for scope in aq.all_calibration_scopes():
        assert P.build_parser().parse_args(base + ["--calibrate-scope", scope]).calibrate_scope == scope
    with pytest.raises(SystemExit):
        P.build_parser().parse_args(base + ["--calibrate-scope", "none"])


def test_recipe_from_ranges_takes_the_tails_two_layers():
    t = "down_blocks.1.attentions.0."
    ranges = {t + "transformer_blocks.0.ff.net.2.weight": 7.5, t + "proj_out.weight": 3.25}
    assert aq.recipe_from_ranges(ranges) == {t + "transformer_blocks.0.ff.net.2": 7.5, t + "proj_out": 3.25}
    assert aq.recipe_from_ranges(ranges, skip=[t + "proj_out"]) == {t + "transformer_blocks.0.ff.net.2": 7.5}


# ---- the compiled kernels ----
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_smgemm_q8_compiles_for_gfx950_without_scratch(tmp_path):
    res = kernel_resources(os.path.join(CSRC, "smgemm_q8.hip"), tmp_path)
    kernels = {k: v for k, v in res.items() if "smgemm_q8_kernel" in k}
    assert len(kernels) == 2 and any("ILi32E" in k for k in kernels) and any("ILi64E" in k for k in kernels), list(res)   # both tile heights
    for name, (vgpr, scratch) in res.items():
        assert scratch == 0, f"{name}: {scratch} bytes of scratch (register spills)"
        # the ring takes the whole LDS: ONE workgroup of five waves per CU, at most two waves on a SIMD - 512 / 2 registers each
        assert 0 < vgpr <= 256, (name, vgpr)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_smgeglu_i8_has_the_int8_output_instantiations_without_scratch(tmp_path):
    res = kernel_resources(os.path.join(CSRC, "smgeglu_i8.hip"), tmp_path)
    kernels = {k: v for k, v in res.items() if "smgeglu_i8_kernel" in k}
    assert len(kernels) == 4 and sum("Lb1E" in k for k in kernels) == 2, list(res)      # both tile heights, fp16 and int8 output
    for name, (vgpr, scratch) in res.items():
        assert scratch == 0, f"{name}: {scratch} bytes of scratch (register spills)"
        assert 0 < vgpr <= 168, (name, vgpr)                                     # ten waves per CU = three per SIMD: 512 / 3 registers each
