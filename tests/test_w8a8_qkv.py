"""CPU suite: the planner's side of the W8A8 self-attention q|k|v projection (plan tile 22, smqkv_i8.hip), its host weight packer, the
host refusals of its operator in the header's order, the third observe flag and the plumbing of the calibration scope ``attn``.  Tile
22 has no fp16 twin: it is pinned by a descriptor that carries int8 weights and int8 activations, it is never the library's own answer,
and every shape off its rule is refused by name."""
import os

import numpy as np
import pytest

from python_hip_stable_diffusion import _lib, activation_quantization as aq
from test_build_isa import CSRC, HIPCC, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LN, BIAS = 1, 16
# (C, B, Ho, Wo) -> the tile height the grid gives: SD2.1-base's two shapes, the test handle's, SDXL-base's two
ADMITTED = [(640, 2, 32, 32, 128), (1280, 2, 16, 16, 128), (640, 4, 16, 16, 128), (640, 2, 48, 48, 256), (1280, 2, 24, 24, 128)]


def plan(C=640, B=2, Ho=32, Wo=32, tile=22, **kw):
    kw.setdefault("N", 3 * C)
    kw.setdefault("n_trans", 2 * C)
    return _lib.conv_plan(kw.pop("ksize", 1), 1, 1, C, kw.pop("C1", 0), kw.pop("N"), B, Ho, Wo, tile=tile, **kw)


@pytest.mark.parametrize("C, B, Ho, Wo, bm", ADMITTED)
def test_the_rule_admits_the_five_shapes(C, B, Ho, Wo, bm):
    p = plan(C, B, Ho, Wo)
    code = 1 if bm == 128 else 2
    assert (p["tile"], p["staging"], p["kernel"]) == (22, code, f"smqkv_i8 bm{bm}")    # the resolved tile height, as tiles 19 / 20 report it
    assert (p["splitk"], p["slab"], p["workspace_bytes"]) == (1, False, 0)
    assert plan(C, B, Ho, Wo, staging=code)["kernel"] == f"smqkv_i8 bm{bm}"
    tiles = B * Ho * Wo // bm * (3 * C // 160)
    assert tiles % 8 == 0 and B * Ho * Wo // bm >= 2 and C % 160 == 0                  # the rule, restated


def test_both_heights_where_both_tile():
    assert plan(staging=1)["kernel"] == "smqkv_i8 bm128" and plan(staging=2)["kernel"] == "smqkv_i8 bm256"
    assert plan(640, 4, 16, 16, staging=2)["kernel"] == "smqkv_i8 bm256"               # the test handle's shape: 4 x 12 tiles
    with pytest.raises(ValueError, match="plan tile 22"):                                # M = 1152 = 4.5 x 256
        plan(1280, 2, 24, 24, staging=2)


@pytest.mark.parametrize("kw", [
    dict(C=1280, B=2, Ho=8, Wo=8),                        # the mid block, M = 128: a single row of tiles
    dict(C=320, B=2, Ho=64, Wo=64),                       # the 320-channel level: its head is one launch of its own
    dict(C=320, B=2, Ho=16, Wo=16),
    dict(flags=LN | BIAS),                                # the LayerNorm fold: the int8 activations ARE the LayerNorm's output
    dict(ksize=3),                                        # a 3x3 conv
    dict(C1=640),                                         # a second source
    dict(n_trans=0),                                      # a plain projection: no V^T
    dict(n_trans=640),                                    # V^T that is not the last third
    dict(N=1920 + 160),                                   # not [Wq | Wk | Wv]
    dict(C=704),                                          # a multiple of 64 but not of 160: q | k | v boundaries inside a tile
    dict(C=800),                                          # ... of 160 but not of 64: no whole K64 stages
    dict(B=1, Ho=12, Wo=16),                              # M = 192: not whole 128-row tiles
    dict(B=32, Ho=4, Wo=6),                               # S = 24 (M = 768, 6 x 12 tiles): a 16-token block would straddle two samples
    dict(B=1, Ho=16, Wo=24),                              # M = 384, 3 x 12 = 36 tiles: not a multiple of 8
    dict(out_mode=2),                                     # a GEGLU
    dict(flags=4),                                        # a residual
    dict(flags=2),                                        # a time embedding
    dict(C=133440),                                       # 127 * 127 * K >= 2^31
    dict(staging=3),                                      # no such tile height
])
def test_shapes_tile_22_refuses(kw):
    with pytest.raises(ValueError, match="plan tile 22"):
        plan(**kw)


@pytest.mark.parametrize("kw", [dict(), dict(flags=LN | BIAS), dict(C=1280, Ho=16, Wo=16, flags=LN | BIAS), dict(C=640, B=4, Ho=16, Wo=16, flags=LN | BIAS)])
def test_tile_22_is_never_the_librarys_own_answer(kw):
    p = plan(tile=0, **kw)
    assert p["tile"] != 22 and "smqkv" not in p["kernel"]


# ---- the host packer ----
def pack_numpy(wq):
    """the header's layout: strip t holds the stacked rows 16 t .. 16 t + 15, every row whole"""
    n3, k = wq.shape
    out = np.empty((n3 // 16, 16, k), np.int8)
    for t in range(n3 // 16):
        out[t] = wq[16 * t:16 * t + 16]
    return out


@pytest.mark.parametrize("c", [64, 320, 640])
def test_packer_is_the_numpy_restatement(c):
    rs = np.random.RandomState(c)
    wq = rs.randint(-127, 128, size=(3 * c, c)).astype(np.int8)
    got = _lib.w8a8_pack_qkv(wq)
    assert got.dtype == np.int8 and got.shape == (3 * c // 16, 16, c) and np.array_equal(got, pack_numpy(wq))
    if c % 160 == 0:                                                             # a tile of 160 columns: ten consecutive strips of ONE matrix
        for t in range(3 * c // 160):
            assert np.array_equal(got[10 * t:10 * t + 10].reshape(160, c), wq[160 * t:160 * t + 160])
            assert (160 * t) // c == (160 * t + 159) // c


def test_packer_size_query_and_refusals():
    lib = _lib.lib()
    n = _lib.C.c_size_t(0)
    wq = np.zeros((192, 64), np.int8)
    assert lib.sd_op_w8a8_pack_qkv(_lib.ptr(wq), 64, None, _lib.C.byref(n)) == 0 and n.value == 3 * 64 * 64
    assert lib.sd_op_w8a8_pack_qkv(None, 64, None, _lib.C.byref(n)) == -1
    assert lib.sd_op_w8a8_pack_qkv(_lib.ptr(wq), 64, None, None) == -1
    assert lib.sd_op_w8a8_pack_qkv(_lib.ptr(wq), 0, None, _lib.C.byref(n)) == -1
    with pytest.raises(ValueError):
        _lib.w8a8_pack_qkv(np.zeros((288, 96), np.int8))                          # not whole K64 stages
    with pytest.raises(ValueError):
        _lib.w8a8_pack_qkv(np.zeros((128, 64), np.int8))                          # not three matrices
    with pytest.raises(ValueError):
        _lib.w8a8_pack_qkv(np.zeros((192, 64, 1, 1), np.int8))


def test_new_symbols_are_in_the_header_and_the_library():
    header = open(os.path.join(ROOT, "include", "sd_mi355x.h")).read()
    for sym in ("sd_op_qkv_w8a8", "sd_op_w8a8_pack_qkv", "sd_weights_observe_qkv"):
        assert f"int {sym}(" in header and hasattr(_lib.lib(), sym), sym


# ---- host refusals of the operator: everything in front of the first device call, in the header's order ----
def test_qkv_w8a8_host_refusals_in_the_headers_order():
    B, HW, C = 1, 256, 640
    M, N = B * HW, 3 * C
    xq, wq, sc = np.ones((M, C), np.int8), np.ones((N, C), np.int8), np.ones(N, np.float32)
    lib = _lib.lib()
    oqk, ovt = np.empty(M * 2 * C, np.float16), np.empty(B * C * HW, np.float16)
    plan_ = (_lib.C.c_int * 4)()
    nan = float("nan")
    args = lambda **kw: [kw.get("xq", _lib.ptr(xq)), kw.get("wq", _lib.ptr(wq)), kw.get("sc", _lib.fptr(sc)), kw.get("absmax", nan), None,   # noqa: E731
                         kw.get("oqk", _lib.ptr(oqk)), kw.get("ovt", _lib.ptr(ovt)), kw.get("B", B), kw.get("HW", HW), kw.get("C", C), 1.0, 1,
                         kw.get("bm", 0), kw.get("plan", plan_), 1, None]
    for kw in (dict(xq=None), dict(wq=None), dict(sc=None), dict(oqk=None), dict(ovt=None), dict(plan=None), dict(B=0), dict(HW=0), dict(bm=64), dict()):
        assert lib.sd_op_qkv_w8a8(*args(**kw)) == -1, kw                         # SD_ERR_INVALID_ARGUMENT (the last one: act_absmax)
    with pytest.raises(ValueError, match="bm = 64"):                             # (1) in front of (2): an empty problem does not get a word in
        _lib.qkv_w8a8(xq[:0], wq, sc, nan, 1, bm=64)
    with pytest.raises(ValueError, match="empty"):                               # (2) in front of (3)
        _lib.qkv_w8a8(xq[:0], wq, sc, nan, 1)
    with pytest.raises(ValueError, match="plan tile 22"):                        # (3) M = 256 has one 256-row tile
        _lib.qkv_w8a8(xq, wq, sc, nan, 1, bm=256)
    with pytest.raises(ValueError, match="plan tile 22"):                        # (3) S = 8
        _lib.qkv_w8a8(xq, wq, sc, nan, 32)
    with pytest.raises(ValueError, match="plan tile 22"):                        # (3) M = 384: 3 x 12 tiles
        _lib.qkv_w8a8(np.ones((384, C), np.int8), wq, sc, nan, 1)
    with pytest.raises(ValueError, match="plan tile 22"):                        # (3) C = 320
        _lib.qkv_w8a8(xq[:, :320], wq[:960, :320], sc[:960], nan, 1)
    # (4) in front of (5): the first width past the bound that the rule otherwise tiles - refused before a byte of it is read
    # (HW = 1024: 4 x 2502 tiles of 256 rows, a multiple of 8)
    assert lib.sd_op_qkv_w8a8(*args(C=133440, HW=1024)) == -1 and b"exact int32 sums" in lib.sd_last_error()
    assert lib.sd_op_qkv_w8a8(*args(C=133120 + 64, HW=1024)) == -1 and b"not eligible for plan tile 22" in lib.sd_last_error()   # (3): 133184 is off the rule
    bad_w, bad_x = wq.copy(), xq.copy()
    bad_w[5, 7] = bad_x[3, 9] = -128
    zeros = np.zeros(N, np.float32)
    for absmax in (0.0, -1.0, nan, float("inf")):
        with pytest.raises(ValueError, match="act_absmax"):                      # (5) in front of (6)
            _lib.qkv_w8a8(bad_x, bad_w, zeros, absmax, 1)
    for q_scale in (nan, float("inf")):
        with pytest.raises(ValueError, match="q_scale"):                         # (5), its second half
            _lib.qkv_w8a8(bad_x, bad_w, zeros, 1.0, 1, q_scale=q_scale)
    with pytest.raises(ValueError, match="w_scale"):                             # (6) in front of (7)
        _lib.qkv_w8a8(bad_x, bad_w, zeros, 1.0, 1)
    with pytest.raises(ValueError, match="weight value -128"):                   # (7) in front of (8)
        _lib.qkv_w8a8(bad_x, bad_w, sc, 1.0, 1)
    with pytest.raises(ValueError, match="activation value -128 at element %d" % (3 * C + 9)):   # (8)
        _lib.qkv_w8a8(bad_x, wq, sc, 1.0, 1)
    if not _lib.lib().sd_device_count() > 0:                                     # a valid call reaches the device: without one, the no-GPU error
        with pytest.raises(RuntimeError, match="no HIP device"):
            _lib.qkv_w8a8(xq, wq, sc, 1.0, 1)
    with pytest.raises(ValueError):                                              # the wrapper's own shape checks
        _lib.qkv_w8a8(xq, wq[:N - 16], sc[:N - 16], 1.0, 1)
    with pytest.raises(ValueError):
        _lib.qkv_w8a8(xq, wq, sc, 1.0, 1, out_qk=np.empty(8, np.float16))


# ---- the third observe flag and the scope ----
def test_observe_qkv_flag_contract():
    from python_hip_stable_diffusion import hip_model
    assert hip_model.observe_level("attn") == 2                                  # level 2 with the three flags beside it
    store = hip_model.Weights(tensors={"w": np.zeros((4, 4), np.float32)})
    try:
        lib = _lib.lib()
        assert lib.sd_weights_observe_qkv(store._h, 1) == 0 and lib.sd_weights_observe_qkv(store._h, 0) == 0
        for bad in (2, -1, 3):
            assert lib.sd_weights_observe_qkv(store._h, bad) == -1
        assert lib.sd_weights_observe_qkv(None, 1) == -1
        for on in ("attn", False, "attn", "geglu", "gemm", "all", True, False):
            store.observe_activations(on)
        for bad in ("attention", "qkv", "attns"):
            with pytest.raises(ValueError):
                store.observe_activations(bad)
        assert lib.sd_weights_observe_activations(store._h, 3) == -1             # the level entry keeps its three levels
    finally:
        store.close()


def test_scope_mapping_and_cli_choices():
    from python_hip_stable_diffusion import pipeline as P
    assert list(aq.CALIBRATION_SCOPES) == ["stream", "all", "gemm", "geglu"]     # unchanged
    assert aq.ATTENTION_SCOPES == {"attn": "attn"}
    assert list(aq.calibration_scopes()) == ["stream", "all", "gemm", "geglu", "attn"] and aq.calibration_scopes()["stream"] is True
    base = ["--prompt", "x", "-i", "in", "-o", "out", "--seed", "1"]
    assert P.build_parser().parse_args(base).calibrate_scope == "stream"
    for scope in aq.calibration_scopes():
        assert P.build_parser().parse_args(base + ["--calibrate-scope", scope]).calibrate_scope == scope
    with pytest.raises(SystemExit):
        P.build_parser().parse_args(base + ["--calibrate-scope", "none"])


def test_recipe_from_ranges_takes_the_three_projections_with_one_value():
    b = "down_blocks.1.attentions.0.transformer_blocks.0.attn1."
    ranges = {b + p + ".weight": 5.25 for p in ("to_q", "to_k", "to_v")}
    assert aq.recipe_from_ranges(ranges) == {b + "to_q": 5.25, b + "to_k": 5.25, b + "to_v": 5.25}


# ---- the compiled kernel ----
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_smqkv_i8_compiles_for_gfx950_without_scratch(tmp_path):
    res = kernel_resources(os.path.join(CSRC, "smqkv_i8.hip"), tmp_path)
    kernels = {k: v for k, v in res.items() if "smqkv_i8_kernel" in k}
    assert len(kernels) == 2, list(res)                                          # both tile heights
    for name, (vgpr, scratch) in res.items():
        assert scratch == 0, f"{name}: {scratch} bytes of scratch (register spills)"
        assert 0 < vgpr <= 168, (name, vgpr)                                     # ten waves per CU = three per SIMD: 512 / 3 registers each
