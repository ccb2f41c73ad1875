"""CPU suite: the planner's side of the W8A8 GEGLU projection (plan tile 20, smgeglu_i8.hip), its host weight packer, the host refusals
of the two operators and the plumbing of the fourth calibration scope.  Tile 20 is tile 13's geometry - the same tile heights, tile
counts and eligibility, both heights - pinned by a descriptor that carries int8 weights and int8 activations; it is never the
library's own answer, it does not take the LayerNorm fold, and every shape the kernel does not take is refused by name."""
import os

import numpy as np
import pytest

from python_hip_stable_diffusion import _lib, activation_quantization as aq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEGLU, BIAS, LN = 2, 16, 1
# ff.net.0.proj of the 16x16 level at CFG batch 2 (M = 512), un-folded: the bias alone
SHAPE = dict(ksize=1, stride=1, up=1, C0=1280, C1=0, N=10240, B=2, Ho=16, Wo=16, out_mode=GEGLU, flags=BIAS)
AT_32 = dict(C0=640, N=5120, Ho=32, Wo=32)                 # the same layer of the 32x32 level: M = 2048
# (M, N2) of tests/test_w8a8_geglu_gpu.py at K = 192, as (B, Ho, Wo, N, bm)
SMALL = [(1, 16, 16, 640, 128), (1, 16, 32, 320, 128), (1, 16, 24, 1280, 128), (1, 16, 32, 640, 256), (1, 24, 32, 1280, 256)]


def plan(**kw):
    d = dict(SHAPE)
    d.update(kw)
    return _lib.conv_plan(d.pop("ksize"), d.pop("stride"), d.pop("up"), d.pop("C0"), d.pop("C1"), d.pop("N"), d.pop("B"), d.pop("Ho"), d.pop("Wo"), **d)


def test_tile_20_is_tile_13s_plan_from_int8():
    for kw, bm in ((dict(), 128), (AT_32, 256)):
        p20, p13 = plan(tile=20, **kw), plan(tile=13, **kw)
        assert p20["tile"] == 20 and p13["tile"] == 13
        assert p20["kernel"] == f"smgeglu_i8 bm{bm}" and p13["kernel"] == f"smgeglu bm{bm}"
        assert p20["staging"] == (1 if bm == 128 else 2)                          # the resolved tile height, as tiles 16 and 19 report it
        assert (p20["splitk"], p20["slab"], p20["workspace_bytes"]) == (p13["splitk"], p13["slab"], p13["workspace_bytes"]) == (1, False, 0)
        assert p20["copies"] == (False, False, False)


@pytest.mark.parametrize("B, Ho, Wo, N, bm", SMALL)
def test_tile_20_on_the_small_shapes_at_both_heights(B, Ho, Wo, N, bm):
    code = 1 if bm == 128 else 2
    kw = dict(C0=192, N=N, B=B, Ho=Ho, Wo=Wo)
    p = plan(tile=20, staging=code, **kw)
    assert (p["tile"], p["staging"], p["kernel"]) == (20, code, f"smgeglu_i8 bm{bm}")
    assert plan(tile=13, staging=code, **kw)["kernel"] == f"smgeglu bm{bm}"
    assert plan(tile=20, staging=code, flags=0, **kw)["tile"] == 20               # the bias may be absent


@pytest.mark.parametrize("kw", [dict(), AT_32, dict(flags=BIAS | LN), dict(flags=BIAS | LN, **AT_32), dict(C0=320, N=2560, Ho=64, Wo=64), dict(Ho=8, Wo=8)])
def test_tile_20_is_never_the_librarys_own_answer(kw):
    """... and with tile = 0 the answers for GEGLU descriptors are what they were: 13 on the two step shapes, folded or not"""
    p = plan(**kw)
    assert p["tile"] != 20 and "smgeglu_i8" not in p["kernel"]
    if kw.get("Ho", 16) in (16, 32):
        assert p["tile"] == 13 and p["kernel"] == ("smgeglu bm256" if "C0" in kw else "smgeglu bm128")


@pytest.mark.parametrize("kw", [
    dict(flags=BIAS | LN),                                # the LayerNorm fold: the int8 activations ARE the LayerNorm's output
    dict(ksize=3),                                        # a 3x3 conv
    dict(C0=640, C1=640),                                 # a second source
    dict(N=10240 + 64),                                   # not whole 160-row tiles
    dict(C0=96),                                          # not whole K64 stages
    dict(B=1, Ho=12, Wo=16),                              # M = 192: not whole 128-row tiles
    dict(B=1, Ho=8, Wo=16, staging=1),                    # M = 128: a single row of tiles
    dict(B=1, Ho=16, Wo=24, N=320),                       # 3 x 2 = 6 tiles, not a multiple of 8
    dict(out_mode=0),                                     # a plain projection
    dict(flags=BIAS | 4),                                 # a residual
    dict(C0=133184),                                      # 127 * 127 * K >= 2^31
    dict(staging=3),                                      # no such tile height
])
def test_shapes_tile_20_refuses(kw):
    with pytest.raises(ValueError, match="plan tile 20"):
        plan(tile=20, **kw)


def test_the_int32_bound_is_the_last_stage_that_fits():
    p = plan(tile=20, C0=133120)
    assert p["tile"] == 20 and p["kernel"] == "smgeglu_i8 bm128"


# ---- the host packer ----
def pack_numpy(wq):
    """the header's layout: strip 2 U + v holds the checkpoint rows v * N2 / 2 + 16 U + (0 .. 15), every row whole"""
    n2, k = wq.shape
    out = np.empty((n2 // 16, 16, k), np.int8)
    for strip in range(n2 // 16):
        U, v = strip >> 1, strip & 1
        out[strip] = wq[v * (n2 // 2) + 16 * U:][:16]
    return out


@pytest.mark.parametrize("n2, k", [(32, 64), (320, 192), (640, 1280)])
def test_packer_is_the_numpy_restatement(n2, k):
    rs = np.random.RandomState(n2 * 10000 + k)
    wq = rs.randint(-127, 128, size=(n2, k)).astype(np.int8)
    got = _lib.w8a8_pack_geglu(wq)
    assert got.dtype == np.int8 and got.shape == (n2 // 16, 16, k) and np.array_equal(got, pack_numpy(wq))
    # a tile of 80 output columns: ten consecutive strips = the value and gate rows of its five 16-column units
    if n2 % 160 == 0:
        t = n2 // 160 - 1
        rows = np.concatenate([np.arange(16) + v * (n2 // 2) + 16 * (5 * t + u) for u in range(5) for v in (0, 1)])
        assert np.array_equal(got[10 * t:10 * t + 10].reshape(160, k), wq[rows])


def test_packer_size_query_and_refusals():
    lib = _lib.lib()
    n = _lib.C.c_size_t(0)
    wq = np.zeros((64, 128), np.int8)
    assert lib.sd_op_w8a8_pack_geglu(_lib.ptr(wq), 64, 128, None, _lib.C.byref(n)) == 0 and n.value == 64 * 128
    assert lib.sd_op_w8a8_pack_geglu(None, 64, 128, None, _lib.C.byref(n)) == -1
    assert lib.sd_op_w8a8_pack_geglu(_lib.ptr(wq), 64, 128, None, None) == -1
    with pytest.raises(ValueError):
        _lib.w8a8_pack_geglu(np.zeros((64, 96), np.int8))                         # not whole K64 stages
    with pytest.raises(ValueError):
        _lib.w8a8_pack_geglu(np.zeros((48, 64), np.int8))                         # not whole value / gate strips
    with pytest.raises(ValueError):
        _lib.w8a8_pack_geglu(np.zeros((64, 64, 3, 3), np.int8))                   # a 3x3 weight


def test_new_symbols_are_in_the_header_and_the_library():
    header = open(os.path.join(ROOT, "include", "sd_mi355x.h")).read()
    for sym in ("sd_op_layernorm_q8", "sd_op_geglu_w8a8", "sd_op_w8a8_pack_geglu", "sd_weights_observe_geglus"):
        assert f"int {sym}(" in header and hasattr(_lib.lib(), sym), sym


# ---- host refusals of the two operators: everything in front of the first device call ----
def test_geglu_w8a8_host_refusals_in_the_headers_order():
    M, K, N2 = 256, 192, 640
    xq, wq, sc = np.ones((M, K), np.int8), np.ones((N2, K), np.int8), np.ones(N2, np.float32)
    lib = _lib.lib()
    out = np.empty(M * N2 // 2, np.float16)
    plan_ = (_lib.C.c_int * 4)()
    args = lambda **kw: [kw.get("xq", _lib.ptr(xq)), kw.get("wq", _lib.ptr(wq)), kw.get("sc", _lib.fptr(sc)), kw.get("absmax", float("nan")), None,   # noqa: E731
                         kw.get("out", _lib.ptr(out)), kw.get("M", M), K, N2, kw.get("bm", 0), kw.get("plan", plan_), 1, None]
    for kw in (dict(xq=None), dict(wq=None), dict(sc=None), dict(out=None), dict(plan=None), dict(M=0), dict(bm=64), dict()):
        assert lib.sd_op_geglu_w8a8(*args(**kw)) == -1, kw                       # SD_ERR_INVALID_ARGUMENT (the last one: act_absmax)
    with pytest.raises(ValueError, match="bm = 64"):                             # (1) in front of (2): the empty weight does not get a word in
        _lib.geglu_w8a8(xq, wq[:0], sc[:0], 1.0, bm=64)
    with pytest.raises(ValueError, match="plan tile 20"):                        # (3) N2 = 320 at M = 256: 2 x 2 = 4 tiles
        _lib.geglu_w8a8(xq, wq[:320], sc[:320], float("nan"))
    with pytest.raises(ValueError, match="plan tile 20"):                        # (3) K = 96
        _lib.geglu_w8a8(xq[:, :96], wq[:, :96], sc, float("nan"))
    with pytest.raises(ValueError, match="plan tile 20"):                        # (3) M = 256 has one 256-row tile
        _lib.geglu_w8a8(xq, wq, sc, float("nan"), bm=256)
    with pytest.raises(ValueError, match="133120"):                              # (4) in front of (5)
        _lib.geglu_w8a8(np.zeros((256, 133184), np.int8), np.zeros((640, 133184), np.int8), sc, float("nan"))
    bad_w, bad_x = wq.copy(), xq.copy()
    bad_w[5, 7] = bad_x[3, 9] = -128
    for absmax in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="act_absmax"):                      # (5) in front of (6)
            _lib.geglu_w8a8(bad_x, bad_w, np.zeros(N2, np.float32), absmax)
    with pytest.raises(ValueError, match="w_scale"):                             # (6) in front of (7)
        _lib.geglu_w8a8(bad_x, bad_w, np.zeros(N2, np.float32), 1.0)
    with pytest.raises(ValueError, match="weight value -128"):                   # (7) in front of (8)
        _lib.geglu_w8a8(bad_x, bad_w, sc, 1.0)
    with pytest.raises(ValueError, match="activation value -128 at element %d" % (3 * K + 9)):   # (8)
        _lib.geglu_w8a8(bad_x, wq, sc, 1.0)


def test_layernorm_q8_host_refusals():
    x = np.zeros((4, 64), np.float16)
    g = np.ones(64, np.float32)
    with pytest.raises(ValueError):
        _lib.layernorm_q8(x, g, None, 1.0)
    with pytest.raises(ValueError, match="2048"):
        _lib.layernorm_q8(np.zeros((4, 2056), np.float16), None, None, 1.0)
    with pytest.raises(ValueError, match="multiple of 8"):
        _lib.layernorm_q8(np.zeros((4, 60), np.float16), None, None, 1.0)
    for absmax in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="act_absmax"):
            _lib.layernorm_q8(x, g, g, absmax)
    lib = _lib.lib()
    xq = np.zeros((4, 64), np.int8)
    assert lib.sd_op_layernorm_q8(None, None, None, 1.0, 1e-5, _lib.ptr(xq), 4, 64, 1, None) == -1
    assert lib.sd_op_layernorm_q8(_lib.ptr(x), None, None, 1.0, 1e-5, None, 4, 64, 1, None) == -1
    assert lib.sd_op_layernorm_q8(_lib.ptr(x), None, None, 1.0, 1e-5, _lib.ptr(xq), 0, 64, 1, None) == -1


# ---- the fourth calibration scope ----
def test_recipe_from_ranges_takes_a_geglu_projection():
    name = "down_blocks.1.attentions.0.transformer_blocks.0.ff.net.0.proj"
    assert aq.recipe_from_ranges({name + ".weight": 7.5, "conv_in.weight": 2.0}, skip=["conv_in"]) == {name: 7.5}
    with pytest.raises(ValueError):
        aq.recipe_from_ranges({name + ".weight": 0.0})
    assert list(aq.CALIBRATION_SCOPES) == ["stream", "all", "gemm", "geglu"] and aq.CALIBRATION_SCOPES["geglu"] == "geglu"


def test_observe_scope_geglu_is_accepted_and_switched_off_again():
    from python_hip_stable_diffusion import hip_model
    assert hip_model.observe_level("geglu") == 2                                 # level 2 with both flags beside it
    store = hip_model.Weights(tensors={"w": np.zeros((4, 4), np.float32)})
    try:
        for on in ("geglu", False, "geglu", "gemm", "all", True, False):
            store.observe_activations(on)
        with pytest.raises(ValueError):
            store.observe_activations("geglus")
        lib = _lib.lib()
        assert lib.sd_weights_observe_geglus(store._h, 1) == 0 and lib.sd_weights_observe_geglus(store._h, 0) == 0
        assert lib.sd_weights_observe_geglus(store._h, 2) == -1 and lib.sd_weights_observe_geglus(None, 1) == -1
    finally:
        store.close()


def test_cli_scope_choices():
    from python_hip_stable_diffusion import pipeline as P
    base = ["--prompt", "x", "-i", "in", "-o", "out", "--seed", "1"]
    assert P.build_parser().parse_args(base).calibrate_scope == "stream"
    for scope in aq.CALIBRATION_SCOPES:
        assert P.build_parser().parse_args(base + ["--calibrate-scope", scope]).calibrate_scope == scope
    with pytest.raises(SystemExit):
        P.build_parser().parse_args(base + ["--calibrate-scope", "none"])
