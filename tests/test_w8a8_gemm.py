"""CPU suite: the planner's side of the W8A8 small-M 1x1 GEMM (plan tile 19, smgemm_i8.hip), its host weight packer and the plumbing
of the third calibration scope.  Tile 19 is tile 12's geometry - the same tile heights, tile counts and eligibility - pinned by a
descriptor that carries int8 weights; it is never the library's own answer, and every shape the kernel does not take is refused by
name."""
import numpy as np
import pytest

from python_hip_stable_diffusion import _lib

# attn1.to_out.0 of the 16x16 level at CFG batch 2: bias and residual
SHAPE = dict(ksize=1, stride=1, up=1, C0=1280, C1=0, N=1280, B=2, Ho=16, Wo=16, flags=4 | 16)
AT_32 = dict(C0=640, N=640, Ho=32, Wo=32)                 # the same layer of the 32x32 level: M = 2048


def plan(**kw):
    d = dict(SHAPE)
    d.update(kw)
    return _lib.conv_plan(d.pop("ksize"), d.pop("stride"), d.pop("up"), d.pop("C0"), d.pop("C1"), d.pop("N"), d.pop("B"), d.pop("Ho"), d.pop("Wo"), **d)


def test_tile_19_is_tile_12s_plan_from_int8():
    for kw, bm in ((dict(), 32), (AT_32, 64)):
        p19, p12 = plan(tile=19, **kw), plan(tile=12, **kw)
        assert p19["tile"] == 19 and p12["tile"] == 12
        assert p19["kernel"] == f"smgemm_i8 bm{bm}" and p12["kernel"] == f"smgemm bm{bm}"
        assert p19["staging"] == (1 if bm == 32 else 2)                           # the resolved tile height, as tile 15 reports it
        assert (p19["splitk"], p19["slab"], p19["workspace_bytes"]) == (p12["splitk"], p12["slab"], p12["workspace_bytes"]) == (1, False, 0)
        assert p19["copies"] == p12["copies"] == (False, False, False)
        for staging, forced in ((1, 32), (2, 64)):
            p = plan(tile=19, staging=staging, **kw)
            assert (p["tile"], p["staging"], p["kernel"]) == (19, staging, f"smgemm_i8 bm{forced}")
            assert plan(tile=12, staging=staging, **kw)["kernel"] == f"smgemm bm{forced}"


@pytest.mark.parametrize("kw", [dict(), AT_32, dict(C0=320, N=320, Ho=64, Wo=64), dict(Ho=8, Wo=8)])
def test_tile_19_is_never_the_librarys_own_answer(kw):
    p = plan(**kw)
    assert p["tile"] != 19 and "smgemm_i8" not in p["kernel"]
    if kw in (dict(), AT_32):
        assert p["tile"] == 12                                                   # ... where the fp16 plan is the small-M GEMM


@pytest.mark.parametrize("kw", [
    dict(ksize=3),                                        # a 3x3 conv
    dict(C0=640, C1=640),                                 # a second source (the merged transformer tail)
    dict(N=96),                                           # not whole 80-column tiles
    dict(C0=96),                                          # not whole K64 stages
    dict(B=1, Ho=6, Wo=8),                                # M = 48: not whole 32-row tiles
    dict(B=1, Ho=8, Wo=8, N=160),                         # M = 64, N = 160: 4 tiles, not a multiple of 8
    dict(out_mode=2),                                     # the GEGLU projection
    dict(C0=133184),                                      # 127 * 127 * K >= 2^31
])
def test_shapes_tile_19_refuses(kw):
    with pytest.raises(ValueError, match="plan tile 19"):
        plan(tile=19, **kw)


def test_the_int32_bound_is_the_last_stage_that_fits():
    assert 127 * 127 * 133120 < 2 ** 31 <= 127 * 127 * 133184
    p = plan(tile=19, C0=133120)
    assert p["tile"] == 19 and p["kernel"] == "smgemm_i8 bm32"


# ---- the host packer ----
@pytest.mark.parametrize("n, k", [(80, 64), (160, 192), (320, 1280)])
def test_packer_is_the_numpy_restatement(n, k):
    """[N][K] as the checkpoint holds it: wave w of a tile fetches rows 16 w .. 16 w + 15 of a K64 stage, 64 contiguous bytes each"""
    rs = np.random.RandomState(n * 10000 + k)
    wq = rs.randint(-127, 128, size=(n, k)).astype(np.int8)
    got = _lib.w8a8_pack_gemm(wq)
    assert got.dtype == np.int8 and got.shape == (n, k) and np.array_equal(got, np.ascontiguousarray(wq))
    row, stage = n - 1, k // 64 - 1
    assert np.array_equal(got.reshape(-1)[row * k + 64 * stage:][:64], wq[row, 64 * stage:64 * stage + 64])


def test_packer_refusals():
    with pytest.raises(ValueError):
        _lib.w8a8_pack_gemm(np.zeros((80, 96), np.int8))                          # not whole K64 stages
    with pytest.raises(ValueError):
        _lib.w8a8_pack_gemm(np.zeros((80, 64, 3, 3), np.int8))                    # a 3x3 weight
    with pytest.raises(ValueError):
        _lib.w8a8_pack_gemm(np.zeros((40, 64), np.int8))                          # not whole 16-row strips


# ---- the third calibration scope ----
def test_observe_scope_gemm_is_accepted_and_switched_off_again():
    from python_hip_stable_diffusion import hip_model
    assert hip_model.observe_level("gemm") == 2                                  # level 2 with the projections' flag beside it
    store = hip_model.Weights(tensors={"w": np.zeros((4, 4), np.float32)})
    try:
        for on in ("gemm", False, "gemm", "all", True, False):
            store.observe_activations(on)
        with pytest.raises(ValueError):
            store.observe_activations("gem")
        lib = _lib.lib()
        assert lib.sd_weights_observe_gemms(store._h, 1) == 0 and lib.sd_weights_observe_gemms(store._h, 0) == 0
        assert lib.sd_weights_observe_gemms(store._h, 2) == -1 and lib.sd_weights_observe_gemms(None, 1) == -1
        with pytest.raises(ValueError):                                          # the level entry keeps refusing a fourth level
            _lib.check(lib.sd_weights_observe_activations(store._h, 3))
    finally:
        store.close()


def test_cli_scope_choices():
    from python_hip_stable_diffusion import pipeline as P
    base = ["--prompt", "x", "-i", "in", "-o", "out", "--seed", "1"]
    assert P.build_parser().parse_args(base).calibrate_scope == "stream"
    for scope in ("stream", "all", "gemm"):
        assert P.build_parser().parse_args(base + ["--calibrate-scope", scope]).calibrate_scope == scope
    with pytest.raises(SystemExit):
        P.build_parser().parse_args(base + ["--calibrate-scope", "none"])
