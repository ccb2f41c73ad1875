"""CPU suite: the planner's side of the W8A8 halo conv (plan tile 18, conv3x3_halo_i8.hip) and its host weight packer.  Tile 18 is
tile 7's geometry - the same ring codes, split-K rule and slab workspace - pinned by a descriptor that carries int8 weights; it is
never the library's own answer, and every shape the kernel does not take is refused by name."""
import numpy as np
import pytest

from python_hip_stable_diffusion import _lib

# up_blocks.*.resnets.*.conv1-like 3x3 conv of the 16x16 level at CFG batch 2: timestep embedding, residual, bias
SHAPE = dict(ksize=3, stride=1, up=1, C0=1280, C1=0, N=1280, B=2, Ho=16, Wo=16, flags=2 | 4 | 16)


def plan(**kw):
    d = dict(SHAPE)
    d.update(kw)
    return _lib.conv_plan(d.pop("ksize"), d.pop("stride"), d.pop("up"), d.pop("C0"), d.pop("C1"), d.pop("N"), d.pop("B"), d.pop("Ho"), d.pop("Wo"), **d)


def test_tile_18_is_tile_7s_plan_from_int8():
    p18, p7 = plan(tile=18), plan(tile=7)
    assert p18["tile"] == 18 and p7["tile"] == 7
    assert p18["kernel"].startswith("halo_i8 ring") and p7["kernel"].startswith("halo_ks ring")
    assert (p18["staging"], p18["splitk"], p18["slab"], p18["workspace_bytes"]) == (p7["staging"], p7["splitk"], p7["slab"], p7["workspace_bytes"])
    assert p18["splitk"] >= 2 and p18["workspace_bytes"] == p18["splitk"] * 2 * 16 * 16 * 1280 * 4   # 32 workgroups per split: the rule splits
    assert p18["copies"] == (False, False, False)


def test_tile_18_is_never_the_librarys_own_answer():
    p = plan()
    assert p["tile"] == 7 and p["kernel"].startswith("halo_ks ring")
    for kw in (dict(Ho=32, Wo=32, C0=640, N=640), dict(Ho=64, Wo=64, C0=320, N=320), dict(up=2, Ho=32, Wo=32), dict(C0=1280, C1=640)):
        assert plan(**kw)["tile"] != 18


@pytest.mark.parametrize("staging, stages", [(0, 2), (2, 3), (3, 4), (4, 4), (5, 4)])
def test_ring_codes_are_tile_7s_capped_at_four_stages(staging, stages):
    p = plan(tile=18, staging=staging)
    assert p["staging"] == staging and p["kernel"] == f"halo_i8 ring{stages}"
    assert p["splitk"] == plan(tile=7, staging=staging)["splitk"]


@pytest.mark.parametrize("splitk", [1, 2, 3, 7, 20])
def test_forced_split_k_resolves_like_tile_7(splitk):
    p18, p7 = plan(tile=18, staging=3, splitk=splitk), plan(tile=7, staging=3, splitk=splitk)
    assert (p18["splitk"], p18["slab"], p18["workspace_bytes"]) == (p7["splitk"], p7["slab"], p7["workspace_bytes"])
    assert p18["splitk"] <= 20 and (p18["splitk"] > 1) == p18["slab"]


def test_twins_force_the_slab_path_as_for_tile_7():
    kw = dict(C0=128, N=128, n_twins=1, splitk=1)
    p18, p7 = plan(tile=18, **kw), plan(tile=7, **kw)
    assert p18["slab"] and (p18["splitk"], p18["workspace_bytes"]) == (p7["splitk"], p7["workspace_bytes"]) == (1, 2 * 16 * 16 * 128 * 4)


@pytest.mark.parametrize("kw", [
    dict(ksize=1),                                        # a 1x1 projection
    dict(stride=2, Ho=8, Wo=8),                           # a downsampler
    dict(C0=32),                                          # 32 channels: off the 64-channel chunks
    dict(C0=14848),                                       # 127 * 127 * 9 * Ctot >= 2^31
    dict(C0=7424, C1=7424),                               # ... over both sources
    dict(Ho=4, Wo=16),                                    # an image lower than the tile's halo rule takes
    dict(gnf_groups=32, C0=320, N=320),                   # GroupNorm in the loader: tile 7 only
])
def test_shapes_tile_18_refuses(kw):
    with pytest.raises(ValueError, match="plan tile 18"):
        plan(tile=18, **kw)


def test_the_int32_bound_is_the_last_chunk_that_fits():
    assert 127 * 127 * 9 * 14784 < 2 ** 31 <= 127 * 127 * 9 * (14784 + 64)
    assert plan(tile=18, C0=14784)["tile"] == 18
    assert plan(tile=18, C0=7424, C1=7360)["tile"] == 18


@pytest.mark.parametrize("kw", [dict(up=2, Ho=32, Wo=32), dict(C0=1280, C1=640), dict(up=2, C0=1280, C1=640, Ho=32, Wo=32), dict(N=68, C0=64, Ho=12, Wo=24)])
def test_upsampling_two_source_and_ragged_descriptors_are_accepted(kw):
    p18, p7 = plan(tile=18, **kw), plan(tile=7, **kw)
    assert p18["tile"] == 18 and (p18["splitk"], p18["workspace_bytes"]) == (p7["splitk"], p7["workspace_bytes"])


# ---- the host packer ----
def numpy_pack(wq):
    """(Cout, Ctot, 3, 3) -> (Cout, 9, Ctot): tap-major, the fp16 halo kernel's K order"""
    return np.ascontiguousarray(wq.reshape(wq.shape[0], wq.shape[1], 9).transpose(0, 2, 1))


@pytest.mark.parametrize("cout, ctot", [(64, 64), (68, 128), (4, 192), (33, 64)])
def test_packer_is_the_numpy_restatement(cout, ctot):
    rs = np.random.RandomState(cout * 1000 + ctot)
    wq = rs.randint(-127, 128, size=(cout, ctot, 3, 3)).astype(np.int8)
    got = _lib.w8a8_pack_halo(wq)
    assert got.dtype == np.int8 and got.shape == (cout, 9, ctot) and np.array_equal(got, numpy_pack(wq))
    # row n, tap t, chunk c of the kernel's DMA: 64 contiguous bytes
    n, t, c = cout - 1, 5, ctot // 64 - 1
    assert np.array_equal(got.reshape(-1)[(n * 9 + t) * ctot + 64 * c:][:64], wq[n, 64 * c:64 * c + 64, t // 3, t % 3])


def test_packer_refusals():
    with pytest.raises(ValueError):
        _lib.w8a8_pack_halo(np.zeros((64, 32, 3, 3), np.int8))                    # not whole 64-channel chunks
    with pytest.raises(ValueError):
        _lib.w8a8_pack_halo(np.zeros((64, 64, 1, 1), np.int8))


def test_observe_levels():
    from python_hip_stable_diffusion import hip_model
    assert [hip_model.observe_level(v) for v in (False, True, "all")] == [0, 1, 2]
    with pytest.raises(ValueError):
        hip_model.observe_level("everything")
    store = hip_model.Weights(tensors={"w": np.zeros((4, 4), np.float32)})
    try:
        for on in (True, "all", False):
            store.observe_activations(on)
        with pytest.raises(ValueError):
            _lib.check(_lib.lib().sd_weights_observe_activations(store._h, 3))
    finally:
        store.close()


def test_cli_has_the_calibrate_scope_flag():
    from python_hip_stable_diffusion import pipeline as P
    base = ["--prompt", "x", "-i", "in", "-o", "out", "--seed", "1"]
    assert P.build_parser().parse_args(base).calibrate_scope == "stream"
    assert P.build_parser().parse_args(base + ["--calibrate-scope", "all"]).calibrate_scope == "all"
    with pytest.raises(SystemExit):
        P.build_parser().parse_args(base + ["--calibrate-scope", "none"])
