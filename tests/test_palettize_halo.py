"""CPU suite: the host side of the palettized 3x3 halo conv (plan tile 25, conv3x3_halo_pal.hip) - its index stream, the planner's
answers, the operator entry's refusals in their documented order, the store switch and the CLI flag.  Tile 25 is tile 7's geometry
- the same ring codes, split-K rule and slab workspace - pinned by a descriptor that carries a palette; it is never the library's own
answer, and every shape the kernel does not take is refused by name.

The stream layout, restated (weight_prep.h halo_pal_pack): a compact bit stream, no padding bits; rows are padded to a multiple of 64
with index 0.  Per (64-row n-tile, 64-channel chunk, tap), in that order, one block of nbits * 128 dwords.  Inside a block, dword j of
stream (wk, lane) - wk = 0, 1 the K half, lane 0 .. 63 - is at [j][wk][lane].  A stream is the lane's 32 indices of that step as
little-endian nbits-wide fields: field (2 s + j) * 8 + e = row j * 32 + (lane & 31), channel (2 (2 wk + s) + (lane >> 5)) * 8 + e of
the chunk."""
import numpy as np
import pytest

from python_hip_stable_diffusion import _lib, hip_model
from test_w8a8_halo_gpu import SHAPES

NBITS = (1, 2, 4, 6, 8)
RING = {0: 2, 2: 3, 3: 4, 4: 6, 5: 8}          # plan tile 7's ring code -> weight stages


# ---- the packer ----
def numpy_pack(indices, nbits):
    """the layout of the module docstring in numpy: (n_tiles, chunks, 9, nbits dwords, 2 K halves, 64 lanes, 4 bytes)"""
    cout, ctot = indices.shape[:2]
    nt, nch = -(-cout // 64), ctot // 64
    padded = np.zeros((nt * 64, ctot, 9), np.uint8)
    padded[:cout] = indices.reshape(cout, ctot, 9)
    t, c, wk, lane, s, j, e = np.meshgrid(np.arange(nt), np.arange(nch), np.arange(2), np.arange(64), np.arange(2), np.arange(2), np.arange(8), indexing="ij")
    rows = t * 64 + j * 32 + (lane & 31)
    chans = c * 64 + (2 * (2 * wk + s) + (lane >> 5)) * 8 + e
    fields = padded[rows, chans]                                                 # (nt, nch, wk, lane, s, j, e, tap): field (2 s + j) * 8 + e
    fields = np.moveaxis(fields, -1, 2).reshape(nt, nch, 9, 2, 64, 32)           # (nt, nch, tap, wk, lane, field)
    bits = (fields[..., None] >> np.arange(nbits, dtype=np.uint8)) & 1           # little-endian bits of every field
    stream = np.packbits(bits.reshape(nt, nch, 9, 2, 64, 32 * nbits), axis=-1, bitorder="little")   # nbits dwords, little-endian bytes
    return np.ascontiguousarray(np.moveaxis(stream.reshape(nt, nch, 9, 2, 64, nbits, 4), 5, 3))


@pytest.mark.parametrize("nbits", NBITS)
@pytest.mark.parametrize("cout, ctot", [(64, 64), (68, 128), (4, 192)])
def test_packer_is_the_numpy_restatement(cout, ctot, nbits):
    rs = np.random.RandomState(cout * 1000 + ctot + nbits)
    indices = rs.randint(0, 1 << nbits, size=(cout, ctot, 3, 3)).astype(np.uint8)
    indices.reshape(-1)[:2] = [(1 << nbits) - 1, 0]
    got = _lib.palette_pack_halo(indices, nbits)
    nt = -(-cout // 64)
    assert got.dtype == np.uint8 and got.shape == (nt, ctot // 64, 9, nbits, 2, 64, 4)
    assert got.size == nt * 64 * 9 * ctot * nbits // 8                            # the size formula: no padding bits
    assert np.array_equal(got, numpy_pack(indices, nbits))
    # a NULL stream returns the size alone
    n = _lib.C.c_size_t(0)
    _lib.check(_lib.lib().sd_op_palette_pack_halo(_lib.ptr(indices), cout, ctot, nbits, None, _lib.C.byref(n)))
    assert n.value == got.size
    # row padding carries index 0: with every real index at its maximum, the padded rows' fields are the only zero bits
    if cout % 64:
        ones = _lib.palette_pack_halo(np.full_like(indices, (1 << nbits) - 1), nbits)
        set_bits = int(np.unpackbits(ones).sum())
        assert set_bits == cout * ctot * 9 * nbits and ones.size * 8 - set_bits == (nt * 64 - cout) * ctot * 9 * nbits


def test_packer_refusals():
    with pytest.raises(ValueError):
        _lib.palette_pack_halo(np.zeros((64, 32, 3, 3), np.uint8), 4)             # not whole 64-channel chunks
    with pytest.raises(ValueError):
        _lib.palette_pack_halo(np.zeros((64, 64, 1, 1), np.uint8), 4)
    with pytest.raises(ValueError):
        _lib.palette_pack_halo(np.zeros((64, 64, 3, 3), np.uint8), 3)


# ---- the planner ----
def plan_of(shape, **kw):
    B, C0, C1, H, W, Cout, ups, splitk = shape
    up = 2 if ups else 1
    return _lib.conv_plan(3, 1, up, C0, C1, Cout, B, H * up, W * up, splitk=splitk, **kw)


@pytest.mark.parametrize("name", list(SHAPES))
def test_tile_25_is_tile_7s_plan_from_a_palette(name):
    for staging, depth in RING.items():
        for flags in (0, 2 | 4 | 16):
            p25, p7 = plan_of(SHAPES[name], tile=25, staging=staging, flags=flags), plan_of(SHAPES[name], tile=7, staging=staging, flags=flags)
            assert p25["tile"] == 25 and p7["tile"] == 7
            assert (p25["staging"], p25["splitk"], p25["slab"], p25["workspace_bytes"]) == (p7["staging"], p7["splitk"], p7["slab"], p7["workspace_bytes"])
            assert p25["staging"] == staging and p7["kernel"] == f"halo_ks ring{depth}" and p25["kernel"] == f"halo_pal ring{depth}"
            assert p25["copies"] == (False, False, False)
    assert plan_of(SHAPES[name], tile=0)["tile"] != 25                            # never the library's own answer


def test_tile_25_follows_the_librarys_split_k_rule_like_tile_7():
    kw = dict(ksize=3, stride=1, up=1, C0=1280, C1=0, N=1280, B=2, Ho=16, Wo=16, flags=2 | 4 | 16)
    p25, p7, p0 = _lib.conv_plan(**kw, tile=25), _lib.conv_plan(**kw, tile=7), _lib.conv_plan(**kw)
    assert p0["tile"] == 7 and p25["tile"] == 25
    assert (p25["staging"], p25["splitk"], p25["slab"], p25["workspace_bytes"]) == (p7["staging"], p7["splitk"], p7["slab"], p7["workspace_bytes"])
    assert p25["splitk"] >= 2 and p25["workspace_bytes"] == p25["splitk"] * 2 * 16 * 16 * 1280 * 4
    for shape in (dict(Ho=32, Wo=32, C0=640, N=640), dict(Ho=64, Wo=64, C0=320, N=320), dict(up=2, Ho=32, Wo=32), dict(C0=1280, C1=640),
                  dict(Ho=8, Wo=8)):
        assert _lib.conv_plan(**dict(kw, **shape))["tile"] != 25


@pytest.mark.parametrize("kw", [
    dict(stride=2, Ho=8, Wo=8),                           # a downsampler
    dict(ksize=1),                                        # a 1x1 projection
    dict(C0=32),                                          # C0 % 64 != 0
    dict(N=66),                                           # N % 4 != 0
    dict(Ho=16, Wo=4),                                    # a 4-pixel-wide image
    dict(gnf_groups=32, C0=320, N=320),                   # GroupNorm in the loader: tile 7 only
])
def test_shapes_tile_25_refuses(kw):
    d = dict(ksize=3, stride=1, up=1, C0=128, C1=0, N=128, B=2, Ho=16, Wo=16)
    d.update(kw)
    with pytest.raises(ValueError, match="plan tile 25"):
        _lib.conv_plan(**d, tile=25)


# ---- the operator entry's refusals, in the header's order; none of them needs a GPU ----
def test_operator_refusals_in_their_documented_order():
    lib = _lib.lib()
    x = np.zeros((1, 64, 8, 16), np.float16)
    lut = np.zeros(256, np.float16)
    idx = np.zeros((64, 64, 3, 3), np.uint8)
    out = np.empty(64 * 128, np.float16)

    def call(**kw):
        a = dict(x=_lib.ptr(x), lut=_lib.ptr(lut), nbits=4, idx=_lib.ptr(idx), out=_lib.ptr(out), B=1, Cin=64, C1=0, H=8, W=16, Cout=64, up=0, staging=3,
                 splitk=0)
        a.update(kw)
        status = lib.sd_op_conv2d_palettized_halo(a["x"], None, a["lut"], a["nbits"], a["idx"], None, None, None, a["out"], a["B"], a["Cin"], a["C1"],
                                                  a["H"], a["W"], a["Cout"], a["up"], a["staging"], a["splitk"], None, 1, None)
        return status, lib.sd_last_error().decode()

    bad_idx = idx.copy()
    bad_idx[5, 7, 1, 1] = 16                                                     # >= 2^4
    # one failure per check, in the header's order, and what its message says
    stages = [(dict(x=None), "NULL argument"), (dict(nbits=3), "nbits = 3"), (dict(B=0), "empty problem"), (dict(staging=1), "staging 1"),
              (dict(Cin=32), "plan tile 25"), (dict(idx=_lib.ptr(bad_idx)), "index 16")]
    for k, (_, message) in enumerate(stages):
        kw = {}
        for later, _ in stages[k:]:                                              # this check fails together with every LATER one ...
            kw.update(later)
        status, text = call(**kw)
        assert status == -1 and message in text, (k, text)                       # ... and the message is this check's (SD_ERR_INVALID_ARGUMENT)
    # every argument of every check, alone
    for kw, message in [(dict(lut=None), "NULL"), (dict(idx=None), "NULL"), (dict(out=None), "NULL"), (dict(nbits=0), "nbits = 0"),
                        (dict(nbits=16), "nbits = 16"), (dict(H=0), "empty problem"), (dict(C1=64), "empty problem"), (dict(up=2), "upsample 2"),
                        (dict(staging=6), "staging 6"), (dict(splitk=-1), "splitk -1"), (dict(Cout=66), "plan tile 25"), (dict(H=4), "plan tile 25"),
                        (dict(W=4), "plan tile 25")]:
        status, text = call(**kw)
        assert status == -1 and message in text, (kw, text)
    status, text = call(idx=_lib.ptr(bad_idx))
    assert status == -1 and "index 16" in text and "element" in text and "16 entries" in text
    with pytest.raises(ValueError, match="plan tile 25"):                        # the Python wrapper passes the library's refusal on
        _lib.conv2d_palettized_halo(np.zeros((1, 32, 8, 16), np.float16), lut[:16], idx[:, :32], 4)


# ---- the store switch and the CLI flag ----
def test_store_switch_takes_0_and_1_and_refuses_2():
    store = hip_model.Weights(tensors={"w": np.zeros((4, 4), np.float32)})
    try:
        lib = _lib.lib()
        assert lib.sd_weights_palette_halo(store._h, 1) == 0 and lib.sd_weights_palette_halo(store._h, 0) == 0
        assert lib.sd_weights_palette_halo(store._h, 2) == -1 and lib.sd_weights_palette_halo(store._h, -1) == -1
        assert lib.sd_weights_palette_halo(None, 1) == -1
        for on in (True, False):
            store.palette_halo(on)
        with pytest.raises(ValueError):
            store.palette_halo(2)
    finally:
        store.close()


def test_cli_refuses_palette_halo_without_a_palettization_option():
    from python_hip_stable_diffusion import pipeline as P
    base = ["--prompt", "x", "-i", "in", "-o", "out", "--seed", "1"]
    assert P.build_parser().parse_args(base).palette_halo is False
    assert P.build_parser().parse_args(base + ["--palette-halo"]).palette_halo is True
    with pytest.raises(ValueError, match="--palette-halo"):
        P.main(P.build_parser().parse_args(base + ["--palette-halo"]))
