"""CPU suite: palettized weights on the host - the exact 1-D k-means of sd_weights_palettize, the palette store, the index bit
stream of the palettized weight-stream conv, recipes and the CLI flags.  Through ctypes, no device."""
import ctypes as C
import itertools
import json

import numpy as np
import pytest

from python_hip_stable_diffusion import _lib, hip_model, palettize
from python_hip_stable_diffusion import pipeline as P

NBITS = (1, 2, 4, 6, 8)


def _store(**tensors):
    return hip_model.Weights({k + ".weight": v for k, v in tensors.items()})


def _inertia(values, indices):
    """float64 inertia of a partition with unrounded cluster means"""
    v = values.astype(np.float64).ravel()
    idx = indices.ravel()
    total = 0.0
    for c in np.unique(idx):
        m = v[idx == c]
        total += float(((m - m.mean()) ** 2).sum())
    return total


def _brute_force(values, k):
    """least inertia over all partitions of the sorted values into k contiguous non-empty ranges"""
    v = np.sort(values.astype(np.float64).ravel())
    u = np.unique(v)
    best = np.inf
    for cuts in itertools.combinations(range(1, len(u)), k - 1):
        edges = (0,) + cuts + (len(u),)
        total = 0.0
        for a, b in zip(edges[:-1], edges[1:]):
            m = v[(v >= u[a]) & (v <= u[b - 1])]
            total += float(((m - m.mean()) ** 2).sum())
        best = min(best, total)
    return best


@pytest.mark.parametrize("nbits", (1, 2))
def test_partition_is_the_brute_force_optimum(nbits):
    rs = np.random.RandomState(7 + nbits)
    for trial in range(12):
        n_distinct = int(rs.randint((1 << nbits) + 1, 13))
        pool = (rs.randn(n_distinct) * 0.05).astype(np.float16)
        assert len(np.unique(pool)) == n_distinct
        x = pool[rs.randint(0, n_distinct, size=64)]
        x[:n_distinct] = pool                                   # every value present
        w = _store(t=x.reshape(8, 8))
        w.palettize("t.weight", nbits)
        lut, idx = w.read_palette("t.weight")
        got, want = _inertia(x.reshape(8, 8), idx), _brute_force(x, 1 << nbits)
        assert got <= want * (1 + 1e-9) + 1e-18, (trial, got, want)
        # ranges are contiguous in value: the index never decreases along the sorted values
        order = np.argsort(x, kind="stable")
        assert np.all(np.diff(idx.ravel()[order].astype(int)) >= 0)
        w.close()


@pytest.mark.parametrize("nbits", (2, 4, 6, 8))
def test_inertia_is_not_above_scikit_learns_kmeans(nbits):
    cluster = pytest.importorskip("sklearn.cluster")
    x = (np.random.RandomState(0).randn(256, 256) * 0.03).astype(np.float16)
    w = _store(t=x)
    w.palettize("t.weight", nbits)
    _, idx = w.read_palette("t.weight")
    km = cluster.KMeans(1 << nbits, n_init=1, random_state=0).fit(x.astype(np.float64).reshape(-1, 1))
    got = _inertia(x, idx)
    print(f"nbits {nbits}: DP inertia {got:.6e}, scikit-learn {km.inertia_:.6e}")
    assert got <= km.inertia_ * (1 + 1e-6)
    w.close()


@pytest.mark.parametrize("nbits", NBITS)
def test_palette_structure(nbits):
    x32 = (np.random.RandomState(3).randn(48, 40) * 0.03).astype(np.float32)    # fp32 in: clustered as fp16
    x = x32.astype(np.float16)
    w = hip_model.Weights({"t.weight": x32})
    assert w.palette_bits("t.weight") == 0
    err = w.palettize("t.weight", nbits)
    assert w.palette_bits("t.weight") == nbits
    lut, idx = w.read_palette("t.weight")
    assert lut.shape == (1 << nbits,) and idx.shape == x.shape and idx.max() < (1 << nbits)
    assert np.all(np.diff(lut.astype(np.float64)) >= 0)                         # ascending
    assert np.array_equal(w.read("t.weight"), lut[idx].astype(np.float32))      # stored data == lut[indices]
    recomputed = float(((x.astype(np.float64) - lut[idx].astype(np.float64)) ** 2).sum())
    assert err == pytest.approx(recomputed, rel=1e-12, abs=1e-30)
    w2 = hip_model.Weights({"t.weight": x32})                                   # a second run: the same bits
    assert w2.palettize("t.weight", nbits) == err
    lut2, idx2 = w2.read_palette("t.weight")
    assert np.array_equal(lut.view(np.uint16), lut2.view(np.uint16)) and np.array_equal(idx, idx2)
    w.add("t.weight", x32)                                                      # plain values drop the palette
    assert w.palette_bits("t.weight") == 0
    w.close()
    w2.close()


@pytest.mark.parametrize("nbits", NBITS)
def test_few_distinct_values_are_reconstructed_exactly(nbits):
    rs = np.random.RandomState(nbits)
    for n_distinct in sorted({1, 2, 1 << nbits, max(1, (1 << nbits) - 1)}):
        pool = np.unique((rs.randn(4 * n_distinct + 8) * 0.1).astype(np.float16))[:n_distinct]
        x = pool[rs.randint(0, len(pool), size=(16, 24))]
        w = _store(t=x)
        assert w.palettize("t.weight", nbits) == 0.0
        lut, idx = w.read_palette("t.weight")
        assert np.array_equal(lut[idx], x) and np.array_equal(w.read("t.weight"), x.astype(np.float32))
        assert np.all(lut[len(pool) - 1:] == pool[-1])                          # the last value repeated
        w.close()


def test_add_palettized_round_trips_and_refusals():
    rs = np.random.RandomState(5)
    w = hip_model.Weights()
    for nbits in NBITS:
        lut = (rs.randn(1 << nbits)).astype(np.float16)
        lut[0] = np.float16(-0.0)
        idx = rs.randint(0, 1 << nbits, size=(6, 5, 3, 3)).astype(np.uint8)
        w.add_palettized(f"p{nbits}.weight", lut, idx, nbits)
        assert w.palette_bits(f"p{nbits}.weight") == nbits
        lut2, idx2 = w.read_palette(f"p{nbits}.weight")
        assert np.array_equal(lut.view(np.uint16), lut2.view(np.uint16)) and np.array_equal(idx, idx2)
        assert np.array_equal(w.read(f"p{nbits}.weight"), lut[idx].astype(np.float32))
    assert w.shapes()["p4.weight"] == (6, 5, 3, 3) and len(w) == len(NBITS)
    lib = _lib.lib()
    lut = np.zeros(256, np.float16)
    idx = np.zeros((4, 4), np.uint8)
    shape = (C.c_int64 * 2)(4, 4)
    err = C.c_double(0)
    for bad in (0, 3, 5, 7, 9, 16, -1):                                         # before any work, also for an unknown name
        assert lib.sd_weights_palettize(w._h, b"p4.weight", bad, C.byref(err)) == -1
        assert lib.sd_weights_palettize(w._h, b"missing.weight", bad, C.byref(err)) == -1
        assert lib.sd_weights_add_palettized(w._h, b"q.weight", _lib.ptr(lut), bad, _lib.ptr(idx), shape, 2) == -1
        with pytest.raises(ValueError):
            w.palettize("p4.weight", bad)
    assert lib.sd_weights_palettize(w._h, b"missing.weight", 4, C.byref(err)) == -2
    assert b"missing.weight" in lib.sd_last_error()
    with pytest.raises(KeyError):
        w.palettize("missing.weight", 4)
    idx[3, 3] = 4                                                               # index >= 2^nbits
    assert lib.sd_weights_add_palettized(w._h, b"q.weight", _lib.ptr(lut), 2, _lib.ptr(idx), shape, 2) == -1
    assert w.palette_bits("q.weight") == 0 and "q.weight" not in w.shapes()
    idx[3, 3] = 3
    assert lib.sd_weights_add_palettized(w._h, b"q.weight", _lib.ptr(lut), 2, _lib.ptr(idx), shape, 2) == 0
    assert lib.sd_weights_palette_bits(w._h, b"missing.weight") == 0
    w.close()


def _pack_reference(indices, nbits):
    """The bit-stream layout restated: per (strip, slice, lane) the 16 * taps indices of the lane's MFMA fragments (fragment j,
    element e: row strip * 32 + (lane & 31), channel slice * 32 + (j & 1) * 16 + (lane >> 5) * 8 + e, tap j >> 1) as little-endian
    nbits-wide fields, padded to whole 16-byte words; word q of all lanes at [strip][slice][q][lane]."""
    N, Ctot, k, _ = indices.shape
    taps = k * k
    idx = indices.reshape(N, Ctot, taps)
    nf = 2 * taps
    words = (nf * 8 * nbits + 127) // 128
    out = np.zeros((N // 32, Ctot // 32, words, 64, 16), np.uint8)
    lane = np.arange(64)
    for strip in range(N // 32):
        for sl in range(Ctot // 32):
            big = [0] * 64                                                       # one Python integer per lane
            for j in range(nf):
                for e in range(8):
                    f = j * 8 + e
                    v = idx[strip * 32 + (lane & 31), sl * 32 + (j & 1) * 16 + (lane >> 5) * 8 + e, j >> 1]
                    for ln in range(64):
                        big[ln] |= int(v[ln]) << (f * nbits)
            for ln in range(64):
                raw = np.frombuffer(big[ln].to_bytes(words * 16, "little"), np.uint8)
                out[strip, sl, :, ln, :] = raw.reshape(words, 16)
    return out


@pytest.mark.parametrize("ksize", (1, 3))
@pytest.mark.parametrize("nbits", NBITS)
def test_bit_stream_layout(nbits, ksize):
    rs = np.random.RandomState(10 * nbits + ksize)
    N, Ctot = 64, 96
    top = (1 << nbits) - 1
    idx = rs.randint(0, top + 1, size=(N, Ctot, ksize, ksize)).astype(np.uint8)
    # the first and the last field of a lane, at both ends of the index range: lane 0 / lane 63 of (strip 0, slice 0) and of the
    # last (strip, slice): field 0 = (row, channel + 0, tap 0), last field = (row, channel + 16 + 7, last tap)
    for (n, c), (first, last) in {(0, 0): (0, top), (31, 8): (top, 0), (N - 32, Ctot - 32): (top, top), (N - 1, Ctot - 24): (0, 0)}.items():
        idx[n, c, 0, 0] = first
        idx[n, c + 16 + 7, ksize - 1, ksize - 1] = last
    got = _lib.palette_pack(idx, nbits)
    want = _pack_reference(idx, nbits)
    assert got.shape == want.shape
    assert got.shape[2] == {9: {8: 9, 6: 7, 4: 5, 2: 3, 1: 2}, 1: {8: 1, 6: 1, 4: 1, 2: 1, 1: 1}}[ksize * ksize][nbits]
    assert np.array_equal(got, want)


def test_bit_stream_refusals():
    lib = _lib.lib()
    n = C.c_size_t(0)
    idx = np.zeros((32, 32, 1, 1), np.uint8)
    assert lib.sd_op_palette_pack(_lib.ptr(idx), 32, 32, 1, 3, None, C.byref(n)) == -1
    assert lib.sd_op_palette_pack(_lib.ptr(idx), 32, 48, 1, 4, None, C.byref(n)) == -1
    assert lib.sd_op_palette_pack(_lib.ptr(idx), 32, 32, 2, 4, None, C.byref(n)) == -1
    assert lib.sd_op_palette_pack(_lib.ptr(idx), 32, 32, 1, 4, None, C.byref(n)) == 0 and n.value == 1024


# ---- recipes and the CLI ----
def _checkpoint():
    rs = np.random.RandomState(1)
    return {"a.conv.weight": rs.randn(8, 8, 3, 3).astype(np.float16),          # 576
            "a.conv.bias": rs.randn(8).astype(np.float16),
            "b.proj.weight": rs.randn(40, 30).astype(np.float16),              # 1200
            "c.norm.weight": rs.randn(2000).astype(np.float16),                # 1-D: never
            "d.small.weight": rs.randn(4, 4).astype(np.float16)}


def test_palettizable_follows_the_reference_rule():
    ck = _checkpoint()
    w = hip_model.Weights(ck)
    assert palettize.PALETTIZE_MIN_SIZE == 1e5
    assert palettize.palettizable(w) == [] == palettize.palettizable(ck)
    assert palettize.palettizable(w, min_size=500) == ["a.conv", "b.proj"] == palettize.palettizable(ck, min_size=500)
    assert palettize.palettizable(w, min_size=576) == ["b.proj"]                # strictly more than min_size
    w.close()


def test_recipe_parsing_and_application(tmp_path):
    pre = {"model_version": "stabilityai/stable-diffusion-2-1-base",
           "recipes": {"recipe_4.50_bit_mixedpalette": {"a.conv": 4, "b.proj": 16}, "bad": {"a.conv": 3}}}
    path = tmp_path / "pre_analysis.json"
    path.write_text(json.dumps(pre))
    recipe = palettize.load_recipe(str(path), "recipe_4.50_bit_mixedpalette")
    assert recipe == {"a.conv": 4, "b.proj": 16} == palettize.load_recipe(pre, "recipe_4.50_bit_mixedpalette")
    with pytest.raises(KeyError, match="recipe_9"):
        palettize.load_recipe(str(path), "recipe_9")
    with pytest.raises(ValueError):
        palettize.load_recipe(str(path), "bad")
    w = hip_model.Weights(_checkpoint())
    errs = palettize.apply(w, recipe=recipe)
    assert list(errs) == ["a.conv"] and errs["a.conv"] > 0
    assert w.palette_bits("a.conv.weight") == 4 and w.palette_bits("b.proj.weight") == 0      # 16 = left alone
    assert w.palette_bits("a.conv.bias") == 0
    with pytest.raises(KeyError, match="no.such.module"):
        palettize.apply(w, recipe={"b.proj": 2, "no.such.module": 4})
    assert w.palette_bits("b.proj.weight") == 0                                 # nothing was changed by the refused recipe
    # a model that shares only some of the recipe's modules (ControlNet, refiner): strict=False takes those and skips the rest
    errs = palettize.apply(w, recipe={"b.proj": 2, "no.such.module": 4}, strict=False)
    assert list(errs) == ["b.proj"] and w.palette_bits("b.proj.weight") == 2
    with pytest.raises(ValueError):
        palettize.apply(w, nbits=4, recipe=recipe)
    with pytest.raises(ValueError):
        palettize.apply(w, nbits=5)
    w.close()
    big = hip_model.Weights({"e.weight": np.zeros((400, 300), np.float16), "f.weight": np.zeros((10, 10), np.float16)})
    assert list(palettize.apply(big, nbits=6)) == ["e"]                         # uniform: the palettizable modules only
    assert big.palette_bits("e.weight") == 6 and big.palette_bits("f.weight") == 0
    big.close()


def test_cli_palettization_flags_reach_get_hip_pipe(tmp_path, monkeypatch):
    base = ["--prompt", "p", "-i", "in", "-o", str(tmp_path)]
    a = P.build_parser().parse_args(base)
    assert a.quantize_nbits is None and a.pre_analysis_json_path is None and a.selected_recipe is None
    assert P.build_parser().parse_args(base + ["--quantize-nbits", "6"]).quantize_nbits == 6
    for bad in ("3", "16", "six"):
        with pytest.raises(SystemExit):
            P.build_parser().parse_args(base + ["--quantize-nbits", bad])
    seen = {}

    class Stop(Exception):
        pass

    def fake_get_hip_pipe(*args, **kwargs):
        seen.update(kwargs)
        raise Stop

    monkeypatch.setattr(P, "get_hip_pipe", fake_get_hip_pipe)
    with pytest.raises(Stop):
        P.main(P.build_parser().parse_args(base + ["--quantize-nbits", "4"]))
    assert seen["quantize_nbits"] == 4 and seen["palettization_recipe"] is None
    path = tmp_path / "pre.json"
    path.write_text(json.dumps({"model_version": "m", "recipes": {"r": {"mid_block.resnets.0.conv1": 2, "conv_in": 16}}}))
    seen.clear()
    with pytest.raises(Stop):
        P.main(P.build_parser().parse_args(base + ["--pre-analysis-json-path", str(path), "--selected-recipe", "r"]))
    assert seen["quantize_nbits"] is None and seen["palettization_recipe"] == {"mid_block.resnets.0.conv1": 2, "conv_in": 16}
    with pytest.raises(ValueError):                                              # one without the other
        P.main(P.build_parser().parse_args(base + ["--selected-recipe", "r"]))
    with pytest.raises(ValueError):
        P.main(P.build_parser().parse_args(base + ["--pre-analysis-json-path", str(path), "--selected-recipe", "r",
                                                   "--quantize-nbits", "4"]))
    with pytest.raises(ValueError):                                              # validated before any device work
        hip_model.HipModel("stabilityai/stable-diffusion-2-1-base", weights={}, quantize_nbits=3)
