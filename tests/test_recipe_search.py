"""CPU suite of the mixed-bit recipe search (python_hip_stable_diffusion.mixed_bit_compression_pre_analysis) and of
Weights.set_values: the loop's logic against a toy numpy model in a real Weights store, build_recipe against a table worked out by
hand, the package's compute_psnr against the oracle's, the fake linear quantizer's three properties.  No GPU."""
import json
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from oracle import psnr as oracle_psnr
from python_hip_stable_diffusion import _lib, hip_model, palettize
from python_hip_stable_diffusion import mixed_bit_compression_pre_analysis as search_mod


# ---- set_values ----
def test_set_values_overwrites_in_place_and_drops_a_palette_mark():
    rs = np.random.RandomState(1)
    a = rs.randn(6, 5, 3, 3).astype(np.float32)
    w = hip_model.Weights({"a.weight": a, "b.weight": rs.randn(4, 4, 1, 1).astype(np.float16)})
    w.palettize("a.weight", 2)
    assert w.palette_bits("a.weight") == 2 and len(np.unique(w.read("a.weight"))) <= 4
    new = rs.randn(6, 5, 3, 3).astype(np.float32)
    w.set_values("a.weight", new)
    assert w.palette_bits("a.weight") == 0
    assert np.array_equal(w.read("a.weight"), new) and w.shapes()["a.weight"] == (6, 5, 3, 3)
    w.quantize_w8a8("b.weight", 3.0)
    assert w.w8a8_info("b.weight") is not None
    w.set_values("b.weight", np.ones(16))
    assert w.w8a8_info("b.weight") is None and np.array_equal(w.read("b.weight"), np.ones((4, 4, 1, 1), np.float32))
    with pytest.raises(ValueError, match="269"):
        w.set_values("a.weight", np.zeros(269))
    with pytest.raises(KeyError):
        w.set_values("c.weight", np.zeros(4))
    assert np.array_equal(w.read("a.weight"), new)                               # the refused calls changed nothing
    w.close()


def test_the_header_declares_the_two_symbols_and_the_library_exports_them():
    header = open(os.path.join(ROOT, "include", "sd_mi355x.h")).read()
    assert re.search(r"^int sd_weights_set_values\(sd_weights\* w, const char\* name, const float\* values, size_t n\);", header, re.M)
    assert re.search(r"^int sd_unet_reload_weights\(sd_unet\* u, const sd_weights\* w, const char\* const\* names, int n_names\);", header, re.M)
    names = [s[0] for s in _lib.SYMBOLS]
    for sym in ("sd_weights_set_values", "sd_unet_reload_weights"):
        assert sym in names and hasattr(_lib.lib(), sym)


# ---- compute_psnr ----
def test_compute_psnr_is_the_oracles():
    rs = np.random.RandomState(7)
    for shape, noise in (((4, 8, 8), 0.1), ((1, 4, 16, 16), 1e-3), ((33,), 2.0)):
        a = rs.randn(*shape).astype(np.float32)
        b = (a + noise * rs.randn(*shape)).astype(np.float32)
        assert search_mod.compute_psnr(a, b) == oracle_psnr.compute_psnr(a, b)
        assert search_mod.compute_psnr(b, a) == oracle_psnr.compute_psnr(b, a)   # the peak is the second argument's
        assert search_mod.compute_psnr(a, b) != search_mod.compute_psnr(b, a)
    same = search_mod.compute_psnr(a, a)
    assert np.isfinite(same) and same == oracle_psnr.compute_psnr(a, a)
    assert search_mod.rounded(same) == float(f"{same:.1f}")


# ---- build_recipe ----
def test_build_recipe_on_a_hand_written_table():
    """Threshold 30 dB (strictly above), default 16 bits, two prompts.
    a (100 elements): 11 / 15 / 21 / 26 / 30.0 dB on average - never ABOVE 30 -> 16 bits.
    b (300): 32 dB at 1 bit -> 1 bit.
    c (600): 20 at 1 bit, 35 at 2 bits, 25 at 4 bits (not monotonic) -> 2 bits, the first width that passes.
    bits = 16 * 100 + 1 * 300 + 2 * 600 = 3100; average = 3100 / 1000 = 3.1; size = 3100 / 8e6 MB."""
    table = {
        "1": {"metadata": {"nbits": 1}, "a": [10.0, 12.0], "b": [31.0, 33.0], "c": [20.0, 20.0]},
        "2": {"metadata": {"nbits": 2}, "a": [15.0, 15.0], "b": [40.0, 40.0], "c": [35.0, 35.0]},
        "4": {"metadata": {"nbits": 4}, "a": [20.0, 22.0], "b": [45.0, 45.0], "c": [25.0, 25.0]},
        "6": {"metadata": {"nbits": 6}, "a": [25.0, 27.0], "b": [50.0, 50.0], "c": [50.0, 50.0]},
        "8": {"metadata": {"nbits": 8}, "a": [30.0, 30.0], "b": [55.0, 55.0], "c": [55.0, 55.0]},
    }
    recipe, stats = search_mod.build_recipe(table, {"a": 100, "b": 300, "c": 600}, 30.0, 16)
    assert recipe == {"a": 16, "b": 1, "c": 2}
    assert stats["nbits"] == 3100 / 1000 and stats["size_mb"] == 3100 / 8e6
    assert f"recipe_{stats['nbits']:.2f}_bit_mixedpalette" == "recipe_3.10_bit_mixedpalette"
    # a default other than 16 is what a tensor that never passes gets
    recipe8, stats8 = search_mod.build_recipe(table, {"a": 100, "b": 300, "c": 600}, 30.0, 8)
    assert recipe8 == {"a": 8, "b": 1, "c": 2} and stats8["nbits"] == (800 + 300 + 1200) / 1000


# ---- the loop on a toy model ----
N_LAYERS, N_PROMPTS = 12, 3
WIDTHS = (2, 6)


def toy_state():
    rs = np.random.RandomState(5)
    sd = {f"layer{i}.weight": (rs.randn(40, 30) * (0.2 + 0.15 * i)).astype(np.float16) for i in range(N_LAYERS)}
    sd["layer0.bias"] = rs.randn(40).astype(np.float16)                          # not a candidate: 1-D
    sd["small.weight"] = rs.randn(10, 30).astype(np.float16)                     # not a candidate: 300 elements
    sd["norm.weight"] = (1 + 0.1 * rs.randn(40)).astype(np.float16)              # a `weight` the linear baseline quantizes, not a candidate
    return sd


class ToyEvaluator:
    """latents[p] = norm * (sum_i W_i x_p) + bias, from the working store's own values; records what differed from the pristine
    values at every call."""

    def __init__(self, pristine):
        self.x = np.random.RandomState(6).randn(N_PROMPTS, 30)
        self.pristine = {k: v.astype(np.float32) for k, v in pristine.items()}
        self.calls = []

    def __call__(self, working):
        vals = {k: working.read(k) for k in self.pristine}
        self.calls.append(sorted(k for k in vals if not np.array_equal(vals[k], self.pristine[k])))
        acc = sum(self.x @ vals[f"layer{i}.weight"].astype(np.float64).T for i in range(N_LAYERS))
        return acc * vals["norm.weight"][None, :] + vals["layer0.bias"][None, :]


@pytest.fixture(scope="module")
def toy_run(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("search"))
    sd = toy_state()
    store = hip_model.Weights(sd)
    ev = ToyEvaluator(sd)
    stats = {}
    results = search_mod.search(store, ev, out, "toy/model", num_recipes=3, min_size=1000, nbits_list=WIDTHS, stats=stats)
    after = {k: store.read(k) for k in sd}
    store.close()
    return dict(out=out, sd=sd, ev=ev, stats=stats, results=results, after=after)


def test_the_search_leaves_the_store_as_it_found_it(toy_run):
    for k, v in toy_run["sd"].items():
        assert np.array_equal(toy_run["after"][k], v.astype(np.float32)), k


def test_single_layer_pass_restores_and_cumulative_pass_follows_the_descending_order(toy_run):
    calls, results = toy_run["ev"].calls, toy_run["results"]
    cands = [f"layer{i}" for i in sorted(range(N_LAYERS), key=str)]                 # palettizable: name order
    assert cands == palettize.palettizable(hip_model.Weights(toy_run["sd"]), 1000)
    n = len(cands)
    assert calls[0] == []                                                        # the reference output
    assert len(calls) == toy_run["stats"]["evaluations"] == 1 + 2 * n * len(WIDTHS) + 1 + 3
    pos = 1
    for nbits in WIDTHS:
        single = results["single_layer"][str(nbits)]
        assert set(single) == set(cands) and all(len(v) == N_PROMPTS for v in single.values())
        # one tensor changed per evaluation, in candidate order: each was restored before the next one was palettized
        assert calls[pos:pos + n] == [[c + ".weight"] for c in cands]
        pos += n
        order = sorted(cands, key=lambda c: -sum(single[c]))
        meta = results["cumulative"][str(nbits)]["metadata"]
        assert meta["candidates"] == order and meta["sizes"] == [1200] * n and meta["cumulative"] is True and meta["nbits"] == nbits
        # nothing is restored inside the pass: the set of changed tensors grows by the next one of the order
        assert calls[pos:pos + n] == [sorted(c + ".weight" for c in order[:k + 1]) for k in range(n)]
        pos += n
        assert [k for k in results["cumulative"][str(nbits)] if k != "metadata"] == order
    # the linear 8-bit baseline changes every `weight` at once, candidate or not, and nothing else
    assert calls[pos] == sorted(k for k in toy_run["sd"] if k.endswith(".weight"))
    # ... and every recipe only candidates
    for c in calls[pos + 1:]:
        assert set(c) <= {x + ".weight" for x in cands}
    assert len(calls[pos + 1:]) == 3


def test_baselines_thresholds_and_recipes(toy_run):
    results = toy_run["results"]
    base = results["baselines"]
    assert base["original"] > 150 and base["linear_8bit"] < base["original"]     # a == b: finite, far above anything lossy
    assert results["model_version"] == "toy/model"
    assert os.path.basename(toy_run["out"] + "/" + search_mod.json_name("toy/model")) == "toy-model_palettization_recipe.json"
    assert set(results) == {"single_layer", "cumulative", "baselines", "recipes", "model_version"}
    assert set(base) == {"original", "linear_8bit"} | set(results["recipes"]) and results["recipes"]
    cands = set(palettize.palettizable(hip_model.Weights(toy_run["sd"]), 1000))
    sizes = {c: 1200 for c in cands}
    thresholds = np.linspace(base["original"] - 1, base["linear_8bit"] + 5, 3)
    expected = {}
    for t in thresholds:
        recipe, stats = search_mod.build_recipe(results["cumulative"], sizes, float(t), 16, WIDTHS)
        expected[f"recipe_{stats['nbits']:.2f}_bit_mixedpalette"] = recipe
    assert results["recipes"] == expected
    # the highest threshold (original - 1) passes nothing: every tensor stays at 16 bits and the model is the pristine one
    assert results["recipes"]["recipe_16.00_bit_mixedpalette"] == {c: 16 for c in cands}
    assert base["recipe_16.00_bit_mixedpalette"] == search_mod.rounded(base["original"])


def test_the_written_file_round_trips_through_load_recipe(toy_run):
    path = os.path.join(toy_run["out"], search_mod.json_name("toy/model"))
    on_disk = json.load(open(path))
    assert on_disk == json.loads(json.dumps(toy_run["results"]))
    cands = set(palettize.palettizable(hip_model.Weights(toy_run["sd"]), 1000))
    for key in on_disk["recipes"]:
        recipe = palettize.load_recipe(path, key)
        assert set(recipe) == cands and set(recipe.values()) <= set(palettize.NBITS) | {16}
        store = hip_model.Weights(toy_run["sd"])
        palettize.apply(store, recipe=recipe)                                    # strict: every module is in the checkpoint
        store.close()
    with pytest.raises(KeyError):
        palettize.load_recipe(path, "recipe_0.00_bit_mixedpalette")


def test_a_partial_file_is_resumed_not_recomputed(toy_run, tmp_path):
    first = toy_run["results"]
    partial = {"single_layer": {"2": first["single_layer"]["2"]}, "cumulative": {}, "model_version": "toy/model"}
    with open(os.path.join(str(tmp_path), search_mod.json_name("toy/model")), "w") as f:
        json.dump(partial, f)
    store = hip_model.Weights(toy_run["sd"])
    ev = ToyEvaluator(toy_run["sd"])
    again = search_mod.search(store, ev, str(tmp_path), "toy/model", num_recipes=3, min_size=1000, nbits_list=WIDTHS)
    store.close()
    assert len(ev.calls) == len(toy_run["ev"].calls) - N_LAYERS                  # the twelve single-layer evaluations at 2 bits are not run
    assert ev.calls[1:] == toy_run["ev"].calls[1 + N_LAYERS:]                    # what follows the reference output is the cumulative pass
    assert again == first                                                        # ... and the result is the uninterrupted run's


def test_search_refuses_bad_widths_and_an_empty_candidate_list(tmp_path):
    store = hip_model.Weights(toy_state())
    ev = ToyEvaluator(toy_state())
    with pytest.raises(ValueError, match="nbits"):
        search_mod.search(store, ev, str(tmp_path), "toy", nbits_list=(3,))
    with pytest.raises(ValueError, match="default_nbits"):
        search_mod.search(store, ev, str(tmp_path), "toy", default_nbits=5)
    with pytest.raises(ValueError, match="candidate"):
        search_mod.search(store, ev, str(tmp_path), "toy", min_size=1e9)
    assert ev.calls == []
    store.close()


def test_default_nbits_palettizes_every_candidate_first_and_the_store_comes_back_pristine(tmp_path):
    sd = toy_state()
    store = hip_model.Weights(sd)
    ev = ToyEvaluator(sd)
    results = search_mod.search(store, ev, str(tmp_path), "toy", default_nbits=6, num_recipes=2, min_size=1000, nbits_list=(2,))
    cands = palettize.palettizable(store, 1000)
    every = sorted(c + ".weight" for c in cands)
    assert ev.calls[0] == [] and ev.calls[1] == every                             # pristine output, then the 6-bit model's: the tables' reference
    assert all(c == every for c in ev.calls[2:2 + 2 * len(cands)])               # both passes run on top of the default palette
    assert set(v for r in results["recipes"].values() for v in r.values()) <= {2, 6}
    for k, v in sd.items():
        assert np.array_equal(store.read(k), v.astype(np.float32)), k
    store.close()


# ---- the linear 8-bit baseline's quantizer ----
def test_fake_linear_quantize_properties():
    """The step is (max(v, 0) - min(v, 0)) / 255 over the tensor.  A value is rounded to a multiple of the step (an error of at most
    half a step) and shifted by the rounded zero point, which cancels; only at the two ends can the sum of the two roundings leave
    [-128, 127] and be clipped, and then both were exact halves: the error is exactly half a step.  The arithmetic is float32: the
    product v * 255 / range and the final multiply each round once, so the bound carries 4 ulp of the largest magnitude."""
    rs = np.random.RandomState(11)
    for shape in ((64, 48), (8, 6, 3, 3), (33,)):
        v = (rs.randn(*shape) * rs.uniform(0.1, 3.0)).astype(np.float32)
        v.flat[3] = 0.0
        v.flat[7] = -0.0
        q = search_mod.fake_linear_quantize(v)
        assert q.dtype == v.dtype and q.shape == v.shape
        assert q.flat[3] == 0.0 and q.flat[7] == 0.0                             # zero is reproduced exactly
        step = (max(v.max(), 0.0) - min(v.min(), 0.0)) / 255.0
        slack = 4 * np.finfo(np.float32).eps * np.abs(v).max()
        assert np.abs(q.astype(np.float64) - v.astype(np.float64)).max() <= 0.5 * step + slack
        for row in q.reshape(-1, q.shape[-1]):                                   # every slice along the last axis
            assert len(np.unique(row)) <= 256
        assert len(np.unique(q)) <= 256
    pos = np.linspace(1.0, 2.0, 500, dtype=np.float32).reshape(10, 50)           # a range that has to be widened to contain 0
    qp = search_mod.fake_linear_quantize(pos)
    assert np.abs(qp - pos).max() <= 0.5 * 2.0 / 255 + 4 * np.finfo(np.float32).eps * 2 and len(np.unique(qp)) <= 129
    zeros = np.zeros((4, 4), np.float32)
    assert np.array_equal(search_mod.fake_linear_quantize(zeros), zeros)
