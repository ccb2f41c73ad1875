"""GPU suite of HipModel.reload_weights (sd_unet_reload_weights): a live handle whose named tensors were swapped computes bit for bit
what a handle freshly built from the new store computes - eagerly and on replay of the graph it captured before the swap - with
no new device memory.  Every comparison is an array_equal; nothing here has a tolerance.

The five configurations are the smallest that still select each kind of upload site (the labels each one is there for are
asserted, so a changed plan cannot silently empty the test): the generic fall-backs (TINY), the small-M GEMM / GEGLU / folded q|k|v /
merged tail of a 640-channel level, the one-launch head, cross-attention chain and tail of the 320-channel 5-head level, SDXL's
add_embedding, and a ControlNet with its conditioning embedding and zero convs."""
import ctypes as C
import functools
import json
import os
import re

import numpy as np
import pytest

from oracle import unet_ref, vae_ref, weights
from python_hip_stable_diffusion import HipModel, HipVaeDecoder, _lib, hip_model
from test_palettize_gemm_gpu import CFG as CFG640
from test_palettize_gpu import TINY, tiny_inputs, tiny_stores

pytestmark = pytest.mark.gpu

CFG320 = unet_ref.make_config(sample_size=64, block_out_channels=(320, 640), down_block_types=(unet_ref.CA, unet_ref.CA),
                              up_block_types=(unet_ref.CAUP, unet_ref.CAUP), layers_per_block=1, attention_head_dim=(5, 10),
                              cross_attention_dim=1024)

# name -> (config, kind, batch, label patterns the configuration is there for)
CASES = {
    "tiny": (TINY, "unet", 2, [r"^layernorm C=", r"^gemm1x1 .*attn1\.to_q ", r"^conv3x3 "]),
    "640": (CFG640, "unet", 4, [r"^gemm1x1\+ln .*attn1\.to_qkv ", r"^geglu1x1\+ln ", r"^gemm1x1 3200->640 .*ff\.net\.2 \+ residual \+ proj_out \+ residual",
                               r"^gemm1x1 640->640 .*proj_in ", r"^time_emb_proj of all resnets"]),
    "320": (CFG320, "unet", 2, [r"^gemm1x1\+gn 320->320 .*proj_in \+ norm1 \+ to_qkv", r"^xattn attn1\.to_out \+ residual \+\+ln q-proj 320->320",
                               r"^gemm1x1 1280->320 .*ff\.net\.2 \+ residual \+ proj_out \+ residual", r"^geglu1x1\+ln 320->2560"]),
    "mini-xl": (unet_ref.CONFIGS["mini-xl"], "unet", 2, [r"^text_time add-embedding"]),
    "mini-control": (unet_ref.CONFIGS["mini-control"], "controlnet", 2, [r"controlnet_down_blocks\.0 ", r"controlnet_mid_block "]),
}
SEED_A, SEED_B = 71, 72


@functools.lru_cache(maxsize=None)
def state_dicts(case):
    cfg, kind, _, _ = CASES[case]
    shapes = unet_ref.controlnet_param_shapes(cfg) if kind == "controlnet" else unet_ref.unet_param_shapes(cfg)
    return tuple(weights.make_state_dict(shapes, seed=s, dtype=np.float16) for s in (SEED_A, SEED_B))


@functools.lru_cache(maxsize=None)
def inputs(case):
    cfg, kind, B, _ = CASES[case]
    hw = cfg["sample_size"]
    kw = dict(sample=weights.seeded_normal((B, 4, hw, hw), 1).astype(np.float16), timestep=np.full(B, 981, np.float16),
              encoder_hidden_states=weights.seeded_normal((B, cfg["cross_attention_dim"], 1, 77), 2).astype(np.float16))
    if cfg["addition_embed_type"] == "text_time":
        text_dim = cfg["projection_class_embeddings_input_dim"] - 6 * cfg["addition_time_embed_dim"]
        kw["time_ids"] = np.tile(np.array([128, 128, 0, 0, 128, 128], np.float16), (B, 1))
        kw["text_embeds"] = weights.seeded_normal((B, text_dim), 3).astype(np.float16)
    if kind == "controlnet":
        kw["controlnet_cond"] = weights.seeded_normal((B, 3, hw * 8, hw * 8), 4).astype(np.float16)
    return kw


def run(model, kw):
    out = model(**kw)
    y = np.concatenate([out[k].ravel() for k in sorted(out)])
    assert np.isfinite(y).all()
    return y


def build(case, store, use_graph=True):
    cfg, kind, B, _ = CASES[case]
    return HipModel(cfg, store, kind=kind, batch=B, use_graph=use_graph)


@pytest.mark.parametrize("case", list(CASES))
def test_reload_of_every_tensor_equals_a_fresh_handle(case):
    sd_a, sd_b = state_dicts(case)
    kw = inputs(case)
    A, B = hip_model.Weights(sd_a), hip_model.Weights(sd_b)
    names = list(sd_a)
    for use_graph in (False, True):
        H = build(case, A, use_graph)
        first = run(H, kw)
        assert np.array_equal(run(H, kw), first)                                # (graph: captured by the first call, replayed by this one)
        used, total = H.arena_used_bytes, H.device_bytes
        H.reload_weights(B, names)
        got = run(H, kw)
        F = build(case, B, use_graph)
        want = run(F, kw)
        assert not np.array_equal(got, first)
        ndiff = np.count_nonzero(got != want)
        assert ndiff == 0, f"{case} use_graph={use_graph}: {ndiff} of {got.size} outputs differ from a fresh handle: an upload site did not follow"
        assert H.arena_used_bytes == used == F.arena_used_bytes and H.device_bytes == total == F.device_bytes
        if use_graph:
            labels = [lab for lab, _, _ in H.profile(1)]
            for pat in CASES[case][3]:
                assert any(re.search(pat, lab) for lab in labels), (pat, labels)
        H.reload_weights(A, names)
        assert np.array_equal(run(H, kw), first)
        assert H.arena_used_bytes == used
        H.close()
        F.close()
    A.close()
    B.close()


# ---- one tensor at a time, one per kind of upload site, on the 640-channel configuration ----
T0 = "down_blocks.1.attentions.0"
SINGLE = [
    "down_blocks.1.resnets.0.conv1.weight", "down_blocks.1.resnets.0.conv_shortcut.weight", "down_blocks.0.resnets.0.time_emb_proj.weight",
    "time_embedding.linear_1.weight", T0 + ".transformer_blocks.0.attn1.to_k.weight", T0 + ".transformer_blocks.0.attn2.to_v.weight",
    T0 + ".transformer_blocks.0.attn2.to_q.weight", T0 + ".transformer_blocks.0.ff.net.0.proj.weight", T0 + ".transformer_blocks.0.ff.net.2.weight",
    T0 + ".proj_out.weight", T0 + ".proj_in.weight", T0 + ".transformer_blocks.0.norm1.weight", T0 + ".transformer_blocks.0.ff.net.0.proj.bias",
    "up_blocks.0.upsamplers.0.conv.weight", "down_blocks.0.downsamplers.0.conv.weight", "conv_in.weight", "conv_out.weight",
]


@pytest.fixture(scope="module")
def live640():
    """(the live handle built from A, a working store that starts as A, A's output)"""
    sd_a, _ = state_dicts("640")
    store = hip_model.Weights(sd_a)
    H = build("640", store)
    first = run(H, inputs("640"))
    yield H, store, first
    H.close()
    store.close()


@pytest.mark.parametrize("name", SINGLE)
def test_reload_of_one_tensor_equals_a_fresh_handle_with_that_tensor_swapped(live640, name):
    H, store, first = live640
    sd_a, sd_b = state_dicts("640")
    kw = inputs("640")
    assert name in sd_a, name
    store.set_values(name, sd_b[name])
    try:
        H.reload_weights(store, [name])
        got = run(H, kw)
        F = build("640", store)
        want = run(F, kw)
        F.close()
        assert not np.array_equal(got, first), f"{name} does not reach the output"
        ndiff = np.count_nonzero(got != want)
        assert ndiff == 0, f"{name}: {ndiff} of {got.size} outputs differ from a fresh handle"
    finally:
        store.set_values(name, sd_a[name])
        H.reload_weights(store, [name])
    assert np.array_equal(run(H, kw), first)


# ---- refusals: each leaves the handle computing exactly what it did ----
def test_refused_reloads_change_nothing_and_a_valid_one_right_after_works():
    pal, plain, n_pal, shapes = tiny_stores(6)
    kw = tiny_inputs()
    H = HipModel(TINY, pal, batch=2)
    first = run(H, kw)
    streamed = [m.group(1) + ".weight" for m in (re.search(r"^\S+\+pal\d+ .* K=\d+ (\S+) #", lab) for lab, _, _ in H.profile(1)) if m]
    assert len(streamed) == H.palette_info()[1] >= 1 and all(s in shapes for s in streamed)
    first = run(H, kw)
    with pytest.raises(NotImplementedError, match=re.escape(streamed[0])):      # held as a palette stream
        H.reload_weights(plain, [streamed[0]])
    assert np.array_equal(run(H, kw), first)
    with pytest.raises(NotImplementedError, match=re.escape(streamed[0])):      # ... and a valid name beside it is not written either
        H.reload_weights(plain, ["conv_in.weight", streamed[0]])
    assert np.array_equal(run(H, kw), first)
    with pytest.raises(KeyError):
        H.reload_weights(plain, ["conv_in.weight", "no.such.tensor"])
    assert np.array_equal(run(H, kw), first)
    sd_b = dict(weights.make_state_dict(unet_ref.unet_param_shapes(TINY), seed=SEED_B, dtype=np.float16))
    wrong = dict(sd_b)
    wrong["conv_out.weight"] = np.zeros((4, 16, 3, 3), np.float16)
    W = hip_model.Weights(wrong)
    with pytest.raises(ValueError, match="conv_out.weight"):
        H.reload_weights(W, ["conv_in.weight", "conv_out.weight"])
    assert np.array_equal(run(H, kw), first)
    W.close()
    # a valid reload right after: every tensor the handle holds as fp16 / fp32, from another seed
    B = hip_model.Weights({k: (pal.read(k).astype(np.float16) if k in streamed else v) for k, v in sd_b.items()})
    loose = [k for k in sd_b if k not in streamed]
    H.reload_weights(B, loose)
    got = run(H, kw)
    F = HipModel(TINY, B, batch=2)                                              # (plain store: the streamed convs run lut[indices] from fp16, the same bits)
    assert np.array_equal(got, run(F, kw)) and not np.array_equal(got, first)
    F.close()
    H.close()
    for s in (pal, plain, B):
        s.close()


def test_a_vae_handle_and_an_observing_handle_are_refused():
    vcfg = vae_ref.VAE_CONFIGS["mini"]
    vsd = weights.make_state_dict(vae_ref.vae_decoder_param_shapes(vcfg), seed=61, dtype=np.float16, gain=1.6)
    vae = HipVaeDecoder(vcfg, vsd, batch=1, latent_height=8, latent_width=8)
    z = weights.seeded_normal((1, vcfg["latent_channels"], 8, 8), 5).astype(np.float16)
    first = vae(z=z)["image"].copy()
    store = hip_model.Weights(vsd)
    names = (C.c_char_p * 1)(b"conv_in.weight")
    assert _lib.lib().sd_unet_reload_weights(vae._h, store._h, names, 1) == -4
    assert b"VAE" in _lib.lib().sd_last_error()
    assert np.array_equal(vae(z=z)["image"], first)
    vae.close()
    store.close()
    sd = weights.make_state_dict(unet_ref.unet_param_shapes(TINY), seed=SEED_A, dtype=np.float16)
    A = hip_model.Weights(sd)
    H = HipModel(TINY, A, batch=2, observe_activations=True)
    first = run(H, tiny_inputs())
    with pytest.raises(NotImplementedError, match="observing"):
        H.reload_weights(A, ["conv_in.weight"])
    assert np.array_equal(run(H, tiny_inputs()), first)
    H.close()
    A.close()


# ---- the recipe search end to end: what it reports is what applying its recipes delivers ----
def test_search_on_the_mini_pipeline_reports_what_fresh_palettized_pipelines_deliver(tmp_path):
    from python_hip_stable_diffusion import mixed_bit_compression_pre_analysis as search_mod
    from python_hip_stable_diffusion import palettize, schedulers
    from python_hip_stable_diffusion.pipeline import HipStableDiffusionPipeline
    from test_pipeline_gpu import StubTextEncoder, StubTokenizer
    cfg = unet_ref.CONFIGS["mini"]
    sd16 = weights.make_state_dict(unet_ref.unet_param_shapes(cfg), seed=21, dtype=np.float16)
    prompts = ["a lighthouse on a rocky shore at dusk", "two red bicycles leaning against a brick wall"]
    widths = (2, 6)

    class ListTokenizer(StubTokenizer):
        """StubTokenizer over a list of prompts, one row each, as the checkpoint tokenizers take them"""

        def __call__(self, text, **kw):
            rows = [StubTokenizer.__call__(self, t, **kw).input_ids for t in ([text] if isinstance(text, str) else text)]
            return type("Enc", (), {"input_ids": np.concatenate(rows)})()

    def evaluator(unet_weights, **kw):
        unet = HipModel(cfg, unet_weights, batch=2 * len(prompts), **kw)
        pipe = HipStableDiffusionPipeline(StubTextEncoder(cfg["cross_attention_dim"]), unet, None, schedulers.DDIMScheduler(), ListTokenizer(),
                                          force_zeros_for_empty_prompt=False)
        return search_mod.PipelineEvaluator(pipe, prompts)

    nothing_changed = search_mod.WorkingStore(None)

    def fresh_rows(recipe):
        """The slow route: a pipeline built from the checkpoint with ``recipe`` applied by palettize.apply at load time."""
        ev = evaluator(sd16, palettization_recipe=recipe)
        out = ev(nothing_changed)
        ev.unet.close()
        return search_mod.psnr_rows(ref_out, out)

    store = hip_model.Weights(sd16)
    live = evaluator(store)
    ref_out = live(nothing_changed)
    candidates = [c for c in palettize.palettizable(store, 1000)
                  if c.startswith("mid_block.attentions.0.transformer_blocks.0.attn") or c == "mid_block.resnets.0.conv1"]
    assert len(candidates) == 9, candidates
    used = live.unet.arena_used_bytes
    stats = {}
    results = search_mod.search(store, live, str(tmp_path), "mini", num_recipes=3, min_size=1000, nbits_list=widths, candidates=candidates,
                                stats=stats)
    assert stats["evaluations"] == 1 + 2 * len(widths) * len(candidates) + 1 + 3
    assert live.unet.arena_used_bytes == used
    # state after the search: the handle computes the reference output, the store holds the checkpoint
    assert np.array_equal(live(nothing_changed), ref_out)
    assert all(np.array_equal(store.read(k), v.astype(np.float32)) for k, v in sd16.items())
    fresh = evaluator(sd16)
    assert np.array_equal(fresh(nothing_changed), ref_out)
    fresh.unet.close()
    text = lambda rows: [f"{x:.1f}" for x in rows]
    for nbits in widths:
        single, cumulative = results["single_layer"][str(nbits)], results["cumulative"][str(nbits)]
        for c in ("mid_block.resnets.0.conv1", candidates[0], candidates[-1]):
            assert text(single[c]) == text(fresh_rows({c: nbits})), (c, nbits)
            assert min(single[c]) < results["baselines"]["original"]            # (the palette really was in the handle)
        last = cumulative["metadata"]["candidates"][-1]
        assert text(cumulative[last]) == text(fresh_rows({c: nbits for c in candidates})), nbits
    path = os.path.join(str(tmp_path), search_mod.json_name("mini"))
    assert results["recipes"] and json.load(open(path)) == json.loads(json.dumps(results))
    for key in results["recipes"]:
        recipe = palettize.load_recipe(path, key)
        assert set(recipe) == set(candidates)
        rows = fresh_rows(recipe)
        assert f"{results['baselines'][key]:.1f}" == f"{search_mod.rounded(sum(rows) / len(rows)):.1f}", key
    assert len({tuple(sorted(r.items())) for r in results["recipes"].values()}) >= 2   # the thresholds tell recipes apart
    live.unet.close()
    store.close()


def test_cli_writes_a_file_the_generation_cli_accepts(tmp_path):
    """``main`` on a diffusers-layout checkpoint directory (real tokenizer and text encoder, the checkpoint's PNDM scheduler): the file
    it writes loads through ``load_recipe`` and builds a pipeline through ``get_hip_pipe(palettization_recipe=...)``."""
    from python_hip_stable_diffusion import mixed_bit_compression_pre_analysis as search_mod
    from python_hip_stable_diffusion import palettize, pipeline as P
    from test_text_encoder_gpu import write_checkpoint_dir
    root = str(tmp_path / "mini-sd")
    os.makedirs(root)
    write_checkpoint_dir(root)
    out = str(tmp_path / "recipes")
    args = search_mod.build_parser().parse_args(["-i", root, "-o", out, "--model-version", "mini/stable-diffusion", "--nbits", "6", "--num-recipes", "2",
                                                 "--min-size", "1.1e6"])
    assert args.default_nbits == 16 and args.latent_size is None and search_mod.build_parser().get_default("num_recipes") == 7
    results = search_mod.main(args, prompts=["a lighthouse on a rocky shore", "two red bicycles"])
    path = os.path.join(out, "mini-stable-diffusion_palettization_recipe.json")
    assert json.load(open(path)) == json.loads(json.dumps(results)) and results["model_version"] == "mini/stable-diffusion"
    cands = results["cumulative"]["6"]["metadata"]["candidates"]
    assert 1 <= len(cands) <= 12 and set(results["single_layer"]) == {"6"}
    for key in results["recipes"]:
        recipe = palettize.load_recipe(path, key)
        assert set(recipe) == set(cands) and set(recipe.values()) <= {6, 16}
        pipe = P.get_hip_pipe(root, "mini/stable-diffusion", palettization_recipe=recipe, disable_safety=True)
        assert pipe.unet.palette_info()[0] == sum(1 for b in recipe.values() if b != 16)
        pipe.unet.close()
