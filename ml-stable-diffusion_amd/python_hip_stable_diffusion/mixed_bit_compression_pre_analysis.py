"""Mixed-bit palettization recipe search on a live UNet handle.

Restates the reference's ``mixed_bit_compression_pre_analysis.py`` (``run_pipe`` :248-277, ``benchmark_signal_integrity`` :280-326,
``descending_psnr_order`` :329-333, ``simulate_quant_fn`` :336-349, ``build_recipe`` :352-373, ``main`` :436-539) and writes its
file: ``{"single_layer", "cumulative" (with metadata.candidates / sizes), "baselines", "recipes", "model_version"}``, accepted
unchanged by ``--pre-analysis-json-path`` / ``--selected-recipe`` (``palettize.load_recipe``).

The search is a loop of about 2 x len(widths) x len(candidates) evaluations: change ONE tensor of the UNet, run one scheduler step
on a fixed list of prompts, compare the latents with the unchanged model's by PSNR.  The reference assigns to ``module.weight.data``
between two pipeline calls; here the change is ``Weights.set_values`` on the working store followed by ``HipModel.reload_weights``
of that one name on the handle, which was built once - no rebuild, no re-capture, no upload of the other tensors.

One evaluation: the candidate is clustered in a scratch one-tensor store by the library's exact 1-D k-means (``Weights.palettize``,
the same ``lut[indices]`` ``palettize.apply`` gives; parity with coremltools' k-means is unpinned, see ``palettize``), the values go
into the working store, the evaluator reloads what changed and runs the step.  The evaluator is an argument of ``search``: a
callable from the ``WorkingStore`` to the latents, one row per prompt, so the loop also runs against a numpy model without a GPU.

What follows the reference to the letter: per-prompt PSNR through ``compute_psnr(ref, test)`` (peak from the second argument), every
value rounded as ``float(f"{x:.1f}")``; with ``default_nbits`` other than 16 all candidates start palettized at that width and the
layer tables are measured against THAT model's output, the baselines and recipes against the pristine one; each cumulative pass
starts from the default model again (the reference runs it on a deep copy); recipes come from the CUMULATIVE tables; thresholds are
``linspace(original - 1, linear_8bit + 5, num_recipes)``; a recipe key that repeats overwrites the earlier one.
What does not: the default prompts are this project's own; the PSNR-versus-size plot is not drawn; at the end the store and the
handle hold the pristine weights again, whatever ``default_nbits`` was.

``fake_linear_quantize`` restates the reference's (:65-135) at what it is called with - mode LINEAR, int8, ``axis=-1``; parity with
coremltools' quantizer is unpinned (coremltools is not a dependency of this project)."""
import argparse
import json
import logging
import os
import time

import numpy as np

from .palettize import NBITS, PALETTIZE_MIN_SIZE, palettizable

logger = logging.getLogger(__name__)

# Signal integrity is computed on these prompts (an argument everywhere; the reference's own list is not used)
DEFAULT_PROMPTS = (
    "a lighthouse on a rocky shore at dusk, waves breaking below",
    "two red bicycles leaning against a brick wall in the rain",
    "a bowl of ripe oranges on a wooden kitchen table by a window",
    "an old steam locomotive crossing a stone viaduct in the mountains",
    "a grey heron standing in shallow water among the reeds",
    "a crowded night market street with paper lanterns overhead",
    "a snow-covered cabin under a sky full of stars",
    "a potter shaping a clay vase on a spinning wheel",
)
SEED = 93
GUIDANCE_SCALE = 7.5


def compute_psnr(a, b):
    """torch2coreml.py:59-74: 20 log10((max|b| + 1e-5) / (rmse(a, b) + 1e-10)); the peak is the SECOND argument's.  Finite for a == b."""
    a = np.asarray(a, np.float64).reshape(-1)
    b = np.asarray(b, np.float64).reshape(-1)
    max_b = np.abs(b).max()
    sumdeltasq = np.sum((a - b) ** 2) / a.size
    return float(20.0 * np.log10((max_b + 1e-5) / (np.sqrt(sumdeltasq) + 1e-10)))


def rounded(x):
    return float(f"{x:.1f}")


def psnr_rows(ref_out, test_out):
    """One rounded PSNR per prompt (pre_analysis.py:320-323)."""
    return [rounded(compute_psnr(r, t)) for r, t in zip(ref_out, test_out)]


def fake_linear_quantize(val, axis=-1):
    """pre_analysis.py:65-135 at mode LINEAR / int8: affine quantization to [-128, 127] over a range widened to contain 0, and back.
    The reference reduces over ``[i for i in range(ndim) if i != axis]``; with the ``axis=-1`` it is called with no i equals -1, so the
    range is the whole tensor's - kept, like everything else, as written there.  Arithmetic in ``val``'s dtype.  An all-zero tensor
    (the reference divides by zero there) comes back unchanged."""
    val = np.asarray(val)
    axes = tuple(i for i in range(val.ndim) if i != axis)
    val_min = np.minimum(0.0, np.amin(val, axis=axes, keepdims=True)).astype(val.dtype)
    val_max = np.maximum(0.0, np.amax(val, axis=axes, keepdims=True)).astype(val.dtype)
    if not np.all(val_max > val_min):
        return val.copy()
    q_min, q_max = -128, 127
    zero_point = np.round((q_min * val_max - q_max * val_min) / (val_max - val_min))
    zero_point = np.clip(zero_point, q_min, q_max).astype(np.int8)
    scale = ((val_max - val_min) / (q_max - q_min)).astype(val.dtype)
    q = np.round(val * (q_max - q_min) / (val_max - val_min)) + zero_point
    q = np.clip(q, q_min, q_max).astype(np.int8)
    return (q.astype(val.dtype) - zero_point.astype(val.dtype)) * scale


class WorkingStore:
    """The ``Weights`` store the search changes, with the names changed since the evaluator last looked (what it has to reload)."""

    def __init__(self, weights):
        self.weights = weights
        self.dirty = set()

    def set_values(self, name, values):
        self.weights.set_values(name, values)
        self.dirty.add(name)

    def read(self, name):
        return self.weights.read(name)

    def take_dirty(self):
        names, self.dirty = sorted(self.dirty), set()
        return names


def palettized_values(values, nbits, seconds=None):
    """``lut[indices]`` of ``values`` at ``nbits`` bits: the library's exact k-means on a scratch one-tensor store."""
    from .hip_model import Weights
    t0 = time.perf_counter()
    scratch = Weights({"w": np.asarray(values, np.float32)})
    try:
        scratch.palettize("w", nbits)
        out = scratch.read("w")
    finally:
        scratch.close()
    if seconds is not None:
        seconds["clustering"] = seconds.get("clustering", 0.0) + time.perf_counter() - t0
    return out


def benchmark_signal_integrity(working, evaluate, candidates, nbits, cumulative, ref_out, seconds=None, counts=None):
    """pre_analysis.py:280-326: palettize one candidate after the other at ``nbits``, one evaluation each.  Single-layer pass: the
    candidate's values go back behind its evaluation (picked up by the next evaluation's reload, or the caller's).  Cumulative pass:
    they stay.  Returns the table {"metadata": ..., candidate: [PSNR per prompt]} and {name: values before} of what is still changed."""
    results = {"metadata": {"nbits": nbits, "out_ngroups": 1, "in_ngroups": 1, "cumulative": cumulative}}
    changed = {}
    for candidate in candidates:
        name = candidate + ".weight"
        before = working.read(name)
        working.set_values(name, palettized_values(before, nbits, seconds))
        test_out = evaluate(working)
        if counts is not None:
            counts["evaluations"] = counts.get("evaluations", 0) + 1
        if cumulative:
            changed[name] = before
        else:
            working.set_values(name, before)
        results[candidate] = psnr_rows(ref_out, test_out)
        logger.info("%d-bit: %s = %s", nbits, candidate, results[candidate])
    return results, changed


def descending_psnr_order(results):
    """Candidates by descending summed PSNR (pre_analysis.py:329-333; like the reference it drops the table's metadata entry)."""
    results.pop("metadata", None)
    return dict(sorted(results.items(), key=lambda item: -sum(item[1])))


def build_recipe(results, sizes, psnr_threshold, default_nbits, nbits_list=NBITS):
    """pre_analysis.py:352-373 over the cumulative tables ``results[str(nbits)]``: for every candidate the first width, ascending,
    whose average PSNR exceeds the threshold, else ``default_nbits``.  Returns (recipe, {"nbits": average bits, "size_mb"})."""
    stats = {"nbits": 0}
    recipe = {}
    for key in results[str(nbits_list[0])]:
        if key == "metadata":
            continue
        achieved = default_nbits
        for nbits in nbits_list:
            row = results[str(nbits)][key]
            if sum(row) / len(row) > psnr_threshold:
                achieved = nbits
                break
        recipe[key] = achieved
        stats["nbits"] += achieved * sizes[key]
    stats["size_mb"] = stats["nbits"] / (8 * 1e6)
    stats["nbits"] /= sum(sizes.values())
    return recipe, stats


def json_name(model_version):
    return f"{model_version.replace('/', '-')}_palettization_recipe.json"


def search(weights, evaluate, out_dir, model_version, default_nbits=16, num_recipes=7, min_size=PALETTIZE_MIN_SIZE, nbits_list=NBITS,
           candidates=None, stats=None):
    """``main`` of the reference (:436-539) on the ``Weights`` store ``weights`` and ``evaluate(WorkingStore) -> latents``.
    ``candidates``: a subset of ``palettizable(weights, min_size)`` (the default).  The file ``out_dir/json_name(model_version)`` is
    written after every phase; one found there is resumed: a ``single_layer`` / ``cumulative`` table it holds is not measured again.
    ``stats`` (a dict) receives ``evaluations``, ``seconds`` {"clustering", "total"} and ``per_phase``.  Returns the results dict."""
    nbits_list = tuple(nbits_list)
    if not nbits_list or any(b not in NBITS for b in nbits_list) or list(nbits_list) != sorted(set(nbits_list)):
        raise ValueError(f"nbits must be an ascending selection of {list(NBITS)}, got {list(nbits_list)}")
    if default_nbits not in NBITS + (16,):
        raise ValueError(f"default_nbits must be one of {list(NBITS) + [16]}, got {default_nbits!r}")
    t_start = time.perf_counter()
    stats = {} if stats is None else stats
    seconds = stats.setdefault("seconds", {})
    shapes = weights.shapes()
    eligible = palettizable(weights, min_size)
    candidates = eligible if candidates is None else [c for c in eligible if c in set(candidates)]
    if not candidates:
        raise ValueError("no candidate tensors: nothing to search")
    sizes_table = {c: int(np.prod(shapes[c + ".weight"])) for c in candidates}
    logger.info("%d candidate tensors with %.3f M total params", len(candidates), sum(sizes_table.values()) / 1e6)
    working = WorkingStore(weights)
    weight_names = sorted(n for n in shapes if n.endswith(".weight"))

    def run():
        stats["evaluations"] = stats.get("evaluations", 0) + 1
        return evaluate(working)

    def restore(saved):
        for name, values in saved.items():
            working.set_values(name, values)

    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, json_name(model_version))
    results = {"single_layer": {}, "cumulative": {}, "model_version": model_version}
    if os.path.isfile(path):
        with open(path) as f:
            results = json.load(f)
        logger.info("resuming from %s", path)

    def save():
        with open(path, "w") as f:
            json.dump(results, f, indent=2)

    pristine_out = run()                                                         # ref_pipe's output: the baselines' reference
    pristine = {}                                                                # values under a default palette, {} at 16 bits
    if default_nbits != 16:
        logger.info("Palettizing the candidates to default %d-bit", default_nbits)
        for c in candidates:
            pristine[c + ".weight"] = working.read(c + ".weight")
            working.set_values(c + ".weight", palettized_values(pristine[c + ".weight"], default_nbits, seconds))
        ref_out = run()                                                          # (:449: the layer tables' reference)
    else:
        ref_out = pristine_out

    for nbits in nbits_list:
        if str(nbits) not in results["single_layer"]:
            results["single_layer"][str(nbits)], _ = benchmark_signal_integrity(working, evaluate, candidates, nbits, False, ref_out, seconds, stats)
            save()
        sorted_candidates = descending_psnr_order(results["single_layer"][str(nbits)])
        if str(nbits) not in results["cumulative"]:
            order = [c for c in sorted_candidates if c in sizes_table]
            table, changed = benchmark_signal_integrity(working, evaluate, order, nbits, True, ref_out, seconds, stats)
            table["metadata"].update({"candidates": order, "sizes": [sizes_table[c] for c in order]})
            results["cumulative"][str(nbits)] = table
            restore(changed)                                                     # the next pass starts from the default model again
            save()

    # uniform baselines against the pristine model (:501-507); back to pristine first
    restore(pristine)
    original = sum(psnr_rows(pristine_out, pristine_out)) / len(pristine_out)
    saved = {}
    for name in weight_names:
        saved[name] = working.read(name)
        working.set_values(name, fake_linear_quantize(saved[name]))
    linear_out = run()
    restore(saved)
    del saved
    results["baselines"] = {"original": original, "linear_8bit": sum(psnr_rows(pristine_out, linear_out)) / len(pristine_out)}
    save()

    # mixed-bit recipes via decreasing PSNR thresholds (:510-539), each measured end to end on the pristine model
    results["recipes"] = {}
    thresholds = np.linspace(results["baselines"]["original"] - 1, results["baselines"]["linear_8bit"] + 5, num_recipes)
    for recipe_no, threshold in enumerate(thresholds):
        recipe, rstats = build_recipe(results["cumulative"], sizes_table, float(threshold), default_nbits, nbits_list)
        saved = {}
        for c, bits in recipe.items():
            if bits != 16:
                saved[c + ".weight"] = working.read(c + ".weight")
                working.set_values(c + ".weight", palettized_values(saved[c + ".weight"], bits, seconds))
        out = run()
        restore(saved)
        achieved = sum(psnr_rows(pristine_out, out)) / len(pristine_out)
        logger.info("Recipe #%d: %.2f-bits @ per-layer %s dB, end-to-end %s dB & %.2f MB", recipe_no, rstats["nbits"], threshold, achieved,
                    rstats["size_mb"])
        key = f"recipe_{rstats['nbits']:.2f}_bit_mixedpalette"
        results["baselines"][key] = rounded(achieved)
        results["recipes"][key] = recipe
        save()

    if working.dirty and hasattr(evaluate, "reload"):                            # leave the handle on the pristine weights too
        evaluate.reload(working)
    seconds["total"] = time.perf_counter() - t_start
    return results


class PipelineEvaluator:
    """``run_pipe`` (pre_analysis.py:248-277) on a ``HipStableDiffusionPipeline`` whose UNet handle was built from the working store at
    batch 2 x len(prompts): one scheduler step from fixed latents, negative prompts "", latents out.  Text embeddings, starting latents
    and the scheduler's tables are computed once, here; an evaluation is ``reload_weights`` of what changed plus one device-loop step.
    ``seconds`` accumulates {"reload", "step"}, ``log`` keeps them per evaluation."""

    def __init__(self, pipe, prompts=DEFAULT_PROMPTS, seed=SEED, guidance_scale=GUIDANCE_SCALE):
        self.pipe, self.unet = pipe, pipe.unet
        prompts = list(prompts)
        n = len(prompts)
        if self.unet.batch != 2 * n:
            raise ValueError(f"the UNet handle has a static batch of {self.unet.batch}; {n} prompts with negative prompts need {2 * n}")
        if guidance_scale <= 1.0:
            raise ValueError("the search runs with classifier-free guidance (negative prompts \"\"): guidance_scale > 1")
        emb, pooled = pipe._encode_prompt(prompts, None, True, [""] * n, None)
        self.kwargs = dict(encoder_hidden_states=emb.astype(np.float16))
        if pipe.xl:
            size = (pipe.height, pipe.width)
            refiner = self.unet.expected_inputs["time_ids"]["shape"][-1] == 5
            self.kwargs.update(pipe._xl_kwargs(self.unet, pooled, size, (0, 0), size, True, n, refiner))
        sch = pipe.scheduler
        sch.set_timesteps(1)
        self.latents = np.asarray(pipe.prepare_latents(n, self.unet.in_channels, pipe.height, pipe.width, None, seed, "numpy"), np.float32)
        self.ts, self.coef, self.hist = sch.device_tables()
        self.scale = sch.sample_scale() if hasattr(sch, "sample_scale") else None
        self.noise = sch.step_noise(self.latents.shape) if hasattr(sch, "step_noise") else None
        self.guidance_scale = guidance_scale
        self.seconds = {"reload": 0.0, "step": 0.0}
        self.log = []                                                            # per evaluation: (tensors reloaded, reload s, step s)

    def reload(self, working):
        names = working.take_dirty()
        if names:
            self.unet.reload_weights(working.weights, names)
        return len(names)

    def __call__(self, working):
        t0 = time.perf_counter()
        n_names = self.reload(working)
        t1 = time.perf_counter()
        lat, _ = self.unet.denoise_loop(self.latents, self.ts, self.coef, self.guidance_scale, history=self.hist, sample_scale=self.scale,
                                        step_noise=self.noise, **self.kwargs)
        t2 = time.perf_counter()
        self.seconds["reload"] += t1 - t0
        self.seconds["step"] += t2 - t1
        self.log.append((n_names, t1 - t0, t2 - t1))
        return lat


def build_parser():
    parser = argparse.ArgumentParser(prog="python -m python_hip_stable_diffusion.mixed_bit_compression_pre_analysis")
    parser.add_argument("-i", required=True, help="Path to a diffusers checkpoint directory (unet/, vae/, text_encoder/, tokenizer/, "
                                                  "scheduler/), as for the generation CLI")
    parser.add_argument("-o", required=True, help="Output directory to save the palettization artifacts (recipe json)")
    parser.add_argument("--model-version", required=True, help="The pre-trained model checkpoint and configuration to restore.")
    parser.add_argument("--default-nbits", choices=NBITS + (16,), default=16, type=int, help="Default number of bits to use for palettization")
    parser.add_argument("--num-recipes", default=7, type=int,
                        help="Maximum number of recipes to generate (with decreasing model size and signal integrity)")
    parser.add_argument("--latent-size", default=None, type=int, help="Latent height and width of the test generations (default: the checkpoint's sample_size)")
    parser.add_argument("--min-size", default=PALETTIZE_MIN_SIZE, type=float,
                        help="Minimum number of elements in a weight tensor to be considered for palettization")
    parser.add_argument("--nbits", nargs="+", default=list(NBITS), type=int, choices=NBITS, help="Restrict the search to these bit widths")
    parser.add_argument("--attention-implementation", default="SPLIT_EINSUM", help="Attention schedule of the UNet kernels")
    return parser


def main(args, prompts=DEFAULT_PROMPTS):
    from .hip_model import Weights
    from .pipeline import _find_weights, get_hip_pipe
    prompts = list(prompts)
    store = Weights(safetensors_path=_find_weights(os.path.join(args.i, "unet")))
    try:
        pipe = get_hip_pipe(args.i, args.model_version, force_zeros_for_empty_prompt=False, attention_implementation=args.attention_implementation,
                            num_images=len(prompts), guidance_scale=GUIDANCE_SCALE, latent_size=args.latent_size, disable_safety=True,
                            unet_weights=store)
        evaluator = PipelineEvaluator(pipe, prompts)
        stats = {}
        results = search(store, evaluator, args.o, args.model_version, default_nbits=args.default_nbits, num_recipes=args.num_recipes,
                         min_size=args.min_size, nbits_list=sorted(set(args.nbits)), stats=stats)
        stats["seconds"].update(evaluator.seconds)
        logger.info("search done: %d evaluations, seconds %s", stats["evaluations"], stats["seconds"])
        pipe.unet.close()
    finally:
        store.close()
    return results


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    main(build_parser().parse_args())
