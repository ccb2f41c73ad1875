"""W8A8 post-training quantization of the UNet at load time.

The reference (``python_coreml_stable_diffusion/activation_quantization.py``) records calibration inputs
(``--generate-calibration-data``), then quantizes the torch UNet with coremltools' ``LinearQuantizer`` under
``quantize_cumulative_config`` (:141-203): symmetric int8, per-output-channel weights, per-tensor activations
(``--quantize-pytorch``).  Here the same scheme runs inside the library: the weight store MARKS a conv weight with its int8
values, its per-channel scales and the range of the activations the conv reads (``sd_weights_quantize_w8a8``), and a handle runs
a marked conv from int8 on ``v_mfma_i32_32x32x32_i8`` wherever its plan is the weight stream (``wstream.hip``, plan tile 17) or the
3x3 / stride-1 halo conv (``conv3x3_halo_i8.hip``, plan tile 18), and a marked plain 1x1 projection (``proj_in``, ``attn1.to_out.0``,
``attn2.to_out.0`` of the 640- / 1280-channel levels) on ``v_mfma_i32_16x16x64_i8`` wherever its plan is the small-M GEMM
(``smgemm_i8.hip``, plan tile 19), and a marked GEGLU projection (``ff.net.0.proj`` of those levels) on the same instruction wherever
its plan is ``smgeglu.hip`` (``smgeglu_i8.hip``, plan tile 20): its ``norm3`` is then not folded into the weights - one LayerNorm launch
writes ``int8(norm3(x))``, the tensor the reference calibrates, and the GEGLU reads it, and the marked self-attention projections
``attn1.to_q`` / ``to_k`` / ``to_v`` of those levels as ONE fused launch (``smqkv_i8.hip``, plan tile 22) behind a LayerNorm launch that
writes ``int8(norm1(x))`` - when all three are named with the same range, which is what ``observe_activations="attn"`` reports; every
other marked conv stays fp16 - the reference's skipped layers: one or two of the three q|k|v tensors or three different ranges, the
8x8 mid block's and the 320-channel level's q|k|v, ``attn2.to_q`` (inside the fused cross-attention launch), the prompt-side
``attn2.to_k`` / ``to_v``, ``conv_shortcut`` s and stride-2 convs.  The tail of a transformer block of those levels: a marked ``ff.net.2``
is not merged with ``proj_out`` - it runs from int8 on the GEGLU product (``smgemm_q8.hip``, plan tile 24), which the int8 GEGLU writes as
int8 itself (no fp16 product exists; behind an fp16 GEGLU one quantizer launch writes it), and a marked ``proj_out`` then runs as plan
tile 19; with ``ff.net.2`` unmarked the merged fp16 launch stays and a marked ``proj_out`` is skipped.  Parity with coremltools' quantizer is NOT pinned
(coremltools is not a dependency of this project): the scales are plain absmax / 127, not the result of its calibration.

The reference's second module class, the ``Einsum`` of every attention (``get_quantizable_modules``, :205-215; the ``'einsum'`` section
of the layer-wise results, :368-372): a recipe names the module, ``<block>.attn1.einsum``, with THREE ranges ``[r_q, r_k, r_v]`` - max |.|
of the module's inputs - and a handle runs a marked self-attention as a quantizer launch and the int8 attention kernel
(``attention_i8.hip``: int8 Q.K^T and P.V MFMAs, the probabilities quantized relative to the true row max; ``sd_weights_quantize_einsum``)
wherever it runs the fp16 head-dim-64 kernel today.  ``attn2.einsum`` (inside the fused cross-attention launches), head dims other
than 64 and shapes off the rule stay fp16, logged once per layer.  The scheme is the project's own; parity with coremltools' quantizer
is unpinned here too.

Calibration happens on the device: ``HipModel(..., observe_activations=True)`` puts an absmax observer in front of every conv
the int8 weight stream could take, ``observe_activations="all"`` in front of every conv either int8 conv kernel could take, ``observe_activations="gemm"`` also in front of
the projections plan tile 19 could take, ``observe_activations="geglu"`` also over the output of ``norm3`` in front of every GEGLU
projection plan tile 20 could take (a LayerNorm and an absmax launch beside the folded fp16 GEGLU, whose output does not change),
``observe_activations="attn"`` also over the output of ``norm1`` in front of every fused q|k|v launch plan tile 22 could take (the same
two launches; the one range is reported under ``attn1.to_q``, ``to_k`` and ``to_v``), ``observe_activations="tail"`` also over the GEGLU
product in front of every ``ff.net.2`` plan tile 24 could take and over a scratch ``ff.net.2`` output in front of its ``proj_out`` -
``observe_activations="einsum"`` also one launch behind every q|k|v producer whose self-attention the int8 attention kernel could take
(three slots ``<module>.q`` / ``.k`` / ``.v``) -
every layer that could run from int8; after any number of forwards ``.activation_ranges()`` is the recipe's raw material.

A recipe is JSON ``{layer: act_absmax}``, ``layer`` the conv's module name (its weight tensor without ``.weight``); a key ending in
``.einsum`` names an attention's Einsum module and carries a list ``[r_q, r_k, r_v]``.

Scope: the UNet - its convs and its self-attention einsums.  ``attn2.einsum``, the refiner, the ControlNets and the layer-wise PSNR
sensitivity search (:363-395, which can now fill both sections of its result file) are out of scope: recipes come from ranges, every
observed layer unless ``skip`` names it.
"""
import json
import logging
import math

logger = logging.getLogger(__name__)

_SUFFIX = ".weight"

# ``--calibrate-scope`` -> ``observe_activations``: each scope observes the previous one's layers and its own
CALIBRATION_SCOPES = {"stream": True, "all": "all", "gemm": "gemm", "geglu": "geglu"}
# the scopes added since, in a mapping of their own: "attn" observes what "geglu" does plus the self-attention q|k|v launches
ATTENTION_SCOPES = {"attn": "attn"}


# ... and "tail" observes what "attn" does plus the transformer tails: the GEGLU product ff.net.2 reads and the input of proj_out
TAIL_SCOPES = {"tail": "tail"}


# ... and "einsum" observes what "tail" does plus the inputs q, k, v of every self-attention the int8 attention kernel could take
EINSUM_SCOPES = {"einsum": "einsum"}

_EINSUM = ".einsum"
_EINSUM_SLOTS = (".q", ".k", ".v")


def is_einsum(layer):
    """a recipe key that names an attention's Einsum module (three ranges), not a conv (one)"""
    return layer.endswith(_EINSUM)


def calibration_scopes():
    """the ``--calibrate-scope`` -> ``observe_activations`` up to "attn", in the order each adds to the one before"""
    return {**CALIBRATION_SCOPES, **ATTENTION_SCOPES}


def all_calibration_scopes():
    """the ``--calibrate-scope`` -> ``observe_activations`` up to "tail", in the order each adds to the one before"""
    return {**calibration_scopes(), **TAIL_SCOPES}


def every_calibration_scope():
    """``all_calibration_scopes()`` and the scope added since, "einsum": what the CLI offers.  (The two functions above keep the values
    their callers pinned, as ``calibration_scopes()`` kept its own when "tail" arrived.)"""
    return {**all_calibration_scopes(), **EINSUM_SCOPES}


def layer_of(tensor_name):
    """``down_blocks.1.resnets.0.conv1.weight`` -> ``down_blocks.1.resnets.0.conv1``"""
    return tensor_name[:-len(_SUFFIX)] if tensor_name.endswith(_SUFFIX) else tensor_name


def recipe_from_ranges(ranges, skip=()):
    """{layer: act_absmax} from ``HipModel.activation_ranges()``.  ``skip``: layers to leave fp16 (what the reference's sensitivity
    search would drop).  A layer whose observed range is 0 (never run, or all-zero input) has no scale and raises ``ValueError``."""
    skip = {layer_of(s) for s in skip}
    recipe = {}
    slots = {}   # einsum module -> {".q": r_q, ".k": r_k, ".v": r_v}
    for layer, absmax in ranges.items():
        layer = layer_of(layer)
        if layer[-2:] in _EINSUM_SLOTS and is_einsum(layer[:-2]):   # the three slots of one observed Einsum fold into one entry
            slots.setdefault(layer[:-2], {})[layer[-2:]] = absmax
            continue
        if layer in skip:
            continue
        recipe[layer] = _checked(layer, absmax)
    for module, got in slots.items():
        if module in skip:
            continue
        if set(got) != set(_EINSUM_SLOTS):
            raise ValueError(f"activation ranges of {module!r}: slots {sorted(got)} observed, an Einsum needs .q, .k and .v")
        recipe[module] = _checked(module, [got[s] for s in _EINSUM_SLOTS])
    return recipe


def _checked(layer, absmax):
    layer = layer_of(str(layer))
    if is_einsum(layer):
        if isinstance(absmax, (str, bytes)) or not hasattr(absmax, "__len__"):
            raise ValueError(f"{layer!r} names an Einsum: its recipe value is a list [r_q, r_k, r_v], got {absmax!r}")
        if len(absmax) != 3:
            raise ValueError(f"{layer!r} names an Einsum: its recipe value is a list [r_q, r_k, r_v], got {len(absmax)} values")
        return [_checked_range(layer, r) for r in absmax]
    if hasattr(absmax, "__len__") and not isinstance(absmax, (str, bytes)):
        raise ValueError(f"{layer!r} names a conv: its recipe value is one act_absmax, got the list {list(absmax)!r} (only a key "
                         "ending in '.einsum' carries three ranges)")
    return _checked_range(layer, absmax)


def _checked_range(layer, absmax):
    absmax = float(absmax)
    if not (math.isfinite(absmax) and absmax > 0.0):
        raise ValueError(f"activation range of {layer!r} is {absmax!r}: a W8A8 layer needs a positive finite act_absmax")
    return absmax


def save_recipe(recipe, path):
    with open(path, "w") as f:
        json.dump({layer_of(k): _checked(k, v) for k, v in recipe.items()}, f, indent=1, sort_keys=True)


def load_recipe(path_or_dict):
    """A recipe file (or an already parsed dict) -> {layer: act_absmax}, values checked."""
    if isinstance(path_or_dict, dict):
        raw = path_or_dict
    else:
        with open(path_or_dict) as f:
            raw = json.load(f)
    if not isinstance(raw, dict):
        raise ValueError("an activation-quantization recipe is a JSON object {layer: act_absmax}")
    return {layer_of(str(k)): _checked(k, v) for k, v in raw.items()}


def apply(weights, recipe):
    """Mark the layers of ``recipe`` in a ``Weights`` store; returns {layer: squared weight error} of its convs (an Einsum has no
    weights: it is marked and returns nothing).  ``KeyError``: a layer the checkpoint does not have (nothing is marked then);
    ``ValueError``: a layer whose tensor carries a palette, or is no conv weight."""
    recipe = load_recipe(recipe)
    names = weights.shapes()
    for layer in recipe:
        if is_einsum(layer):
            if layer[:-len(_EINSUM)] + ".to_q" + _SUFFIX not in names:
                raise KeyError(f"activation-quantization recipe: einsum {layer!r} is not in the checkpoint (no tensor "
                               f"{layer[:-len(_EINSUM)] + '.to_q' + _SUFFIX!r})")
            continue
        if layer + _SUFFIX not in names:
            raise KeyError(f"activation-quantization recipe: layer {layer!r} is not in the checkpoint (no tensor {layer + _SUFFIX!r})")
        if weights.palette_bits(layer + _SUFFIX):
            raise ValueError(f"{layer!r} is palettized (quantize_nbits / palettization recipe) AND named by the activation-quantization "
                             "recipe: a tensor is one or the other")
    for layer, ranges in recipe.items():
        if is_einsum(layer):
            weights.quantize_einsum(layer, *ranges)
    return {layer: weights.quantize_w8a8(layer + _SUFFIX, absmax) for layer, absmax in recipe.items() if not is_einsum(layer)}
