"""Weight palettization of the UNet family at load time.

The reference compresses at conversion time: ``torch2coreml.py --quantize-nbits`` (:182-229, :1705) palettizes every weight
uniformly, ``mixed_bit_compression_apply.py`` applies a per-layer recipe found by ``mixed_bit_compression_pre_analysis.py``.  Here the
same thing happens to the weight store in front of ``sd_unet_create``: each chosen tensor becomes ``lut[indices]`` with one LUT of
``2 ** nbits`` fp16 entries (``fake_palettize`` with one group, pre_analysis.py:139-156).  The clustering is the library's exact 1-D
k-means (``sd_weights_palettize``); its parity with coremltools' ``_get_kmeans_lookup_table_and_weight`` is NOT pinned (coremltools is
not a dependency of this project): the optimum cannot have a larger squared error than any k-means++ run, but the LUTs differ.
The recipe SEARCH lives beside this module (``mixed_bit_compression_pre_analysis``): it makes the file ``load_recipe`` reads, on a
live UNet handle through ``Weights.set_values`` and ``HipModel.reload_weights``.
"""
import json

NBITS = (1, 2, 4, 6, 8)
PALETTIZE_MIN_SIZE = 1e5      # mixed_bit_compression_pre_analysis.py:31


def _shapes(weights):
    return weights.shapes() if hasattr(weights, "shapes") else {k: tuple(v.shape) for k, v in weights.items()}


def palettizable(weights, min_size=PALETTIZE_MIN_SIZE):
    """Module names (tensor name without ``.weight``) of the 2-D / 4-D conv and linear weights with more than ``min_size``
    elements: ``get_palettizable_modules`` (pre_analysis.py:194-202).  ``weights``: a ``Weights`` store or a {name: array} dict."""
    out = []
    for name, shape in sorted(_shapes(weights).items()):
        if not name.endswith(".weight") or len(shape) not in (2, 4):
            continue
        n = 1
        for d in shape:
            n *= int(d)
        if n > min_size:
            out.append(name[:-len(".weight")])
    return out


def load_recipe(pre_analysis_json, selected):
    """{module: nbits} of recipe ``selected`` from a pre-analysis file of the reference's format
    (mixed_bit_compression_apply.py:28-42): ``{"model_version": ..., "recipes": {key: {module: nbits}}}``, nbits in
    {1, 2, 4, 6, 8, 16}, 16 = leave the tensor alone.  ``pre_analysis_json``: a path or the parsed dict."""
    if isinstance(pre_analysis_json, dict):
        pre = pre_analysis_json
    else:
        with open(pre_analysis_json) as f:
            pre = json.load(f)
    recipes = pre.get("recipes", {})
    if selected not in recipes:
        raise KeyError(f"--selected-recipe ({selected}) not found in --pre-analysis-json-path. Available recipes: {list(recipes)}")
    recipe = {str(k): int(v) for k, v in recipes[selected].items()}
    bad = {k: v for k, v in recipe.items() if v not in NBITS + (16,)}
    if bad:
        raise ValueError(f"Some nbits values in the recipe are illegal. Allowed values: {list(NBITS) + [16]}; got {bad}")
    return recipe


def apply(weights, nbits=None, recipe=None, strict=True):
    """Palettize a ``Weights`` store in place; returns {module: squared error}.

    ``nbits``: every module of ``palettizable(weights)`` at that width.  (The reference's uniform mode, torch2coreml.py:182-229,
    hands the whole model to coremltools and so also palettizes the tensors below ``PALETTIZE_MIN_SIZE``; here the small tensors -
    biases, norms, the first and last convs - stay fp16, as in its mixed-bit mode.)
    ``recipe``: {module: nbits} as ``load_recipe`` returns it; 16 skips the module; a module the checkpoint does not have raises
    ``KeyError`` naming it, before anything is changed.  ``strict=False`` skips such modules instead: a recipe is made for ONE model
    (pre_analysis searches the UNet), and the ControlNets and the refiner of the same pipeline share only some of its module names."""
    if (nbits is None) == (recipe is None):
        raise ValueError("palettize.apply takes nbits or a recipe, one of them")
    if recipe is None:
        if nbits not in NBITS:
            raise ValueError(f"nbits must be one of {list(NBITS)}, got {nbits!r}")
        recipe = {m: nbits for m in palettizable(weights)}
    else:
        names = weights.shapes()
        for module, b in recipe.items():
            if b not in NBITS + (16,):
                raise ValueError(f"recipe: {module} asks for {b} bits; allowed: {list(NBITS) + [16]}")
            if module + ".weight" not in names and strict:
                raise KeyError(f"recipe module {module!r} is not in the checkpoint (no tensor {module + '.weight'!r})")
        recipe = {m: b for m, b in recipe.items() if m + ".weight" in names}
    return {m: weights.palettize(m + ".weight", b) for m, b in recipe.items() if b != 16}
