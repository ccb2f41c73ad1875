"""``HipModel`` - the MI355X drop-in for the reference's model-runner seam.

Duck-types ``CoreMLModel`` (python_coreml_stable_diffusion/coreml_model.py:36-120): same
``expected_inputs`` attribute ({name: {"shape", "dtype"}}, coreml_model.py:58-64), same call
signature ``model(**np.ndarray) -> dict[str, np.ndarray]`` (:118-120), same input validation
and exception classes (``_verify_inputs`` :97-116), same tensor names/layouts/dtypes at the
boundary (torch2coreml.py:857-863, :905-908, :952, :988, :1412) with fp32 outputs like the
Core ML models declare (torch2coreml.py:135).  Behind it sits ``libsdmi355.so`` instead of
``MLModel.predict``; static shapes are fixed at construction exactly as conversion fixes them
for a .mlpackage (pipeline.py:112-114).  The attention implementation, a conversion-time flag
in the reference (torch2coreml.py:1678-1685 -> unet.py:39), is a per-handle run-time switch.
"""
import contextlib
import ctypes as C
import logging
import time

import numpy as np

from . import _lib

logger = logging.getLogger(__name__)

CROSS_ATTN_DOWN, DOWN = "CrossAttnDownBlock2D", "DownBlock2D"
CROSS_ATTN_UP, UP = "CrossAttnUpBlock2D", "UpBlock2D"

# Public HF config.json values (not in the reference: it reads them via **pipe.unet.config,
# torch2coreml.py:915).  Validated by parameter count in SURVEY.md Appendix B.
UNET_CONFIGS = {
    "stabilityai/stable-diffusion-2-1-base": dict(
        block_out_channels=(320, 640, 1280, 1280), attention_head_dim=(5, 10, 20, 20), cross_attention_dim=1024),
    "runwayml/stable-diffusion-v1-5": dict(
        block_out_channels=(320, 640, 1280, 1280), attention_head_dim=8, cross_attention_dim=768),
    "stabilityai/stable-diffusion-xl-base-1.0": dict(
        sample_size=128, block_out_channels=(320, 640, 1280), down_block_types=(DOWN, CROSS_ATTN_DOWN, CROSS_ATTN_DOWN),
        up_block_types=(CROSS_ATTN_UP, CROSS_ATTN_UP, UP), attention_head_dim=(5, 10, 20), cross_attention_dim=2048,
        transformer_layers_per_block=(1, 2, 10), addition_embed_type="text_time", addition_time_embed_dim=256,
        projection_class_embeddings_input_dim=2816),
    "stabilityai/stable-diffusion-xl-refiner-1.0": dict(
        sample_size=128, block_out_channels=(384, 768, 1536, 1536),
        down_block_types=(DOWN, CROSS_ATTN_DOWN, CROSS_ATTN_DOWN, DOWN),
        up_block_types=(UP, CROSS_ATTN_UP, CROSS_ATTN_UP, UP), attention_head_dim=(6, 12, 24, 24),
        cross_attention_dim=1280, transformer_layers_per_block=4, addition_embed_type="text_time",
        addition_time_embed_dim=256, projection_class_embeddings_input_dim=2560),
}


def normalize_unet_config(config):
    """Fill UNet2DConditionModel.__init__ defaults (unet.py:801-833) and reject what the
    reference rejects (unet.py:835-880)."""
    if isinstance(config, str):
        if config not in UNET_CONFIGS:
            raise ValueError(f"unknown model version {config!r}; known: {sorted(UNET_CONFIGS)}")
        config = UNET_CONFIGS[config]
    cfg = dict(
        in_channels=4, out_channels=4, sample_size=64, block_out_channels=(320, 640, 1280, 1280),
        down_block_types=(CROSS_ATTN_DOWN,) * 3 + (DOWN,), up_block_types=(UP,) + (CROSS_ATTN_UP,) * 3,
        layers_per_block=2, attention_head_dim=8, cross_attention_dim=768, transformer_layers_per_block=1,
        norm_num_groups=32, norm_eps=1e-5, flip_sin_to_cos=True, freq_shift=0, addition_embed_type=None,
        addition_time_embed_dim=None, projection_class_embeddings_input_dim=None, support_controlnet=False,
        only_cross_attention=False, mid_block_type="UNetMidBlock2DCrossAttn", center_input_sample=False)
    unknown_ok = {"use_linear_projection", "act_fn", "downsample_padding", "mid_block_scale_factor",
                  "time_cond_proj_dim", "upcast_attention", "resnet_time_scale_shift", "_class_name",
                  "_diffusers_version", "num_class_embeds", "dual_cross_attention", "class_embed_type",
                  "conditioning_embedding_out_channels", "num_time_ids"}
    for k, v in dict(config).items():
        if k not in cfg and k not in unknown_ok:
            logger.warning("ignoring unknown UNet config key %r", k)
        cfg[k] = v
    if cfg.get("dual_cross_attention") or cfg.get("num_class_embeds") or cfg["only_cross_attention"]:
        raise NotImplementedError("dual_cross_attention / class embeddings / only_cross_attention (unet.py:835-840)")
    if cfg["addition_embed_type"] not in (None, "text_time"):
        raise NotImplementedError(f"addition_embed_type {cfg['addition_embed_type']!r} (unet.py:868-880)")
    if cfg["mid_block_type"] != "UNetMidBlock2DCrossAttn" or cfg["center_input_sample"]:
        raise NotImplementedError("mid_block_type / center_input_sample outside the path (unet.py:919, :987)")
    n = len(cfg["block_out_channels"])
    if n > _lib.SD_MAX_LEVELS:
        raise NotImplementedError(f"more than {_lib.SD_MAX_LEVELS} resolution levels")
    for key in ("attention_head_dim", "transformer_layers_per_block"):
        v = cfg[key]
        cfg[key] = tuple([v] * n) if isinstance(v, int) else tuple(v)
    for t in cfg["down_block_types"]:
        if t not in (CROSS_ATTN_DOWN, DOWN):
            raise NotImplementedError(f"down block type {t}")
    for t in cfg["up_block_types"]:
        if t not in (CROSS_ATTN_UP, UP):
            raise NotImplementedError(f"up block type {t}")
    return cfg


def _fill(arr, values):
    for i, v in enumerate(values):
        arr[i] = int(v)


class Weights(_lib.Handle):
    """Owns an ``sd_weights`` store (checkpoint tensors keyed by diffusers names)."""
    _destroy = "sd_weights_destroy"

    def __init__(self, tensors=None, safetensors_path=None, prefix=None):
        self._h = C.c_void_p()
        self._shapes = None
        _lib.check(_lib.lib().sd_weights_create(C.byref(self._h)))
        if safetensors_path is not None:
            _lib.check(_lib.lib().sd_weights_load_safetensors(
                self._h, str(safetensors_path).encode(), None if prefix is None else prefix.encode()))
        for name, t in (tensors or {}).items():
            self.add(name, t)

    def add(self, name, t):
        t = np.asarray(t)
        if t.dtype == np.float16:
            dt = 0
        else:
            t = t.astype(np.float32, copy=False)
            dt = 1
        t = np.ascontiguousarray(t)
        shape = (C.c_int64 * max(1, t.ndim))(*t.shape)
        _lib.check(_lib.lib().sd_weights_add(self._h, name.encode(), _lib.ptr(t), dt, shape, t.ndim))
        self._shapes = None

    def __len__(self):
        return _lib.lib().sd_weights_count(self._h)

    def shapes(self):
        """{name: shape} of every tensor of the store (listed once, kept until a tensor is added)."""
        if self._shapes is not None:
            return self._shapes
        out = {}
        name = C.create_string_buffer(512)
        shape = (C.c_int64 * 8)()
        ndim = C.c_int(0)
        for i in range(len(self)):
            _lib.check(_lib.lib().sd_weights_tensor_info(self._h, i, name, len(name), shape, C.byref(ndim)))
            out[name.value.decode()] = tuple(int(shape[j]) for j in range(ndim.value))
        self._shapes = out
        return out

    # ---- palettes (sd_mi355x.h "Palettized weights") ----
    def palettize(self, name, nbits):
        """Cluster tensor ``name`` into a LUT of 2 ** nbits fp16 entries (exact 1-D k-means) and replace it by lut[indices]; returns
        the squared error against the fp16-rounded tensor.  ValueError: nbits not in {1, 2, 4, 6, 8}; KeyError: unknown name."""
        err = C.c_double(0)
        status = _lib.lib().sd_weights_palettize(self._h, name.encode(), int(nbits), C.byref(err))
        if status == -2:
            raise KeyError(name)
        _lib.check(status)
        return err.value

    def add_palettized(self, name, lut, indices, nbits):
        """Store a palette computed elsewhere: lut (2 ** nbits,) float16, indices uint8 of the tensor's shape; the tensor is
        lut[indices]."""
        lut = np.ascontiguousarray(lut, dtype=np.float16)
        indices = np.ascontiguousarray(indices, dtype=np.uint8)
        if nbits in (1, 2, 4, 6, 8) and lut.shape != (1 << nbits,):
            raise ValueError(f"add_palettized: the LUT of a {nbits}-bit palette has {1 << nbits} entries, got {lut.shape}")
        shape = (C.c_int64 * max(1, indices.ndim))(*indices.shape)
        _lib.check(_lib.lib().sd_weights_add_palettized(self._h, name.encode(), _lib.ptr(lut), int(nbits), _lib.ptr(indices), shape,
                                                        indices.ndim))
        self._shapes = None

    def palette_bits(self, name):
        """Index width of the tensor's palette, 0 when it has none."""
        return _lib.lib().sd_weights_palette_bits(self._h, name.encode())

    def read(self, name):
        """The stored tensor as float32 (for a palettized tensor: lut[indices])."""
        shape = self.shapes()[name]
        values = np.empty(shape, np.float32)
        _lib.check(_lib.lib().sd_weights_read_palette(self._h, name.encode(), None, None, _lib.fptr(values)))
        return values

    def read_palette(self, name):
        """(lut (2 ** nbits,) float16, indices uint8 of the tensor's shape) of a palettized tensor."""
        nbits = self.palette_bits(name)
        if not nbits:
            raise ValueError(f"tensor {name!r} has no palette")
        lut = np.empty(1 << nbits, np.float16)
        indices = np.empty(self.shapes()[name], np.uint8)
        _lib.check(_lib.lib().sd_weights_read_palette(self._h, name.encode(), _lib.ptr(lut), _lib.ptr(indices), None))
        return lut, indices

    def set_values(self, name, values):
        """Overwrite the values of the existing tensor ``name`` in place; a palette or W8A8 mark on it is dropped.  KeyError: unknown
        name; ValueError: ``values`` has another element count than the tensor."""
        values = np.ascontiguousarray(values, dtype=np.float32)
        status = _lib.lib().sd_weights_set_values(self._h, name.encode(), _lib.fptr(values), values.size)
        if status == -2:
            raise KeyError(name)
        _lib.check(status)

    # ---- W8A8 marks (sd_mi355x.h "W8A8 post-training quantization") ----
    def quantize_w8a8(self, name, act_absmax):
        """Mark conv weight ``name`` for W8A8 with the range of the activations its conv reads; returns the squared weight error.
        KeyError: unknown name; ValueError: not a conv weight, a palettized tensor, act_absmax not positive and finite."""
        err = C.c_double(0)
        status = _lib.lib().sd_weights_quantize_w8a8(self._h, name.encode(), float(act_absmax), C.byref(err))
        if status == -2:
            raise KeyError(name)
        _lib.check(status)
        return err.value

    def w8a8_info(self, name):
        """The activation scale s_a = act_absmax / 127 of a marked tensor, None when it has no mark."""
        s = C.c_float(0)
        return float(s.value) if _lib.lib().sd_weights_w8a8_info(self._h, name.encode(), C.byref(s)) else None

    def quantize_einsum(self, name, q_absmax, k_absmax, v_absmax):
        """Mark the attention Einsum module ``name`` (``<prefix>.einsum``, beside ``<prefix>.to_q.weight``) for W8A8 with the ranges of
        its inputs q, k and v (``sd_weights_quantize_einsum``).  KeyError: no such attention; ValueError: a range not positive and finite."""
        status = _lib.lib().sd_weights_quantize_einsum(self._h, name.encode(), float(q_absmax), float(k_absmax), float(v_absmax))
        if status == -2:
            raise KeyError(name)
        _lib.check(status)

    def einsum_info(self, name):
        """The (q, k, v) ranges of a marked Einsum module, None when it has no mark."""
        r = (C.c_float * 3)()
        return tuple(float(x) for x in r) if _lib.lib().sd_weights_einsum_info(self._h, name.encode(), r) else None

    def palette_halo(self, on=True):
        """Handles created from the store while this is on also run their palettized 3x3 / stride-1 halo convs - resnet ``conv1`` /
        ``conv2``, the two-source convs of the up blocks, upsamplers - from the palette (``sd_weights_palette_halo``, plan tile 25):
        the index stream and the LUT on the device, no fp16 copy, the same bits out.  Off by default."""
        if on not in (False, True, 0, 1):
            raise ValueError(f"palette_halo must be False or True, got {on!r}")
        _lib.check(_lib.lib().sd_weights_palette_halo(self._h, int(on)))
        self._palette_halo = bool(on)

    def observe_activations(self, on=True):
        """Handles created from the store while this is on carry the activation observers (calibration): ``True`` in front of the
        convs the int8 weight stream could take (plan tile 17), ``"all"`` in front of those of the int8 halo conv (plan tile 18) too,
        ``"gemm"`` also in front of the plain 1x1 projections the int8 small-M GEMM could take (plan tile 19), ``"geglu"`` also over
        the LayerNorm output in front of every GEGLU projection the int8 GEGLU kernel could take (plan tile 20), ``"attn"`` also over
        the output of ``norm1`` in front of every fused q|k|v launch the int8 q|k|v kernel could take (plan tile 22; one range,
        reported under ``attn1.to_q``, ``to_k`` and ``to_v``), ``"tail"`` also over the GEGLU product in front of every ``ff.net.2``
        the int8-activation GEMM could take (plan tile 24) and over a scratch ``ff.net.2`` output in front of its ``proj_out``,
        ``"einsum"`` also ONE launch behind every q|k|v producer whose self-attention the int8 attention kernel could take: max |q|,
        |k| and |v|, reported as ``<block>.attn1.einsum.q`` / ``.k`` / ``.v``."""
        _lib.check(_lib.lib().sd_weights_observe_activations(self._h, observe_level(on)))
        _lib.check(_lib.lib().sd_weights_observe_gemms(self._h, int(on in ("gemm", "geglu", "attn", "tail", "einsum"))))
        _lib.check(_lib.lib().sd_weights_observe_geglus(self._h, int(on in ("geglu", "attn", "tail", "einsum"))))
        _lib.check(_lib.lib().sd_weights_observe_qkv(self._h, int(on in ("attn", "tail", "einsum"))))
        _lib.check(_lib.lib().sd_weights_observe_tails(self._h, int(on in ("tail", "einsum"))))
        _lib.check(_lib.lib().sd_weights_observe_einsums(self._h, int(on == "einsum")))

    @classmethod
    @contextlib.contextmanager
    def lend(cls, weights):
        """``weights`` as a store for one ``create`` call: a ``Weights`` passes through and stays open; a .safetensors path
        or a {name: array} dict is loaded into a store that is closed behind the call."""
        if isinstance(weights, cls):
            yield weights
            return
        store = cls(safetensors_path=weights) if isinstance(weights, (str, bytes)) else cls(tensors=weights)
        try:
            yield store
        finally:
            store.close()


def observe_level(on):
    """observe_activations as the level of sd_weights_observe_activations: False 0, True 1, "all" 2; "gemm" is level 2 with the
    projections' flag (sd_weights_observe_gemms) beside it, "geglu" level 2 with that flag and the GEGLUs' (sd_weights_observe_geglus),
    "attn" level 2 with those two and the self-attention q|k|v launches' (sd_weights_observe_qkv), "tail" level 2 with those three and
    the transformer tails' (sd_weights_observe_tails), "einsum" level 2 with those four and the self-attention einsums'
    (sd_weights_observe_einsums)."""
    if isinstance(on, str):
        if on not in ("all", "gemm", "geglu", "attn", "tail", "einsum"):
            raise ValueError(f"observe_activations must be False, True, 'all', 'gemm', 'geglu', 'attn', 'tail' or 'einsum', got {on!r}")
        return 2
    return int(bool(on))


class HipModel(_lib.Model):
    """UNet / control-UNet / ControlNet on one MI355X behind the CoreMLModel interface."""
    _destroy = "sd_unet_destroy"

    def __init__(self, config, weights, kind="unet", batch=2, latent_height=None, latent_width=None,
                 attention_implementation="SPLIT_EINSUM", device=0, use_graph=True, context_len=77, quantize_nbits=None,
                 palettization_recipe=None, recipe_strict=True, activation_quantization=None, observe_activations=False,
                 palette_halo=False):
        if kind not in ("unet", "controlnet"):
            raise ValueError(f"kind must be 'unet' or 'controlnet', got {kind!r}")
        if (activation_quantization is not None or observe_activations) and kind != "unet":
            raise ValueError("activation quantization (W8A8) covers the UNet only: ControlNets are out of scope")
        if activation_quantization is not None and observe_activations:
            raise ValueError("observe_activations calibrates the fp16 model: give it or an activation_quantization recipe, not both")
        if attention_implementation not in _lib.ATTENTION_IMPLEMENTATIONS:
            raise ValueError(f"--attention-implementation must be one of {list(_lib.ATTENTION_IMPLEMENTATIONS)}")
        start = time.time()
        cfg = normalize_unet_config(config)
        self.config = cfg
        self.kind = kind
        h = latent_height or cfg["sample_size"]
        w = latent_width or cfg["sample_size"]
        n = len(cfg["block_out_channels"])
        xl = cfg["addition_embed_type"] == "text_time"
        c = _lib.UNetConfig()
        c.batch, c.in_channels, c.out_channels = batch, cfg["in_channels"], cfg["out_channels"]
        c.height, c.width, c.n_levels = h, w, n
        _fill(c.block_out_channels, cfg["block_out_channels"])
        _fill(c.down_cross_attn, [t == CROSS_ATTN_DOWN for t in cfg["down_block_types"]])
        _fill(c.up_cross_attn, [t == CROSS_ATTN_UP for t in cfg["up_block_types"]])
        c.layers_per_block = cfg["layers_per_block"]
        _fill(c.attention_head_dim, cfg["attention_head_dim"])
        _fill(c.transformer_layers_per_block, cfg["transformer_layers_per_block"])
        c.cross_attention_dim, c.context_len = cfg["cross_attention_dim"], context_len
        c.norm_num_groups, c.norm_eps = cfg["norm_num_groups"], cfg["norm_eps"]
        c.flip_sin_to_cos, c.freq_shift = int(cfg["flip_sin_to_cos"]), float(cfg["freq_shift"])
        self.num_time_ids = 0
        self.text_embed_dim = 0
        if xl:
            c.addition_time_embed_dim = cfg["addition_time_embed_dim"]
            c.projection_class_embeddings_input_dim = cfg["projection_class_embeddings_input_dim"]
            # base: 6 ids + 1280-d pooled text; refiner: 5 ids + 1280-d (StableDiffusionXLPipeline.swift:326-358)
            self.num_time_ids = int(cfg.get("num_time_ids") or
                                    (5 if cfg["projection_class_embeddings_input_dim"] == 2560 else 6))
            c.num_time_ids = self.num_time_ids
            self.text_embed_dim = (cfg["projection_class_embeddings_input_dim"] -
                                   self.num_time_ids * cfg["addition_time_embed_dim"])
        c.support_controlnet = int(bool(cfg["support_controlnet"]) and kind == "unet")
        c.is_controlnet = int(kind == "controlnet")
        c.attention_impl = _lib.ATTENTION_IMPLEMENTATIONS[attention_implementation]
        c.use_graph = int(use_graph)
        self._cfg_struct = c
        self._h = C.c_void_p()
        if quantize_nbits is not None and palettization_recipe is not None:
            raise ValueError("quantize_nbits and palettization_recipe are two ways to say the same thing: give one")
        if quantize_nbits is not None and quantize_nbits not in (1, 2, 4, 6, 8):
            raise ValueError(f"--quantize-nbits must be one of 1, 2, 4, 6, 8, got {quantize_nbits!r}")
        with Weights.lend(weights) as store:
            if quantize_nbits is not None or palettization_recipe is not None:
                # (torch2coreml.py:182-229 quantize_weights / mixed_bit_compression_apply.py: at conversion time there, at load time here;
                # a store the caller lent stays palettized, as a converted model does)
                from . import palettize
                palettize.apply(store, nbits=quantize_nbits, recipe=palettization_recipe, strict=recipe_strict)
            self.activation_quantization = None
            if activation_quantization is not None:
                # (activation_quantization.py:141-203 --quantize-pytorch: at load time here; raises on an unknown layer and on a
                # tensor the palettization above covers, before any device work)
                from . import activation_quantization as aq
                self.activation_quantization = aq.load_recipe(activation_quantization)
                aq.apply(store, self.activation_quantization)
            if observe_activations:
                store.observe_activations(observe_activations)
            halo_was = getattr(store, "_palette_halo", False)
            if palette_halo:   # the palettized 3x3 halo convs stay palettized on the device (plan tile 25)
                store.palette_halo(True)
            try:
                _lib.check(_lib.lib().sd_unet_create(C.byref(c), store._h, device, C.byref(self._h)))
            finally:
                if observe_activations:
                    store.observe_activations(False)   # a lent store goes back as it came
                if palette_halo and not halo_was:
                    store.palette_halo(False)
        if self.activation_quantization is not None:
            from . import activation_quantization as aq
            einsums = {layer for layer in self.activation_quantization if aq.is_einsum(layer)}
            applied = set(self.w8a8_layers())
            stayed = sorted(set(self.activation_quantization) - einsums - applied)
            logger.info("W8A8: %d of %d recipe layers run from int8 (plan tiles 17 / 18 / 19 / 20 / 22)", len(applied),
                        len(self.activation_quantization) - len(einsums))
            if einsums:
                on_i8 = set(self.einsum_layers())
                logger.info("W8A8: %d of %d recipe einsums run on the int8 attention kernel", len(on_i8), len(einsums))
                for layer in sorted(einsums - on_i8):
                    logger.info("W8A8: %s stays fp16 (an attn2.einsum, a head dim other than 64, a shape off the int8 kernel's rule or an "
                                "attention of the general kernels)", layer)
            if stayed:
                logger.info("W8A8: these layers stay fp16 (their plan is none of the weight stream, the halo conv, the plain small-M projection, the "
                            "GEGLU kernel and the fused self-attention q|k|v launch with its three tensors under one range): %s", ", ".join(stayed))
        self.batch, self.latent_height, self.latent_width = batch, h, w
        self.attention_implementation = attention_implementation
        self.num_residuals = _lib.lib().sd_unet_num_residuals(self._h)
        self._attached = []

        f16 = np.dtype(np.float16)
        ei = {
            "sample": {"shape": (batch, cfg["in_channels"], h, w), "dtype": f16},
            "timestep": {"shape": (batch,), "dtype": f16},
            "encoder_hidden_states": {"shape": (batch, cfg["cross_attention_dim"], 1, context_len), "dtype": f16},
        }
        if xl:
            ei["time_ids"] = {"shape": (batch, self.num_time_ids), "dtype": f16}
            ei["text_embeds"] = {"shape": (batch, self.text_embed_dim), "dtype": f16}
        self._res_shapes = self._residual_shapes(cfg, batch, h, w)
        if kind == "controlnet":
            ei["controlnet_cond"] = {"shape": (batch, 3, h * 8, w * 8), "dtype": f16}
        elif c.support_controlnet:
            for i, s in enumerate(self._res_shapes):
                ei[f"additional_residual_{i}"] = {"shape": s, "dtype": f16}
        self.expected_inputs = ei
        logger.info("HipModel(%s) ready in %.1f s, %.2f GB of HBM", kind, time.time() - start,
                    _lib.lib().sd_unet_device_bytes(self._h) / 1e9)

    @staticmethod
    def _residual_shapes(cfg, batch, h, w):
        boc = cfg["block_out_channels"]
        shapes = [(batch, boc[0], h, w)]
        for i in range(len(boc)):
            shapes += [(batch, boc[i], h, w)] * cfg["layers_per_block"]
            if i != len(boc) - 1:
                h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
                shapes.append((batch, boc[i], h, w))
        shapes.append((batch, boc[-1], h, w))
        return shapes

    def _io(self, kwargs, keep):
        io = _lib.UNetIO()

        def put(field, name):
            if name in kwargs:
                a = np.ascontiguousarray(kwargs[name])
                keep.append(a)
                setattr(io, field, a.ctypes.data)

        for f in ("sample", "timestep", "encoder_hidden_states", "time_ids", "text_embeds", "controlnet_cond"):
            put(f, f)
        if self.kind == "unet" and self._cfg_struct.support_controlnet and not self._attached:
            arrs = [np.ascontiguousarray(kwargs[f"additional_residual_{i}"]) for i in range(self.num_residuals)]
            keep.extend(arrs)
            ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
            keep.append(ptrs)
            io.additional_residuals = C.cast(ptrs, C.POINTER(C.c_void_p))
            io.num_additional_residuals = len(arrs)
        return io

    def __call__(self, **kwargs):
        self._verify_inputs(**kwargs)
        keep = []
        io = self._io(kwargs, keep)
        if self.kind == "unet":
            out = np.empty((self.batch, self.config["out_channels"], self.latent_height, self.latent_width),
                           np.float32)
            io.noise_pred = out.ctypes.data
            _lib.check(_lib.lib().sd_unet_forward(self._h, C.byref(io)))
            return {"noise_pred": out}
        outs = [np.empty(s, np.float32) for s in self._res_shapes]
        ptrs = (C.c_void_p * len(outs))(*[o.ctypes.data for o in outs])
        io.residual_outputs = C.cast(ptrs, C.POINTER(C.c_void_p))
        _lib.check(_lib.lib().sd_unet_forward(self._h, C.byref(io)))
        return {f"additional_residual_{i}": o for i, o in enumerate(outs)}

    # ---- beyond the reference surface -----------------------------------------------------
    def set_attention_implementation(self, name):
        if name not in _lib.ATTENTION_IMPLEMENTATIONS:
            raise ValueError(f"--attention-implementation must be one of {list(_lib.ATTENTION_IMPLEMENTATIONS)}")
        _lib.check(_lib.lib().sd_unet_set_attention(self._h, _lib.ATTENTION_IMPLEMENTATIONS[name]))
        self.attention_implementation = name

    def reload_weights(self, weights, names):
        """Swap the values of the tensors ``names`` for those the ``Weights`` store ``weights`` holds (``sd_unet_reload_weights``):
        the handle then computes bit for bit what one freshly built from ``weights`` computes, with no rebuild, no re-capture and no
        new device memory.  ``weights`` is a complete store that differs from the one the handle last took its weights from only in
        the values of ``names``.  KeyError: a name the store does not hold; ValueError: another shape than the handle was built with;
        NotImplementedError: a tensor the handle holds compressed on the device (palette stream, int8), a handle built from an
        observing store.  A refused call changes nothing."""
        names = [n.encode() for n in names]
        arr = (C.c_char_p * max(1, len(names)))(*names)
        status = _lib.lib().sd_unet_reload_weights(self._h, weights._h, arr, len(names))
        if status == -2:
            raise KeyError(_lib.lib().sd_last_error().decode("utf-8", "replace"))
        _lib.check(status)

    def time_forward(self, warmup=2, iters=10):
        """HIP-event milliseconds per forward on the handle's stream (inputs of the last call)."""
        ms = C.c_float(0)
        _lib.check(_lib.lib().sd_unet_time_forward(self._h, warmup, iters, C.byref(ms)))
        return ms.value

    def denoise_loop(self, latents, timesteps, coef, guidance_scale, history=0, sample_scale=None, history_state=None,
                     step_noise=None, progress=None, progress_steps=1, pred=None, **kwargs):
        """Device-resident pipeline.py:500-573.  latents (n_img, C, H, W) float32 -> final latents,
        per-step HIP-event milliseconds.  ``kwargs`` are the loop-invariant model inputs
        (encoder_hidden_states, SDXL time_ids / text_embeds), validated like ``__call__`` validates them
        (coreml_model.py:97-116).  ``history_state`` (history, n_img, C, H, W) float32 carries the
        scheduler's multistep history in and out (updated in place) when a loop continues on another
        handle (SDXL base -> refiner).  ``step_noise`` (len(timesteps), n_img, C, H, W) float32: added to the latents at
        the end of step i - the ancestral samplers' fresh noise, already scaled by sigma_up.
        ``progress(step, n_steps, latents, denoised)``: called between two steps of the device loop (``sd_unet_denoise_loop_progress``;
        StableDiffusionPipeline.swift:332-349) after every step with ``step % progress_steps == 0`` (pipeline.py:570), with copies of
        the latents after that step and - when ``pred`` (len(timesteps), 8), the scheduler's ``denoised_table()``, is given - of its
        de-noised estimate, else None.  A falsy return other than None stops the loop; an exception in the handler stops it too and is
        raised again here once the library call has returned.  ``ms`` then holds the steps that ran - as many as after a full run when
        the stop comes behind the LAST step, so a caller that must know that the handler said stop keeps its verdict itself (the
        pipeline does).  The handler may drive other
        handles (a VAE decoder for a preview), not this one (ValueError)."""
        if self.kind != "unet":
            raise ValueError("denoise_loop needs a UNet handle")
        loop_inputs = {k: v for k, v in self.expected_inputs.items()
                       if k not in ("sample", "timestep") and not k.startswith("additional_residual_")}
        _lib.verify_inputs(loop_inputs, **kwargs)
        if self._cfg_struct.support_controlnet and not self._attached:
            raise ValueError("this UNet consumes ControlNet residuals: attach_controlnets() first, or step through "
                             "__call__ with additional_residual_* inputs")
        lat = np.ascontiguousarray(latents, dtype=np.float32).copy()
        cfg_mul = 2 if guidance_scale > 1.0 else 1                                    # pipeline.py:443
        want = (self.batch // cfg_mul, self.config["in_channels"], self.latent_height, self.latent_width)
        if lat.shape != want or self.batch % cfg_mul:
            raise ValueError(f"Unexpected latents shape, got {lat.shape}, expected {want} (UNet batch {self.batch}, "
                             f"guidance_scale {guidance_scale})")
        ts = np.ascontiguousarray(timesteps, dtype=np.float32).reshape(-1)
        cf = np.ascontiguousarray(coef, dtype=np.float32)
        if cf.size != len(ts) * 8 or len(ts) < 1:
            raise ValueError(f"coef must hold len(timesteps) x 8 = {len(ts) * 8} entries, got {cf.size}")
        if not 0 <= int(history) <= 3:
            raise ValueError(f"history must be in 0..3, got {history}")
        sc = None
        if sample_scale is not None:
            sc = np.ascontiguousarray(sample_scale, dtype=np.float32).reshape(-1)
            if len(sc) != len(ts):
                raise ValueError("sample_scale must have one entry per timestep")
        hs = None
        if history_state is not None and history:
            if (not isinstance(history_state, np.ndarray) or history_state.dtype != np.float32
                    or history_state.shape != (int(history),) + lat.shape or not history_state.flags.c_contiguous):
                raise ValueError(f"history_state must be a C-contiguous float32 array of shape {(int(history),) + lat.shape}")
            hs = history_state
        keep = []
        io = self._io(kwargs, keep)
        if step_noise is not None:
            sn = np.ascontiguousarray(step_noise, dtype=np.float32)
            if sn.shape != (len(ts),) + lat.shape:
                raise ValueError(f"step_noise must have shape {(len(ts),) + lat.shape}, got {sn.shape}")
            keep.append(sn)
            io.step_noise = sn.ctypes.data
        pr = None
        if pred is not None:
            pr = np.ascontiguousarray(pred, dtype=np.float32)
            if pr.shape != (len(ts), 8):
                raise ValueError(f"pred must have shape {(len(ts), 8)}, got {pr.shape}")
        if isinstance(progress_steps, bool) or not isinstance(progress_steps, (int, np.integer)) or progress_steps < 1:
            raise ValueError(f"`progress_steps` has to be a positive integer but is {progress_steps}")
        ms = np.zeros(len(ts), np.float32)
        raised = []

        def trampoline(_user, step, n_steps, lat_p, den_p):
            try:
                snap = np.ctypeslib.as_array(lat_p, shape=lat.shape).copy()
                den = np.ctypeslib.as_array(den_p, shape=lat.shape).copy() if den_p else None
                go = progress(step, n_steps, snap, den)
                return 1 if (go is None or go) else 0
            except BaseException as e:   # an exception cannot unwind through the library: stop the loop, raise behind the call
                raised.append(e)
                return 0

        fn = _lib.PROGRESS_FN(trampoline) if progress is not None else None      # alive until the call has returned
        done = C.c_int(len(ts))
        _lib.check(_lib.lib().sd_unet_denoise_loop_progress(
            self._h, C.byref(io), _lib.fptr(lat), lat.shape[0], len(ts), _lib.fptr(ts), _lib.fptr(cf), _lib.fptr(sc), int(history),
            float(guidance_scale), _lib.fptr(hs), _lib.fptr(ms), _lib.fptr(pr), int(progress_steps),
            None if fn is None else C.cast(fn, C.c_void_p), None, C.byref(done)))
        if raised:
            raise raised[0]
        return lat, ms[:done.value]

    def profile(self, iters=5):
        """[(label, flop, ms)] for every launch-list entry of one forward, in launch order (sd_unet_profile)."""
        return _profile(self._h, iters)

    def attach_controlnets(self, controlnets):
        """Device-resident ControlNet hand-off (sd_unet_attach_controlnets): this UNet runs the given
        ControlNet ``HipModel`` handles before every forward / loop step and reads their residuals from
        HBM.  ``[]`` detaches (residuals then come through ``additional_residual_*`` again)."""
        controlnets = list(controlnets or [])
        for cn in controlnets:
            if not isinstance(cn, HipModel) or cn.kind != "controlnet":
                raise TypeError("attach_controlnets takes HipModel(kind='controlnet') handles")
        arr = (C.c_void_p * max(1, len(controlnets)))(*[cn._h for cn in controlnets])
        _lib.check(_lib.lib().sd_unet_attach_controlnets(self._h, C.cast(arr, C.POINTER(C.c_void_p)), len(controlnets)))
        self._attached = controlnets      # keeps the handles alive while attached
        ei = {k: v for k, v in self.expected_inputs.items() if not k.startswith("additional_residual_")}
        if self._cfg_struct.support_controlnet and not controlnets:
            for i, s_ in enumerate(self._res_shapes):
                ei[f"additional_residual_{i}"] = {"shape": s_, "dtype": np.dtype(np.float16)}
        self.expected_inputs = ei

    def set_controlnet_cond(self, cond):
        """ControlNet handle: upload the conditioning image (B, 3, 8H, 8W) fp16 and embed it once
        (controlnet.py:211-215) for the device-resident hand-off."""
        if self.kind != "controlnet":
            raise ValueError("set_controlnet_cond needs a ControlNet handle")
        want = self.expected_inputs["controlnet_cond"]
        if not isinstance(cond, np.ndarray):
            raise TypeError(f"Expected numpy.ndarray, got {cond} for input: controlnet_cond")
        if cond.dtype != want["dtype"] or cond.shape != want["shape"]:
            raise TypeError(f"Expected {want['dtype']} {want['shape']}, got {cond.dtype} {cond.shape} for input: controlnet_cond")
        c = np.ascontiguousarray(cond)
        _lib.check(_lib.lib().sd_controlnet_set_cond(self._h, _lib.ptr(c), 0))

    @property
    def device_bytes(self):
        return _lib.lib().sd_unet_device_bytes(self._h)

    @property
    def arena_used_bytes(self):
        """Bytes the handle's tensors occupy inside ``device_bytes`` (which counts whole 256-MiB chunks)."""
        return _lib.lib().sd_unet_arena_used_bytes(self._h)

    def palette_info(self):
        """(tensors that arrived with a palette, convs that read theirs on the device - plan tiles 14 / 15 / 16, and 25 in a handle built
        with ``palette_halo`` -, bytes of those convs' index streams and LUTs)."""
        n_pal, n_str, nbytes = C.c_int(0), C.c_int(0), C.c_size_t(0)
        _lib.check(_lib.lib().sd_unet_palette_info(self._h, C.byref(n_pal), C.byref(n_str), C.byref(nbytes)))
        return n_pal.value, n_str.value, nbytes.value

    def w8a8_info(self):
        """(tensors that arrived with a W8A8 mark, convs that run from int8 - plan tile 17 -, bytes of those convs' int8 streams and
        scale vectors).  marked - applied convs stayed fp16."""
        n_marked, n_applied, nbytes = C.c_int(0), C.c_int(0), C.c_size_t(0)
        _lib.check(_lib.lib().sd_unet_w8a8_info(self._h, C.byref(n_marked), C.byref(n_applied), C.byref(nbytes)))
        return n_marked.value, n_applied.value, nbytes.value

    def w8a8_layers(self):
        """Module names of the convs that run from int8, in build order."""
        n = _lib.lib().sd_unet_w8a8_layer(self._h, -1, None, 0)
        if n < 0:
            _lib.check(n)
        name = C.create_string_buffer(512)
        out = []
        for i in range(n):
            if _lib.lib().sd_unet_w8a8_layer(self._h, i, name, len(name)) < 0:
                _lib.check(-1)
            out.append(name.value.decode()[:-len(".weight")])
        return out

    def einsum_info(self):
        """(Einsum marks the weight store arrived with, attentions that run on the int8 attention kernel); ``w8a8_info`` counts convs."""
        n_marked, n_applied = C.c_int(0), C.c_int(0)
        _lib.check(_lib.lib().sd_unet_einsum_info(self._h, C.byref(n_marked), C.byref(n_applied)))
        return n_marked.value, n_applied.value

    def einsum_layers(self):
        """Module names (``<block>.attn1.einsum``) of the attentions that run on the int8 attention kernel, in build order."""
        n = _lib.lib().sd_unet_einsum_layer(self._h, -1, None, 0)
        if n < 0:
            _lib.check(n)
        name = C.create_string_buffer(512)
        out = []
        for i in range(n):
            if _lib.lib().sd_unet_einsum_layer(self._h, i, name, len(name)) < 0:
                _lib.check(-1)
            out.append(name.value.decode())
        return out

    def activation_ranges(self):
        """{layer: max |x| over the conv's input(s) of every forward so far} of a handle built with ``observe_activations=True``
        (empty otherwise; an observed Einsum has three slots ``<module>.q`` / ``.k`` / ``.v``): the calibration of
        ``activation_quantization.recipe_from_ranges``."""
        n = _lib.lib().sd_unet_activation_ranges(self._h, -1, None, 0, None)
        if n < 0:
            _lib.check(n)
        name = C.create_string_buffer(512)
        v = C.c_float(0)
        out = {}
        for i in range(n):
            st = _lib.lib().sd_unet_activation_ranges(self._h, i, name, len(name), C.byref(v))
            if st < 0:
                _lib.check(st)
            slot = name.value.decode()   # a conv's weight tensor, or an einsum's <module>.q / .k / .v
            out[slot[:-len(".weight")] if slot.endswith(".weight") else slot] = float(v.value)
        return out

    def close(self):
        if getattr(self, "_h", None) and getattr(self, "_attached", None):
            try:
                self.attach_controlnets([])
            except Exception:
                pass
        super().close()


def _profile(handle, iters):
    n = C.c_int(0)
    _lib.check(_lib.lib().sd_unet_profile(handle, iters, 0, None, None, None, 0, C.byref(n)))
    cap, lb = n.value, 160
    ms = np.zeros(cap, np.float32)
    flop = np.zeros(cap, np.float64)
    labels = C.create_string_buffer(cap * lb)
    _lib.check(_lib.lib().sd_unet_profile(handle, iters, cap, _lib.fptr(ms), flop.ctypes.data_as(C.POINTER(C.c_double)),
                                          labels, lb, C.byref(n)))
    return [(labels.raw[i * lb:(i + 1) * lb].split(b"\0", 1)[0].decode(), float(flop[i]), float(ms[i])) for i in range(cap)]


VAE_CONFIGS = {   # public AutoencoderKL config of SD 1.x / 2.x (decoder side)
    "stabilityai/stable-diffusion-2-1-base": dict(latent_channels=4, out_channels=3,
                                                   block_out_channels=(128, 256, 512, 512), layers_per_block=2),
}
VAE_CONFIGS["runwayml/stable-diffusion-v1-5"] = VAE_CONFIGS["stabilityai/stable-diffusion-2-1-base"]


class HipVaeDecoder(_lib.Model):
    """``vae_decoder`` model runner: ``decoder(post_quant_conv(z))`` (torch2coreml.py:584-594) behind
    the CoreMLModel interface: ``expected_inputs["z"]`` (pipeline.py:315) and
    ``model(z=...)["image"]`` in [-1, 1] (pipeline.py:316), NCHW fp32.
    ``dtype`` is the model's declared input dtype AND its compute precision, as in the reference's conversion
    (torch2coreml.py:570-578): ``np.float16`` = the MFMA kernels (fp16 storage, fp32 accumulation); ``np.float32`` = fp32
    activations and arithmetic end to end (``compute_fp32``), what the stock SDXL VAE needs."""
    _destroy = "sd_unet_destroy"

    def __init__(self, config, weights, batch=1, latent_height=64, latent_width=64, device=0, use_graph=True,
                 dtype=np.float16):
        if isinstance(config, str):
            if config not in VAE_CONFIGS:
                raise ValueError(f"unknown VAE config {config!r}")
            config = VAE_CONFIGS[config]
        self.config = dict(config)
        boc = tuple(config["block_out_channels"])
        c = _lib.UNetConfig()
        c.batch, c.in_channels, c.out_channels = batch, config["latent_channels"], config["out_channels"]
        c.height, c.width, c.n_levels = latent_height, latent_width, len(boc)
        _fill(c.block_out_channels, boc)
        c.layers_per_block = config["layers_per_block"]
        c.norm_num_groups, c.norm_eps = 32, 1e-6
        c.use_graph = int(use_graph)
        if np.dtype(dtype) not in (np.dtype(np.float16), np.dtype(np.float32)):
            raise ValueError(f"VAE dtype must be float16 or float32, got {dtype}")
        c.compute_fp32 = int(np.dtype(dtype) == np.float32)
        self.compute_dtype = np.dtype(dtype)
        self._h = C.c_void_p()
        with Weights.lend(weights) as store:
            _lib.check(_lib.lib().sd_vae_decoder_create(C.byref(c), store._h, device, C.byref(self._h)))
        self.batch, self.latent_height, self.latent_width = batch, latent_height, latent_width
        up = 2 ** (len(boc) - 1)
        self.image_shape = (batch, config["out_channels"], latent_height * up, latent_width * up)
        self.expected_inputs = {"z": {"shape": (batch, config["latent_channels"], latent_height, latent_width),
                                      "dtype": np.dtype(dtype)}}

    def __call__(self, **kwargs):
        self._verify_inputs(**kwargs)
        z = np.ascontiguousarray(kwargs["z"])
        image = np.empty(self.image_shape, np.float32)
        _lib.check(_lib.lib().sd_vae_decode(self._h, _lib.ptr(z), 1 if z.dtype == np.float32 else 0,
                                            _lib.fptr(image), 0))
        return {"image": image}

    def decode_images(self, z, safety_checker=None, image_post=None, adjustment=0.0, want_image=True, want_rgb8=True):
        """The decoder, then the image post-processing and the safety checker without leaving the device (sd_vae_decode_images;
        pipeline.py:286-320): returns ``{"image"`` (B, 3, H, W) f32 in [-1, 1] ``, "rgb8"`` (B, H, W, 3) uint8 - what
        ``numpy_to_pil`` makes of it - ``, "has_nsfw_concepts"`` (B,) bool ``, "concept_scores"`` (B, n) f32 ``}``; an output that was
        not asked for (``want_image`` / ``want_rgb8`` False, no ``safety_checker``) is None.  The flagged images come back zeroed in
        ``image`` and ``rgb8``.  ``safety_checker``: a ``HipSafetyChecker`` whose static batch divides this decoder's, on the same
        device; it needs ``image_post`` (``safety_checker.image_post(...)``: the checkpoint's CLIPImageProcessor for this image size)."""
        self._verify_inputs(z=z)
        z = np.ascontiguousarray(z)
        if safety_checker is not None and not isinstance(image_post, _lib.ImagePost):
            raise ValueError("decode_images: a safety checker needs image_post (safety_checker.image_post(...))")
        B, _, H, W = self.image_shape
        image = np.empty(self.image_shape, np.float32) if want_image else None
        rgb8 = np.empty((B, H, W, 3), np.uint8) if want_rgb8 else None
        flags = scores = None
        if safety_checker is not None:
            flags = np.empty(B, np.float32)
            scores = np.empty((B, safety_checker._cfg_struct.num_concepts), np.float32)
        _lib.check(_lib.lib().sd_vae_decode_images(
            self._h, _lib.ptr(z), 1 if z.dtype == np.float32 else 0, _lib.fptr(image), _lib.ptr(rgb8),
            safety_checker._h if safety_checker is not None else None, C.byref(image_post) if safety_checker is not None else None,
            float(adjustment), _lib.fptr(flags), _lib.fptr(scores), 0))
        return {"image": image, "rgb8": rgb8, "has_nsfw_concepts": None if flags is None else flags > 0.5, "concept_scores": scores}

    def profile(self, iters=5):
        return _profile(self._h, iters)

    def time_forward(self, warmup=1, iters=5):
        ms = C.c_float(0)
        _lib.check(_lib.lib().sd_unet_time_forward(self._h, warmup, iters, C.byref(ms)))
        return ms.value

    @property
    def device_bytes(self):
        return _lib.lib().sd_unet_device_bytes(self._h)


class HipVaeEncoder(_lib.Model):
    """``vae_encoder`` model runner: ``quant_conv(encoder(x))`` (torch2coreml.py:739-749) behind the CoreMLModel
    interface: ``model(x=...)["latent"]`` = the posterior moments (B, 2*latent_channels, H/8, W/8) fp32,
    [mean | logvar]; sampling and the scale factor stay with the caller (Encoder.swift:48-90)."""
    _destroy = "sd_unet_destroy"

    def __init__(self, config, weights, batch=1, height=512, width=512, device=0, use_graph=True, dtype=np.float16):
        if isinstance(config, str):
            if config not in VAE_CONFIGS:
                raise ValueError(f"unknown VAE config {config!r}")
            config = VAE_CONFIGS[config]
        self.config = dict(config)
        boc = tuple(config["block_out_channels"])
        c = _lib.UNetConfig()
        c.batch, c.in_channels, c.out_channels = batch, 3, 2 * config["latent_channels"]
        c.height, c.width, c.n_levels = height, width, len(boc)
        _fill(c.block_out_channels, boc)
        c.layers_per_block = config["layers_per_block"]
        c.norm_num_groups, c.norm_eps = 32, 1e-6
        c.use_graph = int(use_graph)
        if np.dtype(dtype) not in (np.dtype(np.float16), np.dtype(np.float32)):
            raise ValueError(f"VAE dtype must be float16 or float32, got {dtype}")
        c.compute_fp32 = int(np.dtype(dtype) == np.float32)   # torch2coreml.py:726-733: the SDXL encoder is float32 too
        self.compute_dtype = np.dtype(dtype)
        self._h = C.c_void_p()
        with Weights.lend(weights) as store:
            _lib.check(_lib.lib().sd_vae_encoder_create(C.byref(c), store._h, device, C.byref(self._h)))
        down = 2 ** (len(boc) - 1)
        self.latent_shape = (batch, 2 * config["latent_channels"], height // down, width // down)
        self.expected_inputs = {"x": {"shape": (batch, 3, height, width), "dtype": np.dtype(dtype)}}

    def __call__(self, **kwargs):
        self._verify_inputs(**kwargs)
        x = np.ascontiguousarray(kwargs["x"])
        out = np.empty(self.latent_shape, np.float32)
        _lib.check(_lib.lib().sd_vae_encode(self._h, _lib.ptr(x), 1 if x.dtype == np.float32 else 0, _lib.fptr(out), 0))
        return {"latent": out}

    def encode_latents(self, x, eps, noise, scale_factor, sa, sb):
        """The noised starting latents of image-to-image in one call (``sd_vae_encode_latents``): the encoder, then on the device
        ``sa * (mean + std * eps) * scale_factor + sb * noise[i]`` (Encoder.swift:68-89, Scheduler.swift:83-102).  x as for
        ``__call__`` (batch 1: one starting image feeds every latent), eps (Cz, h, w) and noise (n_images, Cz, h, w) float32
        standard normals -> (n_images, Cz, h, w) float32."""
        self._verify_inputs(x=x)
        _, c2, h, w = self.latent_shape
        if self.latent_shape[0] != 1:
            raise ValueError(f"encode_latents needs an encoder handle of batch 1, this one has batch {self.latent_shape[0]}")
        for name, v in (("eps", eps), ("noise", noise)):
            if not isinstance(v, np.ndarray):
                raise TypeError(f"Expected numpy.ndarray, got {v} for input: {name}")
            if v.dtype != np.float32:
                raise TypeError(f"Expected dtype float32, got {v.dtype} for input: {name}")
        if eps.shape != (c2 // 2, h, w):
            raise TypeError(f"Expected shape {(c2 // 2, h, w)}, got {eps.shape} for input: eps")
        if noise.ndim != 4 or noise.shape[0] < 1 or noise.shape[1:] != (c2 // 2, h, w):
            raise TypeError(f"Expected shape {('n_images', c2 // 2, h, w)}, got {noise.shape} for input: noise")
        x, eps, noise = np.ascontiguousarray(x), np.ascontiguousarray(eps), np.ascontiguousarray(noise)
        out = np.empty(noise.shape, np.float32)
        _lib.check(_lib.lib().sd_vae_encode_latents(self._h, _lib.ptr(x), 1 if x.dtype == np.float32 else 0, _lib.fptr(eps),
                                                    _lib.fptr(noise), noise.shape[0], float(scale_factor), float(sa), float(sb),
                                                    _lib.fptr(out), 0))
        return out

    @property
    def device_bytes(self):
        return _lib.lib().sd_unet_device_bytes(self._h)
