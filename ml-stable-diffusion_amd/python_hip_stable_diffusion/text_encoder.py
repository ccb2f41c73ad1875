"""``HipTextEncoder`` - the CLIP text encoder(s) behind the reference's model-runner seam.

Duck-types the ``text_encoder`` / ``text_encoder_2`` ``CoreMLModel`` objects the pipeline calls
(python_coreml_stable_diffusion/pipeline.py:151-175): ``expected_inputs["input_ids"]`` is (1, 77)
float32 (pipeline.py:173 passes the token ids as float32, a coremltools quirk), the call returns
``{"last_hidden_state", "pooled_outputs"}`` or, for SDXL, ``{"hidden_embeds", "pooled_outputs"}``
(names fixed at torch2coreml.py:439-441).  The arithmetic is transformers' CLIPTextModel /
CLIPTextModelWithProjection (third-party; transformers==4.44.2 in the reference's setup.py:20) with
the causal mask of torch2coreml.py:363-377, run by ``libsdmi355.so`` (csrc/text_encoder.cpp).
Tokenisation stays with transformers' CLIPTokenizer exactly as in the reference (pipeline.py:146-150).
"""
import ctypes as C
import json
import os

import numpy as np

from . import _lib
from .hip_model import Weights

TextEncoderConfig = _lib.TextEncoderConfig


def load_tokenizer(folder):
    """transformers' CLIPTokenizer from a checkpoint's ``tokenizer/`` folder (vocab.json + merges.txt)."""
    if not os.path.isdir(folder):
        raise FileNotFoundError(f"{folder} not found (coreml_model.py:176-178)")
    from transformers import CLIPTokenizer
    return CLIPTokenizer.from_pretrained(folder)


class HipTextEncoder(_lib.Model):
    _destroy = "sd_text_encoder_destroy"

    def __init__(self, config, weights, xl=False, with_projection=None, device=0, use_graph=True):
        cfg = dict(config)
        act = cfg.get("hidden_act", "quick_gelu")
        if act not in _lib.ACTS:
            raise NotImplementedError(f"hidden_act {act!r} (CLIP text towers use quick_gelu or gelu)")
        if with_projection is None:
            with_projection = "WithProjection" in str((cfg.get("architectures") or [""])[0])
        self.config = cfg
        self.xl = xl
        self.eos_token_id = cfg.get("eos_token_id", 2)
        c = TextEncoderConfig()
        c.vocab_size, c.hidden_size = cfg["vocab_size"], cfg["hidden_size"]
        c.intermediate_size, c.num_hidden_layers = cfg["intermediate_size"], cfg["num_hidden_layers"]
        c.num_attention_heads = cfg["num_attention_heads"]
        c.max_position_embeddings = cfg.get("max_position_embeddings", 77)
        c.hidden_act = _lib.ACTS[act]
        c.projection_dim = int(cfg.get("projection_dim", cfg["hidden_size"])) if with_projection else 0
        c.layer_norm_eps = float(cfg.get("layer_norm_eps", 1e-5))
        c.use_graph = int(use_graph)
        self._cfg_struct = c
        self._h = C.c_void_p()
        with Weights.lend(weights) as store:
            _lib.check(_lib.lib().sd_text_encoder_create(C.byref(c), store._h, device, C.byref(self._h)))
        self.seq_len, self.hidden_size = c.max_position_embeddings, c.hidden_size
        self.pooled_dim = c.projection_dim or c.hidden_size
        self.expected_inputs = {"input_ids": {"shape": (1, self.seq_len), "dtype": np.dtype(np.float32)}}

    @classmethod
    def from_pretrained(cls, folder, **kw):
        path = _lib.checkpoint_file(folder)
        with open(os.path.join(folder, "config.json")) as f:
            return cls(json.load(f), path, **kw)

    def eos_index(self, ids):
        """Position whose final-LayerNorm row is pooled (CLIPTextTransformer.forward): the arg-max token id for the
        legacy eos_token_id == 2 configs, else the first occurrence of eos_token_id."""
        ids = np.asarray(ids).reshape(-1)
        if self.eos_token_id == 2:
            return int(np.argmax(ids))
        hits = np.nonzero(ids == self.eos_token_id)[0]
        return int(hits[0]) if len(hits) else 0

    def __call__(self, **kwargs):
        self._verify_inputs(**kwargs)
        ids = np.ascontiguousarray(np.rint(kwargs["input_ids"]).astype(np.int32))
        hidden = np.empty((1, self.seq_len, self.hidden_size), np.float32)
        pooled = np.empty((1, self.pooled_dim), np.float32)
        i32p = ids.ctypes.data_as(C.POINTER(C.c_int32))
        if self.xl:
            _lib.check(_lib.lib().sd_text_encoder_encode(self._h, i32p, self.eos_index(ids), None, _lib.fptr(hidden),
                                                         _lib.fptr(pooled)))
            return {"hidden_embeds": hidden, "pooled_outputs": pooled}
        _lib.check(_lib.lib().sd_text_encoder_encode(self._h, i32p, self.eos_index(ids), _lib.fptr(hidden), None,
                                                     _lib.fptr(pooled)))
        return {"last_hidden_state": hidden, "pooled_outputs": pooled}

    @property
    def device_bytes(self):
        return _lib.lib().sd_text_encoder_device_bytes(self._h)
