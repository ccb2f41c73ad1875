"""CPU suite of the CLIP text encoder (csrc/text_encoder.cpp behind HipTextEncoder): what can be refused on the host is refused
there, before the handle asks for a device - so these raise the same way with and without a GPU."""
import numpy as np
import pytest

from oracle import clip_ref, weights


def test_a_checkpoint_with_a_missing_or_mis_sized_layer_tensor_is_refused_before_any_device_work(sdlib):
    from python_hip_stable_diffusion import HipTextEncoder
    cfg = clip_ref.CONFIGS["mini-l"]
    sd = weights.make_state_dict(clip_ref.param_shapes(cfg), seed=7, dtype=np.float16, gain=2.0)
    name = "text_model.encoder.layers.0.layer_norm2.bias"
    with pytest.raises(FileNotFoundError, match="layers.0.layer_norm2.bias"):
        HipTextEncoder(cfg, {k: v for k, v in sd.items() if k != name})
    name = "text_model.encoder.layers.0.mlp.fc1.weight"
    wrong = dict(sd)
    wrong[name] = np.zeros((cfg["intermediate_size"], cfg["hidden_size"] + 8), np.float16)
    with pytest.raises(ValueError, match="layers.0.mlp.fc1.weight"):
        HipTextEncoder(cfg, wrong)
