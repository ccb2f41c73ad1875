"""W8A8 self-attention einsums without a GPU: the new symbols, the recipe format with its three-range entries, the marks of the weight
store, the host packer of the int8 V^T and the host refusals of sd_op_attention_w8a8 in the header's order."""
import json
import os

import numpy as np
import pytest

import w8a8_einsum_ref as ref
from python_hip_stable_diffusion import _lib, activation_quantization as aq, hip_model
from test_build_isa import CSRC, HIPCC, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = "down_blocks.1.attentions.0.transformer_blocks.0"
EINSUM = BLOCK + ".attn1.einsum"


def test_new_symbols_are_in_the_header_and_the_library():
    header = open(os.path.join(ROOT, "include", "sd_mi355x.h")).read()
    for sym in ("sd_weights_quantize_einsum", "sd_weights_einsum_info", "sd_weights_observe_einsums", "sd_unet_einsum_info", "sd_unet_einsum_layer",
                "sd_op_attention_w8a8", "sd_op_einsum_quantize", "sd_op_w8a8_pack_vt"):
        assert f"int {sym}(" in header and hasattr(_lib.lib(), sym), sym
        assert any(name == sym for name, _, _ in _lib.SYMBOLS), sym
    for fn in (_lib.attention_w8a8, _lib.einsum_quantize, _lib.w8a8_pack_vt, hip_model.Weights.quantize_einsum, hip_model.Weights.einsum_info,
               hip_model.HipModel.einsum_info, hip_model.HipModel.einsum_layers):
        assert callable(fn)
    assert "unpinned" in header[header.index("W8A8 einsums"):header.index("int sd_weights_quantize_einsum(")]


# ---- the recipe format ----
def test_recipe_round_trip_with_list_values(tmp_path):
    recipe = {BLOCK + ".attn1.to_out.0": 3.5, EINSUM: [1.5, 2.25, 7.0]}
    path = str(tmp_path / "r.json")
    aq.save_recipe(recipe, path)
    assert json.load(open(path)) == recipe
    assert aq.load_recipe(path) == recipe and aq.load_recipe(recipe) == recipe
    assert aq.load_recipe({EINSUM: (1, 2, 3)}) == {EINSUM: [1.0, 2.0, 3.0]}
    assert aq.is_einsum(EINSUM) and not aq.is_einsum(BLOCK + ".attn1.to_q")


@pytest.mark.parametrize("bad, key", [({EINSUM: 2.0}, EINSUM), ({EINSUM: [1.0, 2.0]}, EINSUM), ({EINSUM: [1.0, 2.0, 3.0, 4.0]}, EINSUM),
                                      ({EINSUM: [1.0, 0.0, 3.0]}, EINSUM), ({EINSUM: [1.0, float("nan"), 3.0]}, EINSUM),
                                      ({EINSUM: "1,2,3"}, EINSUM), ({BLOCK + ".attn1.to_q": [1.0, 2.0, 3.0]}, BLOCK + ".attn1.to_q"),
                                      ({BLOCK + ".ff.net.2.weight": [4.0]}, BLOCK + ".ff.net.2")])
def test_recipe_value_errors_name_the_key(bad, key, tmp_path):
    with pytest.raises(ValueError) as e:
        aq.load_recipe(bad)
    assert key in str(e.value)
    with pytest.raises(ValueError):
        aq.save_recipe(bad, str(tmp_path / "bad.json"))


def test_every_existing_recipe_loads_as_before():
    old = {BLOCK + ".attn1.to_q": 6.0, "mid_block.resnets.0.conv1.weight": 2.5}
    assert aq.load_recipe(old) == {BLOCK + ".attn1.to_q": 6.0, "mid_block.resnets.0.conv1": 2.5}
    assert aq.recipe_from_ranges({"a.weight": 1.0, "b": 2.0}) == {"a": 1.0, "b": 2.0}


def test_recipe_from_ranges_folds_the_three_slots():
    ranges = {BLOCK + ".attn1.to_out.0.weight": 3.5, EINSUM + ".q": 1.5, EINSUM + ".k": 2.25, EINSUM + ".v": 7.0}
    assert aq.recipe_from_ranges(ranges) == {BLOCK + ".attn1.to_out.0": 3.5, EINSUM: [1.5, 2.25, 7.0]}
    assert aq.recipe_from_ranges(ranges, skip=[EINSUM]) == {BLOCK + ".attn1.to_out.0": 3.5}
    with pytest.raises(ValueError, match="einsum"):
        aq.recipe_from_ranges({EINSUM + ".q": 1.5, EINSUM + ".k": 2.25})          # a slot missing
    with pytest.raises(ValueError, match="einsum"):
        aq.recipe_from_ranges({EINSUM + ".q": 1.5, EINSUM + ".k": 0.0, EINSUM + ".v": 1.0})   # never run


def test_scopes():
    assert aq.EINSUM_SCOPES == {"einsum": "einsum"}
    assert list(aq.every_calibration_scope()) == list(aq.all_calibration_scopes()) + ["einsum"]
    from python_hip_stable_diffusion import pipeline as P
    base = ["--prompt", "x", "-i", "in", "-o", "out", "--seed", "1"]
    assert P.build_parser().parse_args(base + ["--calibrate-scope", "einsum"]).calibrate_scope == "einsum"
    assert hip_model.observe_level("einsum") == 2


# ---- the marks of the weight store ----
def make_store():
    z = np.zeros((64, 64, 1, 1), np.float32)
    return hip_model.Weights(tensors={BLOCK + ".attn1.to_q.weight": z, BLOCK + ".attn1.to_k.weight": z, BLOCK + ".attn2.to_q.weight": z})


def test_store_marks_not_found_bad_range_and_round_trip():
    store = make_store()
    try:
        assert store.einsum_info(EINSUM) is None
        for missing in ("up_blocks.0.attentions.0.transformer_blocks.0.attn1.einsum", BLOCK + ".attn1", BLOCK + ".attn1.to_q", ".einsum"):
            with pytest.raises(KeyError):
                store.quantize_einsum(missing, 1.0, 1.0, 1.0)
        lib = _lib.lib()
        assert lib.sd_weights_quantize_einsum(store._h, b"nowhere.einsum", 1.0, 1.0, 1.0) == -2      # SD_ERR_NOT_FOUND
        for bad in ((0.0, 1.0, 1.0), (1.0, -2.0, 1.0), (1.0, 1.0, float("inf")), (float("nan"), 1.0, 1.0)):
            with pytest.raises(ValueError, match="positive finite"):
                store.quantize_einsum(EINSUM, *bad)
            assert store.einsum_info(EINSUM) is None
        store.quantize_einsum(EINSUM, 1.5, 2.25, 7.0)
        assert store.einsum_info(EINSUM) == (1.5, 2.25, 7.0)
        store.quantize_einsum(EINSUM, 3.0, 2.25, 7.0)                            # a second mark replaces the first
        assert store.einsum_info(EINSUM) == (3.0, 2.25, 7.0)
        store.quantize_einsum(BLOCK + ".attn2.einsum", 1.0, 2.0, 3.0)            # any attention of the store may carry a mark
        assert store.einsum_info(BLOCK + ".attn2.einsum") == (1.0, 2.0, 3.0)
        assert store.w8a8_info(BLOCK + ".attn1.to_q.weight") is None             # an einsum mark is no conv mark
        assert lib.sd_weights_quantize_einsum(None, EINSUM.encode(), 1.0, 1.0, 1.0) == -1 and lib.sd_weights_einsum_info(None, EINSUM.encode(), None) == 0
    finally:
        store.close()


def test_observe_einsums_flag_contract():
    store = make_store()
    try:
        lib = _lib.lib()
        assert lib.sd_weights_observe_einsums(store._h, 1) == 0 and lib.sd_weights_observe_einsums(store._h, 0) == 0
        for bad in (2, -1):
            assert lib.sd_weights_observe_einsums(store._h, bad) == -1
        assert lib.sd_weights_observe_einsums(None, 1) == -1
        for on in ("einsum", False, "einsum", "tail", True, False):
            store.observe_activations(on)
        with pytest.raises(ValueError):
            store.observe_activations("einsums")
    finally:
        store.close()


def test_apply_marks_einsums_and_returns_nothing_for_them():
    store = make_store()
    try:
        errs = aq.apply(store, {EINSUM: [1.5, 2.25, 7.0], BLOCK + ".attn1.to_k": 4.0})
        assert set(errs) == {BLOCK + ".attn1.to_k"}
        assert store.einsum_info(EINSUM) == (1.5, 2.25, 7.0) and store.w8a8_info(BLOCK + ".attn1.to_k.weight") is not None
        with pytest.raises(KeyError, match="einsum"):
            aq.apply(store, {"mid_block.attentions.0.transformer_blocks.0.attn1.einsum": [1.0, 1.0, 1.0]})
    finally:
        store.close()


# ---- the host packer of the int8 V^T ----
@pytest.mark.parametrize("B, C, S", [(1, 2, 64), (2, 3, 192)])
def test_pack_vt_is_the_documented_permutation_inside_every_64_key_tile(B, C, S):
    keys = np.arange(S)
    v = np.empty((B * S, C), np.int8)
    for b in range(B):
        for c in range(C):
            v[b * S:(b + 1) * S, c] = ((keys * 5 + 17 * c + 31 * b) % 251 - 125).astype(np.int8)
    vt = _lib.w8a8_pack_vt(v, B)
    assert vt.shape == (B, C, S) and vt.dtype == np.int8
    p = np.arange(S)
    src = (p & ~31) + ref.vt_key(p & 31)                                          # its own documented formula
    for tile in range(S // 64):                                                   # a permutation within every 64-key tile
        assert sorted(src[64 * tile:64 * tile + 64]) == list(range(64 * tile, 64 * tile + 64))
    assert sorted(ref.vt_key(np.arange(32))) == list(range(32)) and [ref.vt_key(i) for i in (0, 1, 4, 5, 16, 31)] == [0, 1, 8, 9, 4, 31]
    want = v.reshape(B, S, C).transpose(0, 2, 1)[:, :, src]
    assert np.array_equal(vt, want)
    n = np.zeros(1, np.uint64)
    lib = _lib.lib()
    import ctypes as C_
    size = C_.c_size_t(0)
    assert lib.sd_op_w8a8_pack_vt(_lib.ptr(v), B, C, S, None, C_.byref(size)) == 0 and size.value == B * C * S
    assert lib.sd_op_w8a8_pack_vt(_lib.ptr(v), B, C, 48, None, C_.byref(size)) == -1      # S not a multiple of 32
    assert lib.sd_op_w8a8_pack_vt(None, B, C, S, None, C_.byref(size)) == -1 and n[0] == 0


# ---- the host refusals of the operator, in the header's order: no device work in front of any of them ----
def test_attention_w8a8_host_refusals_in_the_headers_order():
    S = 64
    good = np.ones((S, 64), np.int8)
    bad = good.copy()
    bad[3, 5] = -128
    nan = float("nan")
    a = _lib.attention_w8a8
    with pytest.raises(ValueError, match="empty"):                               # (1) in front of everything else
        _lib.check(_lib.lib().sd_op_attention_w8a8(_lib.ptr(bad), _lib.ptr(bad), _lib.ptr(bad), nan, nan, nan, _lib.ptr(np.empty(1, np.float16)), 0, 1, 100, 1, None))
    with pytest.raises(ValueError, match="NULL"):
        _lib.check(_lib.lib().sd_op_attention_w8a8(None, _lib.ptr(bad), _lib.ptr(bad), nan, nan, nan, None, 1, 1, 100, 1, None))
    for s_off in (100, 32, 96):                                                  # (2) the shape rule in front of the bound, the ranges, the values
        with pytest.raises(ValueError, match="off the shape rule"):
            a(bad, bad, bad, nan, nan, nan, 1, 1, S=s_off)
    with pytest.raises(ValueError, match="off the shape rule"):
        a(bad, bad, bad, nan, nan, nan, 1, 1, S=ref.MAX_S + 32)
    with pytest.raises(ValueError, match="133120"):                              # (3) the integer bound in front of the ranges and the values
        a(bad, bad, bad, nan, nan, nan, 1, 1, S=ref.MAX_S + 64)
    for ranges in ((nan, 1.0, 1.0), (1.0, 0.0, 1.0), (1.0, 1.0, float("inf")), (-1.0, 1.0, 1.0)):   # (4) in front of the values
        with pytest.raises(ValueError, match="positive finite"):
            a(bad, bad, bad, *ranges, 1, 1)
    for which, args in (("q", (bad, good, good)), ("k", (good, bad, good)), ("v", (good, good, bad)), ("q", (bad, bad, bad))):   # (5)
        with pytest.raises(ValueError, match=f"{which} value -128"):
            a(*args, 1.0, 1.0, 1.0, 1, 1)
    assert ref.MAX_S == 133120 and 127 * 127 * ref.MAX_S < 2 ** 31 <= 127 * 127 * (ref.MAX_S + 64)


def test_einsum_quantize_host_refusals():
    qk, vt = np.zeros((64, 128), np.float16), np.zeros((1, 64, 64), np.float16)
    with pytest.raises(ValueError, match="positive finite"):
        _lib.einsum_quantize(qk, vt, 0.0, 1.0, 1.0)
    with pytest.raises(ValueError, match="vt_perm_in"):
        _lib.einsum_quantize(qk, vt, 1.0, 1.0, 1.0, vt_perm_in=2)
    with pytest.raises(ValueError, match="einsum_quantize"):
        _lib.einsum_quantize(np.zeros((48, 128), np.float16), np.zeros((1, 64, 48), np.float16), 1.0, 1.0, 1.0)   # S = 48


# ---- the restatement itself ----
def test_restatement_properties():
    rs = np.random.RandomState(5)
    S = 128
    q, k, v = (rs.randint(-127, 128, size=(S, 64)).astype(np.int8) for _ in range(3))
    q[7] = 0                                                                      # every score equal: every p_q is 127
    p = ref.probabilities(q, k, ref.score_scale(2.0, 2.0))
    assert p.min() >= 0 and p.max() == 127 and (p.max(axis=1) == 127).all() and (p[7] == 127).all()
    out = ref.attention(q, k, v, 2.0, 2.0, 3.0, 1, 1)
    want = (v.astype(np.float64).mean(axis=0) * np.float64(ref.scale(3.0))).astype(np.float16)
    assert np.array_equal(out[7].view(np.uint16), want.view(np.uint16))
    x = np.array([0.0, 1.0, -1.0, 0.4999, 2.5, 3.5, 1e4, -1e4, np.inf, -np.inf, np.nan], np.float16)
    assert list(ref.quantize(x, 127.0)) == [0, 1, -1, 0, 2, 4, 127, -127, 127, -127, 0]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_attention_i8_compiles_for_gfx950_without_scratch(tmp_path):
    res = kernel_resources(os.path.join(CSRC, "attention_i8.hip"), tmp_path)
    kernels = {k: v for k, v in res.items() if "attn_i8_kernel" in k}
    assert len(kernels) == 2 and any("ILi4E" in k for k in kernels) and any("ILi8E" in k for k in kernels), list(res)   # 4 and 8 waves
    assert any("einsum_quantize_kernel" in k for k in res) and any("einsum_absmax_kernel" in k for k in res)
    for name, (vgpr, scratch) in res.items():
        assert scratch == 0, f"{name}: {scratch} bytes of scratch (register spills)"
        assert 0 < vgpr <= 128, (name, vgpr)                                     # eight waves per workgroup: two per SIMD, and room for two workgroups
    asm = kernel_resources.last_asm
    assert "v_mfma_i32_32x32x32_i8" in asm and "v_dot4_u32_u8" in asm
