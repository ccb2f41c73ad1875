"""GPU suite: palettized weights on the device.  The palettized weight-stream conv (plan tile 14) decodes its indices in front of
the same MFMAs in the same order as the fp16 weight stream (plan tile 9), so every comparison against tile 9 on lut[indices] is an
array_equal, at the operator, on a whole handle and through the pipeline.

Shapes: the MFMA path of launch_conv takes input channel counts that are multiples of 64 (conv_fast_path_ok), so the operator cases
use the smallest such shapes that still reach each form of the kernel: two slices with six dead waves, a ragged last workgroup of
slices, three K splits, a second source, the upsample gather, the 16-pixel-wide form, ragged and multi-block M of the 1x1 form, and
three images with H != W (a block that is one image, blocks that straddle images with a half-empty last one, one sub-tile per image)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle import psnr, unet_ref, weights
from python_hip_stable_diffusion import HipModel, _lib, hip_model, palettize

pytestmark = pytest.mark.gpu

NBITS = (1, 2, 4, 6, 8)
BIG = 65504.0

# (B, C0, C1, H, W, Cout, k, upsample, nw): H x W is the SOURCE image
CASES = {
    "3x3 W=8 two slices, six dead waves": (1, 64, 0, 8, 8, 32, 3, False, 8),
    "3x3 W=8 ragged last workgroup of slices": (2, 192, 0, 8, 8, 64, 3, False, 4),
    "3x3 W=8 three splits": (2, 320, 0, 8, 8, 64, 3, False, 4),
    "3x3 W=8 second source": (2, 64, 128, 8, 8, 64, 3, False, 8),
    "3x3 W=8 upsample from 4x4": (2, 64, 0, 4, 4, 32, 3, True, 8),
    "3x3 W=16": (2, 64, 0, 16, 16, 32, 3, False, 8),
    "1x1 M=72": (1, 64, 0, 8, 9, 32, 1, False, 8),
    "1x1 M=200 two M blocks": (2, 64, 0, 10, 10, 32, 1, False, 4),
    # H != W: the loader finds image and row of each 8-row sub-tile from H / 8 sub-tiles per image
    "3x3 16x8 a block is one image": (2, 64, 0, 16, 8, 32, 3, False, 8),
    "3x3 24x8 batch 3 blocks straddle images": (3, 64, 0, 24, 8, 32, 3, False, 4),
    "3x3 8x16 one sub-tile per image": (2, 64, 0, 8, 16, 32, 3, False, 8),
}


def h16(a):
    return np.asarray(a, np.float32).astype(np.float16)


def make_palette(rs, nbits, ktot, case_no):
    """A LUT with -0, +0, a subnormal, +-65504 and NaN entries no index uses (as many of them as 2^nbits leaves room for beside two
    ordinary values; the small LUTs take turns over the cases), and which entries an index may use: `big` only against the first
    input channel, whose activations are small (and normal fp16 numbers), so that the sums stay inside fp16."""
    n = 1 << nbits
    lut = h16(rs.randn(n) / np.sqrt(ktot))
    specials = [np.float16(-0.0), np.float16(0.0), np.float16(6e-8), np.float16(BIG), np.float16(-BIG)]
    room = max(0, min(len(specials), n - 2)) if n > 2 else 1
    chosen = [specials[(case_no + i) % len(specials)] for i in range(room)]
    for i, v in enumerate(chosen):
        lut[i] = v
    unused = list(range(n - n // 4, n)) if n >= 16 else []
    for i in unused:
        lut[i] = np.float16(np.nan)
    big = [i for i in range(n) if np.isfinite(lut[i]) and abs(float(lut[i])) == BIG]
    ordinary = [i for i in range(n) if i not in unused and i not in big]
    return lut, np.array(ordinary), np.array(big, dtype=np.int64)


def make_case(name, nbits):
    B, C0, C1, H, W, Cout, k, ups, nw = CASES[name]
    case_no = list(CASES).index(name)
    rs = np.random.RandomState(1000 * nbits + case_no)
    ctot = C0 + C1
    lut, ordinary, big = make_palette(rs, nbits, ctot * k * k, case_no)
    idx = ordinary[rs.randint(0, len(ordinary), size=(Cout, ctot, k, k))].astype(np.uint8)
    if len(big):
        sel = rs.rand(Cout, k, k) < 0.5
        idx[:, 0][sel] = big[rs.randint(0, len(big), size=int(sel.sum()))]
    x = h16(rs.randn(B, C0, H, W))
    x[:, 0] = h16(np.sign(rs.randn(B, H, W)) * 2.0 ** -10 * (1 + rs.rand(B, H, W)))   # 65504 x these: at most 128 per product
    x1 = h16(rs.randn(B, C1, H, W)) if C1 else None
    up = 2 if ups else 1
    bias = (0.1 * rs.randn(Cout)).astype(np.float32)
    res = h16(rs.randn(B, Cout, H * up, W * up))
    return dict(x=x, x1=x1, lut=lut, idx=idx, bias=bias, res=res, ups=ups, nw=nw, shape=(B, Cout, H * up, W * up))


def torch_reference(c):
    import torch
    import torch.nn.functional as F
    xs = c["x"] if c["x1"] is None else np.concatenate([c["x"], c["x1"]], axis=1)
    xt = torch.from_numpy(xs.astype(np.float32))
    if c["ups"]:
        xt = F.interpolate(xt, scale_factor=2.0, mode="nearest")
    w = torch.from_numpy(c["lut"][c["idx"]].astype(np.float32))
    y = F.conv2d(xt, w, torch.from_numpy(c["bias"]), padding=c["idx"].shape[2] // 2) + torch.from_numpy(c["res"].astype(np.float32))
    return y.numpy()


def gate(got, ref, what):
    """the gate of tests/test_ops_gpu.py (close): PSNR >= 60 dB, max |err| <= 4e-3 max|ref| + 1e-3"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    p, err, bound = psnr.compute_psnr(got, ref), np.abs(got - ref).max(), 4e-3 * np.abs(ref).max() + 1e-3
    assert p >= 60.0 and err <= bound, f"{what}: PSNR {p:.1f} dB, max|err| {err:.3e} (bound {bound:.3e})"


@pytest.mark.parametrize("nbits", NBITS)
@pytest.mark.parametrize("name", list(CASES))
def test_operator_is_bit_identical_to_the_fp16_weight_stream(name, nbits):
    c = make_case(name, nbits)
    n = int(np.prod(c["shape"]))
    guard = 4 * c["shape"][3] * c["shape"][1]
    buf = np.full(n + guard, np.nan, np.float16)
    out, plan, _ = _lib.conv2d_palettized(c["x"], c["lut"], c["idx"], nbits, bias=c["bias"], res=c["res"], x1=c["x1"], upsample=c["ups"],
                                          nw=c["nw"], out=buf)
    out = out.copy()
    assert np.isnan(buf[n:]).all() and not np.isnan(buf[:n]).any()
    nslices = c["idx"].shape[1] // 32
    assert plan == [14, 4 if c["nw"] == 4 else 0, -(-nslices // c["nw"]), 1], plan
    w = c["lut"][c["idx"]]
    assert np.isfinite(w).all()                                                 # no index reaches a NaN entry
    ref, _, rplan, _ = _lib.conv2d_ex(c["x"], w, bias=c["bias"], res=c["res"], x1=c["x1"], upsample=c["ups"], tile=49 if c["nw"] == 4 else 9)
    assert rplan[0] == 9 and rplan[1:] == plan[1:], (rplan, plan)              # the reference really is the fp16 weight stream
    assert np.array_equal(out.view(np.uint16), ref.view(np.uint16)), f"{name} at {nbits} bits: {np.count_nonzero(out != ref)} elements differ"
    again, _, _ = _lib.conv2d_palettized(c["x"], c["lut"], c["idx"], nbits, bias=c["bias"], res=c["res"], x1=c["x1"], upsample=c["ups"],
                                         nw=c["nw"], iters=3)
    assert np.array_equal(out.view(np.uint16), again.view(np.uint16))
    want = torch_reference(c)
    gate(out, want, f"palettized {name} {nbits} bits")
    gate(ref, want, f"tile 9 {name} {nbits} bits")


def test_operator_refusals():
    rs = np.random.RandomState(0)
    lut = h16(rs.randn(16))
    ok = rs.randint(0, 16, size=(32, 64, 3, 3)).astype(np.uint8)
    x = h16(rs.randn(1, 64, 8, 8))
    _lib.conv2d_palettized(x, lut, ok, 4)
    with pytest.raises(ValueError):                                             # 12-pixel-wide image: not a weight-stream shape
        _lib.conv2d_palettized(h16(rs.randn(1, 64, 8, 12)), lut, ok, 4)
    with pytest.raises(ValueError):                                             # 32 input channels: off the MFMA path
        _lib.conv2d_palettized(h16(rs.randn(1, 32, 8, 8)), lut, ok[:, :32], 4)
    with pytest.raises(ValueError):                                             # 48 output channels
        _lib.conv2d_palettized(x, lut, rs.randint(0, 16, size=(48, 64, 3, 3)).astype(np.uint8), 4)
    bad = ok.copy()
    bad[5, 7, 1, 1] = 16
    with pytest.raises(ValueError, match="index 16"):
        _lib.conv2d_palettized(x, lut, bad, 4)
    with pytest.raises(ValueError):
        _lib.conv2d_palettized(x, lut, ok, 4, nw=2)


# ---- handle ----
TINY = unet_ref.make_config(sample_size=16, block_out_channels=(32, 64), down_block_types=(unet_ref.CA, unet_ref.DN),
                            up_block_types=(unet_ref.UP, unet_ref.CAUP), layers_per_block=1, attention_head_dim=(2, 4), cross_attention_dim=48)
RECIPES = {"6 bits": 6, "mixed 2 / 8 / 16": (2, 8, 16)}


def tiny_stores(recipe):
    """(palettized store, plain store holding the same lut[indices] values, streamable weights by name)"""
    sd16 = weights.make_state_dict(unet_ref.unet_param_shapes(TINY), seed=33, dtype=np.float16)
    pal = hip_model.Weights(sd16)
    modules = palettize.palettizable(pal, min_size=1000)
    assert len(modules) >= 10
    bits = {m: (recipe if isinstance(recipe, int) else recipe[i % len(recipe)]) for i, m in enumerate(modules)}
    palettize.apply(pal, recipe=bits)
    plain = hip_model.Weights({k: (pal.read(k).astype(np.float16) if k.endswith(".weight") and pal.palette_bits(k) else v) for k, v in sd16.items()})
    n_pal = sum(1 for b in bits.values() if b != 16)
    return pal, plain, n_pal, pal.shapes()


def tiny_inputs():
    hw = TINY["sample_size"]
    return dict(sample=weights.seeded_normal((2, 4, hw, hw), 1).astype(np.float16), timestep=np.array([981, 981], np.float16),
                encoder_hidden_states=weights.seeded_normal((2, TINY["cross_attention_dim"], 1, 77), 2).astype(np.float16))


def compare_handles(recipe):
    """Builds the palettized and the plain handle, eager and graph; returns what the tests assert on."""
    pal, plain, n_pal, shapes = tiny_stores(recipe)
    inputs = tiny_inputs()
    r = {"n_pal_expected": n_pal, "equal": []}
    for use_graph in (False, True):
        hp = HipModel(TINY, pal, batch=2, use_graph=use_graph)
        hq = HipModel(TINY, plain, batch=2, use_graph=use_graph)
        for _ in range(2):                                                      # graph: the second call is a replay
            a, b = hp(**inputs)["noise_pred"], hq(**inputs)["noise_pred"]
            r["equal"].append(bool(np.isfinite(a).all() and np.array_equal(a, b)))
        r["info"] = list(hp.palette_info())
        r["info_plain"] = list(hq.palette_info())
        r["used"] = [hp.arena_used_bytes, hq.arena_used_bytes]
        r["device_bytes"] = [hp.device_bytes, hq.device_bytes]
        labels = [lab for lab, _, _ in hp.profile(1)]
        hp.close()
        hq.close()
    # the convs that read their weights from the palette are marked in the op labels: "conv3x3+pal6 64->64 ... K=576 <name> #key"
    marked = [re.search(r"^\S+\+pal\d+ \d+->(\d+) .* K=(\d+) ", lab) for lab in labels]
    r["streamed_weights"] = [int(m.group(1)) * int(m.group(2)) for m in marked if m]
    r["shapes"] = {k: list(v) for k, v in shapes.items()}
    r["bits"] = {k: pal.palette_bits(k) for k in shapes}
    pal.close()
    plain.close()
    return r


@pytest.mark.parametrize("recipe", list(RECIPES))
def test_handle_from_a_palettized_store_equals_the_depalettized_one(recipe):
    r = compare_handles(RECIPES[recipe])
    n_pal, n_streamed, stream_bytes = r["info"]
    assert r["info_plain"] == [0, 0, 0]
    assert n_pal == r["n_pal_expected"] and n_streamed >= 1 and stream_bytes > 0
    assert all(r["equal"]) and len(r["equal"]) == 4, r["equal"]                 # eager twice, graph capture + replay
    used_pal, used_plain = r["used"]
    assert used_pal < used_plain and r["device_bytes"][0] <= r["device_bytes"][1]
    # The streamed convs dropped both fp16 copies - the [Cout][k][k][Cin] upload and the fragment-major one: 4 bytes per weight - and
    # hold stream_bytes instead; every allocation is a multiple of the arena's 256-byte alignment
    assert len(r["streamed_weights"]) == n_streamed
    assert abs((used_plain - used_pal) - (4 * sum(r["streamed_weights"]) - stream_bytes)) <= 256 * n_streamed, (r["used"], r["info"])


def test_handle_with_the_weight_stream_switched_off_uploads_fp16():
    """SD_WSTREAM=0 (an A/B switch, read once per process under SD_TUNE): no conv streams, the palettized store still gives the
    de-palettized handle's bits."""
    env = dict(os.environ, SD_TUNE="1", SD_WSTREAM="0")
    code = ("import sys, json; sys.path[:0] = [%r, %r, %r]\n"
            "import test_palettize_gpu as t\n"
            "r = t.compare_handles(6)\n"
            "print('RESULT ' + json.dumps({k: r[k] for k in ('info', 'equal', 'used')}))\n") % (
        ROOT, os.path.join(ROOT, "ml-stable-diffusion_amd"), os.path.join(ROOT, "tests"))
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert p.returncode == 0 and line, p.stdout[-2000:] + p.stderr[-2000:]
    r = json.loads(line[0][len("RESULT "):])
    assert r["info"][0] >= 10 and r["info"][1] == 0 and r["info"][2] == 0
    assert all(r["equal"]) and len(r["equal"]) == 4
    assert r["used"][0] == r["used"][1]


# ---- pipeline ----
def test_pipeline_quantize_nbits_applies_the_palette_and_equals_the_depalettized_checkpoint():
    from test_pipeline_gpu import StubTextEncoder, StubTokenizer
    from oracle import vae_ref
    from python_hip_stable_diffusion import HipVaeDecoder, schedulers
    from python_hip_stable_diffusion.pipeline import HipStableDiffusionPipeline
    cfg = unet_ref.CONFIGS["mini"]
    sd16 = weights.make_state_dict(unet_ref.unet_param_shapes(cfg), seed=21, dtype=np.float16)
    vcfg = vae_ref.VAE_CONFIGS["mini"]
    vsd16 = weights.make_state_dict(vae_ref.vae_decoder_param_shapes(vcfg), seed=61, dtype=np.float16, gain=1.6)
    hw = cfg["sample_size"]
    store = hip_model.Weights(sd16)
    palettize.apply(store, nbits=6)
    depal = {k: (store.read(k).astype(np.float16) if store.palette_bits(k) else v) for k, v in sd16.items()}
    assert sum(1 for k in sd16 if store.palette_bits(k)) >= 4
    store.close()
    images, infos = [], []
    for w, q in ((sd16, None), (sd16, 6), (depal, None)):
        unet = HipModel(cfg, w, batch=2, attention_implementation="SPLIT_EINSUM", quantize_nbits=q)
        vae = HipVaeDecoder(vcfg, vsd16, batch=1, latent_height=hw, latent_width=hw)
        pipe = HipStableDiffusionPipeline(StubTextEncoder(cfg["cross_attention_dim"]), unet, vae, schedulers.DDIMScheduler(), StubTokenizer(),
                                          force_zeros_for_empty_prompt=False)
        out = pipe("a photo of an astronaut riding a horse", num_inference_steps=3, guidance_scale=7.5, seed=93)
        images.append(out.images.copy())
        infos.append(unet.palette_info())
        unet.close()
    plain, quant, host = images
    p = psnr.compute_psnr(quant, plain)
    print(f"mini pipeline, 6-bit palettes vs fp16: image PSNR {p:.1f} dB; palette info {infos[1]}")
    assert np.isfinite(p) and not np.array_equal(quant, plain)                  # the palette really is applied
    assert np.array_equal(quant, host)                                          # ... and is the de-palettized checkpoint, bit for bit
    assert infos[0] == (0, 0, 0) and infos[2] == (0, 0, 0) and infos[1][0] >= 4 and infos[1][1] >= 1
