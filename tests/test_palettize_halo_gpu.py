"""GPU suite: the palettized 3x3 halo conv (plan tile 25, conv3x3_halo_pal.hip) - tile 7's kernel with the weight fragments decoded from
an index stream and a LUT.  The gate everywhere is identity of bits with tile 7 on the fp16 weights lut[indices] at the same ring code
and split-K: no tolerance in this file.  Then handles built from a palettized store with the store's halo switch on, off, and from the
de-palettized weights, and the pipeline flag.

Shapes: tests/test_w8a8_halo_gpu.py's twelve, one per mechanism of the kernel at the smallest sizes that reach it."""
import re

import numpy as np
import pytest

from oracle import unet_ref, weights
from python_hip_stable_diffusion import HipModel, _lib, hip_model, palettize
from test_palettize_gpu import h16
from test_w8a8_halo_gpu import SHAPES, STEADY

pytestmark = pytest.mark.gpu

NBITS = (1, 2, 4, 6, 8)
RING = {0: 2, 2: 3, 3: 4, 4: 6, 5: 8}          # plan tile 7's ring code -> weight stages
UNEVEN = "split-K through the slabs, uneven, batch 3"
SPECIALS = [-1.5, np.float16(6e-8), -65504.0, 65504.0, -0.0, 0.0]   # a negative, a subnormal, the largest magnitudes, both zeros


def make_case(name, nbits=6):
    """random fp16 LUT with as many of SPECIALS as the palette has room for beside one random entry; every LUT entry occurs among the
    indices, 2^nbits - 1 included; random activations, bias, time embedding, residual (identity of bits is the gate: no structure)"""
    B, C0, C1, H, W, Cout, ups, splitk = SHAPES[name]
    rs = np.random.RandomState(25000 + 16 * list(SHAPES).index(name) + nbits)
    ctot, n = C0 + C1, 1 << nbits
    lut = h16(rs.randn(n) * 0.05)
    k = min(len(SPECIALS), n - 1)
    lut[rs.choice(n, k, replace=False)] = np.array(SPECIALS[:k], np.float16)
    indices = rs.randint(0, n, size=(Cout, ctot, 3, 3)).astype(np.uint8)
    indices.reshape(-1)[rs.choice(indices.size, n, replace=False)] = np.arange(n, dtype=np.uint8)
    assert set(np.unique(indices)) == set(range(n))
    xs = h16(rs.randn(B, ctot, H, W))
    up = 2 if ups else 1
    return dict(x=xs[:, :C0].copy(), x1=xs[:, C0:].copy() if C1 else None, lut=lut, indices=indices, nbits=nbits,
                bias=(0.1 * rs.randn(Cout)).astype(np.float32), temb=(0.1 * rs.randn(B, Cout)).astype(np.float32),
                res=h16(rs.randn(B, Cout, H * up, W * up)), ups=ups, splitk=splitk, shape=(B, Cout, H * up, W * up))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def run_op(c, staging=3, plain=False):
    """tile 25 on case c (plain: no bias, no time embedding, no residual) into a prefilled buffer with a guard behind it; the plan; a
    second run with iters=3 that must agree; returns the output and tile 7's on lut[indices] at the same staging and splitk"""
    n = int(np.prod(c["shape"]))
    guard = 4 * c["shape"][3] * c["shape"][1]
    buf = np.full(n + guard, np.float16(-7.5), np.float16)
    kw = dict(x1=c["x1"], upsample=c["ups"], splitk=c["splitk"])
    if not plain:
        kw.update(bias=c["bias"], temb=c["temb"], res=c["res"])
    out, plan, _ = _lib.conv2d_palettized_halo(c["x"], c["lut"], c["indices"], c["nbits"], staging=staging, out=buf, **kw)
    out = out.copy()
    assert np.array_equal(bits(buf[n:]), bits(np.full(guard, np.float16(-7.5)))), "the guard behind the output was written"
    nch = c["indices"].shape[1] // 64
    splits = -(-nch // -(-nch // c["splitk"]))
    assert plan == [25, staging, splits, int(splits > 1)], plan
    again, plan2, _ = _lib.conv2d_palettized_halo(c["x"], c["lut"], c["indices"], c["nbits"], staging=staging, iters=3, **kw)
    assert plan2 == plan and np.array_equal(bits(out), bits(again)), "two runs differ"
    w = h16(c["lut"][c["indices"]])
    assert np.array_equal(bits(w), bits(c["lut"])[c["indices"]])                  # the fp16 bit patterns the LUT holds (-0, the subnormal)
    want, _, plan7, _ = _lib.conv2d_ex(c["x"], w, x1=c["x1"], upsample=c["ups"], tile=7 + 10 * staging, splitk=c["splitk"],
                                       **({} if plain else dict(bias=c["bias"], temb=c["temb"], res=c["res"])))
    assert plan7 == [7, staging, splits, int(splits > 1)], plan7
    return out, want


def assert_identical(out, want, what):
    assert np.array_equal(bits(out), bits(want)), f"{what}: {np.count_nonzero(bits(out) != bits(want))} of {out.size} elements differ from tile 7"


# ---- operator ----
@pytest.mark.parametrize("name", list(SHAPES))
def test_operator_is_bit_identical_to_tile_7_on_the_depalettized_weights(name):
    c = make_case(name)
    assert_identical(*run_op(c), name)
    assert_identical(*run_op(c, plain=True), name + ", plain epilogue")


@pytest.mark.parametrize("nbits", NBITS)
@pytest.mark.parametrize("name", [STEADY, UNEVEN])
def test_every_index_width(name, nbits):
    assert_identical(*run_op(make_case(name, nbits)), f"{name}, {nbits} bits")


@pytest.mark.parametrize("staging", list(RING))
def test_every_ring_depth(staging):
    c = make_case(STEADY)
    assert _lib.conv_plan(3, 1, 1, 192, 0, 64, 2, 8, 16, tile=25, staging=staging, splitk=1)["kernel"] == f"halo_pal ring{RING[staging]}"
    assert_identical(*run_op(c, staging=staging), f"ring code {staging}")


def test_the_librarys_split_k_rule_runs_too():
    c = dict(make_case(UNEVEN), splitk=0)
    want = _lib.conv_plan(3, 1, 1, 320, 0, 64, 3, 8, 16, flags=2 | 4 | 16, tile=7, staging=3)
    out, plan, _ = _lib.conv2d_palettized_halo(c["x"], c["lut"], c["indices"], 6, bias=c["bias"], temb=c["temb"], res=c["res"], staging=3, splitk=0)
    assert plan == [25, 3, want["splitk"], int(want["slab"])]
    ref = _lib.conv2d_ex(c["x"], h16(c["lut"][c["indices"]]), bias=c["bias"], temb=c["temb"], res=c["res"], tile=37, splitk=0)[0]
    assert_identical(out, ref, "library split-K")


def test_a_valid_call_right_after_each_refused_one():
    c = make_case("first + last chunk")                                          # 128 -> 64 channels on 8 x 16
    good = lambda: _lib.conv2d_palettized_halo(c["x"], c["lut"], c["indices"], 6, bias=c["bias"])[0]   # noqa: E731
    first = good()
    bad_idx = c["indices"].copy()
    bad_idx[3, 70, 2, 0] = 64                                                    # >= 2^6
    refused = [dict(nbits=3), dict(staging=1), dict(staging=6), dict(splitk=-1),
               dict(x=c["x"][:, :96], indices=c["indices"][:, :96]),             # 96 input channels: off the 64-channel chunks
               dict(x=c["x"][:, :, :4]),                                         # a 4-row image
               dict(indices=np.concatenate([c["indices"], c["indices"][:2]])),   # 66 output channels
               dict(indices=bad_idx)]
    for kw in refused:
        a = dict(x=c["x"], indices=c["indices"], nbits=6, staging=3, splitk=0)
        a.update(kw)
        with pytest.raises(ValueError):
            _lib.conv2d_palettized_halo(a["x"], c["lut"], a["indices"], a["nbits"], staging=a["staging"], splitk=a["splitk"])
        assert np.array_equal(bits(good()), bits(first)), kw


# ---- handles ----
# a UNet whose fp16 plan holds single-source and two-source 3x3 halo convs and an upsampler: 64 channels at 32x32, 128 at 16x16
CFG = unet_ref.make_config(sample_size=32, block_out_channels=(64, 128), down_block_types=(unet_ref.DN, unet_ref.CA),
                           up_block_types=(unet_ref.CAUP, unet_ref.UP), layers_per_block=1, attention_head_dim=(2, 4), cross_attention_dim=48)
RECIPES = {"6 bits": 6, "mixed 2 / 8 / 16": (2, 8, 16)}


def inputs():
    hw = CFG["sample_size"]
    return dict(sample=weights.seeded_normal((2, 4, hw, hw), 1).astype(np.float16), timestep=np.array([981, 981], np.float16),
                encoder_hidden_states=weights.seeded_normal((2, CFG["cross_attention_dim"], 1, 77), 2).astype(np.float16))


def conv_labels(labels):
    """{layer: (the label's weight mark, the library's fp16 plan tile for the label's shape key, Cout, Ctot)} of the 3x3 conv labels"""
    r = {}
    for lab in labels:
        m = re.search(r"^conv3x3(\S*) (\d+)->(\d+) @(\d+)x(\d+) M=\d+ K=\d+ (\S+) #0,3,(\d+),(\d+),(\d+),", lab)
        if m:
            mark, cin, cout, ho, wo, name, stride, up, ctot = m.groups()
            tile = _lib.conv_plan(3, int(stride), int(up), int(ctot), 0, int(cout), 2, int(ho), int(wo), flags=16)["tile"]
            r[name] = (mark, tile, int(cout), int(ctot))
    return r


def palettized_store(sd16, recipe):
    store = hip_model.Weights(sd16)
    modules = palettize.palettizable(store, min_size=1000)
    assert len(modules) >= 10
    palettize.apply(store, recipe={m: (recipe if isinstance(recipe, int) else recipe[i % len(recipe)]) for i, m in enumerate(modules)})
    return store


def describe(model):
    """what the tests compare of a handle beside its outputs"""
    return dict(info=model.palette_info(), used=model.arena_used_bytes, labels=[lab for lab, _, _ in model.profile(1)])


@pytest.fixture(scope="module", params=list(RECIPES))
def handles(request):
    recipe = RECIPES[request.param]
    sd16 = weights.make_state_dict(unet_ref.unet_param_shapes(CFG), seed=37, dtype=np.float16)
    never = palettized_store(sd16, recipe)                                       # a store that never sees the switch
    pal = palettized_store(sd16, recipe)
    plain = hip_model.Weights({k: (pal.read(k).astype(np.float16) if k.endswith(".weight") and pal.palette_bits(k) else v) for k, v in sd16.items()})
    r = {"outs": {}, "pal_bits": {k[:-len(".weight")]: pal.palette_bits(k) for k in pal.shapes() if k.endswith(".weight")}}
    inp = inputs()
    for use_graph in (False, True):
        built = {"on": HipModel(CFG, pal, batch=2, use_graph=use_graph, palette_halo=True),
                 "off": HipModel(CFG, pal, batch=2, use_graph=use_graph),         # the same store, after the switch went back off
                 "plain": HipModel(CFG, plain, batch=2, use_graph=use_graph),
                 "never": HipModel(CFG, never, batch=2, use_graph=use_graph)}
        for key, m in built.items():
            r["outs"][key, use_graph] = [m(**inp)["noise_pred"].copy() for _ in range(2)]   # graph: the second call is a replay
            r[key] = describe(m)
        if use_graph:                                                            # reload of a streamed conv: refused, nothing changes
            on = built["on"]
            streamed = sorted(n for n, (mark, tile, _, _) in conv_labels(r["on"]["labels"]).items() if "+pal" in mark and tile == 7)
            r["reload_refused"] = False
            try:
                on.reload_weights(plain, [streamed[0] + ".weight"])
            except NotImplementedError:
                r["reload_refused"] = True
            r["after_reload"] = on(**inp)["noise_pred"].copy()
        for m in built.values():
            m.close()
    for s in (never, pal, plain):
        s.close()
    return r


def test_the_fp16_plan_has_every_kind_of_halo_conv(handles):
    convs = conv_labels(handles["plain"]["labels"])
    halo = {n for n, (_, tile, _, _) in convs.items() if tile == 7}
    labels = {n: lab for lab in handles["plain"]["labels"] for n in halo if f" {n} " in lab}
    assert len(halo) >= 4, halo
    assert any(re.search(r"#0,3,1,2,", lab) for lab in labels.values()), "no upsampling halo conv"
    assert any("up_blocks" in n and n.endswith("conv1") and convs[n][3] > convs[n][2] for n in halo), "no two-source halo conv"
    assert any(n.endswith("conv2") for n in halo) and any(n.startswith("down_blocks") and n.endswith("conv1") for n in halo)


def test_all_three_handles_give_identical_bits(handles):
    first = handles["outs"]["plain", False][0]
    assert np.isfinite(first).all()
    for key, outs in handles["outs"].items():
        for a in outs:
            assert np.array_equal(bits(a), bits(first)), key


def test_switch_on_streams_exactly_the_palettized_tile_7_convs(handles):
    on, off = handles["on"], handles["off"]
    plain = conv_labels(handles["plain"]["labels"])
    want = {n for n, (_, tile, _, _) in plain.items() if tile == 7 and handles["pal_bits"].get(n, 0)}
    got = {n for n, (mark, tile, _, _) in conv_labels(on["labels"]).items() if "+pal" in mark and tile == 7}
    assert got == want and len(want) >= 3
    for n in want:                                                               # the label carries the tensor's width
        assert conv_labels(on["labels"])[n][0] == f"+pal{handles['pal_bits'][n]}"
    assert not {n for n, (mark, tile, _, _) in conv_labels(off["labels"]).items() if "+pal" in mark and tile == 7}
    assert on["info"][0] == off["info"][0] and on["info"][1] - off["info"][1] == len(want)
    # bytes: every such conv dropped its fp16 matrix [Cout][9][Ctot] - or, where the flag-off handle ran an upsampler as plan tile 21,
    # the folded matrix [4][Cout][4][Cin] it held in its place - and holds the stream and the LUT instead
    off_labels = {n: lab for lab in off["labels"] for n in want if f" {n} " in lab}
    held = sum(2 * 16 * plain[n][2] * plain[n][3] if "+subpix" in off_labels[n] else 2 * plain[n][2] * 9 * plain[n][3] for n in want)
    grown = on["info"][2] - off["info"][2]
    assert grown == sum(-(-plain[n][2] // 64) * 64 * 9 * plain[n][3] * handles["pal_bits"][n] // 8 + 512 for n in want)
    assert abs((off["used"] - on["used"]) - (held - grown)) <= 256 * len(want), (off["used"], on["used"], held, grown)
    assert on["used"] < off["used"]


def test_switch_off_is_a_store_that_never_saw_it(handles):
    off, never = handles["off"], handles["never"]
    assert off["info"] == never["info"] and off["used"] == never["used"] and off["labels"] == never["labels"]
    assert handles["plain"]["info"] == (0, 0, 0)


def test_reload_of_a_streamed_conv_is_refused_and_changes_nothing(handles):
    assert handles["reload_refused"]
    assert np.array_equal(bits(handles["after_reload"]), bits(handles["outs"]["on", True][0]))


# ---- pipeline ----
def test_pipeline_palette_halo_produces_the_image_of_quantize_nbits():
    from test_pipeline_gpu import StubTextEncoder, StubTokenizer
    from oracle import vae_ref
    from python_hip_stable_diffusion import HipVaeDecoder, schedulers
    from python_hip_stable_diffusion.pipeline import HipStableDiffusionPipeline
    cfg = unet_ref.CONFIGS["mini"]
    sd16 = weights.make_state_dict(unet_ref.unet_param_shapes(cfg), seed=21, dtype=np.float16)
    vcfg = vae_ref.VAE_CONFIGS["mini"]
    vsd16 = weights.make_state_dict(vae_ref.vae_decoder_param_shapes(vcfg), seed=61, dtype=np.float16, gain=1.6)
    hw = cfg["sample_size"]
    images, infos = [], []
    for halo in (False, True):
        unet = HipModel(cfg, sd16, batch=2, attention_implementation="SPLIT_EINSUM", quantize_nbits=6, palette_halo=halo)
        vae = HipVaeDecoder(vcfg, vsd16, batch=1, latent_height=hw, latent_width=hw)
        pipe = HipStableDiffusionPipeline(StubTextEncoder(cfg["cross_attention_dim"]), unet, vae, schedulers.DDIMScheduler(), StubTokenizer(),
                                          force_zeros_for_empty_prompt=False)
        images.append(pipe("a photo of an astronaut riding a horse", num_inference_steps=3, guidance_scale=7.5, seed=93).images.copy())
        infos.append(unet.palette_info())
        unet.close()
    assert np.array_equal(images[0], images[1])
    assert infos[1][0] == infos[0][0] and infos[1][1] >= infos[0][1]
    print(f"mini pipeline, 6 bits: palette info without / with palette_halo {infos}")
