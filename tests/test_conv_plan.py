"""CPU suite: the conv / GEMM planner (csrc/conv_plan.cpp) through sd_op_conv_plan, which needs no GPU.

tests/golden/conv_plans.json holds what the parent commit of the planner resolved for every distinct descriptor of three
workloads (its header says which and how it was recorded); the planner must reproduce every row exactly."""
import json
import os
import re

import pytest

from conftest import GOLDEN, ROOT
from python_hip_stable_diffusion import _lib

DESC = ["ksize", "stride", "up", "C0", "C1", "N", "B", "Ho", "Wo", "out_mode", "flags", "n_trans", "n_twins", "gnf_groups", "tile", "staging",
        "splitk", "copies"]


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "conv_plans.json")) as f:
        g = json.load(f)
    assert g["desc_fields"] == DESC
    return g


def _query(row):
    return _lib.conv_plan(**dict(zip(DESC, row[:len(DESC)])))


def test_planner_reproduces_every_launch_row_of_the_parent(golden):
    """launch rows: descriptor as launch_conv saw it (copies = the pre-tiled copies the handle held) -> tile, staging, resolved
    split-K, slab, workspace bytes.  The recorded rows of the three workloads, then the enumerated extras: none skipped."""
    assert len(golden["launch_rows"]) >= 100
    rows = golden["launch_rows"] + golden["extra_launch_rows"]
    n = len(DESC)
    bad = []
    for row in rows:
        p = _query(row)
        got = [p["tile"], p["staging"], p["splitk"], int(p["slab"]), p["workspace_bytes"]]
        if got != row[n:n + 5]:
            bad.append((row[:n], row[n:n + 5], got))
    assert not bad, f"{len(bad)} of {len(rows)} rows differ, first: {bad[:3]}"


def test_planner_names_the_copies_the_parent_allocated(golden):
    """build rows: descriptor as UNet::conv_w saw it (no copies yet) -> the wstream / wsgemm / bvgemm copies it allocated"""
    assert len(golden["build_rows"]) >= 100
    rows = golden["build_rows"] + golden["extra_build_rows"]
    n = len(DESC)
    bad = []
    for row in rows:
        got = [int(c) for c in _query(row)["copies"]]
        if got != row[n:n + 3]:
            bad.append((row[:n], row[n:n + 3], got))
    assert not bad, f"{len(bad)} of {len(rows)} rows differ, first: {bad[:3]}"


def test_golden_covers_every_kernel_family(golden):
    n = len(DESC)
    rows = golden["launch_rows"]
    tiles = {r[n] for r in rows}
    assert tiles >= {1, 2, 3, 4, 7, 9, 10, 11, 12, 13}, sorted(tiles)
    assert any(r[n + 2] > 1 and r[0] == 1 and r[n] in (1, 2, 3, 4) for r in rows), "no split-K 1x1 row"
    assert any(r[n + 2] > 1 and r[0] == 3 and r[n] in (1, 2, 3, 4, 7) for r in rows), "no split-K 3x3 row"
    assert any(r[DESC.index("flags")] & 8 for r in rows), "no row with GroupNorm statistics requested"
    assert any(any(r[n:n + 3]) for r in golden["build_rows"]), "no row with a pre-tiled copy"


def _tuned_rows():
    rows = []
    for line in open(os.path.join(ROOT, "ml-stable-diffusion_amd", "csrc", "tuned_convs.inc")):
        if line.startswith("{"):
            rows.append([int(x) for x in re.findall(r"-?\d+", line.split("}")[0])])
    return rows


def _q(**kw):
    base = dict(ksize=1, stride=1, up=1, C0=320, C1=0, N=320, B=2, Ho=16, Wo=16, flags=16)
    base.update(kw)
    return _lib.conv_plan(**base)


def _plan(**kw):   # the plan alone (the copies a handle with these pins would hold are another question)
    p = _q(**kw)
    del p["copies"]
    return p


def test_pins_win_over_the_table_and_the_library_rules():
    # a plain 1x1 shape of the table (kind 0, tiled kernel, M a multiple of 256 so that it can be asked as B = 1, Ho x 16)
    row = next(r for r in _tuned_rows() if r[0] == 0 and r[1] == 1 and r[2] == 1 and r[3] == 1 and r[7] in (1, 2, 3, 4) and r[6] % 256 == 0 and
               r[6] > 2048 and r[4] < 640)   # (M > 2048, K < 640: none of the kernels with rules of their own takes it)
    kind, ks, st, up, ctot, n, m, tile, staging, splitk = row
    shape = dict(C0=ctot, N=n, B=1, Ho=m // 16, Wo=16)
    free = _q(**shape)
    assert (free["tile"], free["staging"]) == (tile, staging)
    other = 1 if tile != 1 else 2
    p = _q(tile=other, **shape)
    assert (p["tile"], p["staging"]) == (other, 0)            # the pinned tile, and with it the caller's staging (none)
    p = _q(staging=2 if staging != 2 else 3, **shape)
    assert p["staging"] == (2 if staging != 2 else 3)         # a pinned staging alone also switches the table off
    p = _q(splitk=2, **shape)
    assert p["splitk"] == 2 and p["slab"] and p["workspace_bytes"] == 2 * m * n * 4
    # the library's own rule for plan tile 12 (1280 -> 1280 at M = 512) gives way to any pin
    sm = dict(C0=1280, N=1280, B=2, Ho=16, Wo=16)
    assert _q(**sm)["tile"] == 12
    p = _q(splitk=1, **sm)
    assert p["tile"] in (1, 2, 3, 4) and p["splitk"] == 1 and not p["slab"]
    assert _q(tile=12, staging=2, **sm) == dict(tile=12, staging=2, splitk=1, slab=False, workspace_bytes=0, copies=(False, False, False),
                                               kernel="smgemm bm64")
    # split-K never has empty splits: 20 K steps pinned to 8 splits run 7 of 3 steps
    p = _q(splitk=8, **sm)
    assert p["splitk"] == 7 and p["workspace_bytes"] == 7 * 512 * 1280 * 4


def test_a_tile_the_shape_does_not_admit_falls_back_as_unpinned():
    free = _q()
    assert free["tile"] in (1, 2, 3, 4)
    for code in (5, 6, 7, 8, 9, 14, -3):     # removed codes, the 3x3 halo kernel, the weight stream without its copy, nonsense
        assert _plan(tile=code, copies=0) == _plan(copies=0), code
    # 3x3 at the 8x8 level: tile 9 only with the pre-tiled copy, else the halo kernel whatever was pinned
    c3 = dict(ksize=3, C0=1280, N=1280, B=2, Ho=8, Wo=8)
    assert _q(**c3)["tile"] == 9 and _q(**c3)["copies"] == (True, False, False)
    assert _plan(tile=9, copies=0, **c3) == _plan(copies=0, **c3)
    assert _q(copies=0, **c3)["tile"] == 7
    assert _q(tile=9, copies=1, **c3)["tile"] == 9
    # GEGLU pairs need 64 n-columns per wave: tiles 2 / 3 are not admitted, 1 / 4 are
    g = dict(C0=320, N=2560, B=1, Ho=8, Wo=16, out_mode=2)
    assert _plan(tile=2, **g) == _plan(tile=5, **g) and _plan(tile=3, **g) == _plan(tile=5, **g)
    assert _q(tile=1, **g)["tile"] == 1 and _q(tile=4, **g)["tile"] == 4
    # the LayerNorm fold and the fused q|k|v cannot split
    assert _q(splitk=4, flags=16 | 1)["splitk"] == 1
    # a forced plan tile 10 / 11 without its pre-tiled weights is an error, not a fall-back
    with pytest.raises(ValueError):
        _q(tile=10, **g)
    with pytest.raises(ValueError):
        _q(tile=11, copies=0, C0=1280, N=1280, B=2, Ho=64, Wo=64)
    # off the MFMA path
    assert _q(C0=4)["tile"] == -1


# ---- what launches: conv_plan()["kernel"] (sd_op_conv_plan_kernel).  The expected lines below restate the decode rules of the plan
# codes (the comment over decode_plan in csrc/conv_plan.cpp) in Python; nothing here is recorded from the library. ----
TILE = {1: (128, 128), 2: (128, 64), 3: (64, 64), 4: (64, 128)}
CODES = (0, 1, 2, 3, 4, 5, 6, 7, 8, 12, 13)
LDS = 160 * 1024


def fits(bm, bn, n, kgroups=1):
    """kgroups rings of n stages of the tile's A and B rows (64 halves each) and [2][bn] floats fit the 160 KB of LDS"""
    return kgroups * n * (bm + bn) * 64 * 2 + 2 * bn * 4 <= LDS


def tiled_kernel(tile, code, nk, lnf=False, half_t=False, pipe_ok=True):
    """tiles 1-4: nk = K steps per resolved split; lnf: LayerNorm fold; half_t: token-transposed output (kOutHalfT)"""
    bm, bn = TILE[tile]

    def igemm(stages, tail=""):
        return f"igemm {bm}x{bn} ring{stages}{tail}"

    def deepest(*depths):
        return igemm(next(n for n in depths if fits(bm, bn, n)))

    if lnf and code == 1:
        code = 0
    if code == 1:
        return igemm(2, " regs")
    if half_t and not lnf:
        return igemm(3 if code >= 2 else 2)
    if code in (12, 13):
        if not lnf and nk >= 4:
            if code == 13 and fits(bm, bn, 4, 2):
                return igemm(4, " kg2")
            if fits(bm, bn, 3, 2):
                return igemm(3, " kg2")
        code -= 10
    if code == 8 and pipe_ok:
        return f"gemm_pipe {bm}x{bn} ring2"
    if code in (6, 7) and pipe_ok:
        return f"gemm_pipe {bm}x{bn} ring{4 if code == 7 and fits(bm, bn, 4) else 3}"
    if code >= 6:
        code = 3
    if code == 5:
        return deepest(8, 6, 4, 3)
    if code == 4:
        return deepest(6, 4, 3)
    if code == 3:
        return deepest(4, 3)
    return igemm(3 if code == 2 else 2)


def halo_kernel(code):
    return "halo_ks ring%d" % (8 if code >= 5 else {4: 6, 3: 4, 2: 3}.get(code, 2))


def halo_gnl_lds_bytes(d, ctot):
    """the halo kernel's LDS with GroupNorm in its loader: two 184-row halo buffers and d stages of 64 weight rows (64 halves each), the
    [3][ctot] fp16 GroupNorm table rounded up to 16 B behind them - or the epilogue's buffers if those are larger"""
    k_loop = (2 * 184 * 64 + d * 64 * 64) * 2 + (6 * ctot + 15) // 16 * 16
    return max(k_loop, 32 * 1024 + 128 * (64 + 8) * 2 + 64 * 4)


# a 1x1 GEMM of 20 K steps (K = 1280) that gemm_pipe_ok admits; n_trans = 2560 is a tile boundary of every tile
GEMM = dict(C0=1280, N=3840, B=2, Ho=16, Wo=16)
MODES = {  # name -> (query arguments, LayerNorm fold, token-transposed output, can split)
    "plain": (dict(flags=16), False, False, True),
    "lnf": (dict(flags=16 | 1), True, False, False),
    "qkv": (dict(flags=16 | 1, n_trans=2560), True, False, False),      # fused q|k|v as the UNet runs it: behind the LayerNorm fold
    "qkv_plain": (dict(flags=16, n_trans=2560), False, False, False),   # the same epilogue without the fold: the plain ring rules
    "half_t": (dict(flags=16, out_mode=1), False, True, False),
}


@pytest.fixture(scope="module")
def tiled_lines():
    """kernel line of every tile 1-4 x code x mode x {unsplit, pinned to 8 splits}; checked against the rules as it is collected"""
    lines = {}
    for mode, (args, lnf, half_t, can_split) in MODES.items():
        for tile in TILE:
            for code in CODES:
                for pin in (1, 8):
                    p = _q(tile=tile, staging=code, splitk=pin, **GEMM, **args)
                    assert (p["tile"], p["staging"]) == (tile, code)
                    # 20 K steps pinned to 8 splits run 7 splits of 3 steps; the fold, the fused q|k|v and kOutHalfT cannot split
                    want_split = 7 if pin == 8 and can_split and not half_t else 1
                    if mode != "half_t":
                        assert p["splitk"] == want_split, (mode, tile, code, pin, p)
                    nk = -(-20 // p["splitk"])
                    assert p["kernel"] == tiled_kernel(tile, code, nk, lnf, half_t), (mode, tile, code, pin, p)
                    lines[mode, tile, code, pin] = p["kernel"]
    return lines


def test_kernel_line_of_every_tile_code_and_epilogue(tiled_lines):
    assert len(tiled_lines) == len(MODES) * 4 * len(CODES) * 2
    assert tiled_lines["plain", 3, 13, 1] == "igemm 64x64 ring4 kg2"
    assert tiled_lines["plain", 3, 13, 8] == "igemm 64x64 ring4"          # 3 K steps per split: no second K group
    assert tiled_lines["plain", 1, 1, 1] == "igemm 128x128 ring2 regs"
    assert tiled_lines["plain", 2, 6, 1] == "gemm_pipe 128x64 ring3"
    assert tiled_lines["lnf", 1, 1, 1] == "igemm 128x128 ring2"            # the fold has no register staging
    assert tiled_lines["lnf", 3, 13, 1] == "igemm 64x64 ring4"             # nor a second K group
    assert tiled_lines["qkv", 4, 8, 1] == "gemm_pipe 64x128 ring2"
    assert tiled_lines["half_t", 3, 7, 1] == "igemm 64x64 ring3"           # kOutHalfT: never the pipelined kernel


def test_ring_depths_the_lds_admits(tiled_lines):
    """the facts that follow from fits(): 128x128 stops at 4 stages and one K group; 128x64 / 64x128 reach 6 stages and two K groups of 3;
    64x64 reaches 8 stages and two K groups of 4"""
    def of(tile):
        return {v for (m, t, c, s), v in tiled_lines.items() if t == tile}
    big = of(1)
    assert not any("ring6" in k or "ring8" in k or "kg2" in k for k in big) and "igemm 128x128 ring4" in big
    for tile in (2, 4):
        bm, bn = TILE[tile]
        got = of(tile)
        assert f"igemm {bm}x{bn} ring6" in got and f"igemm {bm}x{bn} ring3 kg2" in got
        assert not any("ring8" in k or "ring4 kg2" in k for k in got)
    small = of(3)
    assert "igemm 64x64 ring8" in small and "igemm 64x64 ring4 kg2" in small and "igemm 64x64 ring3 kg2" in small
    # the pipelined kernel: 2 / 3 / 4 stages on every tile, nothing deeper
    for tile, (bm, bn) in TILE.items():
        assert {k for k in of(tile) if k.startswith("gemm_pipe")} == {f"gemm_pipe {bm}x{bn} ring{n}" for n in (2, 3, 4)}


def test_kernel_line_3x3_never_the_pipelined_kernel():
    """a 3x3 conv pinned to a tile: codes 6-8 name a kernel that takes 1x1 GEMMs only, so they run igemm_kernel's 4-stage ring (it fits
    every tile; where it did not, 3 stages)"""
    for tile, (bm, bn) in TILE.items():
        for code in CODES:
            p = _q(ksize=3, C0=128, N=128, B=2, Ho=16, Wo=16, tile=tile, staging=code, splitk=1)
            assert p["kernel"] == tiled_kernel(tile, code, 18, pipe_ok=False), (tile, code, p)
            if code in (6, 7, 8):
                assert p["kernel"] == f"igemm {bm}x{bn} ring{4 if fits(bm, bn, 4) else 3}"


def test_kernel_line_halo_conv():
    c3 = dict(ksize=3, C0=320, N=320, B=2, Ho=16, Wo=16)
    for code in (0, 2, 3, 4, 5):
        p = _q(tile=7, staging=code, **c3)
        assert (p["tile"], p["staging"]) == (7, code) and p["kernel"] == halo_kernel(code), (code, p)
    assert [halo_kernel(c) for c in (0, 2, 3, 4, 5)] == ["halo_ks ring2", "halo_ks ring3", "halo_ks ring4", "halo_ks ring6", "halo_ks ring8"]


def test_kernel_line_halo_conv_with_groupnorm_loader():
    """GroupNorm in the loader: 4 stages from code 3 where halo_gnl_lds_bytes(4, Ctot) fits 160 KB, else 3.  The planner admits
    Ctot <= 2048 there, and the 4-stage form then needs at most 92 160 B: no admitted Ctot exceeds the cap, so the fall-back to 3 stages by
    size cannot be reached through the query (asserted below from the formula); Ctot = 2048 stands in for it and reads ring4."""
    assert all(halo_gnl_lds_bytes(4, c) <= LDS for c in range(64, 2049, 64)) and halo_gnl_lds_bytes(4, 2048) == 92160
    for ctot in (320, 2048):
        g = dict(ksize=3, C0=ctot, N=320, B=2, Ho=16, Wo=16, gnf_groups=32)
        assert _q(**g)["kernel"] == "halo_ks ring4"                  # the planner's own code for it is 3
        assert _q(staging=3, **g)["kernel"] == "halo_ks ring4"
        assert _q(staging=2, **g)["kernel"] == "halo_ks ring3"
        p = _q(staging=5, **g)                                       # any other code: the planner makes it 3
        assert (p["tile"], p["staging"], p["kernel"]) == (7, 3, "halo_ks ring4")


def test_kernel_line_groupnorm_folded_1x1():
    g = dict(C0=320, N=320, B=2, Ho=64, Wo=64, gnf_groups=32)   # the planner forces tile 3 and code 6 / 7 / 8
    for code, stages in ((6, 3), (7, 4), (8, 2), (2, 3), (13, 3)):   # any other code becomes 6
        p = _q(staging=code, **g)
        assert (p["tile"], p["kernel"]) == (3, f"gemm_pipe 64x64 ring{stages}"), (code, p)
    p = _q(**g)                                                      # unpinned: the table's code for the shape if it is one of the three
    assert p["tile"] == 3 and p["kernel"] == "gemm_pipe 64x64 ring%d" % {6: 3, 7: 4, 8: 2}[p["staging"]]


def test_kernel_line_of_the_kernels_with_their_own_codes():
    c3 = dict(ksize=3, C0=1280, N=1280, B=2, Ho=8, Wo=8)
    for code, waves in ((0, 8), (4, 4), (8, 8)):
        assert _q(tile=9, staging=code, copies=1, **c3)["kernel"] == f"wstream waves{waves}"
    # tile 11: codes 1-6 are the variant; 0 is bvgemm.hip's own choice - N % 256 == 0, plain epilogue, M < 16384 rows: variant 1;
    # N = 320 (64-column tiles only) at M >= 4096: variant 6
    bv = dict(C0=1280, N=1280, B=2, Ho=64, Wo=64, tile=11, copies=4)
    assert _q(**bv)["kernel"] == "bvgemm v1"
    for code in range(1, 7):
        assert _q(staging=code, **bv)["kernel"] == f"bvgemm v{code}"
    assert _q(C0=1280, N=320, B=2, Ho=64, Wo=64, tile=11, copies=4)["kernel"] == "bvgemm v6"
    # tile 12: 32-row tiles up to M = 1024, else 64; 1 / 2 force 32 / 64
    sm = dict(C0=1280, N=1280, B=2, Ho=16, Wo=16, tile=12)
    assert [_q(staging=c, **sm)["kernel"] for c in (0, 1, 2)] == ["smgemm bm32", "smgemm bm32", "smgemm bm64"]
    assert _q(C0=640, N=640, B=2, Ho=32, Wo=32, tile=12)["kernel"] == "smgemm bm64"
    # tile 13: 128-row tiles where M / 128 x N / 160 tiles are at most 256, else 256; 1 / 2 force 128 / 256
    sg = dict(C0=1280, N=10240, B=2, Ho=16, Wo=16, out_mode=2, tile=13)
    assert [_q(staging=c, **sg)["kernel"] for c in (0, 1, 2)] == ["smgeglu bm128", "smgeglu bm128", "smgeglu bm256"]
    assert _q(C0=640, N=5120, B=2, Ho=32, Wo=32, out_mode=2, tile=13)["kernel"] == "smgeglu bm256"
    assert _q(C0=320, N=2560, B=2, Ho=64, Wo=64, out_mode=2, tile=10, copies=2)["kernel"] == "wsgemm"
    assert _q(C0=4)["kernel"] == "generic"


def _row_query(row):
    """sd_op_conv_plan arguments that ask for a table row's shape with the row's own codes pinned (B x Ho x Wo = M, as square as M allows)"""
    kind, ks, st, up, ctot, n, m, tile, staging, splitk = row
    B = 2 if m % 2 == 0 else 1
    hw = m // B
    ho = next(h for h in range(int(hw ** 0.5), 0, -1) if hw % h == 0)
    if tile == 9 and ks == 3:                    # the weight stream takes 8- and 16-pixel-wide images
        ho = 8
    q = dict(ksize=ks, stride=st, up=up, C0=ctot, N=n, B=B, Ho=ho, Wo=hw // ho, flags=16, tile=tile, staging=staging, splitk=splitk,
             copies=1 if tile == 9 else 0)
    if kind in (1, 3):
        q["flags"] |= 1
    if kind == 2:
        q["out_mode"] = 2
    if kind == 3:
        q["n_trans"] = n // 3 * 2
    return q


def test_kernel_line_of_every_row_of_the_table():
    """what the codes of tuned_convs.inc launch today, row by row: the row's (tile, staging, splitk) pinned on the row's shape"""
    rows = _tuned_rows()
    assert len(rows) >= 80
    seen = set()
    for row in rows:
        kind, ks, st, up, ctot, n, m, tile, staging, splitk = row
        p = _q(**_row_query(row))
        assert (p["tile"], p["staging"]) == (tile, staging), (row, p)
        if tile == 7:
            want = halo_kernel(staging)
        elif tile == 9:
            want = "wstream waves%d" % (4 if staging == 4 else 8)
        else:
            pipe_ok = ks == 1 and st == 1 and up == 1 and m * ctot * 2 < 2 ** 31 and n * ks * ks * ctot * 2 < 2 ** 31
            nk = -(-(ks * ks * ctot // 64) // p["splitk"])
            want = tiled_kernel(tile, staging, nk, lnf=kind in (1, 3), pipe_ok=pipe_ok)
        assert p["kernel"] == want, (row, p, want)
        seen.add(want)
    # the table reaches the pipelined kernel's 2- and 3-stage rings, igemm_kernel's 3- / 4-stage rings and both halo depths it names
    assert {"gemm_pipe 64x64 ring3", "gemm_pipe 64x64 ring2", "gemm_pipe 128x128 ring2", "halo_ks ring4", "halo_ks ring6", "wstream waves8"} <= seen, sorted(seen)
