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
    assert _q(tile=12, staging=2, **sm) == dict(tile=12, staging=2, splitk=1, slab=False, workspace_bytes=0, copies=(False, False, False))
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
