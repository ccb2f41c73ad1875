"""CPU suite of the palettized GEGLU projection (plan tile 16, smgeglu.hip smgeglu_pal_kernel): the index bit stream against a numpy
restatement of the layout the header describes, a replay of the kernel's LDS-DMA issue order that checks every hand-counted vmcnt
immediate, the refusals of the operator entry (all made on the host, in front of any device work), and the planner's answers for the
fp16 descriptors of the shapes a handle meets."""
import numpy as np
import pytest

from python_hip_stable_diffusion import _lib

NBITS = (1, 2, 4, 6, 8)
GROUP = 8            # K64 stages per group of the stream


def strip_rows(n2):
    """include/sd_mi355x.h, sd_op_palette_pack_geglu: strip 2 U + v holds the checkpoint rows v * N2 / 2 + 16 U + r16."""
    s = np.arange(n2 // 16)
    return ((s & 1) * (n2 // 2) + 16 * (s >> 1))[:, None] + np.arange(16)[None, :]           # [strip][r16]


def pack_reference(idx, nbits):
    """... per strip as sd_op_palette_pack_gemm: lane l = 16 g + r16 owns, per stage s and sub-step kk, the indices of row r16 of the
    strip at columns 64 s + 32 kk + 8 g + e; its 128 indices of a group of 8 stages in the order (s, kk, e) are little-endian
    nbits-wide fields in nbits 16-byte words; word q at [strip][group][q][lane][16 B]; stages beyond K / 64 are zero fields."""
    n2, k = idx.shape
    groups = -(-(k // 64) // GROUP)
    padded = np.zeros((n2, groups * GROUP * 64), np.uint8)
    padded[:, :k] = idx
    rows = strip_rows(n2)
    lane = np.arange(64)
    f = np.arange(GROUP * 16)
    s, kk, e = f >> 4, (f >> 3) & 1, f & 7
    col = (64 * s + 32 * kk + e)[None, :] + 8 * (lane >> 4)[:, None]                          # [lane][field] inside a group
    fields = np.empty((n2 // 16, groups, 64, GROUP * 16), np.uint8)
    for strip in range(n2 // 16):
        for grp in range(groups):
            fields[strip, grp] = padded[rows[strip][lane & 15][:, None], grp * GROUP * 64 + col]
    bits = (fields[..., None] >> np.arange(nbits, dtype=np.uint8)) & 1                        # little-endian inside a field
    by = np.packbits(bits.reshape(n2 // 16, groups, 64, GROUP * 16 * nbits), axis=-1, bitorder="little")
    return by.reshape(n2 // 16, groups, 64, nbits, 16).transpose(0, 1, 3, 2, 4)


def unpack(stream, n2, k, nbits):
    """the inverse, written on its own: (indices the stream holds in checkpoint row order, the padding fields)"""
    strips, groups = stream.shape[:2]
    by = stream.transpose(0, 1, 3, 2, 4).reshape(strips, groups, 64, nbits * 16)
    bits = np.unpackbits(by, axis=-1, bitorder="little").reshape(strips, groups, 64, GROUP * 16, nbits)
    fields = (bits.astype(np.uint32) << np.arange(nbits, dtype=np.uint32)).sum(-1)
    out = np.full((n2, groups * GROUP * 64), 255, np.uint32)
    for strip in range(strips):
        value_or_gate, unit = strip & 1, strip >> 1
        for lane in range(64):
            row = value_or_gate * (n2 // 2) + 16 * unit + (lane & 15)
            for grp in range(groups):
                for st in range(GROUP):
                    for kk in range(2):
                        c0 = grp * GROUP * 64 + 64 * st + 32 * kk + 8 * (lane >> 4)
                        out[row, c0:c0 + 8] = fields[strip, grp, lane, (2 * st + kk) * 8:(2 * st + kk) * 8 + 8]
    return out[:, :k], out[:, k:]


@pytest.mark.parametrize("nbits", NBITS)
@pytest.mark.parametrize("n2,k", [(320, 64), (640, 192), (320, 576), (1280, 1280)])
def test_palette_pack_geglu_against_the_documented_layout(n2, k, nbits):
    rs = np.random.RandomState(n2 + k + nbits)
    idx = rs.randint(0, 1 << nbits, size=(n2, k)).astype(np.uint8)
    idx[0, 0], idx[-1, -1] = (1 << nbits) - 1, (1 << nbits) - 1                               # both ends carry all-ones fields
    got = _lib.palette_pack_geglu(idx, nbits)
    groups = -(-(k // 64) // GROUP)
    assert got.shape == (n2 // 16, groups, nbits, 64, 16) and got.dtype == np.uint8
    assert got.size == (n2 // 16) * groups * nbits * 1024                                     # the size formula
    want = pack_reference(idx, nbits)
    assert np.array_equal(got, want), f"{np.count_nonzero(got != want)} bytes differ"
    back, padding = unpack(got, n2, k, nbits)
    assert np.array_equal(back, idx)
    assert padding.size == n2 * (groups * GROUP * 64 - k) and not padding.any()
    # the same stream as the small-M GEMM's packer over the strips' rows: one packing rule
    assert np.array_equal(got, _lib.palette_pack_gemm(idx[strip_rows(n2).reshape(-1)], nbits))


def test_palette_pack_geglu_refusals():
    for bad_shape in ((48, 64), (64, 96)):
        with pytest.raises(ValueError):
            _lib.palette_pack_geglu(np.zeros(bad_shape, np.uint8), 4)
    with pytest.raises(ValueError):
        _lib.palette_pack_geglu(np.zeros((64, 64), np.uint8), 3)
    with pytest.raises(ValueError):
        _lib.palette_pack_geglu(np.zeros((64, 64, 1, 1), np.uint8), 4)


# ---- the K loop's hand-counted waits (smgeglu.hip, header comment of the palettized kernel) ----
NST = 3              # ring stages
HALF = 4             # stages per half-group of index words


def replay(nk, nbits, full, n_old):
    """One wave's LDS-DMA pieces in the kernel's issue order, with the immediates of its waits by the kernel's formula.  vmcnt(n)
    returns once all but the youngest n pieces have landed (they retire in order).  Checks, at every wait for a stage, that the
    immediate EQUALS the number of pieces younger than that stage's last piece - not more (the stage would not have landed), not
    fewer (the wait would drain newer stages) - and that LUT, gamma and every half-group of index words have landed where they are
    first read, that the transit buffer is re-filled only after it was read, and that a ring slot is re-filled only behind the wait
    that follows its stage.  n_old: the LUT / gamma pieces this wave brings (0-5, uneven over the waves)."""
    P = 2 if full else 1                       # activation pieces per stage: the first FULL = 6 waves bring two, the others one
    HQ = max(1, nbits // 2)                    # index words per half-group
    issued = []                                # tags, oldest first
    landed = 0                                 # pieces known to have landed

    def issue(tag, n):
        issued.extend([tag] * n)

    def wait(imm):
        nonlocal landed
        landed = max(landed, len(issued) - imm)

    def has_landed(tag):
        return tag in issued and max(i for i, t in enumerate(issued) if t == tag) < landed

    def younger(tag):
        return len(issued) - 1 - max(i for i, t in enumerate(issued) if t == tag)

    def wait_stage(s):
        imm = P * min(NST - 2, nk - 1 - s) + (HQ if s % HALF == 1 else 0)         # the kernel's wait_stage
        assert imm == younger(("stage", s)), (nk, nbits, full, s, imm, younger(("stage", s)))
        assert imm <= 63
        wait(imm)
        assert has_landed(("stage", s))

    transit, cur = None, None                  # half-group in the transit buffer / in registers
    passed = -1                                # newest stage whose wait (+ barrier) this wave has passed

    def issue_half(i):
        nonlocal transit
        assert transit is None or cur == transit, "the transit buffer is re-filled before it was read"
        issue(("half", i), HQ)
        transit = i

    def read_words(i):
        nonlocal cur
        assert transit == i and has_landed(("half", i)), (nk, nbits, full, i)
        cur = i

    def issue_stage(s):
        assert s < NST or passed >= s - NST + 1, "slot re-filled before the barrier behind its stage"
        issue(("stage", s), P)

    def decode(s):
        assert cur == s // HALF and has_landed("old"), (nk, nbits, full, s, cur)
        assert s < NST or passed >= s - NST + 1, "weight rows written into a slot before the barrier behind its last stage"

    issue("old", max(n_old, 1))                # (at least one tag so that the check below has something to look at)
    issue_half(0)
    for p in range(min(NST - 1, nk)):
        issue_stage(p)
    imm_a = P * min(NST - 1, nk)               # wait A
    assert imm_a == younger(("half", 0))
    wait(imm_a)
    assert has_landed("old") and has_landed(("half", 0))
    read_words(0)
    decode(0)
    wait_stage(0)
    passed = 0
    if nk > 1:
        issue_half(1)
    if NST - 1 < nk:
        issue_stage(NST - 1)
    for rel in range(nk):
        if rel + 1 < nk:
            if (rel + 1) % HALF == 0:
                read_words((rel + 1) // HALF)
            decode(rel + 1)
            wait_stage(rel + 1)
            passed = rel + 1
            if (rel + 1) % HALF == 0:
                issue_half((rel + 1) // HALF + 1)
            if rel + NST < nk:
                issue_stage(rel + NST)
    wait(0)                                    # the drain behind the loop
    assert landed == len(issued)


@pytest.mark.parametrize("nbits", NBITS)
def test_every_counted_wait_equals_the_pieces_younger_than_its_stage(nbits):
    for nk in range(1, 45):
        for full in (True, False):
            for n_old in (0, 1, 5):
                replay(nk, nbits, full, n_old)


def test_the_replay_notices_a_wrong_immediate():
    """the check has teeth: with a ring one stage deeper than the formula assumes, the immediates are wrong"""
    global NST
    NST = 4
    try:
        with pytest.raises(AssertionError):
            for nk in range(1, 45):
                replay(nk, 8, True, 1)
    finally:
        NST = 3


# ---- the operator's refusals ----
def _problem(M=256, C=64, N2=640, nbits=4):
    rs = np.random.RandomState(5)
    lut = rs.randn(1 << nbits).astype(np.float16)
    idx = rs.randint(0, 1 << nbits, size=(N2, C)).astype(np.uint8)
    x = rs.randn(M, C).astype(np.float16)
    return x, lut, idx


def test_refusals_need_no_gpu():
    """Validation precedes device work: every one of these is a ValueError on a box without a GPU (where a valid call is a
    RuntimeError: no HIP device)."""
    x, lut, idx = _problem()
    g, b = np.ones(64, np.float32), np.zeros(64, np.float32)
    with pytest.raises(ValueError, match="nbits"):
        _lib.geglu_palettized(x, lut[:8], idx % 8, 3)
    with pytest.raises(ValueError, match="bm"):
        _lib.geglu_palettized(x, lut, idx, 4, bm=64)
    with pytest.raises(ValueError, match="empty"):
        _lib.geglu_palettized(x[:0], lut, idx, 4)
    with pytest.raises(ValueError, match="go together"):
        _lib.geglu_palettized(x, lut, idx, 4, ln_weight=g)
    with pytest.raises(ValueError, match="go together"):
        _lib.geglu_palettized(x, lut, idx, 4, ln_bias=b)
    bad = idx.copy()
    bad[7, 9] = 16
    with pytest.raises(ValueError, match="index 16"):
        _lib.geglu_palettized(x, lut, bad, 4)
    with pytest.raises(ValueError, match="plan tile 16"):                          # N2 = 480: three tiles of 160 rows, 6 tiles in all
        _lib.geglu_palettized(*_problem(N2=480), 4)
    with pytest.raises(ValueError, match="plan tile 16"):                          # M = 200: ragged
        _lib.geglu_palettized(*_problem(M=200), 4)
    with pytest.raises(ValueError, match="plan tile 16"):                          # C = 32: off the MFMA path
        _lib.geglu_palettized(*_problem(C=32), 4)
    with pytest.raises(ValueError, match="plan tile 16"):                          # M = 128: one row of tiles
        _lib.geglu_palettized(*_problem(M=128), 4)
    with pytest.raises(ValueError, match="plan tile 16"):                          # C = 2624: more than the 2560 floats of gamma in LDS
        _lib.geglu_palettized(*_problem(C=2624), 4)
    with pytest.raises(ValueError, match="256 is not built"):                      # 256-row tiles: not built
        _lib.geglu_palettized(*_problem(M=512), 4, bm=256)
    # the order of the checks: nbits, bm, empty, the LayerNorm pair, the index range, the shape
    with pytest.raises(ValueError, match="nbits"):
        _lib.geglu_palettized(x[:0], lut[:8], idx % 8, 3, bm=64, ln_weight=g)
    with pytest.raises(ValueError, match="bm"):
        _lib.geglu_palettized(x[:0], lut, bad, 4, bm=64, ln_weight=g)
    with pytest.raises(ValueError, match="empty"):
        _lib.geglu_palettized(x[:0], lut, bad, 4, ln_weight=g)
    with pytest.raises(ValueError, match="go together"):
        _lib.geglu_palettized(*_problem(N2=480)[:2], bad[:480], 4, ln_weight=g)
    with pytest.raises(ValueError, match="index 16"):
        _lib.geglu_palettized(*_problem(N2=480)[:2], bad[:480], 4)


# (B, H, W, C, N2) -> plan tile and kernel line of the fp16 descriptor (LayerNorm fold + bias), and whether a handle streams it
FP16_PLANS = [
    ((2, 16, 16, 1280, 10240), 13, "smgeglu bm128", True),     # SD2.1-base at CFG batch 2, 16x16 level
    ((2, 32, 32, 640, 5120), 13, "smgeglu bm256", False),      # ... 32x32 level: 256-row tiles, which the palettized kernel does not have
    ((4, 16, 16, 640, 5120), 13, "smgeglu bm128", True),       # M = 1024: the handle test's projections
    ((2, 8, 8, 1280, 10240), None, None, False),               # M = 128: one row of tiles
    ((2, 64, 64, 320, 2560), None, None, False),               # M = 8192: wsgemm.hip's
]


@pytest.mark.parametrize("desc,tile,kernel,streams", FP16_PLANS)
def test_fp16_plans_are_unchanged_and_tile_16_takes_what_tile_13_runs_on_128_row_tiles(desc, tile, kernel, streams):
    """A palette never changes a plan of a handle without palettes: the planner's answers for the fp16 descriptors stay what they
    were and no answer is ever tile 16.  Where the answer is tile 13 on 128-row tiles the shape passes the host validation of the
    palettized entry with bm = 0 (on a box without a GPU the call then stops at the device: RuntimeError, not ValueError);
    everywhere else the entry refuses it - conv_plan_pal_geglu's rule, which reads the same plan."""
    B, H, W, c, n2 = desc
    for flags in (1 | 16, 16, 0):                                                  # fold + bias, plain + bias, plain
        p = _lib.conv_plan(1, 1, 1, c, 0, n2, B, H, W, out_mode=2, flags=flags)
        assert p["tile"] != 16 and "pal" not in p["kernel"], p
        if tile is None:
            assert p["tile"] != 13, p
        else:
            assert p["tile"] == tile and p["kernel"] == kernel and p["splitk"] == 1 and not p["slab"] and p["workspace_bytes"] == 0, p
    x, lut, idx = _problem(M=B * H * W, C=c, N2=n2)
    if streams:
        try:
            out, plan, _ = _lib.geglu_palettized(x, lut, idx, 4, ln_weight=np.ones(c, np.float32), ln_bias=np.zeros(c, np.float32))
        except RuntimeError:
            return
        assert plan == [16, 1, 1, 0]
    else:
        with pytest.raises(ValueError, match="plan tile 16"):
            _lib.geglu_palettized(x, lut, idx, 4)
