"""GPU suite: sd_op_conv_plan reports what launch_conv runs.  For each shape the conv runs once on the library's own plan and once
pinned to the tile code and split-K the query reports; the same kernel with the same split sums in the same order, so the two
outputs are equal bit for bit."""
import numpy as np
import pytest

from python_hip_stable_diffusion import _lib

pytestmark = pytest.mark.gpu

# (ksize, Cin, Cout, B, H, W, expected plan tiles, split-K above 1 expected)
SHAPES = [
    (1, 1280, 1280, 2, 16, 16, (12,), False),       # M = 512: smgemm.hip's rule, 256 workgroups
    (1, 320, 320, 2, 16, 16, (1, 2, 3, 4), False),  # a tiled kernel
    (3, 128, 128, 2, 16, 16, (7,), False),          # the K-split halo kernel
    (3, 1280, 1280, 2, 8, 8, (9,), True),           # M = 128: the weight stream (slabs + combine)
    (1, 2560, 640, 1, 16, 16, (1, 2, 3, 4), True),  # deep K, small M: split-K and the slab combine
    # the software-pipelined ring (gemm_pipe_kernel), which the table's codes 6 / 8 name.  The table's 1280 -> 320 row at M = 8192
    # (tile 3, code 6) is not what a handle runs there: with its pre-tiled copy the shape is bvgemm.hip's by the library's rule, which
    # comes before the table - so that shape pins plan tile 11, and the table's 1280 -> 1280 row at M = 1152 the 3-stage pipelined ring
    (1, 1280, 320, 2, 64, 64, (11,), False),
    (1, 1280, 1280, 2, 24, 24, (3,), False),
    (1, 320, 320, 2, 64, 64, (3,), False),          # the table's only plain 1x1 row with code 8: the 2-stage pipelined ring
]
# what launches for the rows that were added for a kernel, not a tile
KERNELS = {(1280, 320, 8192): "bvgemm v6", (1280, 1280, 1152): "gemm_pipe 64x64 ring3", (320, 320, 8192): "gemm_pipe 64x64 ring2"}


def tile_code(plan):
    """sd_op_conv2d's `tile` argument for a plan (table at the top of capi_ops.cpp)"""
    if plan["tile"] == 12:
        return 140 + plan["staging"]
    if plan["tile"] == 11:
        return 110 + plan["staging"]
    assert 1 <= plan["tile"] <= 9
    return plan["tile"] + 10 * plan["staging"]


@pytest.mark.parametrize("k,cin,cout,B,H,W,tiles,split", SHAPES)
def test_query_reports_the_plan_the_launch_runs(k, cin, cout, B, H, W, tiles, split):
    rs = np.random.RandomState(cin + cout + k)
    x = rs.randn(B, cin, H, W).astype(np.float16)
    w = (rs.randn(cout, cin, k, k) / np.sqrt(cin * k * k)).astype(np.float16)
    bias = rs.randn(cout).astype(np.float32)
    plan = _lib.conv_plan(k, 1, 1, cin, 0, cout, B, H, W, flags=16)
    assert plan["tile"] in tiles, plan
    assert plan["kernel"] == KERNELS.get((cin, cout, B * H * W), plan["kernel"]), plan
    assert (plan["splitk"] > 1) == split and plan["slab"] == split, plan
    assert (plan["workspace_bytes"] > 0) == split
    free, _ = _lib.conv2d(x, w, bias=bias)
    pinned, _ = _lib.conv2d(x, w, bias=bias, tile=tile_code(plan), splitk=plan["splitk"])
    assert np.isfinite(free.astype(np.float32)).all() and np.abs(free.astype(np.float32)).max() > 0.1
    assert np.array_equal(free.view(np.uint16), pinned.view(np.uint16)), plan
