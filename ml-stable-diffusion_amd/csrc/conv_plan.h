// The one planner of launch_conv: which kernel family a conv / 1x1 GEMM descriptor runs on, with which ring, split-K and
// workspace, and which pre-tiled weight copies its handle must hold.  Host code only (conv_plan.cpp makes no HIP call), so the
// CPU suite pins it row by row (tests/test_conv_plan.py through sd_op_conv_plan).
#pragma once
#include "kernels.h"

namespace sd {

struct ConvPlan {
  int tile;        // 1: 128x128, 2: 128x64, 3: 64x64, 4: 64x128 (igemm.hip), 7: the K-split halo conv (conv3x3_halo.hip), 9: wstream.hip,
                   // 10: wsgemm.hip, 11: bvgemm.hip, 12: smgemm.hip, 13: smgeglu.hip, 14: wstream.hip from palettized weights,
                   // 15: smgemm.hip from palettized weights; -1 = not on the MFMA path (launch_conv_generic)
  int staging;     // ring code (tiles 1-4, 7: launch_tile / launch_halo_ks), wave-count code (9, 14: 4 = four waves, else eight), variant (11, 12, 13),
                   // tile height (15: 1 / 2 = 32 / 64 rows)
  int splitk;      // resolved: what the launch runs, no empty splits (halo: over 64-channel chunks; tile 9: the slab count)
  bool slab;       // the output leaves through fp32 slabs (split-K, weight stream, GroupNorm twins)
  size_t workspace_bytes;   // exactly what this launch needs of ConvWorkspace::partial
};
// Pure function of the descriptor, the tuner candidate, the run-time table and the environment switches.  Raises the checks
// that belong to the plan (a forced tile the shape does not admit, the GroupNorm-loader / GroupNorm-fold shapes).
ConvPlan conv_plan(const ConvDesc& d);

// the pre-tiled weight copies a handle must hold for this conv (d.w_tiled / w_ws / w_bv are not looked at)
struct ConvWeightCopies {
  bool wstream, wsgemm, bvgemm;
};
ConvWeightCopies conv_plan_copies(const ConvDesc& d);

// A handle that holds a palette for this conv's weights asks at build time: 4 / 8 = run it from the index stream (plan tile 14) with
// that many waves per workgroup - the conv's plan with fp16 copies would be the weight stream with that wave count; 0 = upload the
// de-palettized tensor and run as ever.  d.w / w_tiled / w_pal are not looked at.
int conv_plan_pal_waves(const ConvDesc& d);
// The same question for the small-M 1x1 GEMM (plan tile 15): 32 / 64 = this conv, uploaded as fp16 with the copies a handle would hold,
// would get plan tile 12 by the library's own rule with that tile height - run it from the index stream of smgemm_pal_pack instead;
// 0 = no (SD_SMGEMM=0, two sources, a LayerNorm fold, any other plan): upload the de-palettized tensor.
int conv_plan_pal_gemm(const ConvDesc& d);

// the SD_LOG_CONVS line of a launch (bm / n_fast: what smgemm.hip / smgeglu.hip add to theirs)
void conv_plan_log(const ConvDesc& d, const ConvPlan& p, int bm = 0, int n_fast = 0);

// Tile order inside an XCD's run of workgroup ids, from an estimate of the bytes each order pulls through the fabric into the 8 XCD L2s:
//   m fastest: every weight panel once; the activations once per XCD when they fit an L2, else once per n-tile
//   n fastest: the activations once; the weights once per XCD when they fit an L2, else once per m-tile
// nbm / nbn: tile counts along m / n.  ab_switch: honour SD_TILE_ORDER (igemm.hip only).
// (SD_TILE_ORDER=2: round 3's first rule, activations x (n-tiles - 1) > 7 x weights - same step time at batch 2, but it
// sent the 1280 -> 1280 GEMMs of the 16x16 level n-fast: 27 MB of fabric reads per launch for 4.6 MB of operands)
bool choose_tile_order(double a_bytes, double w_bytes, double nbm, double nbn, bool ab_switch);

bool conv_reduce_stats_on();   // SD_REDUCE_STATS: the slab combine also leaves the GroupNorm statistics of its result

// shape rules and tile geometry shared by the planner and the launchers
constexpr int kConvBK = 64;   // K step (halves) of the MFMA kernels
bool halo_ks_ok(const ConvDesc& d);
bool gemm_pipe_ok(int ksize, int stride, int up, int M, int N, int K, int C0, int C1);
void tile_dims(int tile, int& bm, int& bn);

}  // namespace sd
