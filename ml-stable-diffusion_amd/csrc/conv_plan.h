// The one planner of launch_conv: which kernel family a conv / 1x1 GEMM descriptor runs on, with which ring, split-K and
// workspace, and which pre-tiled weight copies its handle must hold.  Host code only (conv_plan.cpp makes no HIP call), so the
// CPU suite pins it row by row (tests/test_conv_plan.py through sd_op_conv_plan).
#pragma once
#include <string>

#include "kernels.h"

namespace sd {

// the kernel a plan launches (tile -1 / 1-4 / 7 / 18 / 25 / 21 / 9 / 14 / 17 / 10 / 11 / 12 / 15 / 19 / 13 / 16 / 20 / 22 / 24 of the wire format below)
enum class ConvKernel { Generic, Igemm, GemmPipe, HaloKs, HaloI8, HaloPal, HaloSubpix, Wstream, WstreamPal, WstreamI8, Wsgemm, Bvgemm, Smgemm, SmgemmPal, SmgemmI8, Smgeglu, SmgegluPal, SmgegluI8, SmqkvI8, SmgemmQ8 };

struct ConvPlan {
  // The wire format: what ConvDesc::tile / staging pins, tuned_convs.inc rows, SD_PLAN_TABLE and sd_tune_set_candidate say and what
  // sd_op_conv_plan, plan_out and SD_LOG_CONVS report.  Read by decode_plan (conv_plan.cpp) and by nothing else.
  int tile;        // 1: 128x128, 2: 128x64, 3: 64x64, 4: 64x128 (igemm.hip), 7: the K-split halo conv (conv3x3_halo.hip), 9: wstream.hip,
                   // 10: wsgemm.hip, 11: bvgemm.hip, 12: smgemm.hip, 13: smgeglu.hip, 14: wstream.hip from palettized weights,
                   // 15: smgemm.hip from palettized weights, 17: wstream.hip from int8 weights and activations (W8A8),
                   // 18: the halo conv from int8 weights and activations (conv3x3_halo_i8.hip; never the library's own answer),
                   // 19: the small-M GEMM from int8 weights and activations (smgemm_i8.hip, tile 12's tiles; never the library's own answer),
                   // 20: the GEGLU projection from int8 weights and int8 activations written by the LayerNorm in front of it
                   // (smgeglu_i8.hip, tile 13's tiles at both heights; never the library's own answer);
                   // 21: the upsampler conv as four 2x2 phase convs on the low-res halo (conv3x3_halo_sp.hip; only with ConvDesc::subpix);
                   // 22: the self-attention q|k|v projection from int8 weights and int8 activations written by the LayerNorm in front
                   // of it (smqkv_i8.hip, BM x 160-column tiles at tile 20's two heights; never the library's own answer);
                   // 24: the small-M GEMM from int8 weights and int8 activations written by their producer (smgemm_q8.hip, tile 12 / 19's
                   // tiles; never the library's own answer; 23 is not in use);
                   // 25: the halo conv from palettized weights (conv3x3_halo_pal.hip, tile 7's ring codes, split-K and
                   // slabs; never the library's own answer);
                   // -1 = not on the MFMA path (launch_conv_generic)
  int staging;     // per-family code: decode_plan
  int splitk;      // resolved: what the launch runs, no empty splits (halo: over 64-channel chunks; tile 9: the slab count)
  bool slab;       // the output leaves through fp32 slabs (split-K, weight stream, GroupNorm twins)
  size_t workspace_bytes;   // exactly what this launch needs of ConvWorkspace::partial
  // What the codes mean for this descriptor, resolved once by conv_plan(): all a launcher reads.
  ConvKernel kernel = ConvKernel::Generic;
  int bm = 0, bn = 0;        // Igemm / GemmPipe / HaloKs / HaloI8 / HaloPal (128 x 64, as its tile counts): tile rows x columns; Smgemm* / Smgeglu* / SmqkvI8: bm, tile rows
  int stages = 0;            // Igemm / GemmPipe / HaloKs / HaloI8 / HaloPal / HaloSubpix: the ring depth that runs, after the fall-back to one that fits the LDS
  int kgroups = 1;           // Igemm: 2 = in-workgroup split-K, two K groups of four waves with a ring each
  bool reg_staged = false;   // Igemm: A / B travel HBM -> VGPR -> LDS (the A/B reference form), two stages
  int waves = 0;             // Wstream*: waves (K slices) per workgroup, 4 or 8
  int variant = 0;           // Bvgemm: 1-6 (bvgemm.hip), the library's choice already made
};
// Pure function of the descriptor, the tuner candidate, the run-time table and the environment switches.  Raises the checks
// that belong to the plan (a forced tile the shape does not admit, the GroupNorm-loader / GroupNorm-fold shapes).
ConvPlan conv_plan(const ConvDesc& d);

// the pre-tiled weight copies a handle must hold for this conv (d.w_tiled / w_ws / w_bv are not looked at)
struct ConvWeightCopies {
  bool wstream, wsgemm, bvgemm;
};
ConvWeightCopies conv_plan_copies(const ConvDesc& d);

// The build-time question of whoever holds a compressed form of this conv's weights: does a kernel read that form on the device?
// d is the conv as it would run from fp16 (d.w / the copies / d.cw are not looked at), `held` what the weight store holds for the
// tensor, `opt_in` the call site's consent to a pinned 1x1 / GEGLU kernel (a pinned op cannot move to igemm_kernel when a later
// GroupNorm asks for epilogue statistics).  The answer is the source kind with its pin in wire-format codes (ConvDesc::tile /
// staging), or Fp16: upload the de-compressed tensor and run as ever.  A kind is taken exactly where the plan of the fp16 conv, with
// the copies a handle would hold, is the kind's fp16 twin by the library's own rule, with the twin's wave count / tile height:
//   Palette: opted-in GEGLU (tile 16 for tile 13 on the 128-row tiles the palettized kernel has), then the weight stream (tile 14 for
//            tile 9), then the opted-in single-source small-M GEMM (tile 15 for tile 12), then - only where the store's halo switch
//            is on (`pal_halo`, sd_weights_palette_halo) - the halo conv (tile 25 for tile 7 without the GroupNorm loader, with that
//            plan's ring code and split-K: halo_pal_ok)
//   W8A8:    the weight stream (tile 17) by tile 14's predicate, then the halo conv (tile 18 for tile 7 without the GroupNorm loader,
//            with that plan's ring code and split-K; Ctot <= kHaloI8MaxCtot), then the opted-in single-source small-M GEMM (tile 19 for
//            tile 12: tile 15's predicate; K <= kSmI8MaxK holds wherever tile 12 is the library's rule); an observing store asks this
//            without holding a mark, with the call site's consent only when it observes the projections too.  In front of all of
//            them, as the palette branch does for tile 16: the opted-in GEGLU (tile 20 for tile 13 at the same tile height, both
//            heights) - asked WITHOUT the LayerNorm fold's fields, which tile 20 does not take (the caller un-folds: UNet::transformer_block)
//            - and the opted-in fused q|k|v launch (tile 22, which has no fp16 twin: taken wherever smqkv_i8_shape_ok admits the
//            un-folded descriptor, at the height smqkv_i8_bm resolves; `held` then speaks for all three tensors - the caller has
//            checked that each carries a mark and that the marks share one range) - and the opted-in plain projection whose
//            descriptor says that its activations arrive as int8 (d.x0_i8 set: ff.net.2 behind the GEGLU, UNet::transformer_block; tile
//            24, which has no fp16 twin to follow either - the un-merged ff.net.2 of the 1280-channel level is deeper than tile 12's own
//            rule goes: taken wherever smgemm_q8_wanted admits the descriptor, while SD_SMGEMM leaves tile 12 on)
enum class StoredWeights { Fp16, Palette, W8A8 };
struct WeightPin {
  WeightSource kind = WeightSource::Fp16;
  int tile = 0, staging = 0;
  int splitk = 0;   // I8Halo / PalHalo: the fp16 plan's resolved split-K (ConvDesc::splitk); 0 for the other kinds
};
WeightPin conv_plan_weights(const ConvDesc& d, StoredWeights held, bool opt_in, bool pal_halo = false);
// The pin of a kind by the caller's own choice (the operator entry points): n = waves per workgroup (4, anything else eight) of the
// weight-stream kinds, the tile height of the others (32 / 64, 128 / 256; 0 = by the shape)
WeightPin conv_plan_pin(WeightSource kind, int n);

// the SD_LOG_CONVS line of a launch (n_fast: what smgemm.hip / smgeglu.hip add to theirs)
void conv_plan_log(const ConvDesc& d, const ConvPlan& p, int n_fast = 0);

// What launches, as one line (sd_op_conv_plan_kernel): the kernel's name, then only the fields that kernel has -
//   "igemm <bm>x<bn> ring<stages>[ kg2][ regs]"    "gemm_pipe <bm>x<bn> ring<stages>"    "halo_ks ring<stages>"    "halo_i8 ring<stages>"
//   "conv3x3_halo_sp ring<stages>"                 "halo_pal ring<stages>"
//   "wstream waves<n>"   "wstream_pal waves<n>"    "wstream_i8 waves<n>"                 "wsgemm"    "bvgemm v<variant>"
//   "smgemm bm<bm>"      "smgemm_pal bm<bm>"       "smgemm_i8 bm<bm>"                    "smgeglu bm<bm>"    "smgeglu_pal bm<bm>"
//   "smgeglu_i8 bm<bm>"  "smqkv_i8 bm<bm>"        "smgemm_q8 bm<bm>"                    "generic"
std::string conv_plan_kernel_name(const ConvPlan& p);

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
// Plan tile 25, the one predicate: tile 7's shapes with the plain split-able epilogue, no GroupNorm in the loader, no ablation build
// (tile 18's rule without its int32 bound - nothing here sums in int32)
bool halo_pal_ok(const ConvDesc& d);
// Plan tile 21 (ConvDesc::subpix): the general admissibility - halo_ks_ok's conditions on the LOW-RES image (3x3, stride 1, up 2,
// kOutHalf, C0 % 64 == 0, N % 4 == 0, Hi >= 8, Wi >= 8), one source, fp16 weights, no GroupNorm loader, no twins, no LayerNorm fold /
// q|k|v, 32-bit buffer offsets.  halo_sp_refusal names the first condition a descriptor misses, nullptr when it misses none.
const char* halo_sp_refusal(const ConvDesc& d);
inline bool halo_sp_ok(const ConvDesc& d) { return halo_sp_refusal(d) == nullptr; }
// The shapes the library takes tile 21 for on its own: the list measured in a step, in the manner of conv_plan_is_tuned.
// SD_UP_SUBPIX (with SD_TUNE): 0 = none, 1 = the list (the default), 2 = every shape halo_sp_ok admits (measuring, small handles).
bool subpixel_wanted(const ConvDesc& d);
bool gemm_pipe_ok(int ksize, int stride, int up, int M, int N, int K, int C0, int C1);

// LDS budgets, stated once: decode_plan picks the ring that runs by them, the launchers assert them per instantiation.
constexpr size_t kLdsBudget = 160 * 1024;
// igemm_kernel / gemm_pipe_kernel: kgroups rings of nst stages of a bm x bn tile's A and B rows, then [2][bn] floats of epilogue constants
constexpr size_t ring_bytes(int bm, int bn, int nst) { return (size_t)nst * (bm + bn) * kConvBK * sizeof(half_t); }
constexpr bool ring_fits(int bm, int bn, int nst, int kgroups = 1) { return kgroups * ring_bytes(bm, bn, nst) + 2 * bn * sizeof(float) <= kLdsBudget; }
// conv3x3_halo_ks_kernel: two halo buffers, d stages of bn weight rows, [bn] floats of epilogue constants
constexpr int kHaloLdsRows = 184;
constexpr size_t halo_lds_bytes(int bn, int d) {
  return ((size_t)2 * kHaloLdsRows * kConvBK + (size_t)d * bn * kConvBK) * sizeof(half_t) + bn * sizeof(float);
}
// the same with GroupNorm in the loader: the [3][ctot] fp16 GroupNorm table takes the place of the epilogue constants behind the ring
constexpr size_t halo_gnl_lds_bytes(int d, int ctot) {
  const size_t k_loop = halo_lds_bytes(64, d) - 64 * sizeof(float) + (((size_t)6 * ctot + 15) & ~(size_t)15);
  const size_t epilogue = 32 * 1024 + 128 * (64 + 8) * 2 + 64 * sizeof(float);
  return k_loop > epilogue ? k_loop : epilogue;
}
// conv3x3_halo_i8_kernel: one fp16 staging buffer of tile 7's halo rows, two int8 halo images (64 B per pixel, halo rows kHaloI8Pitch
// pixels apart, kHaloI8Rows pixels with the rows the last DMA piece carries past the halo), d stages of 64 int8 weight rows, [2][64]
// floats of epilogue constants
constexpr int kHaloI8Pitch = 20, kHaloI8Rows = 204;
constexpr size_t halo_i8_lds_bytes(int d) {
  return (size_t)kHaloLdsRows * kConvBK * sizeof(half_t) + (size_t)2 * kHaloI8Rows * kConvBK + (size_t)d * 64 * kConvBK + 2 * 64 * sizeof(float);
}
// conv3x3_halo_pal_kernel (plan tile 25): tile 7's two halo buffers, d stages of kHaloPalStageBytes (one block of the index stream,
// 512 * nbits <= 4096 bytes, at a fixed pitch), then 1 KB: the 512-B LUT, [64] floats of epilogue constants, and the 256 B the LUT's
// one DMA piece (64 lanes x 16 B) carries past them.  80 896 B at d = 8: two workgroups per CU at every depth.
constexpr int kHaloPalStageBytes = 4096;
constexpr size_t halo_pal_lds_bytes(int d) { return (size_t)2 * kHaloLdsRows * kConvBK * sizeof(half_t) + (size_t)d * kHaloPalStageBytes + 1024; }
static_assert(2 * halo_pal_lds_bytes(8) <= kLdsBudget, "plan tile 25: two workgroups per CU with the deepest ring");
// exact int32 sums: 127 * 127 * 9 * Ctot < 2^31
constexpr int kHaloI8MaxCtot = 14784;
static_assert(127LL * 127 * 9 * kHaloI8MaxCtot < (1LL << 31) && 127LL * 127 * 9 * (kHaloI8MaxCtot + 64) >= (1LL << 31), "int32 bound of plan tile 18");
// smgemm_i8_kernel (plan tile 19) sums the whole K of a 1x1 GEMM in int32: 127 * 127 * K < 2^31, the last multiple of 64 that fits
constexpr int kSmI8MaxK = 133120;
static_assert(127LL * 127 * kSmI8MaxK < (1LL << 31) && 127LL * 127 * (kSmI8MaxK + 64) >= (1LL << 31), "int32 bound of plan tile 19");
// (smgeglu_i8_kernel, plan tile 20, smqkv_i8_kernel, plan tile 22, and smgemm_q8_kernel, plan tile 24, sum the whole K of their 1x1 GEMMs
// the same way: the same bound)

// Plan tile 22 (smqkv_i8.hip): the fused q|k|v projection [Wq | Wk | Wv] (3C, C) of a self-attention from int8 weights and the int8
// output of norm1 - BM x kSmQkvCols tiles, BM = 128 / 256 (variant 1 / 2; 0: by the grid, tile 13's rule - 128 rows while that grid
// stays within one round of 256 workgroups).  The rule, host only:
//   * a single-source 1x1 GEMM, kOutHalf, N = 3 C0 with the V columns leaving transposed (n_trans = 2 C0), no LayerNorm fold (the int8
//     activations ARE the LayerNorm's output), no time embedding, residual, GroupNorm statistics, twins, phase clocks or debug hooks;
//   * C0 >= 640 - the levels whose self-attention is a launch of its own; the 320-channel level's head is ONE launch
//     (gn_proj_qkv_kernel), and a rule that admitted its width would have the observers and the accounting promise a layer no handle
//     runs from int8 - C0 % kSmQkvCols == 0, so that a tile lies inside q, k or v and the boundaries fall on tile boundaries,
//     C0 % 64 == 0 (whole K64 stages), C0 <= kSmI8MaxK;
//   * S = Ho * Wo a multiple of 16: a lane's four V^T tokens and the 16-token blocks vt_perm permutes lie in one sample; ldT >= S, ldT % 8 == 0;
//   * q_cols 0 (no q_scale) or C0 (the queries, whole tiles);
//   * M % BM == 0, at least two tile rows, a tile count that is a multiple of 8 (the XCD runs of sm_tile.h) and at most 65535.
// Plan tile 24 (smgemm_q8.hip) in a handle: smgemm_q8_shape_ok - tile 19's eligibility - on the grids tile 12's own rule takes (M from
// 256 to 2048, 192 to 256 tiles: one round of the chip; the 8 x 8 mid block at M = 128 is not among them), at any K up to kSmI8MaxK, no
// GroupNorm statistics wanted of the output.
bool smgemm_q8_wanted(const ConvDesc& d);
constexpr int kSmQkvCols = 160;
bool smqkv_i8_shape_ok(const ConvDesc& d, int variant);
bool smqkv_i8_tiles(const ConvDesc& d, int variant);   // the rule without the int32 bound (an operator entry names that refusal on its own)
int smqkv_i8_bm(const ConvDesc& d, int variant);   // the tile height of a variant: 128 or 256

}  // namespace sd
