// The conv / GEMM planner (conv_plan.h).  No kernel and no HIP call in this file.
#include "conv_plan.h"

#include <algorithm>
#include <cstring>

namespace sd {

namespace {

constexpr int BK = kConvBK;

// the sizes the rules below are written in (IgemmArgs carries the same numbers to the kernels: igemm_device.h make_args)
struct Dims {
  int Ctot, M, N, K, HoWo, nk_total, tiles_x, tiles_y;
};
Dims dims_of(const ConvDesc& d) {
  Dims a;
  a.Ctot = d.C0 + (d.x1 ? d.C1 : 0);
  a.M = d.B * d.Ho * d.Wo;
  a.N = d.N;
  a.K = d.ksize * d.ksize * a.Ctot;
  a.HoWo = d.Ho * d.Wo;
  a.nk_total = a.K / BK;
  a.tiles_x = cdiv(d.Wo, 16);   // halo kernels: stride 1, so output = (upsampled) input extent
  a.tiles_y = cdiv(d.Ho, 8);
  return a;
}

// The A/B switches of the plan, each read here and nowhere else (SD_TUNE only: sd_common.h tune_env_int).
//   SD_WSTREAM=0 takes plan tile 9 out of every plan; SD_WSGEMM / SD_BVGEMM / SD_SMGEMM / SD_SMGEGLU=0 keep the library's own rule
//   from taking tiles 10 / 11 / 12 / 13 (a forced tile still runs); SD_REDUCE_STATS=1: GroupNorm statistics from the slab combine
//   (measured: the step loses 0.25 ms with it, LAB_NOTES.md r5 - off unless asked for); SD_QKV_I8=0 takes plan tile 22 out of every
//   plan: a marked q|k|v launch stays the folded fp16 launch (conv_plan_weights), a pinned descriptor is refused
struct Switches {
  bool wstream, wsgemm, bvgemm, smgemm, smgeglu, reduce_stats, tuning, qkv_i8;
};
const Switches& switches() {
  static const Switches s = {tune_env_int("SD_WSTREAM", 1) != 0, tune_env_int("SD_WSGEMM", 1) != 0, tune_env_int("SD_BVGEMM", 1) != 0,
                             tune_env_int("SD_SMGEMM", 1) != 0, tune_env_int("SD_SMGEGLU", 1) != 0, tune_env_int("SD_REDUCE_STATS", 0) != 0,
                             getenv("SD_TUNE") != nullptr, tune_env_int("SD_QKV_I8", 1) != 0};
  return s;
}

struct Plan {
  int tile;     // 1: 128x128, 2: 128x64, 3: 64x64, 4: 64x128
  int splitk;
  int staging = 0;   // the code beside the tile (decode_plan)
};

// the LayerNorm fold needs whole rows per workgroup, the fused q|k|v epilogue has no slab path
bool can_split(const ConvDesc& d) { return d.out_mode == kOutHalf && !d.ln_colsum && !d.out_t; }
// the weight-streaming kernel can take this conv: its pre-tiled weights exist and the shape is its own (SD_WSTREAM: tile_ok)
bool can_stream(const ConvDesc& d) { return d.w_tiled != nullptr && can_split(d) && wstream_shape_ok(d); }
// a descriptor with a compressed weight source (ConvDesc::cw) is pinned to the source's kernel: it holds no fp16 weights to run anything
// else on.  Plan tiles 14 / 17: the palettized / int8 weight stream
bool pal_stream(const ConvDesc& d) { return d.cw.kind == WeightSource::PalWstream; }
bool i8_stream(const ConvDesc& d) { return d.cw.kind == WeightSource::I8Wstream; }
// plan tile 18: the int8 halo conv - tile 7's shapes without the GroupNorm loader, inside the int32 bound
bool i8_halo(const ConvDesc& d) { return d.cw.kind == WeightSource::I8Halo; }
bool halo_i8_ok(const ConvDesc& d) {
  return halo_pal_ok(d) && d.C0 + (d.x1 ? d.C1 : 0) <= kHaloI8MaxCtot;   // (halo_pal_ok: the rule without the int32 bound)
}
// plan tile 25: the palettized halo conv - tile 7's shapes without the GroupNorm loader (halo_pal_ok below: no int32 bound)
bool pal_halo(const ConvDesc& d) { return d.cw.kind == WeightSource::PalHalo; }
// plan tile 15: the small-M 1x1 GEMM;  plan tile 16: the GEGLU projection
bool pal_gemm(const ConvDesc& d) { return d.cw.kind == WeightSource::PalGemm; }
bool pal_geglu(const ConvDesc& d) { return d.cw.kind == WeightSource::PalGeglu; }
// plan tile 19: the small-M 1x1 GEMM from int8 weights and activations
bool i8_gemm(const ConvDesc& d) { return d.cw.kind == WeightSource::I8Gemm; }
// plan tile 20: the GEGLU projection from int8 weights and int8 activations
bool i8_geglu(const ConvDesc& d) { return d.cw.kind == WeightSource::I8Geglu; }
// plan tile 22: the fused q|k|v projection from int8 weights and int8 activations
bool i8_qkv(const ConvDesc& d) { return d.cw.kind == WeightSource::I8Qkv; }
// plan tile 24: the small-M 1x1 GEMM from int8 weights and int8 activations
bool i8_gemm_q(const ConvDesc& d) { return d.cw.kind == WeightSource::I8GemmQ; }
// tiles 9 / 14 / 17: the code's wave count (decode_plan)
int wstream_waves(int code) { return code == 4 ? 4 : 8; }
// fp32 slabs of a launch: one per split, one when only `slab` (weight stream, GroupNorm twins) asks for the slab path
size_t slab_bytes(const Dims& a, int splits, bool slab) { return (splits > 1 || slab) ? (size_t)splits * a.M * a.N * sizeof(float) : 0; }

// Heuristic (overridden per shape by the measured table in tuned_convs.inc when present):
// prefer the biggest tile whose grid, multiplied by the split-K it can afford (>= 16 K-tiles per
// split), still gives every CU work (>= ~1.5 workgroups per CU); deep-K small-M layers (8x8 /
// 16x16 levels stream weights: SURVEY.md 7.3(1)) end up split, shallow 1x1 GEMMs end up on the
// small tile with many workgroups.
// kind: 0 plain epilogue (bias / timestep embedding / residual), 1 LayerNorm-folded, 2 GEGLU (LayerNorm-folded or
// not), 3 fused q|k|v (LayerNorm-folded, V columns leave transposed).  staging: see decode_plan.
struct TunedConv { int kind, ksize, stride, up, ctot, n, m, tile, staging, splitk; };
#if __has_include("tuned_convs.inc")
static const TunedConv kTuned[] = {
#include "tuned_convs.inc"
};
static const int kNumTuned = sizeof(kTuned) / sizeof(kTuned[0]);
#else
static const TunedConv* kTuned = nullptr;
static const int kNumTuned = 0;
#endif

// SD_PLAN_TABLE=<file>: rows "{kind, ksize, stride, up, Ctot, N, M, tile, staging, splitk}" (the format of
// tuned_convs.inc) read at first use and consulted BEFORE the compiled-in table - how tools/tune_plans.py
// validates a freshly measured table in the same GPU session without a rebuild.
bool parse_plan_row(const char* line, TunedConv& r) {
  return sscanf(line, " {%d, %d, %d, %d, %d, %d, %d, %d, %d, %d}", &r.kind, &r.ksize, &r.stride, &r.up, &r.ctot, &r.n, &r.m, &r.tile,
                &r.staging, &r.splitk) == 10;
}
std::vector<TunedConv>& runtime_table() {
  static std::vector<TunedConv> table = [] {
    std::vector<TunedConv> t;
    const char* path = tune_env_set("SD_PLAN_TABLE") ? getenv("SD_PLAN_TABLE") : nullptr;
    if (!path) return t;
    FILE* f = fopen(path, "r");
    if (!f) {
      fprintf(stderr, "[sd] SD_PLAN_TABLE=%s cannot be opened - ignored\n", path);
      return t;
    }
    char line[512];
    while (fgets(line, sizeof(line), f)) {
      TunedConv r;
      if (parse_plan_row(line, r)) t.push_back(r);
    }
    fclose(f);
    fprintf(stderr, "[sd] SD_PLAN_TABLE=%s: %zu plans\n", path, t.size());
    return t;
  }();
  return table;
}

// measurement hook (sd_tune_set_candidate): while tile != 0 every conv whose constraints allow it runs this plan,
// so one profiled forward evaluates a candidate on every layer shape at once, in sequence (tools/tune_plans.py)
struct TuneCandidate { int tile = 0, staging = 0, splitk = 0; };
TuneCandidate g_tune;

void tile_dims(int tile, int& bm, int& bn) {
  switch (tile) {
    case 7: bm = 128; bn = 64; break;    // halo conv (8x16-pixel tile), K-split waves + register double buffering
    case 1: bm = 128; bn = 128; break;
    case 2: bm = 128; bn = 64; break;
    case 3: bm = 64; bn = 64; break;
    default: bm = 64; bn = 128; break;
  }
}

int conv_kind(const ConvDesc& d) {
  if (d.out_t) return 3;
  if (d.out_mode == kOutGeglu) return 2;
  return d.ln_colsum ? 1 : 0;
}

// the table match: a row is for this descriptor's shape key (choose_plan adds "and its tile is admissible")
bool table_match(const TunedConv& t, const ConvDesc& d, const Dims& a) {
  return t.kind == conv_kind(d) && t.ksize == d.ksize && t.stride == d.stride && t.up == d.up && t.ctot == a.Ctot && t.n == a.N && t.m == a.M;
}

Plan choose_plan(const ConvDesc& d, const Dims& a) {
  Plan p{d.tile, d.splitk};
  p.staging = d.staging;
  const bool geglu = d.out_mode == kOutGeglu;
  const bool split_ok = can_split(d);
  // plan tiles: 1 = 128x128, 2 = 128x64, 3 = 64x64, 4 = 64x128 (igemm_kernel / gemm_pipe_kernel), 7 = the halo conv.  Codes 5 / 6
  // (round 2's first halo kernel) and 8 / 9 (256x128 / 256x256 GEMM tiles, measured in round 3 and selected nowhere) were removed
  // in round 4: a caller or table row that names them gets the heuristic.
  auto is_halo = [](int c) { return c == 7; };
  // plan tile 9 = the weight-streaming kernel of wstream.hip (needs the pre-tiled weights; its slab count follows from the wave
  // count its code names).  SD_WSTREAM=0 (with SD_TUNE) takes it out of every plan: A/B.
  auto tile_ok = [&](int c) {
    if (c == 9) return switches().wstream && can_stream(d);
    if (!((c >= 1 && c <= 4) || c == 7)) return false;
    if (is_halo(c)) return halo_ks_ok(d) && !d.ln_colsum && !d.out_t && !geglu;
    int bm, bn;
    tile_dims(c, bm, bn);
    if (geglu && c != 1 && c != 4) return false;       // GEGLU value/gate pairs need 64 n-columns per wave
    if (d.out_t && d.n_trans % bn != 0) return false;  // the q|k / v boundary must be a tile boundary
    return true;
  };
  if (!tile_ok(p.tile)) p.tile = 0;
  auto blocks_of = [&](int c) {
    int bm, bn;
    tile_dims(c, bm, bn);
    const long mt = is_halo(c) ? (long)d.B * a.tiles_x * a.tiles_y : cdiv(a.M, bm);
    return mt * cdiv(a.N, bn);
  };
  auto ksteps = [&](int c) { return is_halo(c) ? a.Ctot / BK : a.nk_total; };   // split-K granularity
  auto max_split = [&](int c) {
    // a split costs a dependent reduce launch (~6 us): worth it only while each split still runs >= 16 K
    // steps (measured: 20-step 1x1 GEMMs lose 2.5 us when split in two, 180-step 3x3 convs peak at 8 splits)
    const int per_min = is_halo(c) ? 2 : 16;     // halo splits whole 64-channel chunks (9 K steps each)
    int s = 1;
    while (split_ok && s < 16 && ksteps(c) / (s * 2) >= per_min) s *= 2;
    return s;
  };
  // the caller chose (operator-level A/B tests); an int8 / palettized halo conv is tile 7's plan whatever a table row or a tuner candidate says
  const bool pinned = p.tile != 0 || p.splitk != 0 || p.staging != 0 || i8_halo(d) || pal_halo(d);
  if (i8_halo(d) || pal_halo(d)) p.tile = 7;
  if (!pinned && g_tune.tile != 0 && tile_ok(g_tune.tile)) {
    p.tile = g_tune.tile;
    p.staging = g_tune.staging;
    p.splitk = g_tune.splitk;
  } else if (!pinned) {
    auto match = [&](const TunedConv& t) { return table_match(t, d, a) && tile_ok(t.tile); };
    const TunedConv* hit = nullptr;
    for (const TunedConv& t : runtime_table())
      if (!hit && match(t)) hit = &t;
    for (int i = 0; i < kNumTuned && !hit; ++i)
      if (match(kTuned[i])) hit = &kTuned[i];
    if (hit) {
      p.tile = hit->tile;
      p.staging = hit->staging;
      p.splitk = hit->splitk;
    }
  }
  // (measured and dropped, round 3: sending every untuned 1x1 GEMM with M >= 8192 to the software-pipelined kernel's 128x64
  // tile - 10-25 % faster stand-alone at UNet batch 16 - made the batch-16 step 1.3 % and the batch-4 step 0.6 % SLOWER in
  // sequence; the pipelined kernel is only used where tools/tune_e2e.py accepted it end to end)
  // 8x8 level at any small batch: a 3x3 conv there is a weight stream (wstream.hip), whatever the table says for M = 128
  if (p.tile == 0 && tile_ok(9) && d.ksize == 3 && a.HoWo <= 64 && a.M <= 256) p.tile = 9;
  if (p.tile == 9) {
    p.splitk = 1;   // (the slab count follows from the wave count: conv_plan)
    return p;
  }
  if (p.tile == 0 && tile_ok(7)) {
    // no measured plan for this shape: the K-split halo kernel with the 4-stage ring won every 3x3 / stride-1 shape that was
    // tuned (SD2.1-base, SDXL-base, SD1.5: tuned_convs.inc); split-K below as for the other kernels
    p.tile = 7;
    if (p.staging == 0) p.staging = 3;
  }
  if (p.tile == 0) {
    p.tile = 3;
    for (int c : {1, 2, 4, 3}) {
      if (!tile_ok(c)) continue;
      if (blocks_of(c) * max_split(c) >= 384 || c == 3) { p.tile = c; break; }
    }
    if (!tile_ok(p.tile)) p.tile = 4;
  }
  if (p.splitk == 0) {
    p.splitk = 1;
    const int ms = max_split(p.tile);
    const long want = p.tile == 7 ? 192 : 384;   // the pipelined halo kernel is at its best from ~160 workgroups (1 per CU)
    while (blocks_of(p.tile) * p.splitk < want && p.splitk < ms) p.splitk *= 2;
  }
  if (!split_ok) p.splitk = 1;
  if (p.splitk > ksteps(p.tile)) p.splitk = ksteps(p.tile);
  if (p.splitk < 1) p.splitk = 1;
  return p;
}

// Would the plan of this conv be the weight-streaming kernel (plan tile 9) if its fragment-major weight copy existed?  The ONE
// predicate the copy is allocated by (a second, looser copy of this rule left ~430 MB of copies per handle that no
// kernel reads).
bool plan_is_wstream(const ConvDesc& d0) {
  if (!wstream_shape_ok(d0)) return false;
  ConvDesc d = d0;
  static const half_t present = 0;
  d.w_tiled = &present;   // choose_plan only tests the pointer
  return choose_plan(d, dims_of(d)).tile == 9;
}

}  // namespace

// the K-split halo kernel also folds the nearest-x2 upsample into its gather and takes 8-pixel-wide images (half of each
// 8x16 tile is then padding: the 8x8 level streams weights, MFMA work is not what bounds it)
bool halo_ks_ok(const ConvDesc& d) {
  const int c1 = d.x1 ? d.C1 : 0;
  return d.ksize == 3 && d.stride == 1 && (d.up == 1 || d.up == 2) && d.pad < 0 && d.out_mode == kOutHalf && d.Wo >= 8 && d.Ho >= 8 &&
         d.C0 % BK == 0 && c1 % BK == 0 && d.N % 4 == 0;
}

bool halo_pal_ok(const ConvDesc& d) { return halo_ks_ok(d) && can_split(d) && !d.gnf_partial && !d.debug; }

const char* halo_sp_refusal(const ConvDesc& d) {
  if (d.x1) return "a second source";
  if (d.ksize != 3) return "not a 3x3 conv";
  if (d.stride != 1) return "stride is not 1";
  if (d.up != 2) return "no nearest-x2 upsample (up is not 2)";
  if (d.pad >= 0) return "explicit padding";
  if (d.out_mode != kOutHalf) return "the output mode is not plain fp16 (GEGLU / transposed)";
  if (d.ln_colsum || d.out_t) return "a LayerNorm fold / fused q|k|v epilogue";
  if (d.Ho != 2 * d.Hi || d.Wo != 2 * d.Wi) return "the output is not twice the input";
  if (d.Hi < 8) return "Hi < 8";
  if (d.Wi < 8) return "Wi < 8";
  if (d.C0 % BK != 0) return "C0 is no multiple of 64";
  if (d.N % 4 != 0) return "N is no multiple of 4";
  if (d.gnf_partial) return "GroupNorm in the loader";
  if (d.n_twins > 0) return "GroupNorm twins";
  if (d.cw.kind != WeightSource::Fp16) return "a compressed weight source";
  if (d.debug) return "an ablation build";
  const size_t lim = (size_t)1 << 31;
  if ((size_t)d.B * d.Hi * d.Wi * d.C0 * 2 >= lim || (size_t)16 * d.N * d.C0 * 2 >= lim) return "an operand of 2 GiB or more";
  return nullptr;
}

// Which upsampler shapes run as tile 21 on the library's own rule: those whose STEP measured faster with it than without (graph
// replay, interleaved pairs with disjoint ranges; LAB_NOTES.md round 28), keyed like a tuned_convs.inc row by (Ctot, N, M of the output).
bool subpixel_wanted(const ConvDesc& d) {
  static const int mode = tune_env_int("SD_UP_SUBPIX", 1);
  if (mode == 0 || !halo_sp_ok(d)) return false;
  const int M = d.B * d.Ho * d.Wo;
  static const int only_m = tune_env_int("SD_UP_SUBPIX_M", 0);   // mode 2 on the one shape with this many output pixels: a candidate's own A/B
  if (mode >= 2) return only_m == 0 || only_m == M;
  struct Shape { int ctot, n, m; };
  static const Shape kMeasured[] = {
      {1280, 1280, 2048},   // SD2.1-base up_blocks.1, 16x16 -> 32x32 at CFG batch 2: 65.4 -> 45.4 us in sequence
      {640, 640, 8192},     // SD2.1-base up_blocks.2, 32x32 -> 64x64: 59.5 -> 39.4 us in sequence
      // (1280 -> 1280, 8x8 -> 16x16, M = 512 is weight-stream-bound and reads 52 MB instead of 29.5: 27.8 -> 31.2 us in sequence, not taken)
      {0, 0, 0}};   // (terminator; a row of zeros matches nothing)
  for (const Shape& s : kMeasured)
    if (s.ctot == d.C0 && s.n == d.N && s.m == M && s.ctot != 0) return true;
  return false;
}

bool gemm_pipe_ok(int ksize, int stride, int up, int M, int N, int K, int C0, int C1) {
  const size_t lim = (size_t)1 << 31;
  return ksize == 1 && stride == 1 && up == 1 && (size_t)M * std::max(C0, C1) * 2 < lim && (size_t)N * K * 2 < lim;
}

bool conv_fast_path_ok(const ConvDesc& d) {
  const int c1 = d.x1 ? d.C1 : 0;
  if (d.C0 % BK != 0 || c1 % BK != 0) return false;
  if (d.N % 4 != 0) return false;
  if (d.out_mode == kOutGeglu && d.N % 64 != 0) return false;
  if (!(d.ksize == 1 || d.ksize == 3)) return false;
  if (!(d.up == 1 || d.up == 2)) return false;
  return true;
}

// plan tile 22's tiles (the rule: conv_plan.h)
int smqkv_i8_bm(const ConvDesc& d, int variant) {
  if (variant == 1) return 128;
  if (variant == 2) return 256;
  const long M = (long)d.B * d.Ho * d.Wo;
  return M % 128 == 0 && M / 128 * (d.N / kSmQkvCols) <= 256 ? 128 : 256;
}
bool smqkv_i8_shape_ok(const ConvDesc& d, int variant) { return smqkv_i8_tiles(d, variant) && d.C0 <= kSmI8MaxK; }
bool smqkv_i8_tiles(const ConvDesc& d, int variant) {
  if (variant < 0 || variant > 2) return false;
  if (!(d.ksize == 1 && d.stride == 1 && d.up == 1 && !d.x1 && d.out_mode == kOutHalf && !d.ln_colsum && !d.temb && !d.res && !d.gnf_partial &&
        !d.gn_partial && d.n_twins == 0 && !d.debug && !d.prof && !d.subpix))
    return false;
  const int C = d.C0;
  if (!(C >= 640 && C % kSmQkvCols == 0 && C % 64 == 0 && d.N == 3 * C && d.n_trans == 2 * C && (d.q_cols == 0 || d.q_cols == C)))
    return false;
  const long S = (long)d.Ho * d.Wo, M = d.B * S;
  if (!(S % 16 == 0 && d.ldT >= S && d.ldT % 8 == 0)) return false;
  const int bm = smqkv_i8_bm(d, variant);
  const long mt = M / bm, nt = d.N / kSmQkvCols;
  return M % bm == 0 && mt >= 2 && (mt * nt) % 8 == 0 && mt * nt <= 65535;
}

// plan tile 24 in a handle (the rule: conv_plan.h)
bool smgemm_q8_wanted(const ConvDesc& d) {
  if (!smgemm_q8_shape_ok(d, 0) || d.gn_partial) return false;
  const long M = (long)d.B * d.Ho * d.Wo;
  const long tiles = M / smgemm_bm(d, 0) * (d.N / 80);
  return M >= 256 && M <= 2048 && tiles >= 192 && tiles <= 256;
}

namespace {

// resolved split-K of plan tile 21: tile 7's rule (workgroups for every CU, a split keeps >= 2 chunks) over its grid of
// 4 phases x low-res tiles x n-tiles; whole 64-channel chunks, no empty splits
int subpix_splits(const ConvDesc& d, const Dims& a) {
  const int steps = a.Ctot / BK;
  int s = d.splitk;
  if (s == 0) {
    const long blocks = 4L * d.B * cdiv(d.Wi, 16) * cdiv(d.Hi, 8) * cdiv(a.N, 64);
    s = 1;
    while (blocks * s < 192 && s < 16 && steps / (s * 2) >= 2) s *= 2;
  }
  s = std::min(std::max(s, 1), steps);
  return cdiv(steps, cdiv(steps, s));
}

// the plan in the wire format: tile, code, resolved split-K, slab, workspace
ConvPlan plan_codes(const ConvDesc& d) {
  const CompressedWeights& cw = d.cw;
  // (an int8 halo descriptor off the MFMA path has no direct kernel to fall to: refused like every other shape tile 18 does not take)
  if (i8_halo(d))
    SD_REQUIRE(conv_fast_path_ok(d) && cw.stream && cw.scale && halo_i8_ok(d), kInvalidArgument,
               "plan tile 18 (conv3x3_halo_i8.hip, int8) needs the int8 weights, the scales and a 3x3 / stride-1 shape of the halo conv with "
               "at most %d input channels (k=%d stride=%d up=%d C0=%d C1=%d N=%d)", kHaloI8MaxCtot, d.ksize, d.stride, d.up, d.C0, d.x1 ? d.C1 : 0, d.N);
  // (nor has a palettized halo descriptor: tile 25 takes it or nobody does)
  if (pal_halo(d))
    SD_REQUIRE(conv_fast_path_ok(d) && cw.stream && cw.lut && palette_bits_ok(cw.bits) && halo_pal_ok(d), kInvalidArgument,
               "plan tile 25 (conv3x3_halo_pal.hip) needs the index stream, the LUT and a 3x3 / stride-1 shape of the halo conv without "
               "GroupNorm in the loader (k=%d stride=%d up=%d C0=%d C1=%d N=%d %dx%d)", d.ksize, d.stride, d.up, d.C0, d.x1 ? d.C1 : 0, d.N, d.Ho, d.Wo);
  // (nor has an int8 GEMM descriptor: tile 19 takes it or nobody does)
  if (i8_gemm(d))
    SD_REQUIRE(conv_fast_path_ok(d) && cw.stream && cw.scale && d.staging >= 0 && d.staging <= 2 && smgemm_i8_shape_ok(d, d.staging), kInvalidArgument,
               "plan tile 19 (smgemm_i8.hip, int8) needs the int8 weights, the scales and a single-source shape of the small-M GEMM with K <= %d "
               "(k=%d C0=%d C1=%d N=%d M=%d mode=%d)", kSmI8MaxK, d.ksize, d.C0, d.x1 ? d.C1 : 0, d.N, d.B * d.Ho * d.Wo, d.out_mode);
  // (nor has an int8 GEGLU descriptor: tile 20 takes it or nobody does)
  if (i8_geglu(d))
    SD_REQUIRE(conv_fast_path_ok(d) && cw.stream && cw.scale && d.staging >= 0 && d.staging <= 2 && smgeglu_i8_shape_ok(d, d.staging), kInvalidArgument,
               "plan tile 20 (smgeglu_i8.hip, int8) needs the int8 weights, the scales and an un-folded shape of the GEGLU kernel with K <= %d "
               "(k=%d C0=%d C1=%d N=%d M=%d mode=%d ln=%d)", kSmI8MaxK, d.ksize, d.C0, d.x1 ? d.C1 : 0, d.N, d.B * d.Ho * d.Wo, d.out_mode, d.ln_colsum ? 1 : 0);
  // (nor has an int8 q|k|v descriptor: tile 22 takes it or nobody does)
  if (i8_qkv(d))
    SD_REQUIRE(conv_fast_path_ok(d) && switches().qkv_i8 && cw.stream && cw.scale && d.staging >= 0 && d.staging <= 2 && smqkv_i8_shape_ok(d, d.staging),
               kInvalidArgument,
               "plan tile 22 (smqkv_i8.hip, int8) needs the int8 weights, the scales and an un-folded q|k|v shape of its tiles with K <= %d "
               "(k=%d C0=%d C1=%d N=%d n_trans=%d M=%d S=%d mode=%d ln=%d%s)", kSmI8MaxK, d.ksize, d.C0, d.x1 ? d.C1 : 0, d.N, d.n_trans,
               d.B * d.Ho * d.Wo, d.Ho * d.Wo, d.out_mode, d.ln_colsum ? 1 : 0, switches().qkv_i8 ? "" : "; SD_QKV_I8=0");
  // (nor has an int8 GEMM descriptor whose activations arrive quantized: tile 24 takes it or nobody does)
  if (i8_gemm_q(d))
    SD_REQUIRE(conv_fast_path_ok(d) && cw.stream && cw.scale && d.staging >= 0 && d.staging <= 2 && smgemm_q8_shape_ok(d, d.staging), kInvalidArgument,
               "plan tile 24 (smgemm_q8.hip, int8) needs the int8 weights, the scales and a single-source shape of the small-M GEMM with K <= %d "
               "(k=%d C0=%d C1=%d N=%d M=%d mode=%d)", kSmI8MaxK, d.ksize, d.C0, d.x1 ? d.C1 : 0, d.N, d.B * d.Ho * d.Wo, d.out_mode);
  // the sub-pixel upsampler holds the folded matrix and nothing else: tile 21 takes it or nobody does (no table row, no tuner candidate)
  if (d.subpix) {
    SD_REQUIRE(conv_fast_path_ok(d) && halo_sp_ok(d) && (d.tile == 0 || d.tile == 21), kInvalidArgument,
               "plan tile 21 (conv3x3_halo_sp.hip) does not take this conv: %s (k=%d stride=%d up=%d C0=%d C1=%d N=%d %dx%d tile=%d)",
               halo_sp_refusal(d) ? halo_sp_refusal(d) : "another tile is pinned", d.ksize, d.stride, d.up, d.C0, d.x1 ? d.C1 : 0, d.N, d.Hi, d.Wi, d.tile);
    const Dims a = dims_of(d);
    ConvPlan r{21, d.staging ? d.staging : 3, 1, false, 0};
    r.splitk = subpix_splits(d, a);
    r.slab = r.splitk > 1;
    r.workspace_bytes = slab_bytes(a, r.splitk, r.slab);
    return r;
  }
  if (!conv_fast_path_ok(d)) return ConvPlan{-1, 0, 1, false, 0};
  // a compressed weight source, in front of the tuner candidate, the tables and every rule: nothing moves it
  switch (cw.kind) {
    case WeightSource::Fp16: break;
    case WeightSource::PalWstream:
    case WeightSource::I8Wstream: {   // the code of tile 9
      const bool i8 = i8_stream(d);
      SD_REQUIRE(cw.stream && (i8 ? cw.scale != nullptr : cw.lut != nullptr) && can_split(d) && wstream_shape_ok(d), kInvalidArgument, "%s",
                 i8 ? "plan tile 17 (wstream.hip, int8) needs the int8 stream, the scales and a shape of the weight stream"
                    : "plan tile 14 (wstream.hip, palettized) needs the index stream, the LUT and a shape of the weight stream");
      ConvPlan r{i8 ? 17 : 14, d.staging, 1, true, 0};
      r.splitk = wstream_splits(d, wstream_waves(d.staging));
      r.workspace_bytes = slab_bytes(dims_of(d), r.splitk, true);
      return r;
    }
    case WeightSource::PalHalo:
    case WeightSource::I8Halo: {   // tile 7's ring code, split-K rule and slab arithmetic (checked above)
      const Dims a = dims_of(d);
      const Plan p = choose_plan(d, a);
      ConvPlan r{pal_halo(d) ? 25 : 18, p.staging, 1, true, 0};
      const int steps = a.Ctot / BK;
      r.splitk = cdiv(steps, cdiv(steps, p.splitk));
      r.slab = r.splitk > 1 || d.n_twins > 0;
      r.workspace_bytes = slab_bytes(a, r.splitk, r.slab);
      return r;
    }
    case WeightSource::PalGemm:   // the code of tile 12 in, the resolved tile height out; no workspace
      SD_REQUIRE(cw.stream && cw.lut && palette_bits_ok(cw.bits) && !d.x1 && d.staging >= 0 && d.staging <= 2 && smgemm_shape_ok(d, d.staging), kInvalidArgument,
                 "plan tile 15 (smgemm.hip, palettized) needs the index stream, the LUT and a single-source shape of the small-M GEMM");
      return ConvPlan{15, smgemm_bm(d, d.staging) == 32 ? 1 : 2, 1, false, 0};
    case WeightSource::I8Gemm:   // the code of tile 12 in, the resolved tile height out; no split-K, no slab, no workspace (checked above)
      return ConvPlan{19, smgemm_bm(d, d.staging) == 32 ? 1 : 2, 1, false, 0};
    case WeightSource::PalGeglu:   // the code of tile 13 in, the resolved tile height out (128 rows: code 1; 256 is not built)
      SD_REQUIRE(cw.stream && cw.lut && palette_bits_ok(cw.bits) && (cw.ln_gamma != nullptr) == (d.ln_colsum != nullptr) && smgeglu_pal_shape_ok(d, d.staging),
                 kInvalidArgument,
                 "plan tile 16 (smgeglu.hip, palettized) needs the index stream, the LUT, the norm weight with the LayerNorm fold and a shape of "
                 "the GEGLU kernel with 128-row tiles");
      return ConvPlan{16, 1, 1, false, 0};
    case WeightSource::I8Geglu:   // the code of tile 13 in, the resolved tile height out; no split-K, no slab, no workspace (checked above)
      return ConvPlan{20, smgeglu_bm(d, d.staging) == 128 ? 1 : 2, 1, false, 0};
    case WeightSource::I8Qkv:   // the tile height's code in (0 = by the grid), the resolved one out; no split-K, no slab, no workspace (checked above)
      return ConvPlan{22, smqkv_i8_bm(d, d.staging) == 128 ? 1 : 2, 1, false, 0};
    case WeightSource::I8GemmQ:   // as I8Gemm
      return ConvPlan{24, smgemm_bm(d, d.staging) == 32 ? 1 : 2, 1, false, 0};
  }
  const Switches& sw = switches();
  // the library's own rules for tiles 10-13 apply where nothing else was asked for (a tuner candidate in force also keeps them off)
  const bool free_choice = d.tile == 0 && d.splitk == 0 && d.staging == 0 && g_tune.tile == 0;
  // plan tile 10: the weight-stationary GEGLU kernel (wsgemm.hip) wherever its pre-tiled weights exist
  if (d.w_ws && wsgemm_shape_ok(d) && (d.tile == 10 || (sw.wsgemm && free_choice && wsgemm_wanted(d)))) return ConvPlan{10, 0, 1, false, 0};
  SD_REQUIRE(d.tile != 10, kInvalidArgument, "plan tile 10 (wsgemm.hip) needs the pre-tiled weights and an eligible GEGLU shape");
  // plan tile 11: weights global -> VGPR (bvgemm.hip), on the library's rule or forced (the code then forces a variant)
  if (sw.bvgemm && d.w_bv && free_choice && bvgemm_wanted(d)) return ConvPlan{11, 0, 1, false, 0};
  if (d.tile == 11) {
    SD_REQUIRE(d.w_bv && bvgemm_shape_ok(d), kInvalidArgument, "plan tile 11 (bvgemm.hip) needs the pre-tiled weights and an eligible 1x1 shape");
    return ConvPlan{11, d.staging, 1, false, 0};
  }
  // plan tiles 12 (smgemm.hip) / 13 (smgeglu.hip): the code of a forced plan forces a tile height (the launchers check its shape)
  if (d.tile == 12 || (sw.smgemm && free_choice && smgemm_wanted(d))) return ConvPlan{12, d.tile == 12 ? d.staging : 0, 1, false, 0};
  if (d.tile == 13 || (sw.smgeglu && free_choice && smgeglu_wanted(d))) return ConvPlan{13, d.tile == 13 ? d.staging : 0, 1, false, 0};

  const Dims a = dims_of(d);
  Plan p = choose_plan(d, a);
  const bool twins = d.n_twins > 0;
  if (d.gnf_partial && d.ksize == 3) {   // GroupNorm(+SiLU) applied in the halo loader of the K-split 3x3 kernel (GNL)
    SD_REQUIRE(conv_gn_loader_ok(d) && d.gnf_silu == 1 && d.gnf_gamma && d.gnf_beta && d.gnf_entries >= 1 && d.gnf_entries <= 128 && !twins, kInvalidArgument,
               "GroupNorm in the conv loader: Ctot=%d groups=%d entries=%d up=%d", a.Ctot, d.gnf_groups, d.gnf_entries, d.up);
    p.tile = 7;
    if (p.staging != 2 && p.staging != 3) p.staging = 3;
    p.splitk = 1;
  } else if (d.gnf_partial) {   // GroupNorm folded into this 1x1 GEMM: gemm_pipe_kernel's 64 x 64 tile (the only GNF instantiation)
    SD_REQUIRE(d.ksize == 1 && d.stride == 1 && !d.x1 && d.out_mode == kOutHalf && !d.ln_colsum && !d.out_t && !twins &&
                   gemm_pipe_ok(d.ksize, d.stride, d.up, a.M, a.N, a.K, d.C0, 0) &&
                   d.gnf_gamma && d.gnf_beta && d.gnf_groups >= 1 && d.gnf_groups <= 32 && a.K % d.gnf_groups == 0 && a.K <= 2048 &&
                   d.gnf_entries >= 1 && d.gnf_entries <= 128 && a.HoWo % 64 == 0,
               kInvalidArgument, "GroupNorm fold: K=%d groups=%d entries=%d HoWo=%d", a.K, d.gnf_groups, d.gnf_entries, a.HoWo);
    p.tile = 3;
    if (p.staging != 6 && p.staging != 7 && p.staging != 8) p.staging = 6;
    p.splitk = 1;
  }
  ConvPlan r{p.tile, p.staging, 1, true, 0};
  if (p.tile == 9) {   // weight-streaming kernel: one slab per nw input-channel slices, always through the combine
    r.splitk = wstream_splits(d, wstream_waves(p.staging));
  } else {             // no empty splits
    const int steps = p.tile == 7 ? a.Ctot / BK : a.nk_total;
    r.splitk = cdiv(steps, cdiv(steps, p.splitk));
    r.slab = r.splitk > 1 || twins;
  }
  r.workspace_bytes = slab_bytes(a, r.splitk, r.slab);
  return r;
}

// THE decode of the wire format: what (tile, staging) launch for this descriptor.  Every per-family meaning of `staging` is here.
//   tiles 1-4: 0 = 2 stages, 1 = register staging, 2 / 3 / 4 / 5 = ring of 3 / 4 / 6 / 8 stages; 6 / 7 / 8 = gemm_pipe_kernel with 3 / 4 / 2
//              stages where gemm_pipe_ok, else as 3; 12 / 13 = the 3- / 4-stage ring with in-workgroup split-K (two K groups) where the
//              epilogue is the plain one, a split runs >= 4 K steps and two rings fit, else as 2 / 3.  A ring that does not fit the LDS
//              runs as the deepest shallower one that does.  The LayerNorm fold has no register staging (1 as 0); the token-transposed
//              output (kOutHalfT) has register staging and rings of 2 / 3 stages only.
//   tile 7:    0 / 2 / 3 / 4 / 5 = 2 / 3 / 4 / 6 / 8 weight stages; GroupNorm in the loader: 4 stages from code 3 where its table fits, else 3
//   tile 18:   tile 7's codes; the int8 kernel has rings of 2 / 3 / 4 stages, a deeper code runs the 4-stage one
//   tile 25:   tile 7's codes and depths as they are (no GroupNorm loader)
//   tile 21:   tile 7's codes; the sub-pixel kernel has rings of 3 / 4 stages: 2 = 3 stages, anything else 4
//   tiles 9 / 14 / 17: 4 = four waves per workgroup, anything else eight      tile 11: 1-6 = the variant, anything else the library's choice
//   tiles 12 / 15 / 19 / 24 / 13 / 16 / 20 / 22: 1 / 2 = the lower / higher tile (32 / 64, 128 / 256 rows), 0 = by the shape
void decode_plan(const ConvDesc& d, ConvPlan& p) {
  const Dims a = dims_of(d);
  int code = p.staging;
  switch (p.tile) {
    case -1: p.kernel = ConvKernel::Generic; return;
    case 9: case 14: case 17:
      p.kernel = p.tile == 9 ? ConvKernel::Wstream : p.tile == 14 ? ConvKernel::WstreamPal : ConvKernel::WstreamI8;
      p.waves = wstream_waves(code);
      return;
    case 10: p.kernel = ConvKernel::Wsgemm; return;
    case 11:
      p.kernel = ConvKernel::Bvgemm;
      p.variant = code >= 1 && code <= 6 ? code : bvgemm_auto_variant(d);
      return;
    case 12: case 15: case 19: case 24:
      p.kernel = p.tile == 12 ? ConvKernel::Smgemm : p.tile == 15 ? ConvKernel::SmgemmPal : p.tile == 19 ? ConvKernel::SmgemmI8 : ConvKernel::SmgemmQ8;
      p.bm = code >= 0 && code <= 2 ? smgemm_bm(d, code) : 0;   // (0: no such tile - the launcher refuses it)
      return;
    case 13: case 16: case 20:
      p.kernel = p.tile == 13 ? ConvKernel::Smgeglu : p.tile == 16 ? ConvKernel::SmgegluPal : ConvKernel::SmgegluI8;
      p.bm = code >= 0 && code <= 2 ? smgeglu_bm(d, code) : 0;
      return;
    case 22:
      p.kernel = ConvKernel::SmqkvI8;
      p.bm = code >= 0 && code <= 2 ? smqkv_i8_bm(d, code) : 0;
      return;
    default: break;
  }
  if (p.tile == 18) {
    tile_dims(7, p.bm, p.bn);
    p.kernel = ConvKernel::HaloI8;
    p.stages = code >= 3 ? 4 : code == 2 ? 3 : 2;
    return;
  }
  if (p.tile == 25) {
    tile_dims(7, p.bm, p.bn);
    p.kernel = ConvKernel::HaloPal;
    p.stages = code >= 5 ? 8 : code == 4 ? 6 : code == 3 ? 4 : code == 2 ? 3 : 2;
    return;
  }
  if (p.tile == 21) {
    tile_dims(7, p.bm, p.bn);
    p.kernel = ConvKernel::HaloSubpix;
    p.stages = code == 2 ? 3 : 4;
    return;
  }
  tile_dims(p.tile, p.bm, p.bn);
  if (p.tile == 7) {
    p.kernel = ConvKernel::HaloKs;
    if (d.gnf_partial) p.stages = code >= 3 && halo_gnl_lds_bytes(4, a.Ctot) <= kLdsBudget ? 4 : 3;
    else p.stages = code >= 5 ? 8 : code == 4 ? 6 : code == 3 ? 4 : code == 2 ? 3 : 2;
    return;
  }
  p.kernel = ConvKernel::Igemm;
  p.stages = 2;
  const bool lnf = d.ln_colsum != nullptr;
  auto fits = [&](int nst, int kgroups = 1) { return ring_fits(p.bm, p.bn, nst, kgroups); };
  if (lnf && code == 1) code = 0;
  if (code == 1) {
    p.reg_staged = true;
    return;
  }
  if (!lnf && d.out_mode == kOutHalfT) {
    if (code >= 2) p.stages = 3;
    return;
  }
  if (code == 12 || code == 13) {
    const bool two_groups = !lnf && cdiv(a.nk_total, p.splitk) >= 4;
    if (two_groups && code == 13 && fits(4, 2)) p.stages = 4, p.kgroups = 2;
    else if (two_groups && fits(3, 2)) p.stages = 3, p.kgroups = 2;
    if (p.kgroups == 2) return;
    code -= 10;
  }
  // (a GroupNorm-folded 1x1 arrives here as tile 3 with code 6 / 7 / 8 and gemm_pipe_ok checked: gemm_pipe_kernel's GNF instantiation)
  if (code >= 6 && code <= 8 && gemm_pipe_ok(d.ksize, d.stride, d.up, a.M, a.N, a.K, d.C0, d.x1 ? d.C1 : 0)) {
    p.kernel = ConvKernel::GemmPipe;
    p.stages = code == 8 ? 2 : (code == 7 && fits(4)) ? 4 : 3;
    return;
  }
  if (code >= 6) code = 3;
  const int asked = code >= 5 ? 8 : code == 4 ? 6 : code == 3 ? 4 : code == 2 ? 3 : 2;
  for (int nst : {8, 6, 4, 3, 2})
    if (nst <= asked && fits(nst)) {
      p.stages = nst;
      return;
    }
}

}  // namespace

ConvPlan conv_plan(const ConvDesc& d) {
  ConvPlan p = plan_codes(d);
  decode_plan(d, p);
  return p;
}

std::string conv_plan_kernel_name(const ConvPlan& p) {
  const std::string tile = std::to_string(p.bm) + "x" + std::to_string(p.bn), ring = " ring" + std::to_string(p.stages);
  switch (p.kernel) {
    case ConvKernel::Igemm: return "igemm " + tile + ring + (p.kgroups == 2 ? " kg2" : "") + (p.reg_staged ? " regs" : "");
    case ConvKernel::GemmPipe: return "gemm_pipe " + tile + ring;
    case ConvKernel::HaloKs: return "halo_ks" + ring;
    case ConvKernel::HaloI8: return "halo_i8" + ring;
    case ConvKernel::HaloPal: return "halo_pal" + ring;
    case ConvKernel::HaloSubpix: return "conv3x3_halo_sp" + ring;
    case ConvKernel::Wstream: return "wstream waves" + std::to_string(p.waves);
    case ConvKernel::WstreamPal: return "wstream_pal waves" + std::to_string(p.waves);
    case ConvKernel::WstreamI8: return "wstream_i8 waves" + std::to_string(p.waves);
    case ConvKernel::Wsgemm: return "wsgemm";
    case ConvKernel::Bvgemm: return "bvgemm v" + std::to_string(p.variant);
    case ConvKernel::Smgemm: return "smgemm bm" + std::to_string(p.bm);
    case ConvKernel::SmgemmPal: return "smgemm_pal bm" + std::to_string(p.bm);
    case ConvKernel::SmgemmI8: return "smgemm_i8 bm" + std::to_string(p.bm);
    case ConvKernel::SmgemmQ8: return "smgemm_q8 bm" + std::to_string(p.bm);
    case ConvKernel::Smgeglu: return "smgeglu bm" + std::to_string(p.bm);
    case ConvKernel::SmgegluPal: return "smgeglu_pal bm" + std::to_string(p.bm);
    case ConvKernel::SmgegluI8: return "smgeglu_i8 bm" + std::to_string(p.bm);
    case ConvKernel::SmqkvI8: return "smqkv_i8 bm" + std::to_string(p.bm);
    default: return "generic";
  }
}

// Workspace a handle reserves for this conv at build time.  The descriptor may still change before it is launched - the GroupNorm
// hook attaches statistics or twins, a tuner candidate or a run-time table row changes the split - so this is the split-K plan of
// the tiled kernels with head room, an upper bound of conv_plan(d).workspace_bytes for every plan the descriptor can later get:
//   - under SD_TUNE (tools/tune_plans.py), room for the 16 splits of any candidate of the sweep;
//   - with the weight-stream copy present, its slab count at four waves per workgroup (the most slabs it writes);
//   - the unresolved split-K (the launch may use fewer splits), one slab when only the GroupNorm twins ask for it.
size_t conv_workspace_bytes(const ConvDesc& d) {
  if (!conv_fast_path_ok(d) || pal_gemm(d) || pal_geglu(d) || i8_gemm(d) || i8_geglu(d) || i8_qkv(d) || i8_gemm_q(d)) return 0;   // (tiles 15 / 16 / 19 / 20 / 22 / 24: no slabs)
  const Dims a = dims_of(d);
  if (d.subpix) return halo_sp_ok(d) ? slab_bytes(a, subpix_splits(d, a), false) : 0;   // (tile 21: pinned, no candidate or table row moves its split)
  const Plan p = choose_plan(d, a);
  int splits = (switches().tuning && can_split(d)) ? std::max(p.splitk, 16) : p.splitk;
  const bool stream = can_stream(d) || ((pal_stream(d) || i8_stream(d)) && can_split(d) && wstream_shape_ok(d));   // tiles 14 / 17 as tile 9
  if (stream) splits = std::max(splits, wstream_splits(d, 4));
  return slab_bytes(a, splits, d.n_twins > 0 || stream);
}

ConvWeightCopies conv_plan_copies(const ConvDesc& d0) {
  ConvWeightCopies c{false, false, false};
  if (!conv_fast_path_ok(d0) || d0.subpix) return c;   // (tile 21 reads the folded matrix alone)
  ConvDesc d = d0;
  d.w_tiled = d.w_ws = d.w_bv = nullptr;
  const Switches& sw = switches();
  const int k = d.ksize, M = d.B * d.Ho * d.Wo;
  // small-M layers: the weight-streaming kernel (plan tile 9) needs the fragment-major copy of the weights
  // (SD_TUNE: every shape a plan sweep may send there; production: exactly the convs whose plan IS tile 9)
  const bool ws_candidate = sw.tuning ? ((k == 3 && M <= 512) || (k == 1 && M <= 128)) : plan_is_wstream(d);
  c.wstream = sw.wstream && wstream_shape_ok(d) && ws_candidate;
  // widest-M GEGLU projection (K = 320): the weight-stationary kernel reads its own fragment-major copy (wsgemm.hip)
  c.wsgemm = sw.wsgemm && wsgemm_wanted(d);
  // large-M 1x1 GEMMs: weights global -> VGPR (bvgemm.hip) reads its own fragment-major copy; tile 10 comes first in conv_plan
  c.bvgemm = sw.bvgemm && !c.wsgemm && bvgemm_wanted(d);
  return c;
}

namespace {
// the plan of this conv run from fp16 with the pre-tiled copies `c` present (conv_plan only tests the pointers)
ConvPlan fp16_plan(const ConvDesc& d0, const ConvWeightCopies& c) {
  static const half_t present = 0;
  ConvDesc d = d0;
  d.cw = CompressedWeights{};
  d.w_tiled = c.wstream ? &present : nullptr;
  d.w_ws = c.wsgemm ? &present : nullptr;
  d.w_bv = c.bvgemm ? &present : nullptr;
  return conv_plan(d);
}
}  // namespace

WeightPin conv_plan_pin(WeightSource kind, int n) {
  switch (kind) {
    case WeightSource::PalWstream: return {kind, 14, n == 4 ? 4 : 0};
    case WeightSource::I8Wstream: return {kind, 17, n == 4 ? 4 : 0};
    case WeightSource::I8Halo: return {kind, 18, n};   // n: tile 7's ring code as it is
    case WeightSource::PalHalo: return {kind, 25, n};  // the same
    case WeightSource::PalGemm: return {kind, 15, n == 32 ? 1 : n == 64 ? 2 : 0};
    case WeightSource::I8Gemm: return {kind, 19, n == 32 ? 1 : n == 64 ? 2 : 0};
    case WeightSource::PalGeglu: return {kind, 16, n == 128 ? 1 : n == 256 ? 2 : 0};
    case WeightSource::I8Geglu: return {kind, 20, n == 128 ? 1 : n == 256 ? 2 : 0};
    case WeightSource::I8Qkv: return {kind, 22, n == 128 ? 1 : n == 256 ? 2 : 0};
    case WeightSource::I8GemmQ: return {kind, 24, n == 32 ? 1 : n == 64 ? 2 : 0};
    default: return {};
  }
}

// conv_plan itself answers each question (one predicate: an A/B switch, a tuner candidate, a forced plan, GroupNorm statistics asked
// of the conv or a shape the twin's own rule refuses all give another kernel there).
WeightPin conv_plan_weights(const ConvDesc& d, StoredWeights held, bool opt_in, bool pal_halo_on) {
  if (held == StoredWeights::Fp16 || !conv_fast_path_ok(d)) return {};
  const Switches& sw = switches();
  const bool palette = held == StoredWeights::Palette, one_by_one = opt_in && palette && d.ksize == 1 && !d.x1;
  if (one_by_one && d.out_mode == kOutGeglu && sw.smgeglu) {   // tile 13, on the 128-row tiles the palettized kernel has
    const ConvPlan p = fp16_plan(d, conv_plan_copies(d));
    if (p.kernel == ConvKernel::Smgeglu && smgeglu_pal_shape_ok(d, 0)) return conv_plan_pin(WeightSource::PalGeglu, p.bm);
  }
  // tile 13 at either tile height, for the int8 kernel that reads the LayerNorm's int8 output: asked with the fold's fields (the fp16
  // plan of the call site) or without them - the answer's descriptor never carries them
  if (opt_in && held == StoredWeights::W8A8 && d.ksize == 1 && !d.x1 && d.out_mode == kOutGeglu && sw.smgeglu) {
    const ConvPlan p = fp16_plan(d, conv_plan_copies(d));
    ConvDesc plain = d;
    plain.ln_colsum = nullptr;
    if (p.kernel == ConvKernel::Smgeglu && smgeglu_i8_shape_ok(plain, p.bm == 128 ? 1 : 2)) return conv_plan_pin(WeightSource::I8Geglu, p.bm);
  }
  // a plain projection whose producer hands it int8 activations (d.x0_i8: ff.net.2 behind the GEGLU), for the int8 kernel that streams
  // them: no fp16 twin to follow either - the rule of smgemm_q8_wanted alone, behind the switch that takes tile 12 away
  if (opt_in && held == StoredWeights::W8A8 && d.ksize == 1 && !d.x1 && d.out_mode == kOutHalf && d.n_trans == 0 && d.x0_i8) {
    if (sw.smgemm && !d.ln_colsum && smgemm_q8_wanted(d)) return conv_plan_pin(WeightSource::I8GemmQ, smgemm_bm(d, 0));
    return {};
  }
  // the fused q|k|v launch (V columns transposed), for the int8 kernel that reads norm1's int8 output: no fp16 twin to follow - the
  // shape rule alone, asked of the descriptor without the fold's fields, at the height the grid gives
  if (opt_in && held == StoredWeights::W8A8 && d.ksize == 1 && !d.x1 && d.out_mode == kOutHalf && d.n_trans > 0 && sw.qkv_i8) {
    ConvDesc plain = d;
    plain.ln_colsum = nullptr;
    if (smqkv_i8_shape_ok(plain, 0)) return conv_plan_pin(WeightSource::I8Qkv, smqkv_i8_bm(plain, 0));
    return {};
  }
  // tile 9 with the fragment-major copy present: its wave count, i.e. its slab count
  if (sw.wstream && !d.ln_colsum && plan_is_wstream(d)) {
    const ConvPlan p = fp16_plan(d, {true, false, false});
    if (p.kernel == ConvKernel::Wstream) return conv_plan_pin(palette ? WeightSource::PalWstream : WeightSource::I8Wstream, p.waves);
  }
  if (one_by_one && d.out_mode == kOutHalf && sw.smgemm && !d.ln_colsum) {   // tile 12
    const ConvPlan p = fp16_plan(d, conv_plan_copies(d));
    if (p.kernel == ConvKernel::Smgemm) return conv_plan_pin(WeightSource::PalGemm, p.bm);
  }
  if (opt_in && held == StoredWeights::W8A8 && d.ksize == 1 && !d.x1 && d.out_mode == kOutHalf && sw.smgemm && !d.ln_colsum) {   // tile 12, as above
    const ConvPlan p = fp16_plan(d, conv_plan_copies(d));
    if (p.kernel == ConvKernel::Smgemm && smgemm_i8_shape_ok(d, 0)) return conv_plan_pin(WeightSource::I8Gemm, p.bm);
  }
  const bool i8h = held == StoredWeights::W8A8 && halo_i8_ok(d), palh = palette && pal_halo_on && halo_pal_ok(d);
  if (i8h || palh) {   // tile 7 without the GroupNorm loader: its ring code and resolved split-K
    const ConvPlan p = fp16_plan(d, conv_plan_copies(d));
    if (p.kernel == ConvKernel::HaloKs) {
      WeightPin pin = conv_plan_pin(i8h ? WeightSource::I8Halo : WeightSource::PalHalo, p.staging);
      pin.splitk = p.splitk;
      return pin;
    }
  }
  return {};
}

// Does the compiled-in plan table hold a row for this shape - a plan that was measured in a step?
bool conv_plan_is_tuned(const ConvDesc& d) {
  if (!conv_fast_path_ok(d)) return false;
  const Dims a = dims_of(d);
  for (int i = 0; i < kNumTuned; ++i)
    if (table_match(kTuned[i], d, a)) return true;
  return false;
}

// sd_tune_set_plan_table: replace the run-time table by the rows of `text` (tuned_convs.inc format, one per line) - how
// tools/tune_e2e.py tries one plan after another against the graph replay time of the whole step in ONE process
int conv_plan_table_set(const char* text) {
  std::vector<TunedConv>& t = runtime_table();
  t.clear();
  if (!text) return 0;
  const char* p = text;
  while (*p) {
    const char* e = strchr(p, '\n');
    std::string line(p, e ? (size_t)(e - p) : strlen(p));
    TunedConv r;
    if (parse_plan_row(line.c_str(), r)) t.push_back(r);
    if (!e) break;
    p = e + 1;
  }
  return (int)t.size();
}

void conv_tune_set_candidate(int tile, int staging, int splitk) {
  g_tune.tile = tile;
  g_tune.staging = staging;
  g_tune.splitk = splitk;
}

void conv_plan_log(const ConvDesc& d, const ConvPlan& p, int n_fast) {
  static const bool on = tune_env_set("SD_LOG_CONVS");
  if (!on) return;
  const Dims a = dims_of(d);
  const int c1 = d.x1 ? d.C1 : 0;
  if (p.tile == 9 || p.tile == 14 || p.tile == 17)
    fprintf(stderr, "[sd conv] k%d up%d C0=%d C1=%d M=%d N=%d K=%d tile=%d nw=%d slabs=%d twins=%d bits=%d\n", d.ksize, d.up, d.C0, c1, a.M, a.N,
            a.K, p.tile, p.waves, p.splitk, d.n_twins, p.tile == 14 ? d.cw.bits : p.tile == 17 ? 8 : 16);
  else if (p.tile == 12 || p.tile == 13)
    fprintf(stderr, "[sd conv] k1 s1 up1 C0=%d C1=%d M=%d N=%d K=%d mode=%d tile=%d bm=%d n_fast=%d\n", d.C0, c1, a.M, a.N, a.K, d.out_mode, p.tile, p.bm,
            n_fast);
  else if (p.tile == 15 || p.tile == 16)
    fprintf(stderr, "[sd conv] k1 s1 up1 C0=%d C1=%d M=%d N=%d K=%d mode=%d tile=%d bm=%d n_fast=%d bits=%d\n", d.C0, c1, a.M, a.N, a.K, d.out_mode,
            p.tile, p.bm, n_fast, d.cw.bits);
  else if (p.tile == 19 || p.tile == 20 || p.tile == 22 || p.tile == 24)
    fprintf(stderr, "[sd conv] k1 s1 up1 C0=%d C1=%d M=%d N=%d K=%d mode=%d tile=%d bm=%d n_fast=%d bits=8\n", d.C0, c1, a.M, a.N, a.K, d.out_mode, p.tile,
            p.bm, n_fast);
  else if (p.tile == 25)
    fprintf(stderr, "[sd conv] k%d s%d up%d C0=%d C1=%d M=%d N=%d K=%d mode=%d tile=%d splitk=%d bits=%d\n", d.ksize, d.stride, d.up, d.C0, c1, a.M, a.N,
            a.K, d.out_mode, p.tile, p.splitk, d.cw.bits);
  else if (p.tile == 18)
    fprintf(stderr, "[sd conv] k%d s%d up%d C0=%d C1=%d M=%d N=%d K=%d mode=%d tile=%d splitk=%d bits=8\n", d.ksize, d.stride, d.up, d.C0, c1, a.M, a.N,
            a.K, d.out_mode, p.tile, p.splitk);
  else if (p.tile == 21)
    fprintf(stderr, "[sd conv] k%d s%d up%d C0=%d C1=%d M=%d N=%d K=%d mode=%d tile=%d splitk=%d subpix K'=%d\n", d.ksize, d.stride, d.up, d.C0, c1, a.M,
            a.N, a.K, d.out_mode, p.tile, p.splitk, 4 * a.Ctot);
  else
    fprintf(stderr, "[sd conv] k%d s%d up%d C0=%d C1=%d M=%d N=%d K=%d mode=%d tile=%d splitk=%d\n", d.ksize, d.stride, d.up, d.C0, c1, a.M, a.N,
            a.K, d.out_mode, p.tile, p.splitk);
}

bool choose_tile_order(double a_bytes, double w_bytes, double nbm, double nbn, bool ab_switch) {
  const double l2 = 3.5e6;   // what one 4-MB L2 keeps of an operand next to the other one's stream
  const double m_fast_cost = w_bytes + a_bytes * (a_bytes <= l2 ? std::min(8.0, nbn) : nbn);
  const double n_fast_cost = a_bytes + w_bytes * (w_bytes <= l2 ? std::min(8.0, nbm) : nbm);
  static const int forced = tune_env_int("SD_TILE_ORDER", -1);   // A/B switch: 0 / 1 / 2
  if (ab_switch && forced == 2) return nbn > 1 && a_bytes * (nbn - 1) > 7.0 * w_bytes;
  if (ab_switch && forced >= 0) return forced != 0;
  return nbn > 1 && n_fast_cost < m_fast_cost;
}

bool conv_reduce_stats_on() { return switches().reduce_stats; }

}  // namespace sd
