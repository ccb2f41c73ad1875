// Operator-level sd_op_* entry points of libsdmi355 (include/sd_mi355x.h): each drives one kernel, or one short launch sequence of
// the UNet graph, from host tensors in the reference's layouts, so that a test can pin it against the oracle.  The weights go
// through the layout rules of weight_prep.h - the ones the UNet builder applies - before they reach the device.
//
// Plan codes of the entry points (A/B testing and tuning tools; the header describes them for callers):
//   conv `tile` (sd_op_conv2d, _conv2d_ex, _groupnorm, _groupnorm_proj, _groupnorm_conv3x3): plan tile = tile % 10, staging = tile / 10
//     tile    0 the library's plan, 1 128x128, 2 128x64, 3 64x64, 4 64x128, 7 the 3x3 halo kernel, 9 wstream.hip (needs w_tiled)
//     staging the code that goes with the tile (ring depth, register staging, the pipelined kernel, in-workgroup split-K, wave count):
//             decoded by decode_plan (conv_plan.cpp) and nowhere else; sd_op_conv_plan_kernel names the kernel a pair launches
//     sd_op_conv2d / sd_op_conv2d_ex alone: 110-116 plan tile 11 (bvgemm.hip: its own choice / variants 1-6, needs w_bv),
//                                           140-142 plan tile 12 (smgemm.hip: tile height by M / 32 rows / 64 rows)
//     (plan tiles 14 / 15 read palettized weights: sd_op_conv2d_palettized / sd_op_gemm_palettized; plan tile 17 int8 ones: sd_op_conv2d_w8a8)
//     sd_op_conv2d_ex is sd_op_conv2d with the ConvDesc fields the UNet / VAE builders set on top (second source, timestep embedding,
//     the encoder's explicit padding, one GroupNorm twin) and reads the plan that ran back: plan_out = {tile, staging, splitk, slab}
//   sd_op_geglu_ln `kernel`: 0 the library's plan, 1 the tiled igemm / gemm_pipe kernels, 2 plan tile 10 (wsgemm.hip),
//     2 + 10 n ablation build n of that kernel, 3-9 plan tile 11 (bvgemm.hip: its own choice / variants 1-6),
//     100 plan tile 13 (smgeglu.hip) with the tile height by the grid size, 101 / 102 its 128- / 256-row tiles,
//     110-112 the same through the phase-clock build, which prints its table
//   sd_op_qkv_ln `kernel`: 0 the library's plan, 1 the tiled kernels, 2 plan tile 10 (wsgemm.hip), 3 plan tile 11 (bvgemm.hip:
//     its own choice), 4 + v its variant v + 1
//   sd_op_ffn_out_proj `fused`: 0 two 1x1 GEMMs, 1 one launch (xattn_out.hip ffn_proj), 2-5 the merged tail (wfold.hip, then ONE
//     two-source GEMM): 2 the library's plan, 3 igemm_kernel's 64x64 tile, 4 / 5 smgemm.hip's 32- / 64-row tiles
//   sd_op_attention `variant`: 0 default dispatch, 1 never the software-pipelined d = 64 kernel (attention8.hip), 2 that kernel with
//     pre-scaled q, 3 default dispatch with q and k as rows of ONE [B][S][2C] buffer (ldq = ldk = 2C, what a handle's self-attention
//     reads; Sq == Sk), 100 + u its balanced form with u units per workgroup (0: the launch's own split)
//     (sd_op_attention_kernel names the kernel a shape and variant launch: attention_op_desc below builds the descriptor for both)
//
// Device buffers: every one comes from the entry point's Scratch (capi_util.h) - guards of 0xff in front and behind, outputs and
// workspaces poisoned, every guard checked when the scratch leaves scope.  No entry point allocates device memory any other way.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <initializer_list>

#include "capi_util.h"
#include "conv_plan.h"
#include "weight_prep.h"

namespace sd {
namespace {

const half_t* f16(const void* p) { return reinterpret_cast<const half_t*>(p); }

// (B, C, H, W) f16 on the host -> [B][H][W][C] on the device
half_t* upload_nhwc(Scratch& sc, const void* x, int B, int C, int H, int W) {
  const half_t* src = f16(x);
  std::vector<half_t> t((size_t)B * C * H * W);
  for (int b = 0; b < B; ++b)
    for (int c = 0; c < C; ++c)
      for (int p = 0; p < H * W; ++p) t[((size_t)b * H * W + p) * C + c] = src[((size_t)b * C + c) * H * W + p];
  return sc.dev<half_t>(t.size(), t.data());
}
// BC1S (B, C, 1, S) -> token-major [B * S][C]: NCHW with H = 1, W = S
half_t* upload_tokens(Scratch& sc, const void* x, int B, int C, int S) { return upload_nhwc(sc, x, B, C, 1, S); }

// (B, C, 1, Sk) -> V^T [B][C][ldv], rows zero-padded; perm: the middle 4-key blocks of every 16 keys swapped (AttnDesc::vt_perm)
half_t* upload_vt(Scratch& sc, const void* v, int B, int C, int Sk, int ldv, bool perm) {
  const half_t* src = f16(v);
  std::vector<half_t> t((size_t)B * C * ldv, (half_t)0);
  for (size_t r = 0; r < (size_t)B * C; ++r)
    for (int s = 0; s < Sk; ++s) {
      const int o = s & 15;
      t[r * ldv + (perm && o >= 4 && o < 12 ? s + (o < 8 ? 4 : -4) : s)] = src[r * Sk + s];
    }
  return sc.dev<half_t>(t.size(), t.data());
}

// device [B][H][W][C] -> (B, C, H, W) f16 host buffer
void download_nchw(const half_t* dev, void* out, int B, int C, int H, int W) {
  std::vector<half_t> t((size_t)B * C * H * W);
  SD_HIP(hipMemcpy(t.data(), dev, t.size() * 2, hipMemcpyDeviceToHost));
  half_t* dst = reinterpret_cast<half_t*>(out);
  for (int b = 0; b < B; ++b)
    for (int c = 0; c < C; ++c)
      for (int p = 0; p < H * W; ++p) dst[((size_t)b * C + c) * H * W + p] = t[((size_t)b * H * W + p) * C + c];
}
void download_tokens(const half_t* dev, void* out, int B, int C, int S) { download_nchw(dev, out, B, C, 1, S); }

// [Cout][Cin][k][k] f16 -> [Cout][k][k][Cin] on the device
half_t* upload_conv_weight(Scratch& sc, const void* w, int cout, int cin, int k) {
  std::vector<half_t> t((size_t)cout * cin * k * k);
  retile_ohwi(f16(w), cout, cin, k, false, t.data());
  return sc.dev<half_t>(t.size(), t.data());
}

// a projection [cout][cin] f16 with the LayerNorm in front of it folded in (gamma == beta == NULL: none to fold)
struct FoldedProj {
  half_t* w;
  float *bias, *colsum;
};
FoldedProj upload_ln_folded(Scratch& sc, const void* w, const float* bias, const float* gamma, const float* beta, int cout, int cin,
                            bool geglu) {
  std::vector<half_t> wf((size_t)cout * cin);
  std::vector<float> bf(cout), cs(cout);
  fold_layernorm_rows(f16(w), bias, gamma, beta, cout, cin, 0, geglu, wf.data(), cs.data(), bf.data());
  return {sc.dev<half_t>(wf.size(), wf.data()), sc.dev<float>(cout, bf.data()), sc.dev<float>(cout, cs.data())};
}

// GroupNorm partial buffer, poisoned: a consumer must only read what the producer wrote (1e30, finite: a folded statistic comes
// out wrong, not NaN)
float* poisoned_gn_partial(Scratch& sc, int B, int HW, int groups) {
  std::vector<float> poison(groupnorm_scratch_floats(B, HW, groups), 1.0e30f);
  return sc.dev<float>(poison.size(), poison.data(), "GroupNorm partials");
}

// split-K workspace large enough for every one of these launches; poisoned, as a handle reuses its workspace dirty: a slab that is
// combined without having been written shows
ConvWorkspace workspace_for(Scratch& sc, std::initializer_list<ConvDesc> descs) {
  ConvWorkspace ws;
  for (const ConvDesc& d : descs) ws.partial_bytes = std::max(ws.partial_bytes, conv_workspace_bytes(d));
  if (ws.partial_bytes) ws.partial = reinterpret_cast<float*>(sc.out<char>(ws.partial_bytes, "split-K workspace"));
  return ws;
}

// stride-1 conv that keeps the image size (ksize 1: a GEMM over the pixels)
ConvDesc conv_desc(const half_t* in, int cin, const half_t* w, const float* bias, const half_t* res, half_t* out, int B, int H, int W,
                   int N, int ksize = 1) {
  ConvDesc d;
  d.x0 = in; d.C0 = cin; d.w = w; d.bias = bias; d.res = res; d.out = out;
  d.B = B; d.Hi = H; d.Wi = W; d.Ho = H; d.Wo = W;
  d.ksize = ksize; d.N = N;
  return d;
}
// 1x1 GEMM over [B][1][S] tokens
ConvDesc token_gemm(const half_t* in, int cin, const half_t* w, const float* bias, const half_t* res, half_t* out, int B, int S, int N) {
  return conv_desc(in, cin, w, bias, res, out, B, 1, S, N);
}

// conv `tile` code -> plan tile + staging (table at the top); gemm_codes: the 1x1-GEMM ranges sd_op_conv2d alone accepts
void apply_tile_code(ConvDesc& d, int code, bool gemm_codes = false) {
  d.tile = code % 10;
  d.staging = code / 10;
  if (gemm_codes && code >= 110 && code <= 116) d.tile = 11, d.staging = code - 110;
  if (gemm_codes && code >= 140 && code <= 142) d.tile = 12, d.staging = code - 140;
}

// the pre-tiled weight copies a forced plan reads: tile 9 w_tiled (wstream.hip), tile 10 w_ws (wsgemm.hip), tile 11 w_bv (bvgemm.hip)
int concat_channels(const ConvDesc& d) { return d.C0 + (d.x1 ? d.C1 : 0); }
void tile_for_wstream(Scratch& sc, ConvDesc& d, const char* refusal) {
  SD_REQUIRE(wstream_shape_ok(d), kInvalidArgument, "%s", refusal);
  half_t* wtd = sc.out<half_t>(wstream_tiled_halves(d.N, concat_channels(d), d.ksize), "w_tiled (wstream.hip copy)");
  launch_wstream_retile(d.w, wtd, d.N, concat_channels(d), d.ksize, sc.stream);
  d.w_tiled = wtd;
}
void tile_for_wsgemm(Scratch& sc, ConvDesc& d) {
  half_t* wtd = sc.out<half_t>(wsgemm_tiled_halves(d.N), "w_ws (wsgemm.hip copy)");
  launch_wsgemm_retile(d.w, wtd, d.N, d.out_mode == kOutGeglu, sc.stream);
  d.w_ws = wtd;
}
void tile_for_bvgemm(Scratch& sc, ConvDesc& d, const char* refusal) {
  SD_REQUIRE(bvgemm_shape_ok(d), kInvalidArgument, "%s", refusal);
  half_t* wtd = sc.out<half_t>(bvgemm_tiled_halves(d.N, concat_channels(d)), "w_bv (bvgemm.hip copy)");
  launch_bvgemm_retile(d.w, wtd, d.N, concat_channels(d), d.out_mode == kOutGeglu, sc.stream);
  d.w_bv = wtd;
}

// compressed weights as an entry point receives them on the host: a palette lut[indices] or W8A8 values q * w_scale[n]
struct HostWeights {
  WeightSource kind = WeightSource::Fp16;
  const void* lut = nullptr;          // palettes: 2^bits f16
  const uint8_t* indices = nullptr;   // (Cout, Cin + C1, k, k)
  int bits = 0;
  const int8_t* q = nullptr;          // W8A8: (Cout, Cin + C1, k, k)
  const float* w_scale = nullptr;     // (Cout,)
  float act_absmax = 0.f;             // the activations are quantized with act_absmax / 127
};

// What sd_op_conv2d_ex sets on top of sd_op_conv2d (header); default-constructed: sd_op_conv2d itself.
struct ConvOpExtra {
  const char* entry = "conv2d";   // the entry point that runs conv2d_op (what the scratch's guard report names)
  const void* x1 = nullptr;   // second source (B, C1, H, W) f16
  int C1 = 0;
  const float* temb = nullptr;   // (B, Cout) f32
  int pad_mode = 0;              // 1: the VAE encoder's F.pad(x, (0, 1, 0, 1)) + pad-0 stride-2 conv
  int twin_groups = 0;           // > 0: one GroupNorm twin over exactly this output
  const float *twin_gamma = nullptr, *twin_beta = nullptr;
  float twin_eps = 1e-5f;
  int twin_silu = 0;
  void* out_twin = nullptr;
  int* plan_out = nullptr;       // {tile, staging, splitk, slab} of the plan that ran; -1: the direct kernels
  HostWeights cw;                // sd_op_conv2d_palettized / sd_op_conv2d_w8a8: the weights arrive compressed (w is NULL)
  int nw = 0;                    // ... with this many waves per workgroup: 4, else 8 (sd_op_conv2d_w8a8_halo / _palettized_halo: tile 7's ring code)
};

// The compressed weights of a descriptor as the UNet builder uploads them (Net::upload_compressed) - the packed stream of the kind
// with its LUT / scales - and the kind's pin by the caller's n (conv_plan_pin: waves per workgroup or tile height)
void upload_compressed(Scratch& sc, ConvDesc& d, const char* what, const HostWeights& h, int n) {
  auto up = [&sc](const auto* host, size_t count) { return sc.dev(count, host); };
  d.cw = h.q ? upload_w8a8(up, h.kind, what, h.q, h.w_scale, h.act_absmax, d.N, concat_channels(d), d.ksize)
                                           : upload_palettized(up, h.kind, what, f16(h.lut), h.bits, h.indices, d.N, concat_channels(d), d.ksize);
  const WeightPin pin = conv_plan_pin(h.kind, n);
  d.tile = pin.tile;
  d.staging = pin.staging;
}

// (B, N) f32 rows on the device as the UNet keeps its time_emb_proj outputs: a column block of a wider row buffer, every other float
// of which is poisoned - a kernel that reads a neighbouring column or another row's padding leaves garbage, not a near miss
constexpr int kOpTembOffset = 4, kOpTembTail = 8;
const float* upload_temb_rows(Scratch& sc, const float* temb, int B, int N, int* stride) {
  const int ld = kOpTembOffset + (N + 3) / 4 * 4 + kOpTembTail;
  std::vector<float> rows((size_t)B * ld, 1.0e30f);
  for (int b = 0; b < B; ++b) std::copy(temb + (size_t)b * N, temb + (size_t)(b + 1) * N, rows.begin() + (size_t)b * ld + kOpTembOffset);
  *stride = ld;
  return sc.dev<float>(rows.size(), rows.data()) + kOpTembOffset;
}

// the body of sd_op_conv2d / sd_op_conv2d_ex
void conv2d_op(const void* x, const void* w, const float* bias, const void* res, void* out, int B, int Cin, int H, int W, int Cout,
               int ksize, int stride, int upsample, int tile, int splitk, int force_generic, int iters, float* ms, const ConvOpExtra& e) {
  SD_REQUIRE(x && (w || e.cw.indices || e.cw.q) && out, kInvalidArgument, "NULL argument");
  SD_REQUIRE((ksize == 1 || ksize == 3) && (stride == 1 || stride == 2) && (upsample == 0 || upsample == 1),
             kInvalidArgument, "conv2d: ksize %d stride %d upsample %d not on the path", ksize, stride, upsample);
  SD_REQUIRE(e.C1 >= 0 && (e.C1 == 0 || e.x1), kInvalidArgument, "conv2d: C1 = %d needs the second source x1", e.C1);
  SD_REQUIRE(e.pad_mode == 0 || (e.pad_mode == 1 && ksize == 3 && stride == 2 && !upsample), kInvalidArgument,
             "conv2d: pad_mode %d (1 = the (0,1,0,1) padding of a 3x3 / stride-2 conv without upsample; ksize %d stride %d upsample %d)",
             e.pad_mode, ksize, stride, upsample);
  SD_REQUIRE(e.twin_groups == 0 || (e.twin_groups > 0 && e.twin_gamma && e.twin_beta && e.out_twin), kInvalidArgument,
             "conv2d: a GroupNorm twin needs twin_gamma, twin_beta and out_twin (twin_groups %d)", e.twin_groups);
  Scratch sc(e.entry);
  const int up = upsample ? 2 : 1, pad = ksize / 2;
  // pad_mode 1: one row / column of zeros behind the image only (the sizes of Net::conv_w)
  const int Ho = e.pad_mode ? (H * up + 1 - ksize) / stride + 1 : (H * up + 2 * pad - ksize) / stride + 1;
  const int Wo = e.pad_mode ? (W * up + 1 - ksize) / stride + 1 : (W * up + 2 * pad - ksize) / stride + 1;
  SD_REQUIRE(Ho >= 1 && Wo >= 1, kInvalidArgument, "conv2d: empty output (%dx%d)", Ho, Wo);
  ConvDesc d;
  d.x0 = upload_nhwc(sc, x, B, Cin, H, W);
  d.C0 = Cin;
  if (e.C1 > 0) {
    d.x1 = upload_nhwc(sc, e.x1, B, e.C1, H, W);
    d.C1 = e.C1;
  }
  if (e.cw.kind == WeightSource::Fp16) d.w = upload_conv_weight(sc, w, Cout, Cin + e.C1, ksize);
  d.bias = bias ? sc.dev<float>(Cout, bias) : nullptr;
  if (e.temb) d.temb = upload_temb_rows(sc, e.temb, B, Cout, &d.temb_stride);
  if (res) d.res = upload_nhwc(sc, res, B, Cout, Ho, Wo);
  half_t* dout = sc.out<half_t>((size_t)B * Ho * Wo * Cout, "out");
  d.out = dout;
  d.B = B; d.Hi = H; d.Wi = W; d.Ho = Ho; d.Wo = Wo;
  d.ksize = ksize; d.stride = stride; d.up = up; d.N = Cout;
  if (e.pad_mode) d.pad = 0;
  apply_tile_code(d, tile, true);
  d.splitk = splitk;
  d.debug = force_generic >= 2 ? force_generic - 1 : 0;   // 2: loads only, 3: compute only (ablation)
  if (d.debug & 4) d.prof = sc.out<long long>(8, "phase clock");
  const bool fast = force_generic != 1 && conv_fast_path_ok(d);
  if (e.cw.kind == WeightSource::PalWstream)
    SD_REQUIRE(fast && wstream_shape_ok(d), kInvalidArgument, "conv2d_palettized: shape not eligible for plan tile 14 (wstream.hip: k=%d C0=%d C1=%d N=%d %dx%d)",
               ksize, Cin, e.C1, Cout, Ho, Wo);
  // (W8A8: shape and values were checked on the host by the entry point)
  if (e.cw.kind != WeightSource::Fp16)
    upload_compressed(sc, d, e.cw.kind == WeightSource::PalWstream ? "palettized conv" : e.cw.kind == WeightSource::PalHalo ? "conv2d_palettized_halo" : e.cw.kind == WeightSource::I8Halo ? "conv2d_w8a8_halo" : "conv2d_w8a8", e.cw, e.nw);
  half_t* dtwin = nullptr;
  if (e.twin_groups) {   // the GroupNorm as a twin of the conv's slab combine (sd_op_conv2d_groupnorm's producer_stats = 2)
    SD_REQUIRE(fast, kInvalidArgument, "conv2d: GroupNorm twins need the MFMA path");
    dtwin = sc.out<half_t>((size_t)B * Ho * Wo * Cout, "out_twin");
    d.n_twins = 1;
    d.twin[0].y = dtwin;
    d.twin[0].ld = Cout;
    d.twin[0].c_off = 0;
    d.twin[0].cpg = Cout / e.twin_groups;
    d.twin[0].gamma = sc.dev<float>(Cout, e.twin_gamma);
    d.twin[0].beta = sc.dev<float>(Cout, e.twin_beta);
    d.twin[0].eps = e.twin_eps;
    d.twin[0].silu = e.twin_silu;
    SD_REQUIRE(Cout % e.twin_groups == 0 && reduce_twin_ok(Ho * Wo, Cout, 1, d.twin), kInvalidArgument,
               "conv2d: shape not eligible for a GroupNorm twin (HW=%d C=%d groups=%d)", Ho * Wo, Cout, e.twin_groups);
  }
  ConvWorkspace ws;
  // the pre-tiled weight copies: what a forced plan reads, else exactly what the planner names for the library's own plan
  const ConvWeightCopies copies = (fast && tile == 0 && splitk == 0 && !d.debug && d.cw.kind == WeightSource::Fp16) ? conv_plan_copies(d) : ConvWeightCopies{false, false, false};
  if (fast && (d.tile == 9 || copies.wstream)) tile_for_wstream(sc, d, "conv2d: shape not eligible for plan tile 9 (wstream.hip)");
  if (fast && (d.tile == 11 || copies.bvgemm)) tile_for_bvgemm(sc, d, "conv2d: shape not eligible for plan tile 11 (bvgemm.hip)");
  if (fast && d.tile != 11 && d.tile != 12) ws = workspace_for(sc, {d});
  // N <= 8 (conv_out of the UNet / the VAE): the small-N kernels the handles use, unless the direct kernel was asked for
  const bool small_n = !fast && force_generic == 0 && Cout <= 8 && Cin % 8 == 0 && ksize == 3 && stride == 1 && !res && !d.x1 && !d.temb && !e.pad_mode;
  if (e.plan_out) {   // the plan launch_conv is about to resolve for this descriptor
    const ConvPlan p = fast ? conv_plan(d) : ConvPlan{-1, -1, -1, false, 0};
    e.plan_out[0] = p.tile; e.plan_out[1] = p.staging; e.plan_out[2] = p.splitk; e.plan_out[3] = fast ? (p.slab ? 1 : 0) : -1;
  }
  sc.timed(iters, ms, [&] {
    if (fast)
      launch_conv(d, ws, sc.stream);
    else if (small_n)
      launch_conv_small_n(d, nullptr, sc.stream);
    else
      launch_conv_generic(d, 0, sc.stream);
  });
  if (d.prof) {
    long long t[8];
    SD_HIP(hipMemcpy(t, d.prof, sizeof(t), hipMemcpyDeviceToHost));
    fprintf(stderr, "[sd prof] block0: prologue %lld, k-loop %lld, epilogue %lld shader cycles; total %lld cycles = %lld ticks of the 100 MHz wall clock\n",
            t[1] - t[0], t[2] - t[1], t[3] - t[2], t[3] - t[0], t[4]);
  }
  download_nchw(dout, out, B, Cout, Ho, Wo);
  if (dtwin) download_nchw(dtwin, e.out_twin, B, Cout, Ho, Wo);
}

// The producer of the conv2d_groupnorm* entries: a k x k stride-1 conv (+ bias, + residual) that writes its output to a fresh
// buffer (d.out) under the tile code's plan, without split-K
ConvDesc producer_conv(Scratch& sc, const void* x, const void* w, const float* bias, const void* res, int B, int Cin, int H, int W,
                       int Cout, int ksize, int tile) {
  ConvDesc d = conv_desc(upload_nhwc(sc, x, B, Cin, H, W), Cin, upload_conv_weight(sc, w, Cout, Cin, ksize),
                         bias ? sc.dev<float>(Cout, bias) : nullptr, res ? upload_nhwc(sc, res, B, Cout, H, W) : nullptr,
                         sc.out<half_t>((size_t)B * H * W * Cout, "conv_out"), B, H, W, Cout, ksize);
  apply_tile_code(d, tile);
  d.splitk = 1;
  return d;
}

// the consumer of a folded GroupNorm reads the producer's raw output and its statistics entries
void fold_groupnorm(ConvDesc& d, const half_t* x, const float* partial, const float* gamma, const float* beta, float eps, int groups,
                    int entries) {
  d.x0 = x;
  d.gnf_partial = partial;
  d.gnf_gamma = gamma;
  d.gnf_beta = beta;
  d.gnf_eps = eps;
  d.gnf_groups = groups;
  d.gnf_entries = entries;
}

// LayerNorm-folded q|k|v GEMM: columns [0, 2C) to qk (queries scaled by q_scale), the V columns token-transposed to vt [B][C][HW]
ConvDesc qkv_desc(const half_t* in, const FoldedProj& f, float ln_eps, half_t* qk, half_t* vt, int B, int H, int W, int C, float q_scale,
                  int vt_perm) {
  ConvDesc d = conv_desc(in, C, f.w, f.bias, nullptr, qk, B, H, W, 3 * C);
  d.ln_colsum = f.colsum;
  d.ln_eps = ln_eps;
  d.out_t = vt;
  d.n_trans = 2 * C;
  d.ldT = H * W;
  d.vt_perm = vt_perm ? 1 : 0;
  d.q_scale = q_scale;
  d.q_cols = C;
  return d;
}

// (B, C, HW) -> [B][HW][C] and back, on the host
template <typename T>
std::vector<T> host_nhwc(const T* src, int B, int C, int HW) {
  std::vector<T> t((size_t)B * C * HW);
  for (int b = 0; b < B; ++b)
    for (int c = 0; c < C; ++c)
      for (int p = 0; p < HW; ++p) t[((size_t)b * HW + p) * C + c] = src[((size_t)b * C + c) * HW + p];
  return t;
}
template <typename T>
void host_nchw(const std::vector<T>& t, T* dst, int B, int C, int HW) {
  for (int b = 0; b < B; ++b)
    for (int c = 0; c < C; ++c)
      for (int p = 0; p < HW; ++p) dst[((size_t)b * C + c) * HW + p] = t[((size_t)b * HW + p) * C + c];
}
template <typename T>
std::vector<T> download(const T* dev, size_t n) {
  std::vector<T> t(n);
  SD_HIP(hipMemcpy(t.data(), dev, n * sizeof(T), hipMemcpyDeviceToHost));
  return t;
}

}  // namespace
}  // namespace sd

using namespace sd;

extern "C" {

// What sd_op_attention and sd_op_attention_kernel share: the entry's host refusals, in its order, and every field of the descriptor that
// is not an address.
static AttnDesc attention_op_desc(int impl, int B, int heads, int d, int Sq, int Sk, int variant) {
  SD_REQUIRE(impl >= 0 && impl <= 2, kInvalidArgument, "unknown attention implementation %d", impl);
  SD_REQUIRE(B > 0 && heads > 0 && d > 0 && Sq > 0 && Sk > 0, kInvalidArgument, "empty attention problem");
  SD_REQUIRE(variant != 3 || Sq == Sk, kInvalidArgument, "attention variant 3 (q | k in one buffer) needs Sq == Sk (%d, %d)", Sq, Sk);
  const int C = heads * d;
  // the software-pipelined d = 64 kernel reads V^T in its own key order (AttnDesc::vt_perm)
  const bool perm = variant != 1 && attention8_shape_ok(d, Sq, Sk);
  AttnDesc a;
  a.ldq = a.ldk = variant == 3 ? 2 * C : C;   // 3: q and k are rows of ONE [B][S][2C] buffer (qkv_desc's qk)
  a.B = B; a.heads = heads; a.d = d; a.Sq = Sq; a.Sk = Sk;
  a.ldv = (Sk + 7) / 8 * 8; a.ldo = C;
  a.impl = impl;
  a.variant = variant == 3 ? 0 : variant;   // (3: the default dispatch, only the addresses differ)
  a.vt_perm = perm ? 1 : 0;
  if (variant == 2) {   // the caller multiplied d^-0.5 * log2(e) into q before rounding it to fp16 (what the UNet's q|k|v GEMM does)
    SD_REQUIRE(perm, kInvalidArgument, "attention variant 2 (pre-scaled q) needs attention8's shape (d %d Sq %d Sk %d)", d, Sq, Sk);
    a.q_prescaled = 1;
  }
  if (variant >= 100) {   // attention8's balanced form, variant - 100 units per workgroup (0: the launch's own split)
    SD_REQUIRE(perm, kInvalidArgument, "attention variant %d (balanced form) needs attention8's shape (d %d Sq %d Sk %d)", variant, d, Sq, Sk);
    a.variant = 0;
    a.sk_force = 1;
    a.sk_upw = variant - 100;
  }
  return a;
}
// the scratch of the balanced form where attention8 wants it for this problem (sizes into the descriptor; false: the classic grid)
static bool attention_op_wants_scratch(AttnDesc& a, int variant) {
  size_t pb = 0;
  int nc = 0;
  if (a.vt_perm && attention8_sk_scratch(a, &pb, &nc)) {
    a.sk_part_bytes = pb;
    a.sk_cnt_n = nc;
    return true;
  }
  SD_REQUIRE(variant < 100, kInvalidArgument, "attention variant %d: the balanced form cannot run this shape", variant);
  return false;
}
static void check_attention_w8a8_shape(int B, int heads, int S) {
  SD_REQUIRE(B > 0 && heads > 0 && S > 0, kInvalidArgument, "attention_w8a8: empty problem");
  SD_REQUIRE(S >= 64 && S % 64 == 0, kInvalidArgument, "attention_w8a8: S = %d is off the shape rule (head dim 64, S a positive multiple of 64)", S);
  SD_REQUIRE(attention_i8_shape_ok(64, S, S), kInvalidArgument, "attention_w8a8: S = %d, the exact integer sums hold up to %d", S, kAttnI8MaxS);
}

int sd_op_attention(int impl, const void* q, const void* k, const void* v, void* out, int B, int heads, int d,
                    int Sq, int Sk, int variant, int iters, float* ms) {
  return guarded([&] {
    SD_REQUIRE(q && k && v && out, kInvalidArgument, "NULL argument");
    AttnDesc a = attention_op_desc(impl, B, heads, d, Sq, Sk, variant);
    Scratch sc("attention");
    const int C = heads * d;
    if (variant == 3) {   // q and k as a self-attention of a handle reads them: rows of ONE [B][S][2C] buffer (qkv_desc's qk)
      const half_t *qs = f16(q), *ks = f16(k);
      std::vector<half_t> qk((size_t)B * Sq * 2 * C);
      for (int b = 0; b < B; ++b)
        for (int c = 0; c < C; ++c)
          for (int s = 0; s < Sq; ++s) {
            qk[((size_t)b * Sq + s) * 2 * C + c] = qs[((size_t)b * C + c) * Sq + s];
            qk[((size_t)b * Sq + s) * 2 * C + C + c] = ks[((size_t)b * C + c) * Sq + s];
          }
      const half_t* dqk = sc.dev<half_t>(qk.size(), qk.data(), "q | k");
      a.q = dqk;
      a.k = dqk + C;
    } else {
      a.q = upload_tokens(sc, q, B, C, Sq);
      a.k = upload_tokens(sc, k, B, C, Sk);
    }
    a.vt = upload_vt(sc, v, B, C, Sk, a.ldv, a.vt_perm != 0);
    half_t* o = sc.out<half_t>((size_t)B * Sq * C, "out");
    a.out = o;
    if (attention_op_wants_scratch(a, variant)) {
      a.sk_part = reinterpret_cast<float*>(sc.out<char>(a.sk_part_bytes, "sk_part"));
      a.sk_cnt = sc.zeroed<unsigned>(a.sk_cnt_n, "sk_cnt");   // zeroed: AttnDesc::sk_cnt is "ZEROED once by the owner", the kernel leaves it at zero
    }
    sc.timed(iters, ms, [&] { launch_attention(a, sc.stream); });
    download_tokens(o, out, B, C, Sq);
  });
}

// Which kernel would sd_op_attention (int8 == 0) or sd_op_attention_w8a8 (int8 != 0: impl, d, Sk and variant are not read) launch for
// this problem?  The descriptor those entries build, handed to the choice function their launcher calls.  Host only: nothing launched.
int sd_op_attention_kernel(int int8, int impl, int B, int heads, int d, int Sq, int Sk, int variant, char* text, int text_bytes) {
  return guarded([&] {
    SD_REQUIRE(text && text_bytes >= 1, kInvalidArgument, "bad attention_kernel arguments");
    AttnKernel c;
    if (int8) {
      check_attention_w8a8_shape(B, heads, Sq);
      AttnI8Desc di;
      di.B = B; di.heads = heads; di.S = Sq;
      c = attention_i8_kernel(di);
    } else {
      AttnDesc a = attention_op_desc(impl, B, heads, d, Sq, Sk, variant);
      static float part_stand_in;      // never dereferenced: attention8_kernel asks only whether scratch is offered, and how much
      static unsigned cnt_stand_in;
      if (attention_op_wants_scratch(a, variant)) {
        a.sk_part = &part_stand_in;
        a.sk_cnt = &cnt_stand_in;
      }
      c = attention_kernel(a);
    }
    const std::string name = attention_kernel_name(c);
    SD_REQUIRE((int)name.size() < text_bytes, kInvalidArgument, "attention_kernel: the text buffer holds %d bytes, the line needs %zu", text_bytes, name.size() + 1);
    memcpy(text, name.c_str(), name.size() + 1);
  });
}

// The einsum quantizer on a handle's layouts (attention_i8.hip einsum_quantize_kernel): qk (B * S, 2C) f16 = q | k rows, vt (B, C, ldv) f16
// in the key order vt_perm_in (0 natural, 1 attention8's) -> qk_q (B * S, 2C) int8, vt_q (B, C, S) int8 in the int8 kernel's key order.
// q_range_eff is the range of the STORED queries (r_q times the producer's pre-scale, or r_q itself).
int sd_op_einsum_quantize(const void* qk, const void* vt, int B, int S, int C, int ldv, int vt_perm_in, float q_range_eff, float k_absmax,
                          float v_absmax, int8_t* qk_q, int8_t* vt_q, int iters, float* ms) {
  return guarded([&] {
    SD_REQUIRE(qk && vt && qk_q && vt_q, kInvalidArgument, "NULL argument");
    SD_REQUIRE(B > 0 && S > 0 && C > 0 && S % 32 == 0 && C % 8 == 0 && ldv >= S && ldv % 4 == 0 && (vt_perm_in == 0 || vt_perm_in == 1), kInvalidArgument,
               "einsum_quantize: B %d S %d C %d ldv %d vt_perm_in %d (S a multiple of 32, C of 8, ldv of 4 and at least S, vt_perm_in 0 or 1)", B, S, C,
               ldv, vt_perm_in);
    SD_REQUIRE(w8a8_absmax_ok(q_range_eff) && w8a8_absmax_ok(k_absmax) && w8a8_absmax_ok(v_absmax), kInvalidArgument,
               "einsum_quantize: ranges %g, %g, %g: each must be a positive finite number", (double)q_range_eff, (double)k_absmax, (double)v_absmax);
    const float inv_q = 127.0f / q_range_eff, inv_k = 127.0f / k_absmax, inv_v = 127.0f / v_absmax;
    SD_REQUIRE(std::isfinite(inv_q) && std::isfinite(inv_k) && std::isfinite(inv_v), kInvalidArgument, "einsum_quantize: a range has no finite inverse scale");
    Scratch sc("einsum_quantize");
    const size_t n_qk = (size_t)B * S * 2 * C, n_vt = (size_t)B * C * ldv, n_vq = (size_t)B * C * S;
    const half_t* dqk = sc.dev<half_t>(n_qk, f16(qk), "qk");
    const half_t* dvt = sc.dev<half_t>(n_vt, f16(vt), "vt");
    int8_t* dq = sc.out<int8_t>(n_qk, "qk_q", kOpGuard, 0x80);   // -128: a value the quantizer never writes (0xff is -1)
    int8_t* dv = sc.out<int8_t>(n_vq, "vt_q", kOpGuard, 0x80);
    sc.timed(iters, ms, [&] { launch_einsum_quantize(dqk, dvt, B, S, C, ldv, vt_perm_in, inv_q, inv_k, inv_v, dq, dv, sc.stream); });
    SD_HIP(hipMemcpy(qk_q, dq, n_qk, hipMemcpyDeviceToHost));
    SD_HIP(hipMemcpy(vt_q, dv, n_vq, hipMemcpyDeviceToHost));
  });
}

// v (B * S, C) int8 token-major, natural key order -> vt_q (B, C, S): V^T with every 32 keys in attention_i8_vt_key's order (host only)
static void pack_vt_i8(const int8_t* v, int B, int C, int S, int8_t* vt_q) {
  for (int b = 0; b < B; ++b)
    for (int c = 0; c < C; ++c)
      for (int p = 0; p < S; ++p)
        vt_q[((size_t)b * C + c) * S + p] = v[((size_t)b * S + (p & ~31) + attention_i8_vt_key(p & 31)) * C + c];
}

int sd_op_w8a8_pack_vt(const int8_t* v, int B, int C, int S, int8_t* vt_q, size_t* bytes) {
  return guarded([&] {
    SD_REQUIRE(v && bytes, kInvalidArgument, "NULL argument");
    SD_REQUIRE(B > 0 && C > 0 && S > 0 && S % 32 == 0, kInvalidArgument, "w8a8_pack_vt: B %d C %d S %d (S a multiple of 32)", B, C, S);
    *bytes = (size_t)B * C * S;
    if (vt_q) pack_vt_i8(v, B, C, S, vt_q);
  });
}

// The self-attention einsums in W8A8 (attention_i8.hip): q_q, k_q, v_q (B * S, heads * 64) int8 token-major in natural key order ->
// out (B * S, heads * 64) f16.  Every check runs on the host in front of the first device call (Scratch), in the order the header lists.
int sd_op_attention_w8a8(const int8_t* q_q, const int8_t* k_q, const int8_t* v_q, float q_absmax, float k_absmax, float v_absmax, void* out, int B,
                         int heads, int S, int iters, float* ms) {
  return guarded([&] {
    SD_REQUIRE(q_q && k_q && v_q && out, kInvalidArgument, "NULL argument");
    check_attention_w8a8_shape(B, heads, S);
    SD_REQUIRE(w8a8_absmax_ok(q_absmax) && w8a8_absmax_ok(k_absmax) && w8a8_absmax_ok(v_absmax), kInvalidArgument,
               "attention_w8a8: ranges %g, %g, %g: each must be a positive finite number", (double)q_absmax, (double)k_absmax, (double)v_absmax);
    const int C = heads * 64;
    const size_t n = (size_t)B * S * C;
    const int8_t* const ins[3] = {q_q, k_q, v_q};
    for (int t = 0; t < 3; ++t)
      for (size_t i = 0; i < n; ++i)
        SD_REQUIRE(ins[t][i] != -128, kInvalidArgument, "attention_w8a8: %s value -128 at element %zu, the symmetric range is [-127, 127]",
                   t == 0 ? "q" : t == 1 ? "k" : "v", i);
    // the device images a handle's quantizer leaves: q | k rows of one (B * S, 2C) matrix, V^T in the kernel's key order
    std::vector<int8_t> qk(2 * n), vt(n);
    for (size_t r = 0; r < (size_t)B * S; ++r) {
      std::copy(q_q + r * C, q_q + (r + 1) * C, qk.begin() + r * 2 * C);
      std::copy(k_q + r * C, k_q + (r + 1) * C, qk.begin() + r * 2 * C + C);
    }
    pack_vt_i8(v_q, B, C, S, vt.data());
    Scratch sc("attention_w8a8");
    const int8_t* dqk = sc.dev<int8_t>(qk.size(), qk.data(), "q | k");
    AttnI8Desc d;
    d.q = dqk;
    d.k = dqk + C;
    d.vt = sc.dev<int8_t>(vt.size(), vt.data(), "vt");
    half_t* o = sc.out<half_t>(n, "out");
    d.out = o;
    d.B = B; d.heads = heads; d.S = S;
    d.ldq = d.ldk = 2 * C; d.ldv = S; d.ldo = C;
    d.q_absmax = q_absmax; d.k_absmax = k_absmax; d.v_absmax = v_absmax;
    sc.timed(iters, ms, [&] { launch_attention_i8(d, sc.stream); });
    SD_HIP(hipMemcpy(out, o, n * 2, hipMemcpyDeviceToHost));
  });
}

int sd_op_layernorm(const void* x, const float* weight, const float* bias, void* out, int B, int C, int S, float eps,
                    int iters, float* ms) {
  return guarded([&] {
    SD_REQUIRE(x && weight && bias && out, kInvalidArgument, "NULL argument");
    Scratch sc("layernorm");
    half_t* dx = upload_tokens(sc, x, B, C, S);
    half_t* dy = sc.out<half_t>((size_t)B * S * C, "out");
    float* dw = sc.dev<float>(C, weight);
    float* db = sc.dev<float>(C, bias);
    sc.timed(iters, ms, [&] { launch_layernorm(dx, dw, db, dy, B * S, C, eps, sc.stream); });
    download_tokens(dy, out, B, C, S);
  });
}

int sd_op_groupnorm(const void* x, const float* weight, const float* bias, void* out, int B, int C, int H, int W,
                    int groups, float eps, int silu, int iters, float* ms) {
  return guarded([&] {
    SD_REQUIRE(x && weight && bias && out, kInvalidArgument, "NULL argument");
    Scratch sc("groupnorm");
    half_t* dx = upload_nhwc(sc, x, B, C, H, W);
    half_t* dy = sc.out<half_t>((size_t)B * H * W * C, "out");
    float* dw = sc.dev<float>(C, weight);
    float* db = sc.dev<float>(C, bias);
    float* partial = poisoned_gn_partial(sc, B, H * W, groups);
    sc.timed(iters, ms, [&] {
      launch_groupnorm(dx, C, nullptr, 0, partial, dw, db, dy, B, H * W, groups, eps, silu, sc.stream);
    });
    download_nchw(dy, out, B, C, H, W);
  });
}

int sd_op_groupnorm_shortcut(const void* x0, const void* x1, const float* gn_weight, const float* gn_bias, const void* w, const float* bias,
                             void* out_gn, void* out_sc, int B, int C0, int C1, int H, int W, int N, int groups, float eps, int silu,
                             int side, int iters, float* ms) {
  return guarded([&] {
    SD_REQUIRE(x0 && gn_weight && gn_bias && w && out_gn && out_sc, kInvalidArgument, "NULL argument");
    if (!x1) C1 = 0;
    const int C = C0 + C1;
    Scratch sc("groupnorm_shortcut");
    half_t* d0 = upload_nhwc(sc, x0, B, C0, H, W);
    half_t* d1 = x1 ? upload_nhwc(sc, x1, B, C1, H, W) : nullptr;
    half_t* dy = sc.out<half_t>((size_t)B * H * W * C, "out_gn");
    half_t* ds = sc.out<half_t>((size_t)B * H * W * N, "out_sc");
    float* dgw = sc.dev<float>(C, gn_weight);
    float* dgb = sc.dev<float>(C, gn_bias);
    float* partial = poisoned_gn_partial(sc, B, H * W, groups);
    // conv_shortcut: a 1x1 conv over the channel concat (x0 | x1), weights [N][C] as they are
    ConvDesc d = conv_desc(d0, C0, sc.dev<half_t>((size_t)N * C, f16(w)), bias ? sc.dev<float>(N, bias) : nullptr, nullptr, ds, B, H, W, N);
    d.x1 = d1;
    d.C1 = C1;
    SD_REQUIRE(conv_fast_path_ok(d), kInvalidArgument, "groupnorm_shortcut: C0=%d C1=%d N=%d not MFMA-tileable", C0, C1, N);
    SD_REQUIRE(!side || gn_side_gemm_ok(d), kUnsupported, "groupnorm_shortcut: the GEMM cannot ride in the GroupNorm launch (M=%d)", B * H * W);
    ConvWorkspace ws = workspace_for(sc, {d});
    sc.timed(iters, ms, [&] {
      if (side) {
        launch_groupnorm(d0, C0, d1, C1, partial, dgw, dgb, dy, B, H * W, groups, eps, silu, sc.stream, 0, &d);
      } else {
        launch_groupnorm(d0, C0, d1, C1, partial, dgw, dgb, dy, B, H * W, groups, eps, silu, sc.stream);
        launch_conv(d, ws, sc.stream);
      }
    });
    download_nchw(dy, out_gn, B, C, H, W);
    download_nchw(ds, out_sc, B, N, H, W);
  });
}

// tile = 0 and splitk = 0 mirror a handle: the entry holds the pre-tiled weight copies conv_plan_copies names, so the launch runs the
// plan a UNet's conv of this shape runs (plan tiles 9 / 11 included; sd_op_conv_plan says which).  A forced tile holds its own copy only.
int sd_op_conv2d(const void* x, const void* w, const float* bias, const void* res, void* out, int B, int Cin, int H,
                 int W, int Cout, int ksize, int stride, int upsample, int tile, int splitk, int force_generic,
                 int iters, float* ms) {
  return guarded([&] { conv2d_op(x, w, bias, res, out, B, Cin, H, W, Cout, ksize, stride, upsample, tile, splitk, force_generic, iters, ms, ConvOpExtra{}); });
}

int sd_op_conv2d_ex(const void* x, const void* x1, const void* w, const float* bias, const float* temb, const void* res, void* out, int B,
                    int Cin, int C1, int H, int W, int Cout, int ksize, int stride, int upsample, int pad_mode, int twin_groups,
                    const float* twin_gamma, const float* twin_beta, float twin_eps, int twin_silu, void* out_twin, int tile, int splitk,
                    int force_generic, int* plan_out, int iters, float* ms) {
  return guarded([&] {
    SD_REQUIRE(plan_out, kInvalidArgument, "NULL argument");
    ConvOpExtra e;
    e.entry = "conv2d_ex";
    e.x1 = x1; e.C1 = C1; e.temb = temb; e.pad_mode = pad_mode;
    e.twin_groups = twin_groups; e.twin_gamma = twin_gamma; e.twin_beta = twin_beta; e.twin_eps = twin_eps; e.twin_silu = twin_silu;
    e.out_twin = out_twin;
    e.plan_out = plan_out;
    conv2d_op(x, w, bias, res, out, B, Cin, H, W, Cout, ksize, stride, upsample, tile, splitk, force_generic, iters, ms, e);
  });
}

int sd_op_conv2d_palettized(const void* x, const void* x1, const void* lut, int nbits, const uint8_t* indices, const float* bias,
                            const void* res, void* out, int B, int Cin, int C1, int H, int W, int Cout, int ksize, int upsample, int nw,
                            int* plan_out, int iters, float* ms) {
  return guarded([&] {
    SD_REQUIRE(lut && indices, kInvalidArgument, "NULL argument");
    SD_REQUIRE(palette_bits_ok(nbits), kInvalidArgument, "conv2d_palettized: nbits = %d, not one of 1, 2, 4, 6, 8", nbits);
    SD_REQUIRE(nw == 0 || nw == 4 || nw == 8, kInvalidArgument, "conv2d_palettized: nw = %d, not 0, 4 or 8", nw);
    SD_REQUIRE(B > 0 && Cin > 0 && C1 >= 0 && Cout > 0 && H > 0 && W > 0, kInvalidArgument, "conv2d_palettized: empty problem");
    ConvOpExtra e;
    e.entry = "conv2d_palettized";
    e.x1 = x1; e.C1 = C1;
    e.plan_out = plan_out;
    e.cw.kind = WeightSource::PalWstream; e.cw.lut = lut; e.cw.indices = indices; e.cw.bits = nbits;
    e.nw = nw;
    conv2d_op(x, nullptr, bias, res, out, B, Cin, H, W, Cout, ksize, 1, upsample, 0, 0, 0, iters, ms, e);
  });
}

// Every check runs on the host in front of the first device call (Scratch), in the order the header lists them.
int sd_op_conv2d_palettized_halo(const void* x, const void* x1, const void* lut, int nbits, const uint8_t* indices, const float* bias, const float* temb,
                                 const void* res, void* out, int B, int Cin, int C1, int H, int W, int Cout, int upsample, int staging, int splitk,
                                 int* plan_out, int iters, float* ms) {
  return guarded([&] {
    SD_REQUIRE(x && lut && indices && out, kInvalidArgument, "NULL argument");
    SD_REQUIRE(palette_bits_ok(nbits), kInvalidArgument, "conv2d_palettized_halo: nbits = %d, not one of 1, 2, 4, 6, 8", nbits);
    SD_REQUIRE(B > 0 && Cin > 0 && C1 >= 0 && Cout > 0 && H > 0 && W > 0 && (C1 == 0 || x1), kInvalidArgument, "conv2d_palettized_halo: empty problem");
    SD_REQUIRE((upsample == 0 || upsample == 1) && staging >= 0 && staging <= 5 && staging != 1 && splitk >= 0, kInvalidArgument,
               "conv2d_palettized_halo: upsample %d staging %d (plan tile 7's ring codes 0, 2-5) splitk %d", upsample, staging, splitk);
    ConvDesc d;   // the shape alone: what the planner's predicates look at
    d.C0 = Cin;
    if (C1 > 0) d.x1 = f16(x1), d.C1 = C1;
    d.B = B; d.Hi = H; d.Wi = W; d.Ho = H * (upsample ? 2 : 1); d.Wo = W * (upsample ? 2 : 1);
    d.ksize = 3; d.up = upsample ? 2 : 1; d.N = Cout;
    SD_REQUIRE(conv_fast_path_ok(d) && halo_pal_ok(d), kInvalidArgument,
               "conv2d_palettized_halo: shape not eligible for plan tile 25 (conv3x3_halo_pal.hip: C0=%d C1=%d N=%d %dx%d)", Cin, C1, Cout, d.Ho, d.Wo);
    palette_check_indices("conv2d_palettized_halo", indices, (size_t)Cout * (Cin + C1) * 9, nbits);
    ConvOpExtra e;
    e.entry = "conv2d_palettized_halo";
    e.x1 = x1; e.C1 = C1;
    e.temb = temb;
    e.plan_out = plan_out;
    e.cw.kind = WeightSource::PalHalo; e.cw.lut = lut; e.cw.indices = indices; e.cw.bits = nbits;
    e.nw = staging;
    conv2d_op(x, nullptr, bias, res, out, B, Cin, H, W, Cout, 3, 1, upsample, 0, splitk, 0, iters, ms, e);
  });
}

// The index stream of plan tile 25 (weight_prep.h halo_pal_pack).  Host only.
int sd_op_palette_pack_halo(const uint8_t* indices, int Cout, int Ctot, int nbits, uint8_t* stream, size_t* bytes) {
  return guarded([&] {
    SD_REQUIRE(indices && bytes, kInvalidArgument, "NULL argument");
    SD_REQUIRE(palette_bits_ok(nbits) && Cout > 0 && Ctot > 0 && Ctot % 64 == 0, kInvalidArgument, "palette_pack_halo: nbits %d Cout %d Ctot %d", nbits, Cout, Ctot);
    *bytes = halo_pal_bytes(Cout, Ctot, nbits);
    if (stream) halo_pal_pack(indices, Cout, Ctot, nbits, stream);
  });
}

// Every check runs on the host in front of the first device call (Scratch), in the order the header lists them.
int sd_op_conv2d_w8a8(const void* x, const void* x1, const int8_t* wq, const float* w_scale, float act_absmax, const float* bias,
                      const void* res, void* out, int B, int Cin, int C1, int H, int W, int Cout, int ksize, int upsample, int nw,
                      int* plan_out, int iters, float* ms) {
  return guarded([&] {
    SD_REQUIRE(x && wq && w_scale && out, kInvalidArgument, "NULL argument");
    SD_REQUIRE(nw == 0 || nw == 4 || nw == 8, kInvalidArgument, "conv2d_w8a8: nw = %d, not 0, 4 or 8", nw);
    SD_REQUIRE(B > 0 && Cin > 0 && C1 >= 0 && Cout > 0 && H > 0 && W > 0 && (C1 == 0 || x1), kInvalidArgument, "conv2d_w8a8: empty problem");
    SD_REQUIRE((ksize == 1 || ksize == 3) && (upsample == 0 || upsample == 1), kInvalidArgument, "conv2d_w8a8: ksize %d upsample %d", ksize, upsample);
    ConvDesc d;   // the shape alone: what the planner's predicates look at
    d.C0 = Cin;
    if (C1 > 0) d.x1 = f16(x1), d.C1 = C1;
    d.B = B; d.Hi = H; d.Wi = W; d.Ho = H * (upsample ? 2 : 1); d.Wo = W * (upsample ? 2 : 1);
    d.ksize = ksize; d.up = upsample ? 2 : 1; d.N = Cout;
    SD_REQUIRE(conv_fast_path_ok(d) && wstream_shape_ok(d), kInvalidArgument,
               "conv2d_w8a8: shape not eligible for plan tile 17 (wstream.hip: k=%d C0=%d C1=%d N=%d %dx%d)", ksize, Cin, C1, Cout, d.Ho, d.Wo);
    // act_absmax, then w_scale, then the weight values (-128 is outside the symmetric range)
    (void)w8a8_host_copy("conv2d_w8a8", wq, w_scale, act_absmax, Cout, Cin + C1, ksize);
    ConvOpExtra e;
    e.entry = "conv2d_w8a8";
    e.x1 = x1; e.C1 = C1;
    e.plan_out = plan_out;
    e.cw.kind = WeightSource::I8Wstream; e.cw.q = wq; e.cw.w_scale = w_scale; e.cw.act_absmax = act_absmax;
    e.nw = nw;
    conv2d_op(x, nullptr, bias, res, out, B, Cin, H, W, Cout, ksize, 1, upsample, 0, 0, 0, iters, ms, e);
  });
}

// Every check runs on the host in front of the first device call (Scratch), in the order the header lists them.
int sd_op_conv2d_w8a8_halo(const void* x, const void* x1, const int8_t* wq, const float* w_scale, float act_absmax, const float* bias, const float* temb,
                           const void* res, void* out, int B, int Cin, int C1, int H, int W, int Cout, int upsample, int staging, int splitk, int* plan_out,
                           int iters, float* ms) {
  return guarded([&] {
    SD_REQUIRE(x && wq && w_scale && out, kInvalidArgument, "NULL argument");
    SD_REQUIRE(B > 0 && Cin > 0 && C1 >= 0 && Cout > 0 && H > 0 && W > 0 && (C1 == 0 || x1), kInvalidArgument, "conv2d_w8a8_halo: empty problem");
    SD_REQUIRE((upsample == 0 || upsample == 1) && staging >= 0 && staging <= 5 && staging != 1 && splitk >= 0, kInvalidArgument,
               "conv2d_w8a8_halo: upsample %d staging %d (plan tile 7's ring codes 0, 2-5) splitk %d", upsample, staging, splitk);
    ConvDesc d;   // the shape alone: what the planner's predicates look at
    d.C0 = Cin;
    if (C1 > 0) d.x1 = f16(x1), d.C1 = C1;
    d.B = B; d.Hi = H; d.Wi = W; d.Ho = H * (upsample ? 2 : 1); d.Wo = W * (upsample ? 2 : 1);
    d.ksize = 3; d.up = upsample ? 2 : 1; d.N = Cout;
    SD_REQUIRE(conv_fast_path_ok(d) && halo_ks_ok(d), kInvalidArgument,
               "conv2d_w8a8_halo: shape not eligible for plan tile 18 (conv3x3_halo_i8.hip: C0=%d C1=%d N=%d %dx%d)", Cin, C1, Cout, d.Ho, d.Wo);
    SD_REQUIRE(Cin + C1 <= kHaloI8MaxCtot, kInvalidArgument, "conv2d_w8a8_halo: %d input channels, the exact int32 sums of plan tile 18 hold up to %d",
               Cin + C1, kHaloI8MaxCtot);
    // act_absmax, then w_scale, then the weight values (-128 is outside the symmetric range)
    (void)w8a8_host_copy("conv2d_w8a8_halo", wq, w_scale, act_absmax, Cout, Cin + C1, 3, WeightSource::I8Halo);
    ConvOpExtra e;
    e.entry = "conv2d_w8a8_halo";
    e.x1 = x1; e.C1 = C1;
    e.temb = temb;
    e.plan_out = plan_out;
    e.cw.kind = WeightSource::I8Halo; e.cw.q = wq; e.cw.w_scale = w_scale; e.cw.act_absmax = act_absmax;
    e.nw = staging;
    conv2d_op(x, nullptr, bias, res, out, B, Cin, H, W, Cout, 3, 1, upsample, 0, splitk, 0, iters, ms, e);
  });
}

int sd_op_w8a8_pack_halo(const int8_t* wq, int Cout, int Ctot, int8_t* packed, size_t* bytes) {
  return guarded([&] {
    SD_REQUIRE(wq && bytes, kInvalidArgument, "NULL argument");
    SD_REQUIRE(Cout > 0 && Ctot > 0 && Ctot % 64 == 0, kInvalidArgument, "w8a8_pack_halo: Cout %d Ctot %d", Cout, Ctot);
    *bytes = (size_t)Cout * Ctot * 9;
    if (packed) halo_i8_pack(wq, Cout, Ctot, 3, packed);
  });
}

// The fold of an upsampler's 3x3 weights into the four 2x2 phase matrices of plan tile 21 (weight_prep.h subpixel_fold).  Host only.
int sd_op_subpixel_fold(const void* w, int w_f32, int Cout, int Cin, void* folded, size_t* halves) {
  return guarded([&] {
    SD_REQUIRE(w && halves, kInvalidArgument, "NULL argument");
    SD_REQUIRE(Cout > 0 && Cin > 0, kInvalidArgument, "subpixel_fold: Cout %d Cin %d", Cout, Cin);
    *halves = subpixel_fold_halves(Cout, Cin);
    if (!folded) return;
    if (w_f32) subpixel_fold(reinterpret_cast<const float*>(w), Cout, Cin, reinterpret_cast<half_t*>(folded));
    else subpixel_fold(f16(w), Cout, Cin, reinterpret_cast<half_t*>(folded));
  });
}

// Why plan tile 21 refuses a conv of this shape ("" when it takes it): halo_sp_refusal (conv_plan.h).  Host only.
int sd_op_subpixel_refusal(int ksize, int stride, int up, int C0, int C1, int N, int B, int Hi, int Wi, int out_mode, char* text, int text_bytes) {
  return guarded([&] {
    SD_REQUIRE(text && text_bytes >= 1, kInvalidArgument, "bad subpixel_refusal arguments");
    static const half_t present = 0;   // the predicate only tests the pointer
    ConvDesc d;
    d.C0 = C0;
    if (C1 > 0) d.x1 = &present, d.C1 = C1;
    d.B = B; d.Hi = Hi; d.Wi = Wi;
    d.Ho = stride > 0 ? Hi * up / stride : 0; d.Wo = stride > 0 ? Wi * up / stride : 0;
    d.ksize = ksize; d.stride = stride; d.up = up; d.N = N; d.out_mode = out_mode;
    const char* why = halo_sp_refusal(d);
    const std::string line = why ? why : "";
    SD_REQUIRE((int)line.size() < text_bytes, kInvalidArgument, "subpixel_refusal: the text buffer holds %d bytes, the line needs %zu", text_bytes, line.size() + 1);
    memcpy(text, line.c_str(), line.size() + 1);
  });
}

// Nearest-x2 upsample + 3x3 / pad-1 conv as plan tile 21: w (Cout, Cin, 3, 3) f16 is folded by subpixel_fold, as a handle folds it.
// staging: tile 7's ring code (2: three stages, else
// four), splitk 0: the plan's rule.  plan_out = {tile, staging, splitk, slab}.
int sd_op_conv2d_subpixel(const void* x, const void* w, const float* bias, const void* res, void* out, int B, int Cin, int H, int W, int Cout, int splitk,
                          int staging, int* plan_out, int iters, float* ms) {
  return guarded([&] {
    SD_REQUIRE(x && w && out && plan_out, kInvalidArgument, "NULL argument");
    SD_REQUIRE(B > 0 && Cin > 0 && Cout > 0 && H > 0 && W > 0 && splitk >= 0 && staging >= 0 && staging <= 5 && staging != 1, kInvalidArgument,
               "conv2d_subpixel: empty problem, splitk %d or staging %d (plan tile 7's ring codes 0, 2-5)", splitk, staging);
    ConvDesc d;
    d.C0 = Cin;
    d.B = B; d.Hi = H; d.Wi = W; d.Ho = 2 * H; d.Wo = 2 * W;
    d.ksize = 3; d.up = 2; d.N = Cout;
    d.subpix = true;
    d.staging = staging;
    d.splitk = splitk;
    SD_REQUIRE(conv_fast_path_ok(d) && halo_sp_ok(d), kInvalidArgument, "conv2d_subpixel: plan tile 21 (conv3x3_halo_sp.hip) does not take this shape: %s (Cin=%d Cout=%d %dx%d)",
               halo_sp_refusal(d) ? halo_sp_refusal(d) : "off the MFMA path", Cin, Cout, H, W);
    std::vector<half_t> folded(subpixel_fold_halves(Cout, Cin));
    subpixel_fold(f16(w), Cout, Cin, folded.data());
    Scratch sc("conv2d_subpixel");
    d.x0 = upload_nhwc(sc, x, B, Cin, H, W);
    d.w = sc.dev<half_t>(folded.size(), folded.data());
    d.bias = bias ? sc.dev<float>(Cout, bias) : nullptr;
    if (res) d.res = upload_nhwc(sc, res, B, Cout, d.Ho, d.Wo);
    const size_t n_out = (size_t)B * d.Ho * d.Wo * Cout;
    half_t* dout = sc.out<half_t>(n_out, "out");
    d.out = dout;
    const ConvPlan p = conv_plan(d);
    plan_out[0] = p.tile; plan_out[1] = p.staging; plan_out[2] = p.splitk; plan_out[3] = p.slab ? 1 : 0;
    ConvWorkspace ws = workspace_for(sc, {d});
    sc.timed(iters, ms, [&] { launch_conv(d, ws, sc.stream); });
    download_nchw(dout, out, B, Cout, d.Ho, d.Wo);
  });
}

// Every check runs on the host in front of the first device call (Scratch), in the order the header lists them.
int sd_op_gemm_w8a8(const void* x, const int8_t* wq, const float* w_scale, float act_absmax, const float* bias, const void* res, void* out, int B,
                    int Cin, int H, int W, int Cout, int bm, int* plan_out, int iters, float* ms) {
  return guarded([&] {
    SD_REQUIRE(bm == 0 || bm == 32 || bm == 64, kInvalidArgument, "gemm_w8a8: bm = %d, not 0, 32 or 64", bm);
    SD_REQUIRE(x && wq && w_scale && out && plan_out, kInvalidArgument, "NULL argument");
    SD_REQUIRE(B > 0 && Cin > 0 && Cout > 0 && H > 0 && W > 0, kInvalidArgument, "gemm_w8a8: empty problem");
    ConvDesc d;
    d.C0 = Cin;
    d.B = B; d.Hi = H; d.Wi = W; d.Ho = H; d.Wo = W;
    d.N = Cout;
    const int code = conv_plan_pin(WeightSource::I8Gemm, bm).staging;
    SD_REQUIRE(conv_fast_path_ok(d) && smgemm_shape_ok(d, code), kInvalidArgument,
               "gemm_w8a8: shape not eligible for plan tile 19 (smgemm_i8.hip: Cin=%d Cout=%d M=%d bm=%d - Cin a multiple of 64, Cout of 80, M of the "
               "tile height, at least 2 x 2 tiles and a multiple of 8 of them)", Cin, Cout, B * H * W, bm);
    SD_REQUIRE(smgemm_i8_shape_ok(d, code), kInvalidArgument, "gemm_w8a8: K = %d, the exact int32 sums of plan tile 19 hold up to %d", Cin, kSmI8MaxK);
    // act_absmax, then w_scale, then the weight values (-128 is outside the symmetric range)
    (void)w8a8_host_copy("gemm_w8a8", wq, w_scale, act_absmax, Cout, Cin, 1, WeightSource::I8Gemm);
    Scratch sc("gemm_w8a8");
    d.x0 = upload_nhwc(sc, x, B, Cin, H, W);
    d.bias = bias ? sc.dev<float>(Cout, bias) : nullptr;
    if (res) d.res = upload_nhwc(sc, res, B, Cout, H, W);
    half_t* dout = sc.out<half_t>((size_t)B * H * W * Cout, "out");
    d.out = dout;
    HostWeights h;
    h.kind = WeightSource::I8Gemm; h.q = wq; h.w_scale = w_scale; h.act_absmax = act_absmax;
    upload_compressed(sc, d, "gemm_w8a8", h, bm);
    const ConvPlan p = conv_plan(d);
    plan_out[0] = p.tile; plan_out[1] = p.staging; plan_out[2] = p.splitk; plan_out[3] = p.slab ? 1 : 0;
    ConvWorkspace ws;
    sc.timed(iters, ms, [&] { launch_conv(d, ws, sc.stream); });
    download_nchw(dout, out, B, Cout, H, W);
  });
}

int sd_op_w8a8_pack_gemm(const int8_t* wq, int Cout, int K, int8_t* packed, size_t* bytes) {
  return guarded([&] {
    SD_REQUIRE(wq && bytes, kInvalidArgument, "NULL argument");
    SD_REQUIRE(Cout > 0 && K > 0 && Cout % 16 == 0 && K % 64 == 0, kInvalidArgument, "w8a8_pack_gemm: Cout %d K %d", Cout, K);
    *bytes = smgemm_i8_bytes(Cout, K);
    if (packed) smgemm_i8_pack(wq, Cout, K, packed);
  });
}

// LayerNorm that leaves as int8 (the producer of plan tile 20's activations): x (M, C) f16 token-major, ln_weight / ln_bias (C) f32 or
// both NULL (a plain quantize of x) -> xq (M, C) int8 with inv_s = 1 / (act_absmax / 127) as w8a8_host_copy computes it.
int sd_op_layernorm_q8(const void* x, const float* ln_weight, const float* ln_bias, float act_absmax, float eps, int8_t* xq, int M, int C,
                       int iters, float* ms) {
  return guarded([&] {
    SD_REQUIRE(x && xq, kInvalidArgument, "NULL argument");
    SD_REQUIRE(M > 0 && C > 0, kInvalidArgument, "layernorm_q8: empty problem");
    SD_REQUIRE((ln_weight == nullptr) == (ln_bias == nullptr), kInvalidArgument, "layernorm_q8: ln_weight and ln_bias go together");
    SD_REQUIRE(C % 8 == 0 && C <= 2048, kInvalidArgument, "layernorm_q8: C = %d, not a multiple of 8 up to 2048", C);
    SD_REQUIRE(w8a8_absmax_ok(act_absmax), kInvalidArgument, "layernorm_q8: act_absmax = %g, not a positive finite number", (double)act_absmax);
    const float inv_s = 1.0f / (act_absmax / 127.0f);
    SD_REQUIRE(std::isfinite(inv_s) && inv_s > 0.f, kInvalidArgument, "layernorm_q8: act_absmax = %g has no finite inverse scale", (double)act_absmax);
    Scratch sc("layernorm_q8");
    const half_t* dx = sc.dev<half_t>((size_t)M * C, f16(x));
    const float* dw = ln_weight ? sc.dev<float>(C, ln_weight) : nullptr;
    const float* db = ln_bias ? sc.dev<float>(C, ln_bias) : nullptr;
    int8_t* dq = sc.out<int8_t>((size_t)M * C, "xq", kOpGuard, 0x80);   // -128: a value the quantizer never writes (0xff is -1)
    sc.timed(iters, ms, [&] { launch_layernorm_q8(dx, dw, db, dq, M, C, eps, inv_s, sc.stream); });
    SD_HIP(hipMemcpy(xq, dq, (size_t)M * C, hipMemcpyDeviceToHost));
  });
}

// The GEGLU projection in W8A8 (plan tile 20): the body of sd_op_geglu_w8a8 (out) and sd_op_geglu_w8a8_q8 (out_q: the product leaves as
// int8 by out_absmax).  Every check runs on the host in front of the first device call (Scratch), in the order the header lists them.
// The bias goes up interleaved as the UNet builder uploads it (upload_vec(..., geglu)).
static int geglu_w8a8_op(const int8_t* xq, const int8_t* wq, const float* w_scale, float act_absmax, const float* bias, void* out, float out_absmax,
                         int8_t* out_q, bool q8, int M, int C, int N2, int bm, int* plan_out, int iters, float* ms) {
  return guarded([&] {
    SD_REQUIRE(bm == 0 || bm == 128 || bm == 256, kInvalidArgument, "geglu_w8a8: bm = %d, not 0, 128 or 256", bm);
    SD_REQUIRE(xq && wq && w_scale && (q8 ? out_q != nullptr : out != nullptr) && plan_out, kInvalidArgument, "NULL argument");
    SD_REQUIRE(M > 0 && C > 0 && N2 > 0, kInvalidArgument, "geglu_w8a8: empty problem");
    ConvDesc d = token_gemm(nullptr, C, nullptr, nullptr, nullptr, nullptr, 1, M, N2);
    d.out_mode = kOutGeglu;
    const int code = conv_plan_pin(WeightSource::I8Geglu, bm).staging;
    SD_REQUIRE(conv_fast_path_ok(d) && smgeglu_shape_ok(d, code), kInvalidArgument,
               "geglu_w8a8: shape not eligible for plan tile 20 (smgeglu_i8.hip: M=%d C=%d N2=%d bm=%d - C a multiple of 64, N2 of 160, M of the "
               "tile height, at least 2 x 2 tiles and a multiple of 8 of them)", M, C, N2, bm);
    SD_REQUIRE(smgeglu_i8_shape_ok(d, code), kInvalidArgument, "geglu_w8a8: K = %d, the exact int32 sums of plan tile 20 hold up to %d", C, kSmI8MaxK);
    // act_absmax (and out_absmax), then w_scale, then the weight values (-128 is outside the symmetric range), then the activations
    SD_REQUIRE(w8a8_absmax_ok(act_absmax), kInvalidArgument, "geglu_w8a8: act_absmax = %g, not a positive finite number", (double)act_absmax);
    float out_inv_s = 0.f;
    if (q8) {
      SD_REQUIRE(w8a8_absmax_ok(out_absmax), kInvalidArgument, "geglu_w8a8: out_absmax = %g, not a positive finite number", (double)out_absmax);
      out_inv_s = 1.0f / (out_absmax / 127.0f);   // (as w8a8_host_copy computes the factor the consumer's activations were quantized by)
      SD_REQUIRE(std::isfinite(out_inv_s) && out_inv_s > 0.f, kInvalidArgument, "geglu_w8a8: out_absmax = %g has no finite inverse scale", (double)out_absmax);
    }
    (void)w8a8_host_copy("geglu_w8a8", wq, w_scale, act_absmax, N2, C, 1, WeightSource::I8Geglu);
    for (size_t i = 0; i < (size_t)M * C; ++i)
      SD_REQUIRE(xq[i] != -128, kInvalidArgument, "geglu_w8a8: activation value -128 at element %zu, the symmetric range is [-127, 127]", i);
    Scratch sc(q8 ? "geglu_w8a8_q8" : "geglu_w8a8");
    d.x0_i8 = sc.dev<int8_t>((size_t)M * C, xq);
    if (bias) {
      std::vector<float> bi(N2);
      for (int o = 0; o < N2; ++o) bi[geglu_row(o, N2)] = bias[o];
      d.bias = sc.dev<float>(N2, bi.data());
    }
    const size_t n_out = (size_t)M * (N2 / 2);
    half_t* dout = nullptr;
    int8_t* dq = nullptr;
    if (q8) {   // -128: an element the launch skipped reads back as a value the quantizer never writes (0xff is -1)
      dq = sc.out<int8_t>(n_out, "out_q", kOpGuard, 0x80);
      d.out_q8 = dq;
      d.out_inv_s = out_inv_s;
    } else {
      dout = sc.out<half_t>(n_out, "out");
      d.out = dout;
    }
    HostWeights h;
    h.kind = WeightSource::I8Geglu; h.q = wq; h.w_scale = w_scale; h.act_absmax = act_absmax;
    upload_compressed(sc, d, "geglu_w8a8", h, bm);
    const ConvPlan p = conv_plan(d);
    plan_out[0] = p.tile; plan_out[1] = p.staging; plan_out[2] = p.splitk; plan_out[3] = p.slab ? 1 : 0;
    ConvWorkspace ws;
    sc.timed(iters, ms, [&] { launch_conv(d, ws, sc.stream); });
    if (q8) {
      SD_HIP(hipMemcpy(out_q, dq, n_out, hipMemcpyDeviceToHost));
    } else {
      SD_HIP(hipMemcpy(out, dout, n_out * 2, hipMemcpyDeviceToHost));
    }
  });
}

int sd_op_geglu_w8a8(const int8_t* xq, const int8_t* wq, const float* w_scale, float act_absmax, const float* bias, void* out, int M, int C,
                     int N2, int bm, int* plan_out, int iters, float* ms) {
  return geglu_w8a8_op(xq, wq, w_scale, act_absmax, bias, out, 0.f, nullptr, false, M, C, N2, bm, plan_out, iters, ms);
}

int sd_op_geglu_w8a8_q8(const int8_t* xq, const int8_t* wq, const float* w_scale, float act_absmax, const float* bias, float out_absmax,
                        int8_t* out_q, int M, int C, int N2, int bm, int* plan_out, int iters, float* ms) {
  return geglu_w8a8_op(xq, wq, w_scale, act_absmax, bias, nullptr, out_absmax, out_q, true, M, C, N2, bm, plan_out, iters, ms);
}

// The small-M 1x1 GEMM from int8 weights and int8 activations (plan tile 24), token-major.  Every check runs on the host in front of the
// first device call (Scratch), in the order the header lists them.
int sd_op_gemm_q8(const int8_t* xq, const int8_t* wq, const float* w_scale, float act_absmax, const float* bias, const void* res, void* out,
                  int M, int K, int N, int bm, int* plan_out, int iters, float* ms) {
  return guarded([&] {
    SD_REQUIRE(bm == 0 || bm == 32 || bm == 64, kInvalidArgument, "gemm_q8: bm = %d, not 0, 32 or 64", bm);
    SD_REQUIRE(xq && wq && w_scale && out && plan_out, kInvalidArgument, "NULL argument");
    SD_REQUIRE(M > 0 && K > 0 && N > 0, kInvalidArgument, "gemm_q8: empty problem");
    ConvDesc d = token_gemm(nullptr, K, nullptr, nullptr, nullptr, nullptr, 1, M, N);
    const int code = conv_plan_pin(WeightSource::I8GemmQ, bm).staging;
    SD_REQUIRE(conv_fast_path_ok(d) && smgemm_shape_ok(d, code), kInvalidArgument,
               "gemm_q8: shape not eligible for plan tile 24 (smgemm_q8.hip: M=%d K=%d N=%d bm=%d - K a multiple of 64, N of 80, M of the tile height, "
               "at least 2 x 2 tiles and a multiple of 8 of them)", M, K, N, bm);
    SD_REQUIRE(smgemm_q8_shape_ok(d, code), kInvalidArgument, "gemm_q8: K = %d, the exact int32 sums of plan tile 24 hold up to %d", K, kSmI8MaxK);
    // act_absmax, then w_scale, then the weight values (-128 is outside the symmetric range), then the activations
    (void)w8a8_host_copy("gemm_q8", wq, w_scale, act_absmax, N, K, 1, WeightSource::I8GemmQ);
    for (size_t i = 0; i < (size_t)M * K; ++i)
      SD_REQUIRE(xq[i] != -128, kInvalidArgument, "gemm_q8: activation value -128 at element %zu, the symmetric range is [-127, 127]", i);
    Scratch sc("gemm_q8");
    d.x0_i8 = sc.dev<int8_t>((size_t)M * K, xq);
    d.bias = bias ? sc.dev<float>(N, bias) : nullptr;
    if (res) d.res = sc.dev<half_t>((size_t)M * N, f16(res));
    const size_t n_out = (size_t)M * N;
    half_t* dout = sc.out<half_t>(n_out, "out");
    d.out = dout;
    HostWeights h;
    h.kind = WeightSource::I8GemmQ; h.q = wq; h.w_scale = w_scale; h.act_absmax = act_absmax;
    upload_compressed(sc, d, "gemm_q8", h, bm);
    const ConvPlan p = conv_plan(d);
    plan_out[0] = p.tile; plan_out[1] = p.staging; plan_out[2] = p.splitk; plan_out[3] = p.slab ? 1 : 0;
    ConvWorkspace ws;
    sc.timed(iters, ms, [&] { launch_conv(d, ws, sc.stream); });
    SD_HIP(hipMemcpy(out, dout, n_out * 2, hipMemcpyDeviceToHost));
  });
}

int sd_op_w8a8_pack_geglu(const int8_t* wq, int N2, int K, int8_t* packed, size_t* bytes) {
  return guarded([&] {
    SD_REQUIRE(wq && bytes, kInvalidArgument, "NULL argument");
    SD_REQUIRE(N2 > 0 && K > 0 && N2 % 32 == 0 && K % 64 == 0, kInvalidArgument, "w8a8_pack_geglu: N2 %d K %d", N2, K);
    *bytes = smgeglu_i8_bytes(N2, K);
    if (packed) smgeglu_i8_pack(wq, N2, K, packed);
  });
}

// The fused q|k|v projection of a self-attention in W8A8 (plan tile 22).  Every check runs on the host in front of the first device call
// (Scratch), in the order the header lists them.
int sd_op_qkv_w8a8(const int8_t* xq, const int8_t* wq, const float* w_scale, float act_absmax, const float* bias, void* out_qk, void* out_vt,
                   int B, int HW, int C, float q_scale, int vt_perm, int bm, int* plan_out, int iters, float* ms) {
  return guarded([&] {
    SD_REQUIRE(bm == 0 || bm == 128 || bm == 256, kInvalidArgument, "qkv_w8a8: bm = %d, not 0, 128 or 256", bm);
    SD_REQUIRE(xq && wq && w_scale && out_qk && out_vt && plan_out, kInvalidArgument, "NULL argument");
    SD_REQUIRE(B > 0 && HW > 0 && C > 0, kInvalidArgument, "qkv_w8a8: empty problem");
    const int M = B * HW, N = 3 * C;
    ConvDesc d = conv_desc(nullptr, C, nullptr, nullptr, nullptr, nullptr, B, 1, HW, N);
    d.n_trans = 2 * C;
    d.ldT = HW;                          // (the rule wants HW % 16 == 0: no padding columns, out_vt is (B, C, HW) as sd_op_qkv_ln's)
    d.vt_perm = vt_perm ? 1 : 0;
    d.q_scale = q_scale;
    d.q_cols = q_scale != 1.f ? C : 0;  // (a factor of 1: the product is skipped)
    const int code = conv_plan_pin(WeightSource::I8Qkv, bm).staging;
    SD_REQUIRE(conv_fast_path_ok(d) && smqkv_i8_tiles(d, code), kInvalidArgument,
               "qkv_w8a8: shape not eligible for plan tile 22 (smqkv_i8.hip: B=%d HW=%d C=%d bm=%d - C a multiple of 160 and of 64, at least 640, HW a "
               "multiple of 16, B * HW of the tile height, at least 2 tile rows and a multiple of 8 tiles of 160 columns)", B, HW, C, bm);
    SD_REQUIRE(smqkv_i8_shape_ok(d, code), kInvalidArgument, "qkv_w8a8: K = %d, the exact int32 sums of plan tile 22 hold up to %d", C, kSmI8MaxK);
    // act_absmax and q_scale, then w_scale, then the weight values (-128 is outside the symmetric range), then the activations
    SD_REQUIRE(w8a8_absmax_ok(act_absmax), kInvalidArgument, "qkv_w8a8: act_absmax = %g, not a positive finite number", (double)act_absmax);
    SD_REQUIRE(std::isfinite(q_scale), kInvalidArgument, "qkv_w8a8: q_scale = %g, not finite", (double)q_scale);
    (void)w8a8_host_copy("qkv_w8a8", wq, w_scale, act_absmax, N, C, 1, WeightSource::I8Qkv);
    for (size_t i = 0; i < (size_t)M * C; ++i)
      SD_REQUIRE(xq[i] != -128, kInvalidArgument, "qkv_w8a8: activation value -128 at element %zu, the symmetric range is [-127, 127]", i);
    Scratch sc("qkv_w8a8");
    d.x0_i8 = sc.dev<int8_t>((size_t)M * C, xq);
    if (bias) d.bias = sc.dev<float>(N, bias);
    const size_t n_qk = (size_t)M * 2 * C, n_vt = (size_t)B * C * d.ldT;
    half_t* dqk = sc.out<half_t>(n_qk, "out_qk");
    half_t* dvt = sc.out<half_t>(n_vt, "out_vt");
    d.out = dqk;
    d.out_t = dvt;
    HostWeights h;
    h.kind = WeightSource::I8Qkv; h.q = wq; h.w_scale = w_scale; h.act_absmax = act_absmax;
    upload_compressed(sc, d, "qkv_w8a8", h, bm);
    const ConvPlan p = conv_plan(d);
    plan_out[0] = p.tile; plan_out[1] = p.staging; plan_out[2] = p.splitk; plan_out[3] = p.slab ? 1 : 0;
    ConvWorkspace ws;
    sc.timed(iters, ms, [&] { launch_conv(d, ws, sc.stream); });
    SD_HIP(hipMemcpy(out_qk, dqk, n_qk * 2, hipMemcpyDeviceToHost));
    SD_HIP(hipMemcpy(out_vt, dvt, n_vt * 2, hipMemcpyDeviceToHost));
  });
}

int sd_op_w8a8_pack_qkv(const int8_t* wq, int C, int8_t* packed, size_t* bytes) {
  return guarded([&] {
    SD_REQUIRE(wq && bytes, kInvalidArgument, "NULL argument");
    SD_REQUIRE(C > 0 && C % 64 == 0, kInvalidArgument, "w8a8_pack_qkv: C %d, not a positive multiple of 64", C);
    *bytes = smqkv_i8_bytes(3 * C, C);
    if (packed) smqkv_i8_pack(wq, 3 * C, C, packed);
  });
}

int sd_op_w8a8_pack(const int8_t* wq, int Cout, int Ctot, int ksize, int8_t* stream, size_t* bytes) {
  return guarded([&] {
    SD_REQUIRE(wq && bytes, kInvalidArgument, "NULL argument");
    SD_REQUIRE((ksize == 1 || ksize == 3) && Cout > 0 && Ctot > 0 && Cout % 32 == 0 && Ctot % 32 == 0, kInvalidArgument,
               "w8a8_pack: ksize %d Cout %d Ctot %d", ksize, Cout, Ctot);
    *bytes = wstream_i8_bytes(Cout, Ctot, ksize);
    if (stream) wstream_i8_pack(wq, Cout, Ctot, ksize, stream);
  });
}

int sd_op_quantize_weight(const float* w, int Cout, size_t per_row, int8_t* q, float* w_scale, double* sq_err) {
  return guarded([&] {
    SD_REQUIRE(w && q && w_scale && Cout > 0 && per_row > 0, kInvalidArgument, "quantize_weight: NULL argument or empty tensor");
    const double e = w8a8_quantize_weight(w, Cout, per_row, q, w_scale);
    if (sq_err) *sq_err = e;
  });
}

int sd_op_absmax(const void* x, size_t n, float* absmax) {
  return guarded([&] {
    SD_REQUIRE(x && n > 0 && absmax, kInvalidArgument, "absmax: NULL argument or empty tensor");
    Scratch sc("absmax");
    const half_t* dx = sc.dev<half_t>(n, f16(x));
    float* slot = sc.zeroed<float>(1, "absmax slot");   // zeroed: the kernel folds into the slot with an atomic max; calibration clears it first
    launch_absmax_half(dx, n, nullptr, 0, slot, sc.stream);
    SD_HIP(hipStreamSynchronize(sc.stream));
    SD_HIP(hipMemcpy(absmax, slot, sizeof(float), hipMemcpyDeviceToHost));
  });
}

int sd_op_palette_pack(const uint8_t* indices, int Cout, int Ctot, int ksize, int nbits, uint8_t* stream, size_t* bytes) {
  return guarded([&] {
    SD_REQUIRE(indices && bytes, kInvalidArgument, "NULL argument");
    SD_REQUIRE(palette_bits_ok(nbits) && (ksize == 1 || ksize == 3) && Cout > 0 && Ctot > 0 && Cout % 32 == 0 && Ctot % 32 == 0, kInvalidArgument,
               "palette_pack: nbits %d ksize %d Cout %d Ctot %d", nbits, ksize, Cout, Ctot);
    *bytes = wstream_pal_bytes(Cout, Ctot, ksize, nbits);
    if (stream) wstream_pal_pack(indices, Cout, Ctot, ksize, nbits, stream);
  });
}

// Every check runs on the host in front of the first device call (Scratch), in the order the header lists them.
int sd_op_gemm_palettized(const void* x, const void* lut, int nbits, const uint8_t* indices, const float* bias, const void* res, void* out,
                          int B, int Cin, int H, int W, int Cout, int bm, int* plan_out, int iters, float* ms) {
  return guarded([&] {
    SD_REQUIRE(palette_bits_ok(nbits), kInvalidArgument, "gemm_palettized: nbits = %d, not one of 1, 2, 4, 6, 8", nbits);
    SD_REQUIRE(bm == 0 || bm == 32 || bm == 64, kInvalidArgument, "gemm_palettized: bm = %d, not 0, 32 or 64", bm);
    SD_REQUIRE(x && lut && indices && out && plan_out, kInvalidArgument, "NULL argument");
    SD_REQUIRE(B > 0 && Cin > 0 && Cout > 0 && H > 0 && W > 0, kInvalidArgument, "gemm_palettized: empty problem");
    palette_check_indices("gemm_palettized", indices, (size_t)Cout * Cin, nbits);   // (in front of the shape: the header's order)
    ConvDesc d;
    d.C0 = Cin;
    d.B = B; d.Hi = H; d.Wi = W; d.Ho = H; d.Wo = W;
    d.N = Cout;
    SD_REQUIRE(conv_fast_path_ok(d) && smgemm_shape_ok(d, conv_plan_pin(WeightSource::PalGemm, bm).staging), kInvalidArgument,
               "gemm_palettized: shape not eligible for plan tile 15 (smgemm.hip: Cin=%d Cout=%d M=%d bm=%d - Cin a multiple of 64, Cout of 80, M of the "
               "tile height, at least 2 x 2 tiles and a multiple of 8 of them)", Cin, Cout, B * H * W, bm);
    Scratch sc("gemm_palettized");
    d.x0 = upload_nhwc(sc, x, B, Cin, H, W);
    d.bias = bias ? sc.dev<float>(Cout, bias) : nullptr;
    if (res) d.res = upload_nhwc(sc, res, B, Cout, H, W);
    half_t* dout = sc.out<half_t>((size_t)B * H * W * Cout, "out");
    d.out = dout;
    HostWeights h;
    h.kind = WeightSource::PalGemm; h.lut = lut; h.indices = indices; h.bits = nbits;
    upload_compressed(sc, d, "gemm_palettized", h, bm);
    const ConvPlan p = conv_plan(d);
    plan_out[0] = p.tile; plan_out[1] = p.staging; plan_out[2] = p.splitk; plan_out[3] = p.slab ? 1 : 0;
    ConvWorkspace ws;
    sc.timed(iters, ms, [&] { launch_conv(d, ws, sc.stream); });
    download_nchw(dout, out, B, Cout, H, W);
  });
}

int sd_op_palette_pack_gemm(const uint8_t* indices, int Cout, int K, int nbits, uint8_t* stream, size_t* bytes) {
  return guarded([&] {
    SD_REQUIRE(indices && bytes, kInvalidArgument, "NULL argument");
    SD_REQUIRE(palette_bits_ok(nbits) && Cout > 0 && K > 0 && Cout % 16 == 0 && K % 64 == 0, kInvalidArgument,
               "palette_pack_gemm: nbits %d Cout %d K %d", nbits, Cout, K);
    *bytes = smgemm_pal_bytes(Cout, K, nbits);
    if (stream) smgemm_pal_pack(indices, Cout, K, nbits, stream);
  });
}

int sd_op_conv2d_groupnorm(const void* x, const void* w, const float* bias, const void* res, const float* gn_weight,
                           const float* gn_bias, void* conv_out, void* out, int B, int Cin, int H, int W, int Cout, int ksize,
                           int groups, float eps, int silu, int tile, int producer_stats, int* entries, int iters, float* ms) {
  return guarded([&] {
    SD_REQUIRE(x && w && gn_weight && gn_bias && out, kInvalidArgument, "NULL argument");
    SD_REQUIRE(ksize == 1 || ksize == 3, kInvalidArgument, "conv2d_groupnorm: ksize %d", ksize);
    Scratch sc("conv2d_groupnorm");
    ConvDesc d = producer_conv(sc, x, w, bias, res, B, Cin, H, W, Cout, ksize, tile);
    half_t* dconv = d.out;
    half_t* dy = sc.out<half_t>((size_t)B * H * W * Cout, "out");
    const bool fast = conv_fast_path_ok(d);   // else: conv_in's 4-channel MFMA kernel / the direct kernels
    float* partial = poisoned_gn_partial(sc, B, H * W, groups);
    if (producer_stats == 1) {
      d.gn_partial = partial;
      d.gn_groups = groups;
    }
    float* dgw = sc.dev<float>(Cout, gn_weight);
    float* dgb = sc.dev<float>(Cout, gn_bias);
    if (fast && d.tile == 9) tile_for_wstream(sc, d, "conv2d_groupnorm: shape not eligible for plan tile 9");
    if (producer_stats == 2) {   // the GroupNorm as a twin of the conv's slab combine: no GroupNorm launch
      SD_REQUIRE(fast, kInvalidArgument, "conv2d_groupnorm: GroupNorm twins need the MFMA path");
      d.n_twins = 1;
      d.twin[0].y = dy;
      d.twin[0].ld = Cout;
      d.twin[0].c_off = 0;
      d.twin[0].cpg = Cout / groups;
      d.twin[0].gamma = dgw;
      d.twin[0].beta = dgb;
      d.twin[0].eps = eps;
      d.twin[0].silu = silu;
      SD_REQUIRE(Cout % groups == 0 && reduce_twin_ok(H * W, Cout, 1, d.twin), kInvalidArgument,
                 "conv2d_groupnorm: shape not eligible for a GroupNorm twin (HW=%d C=%d groups=%d)", H * W, Cout, groups);
    }
    ConvWorkspace ws;
    if (fast) ws = workspace_for(sc, {d});
    int n_entries = 0;
    sc.timed(iters, ms, [&] {
      n_entries = fast ? launch_conv(d, ws, sc.stream) : launch_conv_generic(d, 0, sc.stream);
      if (producer_stats != 2)
        launch_groupnorm(dconv, Cout, nullptr, 0, partial, dgw, dgb, dy, B, H * W, groups, eps, silu, sc.stream, n_entries);
    });
    if (entries) *entries = n_entries;
    if (conv_out) download_nchw(dconv, conv_out, B, Cout, H, W);
    download_nchw(dy, out, B, Cout, H, W);
  });
}

int sd_op_conv2d_groupnorm_proj(const void* x, const void* w, const float* bias, const void* res, const float* gn_weight,
                                const float* gn_bias, const void* proj_w, const float* proj_bias, void* conv_out, void* out, int B,
                                int Cin, int H, int W, int Cout, int ksize, int Nproj, int groups, float eps, int fold, int tile,
                                int* entries, int iters, float* ms) {
  return guarded([&] {
    SD_REQUIRE(x && w && gn_weight && gn_bias && proj_w && out, kInvalidArgument, "NULL argument");
    SD_REQUIRE(ksize == 1 || ksize == 3, kInvalidArgument, "conv2d_groupnorm_proj: ksize %d", ksize);
    Scratch sc("conv2d_groupnorm_proj");
    ConvDesc d = producer_conv(sc, x, w, bias, res, B, Cin, H, W, Cout, ksize, tile);
    half_t* dconv = d.out;
    half_t* dnorm = sc.out<half_t>((size_t)B * H * W * Cout, "normalised tensor");
    half_t* dy = sc.out<half_t>((size_t)B * H * W * Nproj, "out");
    SD_REQUIRE(conv_fast_path_ok(d), kInvalidArgument, "conv2d_groupnorm_proj: the producer must run on the MFMA path");
    float* partial = poisoned_gn_partial(sc, B, H * W, groups);
    d.gn_partial = partial;
    d.gn_groups = groups;
    float* dgw = sc.dev<float>(Cout, gn_weight);
    float* dgb = sc.dev<float>(Cout, gn_bias);
    // the 1x1 projection over the conv's output
    ConvDesc pd = conv_desc(nullptr, Cout, sc.dev<half_t>((size_t)Nproj * Cout, f16(proj_w)), proj_bias ? sc.dev<float>(Nproj, proj_bias) : nullptr,
                            nullptr, dy, B, H, W, Nproj);
    SD_REQUIRE(conv_fast_path_ok(pd), kInvalidArgument, "conv2d_groupnorm_proj: the projection must run on the MFMA path");
    ConvWorkspace ws = workspace_for(sc, {d, pd});
    int n_entries = 0;
    sc.timed(iters, ms, [&] {
      n_entries = launch_conv(d, ws, sc.stream);
      ConvDesc pp = pd;
      if (fold && n_entries >= 1 && n_entries <= 128) {
        fold_groupnorm(pp, dconv, partial, dgw, dgb, eps, groups, n_entries);
      } else {
        launch_groupnorm(dconv, Cout, nullptr, 0, partial, dgw, dgb, dnorm, B, H * W, groups, eps, 0, sc.stream, n_entries);
        pp.x0 = dnorm;
      }
      launch_conv(pp, ws, sc.stream);
    });
    if (entries) *entries = (fold && n_entries >= 1 && n_entries <= 128) ? n_entries : 0;
    if (conv_out) download_nchw(dconv, conv_out, B, Cout, H, W);
    download_nchw(dy, out, B, Nproj, H, W);
  });
}

int sd_op_conv2d_groupnorm_conv3x3(const void* x, const void* w, const float* bias, const void* res, const float* gn_weight,
                                   const float* gn_bias, const void* w2, const float* bias2, const void* res2, void* conv_out, void* out,
                                   int B, int Cin, int H, int W, int Cout, int ksize, int N2, int groups, float eps, int silu, int fold,
                                   int tile, int staging2, int* entries, int iters, float* ms) {
  return guarded([&] {
    SD_REQUIRE(x && w && gn_weight && gn_bias && w2 && out, kInvalidArgument, "NULL argument");
    SD_REQUIRE(ksize == 1 || ksize == 3, kInvalidArgument, "conv2d_groupnorm_conv3x3: ksize %d", ksize);
    Scratch sc("conv2d_groupnorm_conv3x3");
    ConvDesc d = producer_conv(sc, x, w, bias, res, B, Cin, H, W, Cout, ksize, tile);
    half_t* dconv = d.out;
    half_t* dnorm = sc.out<half_t>((size_t)B * H * W * Cout, "normalised tensor");
    half_t* dy = sc.out<half_t>((size_t)B * H * W * N2, "out");
    SD_REQUIRE(conv_fast_path_ok(d), kInvalidArgument, "conv2d_groupnorm_conv3x3: the producer must run on the MFMA path");
    float* partial = poisoned_gn_partial(sc, B, H * W, groups);
    d.gn_partial = partial;
    d.gn_groups = groups;
    float* dgw = sc.dev<float>(Cout, gn_weight);
    float* dgb = sc.dev<float>(Cout, gn_bias);
    // the 3x3 conv over the normalised tensor
    ConvDesc cd = conv_desc(nullptr, Cout, upload_conv_weight(sc, w2, N2, Cout, 3), bias2 ? sc.dev<float>(N2, bias2) : nullptr,
                            res2 ? upload_nhwc(sc, res2, B, N2, H, W) : nullptr, dy, B, H, W, N2, 3);
    cd.staging = staging2;
    cd.gnf_groups = groups;
    SD_REQUIRE(conv_fast_path_ok(cd), kInvalidArgument, "conv2d_groupnorm_conv3x3: the second conv must run on the MFMA path");
    const bool can_fold = fold && silu && conv_gn_loader_ok(cd);   // (the loader always applies SiLU: every such GroupNorm of the graph has one)
    SD_REQUIRE(!fold || can_fold, kUnsupported, "conv2d_groupnorm_conv3x3: the halo loader cannot normalise C=%d groups=%d @%dx%d", Cout, groups, H, W);
    cd.gnf_groups = 0;
    ConvWorkspace ws = workspace_for(sc, {d, cd});
    int n_entries = 0;
    sc.timed(iters, ms, [&] {
      n_entries = launch_conv(d, ws, sc.stream);
      ConvDesc cc = cd;
      if (fold && n_entries >= 1 && n_entries <= 128) {
        fold_groupnorm(cc, dconv, partial, dgw, dgb, eps, groups, n_entries);
        cc.gnf_silu = silu ? 1 : 0;
      } else {
        launch_groupnorm(dconv, Cout, nullptr, 0, partial, dgw, dgb, dnorm, B, H * W, groups, eps, silu ? 1 : 0, sc.stream, n_entries);
        cc.x0 = dnorm;
      }
      launch_conv(cc, ws, sc.stream);
    });
    if (entries) *entries = (fold && n_entries >= 1 && n_entries <= 128) ? n_entries : 0;
    if (conv_out) download_nchw(dconv, conv_out, B, Cout, H, W);
    download_nchw(dy, out, B, N2, H, W);
  });
}

int sd_op_cross_attention_fused(const void* x, const float* ln_weight, const float* ln_bias, const void* wq, const void* k,
                                const void* v, void* out, int B, int heads, int Sq, int Sk, float eps, int nst, int iters,
                                float* ms) {
  return guarded([&] {
    SD_REQUIRE(x && ln_weight && ln_bias && wq && k && v && out, kInvalidArgument, "NULL argument");
    const int C = heads * 64;
    SD_REQUIRE(B > 0 && heads > 0 && xattn_fused_ok(C, heads, Sq, Sk), kUnsupported,
               "cross_attention_fused: heads %d x 64 channels, Sq %d, Sk %d (<= 96)", heads, Sq, Sk);
    Scratch sc("cross_attention_fused");
    const int ldv = (Sk + 7) / 8 * 8;
    const FoldedProj fq = upload_ln_folded(sc, wq, nullptr, ln_weight, ln_bias, C, C, false);
    XAttnDesc d;
    d.x = upload_tokens(sc, x, B, C, Sq);
    d.wq = fq.w;
    d.bias = fq.bias;
    d.colsum = fq.colsum;
    d.k = upload_tokens(sc, k, B, C, Sk);
    d.vt = upload_vt(sc, v, B, C, Sk, ldv, false);
    half_t* o = sc.out<half_t>((size_t)B * Sq * C, "out");
    d.out = o;
    d.M = B * Sq; d.C = C; d.S = Sq; d.L = Sk; d.ldv = ldv; d.heads = heads;
    d.ln_eps = eps;
    d.nst = nst;
    sc.timed(iters, ms, [&] { launch_xattn_fused(d, sc.stream); });
    download_tokens(o, out, B, C, Sq);
  });
}

int sd_op_cross_attention_block(const void* x, const float* ln_weight, const float* ln_bias, const void* wq, const void* k, const void* v,
                                const void* wo, const float* bo, const void* a1, const void* wo1, const float* bo1, void* out, int B, int heads,
                                int Sq, int Sk, float eps, int fused, int iters, float* ms) {
  return guarded([&] {
    SD_REQUIRE(x && ln_weight && ln_bias && wq && k && v && wo && bo && out, kInvalidArgument, "NULL argument");
    const bool pre = a1 != nullptr;
    SD_REQUIRE(!pre || (wo1 && bo1), kInvalidArgument, "cross_attention_block: a1 needs wo1 and bo1");
    const int C = heads * 64;
    SD_REQUIRE(B > 0 && heads > 0 && xattn_fused_ok(C, heads, Sq, Sk), kUnsupported,
               "cross_attention_block: heads %d x 64 channels, Sq %d, Sk %d (<= 96)", heads, Sq, Sk);
    SD_REQUIRE(!fused || (xattn_out_ok(C, heads, Sq, Sk) && (!pre || heads == 5)), kUnsupported,
               "cross_attention_block: the one-launch form takes 5 or 10 heads (with a1: 5) and Sq %% 32 == 0 (heads %d, Sq %d)", heads, Sq);
    Scratch sc("cross_attention_block");
    const int ldv = (Sk + 7) / 8 * 8;
    half_t* dx = upload_tokens(sc, x, B, C, Sq);
    half_t* da1 = pre ? upload_tokens(sc, a1, B, C, Sq) : nullptr;
    const FoldedProj fq = upload_ln_folded(sc, wq, nullptr, ln_weight, ln_bias, C, C, false);
    half_t* dk = upload_tokens(sc, k, B, C, Sk);
    half_t* dvt = upload_vt(sc, v, B, C, Sk, ldv, false);
    half_t* dwo = sc.dev<half_t>((size_t)C * C, f16(wo));
    float* dbo = sc.dev<float>(C, bo);
    half_t* dwo1 = pre ? sc.dev<half_t>((size_t)C * C, f16(wo1)) : nullptr;
    float* dbo1 = pre ? sc.dev<float>(C, bo1) : nullptr;
    half_t* dh1 = sc.out<half_t>((size_t)B * Sq * C, "h1");
    half_t* da2 = sc.out<half_t>((size_t)B * Sq * C, "attention output");
    half_t* o = sc.out<half_t>((size_t)B * Sq * C, "out");
    if (fused) {
      half_t* wq_t = sc.out<half_t>((size_t)C * C, "wq_t");
      half_t* wo_t = sc.out<half_t>((size_t)C * C, "wo_t");
      launch_xattn_out_retile(fq.w, wq_t, C, sc.stream);
      launch_xattn_out_retile(dwo, wo_t, C, sc.stream);
      XAttnOutDesc d;
      d.x = pre ? da1 : dx; d.wq_t = wq_t; d.q_bias = fq.bias; d.q_colsum = fq.colsum; d.k = dk; d.vt = dvt; d.wo_t = wo_t; d.o_bias = dbo; d.out = o;
      d.M = B * Sq; d.C = C; d.S = Sq; d.L = Sk; d.ldv = ldv; d.heads = heads; d.ln_eps = eps;
      if (pre) {
        half_t* wo1_t = sc.out<half_t>((size_t)C * C, "wo1_t");
        launch_xattn_out_retile(dwo1, wo1_t, C, sc.stream);
        d.h0 = dx; d.wo1_t = wo1_t; d.o1_bias = dbo1;
      }
      sc.timed(iters, ms, [&] { launch_xattn_out(d, sc.stream); });
    } else {
      auto gemm_res = [&](const half_t* in, const half_t* w, const float* bias, const half_t* res, half_t* dst) {   // 1x1 GEMM + residual
        ConvDesc cd = token_gemm(in, C, w, bias, res, dst, B, Sq, C);
        SD_REQUIRE(conv_fast_path_ok(cd), kInvalidArgument, "cross_attention_block: to_out off the MFMA path");
        return cd;
      };
      const half_t* h1 = pre ? dh1 : dx;
      XAttnDesc d;
      d.x = h1; d.wq = fq.w; d.bias = fq.bias; d.colsum = fq.colsum; d.k = dk; d.vt = dvt; d.out = da2;
      d.M = B * Sq; d.C = C; d.S = Sq; d.L = Sk; d.ldv = ldv; d.heads = heads; d.ln_eps = eps;
      ConvDesc c1 = gemm_res(da1 ? da1 : dx, dwo1 ? dwo1 : dwo, dbo1 ? dbo1 : dbo, dx, dh1);   // (only launched with a1)
      ConvDesc c2 = gemm_res(da2, dwo, dbo, h1, o);
      ConvWorkspace ws = workspace_for(sc, {c1, c2});
      sc.timed(iters, ms, [&] {
        if (pre) launch_conv(c1, ws, sc.stream);
        launch_xattn_fused(d, sc.stream);
        launch_conv(c2, ws, sc.stream);
      });
    }
    download_tokens(o, out, B, C, Sq);
  });
}

int sd_op_ffn_out_proj(const void* g, const void* w1, const float* b1, const void* res1, const void* w2, const float* b2, const void* res2,
                       void* out, float* gn_sums, int B, int C, int S, int groups, int fused, int iters, float* ms) {
  return guarded([&] {
    SD_REQUIRE(g && w1 && b1 && res1 && w2 && b2 && res2 && out, kInvalidArgument, "NULL argument");
    const int K1 = 4 * C, M = B * S;
    SD_REQUIRE(B > 0 && C % 64 == 0 && S > 0, kInvalidArgument, "ffn_out_proj: B=%d C=%d S=%d", B, C, S);
    SD_REQUIRE(fused >= 0 && fused <= 5, kInvalidArgument, "ffn_out_proj: fused code %d", fused);
    SD_REQUIRE(fused != 1 || ffn_proj_ok(C, K1, M, S), kUnsupported, "ffn_out_proj: the one-launch form takes C = 320 and S %% 32 == 0 (C=%d S=%d)", C, S);
    SD_REQUIRE(!gn_sums || (groups >= 1 && C % groups == 0), kInvalidArgument, "ffn_out_proj: groups %d", groups);
    Scratch sc("ffn_out_proj");
    half_t* dg = upload_tokens(sc, g, B, K1, S);
    half_t* dr1 = upload_tokens(sc, res1, B, C, S);
    half_t* dr2 = upload_tokens(sc, res2, B, C, S);
    half_t* dw1 = sc.dev<half_t>((size_t)C * K1, f16(w1));
    half_t* dw2 = sc.dev<half_t>((size_t)C * C, f16(w2));
    float* db1 = sc.dev<float>(C, b1);
    float* db2 = sc.dev<float>(C, b2);
    half_t* dh3 = sc.out<half_t>((size_t)M * C, "h3");
    half_t* o = sc.out<half_t>((size_t)M * C, "out");
    const size_t pf = gn_sums ? groupnorm_scratch_floats(B, S, groups) : 0;
    float* partial = gn_sums ? poisoned_gn_partial(sc, B, S, groups) : nullptr;   // only what the producer wrote may be folded
    int n_entries = 0;
    if (fused >= 2) {   // the merged tail: weight fold (once per handle, outside the timed region), then ONE two-source GEMM
      half_t* wm = sc.out<half_t>((size_t)C * (K1 + C), "merged weights");
      float* bm = sc.out<float>(C, "merged bias");
      launch_wfold(dw2, db2, dw1, db1, wm, bm, C, C, K1, sc.stream);
      ConvDesc cd = token_gemm(dg, K1, wm, bm, dr2, o, B, S, C);
      cd.x1 = dr1;
      cd.C1 = C;
      cd.gn_partial = partial;
      cd.gn_groups = groups;
      SD_REQUIRE(conv_fast_path_ok(cd), kInvalidArgument, "ffn_out_proj: off the MFMA path");
      if (fused == 3) cd.tile = 3;
      if (fused >= 4) cd.tile = 12, cd.staging = fused - 3;
      ConvWorkspace ws = workspace_for(sc, {cd});
      sc.timed(iters, ms, [&] { n_entries = launch_conv(cd, ws, sc.stream); });
    } else if (fused) {
      half_t* w1_t = sc.out<half_t>((size_t)C * K1, "w1_t");
      half_t* w2_t = sc.out<half_t>((size_t)C * C, "w2_t");
      launch_xattn_out_retile_nk(dw1, w1_t, C, K1, sc.stream);
      launch_xattn_out_retile_nk(dw2, w2_t, C, C, sc.stream);
      FfnProjDesc d;
      d.g = dg; d.w1_t = w1_t; d.b1 = db1; d.res1 = dr1; d.w2_t = w2_t; d.b2 = db2; d.res2 = dr2; d.out = o;
      d.gn_partial = partial; d.gn_groups = groups; d.M = M; d.C = C; d.K1 = K1; d.S = S;
      sc.timed(iters, ms, [&] { n_entries = launch_ffn_proj(d, sc.stream); });
    } else {
      ConvDesc c1 = token_gemm(dg, K1, dw1, db1, dr1, dh3, B, S, C);
      ConvDesc c2 = token_gemm(dh3, C, dw2, db2, dr2, o, B, S, C);
      SD_REQUIRE(conv_fast_path_ok(c1) && conv_fast_path_ok(c2), kInvalidArgument, "ffn_out_proj: off the MFMA path");
      c2.gn_partial = partial;
      c2.gn_groups = groups;
      ConvWorkspace ws = workspace_for(sc, {c1, c2});
      sc.timed(iters, ms, [&] {
        launch_conv(c1, ws, sc.stream);
        n_entries = launch_conv(c2, ws, sc.stream);
      });
    }
    download_tokens(o, out, B, C, S);
    if (gn_sums) {   // the producer's entries folded on the host: (sum, sumsq) per (sample, group); -1 entries: none written
      std::vector<float> hp(pf);
      SD_HIP(hipMemcpy(hp.data(), partial, pf * sizeof(float), hipMemcpyDeviceToHost));
      for (int b = 0; b < B; ++b)
        for (int gi = 0; gi < groups; ++gi) {
          double s1 = 0.0, s2 = 0.0;
          for (int e = 0; e < n_entries; ++e) {
            s1 += hp[(((size_t)b * groups + gi) * kGnMaxSlabs + e) * 2];
            s2 += hp[(((size_t)b * groups + gi) * kGnMaxSlabs + e) * 2 + 1];
          }
          gn_sums[((size_t)b * groups + gi) * 2] = n_entries ? (float)s1 : NAN;
          gn_sums[((size_t)b * groups + gi) * 2 + 1] = n_entries ? (float)s2 : NAN;
        }
    }
  });
}

int sd_op_fold_linear(const void* wp, const float* bp, const void* w2, const float* b2, void* wm_out, float* bm_out, int N, int J, int K) {
  return guarded([&] {
    SD_REQUIRE(wp && bp && w2 && b2 && wm_out && bm_out && N > 0 && J > 0 && K > 0, kInvalidArgument, "fold_linear: N=%d J=%d K=%d", N, J, K);
    Scratch sc("fold_linear");
    half_t* dwp = sc.dev<half_t>((size_t)N * J, f16(wp));
    half_t* dw2 = sc.dev<half_t>((size_t)J * K, f16(w2));
    float* dbp = sc.dev<float>(N, bp);
    float* db2 = sc.dev<float>(J, b2);
    half_t* merged = sc.out<half_t>((size_t)N * (K + J), "merged weights");
    float* bm = sc.out<float>(N, "merged bias");
    launch_wfold(dwp, dbp, dw2, db2, merged, bm, N, J, K, sc.stream);
    SD_HIP(hipStreamSynchronize(sc.stream));
    SD_HIP(hipMemcpy2D(wm_out, (size_t)K * 2, merged, (size_t)(K + J) * 2, (size_t)K * 2, N, hipMemcpyDeviceToHost));
    SD_HIP(hipMemcpy(bm_out, bm, (size_t)N * sizeof(float), hipMemcpyDeviceToHost));
    // the copied block behind the folded columns must be Wp itself
    std::vector<half_t> tail((size_t)N * J);
    SD_HIP(hipMemcpy2D(tail.data(), (size_t)J * 2, merged + K, (size_t)(K + J) * 2, (size_t)J * 2, N, hipMemcpyDeviceToHost));
    SD_REQUIRE(std::memcmp(tail.data(), wp, tail.size() * 2) == 0, kInternal, "fold_linear: the Wp columns of the merged matrix differ from Wp");
  });
}

int sd_op_geglu(const void* x, const void* w, const float* bias, void* out, int M, int C, int N2, int iters, float* ms) {
  return guarded([&] {
    SD_REQUIRE(x && w && out && N2 % 2 == 0, kInvalidArgument, "bad GEGLU arguments");
    Scratch sc("geglu");
    const int half_n = N2 / 2;
    SD_REQUIRE(half_n % 32 == 0, kUnsupported, "GEGLU needs (N/2) %% 32 == 0");
    std::vector<half_t> wt((size_t)N2 * C);
    retile_ohwi(f16(w), N2, C, 1, true, wt.data());
    std::vector<float> bt(N2, 0.f);
    if (bias)
      for (int o = 0; o < N2; ++o) bt[geglu_row(o, N2)] = bias[o];
    half_t* dout = sc.out<half_t>((size_t)M * half_n, "out");
    ConvDesc d = token_gemm(sc.dev<half_t>((size_t)M * C, f16(x)), C, sc.dev<half_t>(wt.size(), wt.data()),
                            bias ? sc.dev<float>(N2, bt.data()) : nullptr, nullptr, dout, 1, M, N2);
    d.out_mode = kOutGeglu;
    const bool fast = conv_fast_path_ok(d);
    ConvWorkspace ws;
    sc.timed(iters, ms, [&] {
      if (fast)
        launch_conv(d, ws, sc.stream);
      else
        launch_conv_generic(d, 0, sc.stream);
    });
    SD_HIP(hipMemcpy(out, dout, (size_t)M * half_n * 2, hipMemcpyDeviceToHost));
  });
}

// GEGLU projection with the LayerNorm in front of it folded in (unet.py:583-591 norm3 -> :609-617 ff.net.0.proj) by the rule the
// UNet builder folds it with (fold_layernorm_rows): x (M, C) f16 un-normalised rows, ln_weight / ln_bias (C) f32 or both NULL (plain
// GEGLU), w (N2, C) f16 [values | gates], bias (N2) f32 or NULL -> out (M, N2 / 2) f16.
int sd_op_geglu_ln(const void* x, const float* ln_weight, const float* ln_bias, const void* w, const float* bias, void* out, int M, int C,
                   int N2, float eps, int kernel, int iters, float* ms) {
  return guarded([&] {
    const bool smgeglu = kernel >= 100 && kernel <= 112 && kernel % 10 <= 2;   // 100-102, 110-112: plan tile 13 (smgeglu.hip)
    const int sg_variant = smgeglu ? kernel % 10 : 0;                          // tile height by grid size / 128 rows / 256 rows
    const bool sg_clock = smgeglu && kernel >= 110;
    if (smgeglu) kernel = 0;
    const int abl = kernel / 10;   // kernel = 2 + 10 * n: ablation build n of the weight-stationary kernel (measurement tools only)
    kernel %= 10;
    SD_REQUIRE(x && w && out && N2 % 64 == 0 && (ln_weight == nullptr) == (ln_bias == nullptr) && kernel >= 0 && kernel <= 9 &&
                   (abl == 0 || kernel == 2), kInvalidArgument, "bad GEGLU arguments");
    Scratch sc("geglu_ln");
    const int half_n = N2 / 2;
    const FoldedProj f = upload_ln_folded(sc, w, bias, ln_weight, ln_bias, N2, C, true);
    half_t* dout = sc.out<half_t>((size_t)M * half_n, "out");
    ConvDesc d = token_gemm(sc.dev<half_t>((size_t)M * C, f16(x)), C, f.w, f.bias, nullptr, dout, 1, M, N2);
    if (ln_weight) d.ln_colsum = f.colsum;
    d.ln_eps = eps;
    d.out_mode = kOutGeglu;
    SD_REQUIRE(!smgeglu || smgeglu_shape_ok(d, sg_variant), kInvalidArgument,
               "GEGLU shape not eligible for plan tile 13 (smgeglu.hip): M=%d C=%d N2=%d", M, C, N2);
    SD_REQUIRE(conv_fast_path_ok(d), kUnsupported, "GEGLU shape off the MFMA path (C=%d N2=%d)", C, N2);
    // the wsgemm copy: where plan tile 10 is forced (kernel 2), else exactly where the planner names it for the library's own plan
    if (!smgeglu && (kernel == 2 ? wsgemm_shape_ok(d) : kernel == 0 && conv_plan_copies(d).wsgemm)) tile_for_wsgemm(sc, d);
    if (kernel == 2) d.tile = 10;
    size_t sg_prof = 0;
    if (smgeglu) {
      d.tile = 13;
      d.staging = sg_variant;
      if (sg_clock) {
        sg_prof = smgeglu_prof_entries(d, d.staging);
        d.prof = sc.out<long long>(sg_prof, "phase clock");
      }
    } else if (kernel >= 3) {
      tile_for_bvgemm(sc, d, "GEGLU shape not eligible for plan tile 11 (bvgemm.hip)");
      d.w_ws = nullptr;
      d.tile = 11;
      d.staging = kernel - 3;
    }
    d.debug = abl;
    if (abl == 5) d.prof = sc.out<long long>(64, "phase clock");
    ConvWorkspace ws;
    sc.timed(iters, ms, [&] { launch_conv(d, ws, sc.stream); });
    if (sg_prof) {   // every wave's stamps of the last launch: cycles from kernel entry to the end of each phase
      std::vector<long long> t(sg_prof);
      SD_HIP(hipMemcpy(t.data(), d.prof, sg_prof * sizeof(long long), hipMemcpyDeviceToHost));
      static const char* const phase[5] = {"first ring stages + epilogue operands issued", "first stage landed (counted wait + barrier)",
                                           "K loop done", "row statistics exchanged", "last store issued"};
      const size_t waves = sg_prof / 8;
      fprintf(stderr, "[sd prof] smgeglu M=%d K=%d N=%d kernel=%d: %zu waves, shader-clock cycles since the wave's kernel entry (min / mean / max)\n",
              M, C, N2, 110 + sg_variant, waves);
      for (int k = 1; k <= 5; ++k) {
        long long lo = LLONG_MAX, hi = 0;
        double sum = 0.0;
        for (size_t wv = 0; wv < waves; ++wv) {
          const long long dt = t[wv * 8 + k] - t[wv * 8];
          lo = std::min(lo, dt);
          hi = std::max(hi, dt);
          sum += (double)dt;
        }
        fprintf(stderr, "[sd prof]   %-46s %8lld %10.0f %8lld\n", phase[k - 1], lo, sum / (double)waves, hi);
      }
    } else if (d.prof) {   // workgroup (0, 0), thread 0: shader-clock stamps of its first pipeline iterations
      long long t[64];
      SD_HIP(hipMemcpy(t, d.prof, sizeof(t), hipMemcpyDeviceToHost));
      for (int i = 0; i < 6; ++i)
        fprintf(stderr, "[sd prof] wsgemm iteration %d: barrier wait %lld, DMA issue + store %lld, statistics %lld, MFMA || epilogue %lld cycles\n",
                i + 1, t[i * 8 + 1] - t[i * 8], t[i * 8 + 2] - t[i * 8 + 1], t[i * 8 + 3] - t[i * 8 + 2], t[i * 8 + 4] - t[i * 8 + 3]);
    }
    SD_HIP(hipMemcpy(out, dout, (size_t)M * half_n * 2, hipMemcpyDeviceToHost));
  });
}

// The same projection from PALETTIZED weights (plan tile 16).  Every check runs on the host in front of the first device call
// (Scratch), in the order the header lists them.  colsum and the folded bias come from lut[indices] by fold_layernorm_rows, as
// sd_op_geglu_ln computes them; the folded fp16 matrix is a host temporary.
int sd_op_geglu_palettized(const void* x, const float* ln_weight, const float* ln_bias, const void* lut, int nbits, const uint8_t* indices,
                           const float* bias, void* out, int M, int C, int N2, float eps, int bm, int* plan_out, int iters, float* ms) {
  return guarded([&] {
    SD_REQUIRE(palette_bits_ok(nbits), kInvalidArgument, "geglu_palettized: nbits = %d, not one of 1, 2, 4, 6, 8", nbits);
    SD_REQUIRE(bm == 0 || bm == 128 || bm == 256, kInvalidArgument, "geglu_palettized: bm = %d, not 0, 128 or 256", bm);
    SD_REQUIRE(x && lut && indices && out && plan_out, kInvalidArgument, "NULL argument");
    SD_REQUIRE(M > 0 && C > 0 && N2 > 0, kInvalidArgument, "geglu_palettized: empty problem");
    SD_REQUIRE((ln_weight == nullptr) == (ln_bias == nullptr), kInvalidArgument, "geglu_palettized: ln_weight and ln_bias go together");
    palette_check_indices("geglu_palettized", indices, (size_t)N2 * C, nbits);   // (in front of the shape: the header's order)
    static const float present = 0.f;   // the planner only tests the pointers
    ConvDesc d = token_gemm(nullptr, C, nullptr, &present, nullptr, nullptr, 1, M, N2);
    if (ln_weight) d.ln_colsum = &present;
    d.ln_eps = eps;
    d.out_mode = kOutGeglu;
    SD_REQUIRE(conv_fast_path_ok(d) && smgeglu_pal_shape_ok(d, conv_plan_pin(WeightSource::PalGeglu, bm).staging), kInvalidArgument,
               "geglu_palettized: shape not eligible for plan tile 16 (smgeglu.hip: M=%d C=%d N2=%d bm=%d - 128-row tiles only (256 is not "
               "built), C a multiple of 64 up to 2560, N2 of 160, M of 128, at least 2 x 2 tiles and a multiple of 8 of them)", M, C, N2, bm);
    std::vector<half_t> w((size_t)N2 * C), wf(w.size());
    for (size_t i = 0; i < w.size(); ++i) w[i] = f16(lut)[indices[i]];
    std::vector<float> bf(N2), cs(N2);
    fold_layernorm_rows(w.data(), bias, ln_weight, ln_bias, N2, C, 0, true, wf.data(), cs.data(), bf.data());
    Scratch sc("geglu_palettized");
    half_t* dout = sc.out<half_t>((size_t)M * (N2 / 2), "out");
    d.x0 = sc.dev<half_t>((size_t)M * C, f16(x));
    d.out = dout;
    d.bias = sc.dev<float>(N2, bf.data());
    HostWeights h;
    h.kind = WeightSource::PalGeglu; h.lut = lut; h.indices = indices; h.bits = nbits;
    upload_compressed(sc, d, "geglu_palettized", h, bm);
    if (ln_weight) {
      d.ln_colsum = sc.dev<float>(N2, cs.data());
      d.cw.ln_gamma = sc.dev<float>(C, ln_weight);
    }
    const ConvPlan p = conv_plan(d);
    plan_out[0] = p.tile; plan_out[1] = p.staging; plan_out[2] = p.splitk; plan_out[3] = p.slab ? 1 : 0;
    ConvWorkspace ws;
    sc.timed(iters, ms, [&] { launch_conv(d, ws, sc.stream); });
    SD_HIP(hipMemcpy(out, dout, (size_t)M * (N2 / 2) * 2, hipMemcpyDeviceToHost));
  });
}

int sd_op_palette_pack_geglu(const uint8_t* indices, int N2, int K, int nbits, uint8_t* stream, size_t* bytes) {
  return guarded([&] {
    SD_REQUIRE(indices && bytes, kInvalidArgument, "NULL argument");
    SD_REQUIRE(palette_bits_ok(nbits) && N2 > 0 && K > 0 && N2 % 32 == 0 && K % 64 == 0, kInvalidArgument,
               "palette_pack_geglu: nbits %d N2 %d K %d", nbits, N2, K);
    *bytes = smgemm_pal_bytes(N2, K, nbits);
    if (stream) smgeglu_pal_pack(indices, N2, K, nbits, stream);
  });
}

// Fused q|k|v projection of self-attention with norm1 folded in (unet.py:583-586 norm1 -> :74-84 to_q / to_k / to_v as ONE GEMM, as the
// UNet graph runs it): x (B * HW, C) f16 un-normalised tokens, ln_weight / ln_bias (C) f32, w (3C, C) f16 = [Wq | Wk | Wv] (no bias)
// -> out_qk (B * HW, 2C) f16 (the queries multiplied by q_scale on the fp32 accumulator), out_vt (B, C, HW) f16 = V^T, with
// vt_perm in attention8's key order (AttnDesc::vt_perm).
int sd_op_qkv_ln(const void* x, const float* ln_weight, const float* ln_bias, const void* w, void* out_qk, void* out_vt, int B, int HW, int C,
                 float eps, float q_scale, int vt_perm, int kernel, int iters, float* ms) {
  return guarded([&] {
    SD_REQUIRE(x && ln_weight && ln_bias && w && out_qk && out_vt && B >= 1 && HW >= 1 && C % 64 == 0 && kernel >= 0 && kernel <= 9,
               kInvalidArgument, "bad q|k|v arguments");
    Scratch sc("qkv_ln");
    const int N = 3 * C, M = B * HW;
    const FoldedProj f = upload_ln_folded(sc, w, nullptr, ln_weight, ln_bias, N, C, false);
    half_t* dqk = sc.out<half_t>((size_t)M * 2 * C, "out_qk");
    half_t* dvt = sc.out<half_t>((size_t)B * C * HW, "out_vt");
    ConvDesc d = qkv_desc(sc.dev<half_t>((size_t)M * C, f16(x)), f, eps, dqk, dvt, B, 1, HW, C, q_scale, vt_perm);
    SD_REQUIRE(conv_fast_path_ok(d), kUnsupported, "q|k|v shape off the MFMA path (C=%d)", C);
    const ConvWeightCopies copies = conv_plan_copies(d);   // what the library's own plan (kernel 0) reads
    if (kernel == 2 || (kernel == 0 && copies.wsgemm)) {   // the weight-stationary kernel (wsgemm.hip, plan tile 10)
      SD_REQUIRE(wsgemm_shape_ok(d), kInvalidArgument, "q|k|v shape not eligible for plan tile 10 (wsgemm.hip)");
      tile_for_wsgemm(sc, d);
      if (kernel == 2) d.tile = 10;
    } else if (kernel >= 3 || (kernel == 0 && copies.bvgemm)) {
      tile_for_bvgemm(sc, d, "q|k|v shape not eligible for plan tile 11 (bvgemm.hip)");
      if (kernel >= 3) {
        d.tile = 11;
        d.staging = kernel - 3;
      }
    }
    ConvWorkspace ws;
    sc.timed(iters, ms, [&] { launch_conv(d, ws, sc.stream); });
    SD_HIP(hipMemcpy(out_qk, dqk, (size_t)M * 2 * C * 2, hipMemcpyDeviceToHost));
    SD_HIP(hipMemcpy(out_vt, dvt, (size_t)B * C * HW * 2, hipMemcpyDeviceToHost));
  });
}

// The head of a SpatialTransformer (unet.py:553-556 norm -> proj_in, :583-586 norm1 -> :74-84 fused to_q | to_k | to_v) behind a 1x1 conv
// that produces its input x = conv(x_in) and - like the resnet conv in front of it in the UNet - leaves the GroupNorm statistics of x in
// its epilogue.  fused = 1: ONE launch (xattn_out.hip gn_proj_qkv_kernel; 2 / 3: its 64- / 32-token form); 0: GroupNorm launch, proj_in GEMM,
// LayerNorm-folded q|k|v GEMM.
// x_in (B, C, H, W) f16 NCHW; conv_w (C, C); gn_* (C) f32; proj_w (C, C), proj_bias (C); ln_* (C); wqkv (3C, C) -> out_h (B * HW, C),
// out_qk (B * HW, 2C), out_vt (B, C, HW), all f16.  *entries = the producer's partial entries per (sample, group) the fused launch folded.
int sd_op_gn_proj_qkv(const void* x_in, const void* conv_w, const float* gn_weight, const float* gn_bias, const void* proj_w,
                      const float* proj_bias, const float* ln_weight, const float* ln_bias, const void* wqkv, void* out_h, void* out_qk,
                      void* out_vt, int B, int H, int W, int C, int groups, float gn_eps, float ln_eps, float q_scale, int vt_perm, int fused,
                      int* entries, int iters, float* ms) {
  return guarded([&] {
    SD_REQUIRE(x_in && conv_w && gn_weight && gn_bias && proj_w && proj_bias && ln_weight && ln_bias && wqkv && out_h && out_qk && out_vt,
               kInvalidArgument, "NULL argument");
    const int HW = H * W, M = B * HW, N = 3 * C;
    SD_REQUIRE(gn_proj_qkv_ok(C, C / 64, HW, M, HW, groups), kInvalidArgument, "gn_proj_qkv: C=%d HW=%d groups=%d", C, HW, groups);
    Scratch sc("gn_proj_qkv");
    half_t* dx = sc.out<half_t>((size_t)M * C, "producer's output x");
    // the producer
    ConvDesc d = conv_desc(upload_nhwc(sc, x_in, B, C, H, W), C, sc.dev<half_t>((size_t)C * C, f16(conv_w)), nullptr, nullptr, dx, B, H, W, C);
    d.splitk = 1;
    float* partial = poisoned_gn_partial(sc, B, HW, groups);
    d.gn_partial = partial;
    d.gn_groups = groups;
    float* dgw = sc.dev<float>(C, gn_weight);
    float* dgb = sc.dev<float>(C, gn_bias);
    const FoldedProj fq = upload_ln_folded(sc, wqkv, nullptr, ln_weight, ln_bias, N, C, false);   // LayerNorm fold of the fused q|k|v
    half_t* dwp = sc.dev<half_t>((size_t)C * C, f16(proj_w));
    float* dpb = sc.dev<float>(C, proj_bias);
    half_t* dnorm = sc.out<half_t>((size_t)M * C, "normalised tensor");
    half_t* dh = sc.out<half_t>((size_t)M * C, "out_h");
    half_t* dqk = sc.out<half_t>((size_t)M * 2 * C, "out_qk");
    half_t* dvt = sc.out<half_t>((size_t)B * C * HW, "out_vt");
    half_t* dwp_t = sc.out<half_t>((size_t)C * C, "wp_t");
    half_t* dwq_t = sc.out<half_t>((size_t)N * C, "wqkv_t");
    launch_xattn_out_retile_nk(dwp, dwp_t, C, C, sc.stream);
    launch_xattn_out_retile_nk(fq.w, dwq_t, N, C, sc.stream);
    ConvDesc pd = conv_desc(dnorm, C, dwp, dpb, nullptr, dh, B, H, W, C);                      // proj_in of the three-launch path
    ConvDesc qd = qkv_desc(dh, fq, ln_eps, dqk, dvt, B, H, W, C, q_scale, vt_perm);            // fused q|k|v of the three-launch path
    SD_REQUIRE(conv_fast_path_ok(d) && conv_fast_path_ok(pd) && conv_fast_path_ok(qd), kInvalidArgument, "gn_proj_qkv: off the MFMA path");
    ConvWorkspace ws = workspace_for(sc, {d, pd, qd});
    int n_entries = 0;
    static const bool want_clk = tune_env_set("SD_GQ_CLOCK");   // phase clock of the one-launch kernel, printed to stderr
    const size_t n_clk = (size_t)(M / 32) * 5 * 16;
    long long* dclk = want_clk && fused ? sc.out<long long>(n_clk, "phase clock") : nullptr;
    sc.timed(iters, ms, [&] {
      n_entries = launch_conv(d, ws, sc.stream);
      const bool have = n_entries >= 1 && n_entries <= 128;
      if (fused) {
        GnProjQkvDesc g;
        g.clk = dclk;
        g.tok = fused == 2 ? 64 : (fused == 3 ? 32 : 0);   // operator tests: the 64- / 32-token form whatever the launch's rule says
        g.x = dx;
        if (have) {
          g.gn_partial = partial; g.gn_gamma = dgw; g.gn_beta = dgb; g.gn_entries = n_entries;
        } else {   // no producer statistics: the GroupNorm launch, then the fused launch on the normalised tensor
          launch_groupnorm(dx, C, nullptr, 0, partial, dgw, dgb, dnorm, B, HW, groups, gn_eps, 0, sc.stream, n_entries);
          g.x = dnorm;
        }
        g.gn_groups = groups; g.gn_eps = gn_eps;
        g.wp_t = dwp_t; g.p_bias = dpb; g.h = dh;
        g.wqkv_t = dwq_t; g.qkv_bias = fq.bias; g.qkv_colsum = fq.colsum; g.ln_eps = ln_eps;
        g.qk = dqk; g.vt = dvt; g.M = M; g.C = C; g.S = HW; g.ldT = HW; g.vt_perm = vt_perm != 0; g.q_scale = q_scale;
        launch_gn_proj_qkv(g, sc.stream);
      } else {
        launch_groupnorm(dx, C, nullptr, 0, partial, dgw, dgb, dnorm, B, HW, groups, gn_eps, 0, sc.stream, n_entries);
        launch_conv(pd, ws, sc.stream);
        launch_conv(qd, ws, sc.stream);
      }
    });
    if (entries) *entries = (fused && n_entries >= 1 && n_entries <= 128) ? n_entries : 0;
    if (dclk) {
      std::vector<long long> hc(n_clk);
      SD_HIP(hipMemcpy(hc.data(), dclk, n_clk * sizeof(long long), hipMemcpyDeviceToHost));
      static const char* names[13] = {"start -> group statistics folded", "-> constants in LDS", "-> normalised tile in LDS", "-> proj_in MFMAs issued",
                                      "-> h tile in LDS", "-> q MFMAs", "-> q stored", "-> k MFMAs", "-> k stored", "-> v MFMAs", "-> V^T stored", "", ""};
      const size_t nw = n_clk / 16;
      double total = 0;
      for (int ph = 1; ph <= 11; ++ph) {
        double sum = 0, mx = 0;
        for (size_t w = 0; w < nw; ++w) {
          const double dlt = (double)(hc[w * 16 + ph] - hc[w * 16 + ph - 1]);
          sum += dlt;
          mx = std::max(mx, dlt);
        }
        total += sum / nw;
        fprintf(stderr, "gn_proj_qkv phase %2d  mean %8.0f  max %8.0f cycles   %s\n", ph, sum / nw, mx, names[ph - 1]);
      }
      fprintf(stderr, "gn_proj_qkv mean wave %8.0f cycles (%zu waves; the XCDs' counters are not synchronised: no launch-wide span)\n", total, nw);
    }
    SD_HIP(hipMemcpy(out_h, dh, (size_t)M * C * 2, hipMemcpyDeviceToHost));
    SD_HIP(hipMemcpy(out_qk, dqk, (size_t)M * 2 * C * 2, hipMemcpyDeviceToHost));
    SD_HIP(hipMemcpy(out_vt, dvt, (size_t)B * C * HW * 2, hipMemcpyDeviceToHost));
  });
}

// the descriptor sd_op_conv_plan / sd_op_conv_plan_kernel ask about and its plan; c: the copies a handle of the library holds for it
static ConvPlan query_conv_plan(int ksize, int stride, int up, int C0, int C1, int N, int B, int Ho, int Wo, int out_mode, int flags, int n_trans,
                                int n_twins, int gnf_groups, int tile, int staging, int splitk, int copies, ConvWeightCopies& c) {
  SD_REQUIRE(ksize >= 1 && stride >= 1 && up >= 1 && C0 >= 1 && C1 >= 0 && N >= 1 && B >= 1 && Ho >= 1 && Wo >= 1 &&
                 n_trans >= 0 && n_twins >= 0 && n_twins <= 2 && gnf_groups >= 0 && copies >= -1 && copies <= 7,
             kInvalidArgument, "bad conv_plan arguments");
  static const float present[4] = {};   // the planner only tests these pointers
  const half_t* ph = reinterpret_cast<const half_t*>(present);
  ConvDesc d;
  d.x0 = d.w = ph;
  d.C0 = C0;
  if (C1 > 0) d.x1 = ph, d.C1 = C1;
  d.B = B; d.Ho = Ho; d.Wo = Wo; d.Hi = Ho * stride / up; d.Wi = Wo * stride / up;
  d.ksize = ksize; d.stride = stride; d.up = up; d.N = N; d.out_mode = out_mode;
  if (flags & 1) d.ln_colsum = present;
  if (flags & 2) d.temb = present;
  if (flags & 4) d.res = ph;
  if (flags & 8) d.gn_partial = const_cast<float*>(present), d.gn_groups = 32;
  if (flags & 16) d.bias = present;
  if (flags & 32) d.pad = 0;
  if (flags & 64) d.subpix = true;   // the upsampler as four 2x2 phase convs: plan tile 21 or a refusal
  if (n_trans > 0) d.out_t = const_cast<half_t*>(ph), d.n_trans = n_trans, d.ldT = Ho * Wo;
  d.n_twins = n_twins;
  if (gnf_groups > 0) {   // GroupNorm of the input folded into this launch, as the UNet's resnets / transformers ask for it
    d.gnf_partial = d.gnf_gamma = d.gnf_beta = present;
    d.gnf_groups = gnf_groups;
    d.gnf_entries = 1;
    d.gnf_silu = ksize == 3 ? 1 : 0;
  }
  d.tile = tile; d.staging = staging; d.splitk = splitk;
  if (tile == 17) {   // a W8A8 descriptor carries its int8 stream and scales (the planner only tests the pointers)
    d.w = nullptr;
    d.cw.kind = WeightSource::I8Wstream;
    d.cw.stream = d.cw.scale = present;
    d.cw.inv_s = 1.f;
  }
  if (tile == 18) {   // ... and so does one of the int8 halo conv
    d.w = nullptr;
    d.cw.kind = WeightSource::I8Halo;
    d.cw.stream = d.cw.scale = present;
    d.cw.inv_s = 1.f;
  }
  if (tile == 25) {   // ... and a palettized one of the halo conv its index stream and LUT
    d.w = nullptr;
    d.cw.kind = WeightSource::PalHalo;
    d.cw.stream = present;
    d.cw.lut = ph;
    d.cw.bits = 8;
  }
  if (tile == 19) {   // ... and one of the int8 small-M GEMM
    d.w = nullptr;
    d.cw.kind = WeightSource::I8Gemm;
    d.cw.stream = d.cw.scale = present;
    d.cw.inv_s = 1.f;
  }
  if (tile == 20) {   // ... and one of the int8 GEGLU projection, whose activations arrive as int8 too
    d.w = nullptr;
    d.cw.kind = WeightSource::I8Geglu;
    d.cw.stream = d.cw.scale = present;
    d.cw.inv_s = 1.f;
    d.x0_i8 = reinterpret_cast<const int8_t*>(present);
  }
  if (tile == 24) {   // ... and one of the int8 small-M GEMM whose activations arrive as int8
    d.w = nullptr;
    d.cw.kind = WeightSource::I8GemmQ;
    d.cw.stream = d.cw.scale = present;
    d.cw.inv_s = 1.f;
    d.x0_i8 = reinterpret_cast<const int8_t*>(present);
  }
  if (tile == 22) {   // ... and one of the int8 q|k|v projection (asked with n_trans = 2 C0, as the fused q|k|v launch is)
    d.w = nullptr;
    d.cw.kind = WeightSource::I8Qkv;
    d.cw.stream = d.cw.scale = present;
    d.cw.inv_s = 1.f;
    d.x0_i8 = reinterpret_cast<const int8_t*>(present);
  }
  c = conv_plan_copies(d);
  if (copies < 0) copies = (c.wstream ? 1 : 0) | (c.wsgemm ? 2 : 0) | (c.bvgemm ? 4 : 0);   // what a handle of the library holds
  if (copies & 1) d.w_tiled = ph;
  if (copies & 2) d.w_ws = ph;
  if (copies & 4) d.w_bv = ph;
  return conv_plan(d);
}

// Which plan does a conv / 1x1 GEMM of this shape get (conv_plan.h)?  Host only: no GPU, nothing launched.
int sd_op_conv_plan(int ksize, int stride, int up, int C0, int C1, int N, int B, int Ho, int Wo, int out_mode, int flags, int n_trans,
                    int n_twins, int gnf_groups, int tile, int staging, int splitk, int copies, int* plan, unsigned long long* workspace_bytes) {
  return guarded([&] {
    SD_REQUIRE(plan && workspace_bytes, kInvalidArgument, "bad conv_plan arguments");
    ConvWeightCopies c;
    const ConvPlan p = query_conv_plan(ksize, stride, up, C0, C1, N, B, Ho, Wo, out_mode, flags, n_trans, n_twins, gnf_groups, tile, staging, splitk, copies, c);
    plan[0] = p.tile; plan[1] = p.staging; plan[2] = p.splitk; plan[3] = p.slab ? 1 : 0;
    plan[4] = c.wstream ? 1 : 0; plan[5] = c.wsgemm ? 1 : 0; plan[6] = c.bvgemm ? 1 : 0;
    *workspace_bytes = p.workspace_bytes;
  });
}

// The same question, answered with the kernel that launches: conv_plan_kernel_name (conv_plan.h) of the plan, NUL-terminated into text
int sd_op_conv_plan_kernel(int ksize, int stride, int up, int C0, int C1, int N, int B, int Ho, int Wo, int out_mode, int flags, int n_trans,
                           int n_twins, int gnf_groups, int tile, int staging, int splitk, int copies, char* text, int text_bytes) {
  return guarded([&] {
    SD_REQUIRE(text && text_bytes >= 1, kInvalidArgument, "bad conv_plan_kernel arguments");
    ConvWeightCopies c;
    const std::string name = conv_plan_kernel_name(
        query_conv_plan(ksize, stride, up, C0, C1, N, B, Ho, Wo, out_mode, flags, n_trans, n_twins, gnf_groups, tile, staging, splitk, copies, c));
    SD_REQUIRE((int)name.size() < text_bytes, kInvalidArgument, "conv_plan_kernel: the text buffer holds %d bytes, the line needs %zu", text_bytes, name.size() + 1);
    memcpy(text, name.c_str(), name.size() + 1);
  });
}

int sd_op_timestep_embedding(const float* t, float* out, int n, int dim, int flip_sin_to_cos, float freq_shift) {
  return guarded([&] {
    SD_REQUIRE(t && out && n > 0 && dim > 0 && dim % 2 == 0, kInvalidArgument, "bad arguments");
    SD_REQUIRE(flip_sin_to_cos == 1, kUnsupported, "flip_sin_to_cos=False is not on the path");
    Scratch sc("timestep_embedding");
    float* dt = sc.dev<float>(n, t);
    float* dout = sc.out<float>((size_t)n * dim, "out");
    std::vector<float> f = timestep_freq_table(dim, freq_shift);
    float* df = sc.dev<float>(f.size(), f.data());
    launch_timestep_embedding(dt, df, dout, n, dim, sc.stream);
    SD_HIP(hipStreamSynchronize(sc.stream));
    SD_HIP(hipMemcpy(out, dout, (size_t)n * dim * sizeof(float), hipMemcpyDeviceToHost));
  });
}

// The image-to-image start on its own (misc.hip posterior_noise_kernel): moments (2 * Cz, h, w) f32 = [mean | logvar] of one image,
// eps (Cz, h, w), noise / out (n_images, Cz, h, w) f32.
int sd_op_posterior_noise(const float* moments, const float* eps, const float* noise, float* out, int Cz, int h, int w, int n_images,
                          float scale_factor, float sa, float sb, int iters, float* ms) {
  return guarded([&] {
    SD_REQUIRE(moments && eps && noise && out, kInvalidArgument, "NULL argument");
    SD_REQUIRE(Cz > 0 && h > 0 && w > 0 && n_images > 0, kInvalidArgument, "posterior_noise: Cz=%d h=%d w=%d n_images=%d", Cz, h, w, n_images);
    Scratch sc("posterior_noise");
    const size_t n = (size_t)Cz * h * w, total = (size_t)n_images * n;
    float* dm = sc.dev<float>(2 * n, moments);
    float* de = sc.dev<float>(n, eps);
    float* dn = sc.dev<float>(total, noise);
    float* dout = sc.out<float>(total, "out");
    sc.timed(iters, ms, [&] { launch_posterior_noise(dm, de, dn, dout, n, n_images, scale_factor, sa, sb, sc.stream); });
    SD_HIP(hipMemcpy(out, dout, total * sizeof(float), hipMemcpyDeviceToHost));
  });
}

// One launch of cfg_sched_step_kernel (misc.hip) the way the loop launches it, from a zeroed step counter and ticket; the one-row
// tables sit at step 0.
int sd_op_sched_step(const float* noise_pred, float* latents, float* hist, const float* coef, const float* pred, const float* step_noise,
                     float guidance, int cfg, int history, int n_images, int n, float* denoised, int* step_after) {
  return guarded([&] {
    SD_REQUIRE(noise_pred && latents && coef && step_after, kInvalidArgument, "NULL argument");
    SD_REQUIRE((cfg == 1 || cfg == 2) && history >= 0 && history <= 3 && n_images > 0 && n > 0, kInvalidArgument,
               "sched_step: cfg=%d history=%d n_images=%d n=%d", cfg, history, n_images, n);
    SD_REQUIRE((history == 0 || hist) && (pred != nullptr) == (denoised != nullptr), kInvalidArgument,
               "sched_step: history > 0 needs hist, and pred and denoised go together");
    Scratch sc("sched_step");
    const size_t total = (size_t)n_images * n;
    float* dnp = sc.dev<float>((size_t)cfg * total, noise_pred);
    float* dlat = sc.dev<float>(total, latents, "latents");
    float* dhist = history ? sc.dev<float>((size_t)history * total, hist, "history entries") : nullptr;
    float* dden = pred ? sc.out<float>(total, "de-noised latents") : nullptr;
    // zeroed: [0] the step counter, which the loop starts at 0 and the kernel advances, [1] the arrival ticket, which the last
    // workgroup to arrive puts back to 0
    int* dstep = sc.zeroed<int>(2, "step counter | ticket");
    LoopTables tab{};
    tab.coef = sc.dev<float>(8, coef);
    tab.step = dstep;
    tab.ticket = reinterpret_cast<unsigned*>(dstep + 1);
    if (step_noise) tab.noise_tab = sc.dev<float>(total, step_noise);
    if (pred) {
      tab.pred = sc.dev<float>(8, pred);
      tab.denoised = dden;
    }
    launch_cfg_sched_step(dnp, dlat, dhist, tab, guidance, n_images, n, cfg, history, sc.stream);
    SD_HIP(hipStreamSynchronize(sc.stream));
    int st[2];
    SD_HIP(hipMemcpy(st, dstep, sizeof(st), hipMemcpyDeviceToHost));
    SD_REQUIRE(st[1] == 0, kInternal, "sched_step left its arrival ticket at %d", st[1]);
    *step_after = st[0];
    SD_HIP(hipMemcpy(latents, dlat, total * sizeof(float), hipMemcpyDeviceToHost));
    if (dhist) SD_HIP(hipMemcpy(hist, dhist, (size_t)history * total * sizeof(float), hipMemcpyDeviceToHost));
    if (dden) SD_HIP(hipMemcpy(denoised, dden, total * sizeof(float), hipMemcpyDeviceToHost));
  });
}

// Pillow's 8-bit bicubic coefficients of one axis (imgpost.hip resample_coeffs; host only): bounds (out_size, 2) = [xmin, n], coeffs
// (out_size, *ksize), zeros behind the n taps of a row.  A NULL table pointer: the size query, *ksize alone.
int sd_op_resample_coeffs(int in_size, int out_size, int* ksize, int32_t* bounds, int32_t* coeffs) {
  return guarded([&] {
    SD_REQUIRE(ksize, kInvalidArgument, "NULL argument");
    SD_REQUIRE(in_size >= 1 && out_size >= 1 && in_size <= (1 << 20) && out_size <= (1 << 20), kInvalidArgument, "resample_coeffs: %d -> %d",
               in_size, out_size);
    *ksize = resample_ksize(in_size, out_size);
    if (bounds && coeffs) resample_coeffs(in_size, out_size, bounds, coeffs);
  });
}

// imgpost.hip image_rgb8_kernel on host arrays: image (B, 3, H, W) f32 -> rgb8 (B, H, W, 3).
int sd_op_image_rgb8(const float* image, uint8_t* rgb8, int B, int H, int W, int iters, float* ms) {
  return guarded([&] {
    SD_REQUIRE(image && rgb8, kInvalidArgument, "NULL argument");
    SD_REQUIRE(B > 0 && H > 0 && W > 0, kInvalidArgument, "image_rgb8: B=%d H=%d W=%d", B, H, W);
    Scratch sc("image_rgb8");
    const size_t n = (size_t)B * H * W * 3;
    float* din = sc.dev<float>(n, image);
    uint8_t* dout = sc.out<uint8_t>(n, "rgb8", kOpGuard, 0xa5);   // (0xff is white: the bytes start as 0xa5)
    sc.timed(iters, ms, [&] { launch_image_rgb8(din, dout, B, H, W, sc.stream); });
    SD_HIP(hipMemcpy(rgb8, dout, n, hipMemcpyDeviceToHost));
  });
}

// imgpost.hip clip_input_kernel on host arrays: rgb8 (B, H, W, 3) -> clip_input (B, 3, S, S) f16.  The geometry is checked and the
// tables are built on the host before any device work.
int sd_op_clip_input(const uint8_t* rgb8, void* clip_input, int B, int H, int W, int rh, int rw, int S, const float* mean3, const float* std3,
                     int iters, float* ms) {
  return guarded([&] {
    SD_REQUIRE(rgb8 && clip_input && mean3 && std3, kInvalidArgument, "NULL argument");
    SD_REQUIRE(B > 0, kInvalidArgument, "clip_input: B=%d", B);
    const ClipInputPlan plan = plan_clip_input(H, W, rh, rw, S);
    ClipInputDesc d{};
    for (int c = 0; c < 3; ++c) {
      SD_REQUIRE(std3[c] != 0.f, kInvalidArgument, "clip_input: std[%d] is 0", c);
      d.mean[c] = mean3[c], d.std[c] = std3[c];
    }
    Scratch sc("clip_input");
    d.hbounds = sc.dev<int32_t>(plan.hbounds.size(), plan.hbounds.data());
    d.hcoeffs = sc.dev<int32_t>(plan.hcoeffs.size(), plan.hcoeffs.data());
    d.vbounds = sc.dev<int32_t>(plan.vbounds.size(), plan.vbounds.data());
    d.vcoeffs = sc.dev<int32_t>(plan.vcoeffs.size(), plan.vcoeffs.data());
    d.H = H, d.W = W, d.S = S, d.top = (rh - S) / 2, d.left = (rw - S) / 2, d.ksh = plan.ksh, d.ksv = plan.ksv;
    const size_t n = (size_t)B * 3 * S * S;
    uint8_t* din = sc.dev<uint8_t>((size_t)B * H * W * 3, rgb8);
    half_t* dout = sc.out<half_t>(n, "clip_input");
    sc.timed(iters, ms, [&] { launch_clip_input(din, dout, B, d, plan.lds_bytes, sc.stream); });
    SD_HIP(hipMemcpy(clip_input, dout, n * sizeof(half_t), hipMemcpyDeviceToHost));
  });
}

// The safety checker's attention (vit.hip) on the layout its handle feeds it: qkv (B * S, 3 * heads * d) f16 rows [q | k | v] ->
// out (B * S, heads * d) f16.
int sd_op_vit_attention(const void* qkv, void* out, int B, int S, int heads, int d, int iters, float* ms) {
  return guarded([&] {
    SD_REQUIRE(qkv && out, kInvalidArgument, "NULL argument");
    SD_REQUIRE(B > 0 && S > 0 && heads > 0 && d > 0, kInvalidArgument, "empty attention problem");
    SD_REQUIRE(vit_attention_ok(d), kUnsupported, "vit_attention: head dim %d (the kernel is built for 64)", d);
    Scratch sc("vit_attention");
    const int D = heads * d;
    const size_t n = (size_t)B * S * D;
    half_t* dq = sc.dev<half_t>((size_t)B * S * 3 * D, f16(qkv));
    half_t* dout = sc.out<half_t>(n, "out", (size_t)64 * D);   // a guard of 64 rows: one query tile
    sc.timed(iters, ms, [&] { launch_vit_attention(dq, dout, B, S, heads, d, sc.stream); });
    SD_HIP(hipMemcpy(out, dout, n * sizeof(half_t), hipMemcpyDeviceToHost));
  });
}

// The VAE's mid-block attention (vae_attention.hip) on the layout its handle feeds it: q / k / v (B * S, C) f16 -> out (B * S, C) f16.
// Everything that can be refused is refused before any device work.
int sd_op_vae_attention(const void* q, const void* k, const void* v, void* out, int B, int S, int C, int iters, float* ms) {
  return guarded([&] {
    SD_REQUIRE(q && k && v && out, kInvalidArgument, "NULL argument");
    SD_REQUIRE(B > 0 && S > 0 && C > 0, kInvalidArgument, "empty attention problem");
    SD_REQUIRE(vae_attention_ok(C), kUnsupported, "vae_attention: head dim %d (the kernel is built for 64, 128, 256 and 512)", C);
    SD_REQUIRE(B <= 65535, kInvalidArgument, "vae_attention: B=%d", B);
    Scratch sc("vae_attention");
    const size_t n = (size_t)B * S * C;
    half_t* dq = sc.dev<half_t>(n, f16(q));
    half_t* dk = sc.dev<half_t>(n, f16(k));
    half_t* dv = sc.dev<half_t>(n, f16(v));
    half_t* dout = sc.out<half_t>(n, "out", (size_t)64 * C);   // a guard of 64 rows: one query tile
    sc.timed(iters, ms, [&] { launch_vae_attention(dq, dk, dv, dout, B, S, C, sc.stream); });
    SD_HIP(hipMemcpy(out, dout, n * sizeof(half_t), hipMemcpyDeviceToHost));
  });
}

// The safety checker's concept head (vit.hip safety_head_kernel) on host fp32 arrays
int sd_op_safety_head(const float* image_embeds, const float* concept_embeds, const float* special_embeds, const float* concept_w,
                      const float* special_w, float adjustment, int B, int P, int n_concepts, int n_special, float* has_nsfw,
                      float* concept_scores) {
  return guarded([&] {
    SD_REQUIRE(image_embeds && concept_embeds && concept_w && has_nsfw && concept_scores, kInvalidArgument, "NULL argument");
    SD_REQUIRE(B > 0 && P > 0 && n_concepts > 0 && n_special >= 0 && (n_special == 0 || (special_embeds && special_w)), kInvalidArgument,
               "safety_head: B=%d P=%d concepts=%d special=%d", B, P, n_concepts, n_special);
    Scratch sc("safety_head");
    float* di = sc.dev<float>((size_t)B * P, image_embeds);
    float* dc = sc.dev<float>((size_t)n_concepts * P, concept_embeds);
    float* dcw = sc.dev<float>(n_concepts, concept_w);
    float* ds = n_special ? sc.dev<float>((size_t)n_special * P, special_embeds) : nullptr;
    float* dsw = n_special ? sc.dev<float>(n_special, special_w) : nullptr;
    float* dadj = sc.dev<float>(1, &adjustment);
    float* dflag = sc.out<float>(B, "has_nsfw");
    float* dscore = sc.out<float>((size_t)B * n_concepts, "concept_scores");
    launch_safety_head(di, dc, ds, dcw, dsw, dadj, B, P, n_concepts, n_special, dflag, dscore, sc.stream);
    SD_HIP(hipStreamSynchronize(sc.stream));
    SD_HIP(hipMemcpy(has_nsfw, dflag, (size_t)B * sizeof(float), hipMemcpyDeviceToHost));
    SD_HIP(hipMemcpy(concept_scores, dscore, (size_t)B * n_concepts * sizeof(float), hipMemcpyDeviceToHost));
  });
}

// ---------------------------------------------------------------------------------------------------------------------------
// The kernels that only whole models used to reach (vae_f32.hip, norm.hip row_softmax, misc.hip, clip.hip, vit.hip's two layout
// kernels), one entry point each.  Everything that can be refused is refused before any device work; every device output sits in
// front of a guard of NaN patterns that the launch must leave alone, and starts out poisoned itself.
// ---------------------------------------------------------------------------------------------------------------------------
// vae_f32.hip conv_f32_kernel as Net::conv_f32 / the fp32 attention drive it: x (B,Cin,H,W) f32; w_kind 0: w f16 (N,Cin,k,k), 1: w f32
// (N,Cin,k,k) - both through retile_ohwi - 2: w f32 (K = Cin, N) as it stands, ksize 1 only (attention's V); bias (N) / res
// (B,N,Ho,Wo) f32 or NULL; pad_mode as sd_op_conv2d_ex -> out (B,N,Ho,Wo) f32
int sd_op_conv_f32(const float* x, const void* w, int w_kind, const float* bias, const float* res, float* out, int B, int Cin, int H, int W,
                   int N, int ksize, int stride, int upsample, int pad_mode) {
  return guarded([&] {
    SD_REQUIRE(x && w && out, kInvalidArgument, "NULL argument");
    SD_REQUIRE(B > 0 && Cin > 0 && H > 0 && W > 0 && N > 0, kInvalidArgument, "conv_f32: B=%d Cin=%d H=%d W=%d N=%d", B, Cin, H, W, N);
    SD_REQUIRE((ksize == 1 || ksize == 3) && (stride == 1 || stride == 2) && (upsample == 0 || upsample == 1), kInvalidArgument,
               "conv_f32: ksize %d stride %d upsample %d not on the path", ksize, stride, upsample);
    SD_REQUIRE(w_kind >= 0 && w_kind <= 2 && (w_kind != 2 || ksize == 1), kInvalidArgument, "conv_f32: w_kind %d with ksize %d (2 = [K][N], ksize 1 only)",
               w_kind, ksize);
    SD_REQUIRE(pad_mode == 0 || (pad_mode == 1 && ksize == 3 && stride == 2 && !upsample), kInvalidArgument,
               "conv_f32: pad_mode %d (1 = the (0,1,0,1) padding of a 3x3 / stride-2 conv without upsample)", pad_mode);
    const int up = upsample ? 2 : 1, pad = ksize / 2;
    const int Ho = pad_mode ? (H * up + 1 - ksize) / stride + 1 : (H * up + 2 * pad - ksize) / stride + 1;
    const int Wo = pad_mode ? (W * up + 1 - ksize) / stride + 1 : (W * up + 2 * pad - ksize) / stride + 1;
    SD_REQUIRE(Ho >= 1 && Wo >= 1, kInvalidArgument, "conv_f32: empty output (%dx%d)", Ho, Wo);
    const size_t nw = (size_t)N * Cin * ksize * ksize, nout = (size_t)B * Ho * Wo * N;
    Scratch sc("conv_f32");
    ConvF32Desc d;
    const std::vector<float> xh = host_nhwc(x, B, Cin, H * W);
    d.x = sc.dev<float>(xh.size(), xh.data());
    if (w_kind == 0) {
      std::vector<half_t> t(nw);
      retile_ohwi(f16(w), N, Cin, ksize, false, t.data());
      d.w = sc.dev<half_t>(nw, t.data());
    } else if (w_kind == 1) {
      std::vector<float> t(nw);
      retile_ohwi(reinterpret_cast<const float*>(w), N, Cin, ksize, false, t.data());
      d.w = sc.dev<float>(nw, t.data());
    } else {
      d.w = sc.dev<float>(nw, reinterpret_cast<const float*>(w));
    }
    d.w_kind = w_kind;
    d.bias = bias ? sc.dev<float>(N, bias) : nullptr;
    if (res) {
      const std::vector<float> rh = host_nhwc(res, B, N, Ho * Wo);
      d.res = sc.dev<float>(rh.size(), rh.data());
    }
    float* dout = sc.out<float>(nout, "out");
    d.out = dout;
    d.B = B; d.Hi = H; d.Wi = W; d.Cin = Cin; d.Ho = Ho; d.Wo = Wo; d.N = N;
    d.ksize = ksize; d.stride = stride; d.up = up;
    if (pad_mode) d.pad = 0;
    launch_conv_f32(d, sc.stream);
    SD_HIP(hipStreamSynchronize(sc.stream));
    host_nchw(download(dout, nout), out, B, N, Ho * Wo);
  });
}

// vae_f32.hip groupnorm_f32_* (statistics, finalize, apply): x (B,C,H,W) f32, gamma / beta (C) -> out (B,C,H,W) f32.  The statistics
// scratch starts out as NaN patterns: a slab entry that is read without having been written shows.
int sd_op_groupnorm_f32(const float* x, const float* gamma, const float* beta, float* out, int B, int C, int H, int W, int groups, float eps,
                        int silu) {
  return guarded([&] {
    SD_REQUIRE(x && gamma && beta && out, kInvalidArgument, "NULL argument");
    SD_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && groups > 0, kInvalidArgument, "groupnorm_f32: B=%d C=%d H=%d W=%d groups=%d", B, C, H, W, groups);
    SD_REQUIRE(C % groups == 0, kUnsupported, "groupnorm_f32: %d channels, %d groups", C, groups);
    Scratch sc("groupnorm_f32");
    const size_t n = (size_t)B * C * H * W;
    const std::vector<float> xh = host_nhwc(x, B, C, H * W);
    float* dx = sc.dev<float>(n, xh.data());
    char* scratch = sc.out<char>(groupnorm_f32_scratch_bytes(B, groups), "statistics scratch");
    float* dg = sc.dev<float>(C, gamma);
    float* db = sc.dev<float>(C, beta);
    float* dout = sc.out<float>(n, "out");
    launch_groupnorm_f32(dx, scratch, dg, db, dout, B, H * W, C, groups, eps, silu ? 1 : 0, sc.stream);
    SD_HIP(hipStreamSynchronize(sc.stream));
    host_nchw(download(dout, n), out, B, C, H * W);
  });
}

// softmax(scale * x) over each row of x (rows, cols), in place: fp32 = 0 norm.hip row_softmax_kernel on f16 (cols % 8 == 0, <= 8192,
// else SD_ERR_UNSUPPORTED), fp32 = 1 vae_f32.hip row_softmax_f32_kernel on f32 (any cols)
int sd_op_row_softmax(void* x, int rows, int cols, float scale, int fp32) {
  return guarded([&] {
    SD_REQUIRE(x, kInvalidArgument, "NULL argument");
    SD_REQUIRE(rows > 0 && cols > 0 && (fp32 == 0 || fp32 == 1), kInvalidArgument, "row_softmax: rows=%d cols=%d fp32=%d", rows, cols, fp32);
    SD_REQUIRE(fp32 || (cols % 8 == 0 && cols <= 8192), kUnsupported, "row_softmax: cols=%d (need cols %% 8 == 0, <= 8192)", cols);
    Scratch sc("row_softmax");
    const size_t n = (size_t)rows * cols;
    if (fp32) {
      float* d = sc.dev<float>(n, reinterpret_cast<const float*>(x), "x (in place)");
      launch_row_softmax_f32(d, rows, cols, scale, sc.stream);
      SD_HIP(hipStreamSynchronize(sc.stream));
      SD_HIP(hipMemcpy(x, d, n * sizeof(float), hipMemcpyDeviceToHost));
    } else {
      half_t* d = sc.dev<half_t>(n, f16(x), "x (in place)");
      launch_row_softmax(d, rows, cols, scale, sc.stream);
      SD_HIP(hipStreamSynchronize(sc.stream));
      SD_HIP(hipMemcpy(x, d, n * sizeof(half_t), hipMemcpyDeviceToHost));
    }
  });
}

// misc.hip gemv_kernel through launch_gemv: out[b][n] (+)= act_out(sum_k w[n][k] act_in(x[b][k]) + bias[n]); w (N,K) f16, bias (N) or
// NULL, x (B,K) f32, out (B,N) f32 - read first when `accumulate`.  The rows sit on the device as the UNet keeps them: x with a row
// stride of K + 8 floats behind a 4-float offset (16-byte aligned, as the kernel's 16-byte loads need), every other float 1e30; out
// with a row stride of N + 5, the padding NaN patterns that must survive the launch.
int sd_op_gemv(const void* w, const float* bias, const float* x, float* out, int B, int N, int K, int silu_in, int silu_out, int accumulate) {
  return guarded([&] {
    SD_REQUIRE(w && x && out, kInvalidArgument, "NULL argument");
    SD_REQUIRE(B > 0 && N > 0 && K > 0, kInvalidArgument, "gemv: B=%d N=%d K=%d", B, N, K);
    SD_REQUIRE(K % 8 == 0 && K <= 3072, kUnsupported, "gemv: K=%d must be a multiple of 8 and <= 3072", K);
    Scratch sc("gemv");
    const int ldx = K + 8, ldo = N + 5, xoff = 4;
    std::vector<float> xr((size_t)B * ldx + xoff, 1.0e30f);
    for (int b = 0; b < B; ++b) std::copy(x + (size_t)b * K, x + (size_t)(b + 1) * K, xr.begin() + xoff + (size_t)b * ldx);
    const float* dx = sc.dev<float>(xr.size(), xr.data()) + xoff;
    half_t* dw = sc.dev<half_t>((size_t)N * K, f16(w));
    float* db = bias ? sc.dev<float>(N, bias) : nullptr;
    const size_t no = (size_t)B * ldo;
    float* dout = sc.out<float>(no, "out rows");
    if (accumulate) SD_HIP(hipMemcpy2D(dout, ldo * sizeof(float), out, N * sizeof(float), N * sizeof(float), B, hipMemcpyHostToDevice));
    launch_gemv(dw, db, dx, ldx, dout, ldo, B, N, K, silu_in ? 1 : 0, silu_out ? 1 : 0, accumulate ? 1 : 0, sc.stream);
    SD_HIP(hipStreamSynchronize(sc.stream));
    const std::vector<float> t = download(dout, no);
    for (int b = 0; b < B; ++b) {
      for (int c = N; c < ldo; ++c) {
        uint32_t bits;
        memcpy(&bits, &t[(size_t)b * ldo + c], 4);
        SD_REQUIRE(bits == 0xffffffffu, kInternal, "gemv wrote into the padding of output row %d", b);
      }
      std::copy(t.begin() + (size_t)b * ldo, t.begin() + (size_t)b * ldo + N, out + (size_t)b * N);
    }
  });
}

// clip.hip clip_attention_kernel: causal attention of the text encoder over the stacked projection's rows qkv (S, 3 D) f16 = [q | k | v]
// -> out (S, D) f16; S <= 80, head dim D / heads a multiple of 8 and <= 128 (else SD_ERR_UNSUPPORTED)
int sd_op_clip_attention(const void* qkv, void* out, int S, int D, int heads) {
  return guarded([&] {
    SD_REQUIRE(qkv && out, kInvalidArgument, "NULL argument");
    SD_REQUIRE(S > 0 && D > 0 && heads > 0 && D % heads == 0, kInvalidArgument, "clip_attention: S=%d D=%d heads=%d", S, D, heads);
    SD_REQUIRE(S <= 80 && D / heads <= 128 && (D / heads) % 8 == 0, kUnsupported, "clip_attention: S=%d D=%d heads=%d", S, D, heads);
    Scratch sc("clip_attention");
    const size_t n = (size_t)S * D;
    half_t* dq = sc.dev<half_t>(3 * n, f16(qkv));
    half_t* dout = sc.out<half_t>(n, "out");
    launch_clip_attention(dq, dout, S, D, heads, sc.stream);
    SD_HIP(hipStreamSynchronize(sc.stream));
    SD_HIP(hipMemcpy(out, dout, n * sizeof(half_t), hipMemcpyDeviceToHost));
  });
}

// clip.hip clip_embed_kernel: out[s] = tok[clamp(ids[s], 0, vocab - 1)] + pos[s]; ids (S) int32, tok (vocab, D) / pos (S, D) f16 ->
// out (S, D) f16; D % 8 == 0 (else SD_ERR_UNSUPPORTED)
int sd_op_clip_embed(const int32_t* ids, const void* tok, const void* pos, void* out, int S, int D, int vocab) {
  return guarded([&] {
    SD_REQUIRE(ids && tok && pos && out, kInvalidArgument, "NULL argument");
    SD_REQUIRE(S > 0 && D > 0 && vocab > 0, kInvalidArgument, "clip_embed: S=%d D=%d vocab=%d", S, D, vocab);
    SD_REQUIRE(D % 8 == 0, kUnsupported, "clip_embed: hidden size %d", D);
    Scratch sc("clip_embed");
    const size_t n = (size_t)S * D;
    int* di = sc.dev<int>(S, ids);
    half_t* dt = sc.dev<half_t>((size_t)vocab * D, f16(tok));
    half_t* dp = sc.dev<half_t>(n, f16(pos));
    half_t* dout = sc.out<half_t>(n, "out");
    launch_clip_embed(di, dt, dp, dout, S, D, vocab, sc.stream);
    SD_HIP(hipStreamSynchronize(sc.stream));
    SD_HIP(hipMemcpy(out, dout, n * sizeof(half_t), hipMemcpyDeviceToHost));
  });
}

// clip.hip clip_act_kernel, in place over n f16 values: act 0 quick_gelu, 1 exact-erf gelu; n % 8 == 0
int sd_op_clip_act(void* x, size_t n, int act) {
  return guarded([&] {
    SD_REQUIRE(x, kInvalidArgument, "NULL argument");
    SD_REQUIRE(n > 0 && n % 8 == 0 && (act == 0 || act == 1), kInvalidArgument, "clip_act: n=%zu act=%d", n, act);
    Scratch sc("clip_act");
    half_t* d = sc.dev<half_t>(n, f16(x), "x (in place)");
    launch_clip_act(d, n, act, sc.stream);
    SD_HIP(hipStreamSynchronize(sc.stream));
    SD_HIP(hipMemcpy(x, d, n * sizeof(half_t), hipMemcpyDeviceToHost));
  });
}

// The copy kernels at the model boundaries, src -> dst of B * C * H * W elements each, behind one kind code:
//   0 / 1  misc.hip nchw_to_nhwc_kernel       (B,C,H,W) f16 / f32 -> [B][H][W][C] f16
//   2 / 3  vae_f32.hip nchw_to_nhwc_f32_kernel (B,C,H,W) f16 / f32 -> [B][H][W][C] f32
//   4      misc.hip nhwc_to_nchw_f32_kernel    [B][H][W][C] f16 -> (B,C,H,W) f32
//   5      vae_f32.hip nhwc_to_nchw_f32f32     [B][H][W][C] f32 -> (B,C,H,W) f32
//   6      misc.hip bc1s_to_tokens_kernel      (B,C,1,S) f16 -> [B][S][C] f16   (H = 1, W = S)
//   7 / 8  misc.hip half_to_float / float_to_half over the flat buffer
int sd_op_layout(int kind, const void* src, void* dst, int B, int C, int H, int W) {
  return guarded([&] {
    SD_REQUIRE(src && dst, kInvalidArgument, "NULL argument");
    SD_REQUIRE(kind >= 0 && kind <= 8, kInvalidArgument, "layout: kind %d", kind);
    SD_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && (kind != 6 || H == 1), kInvalidArgument, "layout: kind %d B=%d C=%d H=%d W=%d", kind, B, C, H, W);
    Scratch sc("layout");
    const size_t n = (size_t)B * C * H * W;
    const bool src_f32 = kind == 1 || kind == 3 || kind == 5 || kind == 8;
    const bool dst_f32 = kind == 2 || kind == 3 || kind == 4 || kind == 5 || kind == 7;
    const void* ds = src_f32 ? (const void*)sc.dev<float>(n, reinterpret_cast<const float*>(src)) : (const void*)sc.dev<half_t>(n, f16(src));
    float* df = dst_f32 ? sc.out<float>(n, "dst") : nullptr;
    half_t* dh = dst_f32 ? nullptr : sc.out<half_t>(n, "dst");
    switch (kind) {
      case 0: case 1: launch_nchw_to_nhwc(ds, src_f32, dh, B, C, H, W, sc.stream); break;
      case 2: case 3: launch_nchw_to_nhwc_f32(ds, src_f32, df, B, C, H, W, sc.stream); break;
      case 4: launch_nhwc_to_nchw_f32(f16(ds), df, B, C, H, W, sc.stream); break;
      case 5: launch_nhwc_to_nchw_f32f32(reinterpret_cast<const float*>(ds), df, B, C, H, W, sc.stream); break;
      case 6: launch_bc1s_to_tokens(f16(ds), dh, B, C, W, sc.stream); break;
      case 7: launch_half_to_float(f16(ds), df, n, sc.stream); break;
      default: launch_float_to_half(reinterpret_cast<const float*>(ds), dh, n, sc.stream); break;
    }
    SD_HIP(hipStreamSynchronize(sc.stream));
    if (dst_f32)
      SD_HIP(hipMemcpy(dst, df, n * sizeof(float), hipMemcpyDeviceToHost));
    else
      SD_HIP(hipMemcpy(dst, dh, n * sizeof(half_t), hipMemcpyDeviceToHost));
  });
}

// misc.hip sum_half_kernel: out = srcs[0] + ... + srcs[nsrc - 1] over n f16 values (1 <= nsrc <= 4, fp32 accumulation in source order,
// one rounding); add = 1 (nsrc must be 2): add_half_kernel instead.  n % 8 == 0.
int sd_op_sum_half(const void* const* srcs, int nsrc, void* out, size_t n, int add) {
  return guarded([&] {
    SD_REQUIRE(srcs && out, kInvalidArgument, "NULL argument");
    SD_REQUIRE(n > 0 && n % 8 == 0 && nsrc >= 1 && nsrc <= 4 && (add == 0 || (add == 1 && nsrc == 2)), kInvalidArgument,
               "sum_half: n=%zu (a multiple of 8), %d sources (1-4; add_half: 2), add=%d", n, nsrc, add);
    for (int i = 0; i < nsrc; ++i) SD_REQUIRE(srcs[i], kInvalidArgument, "NULL argument");
    Scratch sc("sum_half");
    const half_t* ds[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int i = 0; i < nsrc; ++i) ds[i] = sc.dev<half_t>(n, f16(srcs[i]));
    half_t* dout = sc.out<half_t>(n, "out");
    if (add)
      launch_add_half(ds[0], ds[1], dout, n, sc.stream);
    else
      launch_sum_half(ds, nsrc, dout, n, sc.stream);
    SD_HIP(hipStreamSynchronize(sc.stream));
    SD_HIP(hipMemcpy(out, dout, n * sizeof(half_t), hipMemcpyDeviceToHost));
  });
}

// vit.hip vit_patch_rows_kernel: img (B,3,I,I) f16 -> rows (B (I/p)^2, Kp) f16, columns [3 p p, Kp) zero
int sd_op_vit_patch_rows(const void* img, void* rows, int B, int I, int p, int Kp) {
  return guarded([&] {
    SD_REQUIRE(img && rows, kInvalidArgument, "NULL argument");
    SD_REQUIRE(B > 0 && p >= 1 && I >= p && I % p == 0 && Kp >= 3 * p * p, kInvalidArgument, "vit_patch_rows: B=%d image %d patch %d row %d", B, I, p, Kp);
    Scratch sc("vit_patch_rows");
    const size_t n = (size_t)B * (I / p) * (I / p) * Kp;
    half_t* di = sc.dev<half_t>((size_t)B * 3 * I * I, f16(img));
    half_t* dout = sc.out<half_t>(n, "rows");
    launch_vit_patch_rows(di, dout, B, I, p, Kp, sc.stream);
    SD_HIP(hipStreamSynchronize(sc.stream));
    SD_HIP(hipMemcpy(rows, dout, n * sizeof(half_t), hipMemcpyDeviceToHost));
  });
}

// vit.hip vit_tokens_kernel: patch (B, S - 1, D), cls (D), pos (S, D) f16 -> out (B, S, D) f16; D % 8 == 0, S >= 2 (else SD_ERR_UNSUPPORTED)
int sd_op_vit_tokens(const void* patch, const void* cls, const void* pos, void* out, int B, int S, int D) {
  return guarded([&] {
    SD_REQUIRE(patch && cls && pos && out, kInvalidArgument, "NULL argument");
    SD_REQUIRE(B > 0 && S > 0 && D > 0, kInvalidArgument, "vit_tokens: B=%d S=%d D=%d", B, S, D);
    SD_REQUIRE(D % 8 == 0 && S >= 2, kUnsupported, "vit_tokens: hidden size %d, %d tokens", D, S);
    Scratch sc("vit_tokens");
    const size_t n = (size_t)B * S * D;
    half_t* dp = sc.dev<half_t>((size_t)B * (S - 1) * D, f16(patch));
    half_t* dc = sc.dev<half_t>(D, f16(cls));
    half_t* de = sc.dev<half_t>((size_t)S * D, f16(pos));
    half_t* dout = sc.out<half_t>(n, "out");
    launch_vit_tokens(dp, dc, de, dout, B, S, D, sc.stream);
    SD_HIP(hipStreamSynchronize(sc.stream));
    SD_HIP(hipMemcpy(out, dout, n * sizeof(half_t), hipMemcpyDeviceToHost));
  });
}

// The proof that the scratch's guards and poison can fail: dst = (float)src over n f16 values (misc.hip half_to_float_kernel, one
// element per thread), with one deliberate off-by-one made HERE, by the pointers and counts the launches get.  Every access stays
// inside the two allocations of the scratch (data or guard), so no mode can fault.
//   0 the clean launch                                         -> SD_OK
//   1 + one element written behind dst                         -> SD_ERR_INTERNAL, "back guard"
//   2 + one element written in front of dst                    -> SD_ERR_INTERNAL, "front guard"
//   3 + one element written behind src (an input)              -> SD_ERR_INTERNAL, "back guard"
//   4 the last element of dst skipped                          -> SD_OK, dst[n - 1] is NaN
//   5 src read from its second element on, one behind its end  -> SD_OK, dst[n - 1] is NaN
// dst is copied out in every mode, so a caller sees what a failed call left.
int sd_op_harness_selftest(int mode, const void* src, float* dst, size_t n) {
  return guarded([&] {
    SD_REQUIRE(src && dst, kInvalidArgument, "NULL argument");
    SD_REQUIRE(mode >= 0 && mode <= 5 && n >= 2 && n <= ((size_t)1 << 24), kInvalidArgument, "harness_selftest: mode %d n %zu", mode, n);
    Scratch sc("harness_selftest");
    half_t* ds = sc.dev<half_t>(n, f16(src), "src");
    float* dd = sc.out<float>(n, "dst");
    launch_half_to_float(mode == 5 ? ds + 1 : ds, dd, mode == 4 ? n - 1 : n, sc.stream);
    if (mode == 1) launch_half_to_float(ds, dd + n, 1, sc.stream);
    if (mode == 2) launch_half_to_float(ds, dd - 1, 1, sc.stream);
    if (mode == 3) launch_float_to_half(dd, ds + n, 1, sc.stream);
    SD_HIP(hipStreamSynchronize(sc.stream));
    SD_HIP(hipMemcpy(dst, dd, n * sizeof(float), hipMemcpyDeviceToHost));
  });
}

}  // extern "C"
