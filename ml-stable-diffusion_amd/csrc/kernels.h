// Launch interfaces of the hand-written gfx950 kernels.  All activations are channels-last
// fp16: an image tensor is [B][H][W][C] == a token matrix [M = B*H*W][C]; the reference's BC1S
// sequence layout (layer_norm.py:25) is the same bytes read as [B][S][C].
#pragma once
#include "sd_common.h"

namespace sd {

// ---------------------------------------------------------------------------------------------
// K4/K5: implicit-GEMM convolution / 1x1 GEMM on MFMA (igemm.hip, conv3x3_halo.hip, conv_small.hip; the plan: conv_plan.h)
//   out[m][n] = epilogue( sum_k X[m][k] * W[n][k] ),  k = tap*(C0+C1) + c
// ---------------------------------------------------------------------------------------------
enum OutMode : int {
  kOutHalf = 0,        // half out[M][N]
  kOutHalfT = 1,       // half out[B][N][ldT]   (token-transposed: V^T for attention)
  kOutGeglu = 2,       // half out[M][N/2] = (v+bv) * gelu_erf(g+bg); W rows interleaved 32/32
};

// GroupNorm (+ SiLU) of a conv's OUTPUT written by the conv's own slab-combine pass (wstream.hip reduce_twin_kernel): the
// consumer is torch.nn.GroupNorm over this tensor (unet.py:430-451, :528-531) or over a channel concat in which this tensor
// occupies the group-aligned column range [c_off, c_off + N) (torch.cat of unet.py:213-216 followed by norm1).
struct GnTwin {
  half_t* y = nullptr;           // [M][ld]: the normalised copy goes to columns [c_off, c_off + N)
  int ld = 0, c_off = 0;
  int cpg = 0;                   // channels per group of the consuming GroupNorm
  const float* gamma = nullptr;  // the consumer's affine, indexed by ITS channel (c_off + n)
  const float* beta = nullptr;
  float eps = 1e-5f;
  int silu = 0;
};

// What a conv reads its weights from.  Fp16: ConvDesc::w and its pre-tiled copies.  Every other kind is ONE packed stream on the device
// (the weight_prep.h rule of the kind) that a kernel decodes in front of the MFMAs of its fp16 twin; a descriptor that carries one holds
// no fp16 weights (w == w_tiled == nullptr) and is pinned to the kind's plan tile, so no table row or tuner candidate can move it:
//   PalWstream  tile 14, wstream.hip  wstream_kernel NBITS > 0   stream of wstream_pal_pack   staging: tile 9's code
//   PalGemm     tile 15, smgemm.hip   smgemm_pal_kernel          stream of smgemm_pal_pack    staging: tile 12's code (0 = by M)
//   PalGeglu    tile 16, smgeglu.hip  smgeglu_pal_kernel         stream of smgeglu_pal_pack   staging: tile 13's code
//   PalHalo     tile 25, conv3x3_halo_pal.hip  conv3x3_halo_pal_kernel  stream of halo_pal_pack      staging: tile 7's code
//   I8Wstream   tile 17, wstream.hip  wstream_kernel NBITS = kWsI8 (W8A8)   stream of wstream_i8_pack   staging: tile 9's code
//   I8Halo      tile 18, conv3x3_halo_i8.hip  conv3x3_halo_i8_kernel (W8A8)   stream of halo_i8_pack      staging: tile 7's code
//   I8Gemm      tile 19, smgemm_i8.hip        smgemm_i8_kernel (W8A8)         stream of smgemm_i8_pack    staging: tile 12's code (0 = by M)
//   I8Geglu     tile 20, smgeglu_i8.hip       smgeglu_i8_kernel (W8A8)        stream of smgeglu_i8_pack   staging: tile 13's code (0 = by the grid);
//               the activations arrive quantized (ConvDesc::x0_i8, written by launch_layernorm_q8)
//   I8Qkv       tile 22, smqkv_i8.hip         smqkv_i8_kernel (W8A8)          stream of smqkv_i8_pack     staging: 1 / 2 = 128- / 256-row tiles (0 = by the
//               grid); the stacked [Wq | Wk | Wv] of a fused q|k|v launch, activations quantized by their producer as for I8Geglu
//   I8GemmQ     tile 24, smgemm_q8.hip        smgemm_q8_kernel (W8A8)         stream of smgemm_i8_pack    staging: tile 12's code (0 = by M);
//               tile 19's GEMM with the activations quantized by their producer (ConvDesc::x0_i8: tile 20 with an int8 output, or a
//               plain-form launch_layernorm_q8)
//   (tiles 19, 20, 22, 24: LDS image, ladder, epilogue arithmetic and launch, and the ring geometry, issue and wait of tiles 20 and 22,
//   are sm_i8_ring.h's)
enum class WeightSource { Fp16, PalWstream, PalGemm, PalGeglu, PalHalo, I8Wstream, I8Halo, I8Gemm, I8Geglu, I8Qkv, I8GemmQ };
struct CompressedWeights {
  WeightSource kind = WeightSource::Fp16;
  const void* stream = nullptr;
  // palettes: the tensor's LUT padded to kPalLutHalves fp16 entries and the index width (1, 2, 4, 6, 8)
  const half_t* lut = nullptr;
  int bits = 0;
  // PalGeglu with the LayerNorm fold (ConvDesc::ln_colsum set): the fp32 norm weight [C0] - the kernel multiplies every LUT value by it
  // as fold_layernorm_rows does on the host; null without the fold
  const float* ln_gamma = nullptr;
  // I8Wstream / I8Halo / I8Gemm / I8Geglu / I8Qkv / I8GemmQ: the output scale per column scale[n] = fp32(s_a * s_w[n]) (I8Geglu: rows in the
  // interleaved order of the GEGLU upload, geglu_row) and inv_s = fp32(1 / s_a), the factor the kernel - for I8Geglu / I8Qkv / I8GemmQ
  // the producer in front of it - quantizes its activations by
  const float* scale = nullptr;
  float inv_s = 0.f;
  bool palettized() const { return kind == WeightSource::PalWstream || kind == WeightSource::PalGemm || kind == WeightSource::PalGeglu || kind == WeightSource::PalHalo; }
  const uint8_t* pal() const { return palettized() ? static_cast<const uint8_t*>(stream) : nullptr; }
  bool int8() const { return kind == WeightSource::I8Wstream || kind == WeightSource::I8Halo || kind == WeightSource::I8Gemm || kind == WeightSource::I8Geglu || kind == WeightSource::I8Qkv || kind == WeightSource::I8GemmQ; }
  const int8_t* i8() const { return int8() ? static_cast<const int8_t*>(stream) : nullptr; }
};

struct ConvDesc {
  const half_t* x0 = nullptr;   // [B][Hi][Wi][C0]
  const half_t* x1 = nullptr;   // optional second source (channel concat), [B][Hi][Wi][C1]
  const int8_t* x0_i8 = nullptr;   // cw of kind I8Geglu / I8Qkv / I8GemmQ: the source as int8 [M][C0], quantized by its producer (launch_layernorm_q8, tile 20's int8 output); x0 is not read
  int C0 = 0, C1 = 0;
  const half_t* w = nullptr;    // [N][K] K-major, K = ksize*ksize*(C0+C1), tap-major
  const float* bias = nullptr;  // [N] or null
  const float* temb = nullptr;  // [B][temb_stride] broadcast over pixels, or null
  int temb_stride = 0;
  const half_t* res = nullptr;  // [M][N] residual, or null
  half_t* out = nullptr;
  // cw of kind I8Geglu only: the product leaves as int8 [M][N / 2] = ws_quantize8(the fp16 values `out` would hold, out_inv_s) - the
  // activations of a plan-tile-24 GEMM behind it; `out` is then not written
  int8_t* out_q8 = nullptr;
  float out_inv_s = 0.f;
  int B = 1, Hi = 1, Wi = 1;    // source spatial size (before nearest x2 upsampling)
  int Ho = 1, Wo = 1;           // output spatial size
  int ksize = 1, stride = 1, up = 1;
  int pad = -1;                 // -1: ksize / 2 on every side; 0 with stride 2 = the VAE encoder's (0,1,0,1) padding
  int N = 0;
  int out_mode = kOutHalf;
  int ldT = 0;                  // kOutHalfT: padded token stride
  // tuning overrides (0 = heuristic)
  int tile = 0;                 // plan tile pinned by the caller (ConvPlan::tile, conv_plan.h)
  int splitk = 0;
  long long* prof = nullptr;    // debug bit 2: device buffer of 8 timestamps
  int debug = 0;                // ablation hooks for tools/microbench (results are garbage when != 0)
  int staging = 0;              // the code that goes with the tile: its meaning per kernel family is decode_plan's (conv_plan.cpp)
  // LayerNorm folded into this 1x1 GEMM (x is the UN-normalised input): w = W*gamma, bias = b + W.beta,
  // ln_colsum[n] = sum_k w[n][k]; the kernel derives mean / rstd of each row from its own A tiles
  const float* ln_colsum = nullptr;
  float ln_eps = 1e-5f;
  // fused q|k|v: output columns [n_trans, N) are written token-transposed to out_t [B][N-n_trans][ldT]
  // (attention's V^T), columns [0, n_trans) to out with row length n_trans.  Needs Ho*Wo % 8 == 0.
  half_t* out_t = nullptr;
  int n_trans = 0;
  int vt_perm = 0;              // out_t in the key order of AttnDesc::vt_perm (needs Ho*Wo % 16 == 0)
  // fused q|k|v for attention8: output columns [0, q_cols) - the queries - leave multiplied by q_scale (d^-0.5 * log2 e), applied
  // to the fp32 accumulator BEFORE the one rounding to fp16 (AttnDesc::q_prescaled).  0 columns = off.
  float q_scale = 1.f;
  int q_cols = 0;
  // GroupNorm statistics of the output from the conv's own epilogue (the consumer is a GroupNorm over exactly this
  // tensor, gn_groups groups): partial sums go to gn_partial [B][gn_groups][kGnMaxSlabs][2].  launch_conv returns how
  // many entries per (sample, group) it wrote - 0 when the chosen plan cannot (split-K, ragged tiles): the GroupNorm
  // then runs its own statistics pass.
  float* gn_partial = nullptr;
  int gn_groups = 0;
  // GroupNorm folded into this 1x1 GEMM (SpatialTransformer.norm -> proj_in, unet.py:528-531, :553-556): x0 is the UN-normalised
  // tensor, gnf_partial holds gnf_entries (sum, sumsq) partials per (sample, group) written by x0's producer
  // ([B][gnf_groups][kGnMaxSlabs][2]); the kernel turns them into per-channel scale / shift and applies them to its A fragments
  // (v_pk_fma_f16 between the LDS read and the MFMA).  Needs a single source, Ho * Wo a multiple of the M tile, C0 <= 2048.
  const float* gnf_partial = nullptr;
  const float* gnf_gamma = nullptr;
  const float* gnf_beta = nullptr;
  float gnf_eps = 1e-6f;
  int gnf_groups = 0, gnf_entries = 0;
  // The same fields on a 3x3 / stride-1 conv (round 5): GroupNorm + SiLU (gnf_silu must be 1) of the input applied in the halo LOADER of
  // conv3x3_halo_ks_kernel (ResnetBlock2D norm1 -> conv1, norm2 -> conv2: unet.py:472-481) - every wave normalises the halo pieces
  // it fetched, in LDS, once per workgroup; pixels outside the image stay zero (the conv pads the normalised tensor).  Shapes:
  // conv_gn_loader_ok; the concatenated channel count indexes gamma / beta / the partials.
  int gnf_silu = 0;
  // weights in the fragment-major layout of wstream.hip (launch_wstream_retile), or null: plan tile 9 needs them
  const half_t* w_tiled = nullptr;
  // what the conv reads its weights from when not from the fp16 matrices (CompressedWeights above); kind Fp16 = w and its copies
  CompressedWeights cw;
  // weights in the fragment-major layout of wsgemm.hip (launch_wsgemm_retile), or null: the weight-stationary GEGLU kernel
  // (plan tile 10) needs them; launch_conv takes that kernel whenever they are there and no other plan was forced
  const half_t* w_ws = nullptr;
  // weights in the fragment-major layout of bvgemm.hip (launch_bvgemm_retile; plain or GEGLU row order by out_mode), or null:
  // plan tile 11 (weights global -> VGPR, large-M 1x1 GEMMs) needs them
  const half_t* w_bv = nullptr;
  // n_twins > 0: the output leaves through fp32 slabs and reduce_twin_kernel, which also writes the GroupNorm twins
  // (needs Ho * Wo <= 256 and reduce_twin_ok; launch_conv forces the slab path whatever the plan's split-K)
  GnTwin twin[2];
  int n_twins = 0;
  // The upsampler conv (ksize 3, stride 1, up 2, kOutHalf, one source, fp16 weights) as four 2x2 phase convs on the low-res image (plan
  // tile 21, conv3x3_halo_sp.hip): w is then the folded matrix of weight_prep.h subpixel_fold, [4][N][4][C0], NOT the 3x3 matrix.
  // Shapes: halo_sp_ok (conv_plan.h).  Without the flag nothing about a descriptor's plan changes.
  bool subpix = false;
};

constexpr int kGnMaxSlabs = 256;   // entries per (sample, group) of a GroupNorm partial buffer

struct ConvWorkspace {
  float* partial = nullptr;     // split-K slabs
  size_t partial_bytes = 0;
};

// Workspace bytes a handle reserves for this conv at build time: an upper bound of what any plan it can later get needs (conv_plan.cpp).
size_t conv_workspace_bytes(const ConvDesc& d);
// 256 B of device zeros, the source of padding rows of the conv kernels: allocated by the first call.  Every handle constructor
// (and the operator entry points' Scratch) calls it, so it is never first called under graph capture; launches only read it.
const half_t* device_zero_chunk();
// returns the number of GroupNorm partial entries per (sample, group) written to d.gn_partial (0: none)
int launch_conv(const ConvDesc& d, const ConvWorkspace& ws, hipStream_t s);
struct ConvPlan;   // conv_plan.h: what launch_conv resolved; the launchers of the kernel files below read their fields of it
bool conv_fast_path_ok(const ConvDesc& d);
bool conv_gn_loader_ok(const ConvDesc& d);   // gnf_* on a 3x3 conv (gnf_groups set): the halo kernel can normalise this input in its loader
// tuning hook: plan (tile, staging, splitk in the codes of ConvPlan) forced on every conv that admits it; tile 0 = off
void conv_tune_set_candidate(int tile, int staging, int splitk);
bool conv_plan_is_tuned(const ConvDesc& d);   // tuned_convs.inc has a row for this shape
int conv_plan_table_set(const char* text);   // rows of tuned_convs.inc format; returns the number of plans read

// wstream.hip: the small-M weight-streaming kernel (plan tile 9) and the group-organised slab combine
bool wstream_shape_ok(const ConvDesc& d);                 // shape admits plan tile 9 (d.w_tiled not looked at)
int wstream_splits(const ConvDesc& d, int nw);            // slabs launch_wstream writes with nw waves per workgroup
size_t wstream_tiled_halves(int N, int Ctot, int ksize);
void launch_wstream_retile(const half_t* w, half_t* wt, int N, int Ctot, int ksize, hipStream_t s);
int launch_wstream(const ConvDesc& d, float* partial, int nw, hipStream_t s);   // nw: ConvPlan::waves
// the same launch from palettized weights (d.cw of kind PalWstream): every weight is looked up in the LUT in front of the same
// MFMAs in the same order, so the slabs are bit-identical to launch_wstream's on the de-palettized weights
int launch_wstream_pal(const ConvDesc& d, float* partial, int nw, hipStream_t s);
// the same launch from int8 weights and activations quantized in the loader (d.cw of kind I8Wstream, plan tile 17): exact int32
// sums over a workgroup's slices, scaled per column into the same fp32 slabs
int launch_wstream_i8(const ConvDesc& d, float* partial, int nw, hipStream_t s);
bool reduce_twin_ok(int HW, int N, int n_twins, const GnTwin* tw);
void launch_reduce_twin(const float* partial, int S, int M, int N, int HW, const float* bias, const float* temb, int temb_stride,
                        const half_t* res, half_t* out, int n_twins, const GnTwin* tw, hipStream_t s);

// wsgemm.hip (round 6): weight-stationary GEGLU projection of the 320-channel level (plan tile 10)
bool wsgemm_shape_ok(const ConvDesc& d);
bool wsgemm_wanted(const ConvDesc& d);                               // the library's rule for taking plan tile 10 on its own
size_t wsgemm_tiled_halves(int N);
void launch_wsgemm_retile(const half_t* w, half_t* wt, int N, bool geglu, hipStream_t s);
void launch_wsgemm(const ConvDesc& d, hipStream_t s);

// bvgemm.hip (round 6): 1x1 GEMM with the weights global -> VGPR, activations alone in LDS (plan tile 11)
bool bvgemm_shape_ok(const ConvDesc& d);
size_t bvgemm_tiled_halves(int N, int K);
void launch_bvgemm_retile(const half_t* w, half_t* wt, int N, int K, bool geglu, hipStream_t s);
void launch_bvgemm(const ConvDesc& d, const ConvPlan& p, hipStream_t s);   // p.variant 1-6 (bvgemm.hip)
int bvgemm_auto_variant(const ConvDesc& d);                           // the library's choice of a variant (the planner resolves it)
bool bvgemm_wanted(const ConvDesc& d);                                // the library's rule for taking plan tile 11 on its own

// smgemm.hip: small-M 1x1 GEMM (one source, or two concatenated along K), whole-LDS ring, epilogue from the accumulators (plan tile 12)
bool smgemm_shape_ok(const ConvDesc& d, int variant);                 // variant 1 / 2: 32- / 64-row tiles, 0: by M
bool smgemm_wanted(const ConvDesc& d);                                // the library's rule for taking plan tile 12 on its own
void launch_smgemm(const ConvDesc& d, const ConvPlan& p, hipStream_t s);   // p.bm: 32- or 64-row tiles
int smgemm_bm(const ConvDesc& d, int variant);                        // the tile height of a variant: 32 or 64 (the planner resolves it)
// the same GEMM from palettized weights (plan tile 15: d.cw of kind PalGemm):
// the weights are decoded from the LUT into the fragments of the same MFMAs in the same order, the epilogue is launch_smgemm's, so
// the output is bit-identical to launch_smgemm's on the fp16 weights lut[indices].  One source only.
void launch_smgemm_pal(const ConvDesc& d, const ConvPlan& p, hipStream_t s);
// smgemm_i8.hip: the single-source GEMM on the same tiles from int8 weights and activations (W8A8, plan tile 19: d.cw of kind I8Gemm) -
// the semantics of the int8 weight stream (plan tile 17), not tile 12's rounding; K <= kSmI8MaxK
bool smgemm_i8_shape_ok(const ConvDesc& d, int variant);              // smgemm_shape_ok, one source, inside the int32 bound
void launch_smgemm_i8(const ConvDesc& d, const ConvPlan& p, hipStream_t s);
// smgemm_q8.hip: tile 19's GEMM - tiles, eligibility, epilogue, the same function of the quantized activations - from int8 activations
// written by the producer (W8A8, plan tile 24: d.cw of kind I8GemmQ, d.x0_i8); no quantizer in the K loop
bool smgemm_q8_shape_ok(const ConvDesc& d, int variant);              // smgemm_i8_shape_ok
void launch_smgemm_q8(const ConvDesc& d, const ConvPlan& p, hipStream_t s);

// wfold.hip: two back-to-back linear maps folded into one - merged [N][K + J] = [fp16(Wp W2) | Wp], bm = bp + Wp b2 (Wp [N][J],
// W2 [J][K]; fp32 accumulation in a fixed order, once per handle: UNet::transformer_block's merged tail)
void launch_wfold(const half_t* wp, const float* bp, const half_t* w2, const float* b2, half_t* merged, float* bm, int N, int J, int K,
                  hipStream_t s);

// smgeglu.hip: GEGLU projection (with or without the LayerNorm fold) on BM x 80 tiles, one workgroup per CU, whole-LDS ring, weights
// as uploaded (plan tile 13)
bool smgeglu_shape_ok(const ConvDesc& d, int variant);                // variant 1 / 2: 128- / 256-row tiles, 0: by the grid size
bool smgeglu_wanted(const ConvDesc& d);                               // the library's rule for taking plan tile 13 on its own
int smgeglu_bm(const ConvDesc& d, int variant);                       // the tile height of a variant: 128 or 256 (the planner resolves it)
void launch_smgeglu(const ConvDesc& d, const ConvPlan& p, hipStream_t s);   // p.bm; d.prof set: the phase-clock build, which fills
size_t smgeglu_prof_entries(const ConvDesc& d, int variant);          // this many long long: [workgroup][10 waves][8], six stamps used
// the same launch from palettized weights (plan tile 16: d.cw of kind PalGeglu, ln_gamma with the fold): LUT value times norm weight
// decoded into the weight rows of the same stages in front of the same MFMAs, so the output is bit-identical to launch_smgeglu's on the folded fp16 weights.  128-row tiles only, C0 <= 2560, no phase clocks.
bool smgeglu_pal_shape_ok(const ConvDesc& d, int variant);            // variant 0 / 1 resolving to 128-row tiles
void launch_smgeglu_pal(const ConvDesc& d, const ConvPlan& p, hipStream_t s);
// smgeglu_i8.hip: the projection WITHOUT the fold on the same tiles from int8 weights and int8 activations (W8A8, plan tile 20: d.cw of
// kind I8Geglu, d.x0_i8) - exact int32 sums, scale and bias in fp32, then tile 13's v * gelu_erf(g); both tile heights, K <= kSmI8MaxK.
// With d.out_q8 set the fp16 values leave through ws_quantize8(., d.out_inv_s) as int8 [M][N / 2] instead (the producer of plan tile 24)
bool smgeglu_i8_shape_ok(const ConvDesc& d, int variant);             // smgeglu_shape_ok, no fold, inside the int32 bound
void launch_smgeglu_i8(const ConvDesc& d, const ConvPlan& p, hipStream_t s);
// smqkv_i8.hip: the fused q|k|v projection of a self-attention from int8 weights and int8 activations (W8A8, plan tile 22: d.cw of kind
// I8Qkv, d.x0_i8) - tile 20's K loop on BM x 160-column tiles, q | k to d.out [M][2 C0] (columns below q_cols times q_scale), V^T to
// d.out_t [B][C0][ldT] (vt_perm: attention8's key order).  Shapes: smqkv_i8_shape_ok (conv_plan.h)
void launch_smqkv_i8(const ConvDesc& d, const ConvPlan& p, hipStream_t s);

// calib.hip: box calibration for bench.py - out[0..6] = copy GB/s, dense MFMA TFLOP/s, us per launch of a 323-launch empty
// graph, us per launch of a 323-launch chain of short kernels on cold operands, us per launch of a 323-launch chain handing 8 MB
// over between the XCDs' L2s, ns per dependent load from HBM / from the caches
void run_calibration(int device, float* out);

// conv_small.hip: direct conv for tiny / odd shapes (any Cin, any N): fp32 accumulate, one thread per output
int launch_conv_generic(const ConvDesc& d, int act_silu_out, hipStream_t s);   // returns like launch_conv

// N <= 8 outputs, K % 8 == 0: one wavefront per output pixel.  out_nchw_f32: write float
// [B][N][Ho][Wo] (the UNet's noise_pred boundary), else half NHWC.
void launch_conv_small_n(const ConvDesc& d, float* out_nchw_f32, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// K1-K3: attention (attention.hip).  q [B][Sq][ldq] (head h at column h*d), k [B][Sk][ldk],
// vt [B][heads*d][ldv] (token-transposed), out [B][Sq][ldo].
// ---------------------------------------------------------------------------------------------
enum AttnImpl : int { kAttnOriginal = 0, kAttnSplitEinsum = 1, kAttnSplitEinsumV2 = 2 };

struct AttnDesc {
  const half_t* q = nullptr;
  const half_t* k = nullptr;
  const half_t* vt = nullptr;
  half_t* out = nullptr;
  int B = 1, heads = 1, d = 64, Sq = 0, Sk = 0;
  int ldq = 0, ldk = 0, ldv = 0, ldo = 0;
  int impl = kAttnOriginal;
  int variant = 0;   // A/B testing: 1 = never use the attention8.hip kernel
  // 1: every 16-key group of a vt row is stored [k0-3 | k8-11 | k4-7 | k12-15] - the order in which a lane of the key-major
  // P.V MFMA consumes keys, so its V^T fragment is ONE 16-byte LDS read (attention8.hip; written so by the fused q|k|v GEMM,
  // ConvDesc::vt_perm).  Only attention8 reads this layout; the general kernels need 0.
  int vt_perm = 0;
  // 1: q already carries d^-0.5 * log2(e) (multiplied into the fp32 accumulator of the producing GEMM, ConvDesc::q_scale): attention8
  // does not re-scale (and re-round) it.  Only with vt_perm.
  int q_prescaled = 0;
  // scratch for attention8's balanced form (attention8_sk_scratch says how much this problem wants): partial (m, l, O) results and
  // one arrival counter per query tile, ZEROED once by the owner (the kernel leaves them at zero).  Without it: the classic grid.
  float* sk_part = nullptr;
  size_t sk_part_bytes = 0;
  unsigned* sk_cnt = nullptr;
  int sk_cnt_n = 0;
  int sk_force = 0;   // 1: the balanced form wherever it can run (operator tests; the library's rule otherwise)
  int sk_upw = 0;     // > 0: (query tile, key tile) units per workgroup of the balanced form (operator tests)
};
// the factor a producer of pre-scaled queries multiplies in (head dim d)
inline float attention_q_prescale(int d) { return 1.4426950408889634f / sqrtf((float)d); }
void launch_attention(const AttnDesc& d, hipStream_t s);
bool attention_supported(int d);
// attention8.hip: head dim 64, S_k a multiple of 64 (the UNet's self-attention): LDS-DMA ring, two waves per SIMD, software-
// pipelined across key tiles.  launch_attention dispatches to it; AttnDesc::variant == 1 (or SD_ATTN8=0) keeps the general kernels.
bool attention8_ok(const AttnDesc& d);
// build-time decision (UNet builder, sd_op_attention): will attention8 run this shape?  Then V^T must be produced permuted.
bool attention8_shape_ok(int d, int Sq, int Sk);
void launch_attention8(const AttnDesc& d, hipStream_t s);
// true where attention8 would run the problem in its balanced form (query tiles dealt out evenly over the CUs, partial results
// merged by the last workgroup to arrive), with the scratch that takes: bytes for AttnDesc::sk_part, counters for sk_cnt
bool attention8_sk_scratch(const AttnDesc& d, size_t* part_bytes, int* n_counters);

// What a launcher of the three attention files decides for a problem, stated once per launcher by the host function that launcher itself
// calls (attention_kernel, attention8_kernel, attention_i8_kernel): the launch switches on these fields and on nothing else, so the
// answer sd_op_attention_kernel gives cannot drift from what runs.
enum AttnFamily : int { kAttnFamilyGeneral = 0, kAttnFamily8 = 1, kAttnFamilyI8 = 2 };
struct AttnKernel {
  int family = kAttnFamilyGeneral;
  int waves = 4;             // waves per workgroup: 4 or 8
  int q_tiles = 1;           // 32-query tiles per wave (2: the general kernel's SPLIT_EINSUM_V2 form on whole 512-query chunks, d <= 64)
  int d = 64;                // general kernel: the head dim
  int mode = 0;              // general kernel: 0 the ORIGINAL schedule, 1 the split one (SPLIT_EINSUM, and V2's chunks)
  bool balanced = false;     // attention8: the balanced form, with
  int upw = 0, max_seg = 0;  // ... units per workgroup and the most segments one workgroup can touch
};
// one line: "attn d<d> original|split w<waves> qt<q_tiles>", "attn8 w<waves> classic", "attn8 w<waves> balanced upw=<u> seg=<s>",
// "attn_i8 w<waves>"
std::string attention_kernel_name(const AttnKernel& k);
// compute units of the current device, 256 where there is none to ask
int device_cus();
// THE waves rule of attention8.hip and attention_i8.hip: 256-query (eight-wave) workgroups when they give at least half the CUs one,
// else 128-query ones - more, smaller workgroups
int attention_waves(int B, int heads, int Sq);
AttnKernel attention_kernel(const AttnDesc& d);    // launch_attention's choice, with that launcher's refusals
AttnKernel attention8_kernel(const AttnDesc& d);   // launch_attention8's

// attention_i8.hip: the same self-attention from int8 q, k and V^T on the int8 MFMAs (W8A8: the reference's Einsum modules,
// activation_quantization.py:205-215, unet.py:45-59; the function is stated at the top of attention_i8.hip).  q and k are rows of int8
// matrices (head h at byte column 64 h; ldq / ldk in bytes), vt [B][heads * 64][ldv] int8 with every 32 keys in the order
// attention_i8_vt_key, out [B][S][ldo] fp16.  The ranges are those of the un-scaled q, k and v the reference's Einsum sees.
constexpr int kAttnI8MaxS = 133120;   // 127^2 S < 2^31: the integer sums of P.V are exact up to here
struct AttnI8Desc {
  const int8_t* q = nullptr;
  const int8_t* k = nullptr;
  const int8_t* vt = nullptr;
  half_t* out = nullptr;
  int B = 1, heads = 1, S = 0;
  int ldq = 0, ldk = 0, ldv = 0, ldo = 0;
  float q_absmax = 0.f, k_absmax = 0.f, v_absmax = 0.f;
};
// the shape rule, in one place: head dim 64, S_q == S_k, whole 64-key tiles, inside the exact integer sums
bool attention_i8_shape_ok(int d, int Sq, int Sk);
// position p (0 .. 31) of every 32-key group of the int8 V^T holds this key of the group: the order in which a lane's score registers
// become the packed-byte operand of the P.V MFMA (what vt_perm == 1 is to attention8.hip)
__host__ __device__ inline int attention_i8_vt_key(int p) { return (p & 3) + 8 * ((p >> 2) & 3) + 4 * (p >> 4); }
float attention_i8_score_scale(float q_absmax, float k_absmax, int d);   // c = fp32(s_q * s_k * d^-0.5 * log2 e), s_x = fp32(r_x / 127)
void launch_attention_i8(const AttnI8Desc& d, hipStream_t s);
AttnKernel attention_i8_kernel(const AttnI8Desc& d);   // launch_attention_i8's choice, with its shape refusal
// the quantizer in front of it, one launch: qk [B * S][2C] fp16 -> qk_q int8 by inv_q (columns below C) and inv_k, vt [B][C][ldv] fp16
// in the key order vt_perm_in (0 natural, 1 AttnDesc::vt_perm) -> vt_q [B][C][S] int8 in attention_i8_vt_key's order by inv_v; the
// quantizer is ws_quantize8 (quantize8.h).  S % 32 == 0, C % 8 == 0.
void launch_einsum_quantize(const half_t* qk, const half_t* vt, int B, int S, int C, int ldv, int vt_perm_in, float inv_q, float inv_k,
                            float inv_v, int8_t* qk_q, int8_t* vt_q, hipStream_t s);
// the observer of a calibrating handle, one launch: max |q|, |k| (columns of qk) and |V^T| (the S live columns of each row) folded
// into slots[0..2] like launch_absmax_half
void launch_einsum_absmax(const half_t* qk, const half_t* vt, int B, int S, int C, int ldv, float* slots, hipStream_t s);

// Cross-attention front half in one launch (xattn.hip): out = softmax(to_q(LayerNorm(x)) k^T / sqrt(d)) v per head,
// head dim 64, <= 96 keys (unet.py:87-118 with the prompt's K / V hoisted).  x [M][C] is the UN-normalised input; wq /
// bias / colsum are the LayerNorm-folded projection (UNet::fold_layernorm); k [B][L][C], vt [B][C][ldv], out [M][C].
struct XAttnDesc {
  const half_t* x = nullptr;
  const half_t* wq = nullptr;
  const float* bias = nullptr;
  const float* colsum = nullptr;
  const half_t* k = nullptr;
  const half_t* vt = nullptr;
  half_t* out = nullptr;
  int M = 0, C = 0, S = 0, L = 0, ldv = 0, heads = 0;   // S: query tokens per sample (M = B * S)
  float ln_eps = 1e-5f;
  int impl = kAttnOriginal;   // only checked: SPLIT_EINSUM_V2 rejects S % 512 != 0 like the streaming kernel
  int nst = 0;                // LDS-DMA ring depth 2-5 (0 = heuristic)
};
bool xattn_fused_ok(int C, int heads, int S, int L);
void launch_xattn_fused(const XAttnDesc& d, hipStream_t s);

// The whole cross-attention branch in one launch (xattn_out.hip): out = x + to_out(softmax(to_q(LayerNorm(x)) k^T / 8) v) + b_out
// (unet.py:586-591 around :87-118), C = 320 / 640 (5 / 10 heads of 64), 32 query tokens per workgroup, one wave per head.
// wq_t / wo_t: the LayerNorm-folded to_q weights and the to_out weights in the fragment-major layout of launch_xattn_out_retile
// (C * C halves each); q_bias / q_colsum as XAttnDesc::bias / colsum; o_bias [C]; x [M][C] is the UN-normalised block input and the
// residual; k [B][L][C], vt [B][C][ldv] (columns [L, ldv) zero), out [M][C].
struct XAttnOutDesc {
  const half_t* x = nullptr;
  const half_t* wq_t = nullptr;
  const float* q_bias = nullptr;
  const float* q_colsum = nullptr;
  const half_t* k = nullptr;
  const half_t* vt = nullptr;
  const half_t* wo_t = nullptr;
  const float* o_bias = nullptr;
  half_t* out = nullptr;
  int M = 0, C = 0, S = 0, L = 0, ldv = 0, heads = 0;
  float ln_eps = 1e-5f;
  int impl = kAttnOriginal;
  // five heads only: the SELF-attention's output projection in front, in the same launch (unet.py:588): x is then a1 (the
  // self-attention's output), the kernel first forms h1 = h0 + to_out1(a1) + o1_bias - which never goes to HBM - and runs the
  // cross-attention branch on it.  wo1_t fragment-major like wo_t; null = off.
  const half_t* h0 = nullptr;
  const half_t* wo1_t = nullptr;
  const float* o1_bias = nullptr;
};
// The head of a SpatialTransformer in one launch (xattn_out.hip gn_proj_qkv_kernel, round 6): GroupNorm apply (statistics from the
// producer's partials: gn_partial [B][G][kGnMaxSlabs][2], gn_entries of them per (sample, group); 0 = x is normalised already) ->
// proj_in + bias -> h (stored) -> LayerNorm-folded fused q|k|v (UNet::fold_layernorm: qkv_bias / qkv_colsum [3C]) -> qk [M][2C] with
// the queries multiplied by q_scale, vt [B][C][ldT] (vt_perm: AttnDesc::vt_perm).  wp_t (C x C) / wqkv_t (3C x C) fragment-major
// (launch_xattn_out_retile_nk).  C = 320 only.
struct GnProjQkvDesc {
  const half_t* x = nullptr;
  const float* gn_partial = nullptr;
  const float* gn_gamma = nullptr;
  const float* gn_beta = nullptr;
  int gn_entries = 0, gn_groups = 32;
  float gn_eps = 1e-6f;
  const half_t* wp_t = nullptr;
  const float* p_bias = nullptr;
  half_t* h = nullptr;
  const half_t* wqkv_t = nullptr;
  const float* qkv_bias = nullptr;
  const float* qkv_colsum = nullptr;
  float ln_eps = 1e-5f;
  half_t* qk = nullptr;
  half_t* vt = nullptr;
  int M = 0, C = 0, S = 0, ldT = 0;
  bool vt_perm = false;
  float q_scale = 1.f;
  int tok = 0;                // tokens per workgroup: 0 = the launch's rule, 32 / 64 (operator tests)
  long long* clk = nullptr;   // measurement builds of the operator test: [workgroup][wave][16] cycle stamps of the kernel's phases
};
bool gn_proj_qkv_ok(int C, int heads, int S, int M, int ldT, int G);
void launch_gn_proj_qkv(const GnProjQkvDesc& d, hipStream_t s);
bool xattn_out_ok(int C, int heads, int S, int L);
void launch_xattn_out_retile(const half_t* w, half_t* wt, int C, hipStream_t s);   // [C][C] row-major -> fragment-major
void launch_xattn_out(const XAttnOutDesc& d, hipStream_t s);
// The tail of a SpatialTransformer in one launch (xattn_out.hip ffn_proj_kernel): out = res2 + proj_out(res1 + ff.net.2(g) + b1) + b2
// (unet.py:591 FeedForward.net.2 + residual, :561-563 proj_out + residual); C = 320 only.  g [M][K1 = 4C] the GEGLU product,
// w1_t (C x K1) / w2_t (C x C) fragment-major (launch_xattn_out_retile_nk), res1 = the block's h2, res2 = the transformer's input,
// out [M][C].  gn_partial / gn_groups as ConvDesc: GroupNorm statistics of the output for its consumer; returns the entries per
// (sample, group) written (S / 32, or 0).
struct FfnProjDesc {
  const half_t* g = nullptr;
  const half_t* w1_t = nullptr;
  const float* b1 = nullptr;
  const half_t* res1 = nullptr;
  const half_t* w2_t = nullptr;
  const float* b2 = nullptr;
  const half_t* res2 = nullptr;
  half_t* out = nullptr;
  float* gn_partial = nullptr;
  int gn_groups = 0;
  int M = 0, C = 0, K1 = 0, S = 0;   // S: tokens per sample
};
bool ffn_proj_ok(int C, int K1, int M, int S);
int launch_ffn_proj(const FfnProjDesc& d, hipStream_t s);
void launch_xattn_out_retile_nk(const half_t* w, half_t* wt, int N, int K, hipStream_t s);   // [N][K] row-major -> fragment-major

// ---------------------------------------------------------------------------------------------
// CLIP towers: what the text encoder and the safety checker's vision tower share (clip.hip), and the vision tower's own kernels (vit.hip)
// ---------------------------------------------------------------------------------------------
// in-place MLP activation over n halves: 0 = quick_gelu x * sigmoid(1.702 x), 1 = exact-erf gelu
void launch_clip_act(half_t* x, size_t n, int act, hipStream_t s);
// the text encoder's own two (clip.hip): x[s] = tok[ids[s]] + pos[s], and causal attention over qkv [S][3 D] -> out [S][D]
void launch_clip_embed(const int* ids, const half_t* tok, const half_t* pos, half_t* x, int S, int D, int vocab, hipStream_t s);
void launch_clip_attention(const half_t* qkv, half_t* out, int S, int D, int heads, hipStream_t s);
// Non-causal attention over the stacked projection's rows: qkv [B * S][3 * heads * d] = [q | k | v] -> out [B * S][heads * d], one
// workgroup per (batch, head, 64 queries), any S >= 1, d^-0.5 applied in fp32 inside; d must be 64 (else kUnsupported)
bool vit_attention_ok(int d);
void launch_vit_attention(const half_t* qkv, half_t* out, int B, int S, int heads, int d, hipStream_t s);
// AutoencoderKL mid-block attention (vae_attention.hip): one head of width C over S tokens, q / k / v / out [B * S][C] token-major, one
// workgroup per (batch, 64 queries), keys streamed through LDS, no S x S buffer; any S >= 1, C^-0.5 applied in fp32 inside; C must be
// 64, 128, 256 or 512 (else kUnsupported)
bool vae_attention_ok(int C);
void launch_vae_attention(const half_t* q, const half_t* k, const half_t* v, half_t* out, int B, int S, int C, hipStream_t s);
// img (B, 3, I, I) NCHW -> rows [B * (I / p)^2][Kp], column c * p * p + py * p + px (the flattened conv weight's order), columns
// [3 p p, Kp) zero: the patch-embedding conv becomes a 1x1 GEMM over these rows
void launch_vit_patch_rows(const half_t* img, half_t* rows, int B, int I, int p, int Kp, hipStream_t s);
// x [B][S][D]: row 0 = cls + pos[0], row 1 + j = patch[b][j] + pos[1 + j]   (patch [B][S - 1][D], cls [D], pos [S][D])
void launch_vit_tokens(const half_t* patch, const half_t* cls, const half_t* pos, half_t* x, int B, int S, int D, hipStream_t s);
// The safety checker's concept head, fp32 (vit.hip safety_head_kernel): image_embeds [B][P], concept_embeds [n_concepts][P],
// special_embeds [n_special][P], thresholds concept_w / special_w, adjustment = ONE float in device memory (a handle changes it between
// replays of its captured graph) -> has_nsfw [B] (0 / 1), concept_scores [B][n_concepts]
void launch_safety_head(const float* image_embeds, const float* concept_embeds, const float* special_embeds, const float* concept_w,
                        const float* special_w, const float* adjustment, int B, int P, int n_concepts, int n_special, float* has_nsfw,
                        float* concept_scores, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// K6/K7: norms (norm.hip)
// ---------------------------------------------------------------------------------------------
// y[m][:] = (x[m][:]-mean)*rstd * w + b over the channel dim (LayerNormANE, layer_norm.py:51-80)
// the same LayerNorm leaving as int8 [M][C]: xq = ws_quantize8(fp16 value launch_layernorm stores, inv_s) (quantize8.h); w == b == NULL:
// xq = ws_quantize8(x, inv_s), nothing normalised.  Same shape rule; xq 8-byte aligned.
void launch_layernorm_q8(const half_t* x, const float* w, const float* b, int8_t* xq, int M, int C, float eps, float inv_s, hipStream_t s);
void launch_layernorm(const half_t* x, const float* w, const float* b, half_t* y, int M, int C, float eps,
                      hipStream_t s);
// GroupNorm over NHWC with optional channel-concat second source: deterministic two-pass
// statistics (partial: groupnorm_scratch_floats() floats per call) + apply.
int groupnorm_num_slabs(int B, int HW);
size_t groupnorm_scratch_floats(int B, int HW, int G);
// producer_entries > 0: `partial` already holds that many (sum, sumsq) entries per (sample, group), written by the
// epilogue of the kernel that produced x0 (ConvDesc::gn_partial) - the statistics pass is skipped.
void launch_groupnorm(const half_t* x0, int C0, const half_t* x1, int C1, float* partial, const float* gamma,
                      const float* beta, half_t* y, int B, int HW, int G, float eps, int silu, hipStream_t s,
                      int producer_entries = 0, const ConvDesc* side = nullptr);
// `side` (round 5): an INDEPENDENT 1x1 GEMM - the resnet's conv_shortcut over the same input (unet.py:483-486) - that runs in the
// SAME launch as the GroupNorm's apply / single-launch kernel (igemm.hip gn_*_side_kernel: one grid, the first blocks are the
// GroupNorm, the rest the GEMM's tiles).  Must satisfy gn_side_gemm_ok; its result is complete when the launch is.
bool gn_side_gemm_ok(const ConvDesc& d);
void launch_gn_apply_side(const half_t* x0, int C0, const half_t* x1, int C1, const float* partial, int entries, const float* gamma,
                          const float* beta, half_t* y, int B, int HW, int G, float eps, int silu, int slabs, int ppb, const ConvDesc& side,
                          hipStream_t s);
void launch_gn_fused_side(int vw, const half_t* x0, int C0, const half_t* x1, int C1, const float* gamma, const float* beta, half_t* y, int B,
                          int HW, int G, float eps, int silu, const ConvDesc& side, hipStream_t s);
// true when a GroupNorm of this shape would run a separate statistics launch, i.e. producer statistics pay
bool groupnorm_wants_producer_stats(int HW, int C, int G);

// in-place softmax(scale * x) over each row of a [rows][cols] fp16 matrix (VAE single-head attention)
void launch_row_softmax(half_t* x, int rows, int cols, float scale, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// fp32 compute path of the VAE graphs (vae_f32.hip; torch2coreml.py:570-578, :726-733): fp32 NHWC activations
// ---------------------------------------------------------------------------------------------
struct ConvF32Desc {
  const float* x = nullptr;     // [B][Hi][Wi][Cin]
  const void* w = nullptr;      // w_kind 0: half [N][K], 1: float [N][K], 2: float [K][N];  K = ksize*ksize*Cin, tap-major
  int w_kind = 0;
  const float* bias = nullptr;  // [N] or null
  const float* res = nullptr;   // [M][N] or null
  float* out = nullptr;         // [M][N], M = B*Ho*Wo
  int B = 1, Hi = 1, Wi = 1, Cin = 0, Ho = 1, Wo = 1, N = 0;
  int ksize = 1, stride = 1, up = 1;
  int pad = -1;                 // -1: ksize / 2; 0 with stride 2: the VAE encoder's F.pad(x, (0, 1, 0, 1))
};
void launch_conv_f32(const ConvF32Desc& d, hipStream_t s);
size_t groupnorm_f32_scratch_bytes(int B, int G);
void launch_groupnorm_f32(const float* x, void* scratch, const float* gamma, const float* beta, float* y, int B, int HW, int C, int G,
                          float eps, int silu, hipStream_t s);
void launch_row_softmax_f32(float* x, int rows, int cols, float scale, hipStream_t s);
void launch_nchw_to_nhwc_f32(const void* src, int src_is_f32, float* dst, int B, int C, int H, int W, hipStream_t s);
void launch_nhwc_to_nchw_f32f32(const float* src, float* dst, int B, int C, int H, int W, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// K8/K9 + boundary helpers (misc.hip)
// ---------------------------------------------------------------------------------------------
// sinusoidal embedding [cos|sin] (unet.py:703-728), fp32.  t: [n] fp32, freq: [dim/2] device
// copy of timestep_freq_table(dim, freq_shift) -> out [n][dim]
std::vector<float> timestep_freq_table(int dim, float freq_shift);
void launch_timestep_embedding(const float* t, const float* freq, float* out, int n, int dim, hipStream_t s);
// out[b][n] = act_out( sum_k W[n][k]*act_in(x[b][k]) + bias[n] ); x fp32 [B][ldx], out fp32 [B][ldo]
void launch_gemv(const half_t* w, const float* bias, const float* x, int ldx, float* out, int ldo, int B, int N,
                 int K, int silu_in, int silu_out, int accumulate, hipStream_t s);
void launch_nchw_to_nhwc(const void* src, int src_is_f32, half_t* dst, int B, int C, int H, int W, hipStream_t s);
void launch_nhwc_to_nchw_f32(const half_t* src, float* dst, int B, int C, int H, int W, hipStream_t s);
void launch_half_to_float(const half_t* src, float* dst, size_t n, hipStream_t s);
void launch_float_to_half(const float* src, half_t* dst, size_t n, hipStream_t s);
// y = a + b (fp16), used for ControlNet residual adds when not fused
void launch_add_half(const half_t* a, const half_t* b, half_t* y, size_t n, hipStream_t s);
// y = srcs[0] + ... + srcs[nsrc-1] (nsrc <= 4, fp32 accumulation): device-side ControlNet residual sum
void launch_sum_half(const half_t* const* srcs, int nsrc, half_t* y, size_t n, hipStream_t s);
// BC1S (B,C,1,S) fp16 -> token-major [B][S][C] fp16 (encoder_hidden_states boundary)
void launch_bc1s_to_tokens(const half_t* src, half_t* dst, int B, int C, int S, hipStream_t s);

// Device-resident denoising loop helpers (pipeline.py:500-573).  `step` is a device counter.
struct LoopTables {
  const float* timesteps;   // [n_steps]
  const float* coef;        // [n_steps][8]: cx, cm, ch0..ch2, a, b, flags  (cfg_sched_step_kernel, misc.hip)
  int* step;                // device scalar
  const float* in_scale;    // [n_steps] scale_model_input factor (sigma-space schedulers), or null
  unsigned* ticket;         // device scalar (0 between launches): arrival counter of cfg_sched_step_kernel
  // time-embedding table of the whole schedule (or null): [n_steps][temb_rows][temb_ld] rows precomputed by the UNet's time
  // path for every timestep; loop_prep copies row block `step` to temb_dst, so the step itself launches no time-path kernel
  const float* temb_tab;
  float* temb_dst;
  int temb_rows, temb_ld, temb_n;
  // ancestral samplers: [n_steps][Bimg * CHW] noise (already scaled by sigma_up) added to the latents after step `step`, or null
  const float* noise_tab = nullptr;
  // de-noised tap (progress previews, StableDiffusionPipeline.swift:332 `modelOutputs.last`): with `denoised` set, the step kernel also
  // writes pa*x + pb*eps + sum_j ph[j]*hist[j] of the values its update reads; pred [n_steps][8]: pa, pb, ph0..ph2, 0, 0, 0.  Both or neither.
  const float* pred = nullptr;
  float* denoised = nullptr;   // fp32, the latents' layout
};
// latents fp32 NCHW [Bimg][4][H][W] -> UNet sample fp16 NHWC [cfg*Bimg][H][W][4], timestep buffer
void launch_loop_prep(const float* latents, half_t* sample, float* tbuf, LoopTables t, int Bimg, int C, int H,
                      int W, int cfg, hipStream_t s);
// eps = u + g*(c-u) (pipeline.py:561-562); m = a*x + b*eps; latents = cx*x + cm*m + sum ch_j * hist_j; step++
// [t.denoised = pa*x + pb*eps + sum ph_j * hist_j, from the values before the update]
void launch_cfg_sched_step(const float* noise_pred, float* latents, float* eps_hist, LoopTables t, float guidance,
                           int Bimg, int CHW, int cfg, int hist, hipStream_t s);

// Image-to-image start (Encoder.swift:68-89 + Scheduler.swift:83-102) as one element-wise fp32 launch: moments = the encoder's
// [mean | logvar] NCHW fp32 of ONE image (2 * n floats, n = Cz * h * w); std = exp(0.5 * clamp(logvar, -30, 20));
// z = (mean + std * eps) * scale;  out[i] = sa * z + sb * noise[i] for the n_images (n floats each) of noise / out
void launch_posterior_noise(const float* moments, const float* eps, const float* noise, float* out, size_t n, int n_images,
                            float scale, float sa, float sb, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// Image post-processing behind the VAE decoder (imgpost.hip; pipeline.py:286-320, Decoder.swift:40-68, SafetyChecker.swift:55-99)
// ---------------------------------------------------------------------------------------------
// image (B, 3, H, W) fp32 in [-1, 1] -> rgb8 (B, H, W, 3): (np.clip(image / 2 + 0.5, 0, 1) * 255).round().astype("uint8") bit for bit
void launch_image_rgb8(const float* image, uint8_t* rgb8, int B, int H, int W, hipStream_t s);
// Pillow's 8-bit bicubic resize coefficients of one axis (host): ksize taps per output sample; bounds (out, 2) = [xmin, n],
// coeffs (out, ksize) fixed point with kResampleBits fraction bits, zeros behind the n taps of a row
constexpr int kResampleBits = 22;
int resample_ksize(int in_size, int out_size);
void resample_coeffs(int in_size, int out_size, int32_t* bounds, int32_t* coeffs);
// rgb8 (B, H, W, 3) -> clip_input (B, 3, S, S) fp16: resize to rh x rw (two passes, horizontal first, the intermediate image uint8),
// centre crop to S x S, ((float)u / 255.0f - mean[c]) / std[c] with both divisions IEEE-rounded, rounded to fp16.
// The tables of a geometry on the host (plan_clip_input: checks the geometry and the LDS it needs; no device work) ...
struct ClipInputPlan {
  int H = 0, W = 0, rh = 0, rw = 0, S = 0, ksh = 0, ksv = 0;
  std::vector<int32_t> hbounds, hcoeffs, vbounds, vcoeffs;
  size_t lds_bytes = 0;
};
ClipInputPlan plan_clip_input(int H, int W, int rh, int rw, int S);
// ... and what a launch reads: the same tables in device memory
struct ClipInputDesc {
  const int32_t *hbounds, *hcoeffs, *vbounds, *vcoeffs;
  int H, W, S, top, left, ksh, ksv;
  float mean[3], std[3];
};
void launch_clip_input(const uint8_t* rgb8, half_t* out, int B, const ClipInputDesc& d, size_t lds_bytes, hipStream_t s);

// max |x| over x0 [n0] (and x1 [n1], or null) folded into *slot (a non-negative fp32, atomicMax on its bit pattern): the running
// maximum since the slot was zeroed - the activation observers of a calibrating handle (W8A8) and sd_op_absmax
void launch_absmax_half(const half_t* x0, size_t n0, const half_t* x1, size_t n1, float* slot, hipStream_t s);

void launch_lds_poison(hipStream_t s);   // debug (SD_POISON_LDS): NaN patterns into every CU's LDS
void launch_count_nonfinite_half(const void* p, size_t bytes, unsigned long long* out, hipStream_t s);   // debug scan (SD_NAN_TRACE)

}  // namespace sd
