// What the UNet / ControlNet handle (unet.h) and the VAE handles (vae.h) share: one LaunchList for the device, stream, arena,
// conv workspace, main op list and its graph; the conv / GroupNorm / ResNet block builders in fp16 and fp32; and the executor
// (eager lists, the captured forward, per-forward timing and the per-op profile).
#pragma once
#include "../../include/sd_mi355x.h"
#include "conv_plan.h"
#include "launch_list.h"

#include <functional>
#include <map>
#include <set>

namespace sd {

constexpr int kTembCap = 65536;      // floats per batch row for the batched time_emb_proj outputs
inline int round_up(int x, int a) { return (x + a - 1) / a * a; }

// Link between a conv / GEMM op and the GroupNorm that consumes its output: the GroupNorm (built later) asks the
// producer to leave per-tile (sum, sumsq) partials of the tensor in `partial`; at launch time the producer reports how
// many entries per (sample, group) its plan wrote (0: none - split-K, ragged tiles - the GroupNorm runs its own pass).
// `entries` is written by the producer's launch closure (produced()) and taken by the GroupNorm's (consume()): the GroupNorm op
// sits behind its producer in the launch list (Net::group_norm asserts the positions at build time: ops_pos of the producer <
// its own), and at LAUNCH time a consumer that runs without its producer having run since the last consumption - an op timed on
// its own, a list walked out of order - gets 0 entries, i.e. runs its own statistics pass: stale partials are never folded.
struct GnHook {
  float* partial = nullptr;
  int groups = 0;
  int entries = 0;
  bool fresh = false;            // produced() since the last consume()
  void produced(int n) {
    entries = n;
    fresh = true;
  }
  int consume() {
    const int n = fresh ? entries : 0;
    fresh = false;
    return n;
  }
  int ops_pos = -1;              // index of the producing op in its launch list
  const void* ops_list = nullptr;
};

struct Tensor {
  half_t* p = nullptr;          // fp32 handle (Net::f32_): the same bookkeeping over float elements, read through f()
  int B = 0, H = 0, W = 0, C = 0;
  std::shared_ptr<GnHook> gn;   // set on conv / GEMM outputs
  int M() const { return B * H * W; }
  size_t numel() const { return (size_t)B * H * W * C; }
  float* f() const { return reinterpret_cast<float*>(p); }
};

struct OpTime {
  std::string label;
  double flop;
  float ms;
};

// Arguments of Net::conv / conv_w by name; only cout is required.
struct ConvArgs {
  const Tensor* x2 = nullptr;    // second source: channel concat that is never materialised
  int cout = 0;
  int k = 1, stride = 1, up = 1;
  bool bias = true;              // conv: <name>.bias exists in the checkpoint (conv_w takes its bias pointer)
  const float* temb = nullptr;   // time_emb_proj row added per output channel
  const half_t* res = nullptr;   // residual added in the epilogue
  int out_mode = kOutHalf;
  int ldT = 0;                   // kOutHalfT / fused q|k|v: tokens per transposed row
  bool silu_out = false;
  int pad = -1;                  // 0: diffusers Downsample2D(padding=0), F.pad(x, (0, 1, 0, 1)) then a pad-0 stride-2 conv
  // conv_w only - LayerNorm fold (ln_colsum set) and, with it, the fused q|k|v split (n_trans > 0: columns >= n_trans leave
  // token-transposed in *vt_out, [B][cout - n_trans][ldT])
  const float* ln_colsum = nullptr;
  int n_trans = 0;
  half_t** vt_out = nullptr;
  bool vt_perm = false;          // V^T in attention8's key order (AttnDesc::vt_perm)
  float q_scale = 1.f;           // fused q|k|v: the first q_cols columns leave pre-scaled for attention8 (ConvDesc::q_scale)
  int q_cols = 0;
  // The call site opts in to keeping a palettized 1x1 projection / GEGLU projection (out_mode says which) on the device as a pinned
  // plan tile 15 / 16 (conv_plan_weights).  A pinned op cannot move to igemm_kernel when a later GroupNorm asks for epilogue
  // statistics, so only call sites whose output feeds no GroupNorm set it (proj_in, the two to_out.0 and ff.net.0.proj of a transformer
  // block feed LayerNorms or GEMMs).
  bool keep_compressed = false;
  // The call site opts in to running an upsampler conv (k 3, up 2) as four 2x2 phase convs on the low-res image (plan tile 21): the
  // handle then uploads the folded matrix (weight_prep.h subpixel_fold, 16/9 of the bytes) INSTEAD of the 3x3 one.  Taken only where the
  // weights run from fp16 and subpixel_wanted says so (Net::conv); a W8A8-marked or palettized upsampler runs what it ran without it.
  bool subpix = false;
  // conv_w only - the source as int8 [M][C], written by a layernorm_q8 launch in front of this op (plan tiles 20 and 22 read nothing
  // else; x still gives the shape).  With n_trans > 0 it is the fused q|k|v split without the fold (plan tile 22); with the plain
  // epilogue it is ff.net.2 behind the GEGLU (plan tile 24) - weight_plan is asked with any non-null pointer, the question being
  // "would this projection run from int8 activations"
  const int8_t* x_i8 = nullptr;
  // conv_w only, plan tile 20 - the GEGLU product leaves as int8 [M][cout / 2], quantized with out_inv_s (ConvDesc::out_q8): the
  // activations of the plan-tile-24 ff.net.2 behind it.  The returned tensor then has the shape and NO storage (p == nullptr)
  int8_t* out_q8 = nullptr;
  float out_inv_s = 0.f;
};

// The weights conv_w runs from: an fp16 matrix on the device, or a compressed source with its pin (Net::upload_compressed)
struct ConvWeights {
  const half_t* w = nullptr;
  CompressedWeights cw;
  WeightPin pin;
  bool subpix = false;   // w is the folded matrix of subpixel_fold: the conv runs as plan tile 21 (ConvDesc::subpix)
  ConvWeights(const half_t* fp16, bool folded = false) : w(fp16), subpix(folded) {}
  ConvWeights(const CompressedWeights& c, const WeightPin& p) : cw(c), pin(p) {}
};

class Net {
 public:
  virtual ~Net() { close(); }
  Net(const Net&) = delete;
  float time_forward(int warmup, int iters);
  // HIP-event time of every op of one forward, in launch order (eager launches, cold caches between
  // dependent kernels exactly as inside the graph); median over `iters` passes
  std::vector<OpTime> profile(int iters);
  virtual void set_attention(int impl);
  void drop_graphs() { invalidate_graphs(); }   // measurement hook: the next forward re-captures (sd_tune_set_plan_table)
  size_t device_bytes() const { return ll_.arena.bytes(); }
  size_t arena_used_bytes() const { return ll_.arena.used(); }
  // palettes: tensors of the weight store that arrived with one, convs that read theirs on the device (plan tiles 14, 15 and 16), and
  // the bytes of those convs' index streams and LUTs
  void palette_info(int* n_palettized, int* n_streamed, size_t* stream_bytes) const {
    *n_palettized = pal_tensors_;
    *n_streamed = pal_streamed_;
    *stream_bytes = pal_stream_bytes_;
  }
  // W8A8: tensors of the weight store that arrived with a mark, convs that run from int8 (plan tile 17), and the bytes of those convs'
  // int8 streams and scale vectors
  void w8a8_info(int* n_marked, int* n_applied, size_t* bytes) const {
    *n_marked = i8_marked_;
    *n_applied = i8_applied_;
    *bytes = i8_bytes_;
  }
  // W8A8 einsums (WeightStore::quantize_einsum): marks the handle's weight store arrived with, and the attentions that run on the int8
  // kernel (attention_i8.hip), by module name in build order.  The convs' counters above do not count them.
  void einsum_info(int* n_marked, int* n_applied) const {
    *n_marked = einsum_marked_;
    *n_applied = (int)einsum_names_.size();
  }
  const std::vector<std::string>& einsum_applied() const { return einsum_names_; }
  // the activation observers of a handle built from an observing store, in launch order: fills slot `index` (name of the conv's weight
  // tensor, running max |x| of its source(s) since creation) when it exists; returns the number of slots.  An einsum's three slots are
  // named <module>.q / .k / .v (no weight tensor), the q value divided by the factor its producer pre-scaled the queries by.
  int activation_range(int index, std::string* name, float* absmax);
  const std::vector<std::string>& w8a8_applied() const { return i8_names_; }   // weight tensors of the convs that run from int8, in build order
  const sd_unet_config& config() const { return cfg_; }
  // Swap the values of the tensors `names` for those `ws` holds (sd_unet_reload_weights): every refill record whose sources meet
  // `names` runs again, into the addresses it filled at build time.  Everything is checked before the first byte is overwritten.
  virtual void reload_weights(const WeightStore& ws, const std::vector<std::string>& names);

 protected:
  Net(const sd_unet_config& cfg, const WeightStore& ws, int device);   // checks the shared config fields, then open()
  void open(int device) { ll_.open(device); }
  void seal();    // end of construction: the conv workspace, uploads complete, the weight store is not read again
  void close() { ll_.close(); }

  // ---- build ----
  Tensor new_tensor(int B, int H, int W, int C);
  half_t* upload_conv_weight(const std::string& name, int cout, int cin, int k, bool geglu);
  float* upload_conv_weight_f32(const std::string& name, int cout, int cin, int k);   // the same layout in fp32 (compute_fp32 handles)
  half_t* upload_subpixel_weight(const std::string& name, int cout, int cin);         // a 3x3 upsampler's weights folded for plan tile 21
  float* upload_vec(const std::string& name, int n, bool geglu = false);
  // conv uploads <name>.weight / .bias and emits the op; conv_w (fp16 only) takes device pointers
  Tensor conv(std::vector<Op>& ops, const std::string& name, const Tensor& x, const ConvArgs& a);
  Tensor conv_w(std::vector<Op>& ops, const std::string& name, const ConvWeights& w, const float* bias, const Tensor& x, const ConvArgs& a);
  // What the conv of <name>.weight reads its weights from: the planner's answer (conv_plan_weights) for what the store holds for the
  // tensor - a palette, a W8A8 mark - with the LayerNorm fold for `ln` (asked before fold_layernorm, which then skips the fp16 upload).
  // upload_compressed then uploads a compressed answer (the palette's stream and LUT and, with the fold, `ln_name`.weight; the int8
  // stream and scales) and keeps the handle's counters; an Fp16 answer goes through upload_conv_weight as ever
  WeightPin weight_plan(const std::string& name, const Tensor& x, const ConvArgs& a, bool ln) const;
  ConvWeights upload_compressed(const std::string& name, const WeightPin& pin, int cin, const ConvArgs& a, const std::string& ln_name = std::string());
  // Calibration of the GEGLU projections (WeightStore::observe_geglus while the store observes): would a W8A8 mark on <name>.weight
  // make this GEGLU run as plan tile 20?  Then the caller normalises the GEGLU's input into a scratch tensor and observe_tensor puts
  // an absmax launch over it, into a slot named <name>.weight - two ordinary launches that write nothing the model reads.
  bool observes_geglu(const std::string& name, const Tensor& x, const ConvArgs& a, bool ln) const;
  // Calibration of the transformer tails (WeightStore::observe_tails while the store observes): would a W8A8 mark on <name>.weight make
  // this projection (a: its ConvArgs with x_i8 set, as weight_plan is asked) run as plan tile 24 / (x_i8 null) as plan tile 19?
  bool observes_tail(const std::string& name, const Tensor& x, const ConvArgs& a) const;
  // (report_as: the weight names, without ".weight", the one slot is reported under - <name> alone when empty)
  void observe_tensor(std::vector<Op>& ops, const std::string& name, const Tensor& t, const std::vector<std::string>& report_as = {});
  // Calibration of the einsums (WeightStore::observe_einsums while the store observes): ONE launch over the q | k rows and the V^T
  // a q|k|v producer left, into three slots <module>.q / .k / .v; the q slot is reported divided by q_div (the producer's pre-scale)
  bool observes_einsums() const { return !f32_ && ws_->observe() && ws_->observe_einsums(); }
  void observe_einsum(std::vector<Op>& ops, const std::string& module, const half_t* qk, const half_t* vt, int B, int S, int C, int ldv, float q_div);
  // the handle runs the einsum `module` on the int8 attention kernel
  void einsum_applies(const std::string& module) { einsum_names_.push_back(module); }
  // The fused q|k|v launch `name` over the projections `parts` (to_q, to_k, to_v) in W8A8: qkv_plan answers I8Qkv (plan tile 22) when
  // every part carries a mark, none a palette, all marks share one act_absmax (one int8 tensor carries one scale) and the planner takes
  // the un-folded shape (a: cout, ldT, n_trans, vt_perm, q_scale, q_cols of the launch) - else Fp16: the folded launch as ever.
  // upload_qkv_i8 then uploads the stacked int8 matrix and scales, no fp16 copy, and counts every part as applied, in order.
  // observes_qkv: the store observes them (WeightStore::observe_qkv) and a mark would make this launch plan tile 22 - the caller then
  // puts a LayerNorm + observe_tensor pair beside the folded launch, reported under all parts.
  WeightPin qkv_plan(const std::string& name, const std::vector<std::string>& parts, const Tensor& x, const ConvArgs& a) const;
  bool observes_qkv(const std::string& name, const std::vector<std::string>& parts, const Tensor& x, const ConvArgs& a) const;
  ConvWeights upload_qkv_i8(const std::vector<std::string>& parts, const WeightPin& pin, int cin, int cout_each);
  // 3x3 conv to N <= 8 channels, one wavefront per pixel (conv_small.hip): fp32 NCHW into out_nchw (a model's boundary), else
  // fp16 NHWC into out_nhwc.  An fp32 handle runs the fp32 conv into out_nhwc (or a tensor of its own) and transposes.
  void conv_small_n(std::vector<Op>& ops, const std::string& name, const Tensor& x, int cout, half_t* out_nhwc, float* out_nchw);
  // side (round 5): an independent 1x1 GEMM launched in the SAME grid as the GroupNorm's apply / single-launch kernel
  // (launch_groupnorm); side_label / side_flop describe it in the per-op profile
  Tensor group_norm(std::vector<Op>& ops, const std::string& name, const Tensor& x, const Tensor* x2, float eps,
                    bool silu, const ConvDesc* side = nullptr, const std::string& side_label = std::string(), double side_flop = 0);
  // temb: this resnet's row of time_emb_proj outputs (the UNet registers it), null without a time embedding (VAE)
  Tensor resnet(std::vector<Op>& ops, const std::string& p, const Tensor& x, const Tensor* x2, int cout, const float* temb);

  // ---- refill records (host only, outside the arena) ----
  // Every upload site states its layout ONCE, as a closure from a weight store to the device addresses it allocated: `refill` runs
  // it on the store the handle is built from and keeps it with the names of the tensors it reads, reload_weights runs it again on
  // another store.  `made` (may be null) is the device matrix the closure writes: a derived copy made from it by a device launch
  // (`derive`: the fragment-major retiles) then follows the same sources.
  using Fill = std::function<void(const WeightStore&)>;
  void refill(const std::vector<std::string>& sources, const void* made, Fill fill);
  void derive(const void* from, std::function<void()> launch);
  void holds_compressed(const std::string& wname) { compressed_.insert(wname); }
  virtual void after_reload() {}   // what a handle caches between calls from weights and inputs (the UNet's hoisted K / V^T)

  // ---- run ----
  void run_ops(const std::vector<Op>& ops) { run_ops_on(ops, ll_.stream); }
  void run_ops_on(const std::vector<Op>& ops, hipStream_t s);
  virtual void run_eager() { run_ops(ll_.ops); }   // one forward between the boundary copies, launch by launch
  void run_forward();                              // the same as one graph replay when cfg.use_graph (captured on first use)
  virtual void invalidate_graphs();
  // the op lists of one forward in launch order, for profile()
  virtual std::vector<const std::vector<Op>*> forward_lists() const { return {&ll_.ops}; }

  sd_unet_config cfg_;
  const WeightStore* ws_ = nullptr;   // only valid during construction
  bool f32_ = false;                  // VAE handle with cfg.compute_fp32: fp32 activations on the vae_f32.hip kernels
  LaunchList ll_;                     // ll_.ops is the main list, ll_.graph one captured forward
  bool have_inputs_ = false;

 private:
  ConvDesc conv_shape(const std::string& name, const Tensor& x, const ConvArgs& a) const;
  ConvDesc qkv_shape(const std::string& name, const Tensor& x, const ConvArgs& a) const;
  int pal_tensors_ = 0, pal_streamed_ = 0;
  size_t pal_stream_bytes_ = 0;
  int i8_marked_ = 0, i8_applied_ = 0;
  size_t i8_bytes_ = 0;
  struct Observed {
    std::string first;
    float* second;
    float div = 1.f;   // the value is reported divided by this (1: as observed)
  };
  std::vector<Observed> observed_;
  int einsum_marked_ = 0;
  std::vector<std::string> einsum_names_;
  std::vector<std::string> i8_names_;
  struct Refill {
    std::vector<std::string> sources;
    Fill fill;
  };
  std::vector<Refill> refills_;                                   // in build order: a derived copy behind the matrix it reads
  std::map<std::string, std::vector<int64_t>> source_shape_;      // every tensor a record reads, as the handle was built with it
  std::map<const void*, std::vector<std::string>> made_from_;     // device matrix -> the tensors it was made from
  std::set<std::string> compressed_;                              // tensors held as a palette stream or int8: no fp16 / fp32 form to refill
  bool observing_ = false;                                        // built from an observing store
  Tensor conv_f32(std::vector<Op>& ops, const std::string& name, const Tensor& x, const ConvArgs& a);
  Tensor group_norm_f32(std::vector<Op>& ops, const std::string& name, const Tensor& x, float eps, bool silu);
};

// hipEvents that are destroyed on every exit path
struct EventList {
  std::vector<hipEvent_t> ev;
  explicit EventList(size_t n) {
    ev.reserve(n);
    for (size_t i = 0; i < n; ++i) {
      hipEvent_t e = nullptr;
      SD_HIP(hipEventCreate(&e));
      ev.push_back(e);
    }
  }
  ~EventList() {
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
  }
  hipEvent_t operator[](size_t i) const { return ev[i]; }
};

}  // namespace sd

struct sd_unet {
  std::unique_ptr<sd::Net> impl;
};
