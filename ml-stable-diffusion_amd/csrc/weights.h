// Host-side checkpoint store: {diffusers key -> fp32 tensor}.  Replaces torch's
// load_state_dict + the reference's two load hooks (unet.py:121-146): we keep checkpoint
// tensors as-is and re-lay them out for the kernels when a model handle is built.
#pragma once
#include "sd_common.h"

namespace sd {

struct HostTensor {
  std::vector<int64_t> shape;
  std::vector<float> data;
  size_t numel() const {
    size_t n = 1;
    for (auto s : shape) n *= (size_t)s;
    return n;
  }
};

// A palettized tensor (the reference's fake_palettize with one group, mixed_bit_compression_pre_analysis.py:139-156): the tensor
// the model sees is lut[indices].  The HostTensor beside it already holds those values, so every consumer of the store reads the
// de-palettized weights unchanged; only the weight-stream conv (wstream.hip, plan tile 14) keeps the indices on the device.
struct Palette {
  int nbits = 0;                  // 1, 2, 4, 6 or 8
  std::vector<uint16_t> lut;      // 2^nbits fp16 bit patterns, ascending where palettize() made them
  std::vector<uint8_t> indices;   // one per element, in the tensor's own order
};

// A W8A8 mark on a conv weight (the reference's quantize_cumulative_config, activation_quantization.py:141-203: symmetric int8,
// one scale per output channel for the weights, one per tensor for the activations the conv reads; parity with coremltools'
// quantizer unpinned).  The HostTensor beside it keeps the untouched values: a handle runs the conv from `q` only where its plan is
// the weight stream (wstream.hip, plan tile 17), every other consumer reads fp16 as ever - the reference's "skipped layer".
struct W8A8Mark {
  std::vector<int8_t> q;        // one per element, in the tensor's own order, -127 .. 127
  std::vector<float> w_scale;   // [Cout]
  float act_absmax = 0.f;       // s_a = act_absmax / 127
};

// A W8A8 mark on an attention's Einsum (activation_quantization.py:205-215 collects every Einsum beside every Conv2d; unet.py:45-59 is
// the module): the module has no tensor, so the mark stands on its own under the module's name, <prefix>.einsum beside
// <prefix>.to_q.weight.  The three ranges are max |.| of the module's inputs q, k and v; a handle runs a marked attn1.einsum on the
// int8 attention kernel (attention_i8.hip) where its shape rule holds, everything else in fp16 as ever.
struct EinsumMark {
  float q_absmax = 0.f, k_absmax = 0.f, v_absmax = 0.f;
};

class WeightStore {
 public:
  // marks the Einsum module `name` = <prefix>.einsum (kNotFound when <prefix>.to_q.weight is absent or the name has no ".einsum" suffix;
  // kInvalidArgument: a range that is not a positive finite number)
  void quantize_einsum(const std::string& name, float q_absmax, float k_absmax, float v_absmax);
  const EinsumMark* einsum(const std::string& name) const;   // nullptr: no mark
  size_t einsum_marks() const { return einsum_.size(); }
  const std::map<std::string, EinsumMark>& einsums() const { return einsum_; }   // name order
  // ... and, while observing, ONE launch behind every q|k|v producer whose self-attention the int8 kernel could take: max |q|, |k|, |v|
  void set_observe_einsums(bool on) { observe_einsums_ = on; }
  bool observe_einsums() const { return observe_einsums_; }
  // marks the 4-D tensor `name` (kNotFound when absent; kInvalidArgument: not (Cout, Cin, k, k), a palette on it, act_absmax not a
  // positive finite number, a non-finite weight); returns the squared weight error
  double quantize_w8a8(const std::string& name, float act_absmax);
  const W8A8Mark* w8a8(const std::string& name) const;   // nullptr: no mark
  size_t w8a8_marks() const { return i8_.size(); }
  // handles built from this store put an absmax observer in front of every conv plan tile 17 could take
  void set_observe(int level) { observe_ = level; }   // 0 off, 1 the convs plan tile 17 could take, 2 also those of plan tile 18
  int observe() const { return observe_; }
  // ... and, while observing, in front of every projection plan tile 19 could take at a call site that consents to a pinned 1x1 kernel
  void set_observe_gemms(bool on) { observe_gemms_ = on; }
  bool observe_gemms() const { return observe_gemms_; }
  // ... and over the LayerNorm output in front of every GEGLU projection plan tile 20 could take (two launches beside the folded GEGLU)
  void set_observe_geglus(bool on) { observe_geglus_ = on; }
  bool observe_geglus() const { return observe_geglus_; }
  // ... and over the output of norm1 in front of every fused q|k|v launch plan tile 22 could take (the same two launches)
  void set_observe_qkv(bool on) { observe_qkv_ = on; }
  bool observe_qkv() const { return observe_qkv_; }
  // ... and over the GEGLU product in front of every ff.net.2 plan tile 24 could take, and over a scratch ff.net.2 output in front of its proj_out
  void set_observe_tails(bool on) { observe_tails_ = on; }
  bool observe_tails() const { return observe_tails_; }
  void add(const std::string& name, const void* data, int dtype /*0 f16, 1 f32, 2 bf16*/,
           const int64_t* shape, int ndim);
  void load_safetensors(const std::string& path, const std::string& prefix);
  // overwrites the values of an existing tensor in place (kNotFound when absent, kInvalidArgument unless n is its element count);
  // a palette or a W8A8 mark on it is dropped: the tensor is then a plain one holding `values`
  void set_values(const std::string& name, const float* values, size_t n);
  const HostTensor& get(const std::string& name) const;   // throws kNotFound
  const HostTensor* find(const std::string& name) const;  // nullptr when absent (deprecated VAE attention names accepted)
  bool has(const std::string& name) const { return find(name) != nullptr; }
  size_t size() const { return map_.size(); }
  // Exact 1-D k-means (dynamic programming over the sorted distinct fp16 values) of the stored tensor into 2^nbits entries; the
  // tensor's data becomes lut[indices].  Returns the squared error against the fp16-rounded values it clustered.
  double palettize(const std::string& name, int nbits);
  void add_palettized(const std::string& name, const void* lut_f16, int nbits, const uint8_t* indices, const int64_t* shape, int ndim);
  const Palette* palette(const std::string& name) const;   // nullptr: the tensor has none
  // handles built from this store while the switch is on also run the palettized 3x3 halo convs from their palette (plan tile 25); off
  // by default, and with it off a handle is what it was before the switch existed
  void set_palette_halo(bool on) { palette_halo_ = on; }
  bool palette_halo() const { return palette_halo_; }
  size_t palettes() const { return pal_.size(); }
  const std::map<std::string, HostTensor>& tensors() const { return map_; }   // name order

 private:
  std::map<std::string, HostTensor> map_;
  std::map<std::string, Palette> pal_;
  std::map<std::string, W8A8Mark> i8_;
  std::map<std::string, EinsumMark> einsum_;
  int observe_ = 0;
  bool observe_gemms_ = false;
  bool observe_geglus_ = false;
  bool observe_qkv_ = false;
  bool observe_tails_ = false;
  bool observe_einsums_ = false;
  bool palette_halo_ = false;
};

}  // namespace sd

struct sd_weights {
  sd::WeightStore store;
};
