// Builders and executor shared by the UNet / ControlNet and VAE handles (net.h).
//  * static shapes like the reference's Core ML models (pipeline.py:112-114): everything is allocated once, each tensor owns
//    its bytes (288 GB HBM), so a forward is a pure launch list and is captured into one HIP graph.
//  * channels-last activations, fp16 (or fp32 on a compute_fp32 VAE handle: each op has its two forms as two functions, chosen
//    once at the top of conv / group_norm); weights re-laid-out at load to [Cout][ky][kx][Cin].
#include "net.h"

#include <algorithm>
#include <type_traits>

#include "conv_plan.h"
#include "weight_prep.h"

namespace sd {

Net::Net(const sd_unet_config& cfg, const WeightStore& ws, int device)
    : cfg_(cfg), ws_(&ws), f32_(cfg.compute_fp32 != 0), pal_tensors_((int)ws.palettes()), i8_marked_((int)ws.w8a8_marks()), einsum_marked_((int)ws.einsum_marks()),
      observing_(ws.observe() != 0) {
  SD_REQUIRE(cfg.n_levels >= 1 && cfg.n_levels <= SD_MAX_LEVELS, kInvalidArgument, "n_levels=%d", cfg.n_levels);
  SD_REQUIRE(cfg.batch >= 1 && cfg.height >= 1 && cfg.width >= 1, kInvalidArgument, "bad batch/size");
  SD_REQUIRE(cfg.norm_num_groups >= 1 && cfg.norm_num_groups <= 64, kUnsupported, "norm_num_groups=%d",
             cfg.norm_num_groups);
  open(device);
}

void Net::seal() {
  ll_.seal();
  ws_ = nullptr;
}

Tensor Net::new_tensor(int B, int H, int W, int C) {
  Tensor t;
  t.B = B;
  t.H = H;
  t.W = W;
  t.C = C;
  t.p = ll_.arena.alloc_n<half_t>(t.numel() * (f32_ ? 2 : 1));   // compute_fp32: the same bookkeeping over float elements
  return t;
}

// [Cout][Cin][k][k] (or Linear [Cout][Cin]) -> [Cout][k][k][Cin] fp16.  GEGLU (ff.net.0.proj,
// unet.py:613-617): rows re-ordered so value/gate channels interleave in blocks of 32 and the
// GEMM epilogue can multiply them in registers.
half_t* Net::upload_conv_weight(const std::string& name, int cout, int cin, int k, bool geglu) {
  const size_t expect = (size_t)cout * cin * k * k;
  half_t* d = ll_.arena.alloc_n<half_t>(expect);
  refill({name + ".weight"}, d, [=](const WeightStore& ws) {
    const HostTensor& t = ws.get(name + ".weight");
    SD_REQUIRE(t.numel() == expect, kInvalidArgument, "%s.weight has %zu elements, expected %zu (%d,%d,%d,%d)",
               name.c_str(), t.numel(), expect, cout, cin, k, k);
    std::vector<half_t> host(expect);
    retile_ohwi(t.data.data(), cout, cin, k, geglu, host.data());
    SD_HIP(hipMemcpy(d, host.data(), expect * sizeof(half_t), hipMemcpyHostToDevice));
  });
  return d;
}

// an upsampler's (Cout, Cin, 3, 3) tensor folded into the four 2x2 phase matrices of plan tile 21, [4][Cout][4][Cin] fp16 (subpixel_fold)
half_t* Net::upload_subpixel_weight(const std::string& name, int cout, int cin) {
  const size_t expect = (size_t)cout * cin * 9;
  half_t* d = ll_.arena.alloc_n<half_t>(subpixel_fold_halves(cout, cin));
  refill({name + ".weight"}, d, [=](const WeightStore& ws) {
    const HostTensor& t = ws.get(name + ".weight");
    SD_REQUIRE(t.numel() == expect, kInvalidArgument, "%s.weight has %zu elements, expected %zu (%d,%d,3,3)", name.c_str(), t.numel(), expect, cout, cin);
    std::vector<half_t> host(subpixel_fold_halves(cout, cin));
    subpixel_fold(t.data.data(), cout, cin, host.data());
    SD_HIP(hipMemcpy(d, host.data(), host.size() * sizeof(half_t), hipMemcpyHostToDevice));
  });
  return d;
}

// the same tensor in the same [Cout][k][k][Cin] layout, kept fp32: what the convs of a compute_fp32 handle read (ConvF32Desc::w_kind 1)
float* Net::upload_conv_weight_f32(const std::string& name, int cout, int cin, int k) {
  const size_t expect = (size_t)cout * cin * k * k;
  float* d = ll_.arena.alloc_n<float>(expect);
  refill({name + ".weight"}, d, [=](const WeightStore& ws) {
    const HostTensor& t = ws.get(name + ".weight");
    SD_REQUIRE(t.numel() == expect, kInvalidArgument, "%s.weight has %zu elements, expected %zu (%d,%d,%d,%d)", name.c_str(), t.numel(), expect,
               cout, cin, k, k);
    std::vector<float> host(expect);
    retile_ohwi(t.data.data(), cout, cin, k, false, host.data());
    SD_HIP(hipMemcpy(d, host.data(), expect * sizeof(float), hipMemcpyHostToDevice));
  });
  return d;
}

float* Net::upload_vec(const std::string& name, int n, bool geglu) {
  SD_REQUIRE((int)ws_->get(name).numel() == n, kInvalidArgument, "%s has %zu elements, expected %d", name.c_str(), ws_->get(name).numel(), n);
  float* d = ll_.arena.alloc_n<float>(n);
  refill({name}, d, [=](const WeightStore& ws) {
    const HostTensor& t = ws.get(name);
    SD_REQUIRE((int)t.numel() == n, kInvalidArgument, "%s has %zu elements, expected %d", name.c_str(), t.numel(), n);
    std::vector<float> host(t.data);
    if (geglu)
      for (int o = 0; o < n; ++o) host[geglu_row(o, n)] = t.data[o];
    SD_HIP(hipMemcpy(d, host.data(), (size_t)n * sizeof(float), hipMemcpyHostToDevice));
  });
  return d;
}

// ---- refill records ----------------------------------------------------------------------------
void Net::refill(const std::vector<std::string>& sources, const void* made, Fill fill) {
  for (const std::string& s : sources) source_shape_[s] = ws_->get(s).shape;
  fill(*ws_);
  if (made) made_from_[made] = sources;
  refills_.push_back({sources, std::move(fill)});
}

void Net::derive(const void* from, std::function<void()> launch) {
  auto it = made_from_.find(from);
  SD_REQUIRE(it != made_from_.end(), kInternal, "a derived weight copy of a matrix no refill record made");
  launch();
  refills_.push_back({it->second, [launch](const WeightStore&) { launch(); }});
}

// Order: everything about every name and every record that will run is checked first; then the stream is drained, the records run
// in build order (a blocking copy, then the launches that read it, on the handle's stream), and the stream is drained again.
void Net::reload_weights(const WeightStore& ws, const std::vector<std::string>& names) {
  SD_REQUIRE(!observing_, kUnsupported, "reload_weights: the handle was built from an observing store (its observers' ranges belong to the weights it was built with)");
  const std::set<std::string> wanted(names.begin(), names.end());
  for (const std::string& n : wanted) {
    const HostTensor* t = ws.find(n);
    if (!t) fail(kNotFound, "reload_weights: the store has no tensor '%s'", n.c_str());
    SD_REQUIRE(!compressed_.count(n), kUnsupported, "reload_weights: the handle holds '%s' compressed on the device (a palette stream or int8); only fp16 / fp32 tensors reload",
               n.c_str());
  }
  std::vector<const Refill*> run;
  for (const Refill& r : refills_)
    if (std::any_of(r.sources.begin(), r.sources.end(), [&](const std::string& s) { return wanted.count(s) != 0; })) run.push_back(&r);
  for (const Refill* r : run)
    for (const std::string& s : r->sources) {   // a record reads all its sources again: each must be there, in the shape it was built with
      const HostTensor* t = ws.find(s);
      if (!t) fail(kNotFound, "reload_weights: the store has no tensor '%s' (read together with a named one)", s.c_str());
      SD_REQUIRE(t->shape == source_shape_.at(s), kInvalidArgument, "reload_weights: '%s' has another shape than the tensor the handle was built with", s.c_str());
    }
  if (run.empty()) return;
  SD_HIP(hipSetDevice(ll_.device));
  SD_HIP(hipStreamSynchronize(ll_.stream));
  for (const Refill* r : run) r->fill(ws);
  after_reload();
  SD_HIP(hipStreamSynchronize(ll_.stream));
}

namespace {
// output size of a conv over x, and its ConvDesc / ConvF32Desc pad field (-1: ksize / 2 on every side)
struct ConvGeom {
  int Ho, Wo, pad;
};
ConvGeom conv_geom(const std::string& name, const Tensor& x, const ConvArgs& a) {
  const int Hup = x.H * a.up, Wup = x.W * a.up, pad = a.k / 2;
  if (a.pad >= 0) {   // diffusers Downsample2D(padding=0): F.pad(x, (0, 1, 0, 1)) then a pad-0 stride-2 conv
    SD_REQUIRE(a.pad == 0 && a.stride == 2 && a.k == 3, kUnsupported, "%s: explicit padding %d", name.c_str(), a.pad);
    return {(Hup + 1 - a.k) / a.stride + 1, (Wup + 1 - a.k) / a.stride + 1, 0};
  }
  return {(Hup + 2 * pad - a.k) / a.stride + 1, (Wup + 2 * pad - a.k) / a.stride + 1, -1};
}
}  // namespace

// A tensor the store holds compressed stays compressed on the device where a kernel reads that form (conv_plan_weights): the handle
// uploads the packed stream with its LUT / scales and no fp16 copy (a palettized 3x3 halo conv - resnet conv1 / conv2, the two-source
// convs of the up blocks, upsamplers, which then take plan tile 25 and not the sub-pixel tile 21 - only while the store's switch
// sd_weights_palette_halo is on).  Everywhere else a palettized tensor goes up as lut[indices] and
// a W8A8-marked one as fp16 (the reference's "skipped layer").
Tensor Net::conv(std::vector<Op>& ops, const std::string& name, const Tensor& x, const ConvArgs& a) {
  if (f32_) return conv_f32(ops, name, x, a);
  const int cin = x.C + (a.x2 ? a.x2->C : 0);
  const bool geglu = a.out_mode == kOutGeglu;
  const float* b = a.bias ? upload_vec(name + ".bias", a.cout, geglu) : nullptr;
  const WeightPin pin = weight_plan(name, x, a, false);
  // An observing store (calibration) puts an absmax op over the conv's source(s) in front of every conv the int8 weight stream could
  // take (level 1) or either int8 conv kernel could (level 2: the halo conv too): an ordinary member of the launch list that writes one
  // slot nothing else reads.  A store that also observes the projections (observe_gemms) asks with the call site's consent to a pinned
  // 1x1 kernel, and the small-M int8 GEMM (plan tile 19) may be the answer; without that flag the question and the answer are unchanged.
  const WeightSource could = ws_->observe() && !ws_->palette(name + ".weight") && !a.silu_out
                                 ? conv_plan_weights(conv_shape(name, x, a), StoredWeights::W8A8, ws_->observe_gemms() && a.keep_compressed).kind
                                 : WeightSource::Fp16;
  if (could == WeightSource::I8Wstream || (could == WeightSource::I8Halo && ws_->observe() >= 2) || could == WeightSource::I8Gemm) {
    float* slot = ll_.arena.alloc_n<float>(1);   // (the arena is zeroed: the running maximum starts at 0)
    observed_.push_back({name + ".weight", slot});
    const half_t *p0 = x.p, *p1 = a.x2 ? a.x2->p : nullptr;
    const size_t n0 = x.numel(), n1 = a.x2 ? a.x2->numel() : 0;
    ops.push_back([=](hipStream_t s) { launch_absmax_half(p0, n0, p1, n1, slot, s); });
    ops.back().label = "absmax " + name;
  }
  if (pin.kind != WeightSource::Fp16) return conv_w(ops, name, upload_compressed(name, pin, cin, a), b, x, a);
  // An opted-in upsampler whose weights run from fp16 (an observing store's do: the conv itself stays fp16) goes up folded, as four
  // 2x2 phase convs on the low-res image, where the library's rule takes the shape: plan tile 21 instead of tile 7.  Every question
  // above was asked with the unchanged up = 2 descriptor.
  if (a.subpix && !a.silu_out && subpixel_wanted(conv_shape(name, x, a))) return conv_w(ops, name, ConvWeights(upload_subpixel_weight(name, a.cout, cin), true), b, x, a);
  return conv_w(ops, name, upload_conv_weight(name, a.cout, cin, a.k, geglu), b, x, a);
}

WeightPin Net::weight_plan(const std::string& name, const Tensor& x, const ConvArgs& a, bool ln) const {
  if (f32_ || a.silu_out) return {};
  const StoredWeights held = ws_->palette(name + ".weight") ? StoredWeights::Palette
                             : ws_->w8a8(name + ".weight")  ? StoredWeights::W8A8
                                                            : StoredWeights::Fp16;
  ConvDesc d = conv_shape(name, x, a);
  static const float present = 0.f;   // the planner only tests the pointers
  if (ln) d.ln_colsum = d.bias = &present;
  return conv_plan_weights(d, held, a.keep_compressed, ws_->palette_halo());
}

bool Net::observes_geglu(const std::string& name, const Tensor& x, const ConvArgs& a, bool ln) const {
  if (f32_ || !ws_->observe() || !ws_->observe_geglus() || ws_->palette(name + ".weight") || a.out_mode != kOutGeglu) return false;
  ConvDesc d = conv_shape(name, x, a);
  static const float present = 0.f;   // the planner only tests the pointers
  if (ln) d.ln_colsum = d.bias = &present;
  return conv_plan_weights(d, StoredWeights::W8A8, a.keep_compressed).kind == WeightSource::I8Geglu;
}

bool Net::observes_tail(const std::string& name, const Tensor& x, const ConvArgs& a) const {
  if (f32_ || !ws_->observe() || !ws_->observe_tails() || ws_->palette(name + ".weight") || a.out_mode != kOutHalf) return false;
  const WeightSource could = conv_plan_weights(conv_shape(name, x, a), StoredWeights::W8A8, a.keep_compressed).kind;
  return could == (a.x_i8 ? WeightSource::I8GemmQ : WeightSource::I8Gemm);
}

void Net::observe_tensor(std::vector<Op>& ops, const std::string& name, const Tensor& t, const std::vector<std::string>& report_as) {
  float* slot = ll_.arena.alloc_n<float>(1);   // (the arena is zeroed: the running maximum starts at 0)
  if (report_as.empty()) observed_.push_back({name + ".weight", slot});
  for (const std::string& n : report_as) observed_.push_back({n + ".weight", slot});   // one observation under several names
  const half_t* p0 = t.p;
  const size_t n0 = t.numel();
  ops.push_back([=](hipStream_t s) { launch_absmax_half(p0, n0, nullptr, 0, slot, s); });
  ops.back().label = "absmax " + name;
}

void Net::observe_einsum(std::vector<Op>& ops, const std::string& module, const half_t* qk, const half_t* vt, int B, int S, int C, int ldv, float q_div) {
  float* slots = ll_.arena.alloc_n<float>(3);   // (the arena is zeroed: the running maxima start at 0)
  observed_.push_back({module + ".q", slots, q_div});
  observed_.push_back({module + ".k", slots + 1});
  observed_.push_back({module + ".v", slots + 2});
  ops.push_back([=](hipStream_t s) { launch_einsum_absmax(qk, vt, B, S, C, ldv, slots, s); });
  ops.back().label = "absmax " + module;
}

// the un-folded descriptor of the fused q|k|v launch, as the planner is asked about it
ConvDesc Net::qkv_shape(const std::string& name, const Tensor& x, const ConvArgs& a) const {
  ConvArgs plain = a;
  plain.ln_colsum = nullptr;
  plain.x_i8 = nullptr;
  ConvDesc d = conv_shape(name, x, plain);
  static const half_t present = 0;   // the planner only tests the pointer
  d.out_t = const_cast<half_t*>(&present);
  d.n_trans = a.n_trans;
  d.vt_perm = a.vt_perm ? 1 : 0;
  d.q_scale = a.q_scale;
  d.q_cols = a.q_cols;
  return d;
}

WeightPin Net::qkv_plan(const std::string& name, const std::vector<std::string>& parts, const Tensor& x, const ConvArgs& a) const {
  if (f32_ || a.silu_out || parts.empty()) return {};
  const W8A8Mark* first = nullptr;
  for (const std::string& p : parts) {   // every tensor marked, none palettized, one range: one int8 tensor carries one scale
    const W8A8Mark* m = ws_->w8a8(p + ".weight");
    if (!m || ws_->palette(p + ".weight")) return {};
    if (!first) first = m;
    if (m->act_absmax != first->act_absmax) return {};
  }
  return conv_plan_weights(qkv_shape(name, x, a), StoredWeights::W8A8, true);
}

bool Net::observes_qkv(const std::string& name, const std::vector<std::string>& parts, const Tensor& x, const ConvArgs& a) const {
  if (f32_ || !ws_->observe() || !ws_->observe_qkv()) return false;
  for (const std::string& p : parts)
    if (ws_->palette(p + ".weight")) return false;
  return conv_plan_weights(qkv_shape(name, x, a), StoredWeights::W8A8, true).kind == WeightSource::I8Qkv;
}

ConvWeights Net::upload_qkv_i8(const std::vector<std::string>& parts, const WeightPin& pin, int cin, int cout_each) {
  const size_t per = (size_t)cout_each * cin;
  std::vector<int8_t> q(parts.size() * per);
  std::vector<float> w_scale(parts.size() * cout_each);
  float act_absmax = 0.f;
  for (size_t i = 0; i < parts.size(); ++i) {
    const std::string wname = parts[i] + ".weight";
    const W8A8Mark* i8 = ws_->w8a8(wname);
    SD_REQUIRE(i8 && ws_->get(wname).numel() == per && i8->q.size() == per && i8->w_scale.size() == (size_t)cout_each, kInvalidArgument,
               "%s: expected %zu W8A8 values (%d,%d,1,1)", wname.c_str(), per, cout_each, cin);
    std::copy(i8->q.begin(), i8->q.end(), q.begin() + i * per);
    std::copy(i8->w_scale.begin(), i8->w_scale.end(), w_scale.begin() + i * cout_each);
    act_absmax = i8->act_absmax;   // (equal in all parts: qkv_plan)
  }
  auto up = [this](const auto* host, size_t n) {
    auto* d = ll_.arena.alloc_n<std::remove_cv_t<std::remove_pointer_t<decltype(host)>>>(n);
    SD_HIP(hipMemcpy(d, host, n * sizeof(*host), hipMemcpyHostToDevice));
    return d;
  };
  size_t bytes = 0;
  const CompressedWeights cw = upload_w8a8(up, pin.kind, (parts[0] + ".weight").c_str(), q.data(), w_scale.data(), act_absmax,
                                           (int)parts.size() * cout_each, cin, 1, &bytes);
  i8_applied_ += (int)parts.size();
  i8_bytes_ += bytes;
  for (const std::string& p : parts) i8_names_.push_back(p + ".weight"), holds_compressed(p + ".weight");
  return ConvWeights(cw, pin);
}

ConvWeights Net::upload_compressed(const std::string& name, const WeightPin& pin, int cin, const ConvArgs& a, const std::string& ln_name) {
  const std::string wname = name + ".weight";
  const size_t expect = (size_t)a.cout * cin * a.k * a.k;
  auto up = [this](const auto* host, size_t n) {
    auto* d = ll_.arena.alloc_n<std::remove_cv_t<std::remove_pointer_t<decltype(host)>>>(n);
    SD_HIP(hipMemcpy(d, host, n * sizeof(*host), hipMemcpyHostToDevice));
    return d;
  };
  size_t bytes = 0;
  CompressedWeights cw;
  if (pin.kind == WeightSource::I8Wstream || pin.kind == WeightSource::I8Halo || pin.kind == WeightSource::I8Gemm ||
      pin.kind == WeightSource::I8Geglu || pin.kind == WeightSource::I8GemmQ) {   // q in the kernel's layout, cs[n], inv_s: no fp16 copy
    const W8A8Mark* i8 = ws_->w8a8(wname);
    SD_REQUIRE(i8 && ws_->get(wname).numel() == expect && i8->q.size() == expect && i8->w_scale.size() == (size_t)a.cout, kInvalidArgument,
               "%s: expected %zu W8A8 values (%d,%d,%d,%d)", wname.c_str(), expect, a.cout, cin, a.k, a.k);
    cw = upload_w8a8(up, pin.kind, wname.c_str(), i8->q.data(), i8->w_scale.data(), i8->act_absmax, a.cout, cin, a.k, &bytes);
    ++i8_applied_;
    i8_bytes_ += bytes;
    i8_names_.push_back(wname);
  } else {
    const Palette* pal = ws_->palette(wname);
    SD_REQUIRE(pal && ws_->get(wname).numel() == expect && pal->indices.size() == expect, kInvalidArgument,
               "%s has %zu elements, expected %zu (%d,%d,%d,%d)", wname.c_str(), ws_->get(wname).numel(), expect, a.cout, cin, a.k, a.k);
    SD_REQUIRE(palette_bits_ok(pal->nbits) && pal->lut.size() == (size_t)1 << pal->nbits, kInternal, "%s: a palette of %zu entries for %d bits",
               wname.c_str(), pal->lut.size(), pal->nbits);
    cw = upload_palettized(up, pin.kind, wname.c_str(), reinterpret_cast<const half_t*>(pal->lut.data()), pal->nbits, pal->indices.data(), a.cout,
                           cin, a.k, &bytes);
    if (!ln_name.empty()) cw.ln_gamma = upload_vec(ln_name + ".weight", cin);
    ++pal_streamed_;
    pal_stream_bytes_ += bytes;
  }
  holds_compressed(wname);
  return ConvWeights(cw, pin);
}

int Net::activation_range(int index, std::string* name, float* absmax) {
  if (index < 0 || index >= (int)observed_.size()) return (int)observed_.size();
  SD_HIP(hipSetDevice(ll_.device));
  SD_HIP(hipStreamSynchronize(ll_.stream));
  SD_HIP(hipMemcpy(absmax, observed_[(size_t)index].second, sizeof(float), hipMemcpyDeviceToHost));
  if (observed_[(size_t)index].div != 1.f) *absmax /= observed_[(size_t)index].div;
  *name = observed_[(size_t)index].first;
  return (int)observed_.size();
}

// fp32 compute path (torch2coreml.py:570-578 converts an SDXL checkpoint's own VAE with FLOAT32 precision): the weights stay
// fp32 too - an fp32 checkpoint is not rounded to fp16 on the way in - in the [N][taps][Cin] layout of the fp16 path
Tensor Net::conv_f32(std::vector<Op>& ops, const std::string& name, const Tensor& x, const ConvArgs& a) {
  const int cout = a.cout, k = a.k;
  const float* b = a.bias ? upload_vec(name + ".bias", cout) : nullptr;
  SD_REQUIRE(!a.x2 && !a.temb && !a.ln_colsum && a.out_mode == kOutHalf && !a.silu_out, kInternal, "%s: not a VAE conv", name.c_str());
  const float* w = upload_conv_weight_f32(name, cout, x.C, k);
  const ConvGeom g = conv_geom(name, x, a);
  Tensor out = new_tensor(x.B, g.Ho, g.Wo, cout);
  ConvF32Desc fd;
  fd.x = x.f();
  fd.w = w;
  fd.w_kind = 1;
  fd.bias = b;
  fd.res = reinterpret_cast<const float*>(a.res);
  fd.out = out.f();
  fd.B = x.B; fd.Hi = x.H; fd.Wi = x.W; fd.Cin = x.C; fd.Ho = g.Ho; fd.Wo = g.Wo; fd.N = cout;
  fd.ksize = k; fd.stride = a.stride; fd.up = a.up; fd.pad = g.pad;
  ops.push_back([fd](hipStream_t s) { launch_conv_f32(fd, s); });
  char buf[256];
  snprintf(buf, sizeof(buf), "conv%dx%d fp32 %d->%d @%dx%d %s", k, k, x.C, cout, g.Ho, g.Wo, name.c_str());
  ops.back().label = buf;
  ops.back().flop = 2.0 * x.B * g.Ho * g.Wo * (double)cout * x.C * k * k;
  return out;
}

// the shape, sources and epilogue fields of a conv's descriptor: everything the planner looks at, no weights, no output
ConvDesc Net::conv_shape(const std::string& name, const Tensor& x, const ConvArgs& a) const {
  const Tensor* x2 = a.x2;
  const bool ln = a.ln_colsum != nullptr;
  ConvDesc d;
  d.x0 = x.p;
  d.C0 = x.C;
  if (x2) {
    SD_REQUIRE(x2->B == x.B && x2->H == x.H && x2->W == x.W, kInternal, "%s: concat shape mismatch", name.c_str());
    d.x1 = x2->p;
    d.C1 = x2->C;
  }
  d.temb = a.temb;
  d.temb_stride = kTembCap;
  d.res = a.res;
  d.B = x.B;
  d.Hi = x.H;
  d.Wi = x.W;
  const ConvGeom g = conv_geom(name, x, a);
  d.Ho = g.Ho;
  d.Wo = g.Wo;
  d.pad = g.pad;
  d.ksize = a.k;
  d.stride = a.stride;
  d.up = a.up;
  d.N = a.cout;
  d.out_mode = a.out_mode;
  d.ldT = a.ldT;
  d.ln_colsum = a.ln_colsum;
  d.x0_i8 = a.x_i8;
  if (ln || a.x_i8) {   // (the fused q|k|v launch, folded in fp16 or - plan tile 22 - reading norm1's int8 output)
    d.vt_perm = a.vt_perm ? 1 : 0;
    d.q_scale = a.q_scale;
    d.q_cols = a.q_cols;
  }
  return d;
}

Tensor Net::conv_w(std::vector<Op>& ops, const std::string& name, const ConvWeights& weights, const float* bias, const Tensor& x, const ConvArgs& a) {
  const Tensor* x2 = a.x2;
  const int cout = a.cout, k = a.k;
  const bool geglu = a.out_mode == kOutGeglu, ln = a.ln_colsum != nullptr;
  const half_t* w = weights.w;
  ConvDesc d = conv_shape(name, x, a);
  d.w = w;
  d.bias = bias;
  d.cw = weights.cw;   // a compressed source comes with its pin (all zero beside an fp16 matrix)
  d.tile = weights.pin.tile;
  d.staging = weights.pin.staging;
  d.splitk = weights.pin.splitk;
  d.subpix = weights.subpix;
  Tensor out;
  const bool qkv = (ln || a.x_i8) && a.n_trans > 0;
  if (qkv) {   // fused q|k|v: [M][n_trans] row-major + V^T [B][cout - n_trans][ldT]
    out = new_tensor(x.B, d.Ho, d.Wo, a.n_trans);
    *a.vt_out = ll_.arena.alloc_n<half_t>((size_t)x.B * (cout - a.n_trans) * a.ldT);
    d.out_t = *a.vt_out;
    d.n_trans = a.n_trans;
  } else if (a.out_mode == kOutHalfT) {
    out.B = x.B; out.H = 1; out.W = a.ldT; out.C = cout;   // [B][cout][ldT]
    out.p = ll_.arena.alloc_n<half_t>((size_t)x.B * cout * a.ldT);
  } else if (a.out_q8) {   // (plan tile 20 with an int8 output: the shape alone)
    SD_REQUIRE(geglu && d.cw.kind == WeightSource::I8Geglu && a.out_inv_s > 0.f, kInternal, "%s: an int8 output needs the int8 GEGLU kernel", name.c_str());
    out.B = x.B; out.H = d.Ho; out.W = d.Wo; out.C = cout / 2;
    d.out_q8 = a.out_q8;
    d.out_inv_s = a.out_inv_s;
  } else {
    out = new_tensor(x.B, d.Ho, d.Wo, geglu ? cout / 2 : cout);
  }
  d.out = out.p;
  SD_REQUIRE(!ln || (conv_fast_path_ok(d) && !a.silu_out), kInternal, "%s: LayerNorm fold / fused q|k|v off the MFMA path",
             name.c_str());
  // a GroupNorm built later over exactly this tensor may ask for its statistics from this op's epilogue (GnHook)
  std::shared_ptr<GnHook> hook;
  if (a.out_mode == kOutHalf && !qkv) {
    hook = std::make_shared<GnHook>();
    out.gn = hook;
    hook->ops_pos = (int)ops.size();
    hook->ops_list = &ops;
  }
  auto with_hook = [hook](const ConvDesc& d0) {
    ConvDesc dd = d0;
    if (hook) {
      dd.gn_partial = hook->partial;
      dd.gn_groups = hook->groups;
    }
    return dd;
  };
  const int cin = x.C + (x2 ? x2->C : 0);
  if (conv_fast_path_ok(d) && !a.silu_out) {
    // the pre-tiled (fragment-major) weight copies the plan of this conv reads: exactly what the planner names
    const ConvWeightCopies copies = d.cw.kind != WeightSource::Fp16 ? ConvWeightCopies{false, false, false} : conv_plan_copies(d);
    if (copies.wstream && !ln) {   // small-M layers: the weight-streaming kernel (plan tile 9; never a LayerNorm-fold / q|k|v op)
      half_t* wt = ll_.arena.alloc_n<half_t>(wstream_tiled_halves(cout, cin, k));
      derive(w, [=] { launch_wstream_retile(w, wt, cout, cin, k, ll_.stream); });
      d.w_tiled = wt;
    }
    if (copies.wsgemm) {    // widest-M GEGLU projection (K = 320): the weight-stationary kernel (wsgemm.hip, plan tile 10)
      half_t* wt = ll_.arena.alloc_n<half_t>(wsgemm_tiled_halves(cout));
      derive(w, [=] { launch_wsgemm_retile(w, wt, cout, geglu, ll_.stream); });
      d.w_ws = wt;
    }
    if (copies.bvgemm) {    // large-M 1x1 GEMMs: weights global -> VGPR (bvgemm.hip, plan tile 11)
      half_t* wt = ll_.arena.alloc_n<half_t>(bvgemm_tiled_halves(cout, x.C));
      const int c0 = x.C;
      derive(w, [=] { launch_bvgemm_retile(w, wt, cout, c0, geglu, ll_.stream); });
      d.w_bv = wt;
    }
    ll_.ws_need = std::max(ll_.ws_need, conv_workspace_bytes(d));
    ops.push_back([this, d, hook, with_hook](hipStream_t s) {
      const int n = launch_conv(with_hook(d), ll_.ws_conv, s);
      if (hook) hook->produced(n);
    });
  } else {
    const int so = a.silu_out ? 1 : 0;
    ops.push_back([d, so, hook, with_hook](hipStream_t s) {
      const int n = launch_conv_generic(with_hook(d), so, s);
      if (hook) hook->produced(n);
    });
  }
  char buf[320];
  // trailing "#kind,ksize,stride,up,Ctot,N,M" is the plan-table key of this op (tools/tune_plans.py)
  const int kind = d.out_t ? 3 : (geglu ? 2 : (ln ? 1 : 0));
  // the weight source in the label: "[+ln]+pal<bits>" from a palette (plan tile 14, 15 or 25), "geglu+pal<bits>[+ln]" for plan tile 16,
  // "+w8a8" from int8 weights and quantized activations (plan tiles 17 / 18 / 19 / 20 / 22 / 24), "+q8out+w8a8" where plan tile 20 writes
  // its product as int8
  const WeightSource src = d.cw.kind;
  const std::string lnmark = ln ? "+ln" : "", palmark = "+pal" + std::to_string(d.cw.bits);
  // "+subpix": the upsampler as four 2x2 phase convs (plan tile 21); flop below stays the algorithmic 9-tap count of the map it replaces
  const std::string mark = d.subpix ? "+subpix" : src == WeightSource::PalGeglu ? palmark + lnmark : lnmark + (d.cw.i8() ? (d.out_q8 ? "+q8out+w8a8" : "+w8a8") : src != WeightSource::Fp16 ? palmark : "");
  snprintf(buf, sizeof(buf), "%s%s %d->%d @%dx%d M=%d K=%d %s #%d,%d,%d,%d,%d,%d,%d",
           k == 3 ? "conv3x3" : (geglu ? (src == WeightSource::PalGeglu ? "geglu" : "geglu1x1") : "gemm1x1"), mark.c_str(), cin, cout, d.Ho, d.Wo,
           x.B * d.Ho * d.Wo, cin * k * k, name.c_str(), kind, k, a.stride, a.up, cin, cout, x.B * d.Ho * d.Wo);
  ops.back().label = buf;
  ops.back().flop = 2.0 * x.B * d.Ho * d.Wo * (double)cout * cin * k * k;
  return out;
}

void Net::conv_small_n(std::vector<Op>& ops, const std::string& name, const Tensor& x, int cout, half_t* out_nhwc, float* out_nchw) {
  if (f32_) {   // fp32 weights like every other conv of the handle (conv_f32): conv_out is not the one layer rounded to fp16
    ConvF32Desc fd;
    fd.x = x.f(); fd.w = upload_conv_weight_f32(name, cout, x.C, 3); fd.w_kind = 1; fd.bias = upload_vec(name + ".bias", cout);
    fd.out = out_nhwc ? reinterpret_cast<float*>(out_nhwc) : new_tensor(x.B, x.H, x.W, cout).f();
    fd.B = x.B; fd.Hi = x.H; fd.Wi = x.W; fd.Cin = x.C; fd.Ho = x.H; fd.Wo = x.W; fd.N = cout; fd.ksize = 3;
    ops.push_back([=](hipStream_t s) {
      launch_conv_f32(fd, s);
      if (out_nchw) launch_nhwc_to_nchw_f32f32(fd.out, out_nchw, fd.B, fd.N, fd.Ho, fd.Wo, s);
    });
  } else {
    ConvDesc d;
    d.x0 = x.p;
    d.C0 = x.C;
    d.w = upload_conv_weight(name, cout, x.C, 3, false);
    d.bias = upload_vec(name + ".bias", cout);
    d.out = out_nhwc;
    d.B = x.B; d.Hi = x.H; d.Wi = x.W; d.Ho = x.H; d.Wo = x.W;
    d.ksize = 3; d.stride = 1; d.up = 1; d.N = cout;
    ops.push_back([=](hipStream_t s) { launch_conv_small_n(d, out_nchw, s); });
  }
  ops.back().label = "conv3x3 small-N " + name + (out_nchw ? " -> fp32 NCHW" : "");
  ops.back().flop = 2.0 * x.M() * (double)cout * x.C * 9;
}

Tensor Net::group_norm_f32(std::vector<Op>& ops, const std::string& name, const Tensor& x, float eps, bool silu) {
  const int C = x.C, G = cfg_.norm_num_groups;
  void* scratch = ll_.arena.alloc(groupnorm_f32_scratch_bytes(x.B, G));
  const float* gamma = upload_vec(name + ".weight", C);
  const float* beta = upload_vec(name + ".bias", C);
  Tensor y = new_tensor(x.B, x.H, x.W, C);
  const float* xp = x.f();
  float* yp = y.f();
  const int B = x.B, HW = x.H * x.W, si = silu ? 1 : 0;
  ops.push_back([=](hipStream_t s) { launch_groupnorm_f32(xp, scratch, gamma, beta, yp, B, HW, C, G, eps, si, s); });
  ops.back().label = "groupnorm fp32 C=" + std::to_string(C) + " @" + std::to_string(x.H) + "x" + std::to_string(x.W) + " " + name;
  return y;
}

Tensor Net::group_norm(std::vector<Op>& ops, const std::string& name, const Tensor& x, const Tensor* x2, float eps,
                       bool silu, const ConvDesc* side, const std::string& side_label, double side_flop) {
  SD_REQUIRE(!side || !f32_, kInternal, "%s: side GEMM on the fp32 path", name.c_str());
  const int C = x.C + (x2 ? x2->C : 0);
  const int G = cfg_.norm_num_groups;
  SD_REQUIRE(C % G == 0, kUnsupported, "%s: %d channels not divisible by %d groups", name.c_str(), C, G);
  if (f32_) {
    SD_REQUIRE(!x2, kInternal, "%s: concat GroupNorm on the fp32 path", name.c_str());
    return group_norm_f32(ops, name, x, eps, silu);
  }
  const float* gamma = upload_vec(name + ".weight", C);
  const float* beta = upload_vec(name + ".bias", C);
  Tensor y = new_tensor(x.B, x.H, x.W, C);
  float* partial = ll_.arena.alloc_n<float>(groupnorm_scratch_floats(x.B, x.H * x.W, G));
  const half_t* p0 = x.p;
  const half_t* p1 = x2 ? x2->p : nullptr;
  const int C0 = x.C, C1 = x2 ? x2->C : 0, B = x.B, HW = x.H * x.W, si = silu ? 1 : 0;
  half_t* yp = y.p;
  // single-source GroupNorm that would need its own statistics launch: ask the op that produced x for them
  std::shared_ptr<GnHook> hook;
  if (!x2 && x.gn && !x.gn->partial && groupnorm_wants_producer_stats(HW, C, G)) {
    // (`entries` is handed over at launch time - the producer must run first, in the same launch list)
    SD_REQUIRE(x.gn->ops_list == &ops && x.gn->ops_pos >= 0 && x.gn->ops_pos < (int)ops.size(), kInternal,
               "%s: GroupNorm producer statistics need the producing op earlier in the same launch list", name.c_str());
    hook = x.gn;
    hook->partial = partial;
    hook->groups = G;
  }
  const std::string label = "groupnorm C=" + std::to_string(C) + " @" + std::to_string(x.H) + "x" + std::to_string(x.W) + " " + name;
  if (side) {
    const ConvDesc sd = *side;
    ops.push_back([=](hipStream_t s) {
      launch_groupnorm(p0, C0, p1, C1, partial, gamma, beta, yp, B, HW, G, eps, si, s, hook ? hook->consume() : 0, &sd);
    });
    ops.back().label = label + " || " + side_label;
    ops.back().flop = side_flop;
    return y;
  }
  ops.push_back([=](hipStream_t s) {
    launch_groupnorm(p0, C0, p1, C1, partial, gamma, beta, yp, B, HW, G, eps, si, s, hook ? hook->consume() : 0);
  });
  ops.back().label = label;
  return y;
}

// unet.py:470-489
Tensor Net::resnet(std::vector<Op>& ops, const std::string& p, const Tensor& x, const Tensor* x2, int cout, const float* temb) {
  const int cin = x.C + (x2 ? x2->C : 0);
  // conv_shortcut(x) does not depend on norm1 -> conv1 -> norm2: it rides in norm1's launch (one grid: the GroupNorm's blocks, then
  // the GEMM's tiles - igemm.hip gn_*_side_kernel) instead of a launch of its own.  SD_GN_SIDE=0 (with SD_TUNE): separate launches (A/B).
  static const int side_mode = tune_env_int("SD_GN_SIDE", 1);
  const half_t* side_out = nullptr;
  Tensor t0;
  if (cin != cout && side_mode != 0 && !f32_) {
    ConvDesc sd;
    sd.x0 = x.p;
    sd.C0 = x.C;
    if (x2) {
      sd.x1 = x2->p;
      sd.C1 = x2->C;
    }
    sd.B = x.B;
    sd.Hi = sd.Ho = x.H;
    sd.Wi = sd.Wo = x.W;
    sd.N = cout;
    if (gn_side_gemm_ok(sd)) {
      sd.w = upload_conv_weight(p + ".conv_shortcut", cout, cin, 1, false);
      sd.bias = upload_vec(p + ".conv_shortcut.bias", cout);
      Tensor sc = new_tensor(x.B, x.H, x.W, cout);
      sd.out = sc.p;
      side_out = sc.p;
      char buf[256];
      snprintf(buf, sizeof(buf), "gemm1x1 %d->%d @%dx%d M=%d K=%d %s.conv_shortcut", cin, cout, x.H, x.W, x.M(), cin, p.c_str());
      t0 = group_norm(ops, p + ".norm1", x, x2, cfg_.norm_eps, true, &sd, buf, 2.0 * x.M() * (double)cout * cin);
    }
  }
  if (!side_out) t0 = group_norm(ops, p + ".norm1", x, x2, cfg_.norm_eps, true);
  Tensor h = conv(ops, p + ".conv1", t0, {.cout = cout, .k = 3, .temb = temb});
  Tensor t1 = group_norm(ops, p + ".norm2", h, nullptr, cfg_.norm_eps, true);
  const half_t* shortcut;
  if (side_out) {
    shortcut = side_out;
  } else if (cin != cout) {
    shortcut = conv(ops, p + ".conv_shortcut", x, {.x2 = x2, .cout = cout}).p;
  } else {
    SD_REQUIRE(x2 == nullptr, kInternal, "%s: concat input with identity shortcut", p.c_str());
    shortcut = x.p;
  }
  return conv(ops, p + ".conv2", t1, {.cout = cout, .k = 3, .res = shortcut});
}

void Net::invalidate_graphs() {
  if (ll_.graph) { (void)hipGraphExecDestroy(ll_.graph); ll_.graph = nullptr; }
}

void Net::set_attention(int impl) {
  SD_REQUIRE(impl >= 0 && impl <= 2, kInvalidArgument, "attention impl %d", impl);
  if (impl != cfg_.attention_impl) {
    cfg_.attention_impl = impl;
    invalidate_graphs();
  }
}

void Net::run_ops_on(const std::vector<Op>& ops, hipStream_t s) {
  // SD_NAN_TRACE=1 (with SD_TUNE; eager launches only): after every op the whole arena is scanned for fp16 Inf / NaN patterns and the op
  // after which their number changes is named on stderr (fp32 regions give false positives - read the list with the op in mind).
  static const bool trace = tune_env_set("SD_NAN_TRACE");
  if (trace) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone) {
      unsigned long long* d = nullptr;
      SD_HIP(hipMalloc(&d, sizeof(unsigned long long)));
      auto scan = [&]() {
        SD_HIP(hipMemsetAsync(d, 0, sizeof(unsigned long long), s));
        const Arena& ar = ll_.arena;
        for (size_t i = 0; i < ar.chunks().size(); ++i) launch_count_nonfinite_half(ar.chunks()[i], ar.chunk_bytes()[i], d, s);
        unsigned long long h = 0;
        SD_HIP(hipMemcpyAsync(&h, d, sizeof(h), hipMemcpyDeviceToHost, s));
        SD_HIP(hipStreamSynchronize(s));
        return h;
      };
      unsigned long long last = scan();
      fprintf(stderr, "nan-trace: %llu non-finite fp16 patterns in the arena before the list\n", last);
      for (auto& op : ops) {
        op(s);
        const unsigned long long now = scan();
        if (now != last) fprintf(stderr, "nan-trace: %llu -> %llu after  %s\n", last, now, op.label.c_str());
        last = now;
      }
      (void)hipFree(d);
      return;
    }
  }
  static const bool poison = tune_env_set("SD_POISON_LDS");   // debug: NaN patterns into every CU's LDS in front of every op
  for (auto& op : ops) {
    if (poison) launch_lds_poison(s);
    op(s);
  }
}

void Net::run_forward() {
  if (!cfg_.use_graph) return run_eager();
  if (!ll_.graph) {
    // first run eagerly (sets kernel attributes, warms code objects), then capture
    run_eager();
    SD_HIP(hipStreamSynchronize(ll_.stream));
    ll_.graph = capture_graph(ll_.stream, [&] { run_eager(); });
  }
  SD_HIP(hipGraphLaunch(ll_.graph, ll_.stream));
}

float Net::time_forward(int warmup, int iters) {
  SD_HIP(hipSetDevice(ll_.device));
  SD_REQUIRE(have_inputs_, kInvalidArgument, "time_forward: call sd_unet_forward once first");
  SD_REQUIRE(iters >= 1, kInvalidArgument, "iters must be >= 1");
  for (int i = 0; i < warmup; ++i) run_forward();
  EventList ev(2);
  SD_HIP(hipEventRecord(ev[0], ll_.stream));
  for (int i = 0; i < iters; ++i) run_forward();
  SD_HIP(hipEventRecord(ev[1], ll_.stream));
  SD_HIP(hipEventSynchronize(ev[1]));
  float ms = 0.f;
  SD_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
  return ms / (float)iters;
}

std::vector<OpTime> Net::profile(int iters) {
  SD_HIP(hipSetDevice(ll_.device));
  SD_REQUIRE(have_inputs_, kInvalidArgument, "profile: call sd_unet_forward / sd_vae_decode once first");
  SD_REQUIRE(iters >= 1 && iters <= 100, kInvalidArgument, "iters must be in 1..100");
  hipStream_t stream = ll_.stream;
  std::vector<const Op*> seq;
  for (const auto* list : forward_lists())
    for (const Op& op : *list) seq.push_back(&op);
  const size_t n = seq.size();
  std::vector<std::vector<float>> t(n, std::vector<float>((size_t)iters));
  for (const Op* op : seq) (*op)(stream);   // warm (kernel attributes, code objects)
  SD_HIP(hipStreamSynchronize(stream));
  EventList ev(n + 1);
  for (int it = 0; it < iters; ++it) {
    SD_HIP(hipEventRecord(ev[0], stream));
    for (size_t i = 0; i < n; ++i) {
      (*seq[i])(stream);
      SD_HIP(hipEventRecord(ev[i + 1], stream));
    }
    SD_HIP(hipEventSynchronize(ev[n]));
    for (size_t i = 0; i < n; ++i) SD_HIP(hipEventElapsedTime(&t[i][(size_t)it], ev[i], ev[i + 1]));
  }
  std::vector<OpTime> out;
  for (size_t i = 0; i < n; ++i) {
    std::sort(t[i].begin(), t[i].end());
    out.push_back({seq[i]->label.empty() ? std::string("op") : seq[i]->label, seq[i]->flop, t[i][(size_t)iters / 2]});
  }
  return out;
}

}  // namespace sd
