// Safety checker (diffusers' StableDiffusionSafetyChecker: transformers' CLIPVisionModel ViT-L/14 + visual_projection + the
// concept head, as the reference converts and calls it: torch2coreml.py:1119-1309, pipeline.py:286-311, SafetyChecker.swift) as a
// static launch list of the gfx950 kernels:
//   patch rows gather -> patch-embedding GEMM -> class token + position embeddings -> pre_layrnorm ->
//   L x [LN1 -> q|k|v GEMM -> attention -> out_proj + residual -> LN2 -> fc1 -> activation -> fc2 + residual] ->
//   post_layernorm of the class rows -> visual_projection -> concept head.
// 8 L + 8 + B launches (201 for ViT-L/14 at batch 1; one more wherever the planner splits a GEMM's K), eager on the first call, one
// captured graph afterwards.  The GEMMs run over M = B * 257 ragged rows on whatever plan the conv / GEMM planner gives them.
#include <cmath>
#include <cstring>
#include <functional>

#include "../../include/sd_mi355x.h"
#include "capi_util.h"
#include "kernels.h"
#include "weights.h"

namespace sd {

class SafetyChecker {
 public:
  SafetyChecker(const sd_safety_checker_config& cfg, const WeightStore& ws, int device);
  ~SafetyChecker();
  void run(const void* clip_input, float adjustment, float* has_nsfw, float* concept_scores, float* image_embeds,
           float* last_hidden_state, int flags);
  size_t device_bytes() const { return arena_.bytes(); }
  float last_ms() const { return last_ms_; }

 private:
  // every tensor the handle reads, with the element count the config implies: checked on the host before any device work
  static std::string check_weights(const sd_safety_checker_config& cfg, const WeightStore& ws);
  half_t* upload_stacked(const WeightStore& ws, const std::vector<std::string>& names, int rows_each, int cols, int cols_padded = 0);
  half_t* upload_matrix(const WeightStore& ws, const std::string& name, int rows, int cols, int cols_padded = 0) {
    return upload_stacked(ws, {name}, rows, cols, cols_padded);
  }
  float* upload_vec(const WeightStore& ws, const std::vector<std::string>& names);
  void gemm(const half_t* x, const half_t* w, const float* bias, const half_t* res, half_t* out, int M, int N, int K);
  void launch_all();

  sd_safety_checker_config cfg_;
  int device_ = 0, S_ = 0;
  hipStream_t stream_ = nullptr;
  hipGraphExec_t graph_ = nullptr;
  hipEvent_t e0_ = nullptr, e1_ = nullptr;   // around the launch list of a run
  float last_ms_ = 0.f;
  Arena arena_;
  std::vector<std::function<void(hipStream_t)>> ops_;
  ConvWorkspace ws_conv_;
  size_t ws_need_ = 0;
  half_t* input_ = nullptr;       // clip_input (B, 3, I, I)
  float* adjustment_ = nullptr;   // one float: rewritten in front of every run, read by the head
  float* hidden_f32_ = nullptr;   // encoder output (B, S, D), before post_layernorm
  float* embeds_ = nullptr;       // (B, P)
  float* scores_ = nullptr;       // (B, num_concepts)
  float* flags_ = nullptr;        // (B)
};

namespace {
int patch_k(const sd_safety_checker_config& c) { return 3 * c.patch_size * c.patch_size; }
int patch_k_padded(const sd_safety_checker_config& c) { return (patch_k(c) + 63) / 64 * 64; }

void check_config(const sd_safety_checker_config& c) {
  SD_REQUIRE(c.batch >= 1 && c.image_size >= 1 && c.patch_size >= 1 && c.hidden_size >= 1 && c.intermediate_size >= 1 &&
                 c.num_hidden_layers >= 1 && c.num_attention_heads >= 1 && c.projection_dim >= 1 && c.num_concepts >= 1 &&
                 c.num_special >= 0,
             kInvalidArgument, "bad safety-checker config");
  SD_REQUIRE(c.image_size % c.patch_size == 0, kInvalidArgument, "safety checker: image size %d is no multiple of the patch size %d",
             c.image_size, c.patch_size);
  SD_REQUIRE(c.hidden_size % c.num_attention_heads == 0, kInvalidArgument, "safety checker: hidden size %d / %d heads", c.hidden_size,
             c.num_attention_heads);
  SD_REQUIRE(c.hidden_act == 0 || c.hidden_act == 1, kInvalidArgument, "hidden_act %d (0 quick_gelu, 1 gelu)", c.hidden_act);
  SD_REQUIRE(vit_attention_ok(c.hidden_size / c.num_attention_heads), kUnsupported, "safety checker: head dim %d (the attention kernel is built for 64)",
             c.hidden_size / c.num_attention_heads);
  SD_REQUIRE(c.hidden_size % 64 == 0 && c.hidden_size <= 2048 && c.intermediate_size % 64 == 0, kUnsupported,
             "safety checker: hidden %d / intermediate %d off the GEMM / LayerNorm path", c.hidden_size, c.intermediate_size);
}
}  // namespace

std::string SafetyChecker::check_weights(const sd_safety_checker_config& c, const WeightStore& ws) {
  const std::string vm = ws.has("vision_model.vision_model.embeddings.class_embedding") ? "vision_model.vision_model." : "vision_model.";
  const size_t D = c.hidden_size, I = c.intermediate_size, P = c.projection_dim;
  const size_t S = (size_t)(c.image_size / c.patch_size) * (c.image_size / c.patch_size) + 1;
  auto need = [&](const std::string& name, size_t numel) {
    const HostTensor& t = ws.get(name);   // kNotFound
    SD_REQUIRE(t.numel() == numel, kInvalidArgument, "%s has %zu elements, the config implies %zu", name.c_str(), t.numel(), numel);
  };
  need(vm + "embeddings.class_embedding", D);
  need(vm + "embeddings.patch_embedding.weight", D * patch_k(c));
  need(vm + "embeddings.position_embedding.weight", S * D);
  for (const char* ln : {"pre_layrnorm", "post_layernorm"})
    for (const char* wb : {".weight", ".bias"}) need(vm + ln + wb, D);
  for (int l = 0; l < c.num_hidden_layers; ++l) {
    const std::string p = vm + "encoder.layers." + std::to_string(l);
    for (const char* ln : {".layer_norm1", ".layer_norm2"})
      for (const char* wb : {".weight", ".bias"}) need(p + ln + wb, D);
    for (const char* pr : {".self_attn.q_proj", ".self_attn.k_proj", ".self_attn.v_proj", ".self_attn.out_proj"}) {
      need(p + pr + ".weight", D * D);
      need(p + pr + ".bias", D);
    }
    need(p + ".mlp.fc1.weight", I * D);
    need(p + ".mlp.fc1.bias", I);
    need(p + ".mlp.fc2.weight", D * I);
    need(p + ".mlp.fc2.bias", D);
  }
  need("visual_projection.weight", P * D);
  need("concept_embeds", (size_t)c.num_concepts * P);
  need("concept_embeds_weights", c.num_concepts);
  if (c.num_special > 0) {
    need("special_care_embeds", (size_t)c.num_special * P);
    need("special_care_embeds_weights", c.num_special);
  }
  return vm;
}

SafetyChecker::SafetyChecker(const sd_safety_checker_config& cfg, const WeightStore& ws, int device) : cfg_(cfg), device_(device) {
  check_config(cfg);
  const std::string vm = check_weights(cfg, ws);
  const int B = cfg.batch, D = cfg.hidden_size, L = cfg.num_hidden_layers, H = cfg.num_attention_heads, I = cfg.intermediate_size;
  const int P = cfg.projection_dim, G = cfg.image_size / cfg.patch_size, NP = G * G, S = NP + 1, M = B * S;
  const int K0 = patch_k(cfg), Kp = patch_k_padded(cfg);
  S_ = S;
  int ndev = 0;
  const hipError_t dev_err = hipGetDeviceCount(&ndev);
  SD_REQUIRE(dev_err == hipSuccess && ndev > 0, kHipError, "no HIP device visible (%s): libsdmi355 has no CPU fallback",
             hipGetErrorString(dev_err));
  SD_REQUIRE(device >= 0 && device < ndev, kInvalidArgument, "device %d out of range (%d visible)", device, ndev);
  SD_HIP(hipSetDevice(device));
  SD_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
  SD_HIP(hipEventCreate(&e0_));
  SD_HIP(hipEventCreate(&e1_));
  device_zero_chunk();   // the GEMM launches only read it (never first allocated under graph capture)
  const float eps = cfg.layer_norm_eps > 0 ? cfg.layer_norm_eps : 1e-5f;

  // embeddings: patch conv (no bias) as a GEMM over gathered rows, K zero-padded 3 p p -> Kp on both sides
  input_ = arena_.alloc_n<half_t>((size_t)B * 3 * cfg.image_size * cfg.image_size);
  adjustment_ = arena_.alloc_n<float>(1);
  half_t* wpatch = upload_matrix(ws, vm + "embeddings.patch_embedding.weight", D, K0, Kp);
  half_t* cls = upload_matrix(ws, vm + "embeddings.class_embedding", 1, D);
  half_t* pos = upload_matrix(ws, vm + "embeddings.position_embedding.weight", S, D);
  half_t* rows = arena_.alloc_n<half_t>((size_t)B * NP * Kp);
  half_t* patches = arena_.alloc_n<half_t>((size_t)B * NP * D);
  {
    const half_t* in = input_;
    const int img = cfg.image_size, ps = cfg.patch_size;
    ops_.push_back([=](hipStream_t s) { launch_vit_patch_rows(in, rows, B, img, ps, Kp, s); });
  }
  gemm(rows, wpatch, nullptr, nullptr, patches, B * NP, D, Kp);
  half_t* x0 = arena_.alloc_n<half_t>((size_t)M * D);
  ops_.push_back([=](hipStream_t s) { launch_vit_tokens(patches, cls, pos, x0, B, S, D, s); });
  half_t* x = arena_.alloc_n<half_t>((size_t)M * D);
  {
    const float* g = upload_vec(ws, {vm + "pre_layrnorm.weight"});
    const float* b = upload_vec(ws, {vm + "pre_layrnorm.bias"});
    half_t* y = x;
    ops_.push_back([=](hipStream_t s) { launch_layernorm(x0, g, b, y, M, D, eps, s); });
  }
  for (int l = 0; l < L; ++l) {
    const std::string p = vm + "encoder.layers." + std::to_string(l);
    const float* g1 = upload_vec(ws, {p + ".layer_norm1.weight"});
    const float* b1 = upload_vec(ws, {p + ".layer_norm1.bias"});
    half_t* n1 = arena_.alloc_n<half_t>((size_t)M * D);
    {
      const half_t* xi = x;
      ops_.push_back([=](hipStream_t s) { launch_layernorm(xi, g1, b1, n1, M, D, eps, s); });
    }
    // one stacked q|k|v projection; the attention kernel reads its rows as they are and applies d^-0.5 to the scores
    half_t* wqkv = upload_stacked(ws, {p + ".self_attn.q_proj.weight", p + ".self_attn.k_proj.weight", p + ".self_attn.v_proj.weight"}, D, D);
    float* bqkv = upload_vec(ws, {p + ".self_attn.q_proj.bias", p + ".self_attn.k_proj.bias", p + ".self_attn.v_proj.bias"});
    half_t* qkv = arena_.alloc_n<half_t>((size_t)M * 3 * D);
    gemm(n1, wqkv, bqkv, nullptr, qkv, M, 3 * D, D);
    half_t* att = arena_.alloc_n<half_t>((size_t)M * D);
    ops_.push_back([=](hipStream_t s) { launch_vit_attention(qkv, att, B, S, H, D / H, s); });
    half_t* wo = upload_matrix(ws, p + ".self_attn.out_proj.weight", D, D);
    float* bo = upload_vec(ws, {p + ".self_attn.out_proj.bias"});
    half_t* x1 = arena_.alloc_n<half_t>((size_t)M * D);
    gemm(att, wo, bo, x, x1, M, D, D);   // + residual
    const float* g2 = upload_vec(ws, {p + ".layer_norm2.weight"});
    const float* b2 = upload_vec(ws, {p + ".layer_norm2.bias"});
    half_t* n2 = arena_.alloc_n<half_t>((size_t)M * D);
    ops_.push_back([=](hipStream_t s) { launch_layernorm(x1, g2, b2, n2, M, D, eps, s); });
    half_t* w1 = upload_matrix(ws, p + ".mlp.fc1.weight", I, D);
    float* bb1 = upload_vec(ws, {p + ".mlp.fc1.bias"});
    half_t* hmid = arena_.alloc_n<half_t>((size_t)M * I);
    gemm(n2, w1, bb1, nullptr, hmid, M, I, D);
    const int act = cfg.hidden_act;
    ops_.push_back([=](hipStream_t s) { launch_clip_act(hmid, (size_t)M * I, act, s); });
    half_t* w2 = upload_matrix(ws, p + ".mlp.fc2.weight", D, I);
    float* bb2 = upload_vec(ws, {p + ".mlp.fc2.bias"});
    half_t* x2 = arena_.alloc_n<half_t>((size_t)M * D);
    gemm(hmid, w2, bb2, x1, x2, M, D, I);   // + residual
    x = x2;
  }
  // pooled = post_layernorm(class rows); image_embeds = visual_projection(pooled) (no bias); then the concept head
  SD_REQUIRE(D % 8 == 0 && D <= 3072, kUnsupported, "visual_projection: hidden size %d", D);
  {
    const float* gp = upload_vec(ws, {vm + "post_layernorm.weight"});
    const float* bp = upload_vec(ws, {vm + "post_layernorm.bias"});
    half_t* wproj = upload_matrix(ws, "visual_projection.weight", P, D);
    const int NC = cfg.num_concepts, NS = cfg.num_special;
    const float* ce = upload_vec(ws, {"concept_embeds"});
    const float* cw = upload_vec(ws, {"concept_embeds_weights"});
    const float* se = NS ? upload_vec(ws, {"special_care_embeds"}) : nullptr;
    const float* sw = NS ? upload_vec(ws, {"special_care_embeds_weights"}) : nullptr;
    half_t* pooled = arena_.alloc_n<half_t>((size_t)B * D);
    float* pooled32 = arena_.alloc_n<float>((size_t)B * D);
    hidden_f32_ = arena_.alloc_n<float>((size_t)M * D);
    embeds_ = arena_.alloc_n<float>((size_t)B * P);
    scores_ = arena_.alloc_n<float>((size_t)B * NC);
    flags_ = arena_.alloc_n<float>(B);
    const half_t* xl = x;
    float* h32 = hidden_f32_;
    float* emb = embeds_;
    float* sco = scores_;
    float* flg = flags_;
    const float* adj = adjustment_;
    ops_.push_back([=](hipStream_t s) {
      launch_half_to_float(xl, h32, (size_t)M * D, s);
      for (int b = 0; b < B; ++b) launch_layernorm(xl + (size_t)b * S * D, gp, bp, pooled + (size_t)b * D, 1, D, eps, s);
      launch_half_to_float(pooled, pooled32, (size_t)B * D, s);
      launch_gemv(wproj, nullptr, pooled32, D, emb, P, B, P, D, 0, 0, 0, s);
      launch_safety_head(emb, ce, se, cw, sw, adj, B, P, NC, NS, flg, sco, s);
    });
  }
  if (ws_need_ > 0) {
    ws_conv_.partial = reinterpret_cast<float*>(arena_.alloc(ws_need_));
    ws_conv_.partial_bytes = ws_need_;
  }
  SD_HIP(hipStreamSynchronize(stream_));
}

SafetyChecker::~SafetyChecker() {
  (void)hipSetDevice(device_);
  if (graph_) (void)hipGraphExecDestroy(graph_);
  if (stream_) {
    (void)hipStreamSynchronize(stream_);
    (void)hipStreamDestroy(stream_);
  }
  if (e0_) (void)hipEventDestroy(e0_);
  if (e1_) (void)hipEventDestroy(e1_);
}

// rows of `cols` checkpoint values, stored with `cols_padded` (>= cols, zeros behind) halves per row
half_t* SafetyChecker::upload_stacked(const WeightStore& ws, const std::vector<std::string>& names, int rows_each, int cols, int cols_padded) {
  const size_t ldw = cols_padded ? cols_padded : cols;
  std::vector<half_t> host(names.size() * rows_each * ldw, (half_t)0);
  for (size_t i = 0; i < names.size(); ++i) {
    const HostTensor& t = ws.get(names[i]);
    SD_REQUIRE(t.numel() == (size_t)rows_each * cols, kInvalidArgument, "%s has %zu elements, expected %d x %d", names[i].c_str(),
               t.numel(), rows_each, cols);
    for (int r = 0; r < rows_each; ++r)
      for (int c = 0; c < cols; ++c) host[(i * rows_each + r) * ldw + c] = (half_t)t.data[(size_t)r * cols + c];
  }
  half_t* d = arena_.alloc_n<half_t>(host.size());
  SD_HIP(hipMemcpy(d, host.data(), host.size() * sizeof(half_t), hipMemcpyHostToDevice));
  return d;
}

float* SafetyChecker::upload_vec(const WeightStore& ws, const std::vector<std::string>& names) {
  std::vector<float> host;
  for (const auto& n : names) {
    const HostTensor& t = ws.get(n);
    host.insert(host.end(), t.data.begin(), t.data.end());
  }
  float* d = arena_.alloc_n<float>(host.size());
  SD_HIP(hipMemcpy(d, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
  return d;
}

// out[M][N] = x[M][K] . w[N][K]^T + bias (+ res): the UNet's 1x1 implicit-GEMM path over M ragged rows, as TextEncoder::gemm
void SafetyChecker::gemm(const half_t* x, const half_t* w, const float* bias, const half_t* res, half_t* out, int M, int N, int K) {
  ConvDesc d;
  d.x0 = x;
  d.C0 = K;
  d.w = w;
  d.bias = bias;
  d.res = res;
  d.out = out;
  d.B = 1;
  d.Hi = 1;
  d.Wi = M;
  d.Ho = 1;
  d.Wo = M;
  d.N = N;
  SD_REQUIRE(conv_fast_path_ok(d), kUnsupported, "safety checker GEMM %d x %d not MFMA-tileable", N, K);
  ws_need_ = std::max(ws_need_, conv_workspace_bytes(d));
  ops_.push_back([this, d](hipStream_t s) { launch_conv(d, ws_conv_, s); });
}

void SafetyChecker::launch_all() {
  for (auto& op : ops_) op(stream_);
}

void SafetyChecker::run(const void* clip_input, float adjustment, float* has_nsfw, float* concept_scores, float* image_embeds,
                        float* last_hidden_state, int flags) {
  SD_HIP(hipSetDevice(device_));
  SD_REQUIRE(clip_input != nullptr, kInvalidArgument, "missing input 'clip_input'");
  SD_REQUIRE((flags & ~SD_FLAG_DEVICE_PTRS) == 0, kInvalidArgument, "unknown flags %d", flags);
  const int B = cfg_.batch, D = cfg_.hidden_size;
  const size_t in_bytes = (size_t)B * 3 * cfg_.image_size * cfg_.image_size * sizeof(half_t);
  SD_HIP(hipMemcpyAsync(input_, clip_input, in_bytes, (flags & SD_FLAG_DEVICE_PTRS) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                        stream_));
  SD_HIP(hipMemcpyAsync(adjustment_, &adjustment, sizeof(float), hipMemcpyHostToDevice, stream_));
  SD_HIP(hipStreamSynchronize(stream_));   // `adjustment` lives on this frame
  if (cfg_.use_graph) {
    if (!graph_) {
      launch_all();   // eager first: kernel attributes, code objects
      SD_HIP(hipStreamSynchronize(stream_));
      SD_HIP(hipStreamBeginCapture(stream_, hipStreamCaptureModeThreadLocal));
      hipGraph_t g = nullptr;
      try {
        launch_all();
      } catch (...) {
        (void)hipStreamEndCapture(stream_, &g);
        if (g) (void)hipGraphDestroy(g);
        throw;
      }
      SD_HIP(hipStreamEndCapture(stream_, &g));
      const hipError_t e = hipGraphInstantiate(&graph_, g, nullptr, nullptr, 0);
      (void)hipGraphDestroy(g);
      SD_REQUIRE(e == hipSuccess, kHipError, "hipGraphInstantiate failed: %s", hipGetErrorString(e));
    }
    SD_HIP(hipEventRecord(e0_, stream_));
    SD_HIP(hipGraphLaunch(graph_, stream_));
  } else {
    SD_HIP(hipEventRecord(e0_, stream_));
    launch_all();
  }
  SD_HIP(hipEventRecord(e1_, stream_));
  if (has_nsfw) SD_HIP(hipMemcpyAsync(has_nsfw, flags_, (size_t)B * sizeof(float), hipMemcpyDeviceToHost, stream_));
  if (concept_scores)
    SD_HIP(hipMemcpyAsync(concept_scores, scores_, (size_t)B * cfg_.num_concepts * sizeof(float), hipMemcpyDeviceToHost, stream_));
  if (image_embeds)
    SD_HIP(hipMemcpyAsync(image_embeds, embeds_, (size_t)B * cfg_.projection_dim * sizeof(float), hipMemcpyDeviceToHost, stream_));
  if (last_hidden_state)
    SD_HIP(hipMemcpyAsync(last_hidden_state, hidden_f32_, (size_t)B * S_ * D * sizeof(float), hipMemcpyDeviceToHost, stream_));
  SD_HIP(hipStreamSynchronize(stream_));
  SD_HIP(hipEventElapsedTime(&last_ms_, e0_, e1_));
}

}  // namespace sd

struct sd_safety_checker {
  std::unique_ptr<sd::SafetyChecker> impl;
};

extern "C" {

int sd_safety_checker_create(const sd_safety_checker_config* cfg, const sd_weights* w, int device, sd_safety_checker** out) {
  return sd::guarded([&] {
    SD_REQUIRE(cfg && w && out, sd::kInvalidArgument, "NULL argument");
    auto h = std::make_unique<sd_safety_checker>();
    h->impl = std::make_unique<sd::SafetyChecker>(*cfg, w->store, device);
    *out = h.release();
  });
}
void sd_safety_checker_destroy(sd_safety_checker* c) { delete c; }
size_t sd_safety_checker_device_bytes(const sd_safety_checker* c) { return c ? c->impl->device_bytes() : 0; }
float sd_safety_checker_last_ms(const sd_safety_checker* c) { return c ? c->impl->last_ms() : 0.f; }
int sd_safety_checker_run(sd_safety_checker* c, const void* clip_input, float adjustment, float* has_nsfw, float* concept_scores,
                          float* image_embeds, float* last_hidden_state, int flags) {
  return sd::guarded([&] {
    SD_REQUIRE(c && clip_input, sd::kInvalidArgument, "NULL argument");
    c->impl->run(clip_input, adjustment, has_nsfw, concept_scores, image_embeds, last_hidden_state, flags);
  });
}

}  // extern "C"
