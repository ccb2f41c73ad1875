// Safety checker (diffusers' StableDiffusionSafetyChecker: transformers' CLIPVisionModel ViT-L/14 + visual_projection + the
// concept head, as the reference converts and calls it: torch2coreml.py:1119-1309, pipeline.py:286-311, SafetyChecker.swift) as a
// static launch list of the gfx950 kernels:
//   patch rows gather -> patch-embedding GEMM -> class token + position embeddings -> pre_layrnorm ->
//   L x [LN1 -> q|k|v GEMM -> attention -> out_proj + residual -> LN2 -> fc1 -> activation -> fc2 + residual] ->
//   post_layernorm of the class rows -> visual_projection -> concept head.
// 8 L + 8 + B launches (201 for ViT-L/14 at batch 1; one more wherever the planner splits a GEMM's K), eager on the first call, one
// captured graph afterwards.  The GEMMs run over M = B * 257 ragged rows on whatever plan the conv / GEMM planner gives them.
// The handle is a LaunchList (launch_list.h); the layers are build_clip_stack's (clip_encoder.cpp).  What is this file's: the config
// checks, the patch embedding, the head op, the event pair behind last_ms and the copies out.
#include <cmath>
#include <cstring>

#include "capi_util.h"
#include "safety_checker.h"

namespace sd {

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

SafetyChecker::SafetyChecker(const sd_safety_checker_config& cfg, const WeightStore& ws, int device) : cfg_(cfg) {
  check_config(cfg);
  const int B = cfg.batch, D = cfg.hidden_size, L = cfg.num_hidden_layers, H = cfg.num_attention_heads, I = cfg.intermediate_size;
  const int P = cfg.projection_dim, G = cfg.image_size / cfg.patch_size, NP = G * G, S = NP + 1, M = B * S;
  const int K0 = patch_k(cfg), Kp = patch_k_padded(cfg), NC = cfg.num_concepts, NS = cfg.num_special;
  S_ = S;
  const std::string vm = ws.has("vision_model.vision_model.embeddings.class_embedding") ? "vision_model.vision_model." : "vision_model.";
  ClipStack stack;
  stack.prefix = vm + "encoder.layers.";
  stack.L = L, stack.M = M, stack.D = D, stack.I = I, stack.act = cfg.hidden_act;
  stack.eps = cfg.layer_norm_eps > 0 ? cfg.layer_norm_eps : 1e-5f;
  stack.what = "safety checker";
  // every tensor the handle reads, with the element count the config implies: checked on the host before any device work
  check_numel(ws, vm + "embeddings.class_embedding", D);
  check_numel(ws, vm + "embeddings.patch_embedding.weight", (size_t)D * K0);
  check_numel(ws, vm + "embeddings.position_embedding.weight", (size_t)S * D);
  for (const char* ln : {"pre_layrnorm", "post_layernorm"})
    for (const char* wb : {".weight", ".bias"}) check_numel(ws, vm + ln + wb, D);
  check_clip_stack_weights(ws, stack);
  check_numel(ws, "visual_projection.weight", (size_t)P * D);
  check_numel(ws, "concept_embeds", (size_t)NC * P);
  check_numel(ws, "concept_embeds_weights", NC);
  if (NS > 0) {
    check_numel(ws, "special_care_embeds", (size_t)NS * P);
    check_numel(ws, "special_care_embeds_weights", NS);
  }
  open(device);
  SD_HIP(hipEventCreate(&e0_));
  SD_HIP(hipEventCreate(&e1_));
  const float eps = stack.eps;

  // embeddings: patch conv (no bias) as a GEMM over gathered rows, K zero-padded 3 p p -> Kp on both sides
  input_ = arena.alloc_n<half_t>((size_t)B * 3 * cfg.image_size * cfg.image_size);
  adjustment_ = arena.alloc_n<float>(1);
  half_t* wpatch = upload_rows(ws, {vm + "embeddings.patch_embedding.weight"}, D, K0, Kp);
  half_t* cls = upload_rows(ws, {vm + "embeddings.class_embedding"}, 1, D);
  half_t* pos = upload_rows(ws, {vm + "embeddings.position_embedding.weight"}, S, D);
  half_t* rows = arena.alloc_n<half_t>((size_t)B * NP * Kp);
  half_t* patches = arena.alloc_n<half_t>((size_t)B * NP * D);
  {
    const half_t* in = input_;
    const int img = cfg.image_size, ps = cfg.patch_size;
    push([=](hipStream_t s) { launch_vit_patch_rows(in, rows, B, img, ps, Kp, s); });
  }
  gemm(rows, wpatch, nullptr, nullptr, patches, B * NP, D, Kp, stack.what);
  half_t* x0 = arena.alloc_n<half_t>((size_t)M * D);
  push([=](hipStream_t s) { launch_vit_tokens(patches, cls, pos, x0, B, S, D, s); });
  half_t* x = arena.alloc_n<half_t>((size_t)M * D);
  {
    const float* g = upload_vec(ws, {vm + "pre_layrnorm.weight"}, D);
    const float* b = upload_vec(ws, {vm + "pre_layrnorm.bias"}, D);
    half_t* y = x;
    push([=](hipStream_t s) { launch_layernorm(x0, g, b, y, M, D, eps, s); });
  }
  const half_t* xl = build_clip_stack(*this, ws, stack, x, [=](const half_t* qkv, half_t* att, hipStream_t s) {
    launch_vit_attention(qkv, att, B, S, H, D / H, s);
  });
  // pooled = post_layernorm(class rows); image_embeds = visual_projection(pooled) (no bias); then the concept head
  SD_REQUIRE(D % 8 == 0 && D <= 3072, kUnsupported, "visual_projection: hidden size %d", D);
  {
    const float* gp = upload_vec(ws, {vm + "post_layernorm.weight"}, D);
    const float* bp = upload_vec(ws, {vm + "post_layernorm.bias"}, D);
    half_t* wproj = upload_rows(ws, {"visual_projection.weight"}, P, D);
    const float* ce = upload_vec(ws, {"concept_embeds"}, (size_t)NC * P);
    const float* cw = upload_vec(ws, {"concept_embeds_weights"}, NC);
    const float* se = NS ? upload_vec(ws, {"special_care_embeds"}, (size_t)NS * P) : nullptr;
    const float* sw = NS ? upload_vec(ws, {"special_care_embeds_weights"}, NS) : nullptr;
    half_t* pooled = arena.alloc_n<half_t>((size_t)B * D);
    float* pooled32 = arena.alloc_n<float>((size_t)B * D);
    hidden_f32_ = arena.alloc_n<float>((size_t)M * D);
    embeds_ = arena.alloc_n<float>((size_t)B * P);
    scores_ = arena.alloc_n<float>((size_t)B * NC);
    flags_ = arena.alloc_n<float>(B);
    float* h32 = hidden_f32_;
    float* emb = embeds_;
    float* sco = scores_;
    float* flg = flags_;
    const float* adj = adjustment_;
    push([=](hipStream_t s) {
      launch_half_to_float(xl, h32, (size_t)M * D, s);
      for (int b = 0; b < B; ++b) launch_layernorm(xl + (size_t)b * S * D, gp, bp, pooled + (size_t)b * D, 1, D, eps, s);
      launch_half_to_float(pooled, pooled32, (size_t)B * D, s);
      launch_gemv(wproj, nullptr, pooled32, D, emb, P, B, P, D, 0, 0, 0, s);
      launch_safety_head(emb, ce, se, cw, sw, adj, B, P, NC, NS, flg, sco, s);
    });
  }
  seal();
}

SafetyChecker::~SafetyChecker() {
  close();
  if (e0_) (void)hipEventDestroy(e0_);
  if (e1_) (void)hipEventDestroy(e1_);
}

void SafetyChecker::run(const void* clip_input, float adjustment, float* has_nsfw, float* concept_scores, float* image_embeds,
                        float* last_hidden_state, int flags) {
  SD_HIP(hipSetDevice(device));
  SD_REQUIRE(clip_input != nullptr, kInvalidArgument, "missing input 'clip_input'");
  SD_REQUIRE((flags & ~SD_FLAG_DEVICE_PTRS) == 0, kInvalidArgument, "unknown flags %d", flags);
  const int B = cfg_.batch, D = cfg_.hidden_size;
  const size_t in_bytes = (size_t)B * 3 * cfg_.image_size * cfg_.image_size * sizeof(half_t);
  SD_HIP(hipMemcpyAsync(input_, clip_input, in_bytes, (flags & SD_FLAG_DEVICE_PTRS) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                        stream));
  SD_HIP(hipMemcpyAsync(adjustment_, &adjustment, sizeof(float), hipMemcpyHostToDevice, stream));
  SD_HIP(hipStreamSynchronize(stream));   // `adjustment` lives on this frame
  launch(cfg_.use_graph != 0, e0_);
  SD_HIP(hipEventRecord(e1_, stream));
  if (has_nsfw) SD_HIP(hipMemcpyAsync(has_nsfw, flags_, (size_t)B * sizeof(float), hipMemcpyDeviceToHost, stream));
  if (concept_scores)
    SD_HIP(hipMemcpyAsync(concept_scores, scores_, (size_t)B * cfg_.num_concepts * sizeof(float), hipMemcpyDeviceToHost, stream));
  if (image_embeds)
    SD_HIP(hipMemcpyAsync(image_embeds, embeds_, (size_t)B * cfg_.projection_dim * sizeof(float), hipMemcpyDeviceToHost, stream));
  if (last_hidden_state)
    SD_HIP(hipMemcpyAsync(last_hidden_state, hidden_f32_, (size_t)B * S_ * D * sizeof(float), hipMemcpyDeviceToHost, stream));
  SD_HIP(hipStreamSynchronize(stream));
  SD_HIP(hipEventElapsedTime(&last_ms_, e0_, e1_));
}

}  // namespace sd

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
