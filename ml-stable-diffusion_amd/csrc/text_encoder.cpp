// CLIP text encoder (transformers CLIPTextModel / CLIPTextModelWithProjection as the reference wraps
// them, torch2coreml.py:379-441; call site pipeline.py:151-175) as a static launch list of the gfx950
// kernels: embedding gather -> L x [LN1 -> q|k|v GEMM -> causal attention -> out_proj + residual ->
// LN2 -> fc1 -> activation -> fc2 + residual] -> final LN -> pooled row [-> text_projection].
// One prompt (1 x 77 tokens) per call like the converted Core ML model; runs once per prompt, not per step.
// The handle is a LaunchList (launch_list.h); the layers are build_clip_stack's (clip_encoder.cpp).  What is this file's: the config
// checks, the embedding gather, the final LayerNorm + fp32 copies, the pooled row / text_projection and the copies out.
#include <cmath>
#include <cstring>

#include "../../include/sd_mi355x.h"
#include "capi_util.h"
#include "clip_encoder.h"

namespace sd {

class TextEncoder : LaunchList {
 public:
  TextEncoder(const sd_text_encoder_config& cfg, const WeightStore& ws, int device);
  void encode(const int32_t* input_ids, int eos_index, float* last_hidden_state, float* hidden_embeds, float* pooled);
  size_t device_bytes() const { return arena.bytes(); }

 private:
  sd_text_encoder_config cfg_;
  int* ids_ = nullptr;
  float* final_f32_ = nullptr;    // final_layer_norm(last hidden)       [S][D]
  float* penult_f32_ = nullptr;   // hidden_states[-2]                   [S][D]
  float* pooled_ = nullptr;
  half_t* proj_w_ = nullptr;
};

TextEncoder::TextEncoder(const sd_text_encoder_config& cfg, const WeightStore& ws, int device) : cfg_(cfg) {
  const int D = cfg.hidden_size, S = cfg.max_position_embeddings, L = cfg.num_hidden_layers, H = cfg.num_attention_heads;
  const int I = cfg.intermediate_size;
  SD_REQUIRE(D > 0 && S > 0 && L >= 1 && H > 0 && I > 0 && cfg.vocab_size > 0, kInvalidArgument, "bad text-encoder config");
  SD_REQUIRE(D % 64 == 0 && I % 64 == 0 && D % H == 0, kUnsupported, "text encoder: hidden %d / intermediate %d / heads %d", D,
             I, H);
  SD_REQUIRE(cfg.hidden_act == 0 || cfg.hidden_act == 1, kUnsupported, "hidden_act %d (0 quick_gelu, 1 gelu)", cfg.hidden_act);
  const std::string tm = ws.has("text_model.embeddings.token_embedding.weight") ? "text_model." : "";
  ClipStack stack;
  stack.prefix = tm + "encoder.layers.";
  stack.L = L, stack.M = S, stack.D = D, stack.I = I, stack.act = cfg.hidden_act;
  stack.eps = cfg.layer_norm_eps > 0 ? cfg.layer_norm_eps : 1e-5f;
  stack.what = "text encoder";
  check_clip_stack_weights(ws, stack);
  open(device);
  const float eps = stack.eps;
  half_t* tok = upload_rows(ws, {tm + "embeddings.token_embedding.weight"}, cfg.vocab_size, D);
  half_t* pos = upload_rows(ws, {tm + "embeddings.position_embedding.weight"}, S, D);
  ids_ = arena.alloc_n<int>(S);
  half_t* x = arena.alloc_n<half_t>((size_t)S * D);
  {
    int* ids = ids_;
    const int vocab = cfg.vocab_size;
    push([=](hipStream_t s) { launch_clip_embed(ids, tok, pos, x, S, D, vocab, s); });
  }
  half_t* pen = nullptr;   // hidden_states[-2] = input of the last layer
  const half_t* xl = build_clip_stack(*this, ws, stack, x, [=](const half_t* qkv, half_t* att, hipStream_t s) {
    launch_clip_attention(qkv, att, S, D, H, s);
  }, &pen);
  {
    const float* gf = upload_vec(ws, {tm + "final_layer_norm.weight"}, D);
    const float* bf = upload_vec(ws, {tm + "final_layer_norm.bias"}, D);
    half_t* fin = arena.alloc_n<half_t>((size_t)S * D);
    float* f32 = final_f32_ = arena.alloc_n<float>((size_t)S * D);
    float* p32 = penult_f32_ = arena.alloc_n<float>((size_t)S * D);
    push([=](hipStream_t s) {
      launch_layernorm(xl, gf, bf, fin, S, D, eps, s);
      launch_half_to_float(fin, f32, (size_t)S * D, s);
      launch_half_to_float(pen, p32, (size_t)S * D, s);
    });
  }
  if (cfg.projection_dim > 0) {
    SD_REQUIRE(D % 8 == 0 && D <= 3072, kUnsupported, "text_projection: hidden size %d", D);
    proj_w_ = upload_rows(ws, {"text_projection.weight"}, cfg.projection_dim, D);
    pooled_ = arena.alloc_n<float>(cfg.projection_dim);
  }
  seal();
}

void TextEncoder::encode(const int32_t* input_ids, int eos_index, float* last_hidden_state, float* hidden_embeds,
                         float* pooled) {
  SD_HIP(hipSetDevice(device));
  const int S = cfg_.max_position_embeddings, D = cfg_.hidden_size;
  SD_REQUIRE(input_ids != nullptr, kInvalidArgument, "missing input 'input_ids'");
  SD_REQUIRE(eos_index >= 0 && eos_index < S, kInvalidArgument, "eos_index %d outside the %d-token prompt", eos_index, S);
  SD_HIP(hipMemcpyAsync(ids_, input_ids, (size_t)S * sizeof(int), hipMemcpyHostToDevice, stream));
  launch(cfg_.use_graph != 0);
  if (last_hidden_state)
    SD_HIP(hipMemcpyAsync(last_hidden_state, final_f32_, (size_t)S * D * sizeof(float), hipMemcpyDeviceToHost, stream));
  if (hidden_embeds)
    SD_HIP(hipMemcpyAsync(hidden_embeds, penult_f32_, (size_t)S * D * sizeof(float), hipMemcpyDeviceToHost, stream));
  if (pooled) {
    // pooler_output = final_layer_norm(last)[eos]; text_embeds = text_projection(pooler_output) (no bias)
    const float* row = final_f32_ + (size_t)eos_index * D;
    if (cfg_.projection_dim > 0) {
      launch_gemv(proj_w_, nullptr, row, D, pooled_, cfg_.projection_dim, 1, cfg_.projection_dim, D, 0, 0, 0, stream);
      SD_HIP(hipMemcpyAsync(pooled, pooled_, (size_t)cfg_.projection_dim * sizeof(float), hipMemcpyDeviceToHost, stream));
    } else {
      SD_HIP(hipMemcpyAsync(pooled, row, (size_t)D * sizeof(float), hipMemcpyDeviceToHost, stream));
    }
  }
  SD_HIP(hipStreamSynchronize(stream));
}

}  // namespace sd

struct sd_text_encoder {
  std::unique_ptr<sd::TextEncoder> impl;
};

extern "C" {

int sd_text_encoder_create(const sd_text_encoder_config* cfg, const sd_weights* w, int device, sd_text_encoder** out) {
  return sd::guarded([&] {
    SD_REQUIRE(cfg && w && out, sd::kInvalidArgument, "NULL argument");
    auto h = std::make_unique<sd_text_encoder>();
    h->impl = std::make_unique<sd::TextEncoder>(*cfg, w->store, device);
    *out = h.release();
  });
}
void sd_text_encoder_destroy(sd_text_encoder* t) { delete t; }
size_t sd_text_encoder_device_bytes(const sd_text_encoder* t) { return t ? t->impl->device_bytes() : 0; }
int sd_text_encoder_encode(sd_text_encoder* t, const int32_t* input_ids, int eos_index, float* last_hidden_state,
                           float* hidden_embeds, float* pooled) {
  return sd::guarded([&] {
    SD_REQUIRE(t && input_ids, sd::kInvalidArgument, "NULL argument");
    t->impl->encode(input_ids, eos_index, last_hidden_state, hidden_embeds, pooled);
  });
}

}  // extern "C"
