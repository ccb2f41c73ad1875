#include "clip_encoder.h"

namespace sd {

namespace {
std::vector<std::string> qkv_names(const std::string& p, const char* wb) {
  return {p + "self_attn.q_proj" + wb, p + "self_attn.k_proj" + wb, p + "self_attn.v_proj" + wb};
}
}  // namespace

void check_numel(const WeightStore& ws, const std::string& name, size_t numel) {
  const HostTensor& t = ws.get(name);   // kNotFound
  SD_REQUIRE(t.numel() == numel, kInvalidArgument, "%s has %zu elements, the config implies %zu", name.c_str(), t.numel(), numel);
}

void check_clip_stack_weights(const WeightStore& ws, const ClipStack& c) {
  const size_t D = c.D, I = c.I;
  for (int l = 0; l < c.L; ++l) {
    const std::string p = c.prefix + std::to_string(l) + ".";
    for (const char* ln : {"layer_norm1", "layer_norm2"})
      for (const char* wb : {".weight", ".bias"}) check_numel(ws, p + ln + wb, D);
    for (const auto& n : qkv_names(p, ".weight")) check_numel(ws, n, D * D);
    for (const auto& n : qkv_names(p, ".bias")) check_numel(ws, n, D);
    check_numel(ws, p + "self_attn.out_proj.weight", D * D);
    check_numel(ws, p + "self_attn.out_proj.bias", D);
    check_numel(ws, p + "mlp.fc1.weight", I * D);
    check_numel(ws, p + "mlp.fc1.bias", I);
    check_numel(ws, p + "mlp.fc2.weight", D * I);
    check_numel(ws, p + "mlp.fc2.bias", D);
  }
}

half_t* build_clip_stack(LaunchList& h, const WeightStore& ws, const ClipStack& c, half_t* x, const ClipAttention& attention,
                         half_t** last_input) {
  const int M = c.M, D = c.D, I = c.I, act = c.act;
  const float eps = c.eps;
  for (int l = 0; l < c.L; ++l) {
    const std::string p = c.prefix + std::to_string(l) + ".";
    if (last_input) *last_input = x;
    const float* g1 = h.upload_vec(ws, {p + "layer_norm1.weight"}, D);
    const float* b1 = h.upload_vec(ws, {p + "layer_norm1.bias"}, D);
    half_t* n1 = h.arena.alloc_n<half_t>((size_t)M * D);
    {
      const half_t* xi = x;
      h.push([=](hipStream_t s) { launch_layernorm(xi, g1, b1, n1, M, D, eps, s); });
    }
    // one stacked q|k|v projection (CLIPAttention q_proj / k_proj / v_proj, all with bias); the d^-0.5 scale transformers
    // applies to q is applied to the scores inside the attention kernel (same product)
    half_t* wqkv = h.upload_rows(ws, qkv_names(p, ".weight"), D, D);
    float* bqkv = h.upload_vec(ws, qkv_names(p, ".bias"), D);
    half_t* qkv = h.arena.alloc_n<half_t>((size_t)M * 3 * D);
    h.gemm(n1, wqkv, bqkv, nullptr, qkv, M, 3 * D, D, c.what);
    half_t* att = h.arena.alloc_n<half_t>((size_t)M * D);
    h.push([=](hipStream_t s) { attention(qkv, att, s); });
    half_t* wo = h.upload_rows(ws, {p + "self_attn.out_proj.weight"}, D, D);
    float* bo = h.upload_vec(ws, {p + "self_attn.out_proj.bias"}, D);
    half_t* x1 = h.arena.alloc_n<half_t>((size_t)M * D);
    h.gemm(att, wo, bo, x, x1, M, D, D, c.what);   // + residual
    const float* g2 = h.upload_vec(ws, {p + "layer_norm2.weight"}, D);
    const float* b2 = h.upload_vec(ws, {p + "layer_norm2.bias"}, D);
    half_t* n2 = h.arena.alloc_n<half_t>((size_t)M * D);
    h.push([=](hipStream_t s) { launch_layernorm(x1, g2, b2, n2, M, D, eps, s); });
    half_t* w1 = h.upload_rows(ws, {p + "mlp.fc1.weight"}, I, D);
    float* bb1 = h.upload_vec(ws, {p + "mlp.fc1.bias"}, I);
    half_t* hmid = h.arena.alloc_n<half_t>((size_t)M * I);
    h.gemm(n2, w1, bb1, nullptr, hmid, M, I, D, c.what);
    h.push([=](hipStream_t s) { launch_clip_act(hmid, (size_t)M * I, act, s); });
    half_t* w2 = h.upload_rows(ws, {p + "mlp.fc2.weight"}, D, I);
    float* bb2 = h.upload_vec(ws, {p + "mlp.fc2.bias"}, D);
    half_t* x2 = h.arena.alloc_n<half_t>((size_t)M * D);
    h.gemm(hmid, w2, bb2, x1, x2, M, D, I, c.what);   // + residual
    x = x2;
  }
  return x;
}

}  // namespace sd
