// UNet2DConditionModel / UNet2DConditionModelXL / ControlNetModel as a static launch graph of
// the gfx950 kernels.  Every comment "unet.py:NNN" / "controlnet.py:NNN" cites the reference line
// whose arithmetic the emitted ops reproduce (python_coreml_stable_diffusion/).
//
// Design notes
//  * static shapes like the reference's Core ML models (pipeline.py:112-114): everything is
//    allocated once, each tensor owns its bytes (288 GB HBM), so the forward is a pure launch
//    list and is captured into one HIP graph (~700 launches -> one replay).
//  * channels-last fp16 activations; weights re-laid-out at load to [Cout][ky][kx][Cin];
//    torch.cat skip concat (unet.py:213-216) is never materialised: GroupNorm and the 1x1
//    shortcut read both sources.
//  * prompt-constant work is hoisted: to_k/to_v of every cross-attention (unet.py:95-96) run
//    when encoder_hidden_states changes, not every step (SURVEY.md Appendix E obs. 3); all 22
//    time_emb_proj(SiLU(emb)) (unet.py:477) are one batched GEMV per step.
#include "unet.h"
#include "conv_plan.h"
#include "weight_prep.h"

#ifndef SD_GN_QKV_DEFAULT
#define SD_GN_QKV_DEFAULT 1   // the one-launch head of a SpatialTransformer (UNet::transformer); 0 = the three launches it replaces
#endif

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace sd {

namespace {

// A UNet's up path doubles the image once per level and concatenates it with the skip of the same level (unet.py:213-216, :498-500):
// the latent size must divide by 2^(levels - 1), or the stride-2 convs round up and the concat meets two sizes.  Checked before the
// base class opens the device.  (A ControlNet has no up path: any size its downsamplers take.)
const sd_unet_config& checked_size(const sd_unet_config& cfg) {
  if (!cfg.is_controlnet && cfg.n_levels >= 1 && cfg.n_levels <= SD_MAX_LEVELS) {
    const int q = 1 << (cfg.n_levels - 1);
    SD_REQUIRE(cfg.height % q == 0 && cfg.width % q == 0, kInvalidArgument,
               "latent size %dx%d: a UNet of %d levels needs height and width that divide by %d", cfg.height, cfg.width, cfg.n_levels, q);
  }
  return cfg;
}

}  // namespace

UNet::UNet(const sd_unet_config& cfg, const WeightStore& ws, int device) : Net(checked_size(cfg), ws, device) {
  if (cfg_.support_controlnet && !cfg_.is_controlnet && tune_env_int("SD_CN_CONCURRENT", 1) != 0) {
    SD_HIP(hipStreamCreateWithFlags(&cn_stream_, hipStreamNonBlocking));
    SD_HIP(hipEventCreateWithFlags(&ev_cn_fork_, hipEventDisableTiming));
    SD_HIP(hipEventCreateWithFlags(&ev_cn_join_, hipEventDisableTiming));
  }
  build_unet();
  seal();
}

UNet::~UNet() {
  (void)hipSetDevice(ll_.device);
  if (loop_graph_) (void)hipGraphExecDestroy(loop_graph_);
  close();   // the forward graph and the main stream first, as ever
  if (cn_stream_) {
    (void)hipStreamSynchronize(cn_stream_);
    (void)hipStreamDestroy(cn_stream_);
    (void)hipEventDestroy(ev_cn_fork_);
    (void)hipEventDestroy(ev_cn_join_);
  }
}

// Several bias-free 1x1 projections of the same input as ONE GEMM: weights stacked along Cout
// (attn1.to_q | attn1.to_k, unet.py:93-95): fewer launches, bigger N, same arithmetic.
Tensor UNet::conv_stacked(std::vector<Op>& ops, const std::vector<std::string>& names, const Tensor& x, int cout_each) {
  const int cin = x.C, n = (int)names.size();
  std::vector<std::string> sources;
  for (const std::string& nm : names) sources.push_back(nm + ".weight");
  half_t* d = ll_.arena.alloc_n<half_t>((size_t)n * cout_each * cin);
  refill(sources, d, [=](const WeightStore& ws) {
    std::vector<half_t> host((size_t)n * cout_each * cin);
    for (int i = 0; i < n; ++i) {
      const HostTensor& t = ws.get(sources[i]);
      SD_REQUIRE(t.numel() == (size_t)cout_each * cin, kInvalidArgument, "%s: bad shape", sources[i].c_str());
      for (size_t j = 0; j < t.numel(); ++j) host[(size_t)i * cout_each * cin + j] = (half_t)t.data[j];
    }
    SD_HIP(hipMemcpy(d, host.data(), host.size() * sizeof(half_t), hipMemcpyHostToDevice));
  });
  return conv_w(ops, names[0], d, nullptr, x, {.cout = n * cout_each});
}

// y = LN(x) . W^T + b  ==  rstd*(x . (W*gamma)^T) - rstd*mean*colsum(W*gamma) + (b + W.beta): the
// GEMM runs on the raw rows and applies the row statistics in its epilogue (igemm LNF kernels), so
// the separate LayerNorm launch, its HBM round trip and the fp16 rounding of LN(x) all disappear.
UNet::LnFold UNet::fold_layernorm(const std::string& ln, const std::vector<std::string>& names, int cin, int cout_each,
                                  bool geglu, bool upload_w) {
  const int n = (int)names.size(), ntot = n * cout_each;
  SD_REQUIRE(!geglu || n == 1, kInternal, "GEGLU fold takes one projection");
  // the sources: the LayerNorm's weight and bias, every projection's weight and - where the checkpoint has one - bias
  std::vector<std::string> sources = {ln + ".weight", ln + ".bias"};
  std::vector<char> has_bias(n);
  for (int i = 0; i < n; ++i) {
    sources.push_back(names[i] + ".weight");
    has_bias[i] = ws_->has(names[i] + ".bias");
    if (has_bias[i]) sources.push_back(names[i] + ".bias");
  }
  LnFold f;
  f.w = upload_w ? ll_.arena.alloc_n<half_t>((size_t)ntot * cin) : nullptr;
  f.colsum = ll_.arena.alloc_n<float>(ntot);
  f.bias = ll_.arena.alloc_n<float>(ntot);
  refill(sources, f.w, [=](const WeightStore& ws) {
    const HostTensor& g = ws.get(ln + ".weight");
    const HostTensor& be = ws.get(ln + ".bias");
    SD_REQUIRE((int)g.numel() == cin && (int)be.numel() == cin, kInvalidArgument, "%s: expected %d channels", ln.c_str(), cin);
    std::vector<half_t> w((size_t)ntot * cin);
    std::vector<float> colsum(ntot), bias(ntot);
    for (int i = 0; i < n; ++i) {
      const HostTensor& t = ws.get(names[i] + ".weight");
      SD_REQUIRE(t.numel() == (size_t)cout_each * cin, kInvalidArgument, "%s.weight: bad shape", names[i].c_str());
      const HostTensor* tb = has_bias[i] ? &ws.get(names[i] + ".bias") : nullptr;
      SD_REQUIRE(!tb || (int)tb->numel() == cout_each, kInvalidArgument, "%s.bias: bad shape", names[i].c_str());
      fold_layernorm_rows(t.data.data(), tb ? tb->data.data() : nullptr, g.data.data(), be.data.data(), cout_each, cin, i * cout_each,
                          geglu, w.data(), colsum.data(), bias.data());
    }
    if (f.w) SD_HIP(hipMemcpy(f.w, w.data(), w.size() * sizeof(half_t), hipMemcpyHostToDevice));
    SD_HIP(hipMemcpy(f.colsum, colsum.data(), ntot * sizeof(float), hipMemcpyHostToDevice));
    SD_HIP(hipMemcpy(f.bias, bias.data(), ntot * sizeof(float), hipMemcpyHostToDevice));
  });
  return f;
}

bool UNet::can_fold_ln(const Tensor& x, int cout, bool geglu) const {
  ConvDesc d;
  d.C0 = x.C;
  d.N = cout;
  d.ksize = 1;
  d.out_mode = geglu ? kOutGeglu : kOutHalf;
  static const bool off = tune_env_set("SD_NO_LN_FOLD");   // A/B switch for measurements
  return !off && conv_fast_path_ok(d);
}

Tensor UNet::layer_norm(std::vector<Op>& ops, const std::string& name, const Tensor& x) {
  // LayerNormANE eps default 1e-5 (layer_norm.py:21); checkpoint bias used as x_hat*w + b
  const float* w = upload_vec(name + ".weight", x.C);
  const float* b = upload_vec(name + ".bias", x.C);
  Tensor y = new_tensor(x.B, x.H, x.W, x.C);
  const half_t* xp = x.p;
  half_t* yp = y.p;
  const int M = x.M(), C = x.C;
  ops.push_back([=](hipStream_t s) { launch_layernorm(xp, w, b, yp, M, C, 1e-5f, s); });
  ops.back().label = "layernorm C=" + std::to_string(C) + " M=" + std::to_string(M) + " " + name;
  return y;
}

const float* UNet::register_temb(const std::string& name, int cout) {
  SD_REQUIRE(temb_used_ + cout <= kTembCap, kInternal, "time_emb_proj outputs exceed %d", kTembCap);
  temb_layers_.push_back({name, cout});
  const float* p = temb_all_ + temb_used_;
  temb_used_ += cout;
  return p;
}

// unet.py:470-489 with its time_emb_proj row (unet.py:477)
Tensor UNet::time_resnet(std::vector<Op>& ops, const std::string& p, const Tensor& x, const Tensor* x2, int cout) {
  return resnet(ops, p, x, x2, cout, register_temb(p + ".time_emb_proj", cout));
}

Tensor UNet::attention(std::vector<Op>& ops, const Tensor& q, const half_t* k, const half_t* vt, int heads, int Sq,
                       int Sk, int ldk, int ldv, int ldq, bool vt_perm, bool q_prescaled, const std::string* einsum) {
  Tensor o = new_tensor(q.B, q.H, q.W, q.C);
  // The reference's Einsum of this attention in W8A8 (activation_quantization.py:205-215, unet.py:45-59): where attention8 would run the
  // launch (vt_perm) over one q | k buffer on the int8 kernel's shape rule, a marked einsum becomes two launches - the quantizer over
  // what the q|k|v producer left, and attention_i8.hip - and an observing store gets one observer launch.  Anything else: today's op.
  const bool i8_could = einsum && vt_perm && attention_i8_shape_ok(q.C / heads, Sq, Sk) && ldq == 2 * q.C && ldk == ldq && k == q.p + q.C &&
                        ldv % 16 == 0;
  if (i8_could && observes_einsums())
    observe_einsum(ops, *einsum, q.p, vt, q.B, Sq, q.C, ldv, q_prescaled ? attention_q_prescale(q.C / heads) : 1.f);
  if (const EinsumMark* em = i8_could ? ws_->einsum(*einsum) : nullptr) {
    const int B = q.B, C = q.C, S = Sq;
    int8_t* qk_q = ll_.arena.alloc_n<int8_t>((size_t)B * S * 2 * C);
    int8_t* vt_q = ll_.arena.alloc_n<int8_t>((size_t)B * C * S);
    // r_q is the range of the un-scaled q: the stored queries carry the producer's factor, so the quantizer divides it out
    const float q_range_eff = q_prescaled ? em->q_absmax * attention_q_prescale(C / heads) : em->q_absmax;
    const float inv_q = 127.0f / q_range_eff, inv_k = 127.0f / em->k_absmax, inv_v = 127.0f / em->v_absmax;
    SD_REQUIRE(std::isfinite(inv_q) && std::isfinite(inv_k) && std::isfinite(inv_v), kInvalidArgument, "%s: a range has no finite inverse scale",
               einsum->c_str());
    const half_t *qkp = q.p, *vtp = vt;
    ops.push_back([=](hipStream_t s) { launch_einsum_quantize(qkp, vtp, B, S, C, ldv, 1, inv_q, inv_k, inv_v, qk_q, vt_q, s); });
    ops.back().label = "einsum_q8 " + einsum->substr(0, einsum->size() - std::string(".einsum").size());
    AttnI8Desc d;
    d.q = qk_q;
    d.k = qk_q + C;
    d.vt = vt_q;
    d.out = o.p;
    d.B = B;
    d.heads = heads;
    d.S = S;
    d.ldq = d.ldk = 2 * C;
    d.ldv = S;
    d.ldo = C;
    d.q_absmax = em->q_absmax;
    d.k_absmax = em->k_absmax;
    d.v_absmax = em->v_absmax;
    ops.push_back([this, d](hipStream_t s) {
      // (the run-time implementation switch only keeps its refusal: all three run this one kernel, as they run attention8)
      SD_REQUIRE(cfg_.attention_impl != kAttnSplitEinsumV2 || d.S < 512 || d.S % 512 == 0, kInvalidArgument,
                 "SPLIT_EINSUM_V2 needs S_q %% 512 == 0 (got %d); the reference would silently drop the tail (attention.py:86)", d.S);
      launch_attention_i8(d, s);
    });
    ops.back().label = "attention+i8 h=" + std::to_string(heads) + " d=64 Sq=" + std::to_string(Sq) + " Sk=" + std::to_string(Sk);
    ops.back().flop = 4.0 * q.B * (double)q.C * Sq * Sk;
    einsum_applies(*einsum);
    return o;
  }
  AttnDesc d;
  d.q = q.p;
  d.k = k;
  d.vt = vt;
  d.out = o.p;
  d.B = q.B;
  d.heads = heads;
  d.d = q.C / heads;
  d.Sq = Sq;
  d.Sk = Sk;
  d.ldq = ldq;
  d.ldk = ldk;
  d.ldv = ldv;
  d.ldo = q.C;
  d.vt_perm = vt_perm ? 1 : 0;
  d.q_prescaled = (vt_perm && q_prescaled) ? 1 : 0;
  SD_REQUIRE(attention_supported(d.d), kUnsupported, "head dim %d (C=%d, heads=%d) unsupported", d.d, q.C, heads);
  if (d.vt_perm) {   // attention8's balanced form wants scratch (one buffer for all of this handle's launches: they run in sequence)
    size_t pb = 0;
    int nc = 0;
    if (attention8_sk_scratch(d, &pb, &nc)) {
      if (pb > sk_part_bytes_) {
        sk_part_ = reinterpret_cast<float*>(ll_.arena.alloc(pb));
        sk_part_bytes_ = pb;
      }
      if (nc > sk_cnt_n_) {
        sk_cnt_ = ll_.arena.alloc_n<unsigned>(nc);
        sk_cnt_n_ = nc;
        SD_HIP(hipMemsetAsync(sk_cnt_, 0, (size_t)nc * sizeof(unsigned), ll_.stream));
      }
      d.sk_part = sk_part_;
      d.sk_part_bytes = sk_part_bytes_;
      d.sk_cnt = sk_cnt_;
      d.sk_cnt_n = sk_cnt_n_;
    }
  }
  ops.push_back([this, d](hipStream_t s) {
    AttnDesc dd = d;
    dd.impl = cfg_.attention_impl;   // run-time switch (the reference's global, unet.py:39)
    launch_attention(dd, s);
  });
  ops.back().label = "attention h=" + std::to_string(heads) + " d=" + std::to_string(d.d) + " Sq=" + std::to_string(Sq) +
                     " Sk=" + std::to_string(Sk);
  ops.back().flop = 4.0 * q.B * (double)q.C * Sq * Sk;
  return o;
}

// unet.py:586-591 (+ CrossAttention :87-118, FeedForward/GEGLU :594-617)
Tensor UNet::transformer_block(std::vector<Op>& ops, const std::string& b, const Tensor& h, int heads, const std::string* proj_out,
                               const Tensor* tres, bool* tail_done, const PreQkv* pre, bool* tail_q8) {
  const int C = h.C, S = h.H * h.W, L = cfg_.context_len;
  // --- self attention.  MFMA-tileable widths: norm1 is folded into ONE fused q|k|v GEMM whose V
  // columns leave token-transposed (attention's V^T operand); otherwise LN + stacked q|k + V^T GEMMs.
  const int ldv = round_up(S, 8);
  Tensor qk;
  bool vt_perm = false;   // attention8.hip will run this self-attention: the fused q|k|v GEMM writes V^T in its key order
  bool q_pre = false;     // ... and the queries pre-scaled
  half_t* vtp;
  if (pre) {   // the SpatialTransformer's head launch (UNet::transformer) already wrote this block's q | k and V^T
    qk = pre->qk;
    vtp = pre->vt;
    vt_perm = pre->vt_perm;
    q_pre = pre->q_pre;
  } else if (can_fold_ln(h, 3 * C, false) && S % 8 == 0 && (2 * C) % 64 == 0) {
    const std::string qname = b + ".attn1.to_qkv";
    const std::vector<std::string> parts = {b + ".attn1.to_q", b + ".attn1.to_k", b + ".attn1.to_v"};
    vt_perm = attention8_shape_ok(C / heads, S, S) && S % 16 == 0;
    // attention8 takes the queries with d^-0.5 * log2(e) already in them: multiplied into the fp32 accumulator here
    q_pre = vt_perm;
    ConvArgs qa{.cout = 3 * C, .ldT = ldv, .n_trans = 2 * C, .vt_out = &vtp, .vt_perm = vt_perm,
                .q_scale = q_pre ? attention_q_prescale(C / heads) : 1.f, .q_cols = q_pre ? C : 0};
    // All three projections W8A8-marked with ONE range, on a shape plan tile 22 takes: norm1 is NOT folded - one layernorm_q8 launch
    // writes int8(norm1(h)), the tensor the reference calibrates and quantizes for to_q, to_k and to_v alike, and the q|k|v launch
    // streams it and the stacked int8 matrix (no fp16 copy).  Anything else - one or two marks, three ranges, a shape off the rule -
    // keeps the folded fp16 launch.  An observing store (observe_qkv) leaves the launch as it is and puts a LayerNorm + absmax pair
    // over the same tensor, reported under the three weight names.
    const WeightPin qpin = qkv_plan(qname, parts, h, qa);
    if (observes_qkv(qname, parts, h, qa)) observe_tensor(ops, qname, layer_norm(ops, b + ".norm1", h), parts);
    if (qpin.kind == WeightSource::I8Qkv) {
      const ConvWeights qw = upload_qkv_i8(parts, qpin, C, C);
      float* qb = nullptr;   // (SD checkpoints have no bias on to_q / to_k / to_v; one that has goes up stacked, absent parts zero)
      if (ws_->has(parts[0] + ".bias") || ws_->has(parts[1] + ".bias") || ws_->has(parts[2] + ".bias")) {
        std::vector<std::pair<int, std::string>> present;   // (part, its bias tensor)
        std::vector<std::string> sources;
        for (int i = 0; i < 3; ++i)
          if (ws_->has(parts[i] + ".bias")) present.push_back({i, parts[i] + ".bias"}), sources.push_back(parts[i] + ".bias");
        qb = ll_.arena.alloc_n<float>((size_t)3 * C);
        refill(sources, qb, [=](const WeightStore& ws) {
          std::vector<float> hb((size_t)3 * C, 0.f);
          for (const auto& [i, bname] : present) {
            const HostTensor& tb = ws.get(bname);
            SD_REQUIRE((int)tb.numel() == C, kInvalidArgument, "%s: bad shape", bname.c_str());
            std::copy(tb.data.begin(), tb.data.end(), hb.begin() + (size_t)i * C);
          }
          SD_HIP(hipMemcpy(qb, hb.data(), hb.size() * sizeof(float), hipMemcpyHostToDevice));
        });
      }
      const float* nw = upload_vec(b + ".norm1.weight", C);
      const float* nb = upload_vec(b + ".norm1.bias", C);
      const int M = h.M();
      int8_t* xq = ll_.arena.alloc_n<int8_t>((size_t)M * C);
      const half_t* xp = h.p;
      const float inv_s = qw.cw.inv_s;
      ops.push_back([=](hipStream_t s) { launch_layernorm_q8(xp, nw, nb, xq, M, C, 1e-5f, inv_s, s); });
      ops.back().label = "layernorm_q8 " + b + ".norm1";
      qa.x_i8 = xq;
      qk = conv_w(ops, qname, qw, qb, h, qa);
    } else {
      LnFold f = fold_layernorm(b + ".norm1", parts, C, C, false);
      qa.ln_colsum = f.colsum;
      qk = conv_w(ops, qname, f.w, f.bias, h, qa);
    }
  } else {
    Tensor n1 = layer_norm(ops, b + ".norm1", h);
    qk = conv_stacked(ops, {b + ".attn1.to_q", b + ".attn1.to_k"}, n1, C);   // [M][2C]: q | k
    vtp = conv(ops, b + ".attn1.to_v", n1, {.cout = C, .bias = false, .out_mode = kOutHalfT, .ldT = ldv}).p;
  }
  Tensor q = qk;
  q.C = C;   // logical width of q; rows are 2C apart
  const std::string einsum1 = b + ".attn1.einsum";
  Tensor a1 = attention(ops, q, qk.p + C, vtp, heads, S, S, 2 * C, ldv, 2 * C, vt_perm, q_pre, &einsum1);
  // attn1.to_out + residual -> norm2 -> to_q -> cross-attention -> attn2.to_out + residual as ONE launch at the 5-head level
  // (xattn_out.hip: 32 tokens x all heads per workgroup; h1 never goes to HBM): three launches of 11.6 + 15.3 + 11.6 us become one of
  // 23.7, step 4.493 -> 4.443 ms (profiles/r05_xattn_out_stage2_ab.log).  SD_XATTN_OUT (with SD_TUNE) for the A/B: 0 = the three
  // launches, 1 = only the cross-attention branch in one launch (-0.024 ms), 2 = that at the 10-head level too (64 workgroups of ten
  // waves: +0.04 ms), 3 = the default
  static const int xo_mode = tune_env_int("SD_XATTN_OUT", 3);
  const bool xo_branch = xo_mode != 0 && can_fold_ln(h, C, false) && xattn_fused_ok(C, heads, S, L) && xattn_out_ok(C, heads, S, L) &&
                         (heads == 5 || xo_mode == 2);
  const bool xo_pre = xo_branch && xo_mode == 3 && heads == 5;
  Tensor h1;
  if (!xo_pre) h1 = conv(ops, b + ".attn1.to_out.0", a1, {.cout = C, .res = h.p, .keep_compressed = true});
  // --- cross attention: K / V^T of the prompt are computed by ctx_ops_ when the prompt changes
  const int ldvc = round_up(L, 8);
  Tensor k2 = conv(ctx_ops_, b + ".attn2.to_k", ctx_, {.cout = C, .bias = false});
  Tensor vt2 = conv(ctx_ops_, b + ".attn2.to_v", ctx_, {.cout = C, .bias = false, .out_mode = kOutHalfT, .ldT = ldvc});
  Tensor a2;
  Tensor h2;
  bool branch_done = false;
  if (xo_branch) {
    LnFold f = fold_layernorm(b + ".norm2", {b + ".attn2.to_q"}, C, C, false);
    half_t* wq_t = ll_.arena.alloc_n<half_t>((size_t)C * C);
    derive(f.w, [=] { launch_xattn_out_retile(f.w, wq_t, C, ll_.stream); });
    const half_t* wo = upload_conv_weight(b + ".attn2.to_out.0", C, C, 1, false);
    half_t* wo_t = ll_.arena.alloc_n<half_t>((size_t)C * C);
    derive(wo, [=] { launch_xattn_out_retile(wo, wo_t, C, ll_.stream); });
    h2 = new_tensor(h.B, h.H, h.W, C);
    XAttnOutDesc xd;
    xd.x = xo_pre ? a1.p : h1.p;
    if (xo_pre) {
      const half_t* wo1 = upload_conv_weight(b + ".attn1.to_out.0", C, C, 1, false);
      half_t* wo1_t = ll_.arena.alloc_n<half_t>((size_t)C * C);
      derive(wo1, [=] { launch_xattn_out_retile(wo1, wo1_t, C, ll_.stream); });
      xd.h0 = h.p;
      xd.wo1_t = wo1_t;
      xd.o1_bias = upload_vec(b + ".attn1.to_out.0.bias", C);
    }
    xd.wq_t = wq_t;
    xd.q_bias = f.bias;
    xd.q_colsum = f.colsum;
    xd.k = k2.p;
    xd.vt = vt2.p;
    xd.wo_t = wo_t;
    xd.o_bias = upload_vec(b + ".attn2.to_out.0.bias", C);
    xd.out = h2.p;
    xd.M = h.M();
    xd.C = C;
    xd.S = S;
    xd.L = L;
    xd.ldv = ldvc;
    xd.heads = heads;
    ops.push_back([this, xd](hipStream_t s) {
      XAttnOutDesc dd = xd;
      dd.impl = cfg_.attention_impl;
      launch_xattn_out(dd, s);
    });
    ops.back().label = std::string("xattn") + (xo_pre ? " attn1.to_out + residual +" : "") + "+ln q-proj " + std::to_string(C) + "->" + std::to_string(C) +
                       " + attention h=" + std::to_string(heads) + " d=64 Sq=" + std::to_string(S) + " Sk=" + std::to_string(L) +
                       " + to_out + residual " + b + ".attn2";
    ops.back().flop = (xo_pre ? 6.0 : 4.0) * h.M() * (double)C * C + 4.0 * h.B * (double)C * S * L;
    branch_done = true;
  } else if (can_fold_ln(h1, C, false) && xattn_fused_ok(C, heads, S, L)) {
    // norm2 -> to_q -> softmax(q k^T) v as ONE launch (xattn.hip): the q tile stays in registers
    LnFold f = fold_layernorm(b + ".norm2", {b + ".attn2.to_q"}, C, C, false);
    a2 = new_tensor(h1.B, h1.H, h1.W, C);
    XAttnDesc xd;
    xd.x = h1.p;
    xd.wq = f.w;
    xd.bias = f.bias;
    xd.colsum = f.colsum;
    xd.k = k2.p;
    xd.vt = vt2.p;
    xd.out = a2.p;
    xd.M = h1.M();
    xd.C = C;
    xd.S = S;
    xd.L = L;
    xd.ldv = ldvc;
    xd.heads = heads;
    ops.push_back([this, xd](hipStream_t s) {
      XAttnDesc dd = xd;
      dd.impl = cfg_.attention_impl;
      launch_xattn_fused(dd, s);
    });
    ops.back().label = "xattn+ln q-proj " + std::to_string(C) + "->" + std::to_string(C) + " + attention h=" + std::to_string(heads) +
                       " d=64 Sq=" + std::to_string(S) + " Sk=" + std::to_string(L) + " " + b + ".attn2";
    ops.back().flop = 2.0 * h1.M() * (double)C * C + 4.0 * h1.B * (double)C * S * L;
  } else {
    Tensor q2;
    if (can_fold_ln(h1, C, false)) {
      LnFold f = fold_layernorm(b + ".norm2", {b + ".attn2.to_q"}, C, C, false);
      q2 = conv_w(ops, b + ".attn2.to_q", f.w, f.bias, h1, {.cout = C, .ln_colsum = f.colsum});
    } else {
      Tensor n2 = layer_norm(ops, b + ".norm2", h1);
      q2 = conv(ops, b + ".attn2.to_q", n2, {.cout = C, .bias = false});
    }
    a2 = attention(ops, q2, k2.p, vt2.p, heads, S, L, C, ldvc, C);
  }
  if (!branch_done) h2 = conv(ops, b + ".attn2.to_out.0", a2, {.cout = C, .res = h1.p, .keep_compressed = true});
  // --- GEGLU feed-forward (norm3 folded the same way)
  Tensor g;
  // A palettized ff.net.0.proj whose plan is smgeglu.hip on 128-row tiles stays palettized (plan tile 16): stream, LUT and - with the
  // fold - norm3.weight go up, colsum and the folded bias come from lut[indices] as ever, no fp16 matrix is uploaded
  // A W8A8-marked ff.net.0.proj whose fp16 plan is smgeglu.hip runs as plan tile 20, folded or not: norm3 is NOT folded - one
  // layernorm_q8 launch writes int8(norm3(h2)), the tensor the reference calibrates and quantizes, and the GEGLU streams it with the raw
  // bias.  An observing store (observe_geglus) leaves the GEGLU as it is and puts a LayerNorm + absmax pair over the same tensor.
  const std::string gname = b + ".ff.net.0.proj";
  const bool fold3 = can_fold_ln(h2, 8 * C, true);
  ConvArgs ga{.cout = 8 * C, .out_mode = kOutGeglu, .keep_compressed = true};
  const WeightPin gpin = weight_plan(gname, h2, ga, fold3);
  // The tail, asked before the GEGLU is built.  A W8A8-marked ff.net.2 whose un-merged shape plan tile 24 takes (conv_plan.h
  // smgemm_q8_wanted; not where the 320-channel level's one-launch tail runs) is NOT merged with proj_out: it runs from int8 on
  // int8(v * gelu(g)) - the tensor the reference calibrates and quantizes for it - plus h2, and proj_out is a launch of its own behind
  // it (UNet::transformer; from int8 too where it is marked: plan tile 19).  The GEGLU writes the int8 product itself where it runs plan
  // tile 20 (no fp16 product is allocated); behind any other GEGLU one plain-form layernorm_q8 launch quantizes the product, the same
  // flat buffer read as (4 M, C) rows.  An observing store (observe_tails) leaves the tail as it is and puts observers beside it.
  static const int fp_mode = tune_env_int("SD_FFN_PROJ", 1);
  const bool ffn_one_launch = proj_out && tres && tail_done && fp_mode != 0 && ffn_proj_ok(C, 4 * C, h.M(), S);
  const std::string tname = b + ".ff.net.2";
  Tensor gshape = h2;   // the GEGLU product as the planner sees it
  gshape.C = 4 * C;
  gshape.p = nullptr;
  gshape.gn.reset();
  static const int8_t i8_present = 0;   // the planner only tests the pointer
  ConvArgs ta{.cout = C, .res = h2.p, .keep_compressed = true, .x_i8 = &i8_present};
  const bool tail_rule = !ffn_one_launch && C % 8 == 0 && C <= 2048;   // (what the fall-back quantizer launch takes)
  const WeightPin tpin = tail_rule ? weight_plan(tname, gshape, ta, false) : WeightPin{};
  const bool tail_i8 = tpin.kind == WeightSource::I8GemmQ;
  const bool tail_observed = tail_rule && observes_tail(tname, gshape, ta);
  ConvWeights tw(nullptr);
  int8_t* gq = nullptr;
  if (tail_i8) {
    tw = upload_compressed(tname, tpin, 4 * C, ta);
    gq = ll_.arena.alloc_n<int8_t>((size_t)h2.M() * 4 * C);
  }
  if (observes_geglu(gname, h2, ga, fold3)) observe_tensor(ops, gname, layer_norm(ops, b + ".norm3", h2));
  if (gpin.kind == WeightSource::I8Geglu) {
    if (tail_i8) {
      ga.out_q8 = gq;
      ga.out_inv_s = tw.cw.inv_s;
    }
    const ConvWeights gw = upload_compressed(gname, gpin, C, ga);
    const float* gb = ws_->has(gname + ".bias") ? upload_vec(gname + ".bias", 8 * C, true) : nullptr;
    const float* nw = upload_vec(b + ".norm3.weight", C);
    const float* nb = upload_vec(b + ".norm3.bias", C);
    const int M = h2.M();
    int8_t* xq = ll_.arena.alloc_n<int8_t>((size_t)M * C);
    const half_t* xp = h2.p;
    const float inv_s = gw.cw.inv_s;
    ops.push_back([=](hipStream_t s) { launch_layernorm_q8(xp, nw, nb, xq, M, C, 1e-5f, inv_s, s); });
    ops.back().label = "layernorm_q8 " + b + ".norm3";
    ga.x_i8 = xq;
    g = conv_w(ops, gname, gw, gb, h2, ga);
  } else if (fold3) {
    const WeightPin pin = gpin;
    const bool fp16 = pin.kind == WeightSource::Fp16;
    LnFold f = fold_layernorm(b + ".norm3", {b + ".ff.net.0.proj"}, C, 8 * C, true, fp16);
    ga.ln_colsum = f.colsum;
    g = conv_w(ops, b + ".ff.net.0.proj", fp16 ? ConvWeights(f.w) : upload_compressed(b + ".ff.net.0.proj", pin, C, ga, b + ".norm3"), f.bias, h2, ga);
  } else {
    Tensor n3 = layer_norm(ops, b + ".norm3", h2);
    g = conv(ops, b + ".ff.net.0.proj", n3, {.cout = 8 * C, .out_mode = kOutGeglu, .keep_compressed = true});
  }
  if (tail_i8) {
    if (!ga.out_q8) {   // the product exists in fp16: one quantizer launch over it
      const int rows = 4 * h2.M();
      const half_t* gp = g.p;
      const float inv_s = tw.cw.inv_s;
      ops.push_back([=](hipStream_t s) { launch_layernorm_q8(gp, nullptr, nullptr, gq, rows, C, 1e-5f, inv_s, s); });
      ops.back().label = "quantize_q8 " + tname;
    }
    ta.x_i8 = gq;
    if (tail_q8) *tail_q8 = true;
    return conv_w(ops, tname, tw, upload_vec(tname + ".bias", C), g, ta);
  }
  if (tail_observed) {   // the range ff.net.2 would be quantized with and, through a scratch ff.net.2, the one its proj_out would be
    observe_tensor(ops, tname, g);
    if (proj_out && tres) {
      const ConvArgs pa{.cout = C, .res = tres->p, .keep_compressed = true};
      Tensor h3 = h2;   // (shape)
      h3.gn.reset();
      if (observes_tail(*proj_out, h3, pa)) observe_tensor(ops, *proj_out, conv(ops, tname, g, {.cout = C, .res = h2.p}));
    }
  }
  // the tail of the SpatialTransformer - ff.net.2 + residual -> proj_out + residual - as ONE launch at the 320-channel level
  // (ffn_proj_kernel: the intermediate never goes to HBM, the output's GroupNorm statistics for the next resnet come out of it);
  // five launches less per step, 5.402 -> 5.392 ms on the (slow) box it was measured on (profiles/r05_ffn_proj_ab_slow_box.log);
  // SD_FFN_PROJ=0 (with SD_TUNE): the two GEMM launches (A/B)
  if (ffn_one_launch && g.C == 4 * C) {
    const half_t* w1 = upload_conv_weight(b + ".ff.net.2", C, 4 * C, 1, false);
    half_t* w1_t = ll_.arena.alloc_n<half_t>((size_t)C * 4 * C);
    derive(w1, [=] { launch_xattn_out_retile_nk(w1, w1_t, C, 4 * C, ll_.stream); });
    const half_t* w2 = upload_conv_weight(*proj_out, C, C, 1, false);
    half_t* w2_t = ll_.arena.alloc_n<half_t>((size_t)C * C);
    derive(w2, [=] { launch_xattn_out_retile_nk(w2, w2_t, C, C, ll_.stream); });
    Tensor out = new_tensor(h.B, h.H, h.W, C);
    FfnProjDesc d;
    d.g = g.p;
    d.w1_t = w1_t;
    d.b1 = upload_vec(b + ".ff.net.2.bias", C);
    d.res1 = h2.p;
    d.w2_t = w2_t;
    d.b2 = upload_vec(*proj_out + ".bias", C);
    d.res2 = tres->p;
    d.out = out.p;
    d.M = h.M();
    d.C = C;
    d.K1 = 4 * C;
    d.S = S;
    auto hook = std::make_shared<GnHook>();   // a GroupNorm built later over this tensor may ask for its statistics (as conv_w)
    out.gn = hook;
    hook->ops_pos = (int)ops.size();
    hook->ops_list = &ops;
    ops.push_back([d, hook](hipStream_t s) {
      FfnProjDesc dd = d;
      dd.gn_partial = hook->partial;
      dd.gn_groups = hook->groups;
      hook->produced(launch_ffn_proj(dd, s));
    });
    char buf[256];
    snprintf(buf, sizeof(buf), "gemm1x1 %d->%d @%dx%d M=%d K=%d %s.ff.net.2 + residual + proj_out + residual", 4 * C, C, h.H, h.W, h.M(), 4 * C, b.c_str());
    ops.back().label = buf;
    ops.back().flop = 2.0 * h.M() * (double)C * (4 * C) + 2.0 * h.M() * (double)C * C;
    *tail_done = true;
    return out;
  }
  // The other levels: the same tail as ONE GEMM over the K-concatenation [g | h2] with the folded weights [Wp W2 | Wp] and bias
  // Wp b2 + bp (wfold.hip; both fixed for the life of the handle): h3 = W2 g + b2 + h2 has no other reader, so one launch and the
  // write and read of h3 leave the step, at the same FLOPs and weight bytes.  The two source matrices only pass through a
  // temporary buffer.  Only where the merged GEMM runs a plan that was measured in a step against the two launches it replaces -
  // the two-source rule of smgemm.hip or a row of tuned_convs.inc (SD2.1-base's three levels, SDXL-base 768x768); any other shape
  // keeps the two launches and their own tuned plans.  SD_TAIL_MERGE=0 (with SD_TUNE): the two GEMM launches everywhere (A/B),
  // SD_TAIL_MERGE=2: the merge on every shape of the general rule (for measuring a new one).
  static const int merge_mode = tune_env_int("SD_TAIL_MERGE", 1);
  bool merge = proj_out && tres && tail_done && merge_mode != 0 && g.C == 4 * C && C % 64 == 0 && h.M() <= 2048;
  if (merge && merge_mode != 2) {
    ConvDesc md;
    md.x0 = g.p;
    md.C0 = 4 * C;
    md.x1 = h2.p;
    md.C1 = C;
    md.B = h.B;
    md.Hi = md.Ho = h.H;
    md.Wi = md.Wo = h.W;
    md.N = C;
    merge = smgemm_wanted(md) || conv_plan_is_tuned(md);
  }
  if (merge) {
    const int K1 = 4 * C;
    const std::string n2 = b + ".ff.net.2", np = *proj_out;
    half_t* wm = ll_.arena.alloc_n<half_t>((size_t)C * (K1 + C));
    float* bm = ll_.arena.alloc_n<float>(C);
    refill({n2 + ".weight", np + ".weight", n2 + ".bias", np + ".bias"}, wm, [=](const WeightStore& ws) {
      const HostTensor& t2 = ws.get(n2 + ".weight");
      const HostTensor& tp = ws.get(np + ".weight");
      const HostTensor& tb2 = ws.get(n2 + ".bias");
      const HostTensor& tbp = ws.get(np + ".bias");
      SD_REQUIRE(t2.numel() == (size_t)C * K1 && tp.numel() == (size_t)C * C && (int)tb2.numel() == C && (int)tbp.numel() == C, kInvalidArgument,
                 "%s: ff.net.2 / proj_out parameter shapes", b.c_str());
      // staging buffer, freed below: [b2 | bp] fp32, then [W2 | Wp] fp16 as the two-launch form uploads them
      std::vector<float> hb(2 * (size_t)C);
      std::vector<half_t> hw((size_t)C * K1 + (size_t)C * C);
      for (int i = 0; i < C; ++i) hb[i] = tb2.data[i], hb[C + i] = tbp.data[i];
      for (size_t i = 0; i < t2.numel(); ++i) hw[i] = (half_t)t2.data[i];
      for (size_t i = 0; i < tp.numel(); ++i) hw[t2.numel() + i] = (half_t)tp.data[i];
      char* tmp = nullptr;
      const size_t b_bytes = hb.size() * sizeof(float), w_bytes = hw.size() * sizeof(half_t);
      SD_HIP(hipMalloc(reinterpret_cast<void**>(&tmp), b_bytes + w_bytes));
      try {
        SD_HIP(hipMemcpy(tmp, hb.data(), b_bytes, hipMemcpyHostToDevice));
        SD_HIP(hipMemcpy(tmp + b_bytes, hw.data(), w_bytes, hipMemcpyHostToDevice));
        const float* db = reinterpret_cast<const float*>(tmp);
        const half_t* dw = reinterpret_cast<const half_t*>(tmp + b_bytes);
        launch_wfold(dw + (size_t)C * K1, db + C, dw, db, wm, bm, C, C, K1, ll_.stream);
        SD_HIP(hipStreamSynchronize(ll_.stream));
      } catch (...) {
        (void)hipFree(tmp);
        throw;
      }
      SD_HIP(hipFree(tmp));
    });
    Tensor out = conv_w(ops, b + ".ff.net.2 + residual + proj_out + residual", wm, bm, g, {.x2 = &h2, .cout = C, .res = tres->p});
    ops.back().flop = 2.0 * h.M() * (double)C * K1 + 2.0 * h.M() * (double)C * C;   // the algorithmic count of the two maps
    *tail_done = true;
    return out;
  }
  return conv(ops, b + ".ff.net.2", g, {.cout = C, .res = h2.p});
}

// unet.py:553-563; GroupNorm eps hard-coded 1e-6 (unet.py:528-531)
Tensor UNet::transformer(std::vector<Op>& ops, const std::string& p, const Tensor& x, int heads, int depth) {
  const int G = cfg_.norm_num_groups, C = x.C, HW = x.H * x.W;
  // norm -> proj_in -> norm1 -> to_q | to_k | to_v of block 0 as ONE launch at the 5-head level (xattn_out.hip gn_proj_qkv_kernel: rows are
  // independent once the GroupNorm statistics exist, so a 32-token workgroup carries its rows through both GEMMs in LDS).
  // Three launches of 10 + 9.5 + 15 us become one of 24.5; same box, back to back: 4.415 / 4.430 -> 4.344 / 4.368 ms, eight prompts
  // 18.73 -> 18.45 ms (profiles/r06_gn_qkv_ab.txt).  SD_GN_QKV=0 (with SD_TUNE): the three launches.
  static const int gq_mode = tune_env_int("SD_GN_QKV", SD_GN_QKV_DEFAULT);
  const int ldv0 = round_up(HW, 8);
  const bool gq = gq_mode != 0 && depth >= 1 && x.gn && !x.gn->partial && x.gn->ops_list == &ops &&
                  C % G == 0 && can_fold_ln(x, 3 * C, false) && gn_proj_qkv_ok(C, heads, HW, x.M(), ldv0, G) &&
                  (size_t)x.M() * C * 2 < ((size_t)1 << 31);
  Tensor h;
  PreQkv pre;
  if (gq) {
    const std::string b0 = p + ".transformer_blocks.0";
    float* partial = ll_.arena.alloc_n<float>(groupnorm_scratch_floats(x.B, HW, G));
    std::shared_ptr<GnHook> hook = x.gn;
    hook->partial = partial;
    hook->groups = G;
    Tensor t0 = new_tensor(x.B, x.H, x.W, C);   // the normalised tensor of the fall-back (producer left no statistics)
    h = new_tensor(x.B, x.H, x.W, C);
    const half_t* wp = upload_conv_weight(p + ".proj_in", C, C, 1, false);
    half_t* wp_t = ll_.arena.alloc_n<half_t>((size_t)C * C);
    derive(wp, [=] { launch_xattn_out_retile_nk(wp, wp_t, C, C, ll_.stream); });
    LnFold f = fold_layernorm(b0 + ".norm1", {b0 + ".attn1.to_q", b0 + ".attn1.to_k", b0 + ".attn1.to_v"}, C, C, false);
    half_t* wq_t = ll_.arena.alloc_n<half_t>((size_t)3 * C * C);
    derive(f.w, [=] { launch_xattn_out_retile_nk(f.w, wq_t, 3 * C, C, ll_.stream); });
    pre.qk = new_tensor(x.B, x.H, x.W, 2 * C);
    pre.vt = ll_.arena.alloc_n<half_t>((size_t)x.B * C * ldv0);
    pre.vt_perm = attention8_shape_ok(C / heads, HW, HW) && HW % 16 == 0;
    pre.q_pre = pre.vt_perm;
    GnProjQkvDesc g;
    g.x = x.p;
    g.gn_partial = partial;
    g.gn_gamma = upload_vec(p + ".norm.weight", C);
    g.gn_beta = upload_vec(p + ".norm.bias", C);
    g.gn_groups = G;
    g.gn_eps = 1e-6f;
    g.wp_t = wp_t;
    g.p_bias = upload_vec(p + ".proj_in.bias", C);
    g.h = h.p;
    g.wqkv_t = wq_t;
    g.qkv_bias = f.bias;
    g.qkv_colsum = f.colsum;
    g.ln_eps = 1e-5f;
    g.qk = pre.qk.p;
    g.vt = pre.vt;
    g.M = x.M();
    g.C = C;
    g.S = HW;
    g.ldT = ldv0;
    g.vt_perm = pre.vt_perm;
    g.q_scale = pre.q_pre ? attention_q_prescale(C / heads) : 1.f;
    const int B = x.B;
    ops.push_back([g, hook, t0, B, HW, G, C](hipStream_t s) {
      GnProjQkvDesc gg = g;
      const int n = hook->consume();
      if (n >= 1 && n <= 128) {
        gg.gn_entries = n;
      } else {
        launch_groupnorm(g.x, C, nullptr, 0, const_cast<float*>(g.gn_partial), g.gn_gamma, g.gn_beta, t0.p, B, HW, G, g.gn_eps, 0, s, n);
        gg.x = t0.p;
        gg.gn_entries = 0;
      }
      launch_gn_proj_qkv(gg, s);
    });
    char buf[256];
    snprintf(buf, sizeof(buf), "gemm1x1+gn %d->%d @%dx%d M=%d K=%d %s.proj_in + norm1 + to_qkv %d->%d", C, C, x.H, x.W, x.M(), C, p.c_str(), C, 3 * C);
    ops.back().label = buf;
    ops.back().flop = 8.0 * x.M() * (double)C * C;
  } else {
    Tensor t0 = group_norm(ops, p + ".norm", x, nullptr, 1e-6f, false);
    h = conv(ops, p + ".proj_in", t0, {.cout = x.C, .keep_compressed = true});
  }
  bool tail_done = false, tail_q8 = false;
  const std::string proj_name = p + ".proj_out";
  for (int d = 0; d < depth; ++d) {
    const bool last = d == depth - 1;
    h = transformer_block(ops, p + ".transformer_blocks." + std::to_string(d), h, heads, last ? &proj_name : nullptr, last ? &x : nullptr,
                          last ? &tail_done : nullptr, (gq && d == 0) ? &pre : nullptr, last ? &tail_q8 : nullptr);
  }
  if (tail_done) return h;
  // (behind an int8 ff.net.2 a marked proj_out may run pinned as plan tile 19; a GroupNorm over its output then runs its own statistics pass)
  return conv(ops, p + ".proj_out", h, {.cout = x.C, .res = x.p, .keep_compressed = tail_q8});
}

// down blocks (unet.py:336-350, :389-403) + mid block (unet.py:789-795)
void UNet::down_and_mid(std::vector<Op>& ops, Tensor& h, std::vector<Tensor>& skips) {
  const int n = cfg_.n_levels;
  skips.push_back(h);
  for (int i = 0; i < n; ++i) {
    const int cout = cfg_.block_out_channels[i];
    for (int j = 0; j < cfg_.layers_per_block; ++j) {
      const std::string p = "down_blocks." + std::to_string(i);
      h = time_resnet(ops, p + ".resnets." + std::to_string(j), h, nullptr, cout);
      if (cfg_.down_cross_attn[i])
        h = transformer(ops, p + ".attentions." + std::to_string(j), h, cfg_.attention_head_dim[i],
                        cfg_.transformer_layers_per_block[i]);
      skips.push_back(h);
    }
    if (i != n - 1) {   // Downsample2D: conv 3x3 stride 2 pad 1 (unet.py:503-510)
      h = conv(ops, "down_blocks." + std::to_string(i) + ".downsamplers.0.conv", h, {.cout = cout, .k = 3, .stride = 2});
      skips.push_back(h);
    }
  }
  const int c = cfg_.block_out_channels[n - 1];
  h = time_resnet(ops, "mid_block.resnets.0", h, nullptr, c);
  // the reference passes attention_head_dim[i] with the leaked loop index == last level (unet.py:929)
  h = transformer(ops, "mid_block.attentions.0", h, cfg_.attention_head_dim[n - 1],
                  cfg_.transformer_layers_per_block[n - 1]);
  h = time_resnet(ops, "mid_block.resnets.1", h, nullptr, c);
}

void UNet::finalize_temb() {
  // one [sum Cout][temb_dim] matrix for all time_emb_proj layers (unet.py:442-444, :477)
  const int tdim = cfg_.block_out_channels[0] * 4;
  std::vector<std::string> sources;
  for (auto& [name, cout] : temb_layers_) sources.push_back(name + ".weight"), sources.push_back(name + ".bias");
  temb_w_all_ = ll_.arena.alloc_n<half_t>((size_t)temb_used_ * tdim);
  temb_b_all_ = ll_.arena.alloc_n<float>((size_t)temb_used_);
  refill(sources, temb_w_all_, [this, tdim](const WeightStore& ws) {
    std::vector<half_t> w((size_t)temb_used_ * tdim);
    std::vector<float> b(temb_used_);
    size_t row = 0;
    for (auto& [name, cout] : temb_layers_) {
      const HostTensor& tw = ws.get(name + ".weight");
      const HostTensor& tb = ws.get(name + ".bias");
      SD_REQUIRE(tw.numel() == (size_t)cout * tdim && (int)tb.numel() == cout, kInvalidArgument, "%s: bad shape",
                 name.c_str());
      for (size_t i = 0; i < (size_t)cout * tdim; ++i) w[row * tdim + i] = (half_t)tw.data[i];
      for (int i = 0; i < cout; ++i) b[row + i] = tb.data[i];
      row += cout;
    }
    SD_HIP(hipMemcpy(temb_w_all_, w.data(), w.size() * sizeof(half_t), hipMemcpyHostToDevice));
    SD_HIP(hipMemcpy(temb_b_all_, b.data(), b.size() * sizeof(float), hipMemcpyHostToDevice));
  });
}

void UNet::build_unet() {
  const int B = cfg_.batch, H = cfg_.height, W = cfg_.width, n = cfg_.n_levels;
  const int C0 = cfg_.block_out_channels[0], tdim = C0 * 4, L = cfg_.context_len;
  const bool xl = cfg_.addition_time_embed_dim > 0;
  const bool cn = cfg_.is_controlnet != 0;

  in_sample_ = ll_.arena.alloc_n<half_t>((size_t)B * cfg_.in_channels * H * W);
  in_timestep_ = ll_.arena.alloc_n<half_t>(B);
  in_ehs_ = ll_.arena.alloc_n<half_t>((size_t)B * cfg_.cross_attention_dim * L);
  tbuf_ = ll_.arena.alloc_n<float>(B);
  emb_ = ll_.arena.alloc_n<float>((size_t)B * tdim);
  temb_all_ = ll_.arena.alloc_n<float>((size_t)B * kTembCap);
  x_in_ = new_tensor(B, H, W, cfg_.in_channels);
  ctx_ = new_tensor(B, 1, L, cfg_.cross_attention_dim);

  // ---- input conversions (boundary layouts -> kernel layouts) ----
  {
    half_t* ts = in_timestep_;
    float* tb = tbuf_;
    half_t* smp = in_sample_;
    Tensor xin = x_in_;
    in_ops_.push_back([=](hipStream_t s) {
      launch_half_to_float(ts, tb, B, s);
      launch_nchw_to_nhwc(smp, 0, xin.p, B, xin.C, xin.H, xin.W, s);
    });
    in_ops_.back().label = "boundary: timestep f16->f32, sample NCHW->NHWC";
    half_t* ehs = in_ehs_;
    Tensor ctx = ctx_;
    ctx_ops_.push_back([=](hipStream_t s) { launch_bc1s_to_tokens(ehs, ctx.p, B, ctx.C, ctx.W, s); });
  }

  // ---- time embedding (unet.py:983-984; XL :1076-1088) ----
  {
    auto upload_freq = [&](int dim) {
      std::vector<float> f = timestep_freq_table(dim, cfg_.freq_shift);
      float* d = ll_.arena.alloc_n<float>(f.size());
      SD_HIP(hipMemcpy(d, f.data(), f.size() * sizeof(float), hipMemcpyHostToDevice));
      return d;
    };
    const float* freq = upload_freq(C0);
    float* t_emb = ll_.arena.alloc_n<float>((size_t)B * C0);
    float* e1 = ll_.arena.alloc_n<float>((size_t)B * tdim);
    half_t* w1 = upload_conv_weight("time_embedding.linear_1", tdim, C0, 1, false);
    float* b1 = upload_vec("time_embedding.linear_1.bias", tdim);
    half_t* w2 = upload_conv_weight("time_embedding.linear_2", tdim, tdim, 1, false);
    float* b2 = upload_vec("time_embedding.linear_2.bias", tdim);
    float* tb = tbuf_;
    float* emb = emb_;
    SD_REQUIRE(cfg_.flip_sin_to_cos == 1, kUnsupported, "flip_sin_to_cos=False is not on the path");
    time_ops_.push_back([=](hipStream_t s) {
      launch_timestep_embedding(tb, freq, t_emb, B, C0, s);
      launch_gemv(w1, b1, t_emb, C0, e1, tdim, B, tdim, C0, 0, 1, 0, s);
      launch_gemv(w2, b2, e1, tdim, emb, tdim, B, tdim, tdim, 0, 0, 0, s);
    });
    time_ops_.back().label = "time embedding: sinusoid + 2 GEMV (time_embedding.linear_1/2)";
    tpath_ = TimePath{freq, w1, w2, b1, b2, C0, tdim, !xl};
    if (xl) {
      const int nt = cfg_.num_time_ids, adim = cfg_.addition_time_embed_dim;
      const int pin = cfg_.projection_class_embeddings_input_dim;
      const int text_dim = pin - nt * adim;
      SD_REQUIRE(text_dim > 0, kInvalidArgument, "projection_class_embeddings_input_dim too small");
      in_time_ids_ = ll_.arena.alloc_n<half_t>((size_t)B * nt);
      in_text_embeds_ = ll_.arena.alloc_n<half_t>((size_t)B * text_dim);
      float* tid_f = ll_.arena.alloc_n<float>((size_t)B * nt);
      float* add_in = ll_.arena.alloc_n<float>((size_t)B * pin);   // [text_embeds | time_embeds]
      float* te = ll_.arena.alloc_n<float>((size_t)B * nt * adim);
      float* a1 = ll_.arena.alloc_n<float>((size_t)B * tdim);
      half_t* aw1 = upload_conv_weight("add_embedding.linear_1", tdim, pin, 1, false);
      float* ab1 = upload_vec("add_embedding.linear_1.bias", tdim);
      half_t* aw2 = upload_conv_weight("add_embedding.linear_2", tdim, tdim, 1, false);
      float* ab2 = upload_vec("add_embedding.linear_2.bias", tdim);
      const float* afreq = upload_freq(adim);
      half_t* tids = in_time_ids_;
      half_t* txt = in_text_embeds_;
      time_ops_.push_back([=](hipStream_t s) {
        launch_half_to_float(tids, tid_f, (size_t)B * nt, s);
        launch_timestep_embedding(tid_f, afreq, te, B * nt, adim, s);   // time_ids.flatten() (unet.py:1079)
        for (int b = 0; b < B; ++b) {   // concat([text_embeds, time_embeds], dim=-1) (unet.py:1082)
          launch_half_to_float(txt + (size_t)b * text_dim, add_in + (size_t)b * pin, text_dim, s);
          SD_HIP(hipMemcpyAsync(add_in + (size_t)b * pin + text_dim, te + (size_t)b * nt * adim,
                                (size_t)nt * adim * sizeof(float), hipMemcpyDeviceToDevice, s));
        }
        launch_gemv(aw1, ab1, add_in, pin, a1, tdim, B, tdim, pin, 0, 1, 0, s);
        launch_gemv(aw2, ab2, a1, tdim, emb, tdim, B, tdim, tdim, 0, 0, 1, s);   // emb += aug_emb (:1090)
      });
      time_ops_.back().label = "text_time add-embedding: sinusoid + concat + 2 GEMV";
    }
  }

  // ---- conv_in (unet.py:991) [+ ControlNet conditioning embedding, controlnet.py:211-215] ----
  Tensor h;
  if (cn) {
    in_cond_ = ll_.arena.alloc_n<half_t>((size_t)B * 3 * H * 8 * W * 8);
    Tensor c = new_tensor(B, H * 8, W * 8, 3);
    {
      half_t* src = in_cond_;
      Tensor cc = c;
      cond_ops_.push_back([=](hipStream_t s) { launch_nchw_to_nhwc(src, 0, cc.p, B, 3, cc.H, cc.W, s); });
    }
    const std::string p = "controlnet_cond_embedding";
    int ch = (int)ws_->get(p + ".conv_in.weight").shape[0];
    Tensor e = conv(cond_ops_, p + ".conv_in", c, {.cout = ch, .k = 3, .silu_out = true});
    for (int i = 0; ws_->has(p + ".blocks." + std::to_string(i) + ".weight"); ++i) {
      const int co = (int)ws_->get(p + ".blocks." + std::to_string(i) + ".weight").shape[0];
      e = conv(cond_ops_, p + ".blocks." + std::to_string(i), e, {.cout = co, .k = 3, .stride = 1 + (i % 2), .silu_out = true});
    }
    e = conv(cond_ops_, p + ".conv_out", e, {.cout = C0, .k = 3});
    SD_REQUIRE(e.H == H && e.W == W, kInvalidArgument, "controlnet_cond must be 8x the latent size");
    h = conv(ll_.ops, "conv_in", x_in_, {.cout = C0, .k = 3, .res = e.p});   // sample += cond
  } else {
    h = conv(ll_.ops, "conv_in", x_in_, {.cout = C0, .k = 3});
  }

  std::vector<Tensor> skips;
  down_and_mid(ll_.ops, h, skips);

  // residual shapes (controlnet.py:191-197): one per skip tensor + mid
  for (auto& t : skips) res_shapes_.push_back({t.B, t.C, t.H, t.W});
  res_shapes_.push_back({h.B, h.C, h.H, h.W});

  if (cn) {
    // zero-conv taps (controlnet.py:236-248)
    for (size_t i = 0; i < skips.size(); ++i)
      cn_out_.push_back(conv(ll_.ops, "controlnet_down_blocks." + std::to_string(i), skips[i], {.cout = skips[i].C}));
    cn_out_.push_back(conv(ll_.ops, "controlnet_mid_block", h, {.cout = h.C}));
    for (auto& t : cn_out_) {
      float* o = ll_.arena.alloc_n<float>(t.numel());
      res_out_.push_back(o);
      Tensor tt = t;
      out_ops_.push_back([=](hipStream_t s) { launch_nhwc_to_nchw_f32(tt.p, o, tt.B, tt.C, tt.H, tt.W, s); });
    }
    finalize_temb();
  } else {
    if (cfg_.support_controlnet) {   // unet.py:1009-1022
      std::vector<Tensor> added;
      for (size_t i = 0; i < res_shapes_.size(); ++i) {
        const auto& sh = res_shapes_[i];
        half_t* src = ll_.arena.alloc_n<half_t>((size_t)sh[0] * sh[1] * sh[2] * sh[3]);
        in_res_nchw_.push_back(src);
        Tensor r = new_tensor(sh[0], sh[2], sh[3], sh[1]);
        const Tensor base = (i + 1 == res_shapes_.size()) ? h : skips[i];
        Tensor sum = new_tensor(sh[0], sh[2], sh[3], sh[1]);
        ll_.ops.push_back([=](hipStream_t s) {
          if (attached_.empty()) {   // residuals arrive through the host boundary like the reference (pipeline.py:519-529)
            launch_nchw_to_nhwc(src, 0, r.p, r.B, r.C, r.H, r.W, s);
            launch_add_half(base.p, r.p, sum.p, r.numel(), s);
          } else {                   // device hand-off: skip[i] + sum over ControlNets of residual[i], one launch
            const half_t* srcs[4] = {base.p, nullptr, nullptr, nullptr};
            for (size_t k = 0; k < attached_.size(); ++k) srcs[1 + k] = attached_[k]->cn_out_[i].p;
            launch_sum_half(srcs, 1 + (int)attached_.size(), sum.p, r.numel(), s);
          }
        });
        ll_.ops.back().label = "controlnet residual add " + std::to_string(i);
        if (cn_join_pos_ < 0) cn_join_pos_ = (int)ll_.ops.size() - 1;   // first consumer of the ControlNets' outputs
        added.push_back(sum);
      }
      for (size_t i = 0; i < skips.size(); ++i) skips[i] = added[i];
      h = added.back();
    }
    // ---- up blocks (unet.py:207-225, :266-279, :1025-1041) ----
    for (int i = 0; i < n; ++i) {
      const int lvl = n - 1 - i;
      const int cout = cfg_.block_out_channels[lvl];
      const std::string p = "up_blocks." + std::to_string(i);
      for (int j = 0; j < cfg_.layers_per_block + 1; ++j) {
        Tensor skip = skips.back();
        skips.pop_back();
        h = time_resnet(ll_.ops, p + ".resnets." + std::to_string(j), h, &skip, cout);
        if (cfg_.up_cross_attn[i])
          h = transformer(ll_.ops, p + ".attentions." + std::to_string(j), h, cfg_.attention_head_dim[lvl],
                          cfg_.transformer_layers_per_block[lvl]);
      }
      if (i != n - 1)   // Upsample2D: nearest x2 fused into the conv's gather (unet.py:498-500), or folded into four 2x2 phase convs (plan tile 21)
        h = conv(ll_.ops, p + ".upsamplers.0.conv", h, {.cout = cout, .k = 3, .up = 2, .subpix = true});
    }
    SD_REQUIRE(skips.empty(), kInternal, "skip stack not empty");
    // ---- conv_norm_out -> SiLU -> conv_out (unet.py:1044-1046), fp32 NCHW at the boundary ----
    Tensor t = group_norm(ll_.ops, "conv_norm_out", h, nullptr, cfg_.norm_eps, true);
    noise_pred_ = ll_.arena.alloc_n<float>((size_t)B * cfg_.out_channels * H * W);
    float* np = noise_pred_;
    if (cfg_.out_channels <= 8 && t.C % 8 == 0) {
      conv_small_n(ll_.ops, "conv_out", t, cfg_.out_channels, nullptr, np);
    } else {
      ConvDesc d;
      d.x0 = t.p;
      d.C0 = t.C;
      d.w = upload_conv_weight("conv_out", cfg_.out_channels, t.C, 3, false);
      d.bias = upload_vec("conv_out.bias", cfg_.out_channels);
      d.B = B; d.Hi = H; d.Wi = W; d.Ho = H; d.Wo = W;
      d.ksize = 3; d.stride = 1; d.up = 1; d.N = cfg_.out_channels;
      Tensor o = new_tensor(B, H, W, cfg_.out_channels);
      d.out = o.p;
      ll_.ops.push_back([=](hipStream_t s) {
        launch_conv_generic(d, 0, s);
        launch_nhwc_to_nchw_f32(o.p, np, o.B, o.C, o.H, o.W, s);
      });
    }
    finalize_temb();
  }

  // batched time_emb_proj(SiLU(emb)) for every resnet: one GEMV per step
  {
    half_t* w = temb_w_all_;
    float* b = temb_b_all_;
    float* emb = emb_;
    float* out = temb_all_;
    const int N = temb_used_;
    time_ops_.push_back([=](hipStream_t s) { launch_gemv(w, b, emb, tdim, out, kTembCap, B, N, tdim, 1, 0, 0, s); });
    time_ops_.back().label = "time_emb_proj of all resnets: one batched GEMV N=" + std::to_string(N);
  }
  // loop state (allocated lazily on first denoise_loop)
}

// What the handle keeps between calls that weights went into: the hoisted K / V^T of the prompt (ctx_ops_) and a ControlNet's
// conditioning embedding (cond_ops_).  Their inputs are still on the device, so both are computed again from the new weights; the
// host copies the "did it change" tests compare against stay valid.
void UNet::after_reload() {
  if (have_ctx_) run_ops(ctx_ops_);
  if (have_cond_) run_ops(cond_ops_);
}

void UNet::reload_weights(const WeightStore& ws, const std::vector<std::string>& names) {
  SD_HIP(hipSetDevice(ll_.device));
  if (cn_stream_) SD_HIP(hipStreamSynchronize(cn_stream_));   // attached ControlNets run there, against this handle's inputs
  Net::reload_weights(ws, names);
}

void UNet::invalidate_graphs() {
  Net::invalidate_graphs();
  if (loop_graph_) { (void)hipGraphExecDestroy(loop_graph_); loop_graph_ = nullptr; }
}

void UNet::set_attention(int impl) {
  Net::set_attention(impl);
  for (UNet* cn : attached_) cn->set_attention(impl);   // their launches live inside this handle's graph
}

void UNet::run_main(bool with_time) {
  if (with_time) run_ops(time_ops_);
  for (size_t i = 0; i < ll_.ops.size(); ++i) {
    if (cn_forked_ && (int)i == cn_join_pos_) {   // the attached ControlNets (run_attached) are done: their residuals may be read
      SD_HIP(hipStreamWaitEvent(ll_.stream, ev_cn_join_, 0));
      cn_forked_ = false;
    }
    static const bool poison = tune_env_set("SD_POISON_LDS");
    if (poison) launch_lds_poison(ll_.stream);
    ll_.ops[i](ll_.stream);
  }
  SD_REQUIRE(!cn_forked_, kInternal, "forked ControlNets were never joined");
}

// ---- device-resident ControlNet hand-off ---------------------------------------------------------
void UNet::attach_controlnets(const std::vector<UNet*>& cns) {
  SD_REQUIRE(!cfg_.is_controlnet, kInvalidArgument, "attach_controlnets needs a UNet handle");
  SD_REQUIRE(cns.empty() || cfg_.support_controlnet, kInvalidArgument,
             "this UNet was built without support_controlnet (unet.py:1009-1022)");
  SD_REQUIRE(cns.size() <= 3, kUnsupported, "at most 3 ControlNets per UNet handle, got %zu", cns.size());
  for (UNet* cn : cns) {
    SD_REQUIRE(cn && cn->cfg_.is_controlnet, kInvalidArgument, "attach_controlnets: handle is not a ControlNet");
    SD_REQUIRE(cn->ll_.device == ll_.device, kInvalidArgument, "ControlNet lives on device %d, UNet on %d", cn->ll_.device, ll_.device);
    SD_REQUIRE(cn->cfg_.batch == cfg_.batch && cn->cfg_.height == cfg_.height && cn->cfg_.width == cfg_.width &&
                   cn->cfg_.cross_attention_dim == cfg_.cross_attention_dim && cn->cfg_.context_len == cfg_.context_len,
               kInvalidArgument, "ControlNet static shapes differ from the UNet's");
    SD_REQUIRE(cn->res_shapes_ == res_shapes_, kInvalidArgument, "ControlNet residual shapes differ from the UNet's skips");
  }
  SD_HIP(hipSetDevice(ll_.device));
  SD_HIP(hipStreamSynchronize(ll_.stream));
  // a ControlNet that leaves this handle forgets its conditioning image: re-attaching it later without a fresh
  // sd_controlnet_set_cond must fail loudly instead of running with the previous generation's image
  for (UNet* old : attached_)
    if (std::find(cns.begin(), cns.end(), old) == cns.end()) old->have_cond_ = false;
  attached_ = cns;
  for (UNet* cn : attached_) cn->set_attention(cfg_.attention_impl);
  invalidate_graphs();     // the captured launches bake in which residual sources are read
  have_ctx_ = false;       // the ControlNets' hoisted cross-attention K/V follow this handle's prompt
}

// controlnet.py:211-215: the conditioning embedding depends only on the image -> once per generation
void UNet::set_controlnet_cond(const void* cond, int flags) {
  SD_HIP(hipSetDevice(ll_.device));
  SD_REQUIRE(cfg_.is_controlnet && in_cond_, kInvalidArgument, "set_controlnet_cond needs a ControlNet handle");
  SD_REQUIRE(cond != nullptr, kInvalidArgument, "missing input 'controlnet_cond'");
  const size_t n = (size_t)cfg_.batch * 3 * cfg_.height * 8 * cfg_.width * 8;
  const bool dev = (flags & SD_FLAG_DEVICE_PTRS) != 0;
  SD_HIP(hipMemcpyAsync(in_cond_, cond, n * 2, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ll_.stream));
  run_ops(cond_ops_);
  SD_HIP(hipStreamSynchronize(ll_.stream));
  have_cond_ = true;
  if (!dev) {
    const uint16_t* src = reinterpret_cast<const uint16_t*>(cond);
    last_cond_.assign(src, src + n);
  } else {
    last_cond_.clear();
  }
}

void UNet::set_context_from(const half_t* ehs_dev, hipStream_t s) {
  const size_t n = (size_t)cfg_.batch * cfg_.cross_attention_dim * cfg_.context_len;
  SD_HIP(hipMemcpyAsync(in_ehs_, ehs_dev, n * 2, hipMemcpyDeviceToDevice, s));
  run_ops_on(ctx_ops_, s);
  have_ctx_ = true;
  last_ehs_.clear();
}

void UNet::run_as_controlnet(hipStream_t s, const half_t* x_nhwc, const float* tbuf) {
  SD_REQUIRE(have_cond_, kInvalidArgument, "ControlNet has no conditioning image: call sd_controlnet_set_cond first");
  SD_HIP(hipMemcpyAsync(x_in_.p, x_nhwc, x_in_.numel() * sizeof(half_t), hipMemcpyDeviceToDevice, s));
  SD_HIP(hipMemcpyAsync(tbuf_, tbuf, (size_t)cfg_.batch * sizeof(float), hipMemcpyDeviceToDevice, s));
  run_ops_on(time_ops_, s);
  run_ops_on(ll_.ops, s);
}

void UNet::run_attached() {
  if (attached_.empty()) return;
  if (!cn_stream_ || cn_join_pos_ < 0) {   // serial (SD_CN_CONCURRENT=0)
    for (UNet* cn : attached_) cn->run_as_controlnet(ll_.stream, x_in_.p, tbuf_);
    return;
  }
  //  a stale flag from a run that threw between the fork and the join must not survive; every attached handle is
  // checked BEFORE the fork so that the usual error - no conditioning image - cannot leave the side stream forked
  cn_forked_ = false;
  for (UNet* cn : attached_)
    SD_REQUIRE(cn->have_cond_, kInvalidArgument, "ControlNet has no conditioning image: call sd_controlnet_set_cond first");
  // fork behind the sample / timestep hand-over (everything queued on ll_.stream so far); run_main joins in front of the first residual add
  SD_HIP(hipEventRecord(ev_cn_fork_, ll_.stream));
  SD_HIP(hipStreamWaitEvent(cn_stream_, ev_cn_fork_, 0));
  try {
    for (UNet* cn : attached_) cn->run_as_controlnet(cn_stream_, x_in_.p, tbuf_);
  } catch (...) {
    // join what was forked (eagerly: the main stream waits for the side stream; under capture: the side stream re-joins the
    // capture so that hipStreamEndCapture can discard it), then let the error travel on
    (void)hipEventRecord(ev_cn_join_, cn_stream_);
    (void)hipStreamWaitEvent(ll_.stream, ev_cn_join_, 0);
    throw;
  }
  SD_HIP(hipEventRecord(ev_cn_join_, cn_stream_));
  cn_forked_ = true;
}

void UNet::upload_inputs(const sd_unet_io& io, bool loop_mode) {
  const int B = cfg_.batch, L = cfg_.context_len;
  const bool dev = (io.flags & SD_FLAG_DEVICE_PTRS) != 0;
  const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  auto copy_in = [&](void* dst, const void* src, size_t bytes, const char* what) {
    SD_REQUIRE(src != nullptr, kInvalidArgument, "missing input '%s'", what);
    SD_HIP(hipMemcpyAsync(dst, src, bytes, kind, ll_.stream));
  };
  if (!loop_mode) {
    copy_in(in_sample_, io.sample, (size_t)B * cfg_.in_channels * cfg_.height * cfg_.width * 2, "sample");
    copy_in(in_timestep_, io.timestep, (size_t)B * 2, "timestep");
  }
  if (in_time_ids_) {
    copy_in(in_time_ids_, io.time_ids, (size_t)B * cfg_.num_time_ids * 2, "time_ids");
    const int text_dim = cfg_.projection_class_embeddings_input_dim - cfg_.num_time_ids * cfg_.addition_time_embed_dim;
    copy_in(in_text_embeds_, io.text_embeds, (size_t)B * text_dim * 2, "text_embeds");
  }
  // encoder_hidden_states: re-project K/V only when the prompt embedding changed
  {
    const size_t n = (size_t)B * cfg_.cross_attention_dim * L;
    SD_REQUIRE(io.encoder_hidden_states != nullptr, kInvalidArgument, "missing input 'encoder_hidden_states'");
    bool changed = true;
    if (!dev) {
      const uint16_t* src = reinterpret_cast<const uint16_t*>(io.encoder_hidden_states);
      if (have_ctx_ && last_ehs_.size() == n && std::memcmp(last_ehs_.data(), src, n * 2) == 0) changed = false;
      if (changed) last_ehs_.assign(src, src + n);
    }
    if (changed) {
      SD_HIP(hipMemcpyAsync(in_ehs_, io.encoder_hidden_states, n * 2, kind, ll_.stream));
      run_ops(ctx_ops_);
      have_ctx_ = true;
      for (UNet* cn : attached_) cn->set_context_from(in_ehs_, ll_.stream);   // same prompt (pipeline.py:266-268)
    }
  }
  if (in_cond_) {
    const size_t n = (size_t)B * 3 * cfg_.height * 8 * cfg_.width * 8;
    SD_REQUIRE(io.controlnet_cond != nullptr, kInvalidArgument, "missing input 'controlnet_cond'");
    bool changed = true;
    if (!dev) {
      const uint16_t* src = reinterpret_cast<const uint16_t*>(io.controlnet_cond);
      if (have_cond_ && last_cond_.size() == n && std::memcmp(last_cond_.data(), src, n * 2) == 0) changed = false;
      if (changed) last_cond_.assign(src, src + n);
    }
    if (changed) {
      SD_HIP(hipMemcpyAsync(in_cond_, io.controlnet_cond, n * 2, kind, ll_.stream));
      run_ops(cond_ops_);
      have_cond_ = true;
    }
  }
  if (!in_res_nchw_.empty() && attached_.empty()) {
    SD_REQUIRE(io.additional_residuals && io.num_additional_residuals == (int)in_res_nchw_.size(), kInvalidArgument,
               "expected %zu additional_residual inputs, got %d", in_res_nchw_.size(), io.num_additional_residuals);
    for (size_t i = 0; i < in_res_nchw_.size(); ++i) {
      const auto& sh = res_shapes_[i];
      copy_in(in_res_nchw_[i], io.additional_residuals[i], (size_t)sh[0] * sh[1] * sh[2] * sh[3] * 2,
              "additional_residual");
    }
  }
  have_inputs_ = true;
}

// one forward: boundary conversions, [attached ControlNets,] time embedding, the network, [ControlNet
// boundary outputs]
void UNet::run_eager() {
  run_ops(in_ops_);
  run_attached();
  run_main(true);
  run_ops(out_ops_);
}

void UNet::forward(const sd_unet_io& io) {
  SD_HIP(hipSetDevice(ll_.device));
  upload_inputs(io, false);
  run_forward();
  const bool dev = (io.flags & SD_FLAG_DEVICE_PTRS) != 0;
  const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (cfg_.is_controlnet) {
    SD_REQUIRE(io.residual_outputs != nullptr, kInvalidArgument, "missing residual_outputs");
    for (size_t i = 0; i < res_out_.size(); ++i)
      SD_HIP(hipMemcpyAsync(io.residual_outputs[i], res_out_[i], cn_out_[i].numel() * sizeof(float), kind, ll_.stream));
  } else {
    SD_REQUIRE(io.noise_pred != nullptr, kInvalidArgument, "missing output 'noise_pred'");
    SD_HIP(hipMemcpyAsync(io.noise_pred, noise_pred_,
                          (size_t)cfg_.batch * cfg_.out_channels * cfg_.height * cfg_.width * sizeof(float), kind,
                          ll_.stream));
  }
  SD_HIP(hipStreamSynchronize(ll_.stream));
}

// pipeline.py:500-573 on the device: per step {duplicate latents + fp16 cast, [ControlNets,] UNet, CFG
// combine, scheduler update}; the host only replays one graph per step.
// Progress (StableDiffusionPipeline.swift:332-349, pipeline.py:570-573): between two replays, after every `every`-th step, the
// latents [and the de-noised tap's output] are copied to host buffers of this handle, the stream is drained and `fn` runs on the
// calling thread; fn returning 0 ends the loop behind that step.
void UNet::denoise_loop(const sd_unet_io& io, float* latents, int n_images, int n_steps, const float* timesteps,
                        const float* coef, const float* sample_scale, int history, float guidance, float* history_io,
                        float* ms_per_step, const float* pred, int every, sd_progress_fn fn, void* user, int* steps_done) {
  SD_HIP(hipSetDevice(ll_.device));
  SD_REQUIRE(!cfg_.is_controlnet, kInvalidArgument, "denoise_loop needs a UNet handle");
  const int cfgmul = guidance > 1.0f ? 2 : 1;   // pipeline.py:443
  SD_REQUIRE(cfgmul * n_images == cfg_.batch, kInvalidArgument,
             "UNet batch %d != %d images x %d (guidance_scale %s 1)", cfg_.batch, n_images, cfgmul,
             cfgmul == 2 ? ">" : "<=");
  SD_REQUIRE(cfg_.in_channels == cfg_.out_channels, kInvalidArgument, "loop needs in_channels == out_channels");
  SD_REQUIRE(history >= 0 && history <= 3 && n_steps >= 1, kInvalidArgument, "bad history (%d, max 3) / n_steps (%d)",
             history, n_steps);
  SD_REQUIRE(in_res_nchw_.empty() || !attached_.empty(), kInvalidArgument,
             "a UNet built with support_controlnet needs attached ControlNets for the device-resident loop "
             "(sd_unet_attach_controlnets); host residuals only travel through sd_unet_forward");
  const int C = cfg_.in_channels, H = cfg_.height, W = cfg_.width;
  const size_t lat_n = (size_t)n_images * C * H * W;
  const size_t hist_n = (size_t)3 * cfg_.batch * C * H * W;
  if (!latents_) {
    latents_ = ll_.arena.alloc_n<float>((size_t)cfg_.batch * C * H * W);
    eps_hist_ = ll_.arena.alloc_n<float>(hist_n);
    step_ = ll_.arena.alloc_n<int>(2);   // [0]: step counter, [1]: arrival ticket of cfg_sched_step_kernel
  }
  if (tab_cap_ < n_steps) {
    tab_cap_ = std::max(n_steps, 1024);
    tab_timesteps_ = ll_.arena.alloc_n<float>(tab_cap_);
    tab_coef_ = ll_.arena.alloc_n<float>((size_t)tab_cap_ * 8);
    tab_scale_ = ll_.arena.alloc_n<float>(tab_cap_);
    if (loop_graph_) { (void)hipGraphExecDestroy(loop_graph_); loop_graph_ = nullptr; }
  }
  upload_inputs(io, true);
  SD_HIP(hipMemcpyAsync(latents_, latents, lat_n * sizeof(float), hipMemcpyHostToDevice, ll_.stream));
  SD_HIP(hipMemcpyAsync(tab_timesteps_, timesteps, (size_t)n_steps * sizeof(float), hipMemcpyHostToDevice, ll_.stream));
  SD_HIP(hipMemcpyAsync(tab_coef_, coef, (size_t)n_steps * 8 * sizeof(float), hipMemcpyHostToDevice, ll_.stream));
  SD_HIP(hipMemsetAsync(step_, 0, 2 * sizeof(int), ll_.stream));
  SD_HIP(hipMemsetAsync(eps_hist_, 0, hist_n * sizeof(float), ll_.stream));
  if (history_io && history > 0)   // slot j: [n_images][C][H][W], continuing a loop another handle began (refiner swap)
    for (int j = 0; j < history; ++j)
      SD_HIP(hipMemcpyAsync(eps_hist_ + (size_t)j * lat_n, history_io + (size_t)j * lat_n, lat_n * sizeof(float),
                            hipMemcpyHostToDevice, ll_.stream));
  if (sample_scale)
    SD_HIP(hipMemcpyAsync(tab_scale_, sample_scale, (size_t)n_steps * sizeof(float), hipMemcpyHostToDevice, ll_.stream));
  // Time path out of the step (unet.py:703-728, :454-456): without added conditioning the embedding MLP and the batched
  // time_emb_proj depend on the timestep only, so their outputs for ALL steps of this call are computed here in one batched
  // pass (rows = steps x batch through the same GEMV kernels) and each step copies its rows inside loop_prep - four
  // dependent launches (~65 us) less per step for ~0.5 ms once per call.  Recomputed on every call: nothing is cached
  // across generations.  SDXL's text_time conditioning enters the same MLP: it keeps the in-step path.
  static const bool hoist_off = tune_env_set("SD_NO_TEMB_TABLE");   // A/B switch
  const bool hoist = !hoist_off && tpath_.ok && temb_w_all_ && temb_used_ > 0 && temb_used_ % 4 == 0;
  if (hoist) {
    const int Bt = cfg_.batch, rows = n_steps * Bt;
    if (temb_tab_cap_ < n_steps) {
      temb_tab_cap_ = std::max(n_steps, 64);
      const size_t r = (size_t)temb_tab_cap_ * Bt;
      temb_tab_ = ll_.arena.alloc_n<float>(r * kTembCap);
      tt_tab_ = ll_.arena.alloc_n<float>(r);
      tsin_tab_ = ll_.arena.alloc_n<float>(r * tpath_.c0);
      e1_tab_ = ll_.arena.alloc_n<float>(r * tpath_.tdim);
      emb_tab_ = ll_.arena.alloc_n<float>(r * tpath_.tdim);
      if (loop_graph_) { (void)hipGraphExecDestroy(loop_graph_); loop_graph_ = nullptr; }   // the table address is baked in
    }
    // every call recomputes the table (no caching across generations): one batched pass over all steps' timesteps
    std::vector<float> tt((size_t)rows);
    for (int i = 0; i < n_steps; ++i)
      for (int b = 0; b < Bt; ++b) tt[(size_t)i * Bt + b] = timesteps[i];
    SD_HIP(hipMemcpyAsync(tt_tab_, tt.data(), tt.size() * sizeof(float), hipMemcpyHostToDevice, ll_.stream));
    SD_HIP(hipStreamSynchronize(ll_.stream));   // tt is a local
    const int c0 = tpath_.c0, td = tpath_.tdim;
    launch_timestep_embedding(tt_tab_, tpath_.freq, tsin_tab_, rows, c0, ll_.stream);
    launch_gemv(tpath_.w1, tpath_.b1, tsin_tab_, c0, e1_tab_, td, rows, td, c0, 0, 1, 0, ll_.stream);
    launch_gemv(tpath_.w2, tpath_.b2, e1_tab_, td, emb_tab_, td, rows, td, td, 0, 0, 0, ll_.stream);
    launch_gemv(temb_w_all_, temb_b_all_, emb_tab_, td, temb_tab_, kTembCap, rows, temb_used_, td, 1, 0, 0, ll_.stream);
  }
  LoopTables tab{tab_timesteps_, tab_coef_, step_, sample_scale ? tab_scale_ : nullptr,
                 reinterpret_cast<unsigned*>(step_ + 1), hoist ? temb_tab_ : nullptr, temb_all_, cfg_.batch, kTembCap, temb_used_};
  if (io.step_noise) {   // ancestral samplers: the host's pre-drawn, pre-scaled noise of every step
    const size_t need = (size_t)n_steps * lat_n;
    if (noise_cap_ < need) {
      // the bump arena never frees: size the table with headroom (like the coefficient tables) so that a later call with a few
      // more steps re-uses it instead of abandoning the old block (and the captured loop graph with it)
      const size_t cap = std::max(need + need / 2, (size_t)64 * lat_n);
      noise_tab_ = ll_.arena.alloc_n<float>(cap);
      noise_cap_ = cap;
      if (loop_graph_) { (void)hipGraphExecDestroy(loop_graph_); loop_graph_ = nullptr; }   // the address is baked in
    }
    SD_HIP(hipMemcpyAsync(noise_tab_, io.step_noise, need * sizeof(float), hipMemcpyHostToDevice, ll_.stream));
    tab.noise_tab = noise_tab_;
  }
  const bool tap = pred != nullptr;
  if (tap) {   // the de-noised tap: its table and its output exist from the first call that asks for them
    if (pred_cap_ < n_steps) {
      pred_cap_ = std::max(n_steps, 1024);
      tab_pred_ = ll_.arena.alloc_n<float>((size_t)pred_cap_ * 8);
      if (!denoised_) denoised_ = ll_.arena.alloc_n<float>((size_t)cfg_.batch * C * H * W);
      if (loop_graph_) { (void)hipGraphExecDestroy(loop_graph_); loop_graph_ = nullptr; }   // the addresses are baked in
    }
    SD_HIP(hipMemcpyAsync(tab_pred_, pred, (size_t)n_steps * 8 * sizeof(float), hipMemcpyHostToDevice, ll_.stream));
    tab.pred = tab_pred_;
    tab.denoised = denoised_;
  }
  auto step_ops = [&]() {
    launch_loop_prep(latents_, x_in_.p, tbuf_, tab, n_images, C, H, W, cfgmul, ll_.stream);
    run_attached();
    run_main(!hoist);
    launch_cfg_sched_step(noise_pred_, latents_, eps_hist_, tab, guidance, n_images, C * H * W, cfgmul, history,
                          ll_.stream);
  };
  const int key = n_images * 128 + (io.step_noise ? 64 : 0) + (hoist ? 32 : 0) + (tap ? 16 : 0) + history * 4 + (cfgmul - 1) * 2 +
                  (sample_scale ? 1 : 0);
  // ms_per_step: without a handler step i runs from event i to event i + 1; with one every step has its own pair (2i, 2i + 1), so
  // that neither the snapshot copy nor the handler counts
  const bool pairs = fn != nullptr;
  std::unique_ptr<EventList> ev;
  if (ms_per_step) ev = std::make_unique<EventList>(pairs ? (size_t)n_steps * 2 : (size_t)n_steps + 1);
  if (cfg_.use_graph) {
    // guidance is baked into the captured kernel arguments -> key the graph on its bit pattern too
    int gbits;
    std::memcpy(&gbits, &guidance, 4);
    const int full_key = key ^ (gbits * 31);
    if (!loop_graph_ || loop_graph_key_ != full_key) {
      if (loop_graph_) { (void)hipGraphExecDestroy(loop_graph_); loop_graph_ = nullptr; }
      if (!ll_.graph) {   // make sure every kernel has been launched eagerly once (attributes, code objects)
        launch_loop_prep(latents_, x_in_.p, tbuf_, tab, n_images, C, H, W, cfgmul, ll_.stream);
        run_attached();
        run_main(true);
        SD_HIP(hipStreamSynchronize(ll_.stream));
      }
      loop_graph_ = capture_graph(ll_.stream, step_ops);
      loop_graph_key_ = full_key;
    }
  }
  if (fn) {
    snap_latents_.resize(lat_n);
    if (tap) snap_denoised_.resize(lat_n);
  }
  int done = n_steps;
  for (int i = 0; i < n_steps; ++i) {
    if (ms_per_step && (pairs || i == 0)) SD_HIP(hipEventRecord((*ev)[pairs ? 2 * i : 0], ll_.stream));
    if (cfg_.use_graph)
      SD_HIP(hipGraphLaunch(loop_graph_, ll_.stream));
    else
      step_ops();
    if (ms_per_step) SD_HIP(hipEventRecord((*ev)[pairs ? 2 * i + 1 : i + 1], ll_.stream));
    if (fn && i % every == 0) {   // pipeline.py:570
      SD_HIP(hipMemcpyAsync(snap_latents_.data(), latents_, lat_n * sizeof(float), hipMemcpyDeviceToHost, ll_.stream));
      if (tap) SD_HIP(hipMemcpyAsync(snap_denoised_.data(), denoised_, lat_n * sizeof(float), hipMemcpyDeviceToHost, ll_.stream));
      SD_HIP(hipStreamSynchronize(ll_.stream));
      struct Flag {   // the stream is idle: the handler may drive other handles, this one refuses (capi.cpp require_idle)
        bool& f;
        explicit Flag(bool& b) : f(b) { f = true; }
        ~Flag() { f = false; }
      };
      int go;
      {
        Flag inside(in_handler_);
        go = fn(user, i, n_steps, snap_latents_.data(), tap ? snap_denoised_.data() : nullptr);
      }
      SD_HIP(hipSetDevice(ll_.device));   // the handler may have worked on another device
      if (!go) {
        done = i + 1;
        break;
      }
    }
  }
  SD_HIP(hipMemcpyAsync(latents, latents_, lat_n * sizeof(float), hipMemcpyDeviceToHost, ll_.stream));
  if (history_io && history > 0)
    for (int j = 0; j < history; ++j)
      SD_HIP(hipMemcpyAsync(history_io + (size_t)j * lat_n, eps_hist_ + (size_t)j * lat_n, lat_n * sizeof(float),
                            hipMemcpyDeviceToHost, ll_.stream));
  SD_HIP(hipStreamSynchronize(ll_.stream));
  if (ms_per_step)
    for (int i = 0; i < done; ++i)
      SD_HIP(hipEventElapsedTime(&ms_per_step[i], (*ev)[pairs ? 2 * i : i], (*ev)[pairs ? 2 * i + 1 : i + 1]));
  if (steps_done) *steps_done = done;
}

}  // namespace sd
