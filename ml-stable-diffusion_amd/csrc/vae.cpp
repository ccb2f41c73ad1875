// AutoencoderKL decoder / encoder as static launch graphs of the gfx950 kernels, built from the blocks of net.cpp.
// Both reuse the UNet config struct; all GroupNorm eps = 1e-6, no time embedding.
#include "vae.h"

#include <algorithm>
#include <cmath>

#include "conv_plan.h"
#include "safety_checker.h"

namespace sd {

Vae::Vae(const sd_unet_config& cfg, const WeightStore& ws, int device) : Net(cfg, ws, device) {
  cfg_.norm_eps = 1e-6f;
  if (cfg_.is_vae_decoder == 2)
    build_encoder();
  else
    build_decoder();
  seal();
}

// AutoencoderKL mid-block attention: single head over S = H*W tokens, head dim = C (512 for every SD / SDXL VAE).  Two fp16 routes:
//   S <= 8192 and S % 64 == 0   scores and P materialised per image (S x S fp16) through the GEMM kernel and the row softmax,
//                               three launches per image - every size the benchmarks and goldens were recorded at
//   any other S                 vae_attention.hip: one streaming launch for the whole batch, no score matrix and no V^T copy
//                               (768^2 / 1024^2 images: S = 9216 / 16384; 480^2: S = 3600)
// fp32 handles keep the materialised fp32 steps at any S.
Tensor Vae::attention(std::vector<Op>& ops, const std::string& p, const Tensor& h) {
  const int B = h.B, H = h.H, W = h.W, C = h.C, S = H * W;
  Tensor t0 = group_norm(ops, p + ".group_norm", h, nullptr, 1e-6f, false);
  Tensor q = conv(ops, p + ".to_q", t0, {.cout = C});
  Tensor k = conv(ops, p + ".to_k", t0, {.cout = C});
  const float scale = 1.0f / std::sqrt((float)C);
  if (f32_) {   // the same three steps on the fp32 kernels: K tokens / V play the weight matrices
    Tensor v = conv(ops, p + ".to_v", t0, {.cout = C});
    float* scores = ll_.arena.alloc_n<float>((size_t)S * S);
    Tensor a = new_tensor(B, H, W, C);
    for (int b = 0; b < B; ++b) {
      ConvF32Desc d1;   // scores[q][k] = sum_c Q[q][c] K[k][c]
      d1.x = q.f() + (size_t)b * S * C;
      d1.w = k.f() + (size_t)b * S * C;
      d1.w_kind = 1;
      d1.out = scores;
      d1.B = 1; d1.Hi = 1; d1.Wi = S; d1.Cin = C; d1.Ho = 1; d1.Wo = S; d1.N = S;
      ConvF32Desc d2;   // out[q][c] = sum_k P[q][k] V[k][c]
      d2.x = scores;
      d2.w = v.f() + (size_t)b * S * C;
      d2.w_kind = 2;
      d2.out = a.f() + (size_t)b * S * C;
      d2.B = 1; d2.Hi = 1; d2.Wi = S; d2.Cin = S; d2.Ho = 1; d2.Wo = S; d2.N = C;
      ops.push_back([d1, d2, scores, S, scale](hipStream_t s) {
        launch_conv_f32(d1, s);
        launch_row_softmax_f32(scores, S, S, scale, s);
        launch_conv_f32(d2, s);
      });
      ops.back().label = "VAE attention fp32: QK^T GEMM + row softmax + PV GEMM, S=" + std::to_string(S);
      ops.back().flop = 4.0 * (double)S * S * C;
    }
    return conv(ops, p + ".to_out.0", a, {.cout = C, .res = h.p});
  }
  if (S > 8192 || S % 64 != 0) {   // what the materialised route cannot take: the streaming kernel, one op for the whole batch
    SD_REQUIRE(vae_attention_ok(C), kUnsupported,
               "VAE attention over %d tokens: mid-block width %d (the streaming kernel is built for head dims 64, 128, 256 and 512)", S, C);
    Tensor v = conv(ops, p + ".to_v", t0, {.cout = C});
    Tensor a = new_tensor(B, H, W, C);
    ops.push_back([=](hipStream_t s) { launch_vae_attention(q.p, k.p, v.p, a.p, B, S, C, s); });
    ops.back().label = "VAE attention: streaming QK^T + softmax + PV, one launch, S=" + std::to_string(S);
    ops.back().flop = 4.0 * (double)S * S * C * B;
    return conv(ops, p + ".to_out.0", a, {.cout = C, .res = h.p});
  }
  SD_REQUIRE(C % 64 == 0, kUnsupported, "VAE attention needs C %% 64 == 0");
  Tensor vt = conv(ops, p + ".to_v", t0, {.cout = C, .out_mode = kOutHalfT, .ldT = S});
  half_t* scores = ll_.arena.alloc_n<half_t>((size_t)S * S);
  Tensor a = new_tensor(B, H, W, C);
  for (int b = 0; b < B; ++b) {
    ConvDesc d1;   // scores[q][k] = sum_c Q[q][c] K[k][c]   (K tokens play the role of the weight matrix)
    d1.x0 = q.p + (size_t)b * S * C; d1.C0 = C; d1.w = k.p + (size_t)b * S * C;
    d1.out = scores; d1.B = 1; d1.Hi = 1; d1.Wi = S; d1.Ho = 1; d1.Wo = S; d1.N = S;
    ConvDesc d2;   // out[q][c] = sum_k P[q][k] V^T[c][k]
    d2.x0 = scores; d2.C0 = S; d2.w = vt.p + (size_t)b * C * S;
    d2.out = a.p + (size_t)b * S * C; d2.B = 1; d2.Hi = 1; d2.Wi = S; d2.Ho = 1; d2.Wo = S; d2.N = C;
    ll_.ws_need = std::max(ll_.ws_need, std::max(conv_workspace_bytes(d1), conv_workspace_bytes(d2)));
    ops.push_back([this, d1, d2, scores, S, scale](hipStream_t s) {
      launch_conv(d1, ll_.ws_conv, s);
      launch_row_softmax(scores, S, S, scale, s);
      launch_conv(d2, ll_.ws_conv, s);
    });
    ops.back().label = "VAE attention: QK^T GEMM + row softmax + PV GEMM, S=" + std::to_string(S);
    ops.back().flop = 4.0 * (double)S * S * C;
  }
  return conv(ops, p + ".to_out.0", a, {.cout = C, .res = h.p});
}

// ---------------------------------------------------------------------------------------------
// VAE decoder (diffusers AutoencoderKL.decode, wrapped by the reference in
// torch2coreml.py:584-594: image = decoder(post_quant_conv(z)); called from pipeline.py:313-320).
// Third-party arithmetic restated from the public architecture:
//   post_quant_conv 1x1 -> conv_in 3x3 -> mid [ResNet, 1-head self-attention, ResNet]
//   -> up blocks (3 ResNets each, nearest-x2 + conv3x3 after all but the last)
//   -> GroupNorm(32, 1e-6) -> SiLU -> conv_out 3x3.   All GroupNorm eps = 1e-6, no time embedding.
// Reuses the UNet config struct: block_out_channels = decoder channels in ENCODER order
// (SD: 128,256,512,512), layers_per_block = 2 (decoder uses +1), in_channels = latent channels,
// out_channels = 3, height/width = latent size.
// ---------------------------------------------------------------------------------------------
void Vae::build_decoder() {
  const int B = cfg_.batch, H = cfg_.height, W = cfg_.width, n = cfg_.n_levels;
  const int Cz = cfg_.in_channels;
  std::vector<Op>& ops = ll_.ops;
  in_z_ = ll_.arena.alloc_n<float>((size_t)B * Cz * H * W);
  Tensor z = new_tensor(B, H, W, Cz);
  {
    float* src = in_z_;
    if (f32_) ops.push_back([=](hipStream_t s) { launch_nchw_to_nhwc_f32(src, 1, z.f(), B, Cz, H, W, s); });
    else ops.push_back([=](hipStream_t s) { launch_nchw_to_nhwc(src, 1, z.p, B, Cz, H, W, s); });
  }
  Tensor h = conv(ops, "post_quant_conv", z, {.cout = Cz});
  const int Ctop = cfg_.block_out_channels[n - 1];
  h = conv(ops, "decoder.conv_in", h, {.cout = Ctop, .k = 3});
  h = resnet(ops, "decoder.mid_block.resnets.0", h, nullptr, Ctop, nullptr);
  h = attention(ops, "decoder.mid_block.attentions.0", h);
  h = resnet(ops, "decoder.mid_block.resnets.1", h, nullptr, Ctop, nullptr);
  for (int i = 0; i < n; ++i) {
    const int cout = cfg_.block_out_channels[n - 1 - i];
    const std::string p = "decoder.up_blocks." + std::to_string(i);
    for (int j = 0; j < cfg_.layers_per_block + 1; ++j)
      h = resnet(ops, p + ".resnets." + std::to_string(j), h, nullptr, cout, nullptr);
    if (i != n - 1) h = conv(ops, p + ".upsamplers.0.conv", h, {.cout = cout, .k = 3, .up = 2});
  }
  Tensor t = group_norm(ops, "decoder.conv_norm_out", h, nullptr, 1e-6f, true);
  // conv_out 3x3 -> 3 channels: one wavefront per pixel, written straight as fp32 NCHW
  SD_REQUIRE(cfg_.out_channels <= 8 && t.C % 8 == 0, kUnsupported, "VAE conv_out: %d -> %d channels", t.C,
             cfg_.out_channels);
  image_elems_ = (size_t)t.B * cfg_.out_channels * t.H * t.W;
  image_ = ll_.arena.alloc_n<float>(image_elems_);
  conv_small_n(ops, "decoder.conv_out", t, cfg_.out_channels, nullptr, image_);
}

void Vae::upload_latents(const void* z, int z_is_f32, bool dev) {
  hipStream_t stream = ll_.stream;
  const size_t n = (size_t)cfg_.batch * cfg_.in_channels * cfg_.height * cfg_.width;
  if (z_is_f32) {
    SD_HIP(hipMemcpyAsync(in_z_, z, n * 4, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
  } else {
    if (!z_half_) z_half_ = ll_.arena.alloc_n<half_t>(n);
    SD_HIP(hipMemcpyAsync(z_half_, z, n * 2, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
    launch_half_to_float(z_half_, in_z_, n, stream);
  }
}

// pipeline.py:313-320 hands z = latents / scaling_factor (fp16 or fp32); returns image in [-1, 1]
void Vae::decode(const void* z, int z_is_f32, float* image, int flags) {
  SD_HIP(hipSetDevice(ll_.device));
  hipStream_t stream = ll_.stream;
  const bool dev = (flags & SD_FLAG_DEVICE_PTRS) != 0;
  upload_latents(z, z_is_f32, dev);
  run_forward();
  SD_HIP(hipMemcpyAsync(image, image_, image_elems_ * sizeof(float),
                        dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream));
  SD_HIP(hipStreamSynchronize(stream));
  have_inputs_ = true;
}

// pipeline.py:286-320 behind the decoder's launch list, without the detour through the host: numpy_to_pil's quantisation, then - with a
// checker - CLIPImageProcessor's resize / crop / normalise, the checker itself (SafetyChecker::run on device pointers, in slices of its
// static batch) and filtered_images (torch2coreml.py:1203-1207): the flagged images zeroed in both outputs.
void Vae::decode_images(const void* z, int z_is_f32, float* image, uint8_t* rgb8, SafetyChecker* checker, const sd_image_post* post,
                        float adjustment, float* has_nsfw, float* concept_scores, int flags) {
  const int B = cfg_.batch, C = cfg_.out_channels;
  const int H = cfg_.height << (cfg_.n_levels - 1), W = cfg_.width << (cfg_.n_levels - 1);   // n_levels - 1 upsamplers
  SD_REQUIRE((flags & ~SD_FLAG_DEVICE_PTRS) == 0, kInvalidArgument, "unknown flags %d", flags);
  SD_REQUIRE(C == 3 && image_elems_ == (size_t)B * 3 * H * W, kUnsupported, "decode_images: the decoder writes %zu floats, 8-bit RGB needs %d x 3 x %d x %d",
             image_elems_, B, H, W);
  // everything that can be refused is refused here, before any device work
  ClipInputPlan plan;
  int cb = 0, S = 0, NC = 0;
  if (checker) {
    const sd_safety_checker_config& cc = checker->config();
    cb = cc.batch, S = cc.image_size, NC = cc.num_concepts;
    SD_REQUIRE(post != nullptr, kInvalidArgument, "decode_images: a checker needs the sd_image_post that describes its input");
    SD_REQUIRE(B % cb == 0, kInvalidArgument, "decode_images: the decoder's batch %d is no multiple of the safety checker's %d", B, cb);
    SD_REQUIRE(checker->device_index() == ll_.device, kInvalidArgument, "decode_images: the decoder is on device %d, the safety checker on %d",
               ll_.device, checker->device_index());
    for (int c = 0; c < 3; ++c)
      SD_REQUIRE(post->image_std[c] != 0.f, kInvalidArgument, "decode_images: image_std[%d] is 0", c);
    if (post->resize_h != post_rh_ || post->resize_w != post_rw_ || S != post_S_) plan = plan_clip_input(H, W, post->resize_h, post->resize_w, S);
  }
  SD_HIP(hipSetDevice(ll_.device));
  hipStream_t stream = ll_.stream;
  const bool dev = (flags & SD_FLAG_DEVICE_PTRS) != 0;
  const hipMemcpyKind out_kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  const size_t px = (size_t)H * W;
  upload_latents(z, z_is_f32, dev);
  run_forward();
  if (rgb8 || checker) {
    if (!rgb8_) rgb8_ = ll_.arena.alloc_n<uint8_t>((size_t)B * px * 3);
    launch_image_rgb8(image_, rgb8_, B, H, W, stream);
  }
  if (checker) {
    if (plan.S) {   // a new geometry: its tables into the arena
      auto up = [&](const std::vector<int32_t>& v) {
        int32_t* d = ll_.arena.alloc_n<int32_t>(v.size());
        SD_HIP(hipMemcpyAsync(d, v.data(), v.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
        return d;
      };
      post_desc_.hbounds = up(plan.hbounds), post_desc_.hcoeffs = up(plan.hcoeffs);
      post_desc_.vbounds = up(plan.vbounds), post_desc_.vcoeffs = up(plan.vcoeffs);
      SD_HIP(hipStreamSynchronize(stream));   // `plan` lives on this frame
      post_desc_.H = H, post_desc_.W = W, post_desc_.S = S;
      post_desc_.top = (plan.rh - S) / 2, post_desc_.left = (plan.rw - S) / 2;
      post_desc_.ksh = plan.ksh, post_desc_.ksv = plan.ksv;
      post_lds_ = plan.lds_bytes;
      post_rh_ = plan.rh, post_rw_ = plan.rw, post_S_ = S;
    }
    const size_t per_image = (size_t)3 * S * S;
    if (clip_input_cap_ < B * per_image) {
      clip_input_ = ll_.arena.alloc_n<half_t>(B * per_image);
      clip_input_cap_ = B * per_image;
    }
    ClipInputDesc d = post_desc_;
    for (int c = 0; c < 3; ++c) d.mean[c] = post->image_mean[c], d.std[c] = post->image_std[c];
    launch_clip_input(rgb8_, clip_input_, B, d, post_lds_, stream);
    SD_HIP(hipStreamSynchronize(stream));   // the checker runs on its own stream
    std::vector<float> verdict(B);
    for (int i = 0; i < B; i += cb)
      checker->run(clip_input_ + i * per_image, adjustment, verdict.data() + i, concept_scores ? concept_scores + (size_t)i * NC : nullptr,
                   nullptr, nullptr, SD_FLAG_DEVICE_PTRS);
    SD_HIP(hipSetDevice(ll_.device));
    for (int i = 0; i < B; ++i) {
      if (has_nsfw) has_nsfw[i] = verdict[i];
      if (verdict[i] > 0.5f) {   // the next forward rewrites image_, so zeroing it in place loses nothing
        if (image) SD_HIP(hipMemsetAsync(image_ + i * px * 3, 0, px * 3 * sizeof(float), stream));
        if (rgb8) SD_HIP(hipMemsetAsync(rgb8_ + i * px * 3, 0, px * 3, stream));
      }
    }
  }
  if (image) SD_HIP(hipMemcpyAsync(image, image_, image_elems_ * sizeof(float), out_kind, stream));
  if (rgb8) SD_HIP(hipMemcpyAsync(rgb8, rgb8_, (size_t)B * px * 3, out_kind, stream));
  SD_HIP(hipStreamSynchronize(stream));
  have_inputs_ = true;
}

// ---------------------------------------------------------------------------------------------
// VAE encoder (diffusers AutoencoderKL.encode up to the moments; the reference wraps it as
// latent = quant_conv(encoder(x)), torch2coreml.py:739-749, and samples / scales in Encoder.swift:48-90).
// Third-party arithmetic restated from the public architecture:
//   conv_in 3x3 (3 -> C0) -> down blocks (layers_per_block ResNets, then conv3x3 stride 2 on F.pad(x, (0,1,0,1)) in
//   all but the last) -> mid [ResNet, 1-head self-attention, ResNet] -> GroupNorm(32, 1e-6) -> SiLU -> conv_out 3x3
//   (-> 2 * latent channels) -> quant_conv 1x1.   Config: block_out_channels in encoder order, in_channels = 3,
//   out_channels = 2 * latent channels, height / width = IMAGE size.  Output: moments (B, 2*Cz, H/8, W/8) f32.
// ---------------------------------------------------------------------------------------------
void Vae::build_encoder() {
  const int B = cfg_.batch, H = cfg_.height, W = cfg_.width, n = cfg_.n_levels;
  const int Cm = cfg_.out_channels;
  std::vector<Op>& ops = ll_.ops;
  SD_REQUIRE(cfg_.in_channels == 3 && Cm >= 2 && Cm <= 8, kUnsupported, "VAE encoder: %d -> %d channels", cfg_.in_channels, Cm);
  in_x_ = ll_.arena.alloc((size_t)B * 3 * H * W * 4);
  Tensor x = new_tensor(B, H, W, 3);
  {
    void* src = in_x_;
    Vae* self = this;
    if (f32_) ops.push_back([=](hipStream_t s) { launch_nchw_to_nhwc_f32(src, self->vae_in_f32_, x.f(), B, 3, H, W, s); });
    else ops.push_back([=](hipStream_t s) { launch_nchw_to_nhwc(src, self->vae_in_f32_, x.p, B, 3, H, W, s); });
    ops.back().label = "boundary: image NCHW -> NHWC";
  }
  Tensor h = conv(ops, "encoder.conv_in", x, {.cout = cfg_.block_out_channels[0], .k = 3});
  for (int i = 0; i < n; ++i) {
    const int cout = cfg_.block_out_channels[i];
    const std::string p = "encoder.down_blocks." + std::to_string(i);
    for (int j = 0; j < cfg_.layers_per_block; ++j)
      h = resnet(ops, p + ".resnets." + std::to_string(j), h, nullptr, cout, nullptr);
    if (i != n - 1) h = conv(ops, p + ".downsamplers.0.conv", h, {.cout = cout, .k = 3, .stride = 2, .pad = 0});
  }
  const int Ctop = cfg_.block_out_channels[n - 1];
  h = resnet(ops, "encoder.mid_block.resnets.0", h, nullptr, Ctop, nullptr);
  h = attention(ops, "encoder.mid_block.attentions.0", h);
  h = resnet(ops, "encoder.mid_block.resnets.1", h, nullptr, Ctop, nullptr);
  Tensor t = group_norm(ops, "encoder.conv_norm_out", h, nullptr, 1e-6f, true);
  SD_REQUIRE(t.C % 8 == 0, kUnsupported, "VAE encoder conv_out: %d input channels", t.C);
  Tensor m = new_tensor(t.B, t.H, t.W, Cm);
  conv_small_n(ops, "encoder.conv_out", t, Cm, m.p, nullptr);
  ops.back().flop = 0;   // this op has never reported a FLOP count; the profile tools' totals stay comparable
  Tensor q = conv(ops, "quant_conv", m, {.cout = Cm});
  image_elems_ = q.numel();
  image_ = ll_.arena.alloc_n<float>(image_elems_);
  {
    float* dst = image_;
    if (f32_) ops.push_back([=](hipStream_t s) { launch_nhwc_to_nchw_f32f32(q.f(), dst, q.B, q.C, q.H, q.W, s); });
    else ops.push_back([=](hipStream_t s) { launch_nhwc_to_nchw_f32(q.p, dst, q.B, q.C, q.H, q.W, s); });
    ops.back().label = "boundary: moments NHWC -> NCHW fp32";
  }
}

void Vae::upload_image(const void* x, int x_is_f32, hipMemcpyKind kind) {
  if ((x_is_f32 != 0) != (vae_in_f32_ != 0)) {   // the captured boundary kernel bakes the input dtype in
    vae_in_f32_ = x_is_f32 ? 1 : 0;
    invalidate_graphs();
  }
  const size_t n = (size_t)cfg_.batch * 3 * cfg_.height * cfg_.width;
  SD_HIP(hipMemcpyAsync(in_x_, x, n * (x_is_f32 ? 4 : 2), kind, ll_.stream));
}

void Vae::encode(const void* x, int x_is_f32, float* moments, int flags) {
  SD_HIP(hipSetDevice(ll_.device));
  const bool dev = (flags & SD_FLAG_DEVICE_PTRS) != 0;
  upload_image(x, x_is_f32, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
  run_forward();
  SD_HIP(hipMemcpyAsync(moments, image_, image_elems_ * sizeof(float), dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                        ll_.stream));
  SD_HIP(hipStreamSynchronize(ll_.stream));
  have_inputs_ = true;
}

// generateLatentSamples + Encoder.encode + Scheduler.addNoise (StableDiffusionPipeline.swift:361-379, Encoder.swift:68-89,
// Scheduler.swift:83-102) behind the encoder graph: the moments stay in image_, one more launch on the same stream turns them
// into the n_images noised starting latents.  The random numbers (eps, noise) are the host's, as everywhere in the library.
void Vae::encode_latents(const void* x, int x_is_f32, const float* eps, const float* noise, int n_images, float scale_factor,
                         float sa, float sb, float* latents, int flags) {
  SD_REQUIRE(cfg_.batch == 1 && cfg_.out_channels % 2 == 0, kInvalidArgument,
             "encode_latents: the encoder handle must have batch 1 (one starting image feeds every latent), got %d", cfg_.batch);
  SD_HIP(hipSetDevice(ll_.device));
  hipStream_t stream = ll_.stream;
  const bool dev = (flags & SD_FLAG_DEVICE_PTRS) != 0;
  const hipMemcpyKind in_kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  const size_t n = image_elems_ / 2;   // Cz * h * w
  if (enc_images_cap_ < n_images) {
    enc_eps_ = enc_eps_ ? enc_eps_ : ll_.arena.alloc_n<float>(n);
    enc_noise_ = ll_.arena.alloc_n<float>((size_t)n_images * n);
    enc_latents_ = ll_.arena.alloc_n<float>((size_t)n_images * n);
    enc_images_cap_ = n_images;
  }
  upload_image(x, x_is_f32, in_kind);
  SD_HIP(hipMemcpyAsync(enc_eps_, eps, n * sizeof(float), in_kind, stream));
  SD_HIP(hipMemcpyAsync(enc_noise_, noise, (size_t)n_images * n * sizeof(float), in_kind, stream));
  run_forward();
  launch_posterior_noise(image_, enc_eps_, enc_noise_, enc_latents_, n, n_images, scale_factor, sa, sb, stream);
  SD_HIP(hipMemcpyAsync(latents, enc_latents_, (size_t)n_images * n * sizeof(float),
                        dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream));
  SD_HIP(hipStreamSynchronize(stream));
  have_inputs_ = true;
}

}  // namespace sd
