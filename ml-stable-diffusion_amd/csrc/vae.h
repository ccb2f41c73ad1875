// Host-side builder/executor of the VAE decoder and encoder launch graphs (diffusers AutoencoderKL), fp16 or fp32.
// Spec: torch2coreml.py:584-594 (decoder), :739-749 (encoder); Encoder.swift:48-90.
#pragma once
#include "net.h"

struct sd_image_post;

namespace sd {

class SafetyChecker;

class Vae : public Net {
 public:
  Vae(const sd_unet_config& cfg, const WeightStore& ws, int device);   // cfg.is_vae_decoder: 1 decoder, 2 encoder

  void decode(const void* z, int z_is_f32, float* image, int flags);
  // decode, then the image post-processing on the decoder's stream (imgpost.hip): the 8-bit image and, with a checker, its
  // clip_input, which the checker reads from this handle's device memory in slices of its static batch; the flagged images are
  // zeroed in both outputs.  image / rgb8 / checker (with post, has_nsfw, concept_scores) may each be null.
  void decode_images(const void* z, int z_is_f32, float* image, uint8_t* rgb8, SafetyChecker* checker, const sd_image_post* post,
                     float adjustment, float* has_nsfw, float* concept_scores, int flags);
  void encode(const void* x, int x_is_f32, float* moments, int flags);
  // image-to-image start: the encoder's launch list, then launch_posterior_noise on the moments where the list leaves them
  void encode_latents(const void* x, int x_is_f32, const float* eps, const float* noise, int n_images, float scale_factor,
                      float sa, float sb, float* latents, int flags);

 private:
  void build_decoder();
  void build_encoder();
  Tensor attention(std::vector<Op>& ops, const std::string& p, const Tensor& h);
  void upload_image(const void* x, int x_is_f32, hipMemcpyKind kind);
  void upload_latents(const void* z, int z_is_f32, bool dev);

  float* in_z_ = nullptr;           // decoder: latent input NCHW f32
  half_t* z_half_ = nullptr;
  float* image_ = nullptr;          // decoded image NCHW f32 (encoder: the moments NCHW f32)
  size_t image_elems_ = 0;
  void* in_x_ = nullptr;            // encoder: input image NCHW (f16 or f32)
  int vae_in_f32_ = 0;
  float *enc_eps_ = nullptr, *enc_noise_ = nullptr, *enc_latents_ = nullptr;   // encode_latents: (n), (images, n), (images, n)
  int enc_images_cap_ = 0;
  // decode_images, allocated on first use: the 8-bit image (B, H, W, 3), the checker's input (B, 3, S, S) and the resize tables of
  // the last geometry (the arena does not recycle: a caller that alternates geometries grows it)
  uint8_t* rgb8_ = nullptr;
  half_t* clip_input_ = nullptr;
  size_t clip_input_cap_ = 0;
  int post_rh_ = 0, post_rw_ = 0, post_S_ = 0;
  ClipInputDesc post_desc_{};
  size_t post_lds_ = 0;
};

}  // namespace sd
