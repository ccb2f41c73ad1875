// The safety checker's handle class (safety_checker.cpp), visible to the entry points that feed it from another handle's device
// memory (sd_vae_decode_images).
#pragma once
#include "../../include/sd_mi355x.h"
#include "clip_encoder.h"

namespace sd {

class SafetyChecker : LaunchList {
 public:
  SafetyChecker(const sd_safety_checker_config& cfg, const WeightStore& ws, int device);
  ~SafetyChecker();
  void run(const void* clip_input, float adjustment, float* has_nsfw, float* concept_scores, float* image_embeds,
           float* last_hidden_state, int flags);
  size_t device_bytes() const { return arena.bytes(); }
  const sd_safety_checker_config& config() const { return cfg_; }
  int device_index() const { return device; }
  float last_ms() const { return last_ms_; }

 private:
  sd_safety_checker_config cfg_;
  int S_ = 0;
  hipEvent_t e0_ = nullptr, e1_ = nullptr;   // around the launch list of a run
  float last_ms_ = 0.f;
  half_t* input_ = nullptr;       // clip_input (B, 3, I, I)
  float* adjustment_ = nullptr;   // one float: rewritten in front of every run, read by the head
  float* hidden_f32_ = nullptr;   // encoder output (B, S, D), before post_layernorm
  float* embeds_ = nullptr;       // (B, P)
  float* scores_ = nullptr;       // (B, num_concepts)
  float* flags_ = nullptr;        // (B)
};

}  // namespace sd

struct sd_safety_checker {
  std::unique_ptr<sd::SafetyChecker> impl;
};
