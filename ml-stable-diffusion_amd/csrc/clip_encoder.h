// The transformer stack the two CLIP towers share (transformers' CLIPEncoder: the text encoder's and the safety checker's
// vision tower's), as launches appended to a handle's list, and the one statement of which checkpoint tensors it reads.
#pragma once
#include "launch_list.h"

namespace sd {

struct ClipStack {
  std::string prefix;   // checkpoint keys are prefix + "<layer>." + ...: "text_model.encoder.layers."
  int L = 0;            // layers
  int M = 0;            // rows of the activation matrix (tokens x batch)
  int D = 0, I = 0;     // hidden / intermediate size
  int act = 0;          // launch_clip_act: 0 quick_gelu, 1 gelu
  float eps = 1e-5f;
  const char* what = "";   // names the handle in error texts
};

// Every tensor the stack reads, with the element count the config implies: host only, so a handle calls it before it opens a
// device.  kNotFound for a missing tensor, kInvalidArgument for a wrong size; the message names the tensor.
void check_clip_stack_weights(const WeightStore& ws, const ClipStack& c);
void check_numel(const WeightStore& ws, const std::string& name, size_t numel);   // the same check for one tensor

// Appends L x [LN1 -> stacked q|k|v GEMM -> attention -> out_proj + residual -> LN2 -> fc1 -> activation -> fc2 + residual]
// over x [M][D] to `h`; `attention` launches the tower's attention kernel on qkv [M][3D] -> att [M][D].  Returns the output
// [M][D]; *last_input (when asked for) is the input of the last layer - hidden_states[-2] of the tower.
using ClipAttention = std::function<void(const half_t* qkv, half_t* att, hipStream_t s)>;
half_t* build_clip_stack(LaunchList& h, const WeightStore& ws, const ClipStack& c, half_t* x, const ClipAttention& attention,
                         half_t** last_input = nullptr);

}  // namespace sd
