// Host-side builder/executor of the UNet (and ControlNet) launch graph.
// Spec: python_coreml_stable_diffusion/unet.py:798-1152, controlnet.py:49-250.
#pragma once
#include "net.h"

namespace sd {

// Self-attention operands of a transformer block written ahead of it (UNet::transformer's one-launch head, xattn_out.hip gn_proj_qkv_kernel)
struct PreQkv {
  Tensor qk;               // [M][2C]: q | k
  half_t* vt = nullptr;    // [B][C][round_up(S, 8)]
  bool vt_perm = false;    // V^T in attention8's key order
  bool q_pre = false;      // queries carry d^-0.5 * log2(e)
};

class UNet : public Net {
 public:
  UNet(const sd_unet_config& cfg, const WeightStore& ws, int device);
  ~UNet() override;

  void forward(const sd_unet_io& io);
  // pred / every / fn / user / steps_done: the progress handler of sd_unet_denoise_loop_progress (include/sd_mi355x.h); fn == null:
  // sd_unet_denoise_loop
  void denoise_loop(const sd_unet_io& io, float* latents, int n_images, int n_steps, const float* timesteps,
                    const float* coef, const float* sample_scale, int history, float guidance, float* history_io,
                    float* ms_per_step, const float* pred = nullptr, int every = 1, sd_progress_fn fn = nullptr,
                    void* user = nullptr, int* steps_done = nullptr);
  bool in_progress_handler() const { return in_handler_; }   // the loop is inside its caller's handler: the handle takes no other call
  // device-resident ControlNet hand-off (pipeline.py:259-284, unet.py:1009-1022): this UNet reads the
  // residual tensors of the attached ControlNet handles straight from HBM and sums them on the device
  void attach_controlnets(const std::vector<UNet*>& cns);
  void set_controlnet_cond(const void* cond, int flags);
  void set_attention(int impl) override;
  void reload_weights(const WeightStore& ws, const std::vector<std::string>& names) override;
  int num_residuals() const { return (int)res_shapes_.size(); }

 private:
  // ---- build ----
  void build_unet();
  // LayerNorm `ln` folded into the bias-free/biased 1x1 projections `names` (stacked along Cout) that
  // consume it: returns w' = W*gamma (fp16), colsum of w', bias' = b + W.beta
  struct LnFold {
    half_t* w;
    float* colsum;
    float* bias;
  };
  // upload_w = false: the folded fp16 matrix stays a host temporary (f.w null): the projection runs from its palette
  LnFold fold_layernorm(const std::string& ln, const std::vector<std::string>& names, int cin, int cout_each,
                        bool geglu, bool upload_w = true);
  bool can_fold_ln(const Tensor& x, int cout, bool geglu) const;
  Tensor conv_stacked(std::vector<Op>& ops, const std::vector<std::string>& names, const Tensor& x, int cout_each);
  Tensor layer_norm(std::vector<Op>& ops, const std::string& name, const Tensor& x);
  Tensor time_resnet(std::vector<Op>& ops, const std::string& p, const Tensor& x, const Tensor* x2, int cout);
  Tensor transformer(std::vector<Op>& ops, const std::string& p, const Tensor& x, int heads, int depth);
  // proj_out / tres (last block of a SpatialTransformer only): the transformer's proj_out and its residual - where the tail
  // ff.net.2 + residual -> proj_out + residual runs as ONE launch (xattn_out.hip ffn_proj_kernel) *tail_done is set and the returned
  // tensor is the transformer's output.  pre: the block's self-attention operands where the transformer's head launch already wrote them.
  // *tail_q8 is set where a W8A8-marked ff.net.2 ran un-merged from int8 activations (plan tile 24): proj_out is then a launch of its own
  Tensor transformer_block(std::vector<Op>& ops, const std::string& b, const Tensor& h, int heads, const std::string* proj_out = nullptr,
                           const Tensor* tres = nullptr, bool* tail_done = nullptr, const PreQkv* pre = nullptr, bool* tail_q8 = nullptr);
  Tensor attention(std::vector<Op>& ops, const Tensor& q, const half_t* k, const half_t* vt, int heads, int Sq,
                   int Sk, int ldk, int ldv, int ldq, bool vt_perm = false, bool q_prescaled = false, const std::string* einsum = nullptr);
  // (einsum: the attention's Einsum module, <block>.attn1.einsum, where the launch is a self-attention over a fused q | k buffer: a
  // W8A8 mark on it - WeightStore::quantize_einsum - makes the launch the quantizer + the int8 attention where attention8 would run and
  // attention_i8_shape_ok holds; an observing store with observe_einsums puts launch_einsum_absmax in front of it)
  // scratch of attention8's balanced form (AttnDesc::sk_part / sk_cnt), shared by this handle's self-attention launches
  float* sk_part_ = nullptr;
  size_t sk_part_bytes_ = 0;
  unsigned* sk_cnt_ = nullptr;
  int sk_cnt_n_ = 0;
  void down_and_mid(std::vector<Op>& ops, Tensor& h, std::vector<Tensor>& skips);
  const float* register_temb(const std::string& name, int cout);
  void finalize_temb();
  void upload_inputs(const sd_unet_io& io, bool loop_mode);
  // ControlNet handle driven by a UNet handle: sample / timesteps come from the UNet's device buffers,
  // everything runs on the UNet's stream (and inside its HIP graph)
  void run_as_controlnet(hipStream_t s, const half_t* x_nhwc, const float* tbuf);
  void set_context_from(const half_t* ehs_dev, hipStream_t s);
  void run_attached();
  void invalidate_graphs() override;
  void after_reload() override;
  void run_eager() override;       // in_ops_, attached ControlNets, run_main, out_ops_
  void run_main(bool with_time);   // the main list [behind time_ops_] with the join of the forked ControlNets in place
  std::vector<const std::vector<Op>*> forward_lists() const override { return {&in_ops_, &time_ops_, &ll_.ops, &out_ops_}; }

  // Attached ControlNets run CONCURRENTLY with this UNet's time path and down / mid blocks (pipeline.py:519-529 evaluates them
  // back to back; nothing in the UNet depends on them before the residual adds of unet.py:1009-1022): they are forked onto
  // cn_stream_ behind the sample / timestep hand-over and joined in front of the first residual add (the main list at cn_join_pos_) -
  // eagerly and inside the captured step graphs alike.  SD_CN_CONCURRENT=0 keeps the serial order (A/B).
  hipStream_t cn_stream_ = nullptr;
  hipEvent_t ev_cn_fork_ = nullptr, ev_cn_join_ = nullptr;
  int cn_join_pos_ = -1;
  bool cn_forked_ = false;         // run_attached forked them and run_main has not joined yet

  // static-shape input/output device buffers
  half_t* in_sample_ = nullptr;     // NCHW f16
  half_t* in_timestep_ = nullptr;   // (B,) f16
  half_t* in_ehs_ = nullptr;        // BC1S f16
  half_t* in_time_ids_ = nullptr;
  half_t* in_text_embeds_ = nullptr;
  half_t* in_cond_ = nullptr;       // ControlNet conditioning image NCHW f16
  std::vector<half_t*> in_res_nchw_;   // support_controlnet: residual inputs (NCHW f16)
  std::vector<Tensor> res_nhwc_;       // ... converted to NHWC
  std::vector<std::vector<int>> res_shapes_;   // (B,C,H,W) of each residual
  float* noise_pred_ = nullptr;     // NCHW f32
  std::vector<float*> res_out_;     // ControlNet outputs NCHW f32
  std::vector<Tensor> cn_out_;      // ControlNet outputs NHWC f16

  Tensor x_in_;                     // NHWC sample
  float* tbuf_ = nullptr;           // (B,) f32 timesteps
  float* emb_ = nullptr;            // (B, temb_dim)
  float* temb_all_ = nullptr;       // (B, kTembCap)
  // device loop: time-embedding rows of every step of the current schedule (unconditioned time path only), and the
  // timesteps they were computed for
  float* temb_tab_ = nullptr;       // [steps][B][kTembCap]
  int temb_tab_cap_ = 0;            // in steps
  float *tt_tab_ = nullptr, *tsin_tab_ = nullptr, *e1_tab_ = nullptr, *emb_tab_ = nullptr;   // [steps * B] x {1, C0, tdim, tdim}
  struct TimePath {                 // the unconditioned time path's weights (unet.py:703-728), kept for the table pass
    const float* freq = nullptr;
    const half_t *w1 = nullptr, *w2 = nullptr;
    const float *b1 = nullptr, *b2 = nullptr;
    int c0 = 0, tdim = 0;
    bool ok = false;                // false: text_time conditioning enters the MLP (SDXL) -> in-step path only
  } tpath_;
  int temb_used_ = 0;
  std::vector<std::pair<std::string, int>> temb_layers_;
  half_t* temb_w_all_ = nullptr;
  float* temb_b_all_ = nullptr;
  Tensor ctx_;                      // encoder_hidden_states as tokens [B][L][Cctx]

  std::vector<Op> in_ops_, time_ops_, ctx_ops_, cond_ops_;   // the main list is ll_.ops
  std::vector<Op> out_ops_;          // ControlNet: fp16 NHWC residuals -> fp32 NCHW for the host boundary only
  std::vector<UNet*> attached_;      // UNet with support_controlnet: ControlNets whose outputs it consumes on device
  std::vector<uint16_t> last_ehs_, last_cond_;
  bool have_ctx_ = false, have_cond_ = false;
  hipGraphExec_t loop_graph_ = nullptr;   // one captured step of the denoise loop (ll_.graph: one forward)
  int loop_graph_key_ = -1;

  // denoise-loop state
  float* latents_ = nullptr;
  float* eps_hist_ = nullptr;
  float* tab_timesteps_ = nullptr;
  float* tab_coef_ = nullptr;
  float* tab_scale_ = nullptr;
  int* step_ = nullptr;
  int tab_cap_ = 0;
  float* noise_tab_ = nullptr;      // ancestral samplers: per-step noise of the current call
  size_t noise_cap_ = 0;            // in floats
  // progress handler: the de-noised tap's table and output (allocated by the first call that gives `pred`), the host snapshots
  // the handler reads, and the flag that refuses re-entry while it runs
  float* tab_pred_ = nullptr;       // [pred_cap_][8]
  int pred_cap_ = 0;
  float* denoised_ = nullptr;
  std::vector<float> snap_latents_, snap_denoised_;
  bool in_handler_ = false;
};

}  // namespace sd
