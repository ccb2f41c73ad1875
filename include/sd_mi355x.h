/* libsdmi355 - C ABI of the MI355X-native Stable Diffusion hot path.
 *
 * This is the drop-in boundary for the model-runner seam of apple/ml-stable-diffusion:
 *   python_coreml_stable_diffusion/coreml_model.py:36-120   CoreMLModel(**np.ndarray) -> dict
 *   swift/StableDiffusion/pipeline/Unet.swift:90-144        Unet.predictNoise
 *   swift/StableDiffusion/pipeline/ManagedMLModel.swift:11-127 (load / perform / unload)
 * Each entry point below names the reference interface it replaces.  Plain pointers and sizes
 * only; no torch / numpy types.  All functions return 0 on success or a negative sd_status and
 * leave a message retrievable with sd_last_error() (thread-local).  A handle is NOT thread-safe
 * (one HIP stream per handle, like the one serial DispatchQueue per model of
 * ManagedMLModel.swift:24-69); different handles may be driven from different threads.
 *
 * Tensor conventions at the boundary are the reference's: NCHW images, BC1S sequences, fp16
 * inputs, fp32 outputs (python_coreml_stable_diffusion/torch2coreml.py:135, :857-863).
 */
#ifndef SD_MI355X_H
#define SD_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum sd_status {
  SD_OK = 0,
  SD_ERR_INVALID_ARGUMENT = -1, /* wrong shape/dtype/flag      -> TypeError / ValueError (coreml_model.py:97-116) */
  SD_ERR_NOT_FOUND = -2,        /* missing file / weight key   -> FileNotFoundError (coreml_model.py:176-178)     */
  SD_ERR_HIP = -3,              /* HIP runtime failure         -> RuntimeError                                     */
  SD_ERR_UNSUPPORTED = -4,      /* config outside the path     -> NotImplementedError (unet.py:835-880)            */
  SD_ERR_INTERNAL = -5
} sd_status;

typedef enum sd_dtype { SD_F16 = 0, SD_F32 = 1 } sd_dtype;

/* unet.py:33-36 AttentionImplementations; a per-handle field here instead of the reference's
 * module global unet.py:39 (conversion-time flag torch2coreml.py:1678-1685). */
typedef enum sd_attention_impl {
  SD_ATTN_ORIGINAL = 0,
  SD_ATTN_SPLIT_EINSUM = 1,
  SD_ATTN_SPLIT_EINSUM_V2 = 2
} sd_attention_impl;

const char* sd_last_error(void);
const char* sd_version(void);
/* number of visible HIP devices (<0: error).  The library never falls back to the CPU. */
int sd_device_count(void);

/* ------------------------------------------------------------------------------------------
 * Checkpoints.  Replaces `load_state_dict` of torch2coreml.py:917-918 + the two load hooks of
 * unet.py:121-146: tensors are handed over with their diffusers key names AS-IS (Linear weights
 * may be 2-D or 4-D; LayerNorm bias is the checkpoint's, not the reference's rewritten b/w).
 * ------------------------------------------------------------------------------------------ */
typedef struct sd_weights sd_weights;
int sd_weights_create(sd_weights** out);
/* copies `data` (host memory); shape has ndim entries */
int sd_weights_add(sd_weights* w, const char* name, const void* data, sd_dtype dtype, const int64_t* shape,
                   int ndim);
/* parse a .safetensors file (F16 / F32 / BF16 tensors); `prefix` (may be NULL) is stripped */
int sd_weights_load_safetensors(sd_weights* w, const char* path, const char* prefix);
int sd_weights_count(const sd_weights* w);
/* tensor `index` (0 .. count - 1, in name order): its name (NUL-terminated, cut to name_bytes) and shape (at most 8 dims) */
int sd_weights_tensor_info(const sd_weights* w, int index, char* name, int name_bytes, int64_t* shape8, int* ndim);
/* Overwrites the values of the existing tensor `name` in place (SD_ERR_NOT_FOUND when absent; n must be its element count, else
 * SD_ERR_INVALID_ARGUMENT).  A palette or W8A8 mark on the tensor is dropped: it is then a plain tensor holding `values`.  Host only.
 * With sd_unet_reload_weights this is what replaces the reference's in-place `module.weight.data = ...` of its compression searches
 * (mixed_bit_compression_pre_analysis.py:139-156 fake_palettize, :158-178 simulate_quant_fn and its restore). */
int sd_weights_set_values(sd_weights* w, const char* name, const float* values, size_t n);
void sd_weights_destroy(sd_weights* w);
/* Palettized weights: the reference's conversion-time compression (torch2coreml.py:182-229 --quantize-nbits,
 * mixed_bit_compression_apply.py) with the semantics of its fake_palettize at one group per tensor
 * (mixed_bit_compression_pre_analysis.py:139-156): one LUT of 2^nbits fp16 entries per tensor, uint8 indices, and the tensor every
 * model sees is lut[indices].  nbits is 1, 2, 4, 6 or 8 (anything else SD_ERR_INVALID_ARGUMENT, checked first).
 * sd_weights_palettize clusters the stored tensor `name` (SD_ERR_NOT_FOUND when absent), its values rounded to fp16 first, by EXACT
 * 1-D k-means - dynamic programming over the sorted distinct values, deterministic - and replaces its data by lut[indices]; the LUT
 * is ascending; *sq_err (may be NULL) = sum of squared differences between the fp16-rounded values and lut[indices].  A tensor with
 * no more than 2^nbits distinct values is reproduced exactly.
 * sd_weights_add_palettized stores a palette computed elsewhere: lut 2^nbits f16, indices one uint8 per element (an index
 * >= 2^nbits is SD_ERR_INVALID_ARGUMENT).  sd_weights_palette_bits: the tensor's nbits, 0 when it has no palette.
 * sd_weights_read_palette copies out what the store holds (each output may be NULL): lut 2^nbits f16, indices, and the tensor's
 * values as f32 (values alone also works for a tensor without a palette). */
int sd_weights_palettize(sd_weights* w, const char* name, int nbits, double* sq_err);
int sd_weights_add_palettized(sd_weights* w, const char* name, const void* lut, int nbits, const uint8_t* indices, const int64_t* shape,
                              int ndim);
int sd_weights_palette_bits(const sd_weights* w, const char* name);
/* The palettized 3x3 halo convs, opt-in (host only; on = 0 / 1, any other value is SD_ERR_INVALID_ARGUMENT; off by default).  Handles
 * created from the store while the switch is on run every palettized 3x3 / stride-1 conv whose fp16 plan is the K-split halo conv
 * (plan tile 7, without GroupNorm in the loader) from its palette: conv3x3_halo_pal_kernel, plan tile 25, with that plan's ring code and
 * split-K - resnet conv1 / conv2, the two-source convs of the up blocks and the upsamplers (which then take tile 25, not the
 * sub-pixel tile 21, as a W8A8 one takes tile 18).  Such a conv holds the index stream (ceil(Cout / 64) * 64 * 9 * Ctot * nbits / 8
 * bytes) and the LUT only - no fp16 copy, no sub-pixel fold - and computes bit for bit what it computed from fp16 lut[indices]; its
 * profile label reads "conv3x3+pal<nbits> ...".  With the switch off a handle is, to the byte, what it was without it. */
int sd_weights_palette_halo(sd_weights* w, int on);
int sd_weights_read_palette(const sd_weights* w, const char* name, void* lut, uint8_t* indices, float* values);
/* W8A8 post-training quantization: replaces activation_quantization.py:141-203 (quantize_cumulative_config + the calibration that
 * feeds it) with its scheme - symmetric int8, one scale per OUTPUT CHANNEL for a conv's weights, one scale per TENSOR for the
 * activations it reads.  Parity with coremltools' quantizer is unpinned (coremltools is not part of this code base's test bed).
 *   weights      s_w[n] = absmax_n / 127 (an all-zero row: 1), q = clip(rint(w / s_w[n]), -127, 127): fp32 division, ties to even
 *   activations  s_a = act_absmax / 127 over ALL sources of the conv (both halves of a skip concat);
 *                x_q = clip(rint(fp32(x) * fp32(1 / s_a)), -127, 127) in the kernel; NaN -> 0, +-inf -> +-127
 *   output       fp32(int32 sum) * fp32(s_a * s_w[n]), then bias / time embedding / residual as for any conv
 * sd_weights_quantize_w8a8 MARKS the conv weight `name` (SD_ERR_NOT_FOUND when absent): the store keeps q, s_w and act_absmax beside
 * the untouched values; *sq_err (may be NULL) = sum (w - q s_w)^2.  SD_ERR_INVALID_ARGUMENT: a tensor that is not (Cout, Cin, k, k),
 * a tensor that carries a palette (and sd_weights_palettize refuses a marked tensor), act_absmax not a positive finite number, a
 * non-finite weight.  A UNet handle built from the store runs a marked conv from int8 exactly where its plan would be the weight
 * stream (plan tile 9 -> wstream.hip, plan tile 17) or the 3x3 / stride-1 halo conv with at most 14 784 input channels (plan tile 7
 * -> conv3x3_halo_i8.hip, plan tile 18, with tile 7's ring and split-K) or, at a call site that consents to a pinned 1x1 kernel
 * (proj_in, attn1.to_out.0, attn2.to_out.0), the single-source small-M 1x1 GEMM (plan tile 12 -> smgemm_i8.hip, plan tile 19, with
 * tile 12's tile height) - the same function of its inputs in all three - or, for ff.net.0.proj, the GEGLU projection (plan tile 13 ->
 * smgeglu_i8.hip, plan tile 20, at tile 13's tile height: norm3 is then not folded, one LayerNorm launch writes int8(norm3(x)) with
 * act_absmax / 127 and the GEGLU reads it - sd_op_layernorm_q8 / sd_op_geglu_w8a8) - or, for attn1.to_q / to_k / to_v of a
 * self-attention that runs them as one fused q|k|v launch, that launch (smqkv_i8.hip, plan tile 22: norm1 is then not folded, one
 * LayerNorm launch writes int8(norm1(x)) and the launch reads it and the stacked int8 matrix - sd_op_qkv_w8a8) where ALL THREE tensors
 * are marked with the SAME act_absmax (one int8 tensor carries one scale; the calibration below reports one value under the three
 * names) and the shape is on tile 22's rule (C a multiple of 160 from 640 up, H * W a multiple of 16, whole 128- / 256-row tiles: the
 * 640- and 1280-channel levels, not the 8 x 8 mid block); any other marked conv (one or two of the three, three ranges, the
 * 320-channel level's one-launch head, attn2.to_q / to_k / to_v, the merged transformer tail, two-source 1x1, GEGLUs off tile 13,
 * stride 2, channel counts off the tiles) runs fp16 as before - the reference's skipped layers.
 * The tail of a transformer block: a marked ff.net.2 whose un-merged shape is on plan tile 24's rule (4C -> C at 256 <= M <= 2048 on
 * 192 - 256 tiles of 32 / 64 x 80: the 640- and 1280-channel levels of SD2.1-base, not the mid block, C <= 2048) is NOT merged with
 * proj_out: it runs from int8 (smgemm_q8.hip, plan tile 24, + h2) on the GEGLU product quantized with its act_absmax - written as int8
 * by the GEGLU itself where that runs plan tile 20 (no fp16 product exists), else by one quantizer launch over the product - and
 * proj_out then runs as a launch of its own, from int8 (plan tile 19) where it is marked too.  An unmarked ff.net.2 keeps the merged
 * fp16 launch, and a proj_out marked beside it stays "marked, not applied".
 * sd_weights_w8a8_info: 1 when `name` is marked (*act_scale, may be NULL, = s_a), else 0.
 * sd_weights_observe_activations(on): handles created from the store while it is on put an absmax observer in front of every conv
 * that plan tile 17 could take (on = 1) or that plan tile 17 or 18 could take (on = 2) (sd_unet_activation_ranges) - calibration on
 * the device.  0 = off; any other value is SD_ERR_INVALID_ARGUMENT.
 * sd_weights_observe_gemms(on): a flag beside that level - while the store observes (on = 1 or 2 above), handles created from it also
 * put an observer in front of every 1x1 projection plan tile 19 could take.  on = 0 / 1; any other value is SD_ERR_INVALID_ARGUMENT.
 * With the flag off the observer sets are those of the two levels above.
 * sd_weights_observe_geglus(on): a second flag of the same kind (0 / 1, effective only while the store observes) - handles created from
 * it also run, for every ff.net.0.proj plan tile 20 could take, a LayerNorm of the GEGLU's input into a scratch tensor and an observer
 * over it, named by the projection's weight; the GEGLU itself runs folded in fp16 as without the flag, so the outputs do not change.
 * sd_weights_observe_qkv(on): a third flag of the same kind (0 / 1, effective only while the store observes) - handles created from it
 * also run, for every fused q|k|v launch plan tile 22 could take, a LayerNorm of norm1 into a scratch tensor and ONE observer over it,
 * reported under the three weight names attn1.to_q / to_k / to_v with one value; the launch itself runs folded in fp16.
 * sd_weights_observe_tails(on): a fourth flag of the same kind (0 / 1, effective only while the store observes) - handles created from
 * it also put, for every ff.net.2 plan tile 24 could take, an observer over the GEGLU product it reads, named by ff.net.2's weight, and,
 * where that block ends its SpatialTransformer, a scratch ff.net.2 GEMM (+ residual) with an observer over its result, named by
 * proj_out's weight; the merged tail launch itself still runs, so the outputs do not change. */
int sd_weights_quantize_w8a8(sd_weights* w, const char* name, float act_absmax, double* sq_err);
int sd_weights_w8a8_info(const sd_weights* w, const char* name, float* act_scale);
int sd_weights_observe_activations(sd_weights* w, int on);
int sd_weights_observe_gemms(sd_weights* w, int on);
int sd_weights_observe_geglus(sd_weights* w, int on);
int sd_weights_observe_qkv(sd_weights* w, int on);
int sd_weights_observe_tails(sd_weights* w, int on);
/* W8A8 einsums.  The reference's get_quantizable_modules (activation_quantization.py:205-215) collects every Einsum beside every
 * Conv2d: the two products of an attention (unet.py:45-59, called at :108-118).  An Einsum has no tensor, so the store keeps a mark of
 * its own under the MODULE's name, <prefix>.einsum (for example down_blocks.1.attentions.0.transformer_blocks.0.attn1.einsum), with
 * three activation ranges: max |.| of the module's inputs q, k and v.  The scheme is the project's own - symmetric, per tensor; parity
 * with coremltools' quantizer is unpinned, as for every W8A8 layer - and is ONE function, stated at sd_op_attention_w8a8.
 * sd_weights_quantize_einsum: SD_ERR_NOT_FOUND when `name` does not end in ".einsum" or <prefix>.to_q.weight is not in the store,
 * SD_ERR_INVALID_ARGUMENT for a range that is not positive and finite.  A UNet handle built from the store runs a marked attn1.einsum
 * as two launches - the quantizer over the q | k rows and the V^T its q|k|v producer left, and the int8 attention kernel
 * (attention_i8.hip) - wherever it runs the fp16 head-dim-64 kernel (attention8.hip) today: head dim 64, S a multiple of 64 up to
 * 133 120.  Every other marked einsum - attn2.einsum (inside the fused cross-attention launches), head dims other than 64, shapes off
 * the rule, the general attention kernels - stays fp16: marked, not applied (sd_unet_einsum_info).  The einsum holds no weights:
 * sd_unet_reload_weights is unaffected.
 * sd_weights_einsum_info: 1 when `name` is marked (ranges[0..2], may be NULL, = the q, k and v ranges), else 0.
 * sd_weights_observe_einsums(on): a fifth flag of the kind above (0 / 1, effective only while the store observes) - handles created
 * from it put ONE observer launch behind every q|k|v producer whose self-attention the int8 kernel could take; it writes max |q|, max |k|
 * and max |V^T| of what the producer stored.  sd_unet_activation_ranges reports three slots <prefix>.einsum.q / .k / .v, the q value
 * divided by the factor the producer pre-scaled the queries by, so that it is the range of the q the reference's Einsum sees.  The
 * outputs do not change. */
int sd_weights_quantize_einsum(sd_weights* w, const char* name, float q_absmax, float k_absmax, float v_absmax);
int sd_weights_einsum_info(const sd_weights* w, const char* name, float* ranges);
int sd_weights_observe_einsums(sd_weights* w, int on);

/* ------------------------------------------------------------------------------------------
 * UNet / ControlNet.  Config mirrors UNet2DConditionModel.__init__ (unet.py:801-833) with the
 * static shapes Core ML bakes in at conversion time (torch2coreml.py:827-863).
 * ------------------------------------------------------------------------------------------ */
#define SD_MAX_LEVELS 6

typedef struct sd_unet_config {
  int32_t batch;                 /* UNet batch (2 = classifier-free guidance for one image)          */
  int32_t in_channels, out_channels;
  int32_t height, width;         /* latent size (image / 8); a UNet needs both to divide by
                                    2^(n_levels - 1), else SD_ERR_INVALID_ARGUMENT at create         */
  int32_t n_levels;
  int32_t block_out_channels[SD_MAX_LEVELS];
  int32_t down_cross_attn[SD_MAX_LEVELS];   /* 1: CrossAttnDownBlock2D, 0: DownBlock2D               */
  int32_t up_cross_attn[SD_MAX_LEVELS];     /* 1: CrossAttnUpBlock2D,  0: UpBlock2D (up order)       */
  int32_t layers_per_block;
  int32_t attention_head_dim[SD_MAX_LEVELS];           /* = NUMBER of heads (unet.py:194-198, :912)  */
  int32_t transformer_layers_per_block[SD_MAX_LEVELS];
  int32_t cross_attention_dim;
  int32_t context_len;           /* 77                                                               */
  int32_t norm_num_groups;       /* 32                                                               */
  float norm_eps;                /* 1e-5                                                             */
  int32_t flip_sin_to_cos;       /* 1                                                                */
  float freq_shift;              /* 0                                                                */
  int32_t addition_time_embed_dim;                 /* 0: none; SDXL 256 (text_time)                  */
  int32_t projection_class_embeddings_input_dim;   /* SDXL 2816 / refiner 2560                       */
  int32_t num_time_ids;          /* SDXL base 6, refiner 5                                           */
  int32_t support_controlnet;    /* UNet: consume additional_residual_0..N (unet.py:1009-1022)       */
  int32_t is_controlnet;         /* build controlnet.py:49-250 instead of the UNet                   */
  int32_t is_vae_decoder;        /* build the AutoencoderKL decoder (sd_vae_decoder_create)          */
  int32_t attention_impl;        /* sd_attention_impl                                                */
  int32_t use_graph;             /* 1: capture the forward into a HIP graph and replay it            */
  int32_t compute_fp32;          /* VAE handles only: 1 = fp32 activations and arithmetic, the reference's
                                  * float32 VAE of SDXL (torch2coreml.py:570-578 decoder, :726-733 encoder: "z" / "x"
                                  * declared float32, pipeline.py:315 reads the dtype off the model); 0 = fp16 storage */
} sd_unet_config;

typedef struct sd_unet sd_unet;

/* replaces CoreMLModel.__init__ / _load_mlpackage (coreml_model.py:40-95, :155-203) and
 * ManagedMLModel.loadResources (ManagedMLModel.swift:40-47) */
int sd_unet_create(const sd_unet_config* cfg, const sd_weights* w, int device, sd_unet** out);
/* ManagedMLModel.unloadResources (ManagedMLModel.swift:49-52) */
void sd_unet_destroy(sd_unet* u);
int sd_unet_set_attention(sd_unet* u, int impl);
/* Swap the values of named tensors in a live UNet / ControlNet handle - what the reference does by assigning to a torch module's
 * weight between two pipeline calls (mixed_bit_compression_pre_analysis.py:139-178, :206-262).  `w` is a complete store that differs
 * from the store `u` last took its weights from only in the VALUES of the `n_names` tensors `names`.  Afterwards `u` computes bit
 * for bit what a handle freshly created from `w` with the same configuration computes, eagerly and on replay of the graphs it has
 * captured: every folded, stacked, merged and fragment-major device copy made from a named tensor is made again, into the same
 * addresses; nothing is re-captured or allocated (sd_unet_arena_used_bytes / sd_unet_device_bytes do not move); the hoisted
 * cross-attention K / V^T of the current prompt and a ControlNet's conditioning embedding are recomputed.  Only values are read (for
 * a palettized tensor lut[indices]): which kernel a layer runs and the form the handle holds a tensor in do not change.
 * Everything is checked before the first device write, so a refused call leaves the handle computing exactly what it did:
 * SD_ERR_NOT_FOUND a name `w` does not hold; SD_ERR_INVALID_ARGUMENT a tensor whose shape differs from the one the handle was built
 * with; SD_ERR_UNSUPPORTED a named tensor the handle holds compressed on the device (a palette stream, int8 - the message names it),
 * a VAE handle, a handle built from an observing store.  A name the handle reads nowhere is accepted and changes nothing. */
int sd_unet_reload_weights(sd_unet* u, const sd_weights* w, const char* const* names, int n_names);
int sd_unet_num_residuals(const sd_unet* u); /* controlnet.py:191-197 */
/* bytes of HBM held by the handle (weights + activations) */
size_t sd_unet_device_bytes(const sd_unet* u);
/* bytes the handle's tensors occupy inside that memory: the sum of its 256-byte-aligned allocations (sd_unet_device_bytes counts the
 * whole 256-MiB chunks they were carved from) */
size_t sd_unet_arena_used_bytes(const sd_unet* u);
/* Palettes of the handle's weights: *n_palettized tensors of its weight store arrived with a palette; *n_streamed convolutions read
 * theirs on the device - the small-M weight-stream convs (plan tile 14) and the small-M 1x1 projections proj_in / attn1.to_out.0 /
 * attn2.to_out.0 whose plan is smgemm.hip (plan tile 15) and the GEGLU projections ff.net.0.proj whose plan is smgeglu.hip on
 * 128-row tiles (plan tile 16; beside stream and LUT they hold norm3.weight as fp32 where the LayerNorm is folded in), which hold only
 * the index bit stream and the LUT, no fp16 copy - and, in a handle created while the store's sd_weights_palette_halo switch was on,
 * the 3x3 halo convs (plan tile 25: resnet conv1 / conv2, the two-source convs of the up blocks, upsamplers);
 * *stream_bytes = the bytes of those streams and LUTs.  Every other palettized tensor (q|k|v, attn2.to_q, the merged transformer
 * tail, GEGLU projections on 256-row tiles, the halo convs with the switch off) was uploaded as fp16 lut[indices]. */
int sd_unet_palette_info(const sd_unet* u, int* n_palettized, int* n_streamed, size_t* stream_bytes);
/* W8A8 (activation_quantization.py:141-203; sd_weights_quantize_w8a8): *n_marked tensors of the handle's weight store arrived with a
 * mark; *n_applied convolutions run from int8 (plan tiles 17, 18, 19, 20 and 22) and hold the int8 weights in their kernel's layout and one fp32
 * scale per output channel, no fp16 copy; *bytes = the bytes of those weights and scale vectors.  n_marked - n_applied marked convs
 * stayed fp16.  A fused q|k|v launch on plan tile 22 counts its three tensors - sd_unet_w8a8_layer names them in the order to_q, to_k,
 * to_v - and 3C * C + 4 * 3C bytes. */
int sd_unet_w8a8_info(const sd_unet* u, int* n_marked, int* n_applied, size_t* bytes);
/* Which convs those are: returns n_applied (>= 0) or an error code (< 0); index >= 0 fills `name` with the weight tensor of the
 * index-th of them in build order (SD_ERR_INVALID_ARGUMENT when there is no such conv), index < 0 asks for the count alone. */
int sd_unet_w8a8_layer(const sd_unet* u, int index, char* name, int name_bytes);
/* W8A8 einsums (sd_weights_quantize_einsum): *n_marked einsum marks the handle's weight store arrived with; *n_applied attentions run
 * on the int8 kernel.  sd_unet_w8a8_info / sd_unet_w8a8_layer count convs only.  sd_unet_einsum_layer: like sd_unet_w8a8_layer, `name`
 * = the module (<prefix>.einsum) of the index-th applied einsum in build order. */
int sd_unet_einsum_info(const sd_unet* u, int* n_marked, int* n_applied);
int sd_unet_einsum_layer(const sd_unet* u, int index, char* name, int name_bytes);
/* The activation observers of a handle created from an observing store (sd_weights_observe_activations), in launch order.  Returns
 * their number (>= 0) or an error code (< 0).  index >= 0 (SD_ERR_INVALID_ARGUMENT when there is no such slot): `name` = the conv's
 * weight tensor (NUL-terminated, cut to name_bytes), *absmax = max |x| over the conv's source tensor(s) of every forward since the
 * handle was created (an element-wise maximum: NaN elements are skipped).  index < 0: the count alone.  Synchronises the handle's
 * stream.  The observers are ordinary launches of the forward (captured into its graph); they write nothing the model reads. */
int sd_unet_activation_ranges(sd_unet* u, int index, char* name, int name_bytes, float* absmax);

#define SD_FLAG_DEVICE_PTRS 1 /* all data pointers are device pointers on the handle's GPU */

typedef struct sd_unet_io {
  const void* sample;                /* (B, in_channels, H, W) f16                                   */
  const void* timestep;              /* (B,) f16                                                     */
  const void* encoder_hidden_states; /* (B, cross_attention_dim, 1, context_len) f16 BC1S            */
  const void* time_ids;              /* SDXL: (B, num_time_ids) f16, else NULL                       */
  const void* text_embeds;           /* SDXL: (B, proj_dim - num_time_ids*addition_time_embed_dim) f16 */
  const void* controlnet_cond;       /* ControlNet: (B, 3, 8H, 8W) f16                               */
  const void* const* additional_residuals; /* UNet w/ support_controlnet: N pointers, f16 NCHW        */
  int32_t num_additional_residuals;
  void* noise_pred;                  /* UNet out: (B, out_channels, H, W) f32                        */
  void* const* residual_outputs;     /* ControlNet out: N pointers, f32 NCHW                         */
  int32_t flags;
  const float* step_noise;           /* sd_unet_denoise_loop only, optional (HOST pointer): (n_steps, n_images, C, H, W) f32
                                      * added to the latents at the end of step i - the fresh noise of the ancestral
                                      * samplers (EulerAncestralDiscrete, pipeline.py:592-604), already scaled by the
                                      * step's sigma_up, drawn by the host's seeded generator like the reference does */
} sd_unet_io;

/* replaces CoreMLModel.__call__ -> MLModel.predict (coreml_model.py:118-120; call site
 * pipeline.py:531-536) and Unet.predictNoise (Unet.swift:90-144).  Synchronous. */
int sd_unet_forward(sd_unet* u, const sd_unet_io* io);

/* Timing on the handle's own stream with HIP events: runs `iters` forwards on the inputs of
 * the last sd_unet_forward call and returns the mean milliseconds per forward. */
int sd_unet_time_forward(sd_unet* u, int warmup, int iters, float* ms_per_iter);

/* Measurement hook: HIP-event time of every launch-list entry ("op": one kernel, or a kernel plus its
 * split-K reduce) of one forward on the inputs of the last call, in launch order, eager launches (the
 * same dependent-kernel sequence the HIP graph replays), median over `iters` passes.  Fills up to `cap`
 * entries of ms / flop (algorithmic FLOP of MFMA ops, 0 for bandwidth ops) / labels (cap x label_bytes
 * chars, NUL-terminated) and always sets *n_ops to the number of ops.  No reference counterpart: it is
 * what bench.py derives the in-sequence roofline of the dominant kernel family from. */
int sd_unet_profile(sd_unet* u, int iters, int cap, float* ms, double* flop, char* labels, int label_bytes,
                    int* n_ops);

/* ---- debug ABI (tuning / race-guard tools): both entry points below return SD_ERR_UNSUPPORTED unless the process
 * runs with SD_TUNE=1 in its environment; nothing in the product path calls them. ----
 * Tuning hook of the same kind: while tile != 0, every convolution / GEMM whose constraints admit it runs with
 * this plan (tile 1-6, LDS-DMA ring code 0-5, split-K; csrc/igemm.hip) instead of the table's, so ONE profiled
 * forward measures a candidate on every layer shape in sequence (tools/tune_plans.py).  tile = 0 switches it off.
 * Process-global; never set in production. */
int sd_tune_set_candidate(int tile, int staging, int splitk);
/* Measurement hook: replace the run-time plan table (consulted before the compiled-in one; same rows as
 * csrc/tuned_convs.inc, one "{kind, ksize, stride, up, Ctot, N, M, tile, staging, splitk}" per line; NULL = empty) and, when
 * `u` is given, drop its captured HIP graphs so that the next forward re-captures with the new plans.  tools/tune_e2e.py
 * uses it to judge a plan by the graph-replay time of the WHOLE step instead of a per-kernel timing.  Process-global. */
int sd_tune_set_plan_table(const char* rows, sd_unet* u, int* n_plans);

/* Device-resident denoising loop (pipeline.py:500-573 with latents, CFG combine and scheduler
 * update never leaving HBM; Swift twin StableDiffusionPipeline.swift:233-333 incl. imageCount > 1).
 * latents: (n_images, C, H, W) f32 host in/out; the UNet batch must be cfg * n_images with
 * cfg = (guidance_scale > 1 ? 2 : 1) (pipeline.py:443), batch order [uncond..., cond...] (:245).
 * `timesteps` (n_steps) and `coef` (n_steps x 8) come from the host-side scheduler tables; every
 * scheduler on the path (DDIM, PNDM/PLMS Scheduler.swift:137-344, DPM-Solver++ 2M
 * DPMSolverMultistepScheduler.swift:27-273) is the linear multistep rule
 *     eps = u + g*(c - u);  m = a*x + b*eps;  x <- cx*x + cm*m + sum_{j<history} ch[j]*hist[j]
 * with coef row = [cx, cm, ch0, ch1, ch2, a, b, flags]; hist[j] is the m of j+1 pushes ago and
 * flags != 0 keeps this step's m out of the history (PLMS warm-up).  history <= 3.
 * `sample_scale` (may be NULL): n_steps factors of scheduler.scale_model_input (pipeline.py:504-505;
 * 1/sqrt(sigma^2+1) for the sigma-space Euler / LMS schedulers), applied to the UNet input only.
 * `history_io` (may be NULL): (history, n_images, C, H, W) f32 host buffer read before the first
 * step and written after the last, so a loop can continue on another handle (SDXL base -> refiner
 * hand-off, StableDiffusionXLPipeline.swift:205-225).  The encoder_hidden_states / SDXL extras are
 * taken from `io`; ControlNet residuals come from the attached ControlNet handles (below).
 * ms_per_step (may be NULL) receives HIP-event time per loop iteration. */
int sd_unet_denoise_loop(sd_unet* u, const sd_unet_io* io, float* latents, int n_images, int n_steps,
                         const float* timesteps, const float* coef, const float* sample_scale, int history,
                         float guidance_scale, float* history_io, float* ms_per_step);

/* Progress handler of the device-resident loop: what sample(configuration:progressHandler:) hands its handler as PipelineProgress
 * after every step (StableDiffusionPipeline.swift:205-210, :332-349, :411-426) and pipeline.py:570-573 its `callback(i, t, latents)`.
 * step: index into `timesteps`; n_steps: their count (PNDM's doubled entry counts, as Swift's timeSteps.count does); latents: the
 * latents after that step, (n_images, C, H, W) f32; denoised: the scheduler's de-noised estimate of that step (Swift's
 * `modelOutputs.last`, the previews of useDenoisedIntermediates, StableDiffusionPipeline.Configuration.swift:43-44), or NULL when
 * the loop got no `pred`.  Both are host buffers of the handle, valid during the call only.  Returning 0 stops the generation, as
 * the Swift handler's `false` does. */
typedef int (*sd_progress_fn)(void* user, int step, int n_steps, const float* latents, const float* denoised);
/* sd_unet_denoise_loop with that handler; sd_unet_denoise_loop is this entry with pred = NULL, every = 1, fn = NULL.
 * `pred` (may be NULL): n_steps x 8 f32 rows [pa, pb, ph0, ph1, ph2, 0, 0, 0] of the scheduler's de-noised table; with it every step
 * also writes  denoised = pa*x + pb*eps + sum_{j<history} ph[j]*hist[j]  from the x, eps and hist[] its update reads (one more fp32
 * store of the latents per step; the latents, the history and the step count are bit for bit those of a loop without it).
 * After step i with i % every == 0 (the rule of pipeline.py:570; every >= 1) the latents [and `denoised`] are copied to the host, the
 * handle's stream is drained and fn runs on the calling thread.  fn returning 0 stops the loop: `latents` receives the latents after
 * step i, `history_io` is written as at a normal end, *steps_done = i + 1 (n_steps after a full run), the status is SD_OK and only
 * ms_per_step[0 .. i] are filled.  ms_per_step[i] covers step i's device work only, neither the snapshot copy nor the handler.
 * Inside the handler this handle's stream is idle, so other handles may be driven (the VAE decoder for a preview); every entry
 * that would run or reconfigure THIS handle - sd_unet_forward, sd_unet_time_forward, sd_unet_profile, sd_unet_denoise_loop[_progress]
 * (a refusal of either names sd_unet_denoise_loop_progress, the one entry behind both), sd_unet_set_attention,
 * sd_unet_attach_controlnets, sd_tune_set_plan_table - returns SD_ERR_INVALID_ARGUMENT before any device work and leaves the loop
 * undisturbed; the read-only queries (sd_unet_num_residuals, sd_unet_device_bytes, sd_unet_arena_used_bytes, sd_unet_palette_info)
 * answer as always; destroying the handle there is undefined.  steps_done may be NULL only when fn is. */
int sd_unet_denoise_loop_progress(sd_unet* u, const sd_unet_io* io, float* latents, int n_images, int n_steps,
                                  const float* timesteps, const float* coef, const float* sample_scale, int history,
                                  float guidance_scale, float* history_io, float* ms_per_step,
                                  const float* pred /* n_steps x 8 or NULL */, int every,
                                  sd_progress_fn fn, void* user, int* steps_done);

/* ControlNet residuals on the device (replaces the host round trip of pipeline.py:259-284 / :519-529
 * and ControlNet.swift:64-118): `u` (built with support_controlnet) runs the n <= 3 attached
 * ControlNet handles on its own stream before every forward - same sample / timestep /
 * encoder_hidden_states - reads their 13 fp16 residual tensors straight from HBM, sums them over
 * the ControlNets (pipeline.py:269-282) and adds them to its skip / mid tensors (unet.py:1009-1022).
 * With ControlNets attached, sd_unet_forward ignores io->additional_residuals and
 * sd_unet_denoise_loop runs ControlNet + UNet every step.  n = 0 detaches.  The ControlNet handles
 * must outlive the attachment and share the UNet's device and static shapes. */
int sd_unet_attach_controlnets(sd_unet* u, sd_unet* const* controlnets, int n);
/* the conditioning image of an attached ControlNet, (B, 3, 8H, 8W) f16 (pipeline.py:346-357); its
 * embedding (controlnet.py:211-215) is computed once here, not every step */
int sd_controlnet_set_cond(sd_unet* controlnet, const void* controlnet_cond, int flags);

/* ------------------------------------------------------------------------------------------
 * VAE decoder: image = decoder(post_quant_conv(z)) in [-1, 1] (torch2coreml.py:584-594; call
 * site pipeline.py:313-320 `vae_decoder(z=latents / 0.18215)["image"]`; Decoder.swift).  The
 * config reuses sd_unet_config: block_out_channels = the VAE's (128,256,512,512), layers_per_block
 * = 2, in_channels = 4, out_channels = 3, height/width = latent size, norm_num_groups = 32.
 * z: (B, 4, h, w) f16 or f32 (z_dtype); image: (B, 3, 8h, 8w) f32.
 * ------------------------------------------------------------------------------------------ */
int sd_vae_decoder_create(const sd_unet_config* cfg, const sd_weights* w, int device, sd_unet** out);
int sd_vae_decode(sd_unet* vae, const void* z, sd_dtype z_dtype, float* image, int flags);
/* VAE encoder: latent = quant_conv(encoder(x)) (torch2coreml.py:739-749 `vae_encoder`, output "latent";
 * Encoder.swift:48-90 samples mean + std * noise from it and multiplies by the scale factor).  Config reuses
 * sd_unet_config: block_out_channels = the VAE's (128,256,512,512), layers_per_block = 2, in_channels = 3,
 * out_channels = 2 * latent channels (8), height/width = IMAGE size.  x: (B, 3, H, W) f16 or f32 in [-1, 1];
 * moments: (B, 8, H/8, W/8) f32 = [mean | logvar]. */
int sd_vae_encoder_create(const sd_unet_config* cfg, const sd_weights* w, int device, sd_unet** out);
int sd_vae_encode(sd_unet* vae, const void* x, sd_dtype x_dtype, float* moments, int flags);
/* Image-to-image start: the n_images noised starting latents of ONE starting image in one call - what generateLatentSamples
 * (StableDiffusionPipeline.swift:361-379, StableDiffusionXLPipeline.swift:365-381) gets from Encoder.encode (Encoder.swift:48-92:
 * posterior sample of the moments, logvar clamped to [-30, 20], times the scale factor) and Scheduler.addNoise
 * (Scheduler.swift:83-102).  Runs the encoder's launch list, then one element-wise fp32 kernel on the same stream; the moments
 * never reach the host:
 *     z = (mean + exp(0.5 * clamp(logvar, -30, 20)) * eps) * scale_factor;   latents[i] = sa * z + sb * noise[i]
 * The handle must have batch 1.  x as for sd_vae_encode; eps (Cz, H/8, W/8), noise and latents (n_images, Cz, H/8, W/8) f32;
 * eps / noise are standard normals drawn by the caller (sd_numpy_randn, ...), (sa, sb) the scheduler's add-noise coefficients
 * at the first timestep of the truncated schedule.  Host pointers unless SD_FLAG_DEVICE_PTRS. */
int sd_vae_encode_latents(sd_unet* vae_encoder, const void* x, sd_dtype x_dtype, const float* eps, const float* noise, int n_images,
                          float scale_factor, float sa, float sb, float* latents, int flags);
/* operator-level entry, same conventions as the other sd_op_* (host pointers, iters, ms): the single-head mid-block attention of
 * AutoencoderKL, out = softmax(q k^T / sqrt(C)) v with head dim = C over S = h * w tokens, as ONE streaming launch with no S x S
 * buffer - diffusers' mid-block attention inside the reference's VAE wrappers (torch2coreml.py:584-594 decoder, :739-749 encoder;
 * Decoder.swift, Encoder.swift).  q / k / v / out: (B*S, C) f16 token-major rows, as the 1x1 projections write them; any S >= 1.
 * Checked on the host before any device work, in this order: NULL arguments or B, S, C < 1 -> SD_ERR_INVALID_ARGUMENT; C not in
 * {64, 128, 256, 512} -> SD_ERR_UNSUPPORTED.  fp16 VAE handles run this kernel where H*W > 8192 or H*W % 64 != 0. */
int sd_op_vae_attention(const void* q, const void* k, const void* v, void* out, int B, int S, int C, int iters, float* ms);

/* ------------------------------------------------------------------------------------------
 * CLIP text encoder(s): transformers' CLIPTextModel / CLIPTextModelWithProjection as the reference
 * wraps them for conversion (torch2coreml.py:379-441, causal mask -1e4 :363-377) and calls them
 * (pipeline.py:151-175, `text_encoder(input_ids=...)`; TextEncoder.swift / TextEncoderXL.swift).
 * One prompt per call: input_ids (1, max_position_embeddings) int32.  Outputs (each may be NULL), f32:
 *   last_hidden_state (1, S, D)  final_layer_norm(last layer)          - SD 1.x / 2.x context
 *   hidden_embeds     (1, S, D)  hidden_states[-2], no final LN        - SDXL context (:416-428)
 *   pooled            (1, projection_dim) text_projection(final_LN(last)[eos_index]) when
 *                     projection_dim > 0 ("text_embeds"), else (1, D) pooler_output = final_LN(last)[eos_index]
 * Weights use the transformers key names (text_model.embeddings.*, text_model.encoder.layers.N.*,
 * text_model.final_layer_norm.*, text_projection.weight).
 * ------------------------------------------------------------------------------------------ */
typedef struct sd_text_encoder_config {
  int32_t vocab_size, hidden_size, intermediate_size, num_hidden_layers, num_attention_heads;
  int32_t max_position_embeddings; /* 77 */
  int32_t hidden_act;              /* 0: quick_gelu (CLIP ViT-L), 1: gelu (OpenCLIP H / bigG) */
  int32_t projection_dim;          /* 0: CLIPTextModel, > 0: CLIPTextModelWithProjection */
  float layer_norm_eps;            /* 1e-5 */
  int32_t use_graph;
} sd_text_encoder_config;
typedef struct sd_text_encoder sd_text_encoder;
int sd_text_encoder_create(const sd_text_encoder_config* cfg, const sd_weights* w, int device, sd_text_encoder** out);
void sd_text_encoder_destroy(sd_text_encoder* t);
size_t sd_text_encoder_device_bytes(const sd_text_encoder* t);
int sd_text_encoder_encode(sd_text_encoder* t, const int32_t* input_ids, int eos_index, float* last_hidden_state,
                           float* hidden_embeds, float* pooled);

/* ------------------------------------------------------------------------------------------
 * Operator-level entry points (what the parity tests and micro-benchmarks bind).  Host
 * pointers unless SD_FLAG_DEVICE_PTRS; each call is synchronous on an internal stream.
 * `ms` (may be NULL) returns HIP-event kernel time averaged over `iters` (>=1) launches.
 * Every device buffer of an entry sits between a front and a back guard of 0xff bytes; outputs and workspaces start as 0xff too
 * (fp16 / fp32 NaN patterns), so a skipped element or an unwritten split-K slab shows.  A guard byte that changed fails the call
 * with SD_ERR_INTERNAL after the last launch; fills and checks are outside the timed region.  sd_op_harness_selftest proves it.
 * ------------------------------------------------------------------------------------------ */
/* attention.py:24-168.  q (B, h*d, 1, Sq), k/v (B, h*d, 1, Sk) f16 BC1S -> out (B, h*d, 1, Sq) f16.
 * variant (A/B testing): 0 = default dispatch, 1 = never the software-pipelined d = 64 kernel, 2 = q arrives multiplied by
 * d^-0.5 * log2(e) (how the UNet's fused q|k|v GEMM hands its queries to that kernel: scaled in fp32, rounded once),
 * 3 = the default dispatch with q and k uploaded interleaved as ONE [B][S][2 h d] buffer (row strides of 2 h d, how a UNet's
 * self-attention reads the output of its fused q|k|v GEMM; needs Sq == Sk; bit-identical to variant 0),
 * 100 + u = that kernel's balanced grid with u (query tile, key tile) units per workgroup (0: the launch's own split). */
int sd_op_attention(int impl, const void* q, const void* k, const void* v, void* out, int B, int heads, int d,
                    int Sq, int Sk, int variant, int iters, float* ms);
/* Which kernel would sd_op_attention (int8 = 0; `variant` as that entry reads it, 100 + u included) or sd_op_attention_w8a8 (int8 != 0:
 * S = Sq; impl, d, Sk and variant are not read) launch for this problem on the current device?  Host only: no device work, nothing
 * launched; the compute-unit count the rules read is the device's, 256 where there is none.  It refuses what those entries refuse from
 * the shape alone, with their errors.  The answer is what the launcher itself decides (one host function per launcher, which the launch
 * calls), as one NUL-terminated line in text (text_bytes too small: SD_ERR_INVALID_ARGUMENT):
 *   "attn d<d> original w4 qt1"                 attention.hip, the ORIGINAL schedule
 *   "attn d<d> split w<4|8> qt<1|2>"            attention.hip, SPLIT_EINSUM (w4 qt1) and the 512-query chunks of SPLIT_EINSUM_V2: w = waves
 *                                               per workgroup, qt = 32-query tiles per wave (qt2 only with w8 and d <= 64)
 *   "attn8 w<4|8> classic"                      attention8.hip, one workgroup per query tile
 *   "attn8 w<4|8> balanced upw=<u> seg=<s>"     attention8.hip, the balanced form: u (query tile, key tile) units per workgroup, at most s
 *                                               query-tile segments per workgroup
 *   "attn_i8 w<4|8>"                            attention_i8.hip
 * attention8.hip and attention_i8.hip share ONE waves rule: w8 where B * heads * ceil(Sq / 256) >= compute units / 2. */
int sd_op_attention_kernel(int int8, int impl, int B, int heads, int d, int Sq, int Sk, int variant, char* text, int text_bytes);
/* layer_norm.py:51-80.  x (B, C, 1, S) f16, weight/bias (C) f32 -> out (B, C, 1, S) f16 */
int sd_op_layernorm(const void* x, const float* weight, const float* bias, void* out, int B, int C, int S, float eps,
                    int iters, float* ms);
/* torch.nn.GroupNorm (+ optional SiLU) as used by unet.py:430-451,:472-481,:528-531.  NCHW f16 */
int sd_op_groupnorm(const void* x, const float* weight, const float* bias, void* out, int B, int C, int H, int W,
                    int groups, float eps, int silu, int iters, float* ms);
/* The two independent first steps of a ResnetBlock2D with a channel change (unet.py:470-489): norm1 (+ SiLU) over the channel concat
 * (x0 | x1) (x1 may be NULL; the up blocks' torch.cat of unet.py:213-216) and conv_shortcut, a 1x1 conv over the same concat.
 * side = 1: both in ONE launch (the GroupNorm's blocks and the GEMM's tiles share a grid); side = 0: two launches.  The results are
 * bit-identical.  x0 (B,C0,H,W), x1 (B,C1,H,W) f16 NCHW, gn_weight / gn_bias (C0+C1) f32, w (N, C0+C1) f16, bias (N) f32 or NULL
 * -> out_gn (B, C0+C1, H, W), out_sc (B, N, H, W) f16 NCHW. */
int sd_op_groupnorm_shortcut(const void* x0, const void* x1, const float* gn_weight, const float* gn_bias, const void* w, const float* bias,
                             void* out_gn, void* out_sc, int B, int C0, int C1, int H, int W, int N, int groups, float eps, int silu,
                             int side, int iters, float* ms);
/* nn.Conv2d as used by unet.py (k in {1,3}, stride in {1,2}, padding k/2), optional nearest x2
 * upsample before the conv (unet.py:498-500), optional residual add.  x (B,Cin,H,W) f16 NCHW,
 * w (Cout,Cin,k,k) f16, bias (Cout) f32 or NULL, res (B,Cout,Ho,Wo) f16 or NULL -> out f16 NCHW.
 * tile/splitk: 0 = heuristic (tuning hooks). force_generic: 1 = direct non-MFMA kernel. */
int sd_op_conv2d(const void* x, const void* w, const float* bias, const void* res, void* out, int B, int Cin, int H,
                 int W, int Cout, int ksize, int stride, int upsample, int tile, int splitk, int force_generic,
                 int iters, float* ms);
/* sd_op_conv2d plus what the UNet / VAE builders set on their convs (a testing entry: tile, splitk, force_generic, iters, ms as above):
 *   x1, C1        second source (B, C1, H, W) f16 or NULL: the conv runs over the channel concat (x | x1) (the up blocks' torch.cat,
 *                 unet.py:213-216); w is then (Cout, Cin + C1, k, k)
 *   temb          (B, Cout) f32 or NULL: the resnet's time_emb_proj row, added to every pixel of its sample (unet.py:477).  On the
 *                 device it is a column block of a wider, otherwise poisoned row buffer, as the UNet keeps it
 *   pad_mode      0: padding k/2; 1: the VAE encoder's Downsample2D(padding=0) - F.pad(x, (0, 1, 0, 1)), then a pad-0 conv
 *                 (k = 3, stride 2, no upsample; Ho = (H - 2) / 2 + 1)
 *   twin_groups   > 0: the slab combine also writes GroupNorm(twin_groups groups, twin_gamma / twin_beta (Cout) f32, twin_eps)
 *                 (+ SiLU with twin_silu) of the result to out_twin (B, Cout, Ho, Wo) f16 - no GroupNorm launch (the low-res
 *                 conv1 -> norm2 path); refused where the combine cannot hold whole (sample, group) slices
 *   plan_out[4]   the plan the launch ran: tile (1-4 igemm.hip, 7 conv3x3_halo.hip, 9 wstream.hip, 11 bvgemm.hip, 12 smgemm.hip; the
 *                 entries of the compressed sources report theirs: 14 / 15 / 16 palettized, 17 / 18 / 19 / 20 / 22 / 24 W8A8),
 *                 staging, resolved split-K, 1 if the output left through fp32 slabs; all -1: the direct (non-MFMA) kernels
 * res / out are (B, Cout, Ho, Wo). */
int sd_op_conv2d_ex(const void* x, const void* x1, const void* w, const float* bias, const float* temb, const void* res, void* out, int B,
                    int Cin, int C1, int H, int W, int Cout, int ksize, int stride, int upsample, int pad_mode, int twin_groups,
                    const float* twin_gamma, const float* twin_beta, float twin_eps, int twin_silu, void* out_twin, int tile, int splitk,
                    int force_generic, int* plan_out, int iters, float* ms);
/* The small-M weight-stream conv from PALETTIZED weights (plan tile 14): w = lut[indices], lut 2^nbits f16 (nbits 1, 2, 4, 6, 8),
 * indices (Cout, Cin + C1, k, k) uint8; x1 / C1, bias, res, upsample, plan_out, iters, ms as sd_op_conv2d_ex; nw = waves per workgroup
 * (4 or 8, 0 = 8).  Stride 1, padding k / 2.  The result is bit-identical to sd_op_conv2d_ex(tile = 9, or 49 for four waves) on the
 * fp16 weights lut[indices].  A shape the weight stream does not take (wstream.hip: k 3 on 8- or 16-pixel-wide images or k 1,
 * channel counts multiples of 64 in and 32 out) is SD_ERR_INVALID_ARGUMENT. */
int sd_op_conv2d_palettized(const void* x, const void* x1, const void* lut, int nbits, const uint8_t* indices, const float* bias,
                            const void* res, void* out, int B, int Cin, int C1, int H, int W, int Cout, int ksize, int upsample, int nw,
                            int* plan_out, int iters, float* ms);
/* The index bit stream that entry and the UNet builder put on the device (host only, no GPU): indices (Cout, Ctot, k, k) uint8 ->
 * stream; *bytes = its size, stream may be NULL to ask for the size alone.  Per 32-row strip, 32-channel slice and lane, the
 * 16 * k * k indices of the lane in MFMA fragment order (fragment j, element e: row strip * 32 + (lane & 31), channel slice * 32 +
 * (j & 1) * 16 + (lane >> 5) * 8 + e, tap j >> 1) as little-endian nbits-wide fields, padded to whole 16-byte words, word q at
 * [strip][slice][q][lane][16 B]. */
int sd_op_palette_pack(const uint8_t* indices, int Cout, int Ctot, int ksize, int nbits, uint8_t* stream, size_t* bytes);
/* The 3x3 / stride-1 halo conv from PALETTIZED weights (plan tile 25, conv3x3_halo_pal.hip): w = lut[indices], lut
 * 2^nbits f16 (nbits 1, 2, 4, 6, 8), indices (Cout, Cin + C1, 3, 3) uint8; x1 / C1, bias, temb, res, upsample, iters, ms as
 * sd_op_conv2d_ex; staging = plan tile 7's ring code (0 / 2 / 3 / 4 / 5: 2 / 3 / 4 / 6 / 8 weight stages), splitk = split-K over
 * 64-channel chunks (0 = the library's rule for tile 7).  plan_out = {25, ring code, resolved split-K, slab}.  The result is
 * bit-identical to sd_op_conv2d_ex(tile = 7) on the fp16 weights lut[indices] at the same ring code and split-K.  Checked on the host in
 * this order, before any device work, each SD_ERR_INVALID_ARGUMENT: NULL arguments; nbits not in {1, 2, 4, 6, 8}; an empty problem;
 * upsample / staging / splitk off their ranges; a shape the halo conv does not take (channel counts multiples of 64 in and 4 out, an
 * image of at least 8 x 8 outputs); an index >= 2^nbits (the message names it). */
int sd_op_conv2d_palettized_halo(const void* x, const void* x1, const void* lut, int nbits, const uint8_t* indices, const float* bias,
                                 const float* temb, const void* res, void* out, int B, int Cin, int C1, int H, int W, int Cout, int upsample,
                                 int staging, int splitk, int* plan_out, int iters, float* ms);
/* The index bit stream that entry and the UNet builder put on the device (host only): indices (Cout, Ctot, 3, 3) uint8, Ctot a multiple
 * of 64 -> stream; *bytes = its size, ceil(Cout / 64) * 64 * 9 * Ctot * nbits / 8 (no padding bits; rows past Cout carry index 0);
 * stream may be NULL to ask for the size alone.  Per (64-row n-tile, 64-channel chunk, tap), in that order, one block of nbits * 128
 * dwords; dword j of stream (wk, lane) - K half wk = 0, 1, lane 0 .. 63 - at dword (j * 2 + wk) * 64 + lane of the block; a stream is
 * 32 little-endian nbits-wide fields, field (2 s + j) * 8 + e = row 64 n_tile + 32 j + (lane & 31), channel 64 chunk +
 * (2 (2 wk + s) + (lane >> 5)) * 8 + e (weight_prep.h halo_pal_pack). */
int sd_op_palette_pack_halo(const uint8_t* indices, int Cout, int Ctot, int nbits, uint8_t* stream, size_t* bytes);
/* The small-M weight-stream conv in W8A8 (plan tile 17; activation_quantization.py:141-203, semantics at sd_weights_quantize_w8a8):
 * wq (Cout, Cin + C1, k, k) int8, w_scale (Cout) f32, act_absmax the range of x (and x1); x1 / C1, bias, res, upsample, nw, plan_out,
 * iters, ms as sd_op_conv2d_palettized.  plan_out = {17, 4 for four waves else 0, slabs, 1}.  Checked on the host in this order,
 * before any device work, each SD_ERR_INVALID_ARGUMENT: NULL arguments; nw not in {0, 4, 8}; an empty problem; ksize / upsample off the
 * path; a shape the weight stream does not take; act_absmax not a positive finite number; a w_scale that is not; a weight of -128. */
int sd_op_conv2d_w8a8(const void* x, const void* x1, const int8_t* wq, const float* w_scale, float act_absmax, const float* bias,
                      const void* res, void* out, int B, int Cin, int C1, int H, int W, int Cout, int ksize, int upsample, int nw,
                      int* plan_out, int iters, float* ms);
/* The int8 stream that entry and the UNet builder put on the device (host only): wq (Cout, Ctot, k, k) int8 -> stream
 * [Cout / 32][Ctot / 32][k * k][64 lanes][16 B]: lane l of (strip, slice, tap) holds row strip * 32 + (l & 31), channels slice * 32 +
 * (l >> 5) * 16 + (0 .. 15).  *bytes = its size (Cout * Ctot * k * k); stream may be NULL to ask for the size alone. */
int sd_op_w8a8_pack(const int8_t* wq, int Cout, int Ctot, int ksize, int8_t* stream, size_t* bytes);
/* The 3x3 / stride-1 halo conv in W8A8 (plan tile 18, conv3x3_halo_i8.hip; semantics at sd_weights_quantize_w8a8 - the same function
 * of its inputs as sd_op_conv2d_w8a8): wq (Cout, Cin + C1, 3, 3) int8, w_scale (Cout) f32, act_absmax the range of x (and x1); x1 / C1,
 * bias, temb, res, upsample, iters, ms as sd_op_conv2d_ex; staging = plan tile 7's ring code (0 / 2 / 3: 2 / 3 / 4 weight stages; 4 / 5
 * run the 4-stage ring), splitk = split-K over 64-channel chunks (0 = the library's rule for tile 7).
 * plan_out = {18, ring code, resolved split-K, slab}.  Checked on the host in this order, before any device work, each
 * SD_ERR_INVALID_ARGUMENT: NULL arguments; an empty problem; upsample / staging / splitk off their ranges; a shape the halo conv does not
 * take (channel counts multiples of 64 in and 4 out, an image of at least 8 x 8 outputs); more than 14 784 input channels (the int32
 * sums must stay exact: 127 * 127 * 9 * Ctot < 2^31); act_absmax not a positive finite number; a w_scale that is not; a weight of -128. */
int sd_op_conv2d_w8a8_halo(const void* x, const void* x1, const int8_t* wq, const float* w_scale, float act_absmax, const float* bias,
                           const float* temb, const void* res, void* out, int B, int Cin, int C1, int H, int W, int Cout, int upsample,
                           int staging, int splitk, int* plan_out, int iters, float* ms);
/* The int8 weights that entry and the UNet builder put on the device (host only): wq (Cout, Ctot, 3, 3) int8 -> packed (Cout, 9, Ctot),
 * tap-major - the K order of the fp16 halo conv at one byte per weight, so a (row, tap, 64-channel chunk) is 64 contiguous bytes.
 * Ctot a multiple of 64.  *bytes = its size (Cout * Ctot * 9); packed may be NULL to ask for the size alone. */
int sd_op_w8a8_pack_halo(const int8_t* wq, int Cout, int Ctot, int8_t* packed, size_t* bytes);
/* The upsampler conv (Upsample2D, unet.py:498-500: nearest x2, then a 3x3 / pad-1 conv) as four 2x2 convs on the low-res image, one per
 * output phase (Y & 1, X & 1): plan tile 21, conv3x3_halo_sp.hip, 4/9 of the multiply-adds.  sd_op_subpixel_fold is the host-only fold
 * a handle applies once: w (Cout, Cin, 3, 3) f16 (w_f32 = 0) or f32 (1) -> folded (4 phases p = 2a + b, Cout, 4 taps t = 2dy + dx, Cin)
 * f16, tap t at low-res offset (a + dy - 1, b + dx - 1); every folded weight is the fp32 sum of its 1, 2 or 4 source weights in
 * (ky, kx) order, rounded to f16 once.  *halves = 16 * Cout * Cin; folded may be NULL to ask for the size alone.
 * sd_op_subpixel_refusal (host only): the first condition a conv of this shape misses for plan tile 21, "" when it is admitted.
 * sd_op_conv2d_subpixel: x (B, Cin, H, W) f16, w (Cout, Cin, 3, 3) f16 folded as above, bias (Cout) f32 / res (B, Cout, 2H, 2W) f16
 * or NULL -> out (B, Cout, 2H, 2W) f16; staging: plan tile 7's ring code (2: three stages, anything else four), splitk 0: the plan's
 * rule; plan_out = {21, staging, splitk, slab}.  The device output starts as NaN patterns in front of a guard: SD_ERR_INTERNAL when
 * the guard was written.  SD_ERR_INVALID_ARGUMENT naming the refusal for a shape tile 21 does not take. */
int sd_op_subpixel_fold(const void* w, int w_f32, int Cout, int Cin, void* folded, size_t* halves);
int sd_op_subpixel_refusal(int ksize, int stride, int up, int C0, int C1, int N, int B, int Hi, int Wi, int out_mode, char* text, int text_bytes);
int sd_op_conv2d_subpixel(const void* x, const void* w, const float* bias, const void* res, void* out, int B, int Cin, int H, int W, int Cout,
                          int splitk, int staging, int* plan_out, int iters, float* ms);
/* No reference counterpart as an operator; the layer it stands for is any Linear the reference's UNet writes as a 1x1 conv (unet.py:533-551
 * proj_in, :62-118 to_out) under quantize_cumulative_config (activation_quantization.py:141-203).  The single-source small-M 1x1 GEMM in
 * W8A8 (plan tile 19, smgemm_i8.hip; semantics at sd_weights_quantize_w8a8 - the same function of its inputs as sd_op_conv2d_w8a8:
 * out = fp16(((float(int32 sum) * (act_absmax / 127 * w_scale[n])) + bias[n]) + res), one rounding): x (B, Cin, H, W) f16, wq (Cout, Cin)
 * int8, w_scale (Cout) f32, act_absmax the range of x; bias (Cout) f32 / res (B, Cout, H, W) f16 may be NULL; bm = tile height 32 / 64,
 * 0 = by M as plan tile 12; iters, ms as sd_op_conv2d_ex.  plan_out = {19, 1 | 2 (bm 32 | 64), 1, 0}.  Checked on the host in this order,
 * before any device work, each SD_ERR_INVALID_ARGUMENT: bm not 0 / 32 / 64; NULL arguments or an empty problem; a shape plan tile 12 does
 * not tile (Cin a multiple of 64, Cout of 80, M = B H W of the tile height, at least 2 x 2 tiles and a multiple of 8 of them), then
 * Cin > 133120 (the int32 sums must stay exact: 127 * 127 * K < 2^31); act_absmax not a positive finite number; a w_scale that is not; a
 * weight of -128. */
int sd_op_gemm_w8a8(const void* x, const int8_t* wq, const float* w_scale, float act_absmax, const float* bias, const void* res, void* out, int B,
                    int Cin, int H, int W, int Cout, int bm, int* plan_out, int iters, float* ms);
/* The int8 weights that entry and the UNet builder put on the device (host only): wq (Cout, K) int8 -> packed (Cout, K) - the
 * checkpoint's own order: a wave fetches 16 rows x 64 contiguous bytes per K stage and swizzles on the source address.  Cout a multiple
 * of 16, K of 64.  *bytes = its size (Cout * K); packed may be NULL to ask for the size alone. */
int sd_op_w8a8_pack_gemm(const int8_t* wq, int Cout, int K, int8_t* packed, size_t* bytes);
/* No reference counterpart as an operator; the pair stands for norm3 -> ff.net.0.proj (unet.py:583-591, :609-617) under
 * quantize_cumulative_config (activation_quantization.py:141-203), which quantizes the OUTPUT of the LayerNorm and the un-folded weight.
 * sd_op_layernorm_q8: x (M, C) f16 token-major -> xq (M, C) int8 = clip(rint(fp32(y) * (127 / act_absmax)), -127, 127), y the fp16 value
 * sd_op_layernorm stores for that element (NaN -> 0, +-inf -> +-127); ln_weight / ln_bias (C) f32, or both NULL: y = x, a plain quantize.
 * C a multiple of 8 up to 2048, act_absmax a positive finite number; one wavefront per row, 8-byte stores.
 * sd_op_geglu_w8a8 (plan tile 20, smgeglu_i8.hip): xq (M, C) int8, wq (N2, C) int8 in the checkpoint's row order [values | gates], w_scale
 * (N2) f32, act_absmax the range xq was quantized with, bias (N2) f32 or NULL -> out (M, N2 / 2) f16 = fp16(v * gelu_erf(g)) with
 * v = (float(int32 sum over C) * (act_absmax / 127 * w_scale[n_v])) + bias[n_v], g the same on the gate row - each operation rounded to
 * fp32 on its own, the ending that of sd_op_geglu_ln.  bm = tile height 128 / 256, 0 = by the grid as plan tile 13; iters, ms as
 * sd_op_conv2d_ex.  plan_out = {20, 1 | 2 (bm 128 | 256), 1, 0}.  Checked on the host in this order, before any device work, each
 * SD_ERR_INVALID_ARGUMENT: (1) bm not 0 / 128 / 256; (2) NULL arguments or an empty problem; (3) a shape plan tile 13 does not tile (C a
 * multiple of 64, N2 of 160, M of the tile height, at least 2 x 2 tiles and a multiple of 8 of them); (4) C > 133120 (the int32 sums
 * must stay exact); (5) act_absmax not a positive finite number; (6) a w_scale that is not; (7) a weight of -128; (8) an activation of
 * -128. */
int sd_op_layernorm_q8(const void* x, const float* ln_weight, const float* ln_bias, float act_absmax, float eps, int8_t* xq, int M, int C,
                       int iters, float* ms);
int sd_op_geglu_w8a8(const int8_t* xq, const int8_t* wq, const float* w_scale, float act_absmax, const float* bias, void* out, int M, int C,
                     int N2, int bm, int* plan_out, int iters, float* ms);
/* The int8 weights that entry and the UNet builder put on the device (host only): wq (N2, K) int8 [values | gates] -> packed
 * [N2 / 16 strips][16 rows][K]: strip 2 U + v holds the checkpoint rows v * N2 / 2 + 16 U + (0 .. 15) - the value (v = 0) or gate
 * (v = 1) rows of the output's 16-column unit U, every row whole - so a tile of 80 output columns stages ten consecutive strips.  N2 a
 * multiple of 32, K of 64.  *bytes = its size (N2 * K); packed may be NULL to ask for the size alone. */
int sd_op_w8a8_pack_geglu(const int8_t* wq, int N2, int K, int8_t* packed, size_t* bytes);
/* No reference counterpart as operators; the pair stands for ff.net.0.proj -> ff.net.2 (unet.py:591, :609-632) under
 * quantize_cumulative_config (activation_quantization.py:141-203), which quantizes the GEGLU product v * gelu(g) that ff.net.2 reads and
 * ff.net.2's un-merged weight: what a handle runs for a marked ff.net.2 on plan tile 24's rule (sd_weights_quantize_w8a8).
 * sd_op_geglu_w8a8_q8 (plan tile 20 with an int8 output): sd_op_geglu_w8a8's arguments and checks, and out_absmax, the range of the
 * PRODUCT -> out_q (M, N2 / 2) int8 = clip(rint(fp32(y) * (127 / out_absmax)), -127, 127), y the fp16 value sd_op_geglu_w8a8 stores for
 * that element - the quantizer of sd_op_layernorm_q8 in plain form over that launch's output, bit for bit, with no fp16 tensor in
 * between.  plan_out = {20, 1 | 2, 1, 0}.  The device output starts as -128 in front of a guard: SD_ERR_INTERNAL when the guard was
 * written.  Checked in sd_op_geglu_w8a8's order, out_absmax (not a positive finite number) beside act_absmax in (5).
 * sd_op_gemm_q8 (plan tile 24, smgemm_q8.hip): xq (M, K) int8 token-major, wq (N, K) int8, w_scale (N) f32, act_absmax the range xq was
 * quantized with; bias (N) f32 / res (M, N) f16 token-major may be NULL -> out (M, N) f16 token-major
 *   = fp16(((float(int32 sum over K) * fp32(fp32(act_absmax / 127) * w_scale[n])) + bias[n]) + float(res[m][n])), one rounding:
 * sd_op_gemm_w8a8 behind its quantizer, the same function wherever that entry's x quantizes to xq.  bm = tile height 32 / 64, 0 = by M
 * as plan tile 12; iters, ms as sd_op_conv2d_ex.  plan_out = {24, 1 | 2 (bm 32 | 64), 1, 0}.  The device output starts as NaN patterns
 * in front of a guard: SD_ERR_INTERNAL when the guard was written.  Checked on the host in this order, before any device work, each
 * SD_ERR_INVALID_ARGUMENT: (1) bm not 0 / 32 / 64; (2) NULL arguments or an empty problem; (3) a shape plan tile 12 does not tile (K a
 * multiple of 64, N of 80, M of the tile height, at least 2 x 2 tiles and a multiple of 8 of them); (4) K > 133120 (the int32 sums must
 * stay exact); (5) act_absmax not a positive finite number; (6) a w_scale that is not; (7) a weight of -128; (8) an activation of -128. */
int sd_op_geglu_w8a8_q8(const int8_t* xq, const int8_t* wq, const float* w_scale, float act_absmax, const float* bias, float out_absmax,
                        int8_t* out_q, int M, int C, int N2, int bm, int* plan_out, int iters, float* ms);
int sd_op_gemm_q8(const int8_t* xq, const int8_t* wq, const float* w_scale, float act_absmax, const float* bias, const void* res, void* out,
                  int M, int K, int N, int bm, int* plan_out, int iters, float* ms);
/* No reference counterpart as an operator; behind sd_op_layernorm_q8 it stands for norm1 -> attn1.to_q / to_k / to_v (unet.py:583-586 ->
 * :74-84) under quantize_cumulative_config (activation_quantization.py:141-203), which quantizes the OUTPUT of the LayerNorm and the
 * three un-folded weights.  sd_op_qkv_w8a8 (plan tile 22, smqkv_i8.hip): xq (B * HW, C) int8 token-major, wq (3C, C) int8 =
 * [Wq | Wk | Wv] each in the checkpoint's row order, w_scale (3C) f32, act_absmax the range xq was quantized with, bias (3C) f32 or NULL
 * -> what sd_op_qkv_ln hands to attention: out_qk (B * HW, 2C) f16 = q | k, out_vt (B, C, HW) f16 = V^T (vt_perm != 0: the two middle
 * 4-token blocks of every 16 tokens swapped).  For output column n of token m, each operation rounded to fp32 on its own:
 *   v = float(int32 sum over C of xq[m][k] * wq[n][k]) * fp32(fp32(act_absmax / 127) * w_scale[n]);  v = v + bias[n] with a bias;
 *   v = v * q_scale for n < C unless q_scale == 1;  out = fp16(v), one rounding.
 * bm = tile height 128 / 256, 0 = by the grid (128 rows while that grid stays within 256 workgroups); iters, ms as sd_op_conv2d_ex.
 * plan_out = {22, 1 | 2 (bm 128 | 256), 1, 0}.  Checked on the host in this order, before any device work, each
 * SD_ERR_INVALID_ARGUMENT: (1) bm not 0 / 128 / 256; (2) NULL arguments or an empty problem; (3) a shape off plan tile 22's rule (C a
 * multiple of 160 and of 64, at least 640; HW a multiple of 16; B * HW a multiple of the tile height with at least 2 tile rows; a
 * multiple of 8 tiles of bm x 160); (4) C > 133120 (the int32 sums must stay exact); (5) act_absmax not a positive finite number, or
 * q_scale not finite; (6) a w_scale that is not a positive finite number; (7) a weight of -128; (8) an activation of -128. */
int sd_op_qkv_w8a8(const int8_t* xq, const int8_t* wq, const float* w_scale, float act_absmax, const float* bias, void* out_qk, void* out_vt,
                   int B, int HW, int C, float q_scale, int vt_perm, int bm, int* plan_out, int iters, float* ms);
/* The int8 weights that entry and the UNet builder put on the device (host only): wq (3C, C) int8 = [Wq | Wk | Wv] -> packed
 * [3C / 16 strips][16 rows][C]: strip t holds the stacked rows 16 t .. 16 t + 15, every row whole - a tile of 160 output columns stages
 * the ten consecutive strips 10 n_tile .. 10 n_tile + 9.  C a multiple of 64.  *bytes = its size (3C * C); packed may be NULL to ask
 * for the size alone. */
int sd_op_w8a8_pack_qkv(const int8_t* wq, int C, int8_t* packed, size_t* bytes);
/* The self-attention einsums in W8A8 (attention_i8.hip; activation_quantization.py:205-215, unet.py:45-59; marks:
 * sd_weights_quantize_einsum).  Head dim 64, S_q = S_k = S, S a multiple of 64.  THE FUNCTION, with r_q, r_k, r_v the three ranges and
 * s_x = fp32(r_x / 127):
 *   1. x_q = clip(rint(fp32(x) * fp32(127 / r_x)), -127, 127), NaN -> 0, +-inf -> +-127 (sd_op_einsum_quantize; a handle's queries are
 *      stored multiplied by d^-0.5 * log2(e), so their factor is fp32(127 / (r_q * that)): r_q is always the range of the un-scaled q);
 *   2. t[q][k] = fp32(int32 sum_c q_q k_q) * c,  c = fp32(s_q * s_k * d^-0.5 * log2 e) (the product formed in double, rounded once);
 *   3. m[q] = max_k t (the true row max);  p_q = rint(127 * exp2(t - m)), 0 .. 127 (t - m, the exp2 and the product each fp32);
 *   4. N[q][c] = int32 sum_k p_q v_q,  L[q] = sum_k p_q: exact (127^2 S < 2^31 up to S = 133 120);
 *   5. out = fp16(fp32(N) * (s_v / fp32(L))), every operation rounded to fp32 on its own.
 * The result does not depend on the launch geometry; the only inexact step is the hardware exp2.
 * sd_op_attention_w8a8: q_q, k_q, v_q (B * S, heads * 64) int8 token-major in natural key order -> out (B * S, heads * 64) f16
 * token-major; the entry builds the device images (q | k rows of one matrix, V^T in the kernel's key order) on the host.  Host checks,
 * in this order, each SD_ERR_INVALID_ARGUMENT before any device work: (1) a NULL pointer or B, heads or S < 1, (2) S not a multiple
 * of 64, (3) S > 133 120, (4) a range that is not positive and finite, (5) an input value of -128 (q, then k, then v).
 * sd_op_einsum_quantize: the quantizer launch on a handle's layouts - qk (B * S, 2C) f16 = q | k rows, vt (B, C, ldv) f16 V^T in the key
 * order vt_perm_in (0 natural, 1 the fp16 kernel's: the middle 4-key blocks of every 16 keys swapped) -> qk_q (B * S, 2C) int8 and vt_q
 * (B, C, S) int8 in the int8 kernel's key order; q_range_eff = the range of the STORED queries (r_q, times the pre-scale where the
 * producer applied one).  S a multiple of 32, C of 8, ldv of 4.
 * sd_op_w8a8_pack_vt (host only; *bytes = B * C * S, vt_q may be NULL): v (B * S, C) int8 token-major -> vt_q (B, C, S), position p of
 * every 32 keys holding key (p & 3) + 8 * ((p >> 2) & 3) + 4 * (p >> 4) of them - the order in which a lane's score registers become
 * the byte operand of the P.V MFMA. */
int sd_op_attention_w8a8(const int8_t* q_q, const int8_t* k_q, const int8_t* v_q, float q_absmax, float k_absmax, float v_absmax, void* out, int B,
                         int heads, int S, int iters, float* ms);
int sd_op_einsum_quantize(const void* qk, const void* vt, int B, int S, int C, int ldv, int vt_perm_in, float q_range_eff, float k_absmax,
                          float v_absmax, int8_t* qk_q, int8_t* vt_q, int iters, float* ms);
int sd_op_w8a8_pack_vt(const int8_t* v, int B, int C, int S, int8_t* vt_q, size_t* bytes);
/* The host weight quantizer of sd_weights_quantize_w8a8 on its own: w (Cout, per_row) f32 -> q (Cout, per_row) int8, w_scale (Cout)
 * f32, *sq_err (may be NULL).  A non-finite weight is SD_ERR_INVALID_ARGUMENT. */
int sd_op_quantize_weight(const float* w, int Cout, size_t per_row, int8_t* q, float* w_scale, double* sq_err);
/* max |x| over n f16 values on the device (the observers' kernel, misc.hip): exactly the fp32 value of the largest magnitude. */
int sd_op_absmax(const void* x, size_t n, float* absmax);
/* smgemm.hip from PALETTIZED weights (plan tile 15): w = lut[indices], indices (Cout, Cin) uint8; x (B,Cin,H,W), res/out (B,Cout,H,W) f16 NCHW;
 * bm 0 / 32 / 64 (0: by M as tile 12). Bit-identical to sd_op_conv2d(tile 141 / 142) on the fp16 weights lut[indices].
 * plan_out[4] = {15, 1|2, 1, 0}.  Checked on the host in this order, before any device work, each SD_ERR_INVALID_ARGUMENT: nbits not in
 * {1, 2, 4, 6, 8}; bm not in {0, 32, 64}; NULL or empty arguments; an index >= 2^nbits (the message names `index N` and its element); a
 * shape the small-M GEMM does not tile (Cin % 64, Cout % 80, M = B*H*W % bm, at least 2 x 2 tiles, their number a multiple of 8). */
int sd_op_gemm_palettized(const void* x, const void* lut, int nbits, const uint8_t* indices, const float* bias, const void* res, void* out,
                          int B, int Cin, int H, int W, int Cout, int bm, int* plan_out, int iters, float* ms);
/* The index bit stream that entry and the UNet builder put on the device (host only, no GPU): indices (Cout, K) uint8, Cout % 16 == 0,
 * K % 64 == 0 -> *bytes = (Cout / 16) * groups * nbits * 1024 with groups = ceil(K / 512); stream may be NULL (size query).  The wave of
 * 16-row strip n / 16 consumes K in stages of 64, in groups of 8 stages; lane l = 16 g + r16 owns, per stage s and sub-step kk = 0, 1, the
 * indices of W[16 strip + r16][64 s + 32 kk + 8 g + e], e = 0..7.  Its 128 indices of a group, in the order (s, kk, e), are
 * little-endian nbits-wide fields (field f at bits [f * nbits, (f + 1) * nbits)) filling exactly nbits 16-byte words; word q lies at
 * [strip][group][q][lane][16 B].  Fields of stages beyond K / 64 in the last group are zero. */
int sd_op_palette_pack_gemm(const uint8_t* indices, int Cout, int K, int nbits, uint8_t* stream, size_t* bytes);
/* smgeglu.hip from PALETTIZED weights (plan tile 16): the GEGLU projection of sd_op_geglu_ln with w = lut[indices], indices (N2, C) uint8
 * in the checkpoint's row order [values | gates]; x (M, C) f16, ln_weight / ln_bias (C) f32 or both NULL (plain GEGLU), bias (N2) f32 or
 * NULL -> out (M, N2 / 2) f16.  With the LayerNorm the kernel multiplies every LUT value by ln_weight (fp32 product, one rounding to
 * fp16) as the host fold does.  Bit-identical to sd_op_geglu_ln(kernel = 101) on the fp16 weights lut[indices].  bm 0 / 128 / 256
 * (0: by the grid as tile 13); only 128-row tiles are built, so bm = 256 - or bm = 0 on a shape tile 13 would give 256 rows - is
 * refused.  plan_out[4] = {16, 1, 1, 0}.  Checked on the host in this order, before any device work, each SD_ERR_INVALID_ARGUMENT:
 * nbits not in {1, 2, 4, 6, 8}; bm not in {0, 128, 256}; NULL or empty arguments; exactly one of ln_weight / ln_bias given; an index >=
 * 2^nbits (the message names `index N` and its element); a shape the kernel does not tile (C % 64, C <= 2560, N2 % 160, M % 128, at
 * least 2 x 2 tiles, their number a multiple of 8, 128-row tiles). */
int sd_op_geglu_palettized(const void* x, const float* ln_weight, const float* ln_bias, const void* lut, int nbits, const uint8_t* indices,
                           const float* bias, void* out, int M, int C, int N2, float eps, int bm, int* plan_out, int iters, float* ms);
/* The index bit stream that entry and the UNet builder put on the device (host only, no GPU): indices (N2, K) uint8 in the
 * checkpoint's row order, N2 % 32 == 0, K % 64 == 0 -> *bytes = (N2 / 16) * groups * nbits * 1024 with groups = ceil(K / 512); stream
 * may be NULL (size query).  It is the stream of sd_op_palette_pack_gemm over 16-row strips in the order the kernel stages them: strip
 * 2 U + v holds the checkpoint rows v * N2 / 2 + 16 U + r16, r16 = 0..15 - the value (v = 0) or gate (v = 1) rows of output columns
 * 16 U .. 16 U + 15.  Per strip as there: K in stages of 64, groups of 8 stages; lane l = 16 g + r16 owns, per stage s and sub-step
 * kk = 0, 1, the indices of row r16 of the strip at columns 64 s + 32 kk + 8 g + e, e = 0..7; its 128 indices of a group, in the order
 * (s, kk, e), are little-endian nbits-wide fields (field f at bits [f * nbits, (f + 1) * nbits)) filling exactly nbits 16-byte words;
 * word q lies at [strip][group][q][lane][16 B].  Fields of stages beyond K / 64 in the last group are zero. */
int sd_op_palette_pack_geglu(const uint8_t* indices, int N2, int K, int nbits, uint8_t* stream, size_t* bytes);
/* The same conv followed by torch.nn.GroupNorm (+ SiLU) of its output (unet.py:470-489 conv -> norm -> SiLU; stride 1, no
 * upsample): with producer_stats = 1 the GroupNorm statistics come out of the conv kernel's own epilogue (one launch less per
 * GroupNorm), with 0 from the GroupNorm's own statistics pass.  *entries (may be NULL) returns the number of partial
 * (sum, sumsq) entries per (sample, group) the conv wrote - 0 when its plan cannot produce them.  conv_out (may be NULL) receives
 * the conv result, out the normalised tensor; both (B, Cout, H, W) f16 NCHW. */
int sd_op_conv2d_groupnorm(const void* x, const void* w, const float* bias, const void* res, const float* gn_weight,
                           const float* gn_bias, void* conv_out, void* out, int B, int Cin, int H, int W, int Cout, int ksize,
                           int groups, float eps, int silu, int tile, int producer_stats, int* entries, int iters, float* ms);
/* conv -> torch.nn.GroupNorm (no SiLU) -> 1x1 projection: a resnet's last conv followed by SpatialTransformer.norm + proj_in
 * (unet.py:528-531 eps 1e-6, :553-556).  fold = 1: the GroupNorm is applied inside the projection GEMM (statistics from the
 * conv's epilogue, per-channel mean / scale / shift applied to the GEMM's activation fragments: no GroupNorm launch);
 * fold = 0: GroupNorm launch + plain GEMM.  *entries (may be NULL) returns the number of statistics entries the fold consumed
 * (0: it fell back to the GroupNorm launch because the conv's plan wrote none).  proj_w (Nproj, Cout) f16, proj_bias (Nproj)
 * f32 or NULL; conv_out (may be NULL) (B, Cout, H, W), out (B, Nproj, H, W) f16 NCHW. */
int sd_op_conv2d_groupnorm_proj(const void* x, const void* w, const float* bias, const void* res, const float* gn_weight,
                                const float* gn_bias, const void* proj_w, const float* proj_bias, void* conv_out, void* out, int B,
                                int Cin, int H, int W, int Cout, int ksize, int Nproj, int groups, float eps, int fold, int tile,
                                int* entries, int iters, float* ms);
/* conv -> torch.nn.GroupNorm (+ SiLU) -> 3x3 conv (stride 1, padding 1): a ResnetBlock2D's norm2 -> SiLU -> conv2 behind conv1, or
 * norm1 -> SiLU -> conv1 behind the previous block (unet.py:470-489).  fold = 1: the GroupNorm (+ SiLU) is applied in the HALO
 * LOADER of the second conv (statistics from the first conv's epilogue; every wave normalises the halo pieces it fetched, in LDS;
 * pixels outside the image stay zero - the conv pads the NORMALISED tensor): no GroupNorm launch, no round trip of the normalised
 * tensor; fold = 0: GroupNorm launch + plain conv.  *entries (may be NULL): statistics entries the loader consumed (0: it fell
 * back).  w2 (N2, Cout, 3, 3) f16, bias2 (N2) f32 or NULL, res2 (B, N2, H, W) f16 or NULL; staging2: ring code of the second conv
 * (0 = plan table).  conv_out (may be NULL) (B, Cout, H, W), out (B, N2, H, W) f16 NCHW. */
int sd_op_conv2d_groupnorm_conv3x3(const void* x, const void* w, const float* bias, const void* res, const float* gn_weight,
                                   const float* gn_bias, const void* w2, const float* bias2, const void* res2, void* conv_out, void* out,
                                   int B, int Cin, int H, int W, int Cout, int ksize, int N2, int groups, float eps, int silu, int fold,
                                   int tile, int staging2, int* entries, int iters, float* ms);
/* The tail of a SpatialTransformer (unet.py:591 FeedForward.net.2 + residual, :561-563 proj_out + residual):
 * out = res2 + proj_out(res1 + ff.net.2(g) + b1) + b2.  fused = 1: ONE launch (32 tokens x 5 waves per workgroup, C = 320,
 * S % 32 == 0; the intermediate never goes to HBM), fused = 0: the two 1x1 GEMMs.  g (B, 4C, 1, S), res1 / res2 / out (B, C, 1, S) f16,
 * w1 (C, 4C), w2 (C, C) f16, b1 / b2 (C) f32.  gn_sums (may be NULL): (B, groups, 2) f32 - the GroupNorm statistics (sum, sum of
 * squares per sample and group) the launch left for a consuming GroupNorm, folded; NaN when it left none.
 * fused = 2 .. 5: the merged tail - the weights folded on the device ([w2 w1 | w2], bias w2 b1 + b2: sd_op_fold_linear, outside the timed
 * region) and ONE GEMM over the K-concatenation [g | res1] with residual res2, any C % 64 == 0: 2 = on the library's own plan, 3 = forced
 * onto the tiled igemm kernels, 4 / 5 = forced onto smgemm.hip's 32- / 64-row tiles (SD_ERR_INVALID_ARGUMENT for a shape the forced kernel
 * does not tile).  gn_sums with 2 and 3 as with 0. */
int sd_op_ffn_out_proj(const void* g, const void* w1, const float* b1, const void* res1, const void* w2, const float* b2, const void* res2,
                       void* out, float* gn_sums, int B, int C, int S, int groups, int fused, int iters, float* ms);
/* Debug entry of the weight fold behind the merged tail (wfold.hip): wm_out (N, K) f16 = fp16(wp w2) with fp32 accumulation in a fixed
 * order and one round-to-nearest-even, bm_out (N) f32 = bp + wp b2.  wp (N, J), w2 (J, K) f16, bp (N), b2 (J) f32. */
int sd_op_fold_linear(const void* wp, const float* bp, const void* w2, const float* b2, void* wm_out, float* bm_out, int N, int J, int K);
/* Cross-attention front half as one launch (unet.py:87-118 inside :586-591): out = softmax(to_q(LayerNormANE(x)) k^T / 8) v
 * per head, head dim 64, Sk <= 96 (the prompt), any Sq >= 1 (ragged last token tile).  V^T columns [Sk, round_up(Sk, 8)) must be
 * zero (this entry point zero-fills them; the masked probabilities there are 0 but 0 * inf would be NaN).  x (B, heads*64, 1, Sq), k / v (B, heads*64, 1, Sk) f16 BC1S,
 * ln_weight / ln_bias (C) f32 as in the checkpoint (x_hat * w + b), wq (C, C) f16 -> out (B, C, 1, Sq) f16.  nst: LDS-DMA
 * ring depth 2-4 (0 = heuristic). */
int sd_op_cross_attention_fused(const void* x, const float* ln_weight, const float* ln_bias, const void* wq, const void* k,
                                const void* v, void* out, int B, int heads, int Sq, int Sk, float eps, int nst, int iters,
                                float* ms);
/* The whole cross-attention branch of a BasicTransformerBlock (unet.py:586-591 around :87-118):
 * out = x + to_out(softmax(to_q(LayerNormANE(x)) k^T / 8) v) + bo.  fused = 1: ONE launch (xattn_out.hip: 32 tokens x all heads per
 * workgroup; 5 or 10 heads of 64, Sq % 32 == 0), fused = 0: the fused q-projection + attention launch followed by the to_out GEMM
 * with its residual epilogue.  Layouts as sd_op_cross_attention_fused; wo (C, C) f16, bo (C) f32.
 * a1 != NULL (with wo1, bo1): the SELF-attention's output projection in front (unet.py:588): the branch runs on
 * h1 = x + to_out1(a1) + bo1 (a1 the self-attention's output, x the block input) and out = h1 + to_out(...) + bo; the one-launch
 * form (5 heads only) never stores h1. */
int sd_op_cross_attention_block(const void* x, const float* ln_weight, const float* ln_bias, const void* wq, const void* k, const void* v,
                                const void* wo, const float* bo, const void* a1, const void* wo1, const float* bo1, void* out, int B, int heads,
                                int Sq, int Sk, float eps, int fused, int iters, float* ms);
/* GEGLU feed-forward first half (unet.py:609-617): x (M, C) f16, w (8C', C) f16, bias (8C'/.. ) */
int sd_op_geglu(const void* x, const void* w, const float* bias, void* out, int M, int C, int N2, int iters, float* ms);
/* The same projection with the LayerNorm in front of it folded into the GEMM, as the UNet runs it (unet.py:583-591 norm3 ->
 * :609-617; host-side fold of UNet::fold_layernorm): x (M, C) f16 UN-normalised, ln_weight / ln_bias (C) f32 or both NULL,
 * w (N2, C) f16, bias (N2) f32 or NULL -> out (M, N2 / 2) f16.  kernel: 0 = the library's plan, 1 = the tiled GEMM kernels,
 * 2 = the weight-stationary kernel (wsgemm.hip: C = 320, N2 % 256 == 0, M >= 2048; other shapes -> SD_ERR_INVALID_ARGUMENT),
 * 3-9 = bvgemm.hip (its own choice / variants 1-6), 100 = the one-round kernel of smgeglu.hip (plan tile 13: BM x 80 output tiles,
 * one workgroup per CU) with the tile height BM by the grid size, 101 / 102 = BM 128 / 256 forced.  100-102 need C % 64 == 0,
 * N2 % 160 == 0, M % BM == 0, at least two tiles each way and a tile count that is a multiple of 8; other shapes ->
 * SD_ERR_INVALID_ARGUMENT.  110-112 = 100-102 through the kernel's phase-clock build, which prints its per-wave cycle table to
 * stderr (measurement tools only). */
int sd_op_geglu_ln(const void* x, const float* ln_weight, const float* ln_bias, const void* w, const float* bias, void* out, int M, int C,
                   int N2, float eps, int kernel, int iters, float* ms);
/* Fused q|k|v projection of self-attention with norm1 folded in (unet.py:583-586 -> :74-84 as ONE GEMM): x (B * HW, C) f16,
 * ln_weight / ln_bias (C) f32, w (3C, C) f16 = [Wq | Wk | Wv] -> out_qk (B * HW, 2C) f16 with the queries multiplied by q_scale
 * before the rounding, out_vt (B, C, HW) f16 = V^T (vt_perm != 0: the two middle 4-token blocks of every 16 tokens swapped, the key
 * order of the d = 64 attention kernel).  kernel: 0 = the library's plan, 1 = the tiled kernels, 3 = bvgemm.hip, 4 + v = its variant v + 1. */
int sd_op_qkv_ln(const void* x, const float* ln_weight, const float* ln_bias, const void* w, void* out_qk, void* out_vt, int B, int HW, int C,
                 float eps, float q_scale, int vt_perm, int kernel, int iters, float* ms);
/* The head of a SpatialTransformer (unet.py:553-556 norm -> proj_in; :583-586 norm1 -> :74-84 fused to_q | to_k | to_v) behind a 1x1 conv
 * x = conv_w . x_in that leaves the GroupNorm statistics of x in its epilogue, as the resnet conv in front of it does in the UNet.
 * fused = 1: GroupNorm apply, proj_in, LayerNorm and the q|k|v projection in ONE launch (2 / 3: forced to 64 / 32 tokens per workgroup;
 * 64 needs H * W % 64 == 0); 0: the three launches it replaces.
 * x_in (B, C, H, W) f16; conv_w / proj_w (C, C) f16; gn_*, proj_bias, ln_* (C) f32; wqkv (3C, C) f16 -> out_h (B * H * W, C) = proj_in's
 * output, out_qk (B * H * W, 2C) with pre-scaled queries, out_vt (B, C, H * W) (vt_perm as sd_op_qkv_ln), all f16.  C = 320 only.
 * *entries: the producer's statistics entries per (sample, group) folded by the fused launch (0: fall-back GroupNorm launch). */
int sd_op_gn_proj_qkv(const void* x_in, const void* conv_w, const float* gn_weight, const float* gn_bias, const void* proj_w,
                      const float* proj_bias, const float* ln_weight, const float* ln_bias, const void* wqkv, void* out_h, void* out_qk,
                      void* out_vt, int B, int H, int W, int C, int groups, float gn_eps, float ln_eps, float q_scale, int vt_perm, int fused,
                      int* entries, int iters, float* ms);
/* unet.py:703-728 */
int sd_op_timestep_embedding(const float* t, float* out, int n, int dim, int flip_sin_to_cos, float freq_shift);
/* The kernel behind sd_vae_encode_latents alone (Encoder.swift:68-89 + Scheduler.swift:83-102): moments (2 * Cz, h, w) f32 =
 * [mean | logvar], eps (Cz, h, w), noise and out (n_images, Cz, h, w) f32. */
int sd_op_posterior_noise(const float* moments, const float* eps, const float* noise, float* out, int Cz, int h, int w, int n_images,
                          float scale_factor, float sa, float sb, int iters, float* ms);
/* One launch of the loop's step kernel (csrc/misc.hip cfg_sched_step_kernel; pipeline.py:561-569, the update rule documented at
 * sd_unet_denoise_loop) on host arrays: noise_pred (cfg * n_images, n) f32, rows [uncond..., cond...]; latents (n_images, n) in/out;
 * hist (history, n_images, n) in/out, or NULL with history = 0; coef: one row of 8; pred: one row of 8 or NULL; step_noise
 * (n_images, n) or NULL; cfg 1 or 2; history 0..3; denoised (n_images, n) out, needed exactly when pred is given.  *step_after:
 * the device step counter behind the launch (it starts at 0, so 1); the arrival ticket must be back at 0, else SD_ERR_INTERNAL.
 * Every device output sits in front of a poisoned guard that the launch must leave alone. */
int sd_op_sched_step(const float* noise_pred, float* latents, float* hist, const float* coef, const float* pred, const float* step_noise,
                     float guidance, int cfg, int history, int n_images, int n, float* denoised, int* step_after);
/* Which plan does the library give a conv / 1x1 GEMM of this shape?  Host only, read only: needs no GPU and launches nothing.
 * The descriptor as plain ints: C0 (+ C1 > 0: a second, channel-concatenated source) -> N over B x Ho x Wo outputs, up = 1 / 2 (nearest
 * upsample in the gather), out_mode 0 plain, 1 token-transposed, 2 GEGLU; flags: 1 LayerNorm fold, 2 timestep embedding, 4 residual,
 * 8 GroupNorm statistics wanted from the epilogue, 16 bias, 32 explicit zero padding (the stride-2 downsample of the VAE encoder),
 * 64 the upsampler as four 2x2 phase convs (plan tile 21 or SD_ERR_INVALID_ARGUMENT naming the refusal; without it no answer changes);
 * n_trans > 0: fused q|k|v with that many row-major columns; n_twins: GroupNorm twins written by the slab combine; gnf_groups > 0:
 * GroupNorm of the input folded into the launch; tile / staging / splitk: a forced plan (0 = the library's); copies: which pre-tiled
 * weight copies exist (1 wstream, 2 wsgemm, 4 bvgemm; -1 = the ones the library's handle would hold).
 * plan[7] = plan tile (1-4 igemm tiles, 7 halo conv, 9 wstream, 10 wsgemm, 11 bvgemm, 12 smgemm, 13 smgeglu, -1 off the MFMA path; the
 * palettized tiles 14 / 15 / 16 need a palette and are never an answer here: a handle takes 15 exactly where this says 12
 * (sd_op_gemm_palettized) and 16 where this says 13 with 128-row tiles (sd_op_geglu_palettized); tile = 17 asks for a W8A8
 * descriptor - the answer is 17 with the slab count of its wave code (staging 4: four waves, else eight), or SD_ERR_INVALID_ARGUMENT for
 * a shape the weight stream does not take; a handle takes 17 exactly where this says 9 and the tensor carries a W8A8 mark; tile = 18
 * asks for a W8A8 descriptor of the halo conv - the answer is 18 with tile 7's ring code, split-K and workspace for the same staging /
 * splitk, or SD_ERR_INVALID_ARGUMENT naming plan tile 18 for a shape it does not take; a handle takes 18 exactly where this says 7
 * without gnf_groups, Ctot <= 14 784 and the tensor carries a W8A8 mark; tile = 19 asks for a W8A8 descriptor of the small-M 1x1 GEMM -
 * the answer is 19 with the resolved tile height of the same staging (1 / 2 = 32 / 64 rows), split-K 1, no slab, no workspace, or
 * SD_ERR_INVALID_ARGUMENT naming plan tile 19 for a shape it does not take; a handle takes 19 exactly where this says 12 for a
 * single-source plain projection at a consenting call site and the tensor carries a W8A8 mark; tile = 20 asks for a W8A8 descriptor of
 * the GEGLU projection - the answer is 20 with the resolved tile height of the same staging (1 / 2 = 128 / 256 rows), split-K 1, no slab,
 * no workspace, or SD_ERR_INVALID_ARGUMENT naming plan tile 20 for a shape it does not take (the LayerNorm fold, flags & 1, among
 * them); a handle takes 20 exactly where this says 13 for ff.net.0.proj and the tensor carries a W8A8 mark; tile = 22 asks for a W8A8
 * descriptor of the fused q|k|v projection (N = 3 C0, n_trans = 2 C0, no flags) - the answer is 22 with the resolved tile height of
 * the same staging (1 / 2 = 128 / 256 rows, 0 = by the grid), split-K 1, no slab, no workspace, or SD_ERR_INVALID_ARGUMENT naming plan
 * tile 22 for a shape off its rule (sd_op_qkv_w8a8); it has no fp16 twin: a handle takes 22 for every fused q|k|v launch on the rule
 * whose three tensors carry W8A8 marks with one range; tile = 24 asks for a W8A8 descriptor of the small-M 1x1 GEMM whose activations
 * arrive as int8 - the answer is 24 with the resolved tile height of the same staging (1 / 2 = 32 / 64 rows), split-K 1, no slab, no
 * workspace, or SD_ERR_INVALID_ARGUMENT naming plan tile 24 for a shape it does not take: tile 19's shapes (sd_op_gemm_q8); a handle
 * takes it for a marked ff.net.2 on the rule stated at sd_weights_quantize_w8a8; 23 is not in use),
 * staging, resolved split-K, slab (0 / 1), then the copies a handle must hold for this conv: wstream, wsgemm, bvgemm (0 / 1 each).
 * *workspace_bytes: the slab workspace this launch needs. */
int sd_op_conv_plan(int ksize, int stride, int up, int C0, int C1, int N, int B, int Ho, int Wo, int out_mode, int flags, int n_trans,
                    int n_twins, int gnf_groups, int tile, int staging, int splitk, int copies, int* plan, unsigned long long* workspace_bytes);
/* No reference counterpart.  The same question with the same 18 descriptor arguments, answered with the kernel that launches: one
 * NUL-terminated line in text[text_bytes] (64 bytes hold every answer) in the format of csrc/conv_plan.h conv_plan_kernel_name, e.g.
 * "igemm 64x64 ring4 kg2", "gemm_pipe 128x64 ring3", "halo_ks ring6", "halo_i8 ring4", "wstream waves8", "bvgemm v3", "smgemm bm32", "smgemm_i8 bm32", "smgemm_q8 bm32", "generic":
 * kernel family, tile, the ring depth that runs after the fall-back to one that fits the LDS, in-workgroup K groups, register
 * staging, wave count, variant - what the (tile, staging) codes of sd_op_conv_plan mean for this descriptor.  Host only. */
int sd_op_conv_plan_kernel(int ksize, int stride, int up, int C0, int C1, int N, int B, int Ho, int Wo, int out_mode, int flags, int n_trans,
                           int n_twins, int gnf_groups, int tile, int staging, int splitk, int copies, char* text, int text_bytes);
/* numpy legacy stream: np.random.seed(seed); np.random.randn(n) (pipeline.py:331,:726;
 * NumPyRandomSource.swift:28-102).  Host-side, bit-exact. */
int sd_numpy_randn(uint32_t seed, double* out, size_t n);
/* the other two seed-exact sources of the reference (RandomSource.swift): torch's CPU generator
 * (`torch.manual_seed(seed); torch.randn(n)`, TorchRandomSource.swift:116-150) and torch's CUDA generator
 * (Philox4x32-10, NvRandomSource.swift:25-80; `offset` = number of arrays drawn before).  Host-side. */
int sd_torch_randn(uint32_t seed, double* out, size_t n);
int sd_philox_randn(uint64_t seed, uint32_t offset, double* out, size_t n);
/* Box calibration for bench.py (no reference counterpart: measurement infrastructure).  out9[0] = device copy GB/s (1 GiB,
 * read + written bytes), out9[1] = dense v_mfma_f32_32x32x16_f16 register loop TFLOP/s, out9[2] = us per launch of a captured
 * graph of 323 empty launches (the step's launch count), out9[3] = us per launch of a 323-launch chain of short dependent
 * kernels on cold operands, out9[4] = us per launch of a 323-launch chain in which every workgroup reads 16 KB that a workgroup
 * on ANOTHER XCD wrote in the previous launch (8 MB handed over per launch), out9[5] / out9[6] = ns per dependent load from
 * never-touched HBM lines / from a 2-MB table resident in the caches, out9[7] = us per launch of a 323-launch chain of SMALL
 * grids (64 workgroups: 4 MB read, a reduction behind one barrier, 4 MB written - the shape of the launches that a slow box of the
 * pool runs 1.3-2 x slower - and which reads the same on them), out9[8] = COLD CODE: us per launch of a 320-launch chain that walks 32
 * different kernels of ~30 KB of code each minus the same chain repeating one of them - 0.8 us on the fast boxes of the pool, 11 us
 * on the slow ones: the figure `value_normalised` is built on.  Nine floats.  Allocates and frees 2 GiB of device memory; synchronous. */
int sd_calibrate(int device, float* out9);
/* MFMA fragment layout self-check used by the build/smoke tests (returns 0 when the hardware
 * layout matches what the kernels assume; bit 0 the f16 MFMA, bits 1 / 2 the cross-lane exchanges, bit 3 the 32x32x32 int8 MFMA of the W8A8
 * convs, bit 4 the 16x16x64 int8 MFMA of the W8A8 small-M GEMM). */
int sd_selftest_mfma(void);

/* ------------------------------------------------------------------------------------------
 * Safety checker: diffusers' StableDiffusionSafetyChecker (transformers' CLIPVisionModel ViT-L/14, visual_projection and
 * the concept head) as the reference converts it (torch2coreml.py:1119-1309, the head's vectorised forward :1177-1209) and
 * runs it on every generated image (pipeline.py:286-311, step 9 at :578; SafetyChecker.swift; `disableSafety` of the Swift
 * configuration).  Static batch like every model.  Weights use the key names diffusers writes
 * (vision_model.vision_model.embeddings.* / .pre_layrnorm.* (sic) / .encoder.layers.N.* / .post_layernorm.*,
 * visual_projection.weight, concept_embeds, special_care_embeds, concept_embeds_weights, special_care_embeds_weights);
 * a single `vision_model.` prefix is accepted too.  A missing key is SD_ERR_NOT_FOUND, a wrong shape or bad config
 * SD_ERR_INVALID_ARGUMENT, a head dim other than 64 SD_ERR_UNSUPPORTED - all before any device work.
 * `filtered_images` (torch2coreml.py:1203-1207) is deliberately NOT part of this ABI: the images are on the host at that
 * point (pipeline.py:286-311), blackening a flagged one is a host memset, done by the Python wrapper.
 * ------------------------------------------------------------------------------------------ */
typedef struct sd_safety_checker_config {
  int32_t batch, image_size /*224*/, patch_size /*14*/, hidden_size, intermediate_size,
          num_hidden_layers, num_attention_heads, projection_dim, num_concepts /*17*/,
          num_special /*3*/, hidden_act /*0 quick_gelu, 1 gelu*/;
  float layer_norm_eps;
  int32_t use_graph;
} sd_safety_checker_config;
typedef struct sd_safety_checker sd_safety_checker;
/* replaces the load of the converted safety_checker model (pipeline.py:650-656 in get_coreml_pipe; SafetyChecker.swift:21-33) */
int sd_safety_checker_create(const sd_safety_checker_config* cfg, const sd_weights* w, int device, sd_safety_checker** out);
void sd_safety_checker_destroy(sd_safety_checker* c);
size_t sd_safety_checker_device_bytes(const sd_safety_checker* c);
/* replaces `safety_checker(clip_input=, images=, adjustment=)` (pipeline.py:293-304; SafetyChecker.swift:55-99 isSafe).
 * clip_input (B,3,I,I) f16 (a device pointer with SD_FLAG_DEVICE_PTRS); outputs f32 on the host, each may be NULL: has_nsfw (B)
 * 0 / 1, concept_scores (B,num_concepts), image_embeds (B,projection_dim), last_hidden_state (B,S,hidden) BEFORE
 * post_layernorm (transformers' meaning of the name) */
int sd_safety_checker_run(sd_safety_checker* c, const void* clip_input, float adjustment, float* has_nsfw,
                          float* concept_scores, float* image_embeds, float* last_hidden_state, int flags);
/* Measurement hook (no reference counterpart): HIP-event milliseconds of the launch list of the last sd_safety_checker_run - the
 * graph replay, or the eager launches - without the copies in front of and behind it; 0 before the first run. */
float sd_safety_checker_last_ms(const sd_safety_checker* c);
/* operator-level entries, same conventions as the other sd_op_*.
 * CLIPAttention of the vision tower (no mask), head dim 64 only (else SD_ERR_UNSUPPORTED): qkv (B*S, 3*heads*d) f16 rows
 * [q | k | v] as the stacked projection writes them -> out (B*S, heads*d) f16; any S >= 1. */
int sd_op_vit_attention(const void* qkv, void* out, int B, int S, int heads, int d, int iters, float* ms);
/* the concept head (torch2coreml.py:1177-1209), all f32: image_embeds (B,P), concept_embeds (n_concepts,P), special_embeds
 * (n_special,P), thresholds concept_w / special_w -> has_nsfw (B) 0 / 1, concept_scores (B,n_concepts) */
int sd_op_safety_head(const float* image_embeds, const float* concept_embeds, const float* special_embeds,
                      const float* concept_w, const float* special_w, float adjustment, int B, int P,
                      int n_concepts, int n_special, float* has_nsfw, float* concept_scores);

/* ------------------------------------------------------------------------------------------
 * Image post-processing on the device: from the decoder's last conv to the 8-bit image and the safety verdict without a detour
 * through the host.  Replaces, bit for bit, what the reference does in numpy, PIL and transformers' CLIPImageProcessor between its two
 * models (pipeline.py:286-320: decode_latents' clip and transpose, numpy_to_pil, the feature extractor's 8-bit bicubic resize, centre
 * crop, rescale and normalise, the cast to fp16); Decoder.swift:40-68 (the decoder returns an 8-bit image), SafetyChecker.swift:55-99
 * (the checker takes the image and resizes and normalises it itself).
 *   quantise   q = rint(clamp(x * 0.5f + 0.5f, 0, 1) * 255.0f), round-half-to-even, uint8 (B, H, W, 3)
 *   resize     Pillow's 8-bit Image.resize(BICUBIC): two separable passes, horizontal first, the intermediate image rounded to uint8,
 *              22-bit fixed-point coefficients (sd_op_resample_coeffs); a pass whose size does not change is the identity
 *   crop       centre crop to S x S, S = the checker's image_size: top = (resize_h - S) / 2, left = (resize_w - S) / 2
 *   normalise  ((float)u / 255.0f - image_mean[c]) / image_std[c] in fp32, both divisions IEEE-rounded, then fp16 (RNE), (B, 3, S, S)
 * ------------------------------------------------------------------------------------------ */
/* The geometry and constants of CLIPImageProcessor as the checkpoint's preprocessor_config.json resolves them for this image size
 * (pipeline.py:288-291): the size the image is resized to before the crop, and the fp32 roundings of image_mean / image_std. */
typedef struct sd_image_post {
  int32_t resize_h, resize_w;
  float image_mean[3], image_std[3];
} sd_image_post;
/* replaces decode_latents + numpy_to_pil + the feature extractor + `safety_checker(...)` + filtered_images (pipeline.py:286-320,
 * torch2coreml.py:1203-1207; Decoder.swift:40-68 decode, SafetyChecker.swift:55-99 isSafe).  Runs the decoder like sd_vae_decode,
 * then the two kernels on the decoder's stream, feeds `checker` from device memory in slices of its static batch and zeroes the
 * flagged images in `image` and `rgb8`.  z / flags as in sd_vae_decode; image (B,3,H,W) f32 in [-1, 1] and rgb8 (B,H,W,3) follow
 * `flags` like `image` there; has_nsfw (B) 0 / 1 and concept_scores (B,num_concepts) are host memory as in sd_safety_checker_run.
 * image, rgb8 and checker (with post, has_nsfw, concept_scores) may each be NULL; a checker needs `post`.  With no checker this is
 * Decoder.swift's 8-bit output alone.  SD_ERR_INVALID_ARGUMENT before any device work: a decoder batch that is no multiple of the
 * checker's, handles on different devices, resize_h / resize_w below S; SD_ERR_UNSUPPORTED: an odd S, or a downscale so steep that a
 * tile's source rows exceed 64 KB of LDS. */
int sd_vae_decode_images(sd_unet* vae, const void* z, sd_dtype z_dtype, float* image, uint8_t* rgb8, sd_safety_checker* checker,
                         const sd_image_post* post, float adjustment, float* has_nsfw, float* concept_scores, int flags);
/* operator-level entries, same conventions as the other sd_op_*.
 * Pillow's coefficient tables of one axis, in_size -> out_size samples (the resize inside CLIPImageProcessor, pipeline.py:288-291).
 * Host only.  *ksize = taps per output sample; bounds (out_size, 2) = [first source index, tap count]; coeffs (out_size, *ksize),
 * zeros behind a row's taps.  A NULL table pointer is a size query: *ksize alone. */
int sd_op_resample_coeffs(int in_size, int out_size, int* ksize, int32_t* bounds, int32_t* coeffs);
/* numpy_to_pil's quantisation (pipeline.py:313-320 decode_latents + numpy_to_pil; Decoder.swift:40-68): image (B,3,H,W) f32 -> rgb8 (B,H,W,3) */
int sd_op_image_rgb8(const float* image, uint8_t* rgb8, int B, int H, int W, int iters, float* ms);
/* CLIPImageProcessor on 8-bit images (pipeline.py:288-291; SafetyChecker.swift:55-99): rgb8 (B,H,W,3) -> clip_input (B,3,S,S) f16
 * through a resize to rh x rw; mean3 / std3: three floats each */
int sd_op_clip_input(const uint8_t* rgb8, void* clip_input, int B, int H, int W, int rh, int rw, int S, const float* mean3,
                     const float* std3, int iters, float* ms);

/* ------------------------------------------------------------------------------------------
 * Operator-level entries of the kernels that otherwise run only inside whole models: the fp32 VAE path, the VAE's fp16 row
 * softmax, the time-embedding GEMV, the text encoder's own kernels and the copy kernels at the model boundaries.  Host tensors in
 * the reference's layouts; every refusal (SD_ERR_INVALID_ARGUMENT, SD_ERR_UNSUPPORTED) comes before any device work; every device
 * output sits in front of a guard of NaN patterns, and a launch that wrote into it fails the call (SD_ERR_INTERNAL).
 * ------------------------------------------------------------------------------------------ */
/* fp32 implicit-GEMM conv of an fp32 VAE handle: x (B,Cin,H,W) f32; w_kind 0: w f16 (N,Cin,k,k), 1: w f32 (N,Cin,k,k), 2: w f32
 * (Cin,N) with ksize 1 only (attention's P.V); bias (N) / res (B,N,Ho,Wo) f32 or NULL; ksize 1 / 3, stride 1 / 2, upsample 0 / 1
 * (nearest x2 in front), pad_mode as sd_op_conv2d_ex (1: the encoder's (0,1,0,1) padding) -> out (B,N,Ho,Wo) f32 */
int sd_op_conv_f32(const float* x, const void* w, int w_kind, const float* bias, const float* res, float* out, int B, int Cin,
                   int H, int W, int N, int ksize, int stride, int upsample, int pad_mode);
/* fp32 GroupNorm (+ SiLU) of an fp32 VAE handle: x (B,C,H,W) f32, gamma / beta (C) -> out (B,C,H,W) f32; C % groups != 0 is
 * SD_ERR_UNSUPPORTED */
int sd_op_groupnorm_f32(const float* x, const float* gamma, const float* beta, float* out, int B, int C, int H, int W, int groups,
                        float eps, int silu);
/* softmax(scale * x) over each row of x (rows, cols), in place: fp32 = 0 the f16 kernel (cols % 8 == 0 and <= 8192, else
 * SD_ERR_UNSUPPORTED), fp32 = 1 the f32 kernel (any cols) */
int sd_op_row_softmax(void* x, int rows, int cols, float scale, int fp32);
/* out[b][n] (+)= act_out(sum_k w[n][k] * act_in(x[b][k]) + bias[n]), act = SiLU where its flag is set: w (N,K) f16, bias (N) or
 * NULL, x (B,K) f32, out (B,N) f32 (read first with `accumulate`); K % 8 == 0 and <= 3072, else SD_ERR_UNSUPPORTED */
int sd_op_gemv(const void* w, const float* bias, const float* x, float* out, int B, int N, int K, int silu_in, int silu_out,
               int accumulate);
/* causal attention of the text encoder: qkv (S, 3 D) f16 rows [q | k | v] -> out (S, D) f16; S <= 80, head dim D / heads a
 * multiple of 8 and <= 128, else SD_ERR_UNSUPPORTED */
int sd_op_clip_attention(const void* qkv, void* out, int S, int D, int heads);
/* out[s] = tok[clamp(ids[s], 0, vocab - 1)] + pos[s]: ids (S) int32, tok (vocab, D) / pos (S, D) f16 -> out (S, D) f16;
 * D % 8 != 0 is SD_ERR_UNSUPPORTED */
int sd_op_clip_embed(const int32_t* ids, const void* tok, const void* pos, void* out, int S, int D, int vocab);
/* the CLIP MLP activation over n f16 values, in place: act 0 quick_gelu, 1 exact-erf gelu; n % 8 == 0 */
int sd_op_clip_act(void* x, size_t n, int act);
/* the copy kernels, src -> dst of B * C * H * W elements: kind 0 / 1 (B,C,H,W) f16 / f32 -> [B][H][W][C] f16; 2 / 3 the same to
 * f32; 4 / 5 [B][H][W][C] f16 / f32 -> (B,C,H,W) f32; 6 (B,C,1,S) f16 -> [B][S][C] f16 (H = 1, W = S); 7 f16 -> f32 and
 * 8 f32 -> f16 over the flat buffer */
int sd_op_layout(int kind, const void* src, void* dst, int B, int C, int H, int W);
/* out = srcs[0] + ... + srcs[nsrc - 1] over n f16 values, fp32 accumulation in source order, one rounding; 1 <= nsrc <= 4,
 * n % 8 == 0; add = 1 (nsrc 2 only): the two-source add kernel instead */
int sd_op_sum_half(const void* const* srcs, int nsrc, void* out, size_t n, int add);
/* img (B,3,I,I) f16 -> rows (B (I/p)^2, Kp) f16: column c p p + py p + px of a patch's row, columns [3 p p, Kp) zero */
int sd_op_vit_patch_rows(const void* img, void* rows, int B, int I, int p, int Kp);
/* out[b][0] = cls + pos[0], out[b][1 + j] = patch[b][j] + pos[1 + j]: patch (B, S - 1, D), cls (D), pos (S, D) f16 -> out
 * (B, S, D) f16; D % 8 != 0 or S < 2 is SD_ERR_UNSUPPORTED */
int sd_op_vit_tokens(const void* patch, const void* cls, const void* pos, void* out, int B, int S, int D);
/* Self-check of the operator harness (the guarded, poisoned device buffers every sd_op_* entry allocates): dst = (float)src over
 * n f16 values (2 <= n <= 2^24) with one deliberate off-by-one in the entry's own pointer arithmetic, inside its own allocations.
 * mode 0 clean -> SD_OK; 1 one element written behind dst / 2 in front of dst / 3 behind src -> SD_ERR_INTERNAL, the error names
 * the entry point, the buffer, "back guard" or "front guard" and the byte offset; 4 the last element skipped / 5 src read one
 * element behind its end -> SD_OK with dst[n - 1] NaN.  dst is written in every mode. */
int sd_op_harness_selftest(int mode, const void* src, float* dst, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* SD_MI355X_H */
