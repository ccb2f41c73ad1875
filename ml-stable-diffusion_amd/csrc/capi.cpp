// extern "C" surface of libsdmi355 (include/sd_mi355x.h).  Exceptions never cross the ABI:
// every entry point converts sd::Error into a status code + thread-local message.
// The operator-level sd_op_* entry points live in capi_ops.cpp.
#include <cmath>
#include <cstdlib>

#include "capi_util.h"
#include "safety_checker.h"

namespace sd {
int selftest_mfma();   // selftest.hip
}  // namespace sd

using namespace sd;

namespace {
// One handle type, three kinds (cfg.is_vae_decoder: 0 UNet / ControlNet, 1 VAE decoder, 2 VAE encoder): created here ...
void create_handle(const sd_unet_config* cfg, const sd_weights* w, int device, sd_unet** out, int vae_kind = -1) {
  SD_REQUIRE(cfg && w && out, kInvalidArgument, "NULL argument");
  require_device();
  sd_unet_config c = *cfg;
  if (vae_kind >= 0) {
    c.is_vae_decoder = vae_kind;
    c.is_controlnet = 0;
  }
  SD_REQUIRE(!c.compute_fp32 || c.is_vae_decoder, kUnsupported,
             "compute_fp32 is the VAE graphs' option (torch2coreml.py:570-578, :726-733); the UNet kernels store fp16");
  auto h = std::make_unique<sd_unet>();
  if (c.is_vae_decoder)
    h->impl = std::make_unique<Vae>(c, w->store, device);
  else
    h->impl = std::make_unique<UNet>(c, w->store, device);
  *out = h.release();
}
// ... and told apart here: `refusal` is what a VAE handle hears from an entry point of the UNet / ControlNet
UNet& unet_of(sd_unet* u, const char* refusal) {
  UNet* p = dynamic_cast<UNet*>(u->impl.get());
  SD_REQUIRE(p, kInvalidArgument, "%s", refusal);
  return *p;
}
// A handle whose device loop is inside its caller's progress handler (sd_unet_denoise_loop_progress) takes no other call: refused
// here, before any device work, and the loop goes on undisturbed.
void require_idle(const sd_unet* u, const char* entry) {
  const UNet* p = u ? dynamic_cast<const UNet*>(u->impl.get()) : nullptr;
  SD_REQUIRE(!p || !p->in_progress_handler(), kInvalidArgument,
             "%s: this handle is running sd_unet_denoise_loop_progress and is inside its progress handler; the handler may drive "
             "other handles only", entry);
}
Vae& vae_of(sd_unet* u, int kind) {
  Vae* p = dynamic_cast<Vae*>(u->impl.get());
  SD_REQUIRE(p && p->config().is_vae_decoder == kind, kInvalidArgument, "handle is not a VAE %s", kind == 2 ? "encoder" : "decoder");
  return *p;
}
}  // namespace

extern "C" {

const char* sd_last_error(void) { return g_last_error.c_str(); }
const char* sd_version(void) { return "libsdmi355 0.1 (gfx950)"; }

int sd_device_count(void) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    g_last_error = std::string("hipGetDeviceCount: ") + hipGetErrorString(e);
    return kHipError;
  }
  return n;
}

int sd_weights_create(sd_weights** out) {
  return guarded([&] {
    SD_REQUIRE(out != nullptr, kInvalidArgument, "out is NULL");
    *out = new sd_weights();
  });
}
int sd_weights_add(sd_weights* w, const char* name, const void* data, sd_dtype dtype, const int64_t* shape, int ndim) {
  return guarded([&] {
    SD_REQUIRE(w && name && data && shape, kInvalidArgument, "NULL argument");
    w->store.add(name, data, (int)dtype, shape, ndim);
  });
}
int sd_weights_load_safetensors(sd_weights* w, const char* path, const char* prefix) {
  return guarded([&] {
    SD_REQUIRE(w && path, kInvalidArgument, "NULL argument");
    w->store.load_safetensors(path, prefix ? prefix : "");
  });
}
int sd_weights_count(const sd_weights* w) { return w ? (int)w->store.size() : 0; }
int sd_weights_tensor_info(const sd_weights* w, int index, char* name, int name_bytes, int64_t* shape8, int* ndim) {
  return guarded([&] {
    SD_REQUIRE(w && name && name_bytes > 1 && shape8 && ndim, kInvalidArgument, "NULL argument");
    SD_REQUIRE(index >= 0 && (size_t)index < w->store.size(), kInvalidArgument, "tensor index %d of %zu", index, w->store.size());
    auto it = w->store.tensors().begin();
    std::advance(it, index);
    std::snprintf(name, (size_t)name_bytes, "%s", it->first.c_str());
    *ndim = (int)it->second.shape.size();
    std::copy(it->second.shape.begin(), it->second.shape.end(), shape8);
  });
}
int sd_weights_palettize(sd_weights* w, const char* name, int nbits, double* sq_err) {
  return guarded([&] {
    SD_REQUIRE(w && name, kInvalidArgument, "NULL argument");
    const double e = w->store.palettize(name, nbits);
    if (sq_err) *sq_err = e;
  });
}
int sd_weights_add_palettized(sd_weights* w, const char* name, const void* lut, int nbits, const uint8_t* indices, const int64_t* shape,
                              int ndim) {
  return guarded([&] {
    SD_REQUIRE(w && name && lut && indices && (shape || ndim == 0), kInvalidArgument, "NULL argument");
    w->store.add_palettized(name, lut, nbits, indices, shape, ndim);
  });
}
int sd_weights_palette_bits(const sd_weights* w, const char* name) {
  const Palette* p = (w && name) ? w->store.palette(name) : nullptr;
  return p ? p->nbits : 0;
}
int sd_weights_read_palette(const sd_weights* w, const char* name, void* lut, uint8_t* indices, float* values) {
  return guarded([&] {
    SD_REQUIRE(w && name, kInvalidArgument, "NULL argument");
    const HostTensor& t = w->store.get(name);
    const Palette* p = w->store.palette(name);
    SD_REQUIRE(p || (!lut && !indices), kInvalidArgument, "tensor '%s' has no palette", name);
    if (lut) std::copy(p->lut.begin(), p->lut.end(), reinterpret_cast<uint16_t*>(lut));
    if (indices) std::copy(p->indices.begin(), p->indices.end(), indices);
    if (values) std::copy(t.data.begin(), t.data.end(), values);
  });
}
int sd_weights_quantize_w8a8(sd_weights* w, const char* name, float act_absmax, double* sq_err) {
  return guarded([&] {
    SD_REQUIRE(w && name, kInvalidArgument, "NULL argument");
    const double e = w->store.quantize_w8a8(name, act_absmax);
    if (sq_err) *sq_err = e;
  });
}
int sd_weights_w8a8_info(const sd_weights* w, const char* name, float* act_scale) {
  const W8A8Mark* m = (w && name) ? w->store.w8a8(name) : nullptr;
  if (m && act_scale) *act_scale = m->act_absmax / 127.0f;
  return m ? 1 : 0;
}
int sd_weights_palette_halo(sd_weights* w, int on) {
  return guarded([&] {
    SD_REQUIRE(w, kInvalidArgument, "NULL argument");
    SD_REQUIRE(on == 0 || on == 1, kInvalidArgument, "sd_weights_palette_halo: %d (0 off, 1 on)", on);
    w->store.set_palette_halo(on != 0);
  });
}
int sd_weights_observe_activations(sd_weights* w, int on) {
  return guarded([&] {
    SD_REQUIRE(w, kInvalidArgument, "NULL argument");
    SD_REQUIRE(on >= 0 && on <= 2, kInvalidArgument, "sd_weights_observe_activations: level %d (0 off, 1 weight-stream convs, 2 every W8A8-eligible conv)", on);
    w->store.set_observe(on);
  });
}
int sd_weights_observe_gemms(sd_weights* w, int on) {
  return guarded([&] {
    SD_REQUIRE(w, kInvalidArgument, "NULL argument");
    SD_REQUIRE(on == 0 || on == 1, kInvalidArgument, "sd_weights_observe_gemms: %d (0 off, 1 on)", on);
    w->store.set_observe_gemms(on != 0);
  });
}
int sd_weights_observe_geglus(sd_weights* w, int on) {
  return guarded([&] {
    SD_REQUIRE(w, kInvalidArgument, "NULL argument");
    SD_REQUIRE(on == 0 || on == 1, kInvalidArgument, "sd_weights_observe_geglus: %d (0 off, 1 on)", on);
    w->store.set_observe_geglus(on != 0);
  });
}
int sd_weights_observe_qkv(sd_weights* w, int on) {
  return guarded([&] {
    SD_REQUIRE(w, kInvalidArgument, "NULL argument");
    SD_REQUIRE(on == 0 || on == 1, kInvalidArgument, "sd_weights_observe_qkv: %d (0 off, 1 on)", on);
    w->store.set_observe_qkv(on != 0);
  });
}
int sd_weights_observe_tails(sd_weights* w, int on) {
  return guarded([&] {
    SD_REQUIRE(w, kInvalidArgument, "NULL argument");
    SD_REQUIRE(on == 0 || on == 1, kInvalidArgument, "sd_weights_observe_tails: %d (0 off, 1 on)", on);
    w->store.set_observe_tails(on != 0);
  });
}
int sd_weights_observe_einsums(sd_weights* w, int on) {
  return guarded([&] {
    SD_REQUIRE(w, kInvalidArgument, "NULL argument");
    SD_REQUIRE(on == 0 || on == 1, kInvalidArgument, "sd_weights_observe_einsums: %d (0 off, 1 on)", on);
    w->store.set_observe_einsums(on != 0);
  });
}
int sd_weights_quantize_einsum(sd_weights* w, const char* name, float q_absmax, float k_absmax, float v_absmax) {
  return guarded([&] {
    SD_REQUIRE(w && name, kInvalidArgument, "NULL argument");
    w->store.quantize_einsum(name, q_absmax, k_absmax, v_absmax);
  });
}
int sd_weights_einsum_info(const sd_weights* w, const char* name, float* ranges) {
  const EinsumMark* m = (w && name) ? w->store.einsum(name) : nullptr;
  if (m && ranges) ranges[0] = m->q_absmax, ranges[1] = m->k_absmax, ranges[2] = m->v_absmax;
  return m ? 1 : 0;
}
int sd_weights_set_values(sd_weights* w, const char* name, const float* values, size_t n) {
  return guarded([&] {
    SD_REQUIRE(w && name && values, kInvalidArgument, "NULL argument");
    w->store.set_values(name, values, n);
  });
}
void sd_weights_destroy(sd_weights* w) { delete w; }

int sd_unet_create(const sd_unet_config* cfg, const sd_weights* w, int device, sd_unet** out) {
  return guarded([&] { create_handle(cfg, w, device, out); });
}
void sd_unet_destroy(sd_unet* u) { delete u; }
int sd_unet_reload_weights(sd_unet* u, const sd_weights* w, const char* const* names, int n_names) {
  return guarded([&] {
    SD_REQUIRE(u && w && n_names >= 0 && (n_names == 0 || names), kInvalidArgument, "NULL argument");
    require_idle(u, "sd_unet_reload_weights");
    SD_REQUIRE(dynamic_cast<UNet*>(u->impl.get()), kUnsupported, "sd_unet_reload_weights takes a UNet or ControlNet handle, not a VAE");
    std::vector<std::string> v;
    for (int i = 0; i < n_names; ++i) {
      SD_REQUIRE(names[i], kInvalidArgument, "names[%d] is NULL", i);
      v.emplace_back(names[i]);
    }
    u->impl->reload_weights(w->store, v);
  });
}
int sd_unet_set_attention(sd_unet* u, int impl) {
  return guarded([&] {
    SD_REQUIRE(u, kInvalidArgument, "NULL handle");
    require_idle(u, "sd_unet_set_attention");
    u->impl->set_attention(impl);
  });
}
// Debug ABI: process-global plan overrides exist for the tuning / race-guard tools only and are refused unless the
// process runs with SD_TUNE=1 (the product path has no global mutable state).
static void require_tune_env() {
  static const bool on = getenv("SD_TUNE") != nullptr;
  SD_REQUIRE(on, kUnsupported, "sd_tune_* is a debug ABI: set SD_TUNE=1 in the environment to enable it");
}

int sd_tune_set_plan_table(const char* rows, sd_unet* u, int* n_plans) {
  return guarded([&] {
    require_tune_env();
    require_idle(u, "sd_tune_set_plan_table");
    const int n = conv_plan_table_set(rows);
    if (n_plans) *n_plans = n;
    if (u) u->impl->drop_graphs();   // the captured launches bake the old plans in
  });
}
int sd_unet_num_residuals(const sd_unet* u) {
  const UNet* p = u ? dynamic_cast<const UNet*>(u->impl.get()) : nullptr;
  return p ? p->num_residuals() : 0;
}
size_t sd_unet_device_bytes(const sd_unet* u) { return u ? u->impl->device_bytes() : 0; }
size_t sd_unet_arena_used_bytes(const sd_unet* u) { return u ? u->impl->arena_used_bytes() : 0; }
int sd_unet_palette_info(const sd_unet* u, int* n_palettized, int* n_streamed, size_t* stream_bytes) {
  return guarded([&] {
    SD_REQUIRE(u && n_palettized && n_streamed && stream_bytes, kInvalidArgument, "NULL argument");
    u->impl->palette_info(n_palettized, n_streamed, stream_bytes);
  });
}

int sd_unet_w8a8_info(const sd_unet* u, int* n_marked, int* n_applied, size_t* bytes) {
  return guarded([&] {
    SD_REQUIRE(u && n_marked && n_applied && bytes, kInvalidArgument, "NULL argument");
    u->impl->w8a8_info(n_marked, n_applied, bytes);
  });
}
int sd_unet_w8a8_layer(const sd_unet* u, int index, char* name, int name_bytes) {
  int n = 0;
  const int st = guarded([&] {
    SD_REQUIRE(u, kInvalidArgument, "NULL handle");
    const std::vector<std::string>& names = u->impl->w8a8_applied();
    n = (int)names.size();
    SD_REQUIRE(index < n && (index < 0 || (name && name_bytes > 1)), kInvalidArgument, "W8A8 layer %d of %d", index, n);
    if (index >= 0) std::snprintf(name, (size_t)name_bytes, "%s", names[(size_t)index].c_str());
  });
  return st != kOk ? st : n;
}
int sd_unet_einsum_info(const sd_unet* u, int* n_marked, int* n_applied) {
  return guarded([&] {
    SD_REQUIRE(u && n_marked && n_applied, kInvalidArgument, "NULL argument");
    u->impl->einsum_info(n_marked, n_applied);
  });
}
int sd_unet_einsum_layer(const sd_unet* u, int index, char* name, int name_bytes) {
  int n = 0;
  const int st = guarded([&] {
    SD_REQUIRE(u, kInvalidArgument, "NULL handle");
    const std::vector<std::string>& names = u->impl->einsum_applied();
    n = (int)names.size();
    SD_REQUIRE(index < n && (index < 0 || (name && name_bytes > 1)), kInvalidArgument, "einsum layer %d of %d", index, n);
    if (index >= 0) std::snprintf(name, (size_t)name_bytes, "%s", names[(size_t)index].c_str());
  });
  return st != kOk ? st : n;
}
int sd_unet_activation_ranges(sd_unet* u, int index, char* name, int name_bytes, float* absmax) {
  int n = 0;
  const int st = guarded([&] {
    SD_REQUIRE(u, kInvalidArgument, "NULL handle");
    SD_REQUIRE(index < 0 || (name && name_bytes > 1 && absmax), kInvalidArgument, "NULL argument");
    require_idle(u, "sd_unet_activation_ranges");
    std::string s;
    float v = 0.f;
    n = u->impl->activation_range(index, &s, &v);
    SD_REQUIRE(index < n, kInvalidArgument, "activation range %d of %d", index, n);
    if (index >= 0) {
      std::snprintf(name, (size_t)name_bytes, "%s", s.c_str());
      *absmax = v;
    }
  });
  return st != kOk ? st : n;
}

int sd_unet_forward(sd_unet* u, const sd_unet_io* io) {
  return guarded([&] {
    SD_REQUIRE(u && io, kInvalidArgument, "NULL argument");
    require_idle(u, "sd_unet_forward");
    unet_of(u, "handle is a VAE decoder: use sd_vae_decode").forward(*io);
  });
}
int sd_unet_time_forward(sd_unet* u, int warmup, int iters, float* ms_per_iter) {
  return guarded([&] {
    SD_REQUIRE(u && ms_per_iter, kInvalidArgument, "NULL argument");
    require_idle(u, "sd_unet_time_forward");
    *ms_per_iter = u->impl->time_forward(warmup, iters);
  });
}
int sd_unet_denoise_loop_progress(sd_unet* u, const sd_unet_io* io, float* latents, int n_images, int n_steps,
                                  const float* timesteps, const float* coef, const float* sample_scale, int history,
                                  float guidance_scale, float* history_io, float* ms_per_step, const float* pred, int every,
                                  sd_progress_fn fn, void* user, int* steps_done) {
  return guarded([&] {
    SD_REQUIRE(every >= 1, kInvalidArgument, "denoise_loop: every = %d: the handler runs after the steps i with i %% every == 0, every >= 1",
               every);
    SD_REQUIRE(!fn || steps_done, kInvalidArgument, "denoise_loop: a progress handler may stop the loop, so steps_done must not be NULL");
    SD_REQUIRE(u && io && latents && timesteps && coef, kInvalidArgument, "NULL argument");
    require_idle(u, "sd_unet_denoise_loop_progress");
    unet_of(u, "denoise_loop needs a UNet handle")
        .denoise_loop(*io, latents, n_images, n_steps, timesteps, coef, sample_scale, history, guidance_scale, history_io, ms_per_step,
                      pred, every, fn, user, steps_done);
  });
}
int sd_unet_denoise_loop(sd_unet* u, const sd_unet_io* io, float* latents, int n_images, int n_steps,
                         const float* timesteps, const float* coef, const float* sample_scale, int history,
                         float guidance_scale, float* history_io, float* ms_per_step) {
  return sd_unet_denoise_loop_progress(u, io, latents, n_images, n_steps, timesteps, coef, sample_scale, history, guidance_scale,
                                       history_io, ms_per_step, nullptr, 1, nullptr, nullptr, nullptr);
}

int sd_tune_set_candidate(int tile, int staging, int splitk) {
  return guarded([&] {
    require_tune_env();
    SD_REQUIRE(tile >= 0 && tile <= 9 && staging >= 0 && staging <= 8 && splitk >= 0 && splitk <= 64, kInvalidArgument,
               "tune candidate (tile %d, staging %d, splitk %d)", tile, staging, splitk);
    conv_tune_set_candidate(tile, staging, splitk);
  });
}

int sd_unet_profile(sd_unet* u, int iters, int cap, float* ms, double* flop, char* labels, int label_bytes, int* n_ops) {
  return guarded([&] {
    SD_REQUIRE(u && n_ops && cap >= 0 && (cap == 0 || (ms && flop && labels && label_bytes > 1)), kInvalidArgument,
               "NULL argument");
    require_idle(u, "sd_unet_profile");
    const std::vector<OpTime> t = u->impl->profile(iters);
    *n_ops = (int)t.size();
    for (int i = 0; i < (int)t.size() && i < cap; ++i) {
      ms[i] = t[i].ms;
      flop[i] = t[i].flop;
      std::snprintf(labels + (size_t)i * label_bytes, (size_t)label_bytes, "%s", t[i].label.c_str());
    }
  });
}

int sd_unet_attach_controlnets(sd_unet* u, sd_unet* const* controlnets, int n) {
  return guarded([&] {
    SD_REQUIRE(u && n >= 0 && (n == 0 || controlnets), kInvalidArgument, "NULL argument");
    require_idle(u, "sd_unet_attach_controlnets");
    UNet& unet = unet_of(u, "attach_controlnets needs a UNet handle");
    std::vector<UNet*> v;
    for (int i = 0; i < n; ++i) {
      SD_REQUIRE(controlnets[i], kInvalidArgument, "controlnets[%d] is NULL", i);
      v.push_back(dynamic_cast<UNet*>(controlnets[i]->impl.get()));   // null for a VAE handle: refused there as "not a ControlNet"
    }
    unet.attach_controlnets(v);
  });
}

int sd_controlnet_set_cond(sd_unet* cn, const void* controlnet_cond, int flags) {
  return guarded([&] {
    SD_REQUIRE(cn && controlnet_cond, kInvalidArgument, "NULL argument");
    unet_of(cn, "set_controlnet_cond needs a ControlNet handle").set_controlnet_cond(controlnet_cond, flags);
  });
}

int sd_vae_decoder_create(const sd_unet_config* cfg, const sd_weights* w, int device, sd_unet** out) {
  return guarded([&] { create_handle(cfg, w, device, out, 1); });
}
int sd_vae_encoder_create(const sd_unet_config* cfg, const sd_weights* w, int device, sd_unet** out) {
  return guarded([&] { create_handle(cfg, w, device, out, 2); });
}
int sd_vae_encode(sd_unet* vae, const void* x, sd_dtype x_dtype, float* moments, int flags) {
  return guarded([&] {
    SD_REQUIRE(vae && x && moments, kInvalidArgument, "NULL argument");
    vae_of(vae, 2).encode(x, x_dtype == SD_F32, moments, flags);
  });
}
int sd_vae_encode_latents(sd_unet* vae, const void* x, sd_dtype x_dtype, const float* eps, const float* noise, int n_images,
                          float scale_factor, float sa, float sb, float* latents, int flags) {
  return guarded([&] {
    SD_REQUIRE(vae && x && eps && noise && latents, kInvalidArgument, "NULL argument");
    SD_REQUIRE(n_images >= 1, kInvalidArgument, "encode_latents: n_images = %d", n_images);
    vae_of(vae, 2).encode_latents(x, x_dtype == SD_F32, eps, noise, n_images, scale_factor, sa, sb, latents, flags);
  });
}
int sd_vae_decode(sd_unet* vae, const void* z, sd_dtype z_dtype, float* image, int flags) {
  return guarded([&] {
    SD_REQUIRE(vae && z && image, kInvalidArgument, "NULL argument");
    vae_of(vae, 1).decode(z, z_dtype == SD_F32, image, flags);
  });
}

int sd_vae_decode_images(sd_unet* vae, const void* z, sd_dtype z_dtype, float* image, uint8_t* rgb8, sd_safety_checker* checker,
                         const sd_image_post* post, float adjustment, float* has_nsfw, float* concept_scores, int flags) {
  return guarded([&] {
    SD_REQUIRE(vae && z, kInvalidArgument, "NULL argument");
    vae_of(vae, 1).decode_images(z, z_dtype == SD_F32, image, rgb8, checker ? checker->impl.get() : nullptr, post, adjustment, has_nsfw,
                                 concept_scores, flags);
  });
}

namespace {
// MT19937 as numpy's legacy RandomState and torch's CPU generator both use it (init_genrand + genrand_int32)
struct Mt19937 {
  uint32_t key[624];
  int pos = 624;
  explicit Mt19937(uint32_t seed) {
    uint32_t s = seed;
    for (uint32_t i = 0; i < 624; ++i) {
      key[i] = s;
      s = 1812433253u * (s ^ (s >> 30)) + i + 1;
    }
  }
  uint32_t next_u32() {
    if (pos == 624) {
      for (int i = 0; i < 624; ++i) {
        const uint32_t y = (key[i] & 0x80000000u) | (key[(i + 1) % 624] & 0x7fffffffu);
        key[i] = key[(i + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
      }
      pos = 0;
    }
    uint32_t y = key[pos++];
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
  }
};
}  // namespace

// numpy legacy RandomState: MT19937 + 53-bit doubles + Marsaglia polar method
// (NumPyRandomSource.swift:28-102; golden: StableDiffusionTests.swift:52-62)
int sd_numpy_randn(uint32_t seed, double* out, size_t n) {
  return guarded([&] {
    SD_REQUIRE(out || n == 0, kInvalidArgument, "NULL output");
    Mt19937 mt(seed);
    auto next_double = [&]() -> double {
      const uint32_t a = mt.next_u32() >> 5, b = mt.next_u32() >> 6;
      return ((double)a * 67108864.0 + (double)b) / 9007199254740992.0;
    };
    bool has_cached = false;
    double cached = 0.0;
    for (size_t i = 0; i < n; ++i) {
      if (has_cached) {
        out[i] = cached;
        has_cached = false;
        continue;
      }
      double x1, x2, r2;
      do {
        x1 = 2.0 * next_double() - 1.0;
        x2 = 2.0 * next_double() - 1.0;
        r2 = x1 * x1 + x2 * x2;
      } while (r2 >= 1.0 || r2 == 0.0);
      const double f = std::sqrt(-2.0 * std::log(r2) / r2);
      cached = f * x1;
      has_cached = true;
      out[i] = f * x2;
    }
  });
}

// torch.manual_seed(seed); torch.randn(n) on the CPU (TorchRandomSource.swift:116-150): 24-bit uniforms, Box-Muller
// over blocks of 16, ragged tail from 53-bit doubles over the last 16; n < 16 scalar Box-Muller with the sine cached
int sd_torch_randn(uint32_t seed, double* out, size_t n) {
  return guarded([&] {
    SD_REQUIRE(out || n == 0, kInvalidArgument, "NULL output");
    Mt19937 mt(seed);
    const double two_pi = 6.283185307179586476925286766559;
    auto next_double53 = [&]() -> double {
      const uint64_t hi = mt.next_u32(), lo = mt.next_u32();
      return (double)(((hi << 32) | lo) & 9007199254740991ull) * (1.0 / 9007199254740992.0);
    };
    if (n < 16) {
      bool has_cached = false;
      double cached = 0.0;
      for (size_t i = 0; i < n; ++i) {
        if (has_cached) {
          out[i] = cached;
          has_cached = false;
          continue;
        }
        const double u1 = next_double53();
        const double u2 = 1.0 - next_double53();
        const double radius = std::sqrt(-2.0 * std::log(u2));
        cached = radius * std::sin(two_pi * u1);
        has_cached = true;
        out[i] = radius * std::cos(two_pi * u1);
      }
      return;
    }
    for (size_t i = 0; i < n; ++i) out[i] = (double)(mt.next_u32() & 16777215u) * (1.0 / 16777216.0);
    auto fill16 = [&](size_t i) {
      for (size_t j = 0; j < 8; ++j) {
        const double u1 = 1.0 - out[i + j], u2 = out[i + j + 8];
        const double radius = std::sqrt(-2.0 * std::log(u1)), theta = two_pi * u2;
        out[i + j] = radius * std::cos(theta);
        out[i + j + 8] = radius * std::sin(theta);
      }
    };
    for (size_t i = 0; i + 15 < n; i += 16) fill16(i);
    if (n % 16) {
      // ragged tail: the last 16 values are redrawn.  torch draws them like the rest (24-bit floats); the Swift
      // restatement draws 53-bit doubles here (TorchRandomSource.swift:135-137).  Latent counts on the path are
      // multiples of 16, where the two agree; torch itself is followed for the tail (tests pin it against torch).
      for (size_t i = n - 16; i < n; ++i) out[i] = (double)(mt.next_u32() & 16777215u) * (1.0 / 16777216.0);
      fill16(n - 16);
    }
  });
}

// torch.randn on a CUDA device (NvRandomSource.swift:25-80): Philox4x32-10, counter (offset, 0, i, 0), key = seed,
// Box-Muller on the first two output words of element i
int sd_philox_randn(uint64_t seed, uint32_t offset, double* out, size_t n) {
  return guarded([&] {
    SD_REQUIRE(out || n == 0, kInvalidArgument, "NULL output");
    const double pi = 3.14159265358979323846;
    for (size_t i = 0; i < n; ++i) {
      uint32_t c0 = offset, c1 = 0, c2 = (uint32_t)i, c3 = 0;
      uint32_t k0 = (uint32_t)(seed & 0xffffffffu), k1 = (uint32_t)(seed >> 32);
      for (int r = 0; r < 10; ++r) {
        const uint64_t v1 = (uint64_t)c0 * 0xD2511F53u, v2 = (uint64_t)c2 * 0xCD9E8D57u;
        const uint32_t n0 = (uint32_t)(v2 >> 32) ^ c1 ^ k0, n1 = (uint32_t)v2;
        const uint32_t n2 = (uint32_t)(v1 >> 32) ^ c3 ^ k1, n3 = (uint32_t)v1;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        if (r < 9) {
          k0 += 0x9E3779B9u;
          k1 += 0xBB67AE85u;
        }
      }
      const double u = (double)c0 / 4294967296.0 + (1.0 / 8589934592.0);
      const double v = (double)c1 * (pi / 2147483648.0) + (pi / 4294967296.0);
      out[i] = std::sqrt(-2.0 * std::log(u)) * std::sin(v);
    }
  });
}

int sd_calibrate(int device, float* out9) {
  return guarded([&] {
    SD_REQUIRE(out9, kInvalidArgument, "NULL argument");
    require_device();
    run_calibration(device, out9);
  });
}

int sd_selftest_mfma(void) {
  int rc = 0;
  int st = guarded([&] {
    require_device();
    rc = selftest_mfma();
  });
  return st != kOk ? st : rc;
}

}  // extern "C"
