#include "weights.h"

#include "weight_prep.h"

#include <algorithm>
#include <cstdarg>
#include <cstring>
#include <fstream>

namespace sd {

thread_local std::string g_last_error;

void fail(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  throw Error(code, buf);
}

// ---- Arena: chunked bump allocator (chunks of >= 256 MiB; HBM is 288 GB, nothing is recycled) ----
Arena::~Arena() {
  for (void* p : chunks_) (void)hipFree(p);
}

void* Arena::alloc(size_t bytes) {
  bytes = align_up(bytes ? bytes : 1, 256);
  if (chunks_.empty() || cur_ + bytes > cap_) {
    size_t chunk = std::max<size_t>(bytes, (size_t)256 << 20);
    void* p = nullptr;
    SD_HIP(hipMalloc(&p, chunk));
    SD_HIP(hipMemset(p, 0, chunk));
    SD_HIP(hipDeviceSynchronize());   // the memset runs on the null stream; handles use their own
    chunks_.push_back(p);
    sizes_.push_back(chunk);
    cap_ = chunk;
    cur_ = 0;
    total_ += chunk;
  }
  char* p = reinterpret_cast<char*>(chunks_.back()) + cur_;
  cur_ += bytes;
  used_ += bytes;
  return p;
}

// ---- WeightStore ------------------------------------------------------------------------------
static inline float half_bits_to_float(uint16_t h) {
  _Float16 v;
  std::memcpy(&v, &h, 2);
  return (float)v;
}
static inline float bf16_bits_to_float(uint16_t h) {
  uint32_t u = (uint32_t)h << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

void WeightStore::add(const std::string& name, const void* data, int dtype, const int64_t* shape, int ndim) {
  SD_REQUIRE(data && ndim >= 0 && ndim <= 8, kInvalidArgument, "weights.add(%s): bad arguments", name.c_str());
  HostTensor t;
  t.shape.assign(shape, shape + ndim);
  size_t n = t.numel();
  t.data.resize(n);
  if (dtype == 1) {
    std::memcpy(t.data.data(), data, n * 4);
  } else if (dtype == 0) {
    const uint16_t* s = reinterpret_cast<const uint16_t*>(data);
    for (size_t i = 0; i < n; ++i) t.data[i] = half_bits_to_float(s[i]);
  } else if (dtype == 2) {
    const uint16_t* s = reinterpret_cast<const uint16_t*>(data);
    for (size_t i = 0; i < n; ++i) t.data[i] = bf16_bits_to_float(s[i]);
  } else {
    fail(kInvalidArgument, "weights.add(%s): unknown dtype %d", name.c_str(), dtype);
  }
  map_[name] = std::move(t);
  pal_.erase(name);   // plain values replace whatever palette the name had
  i8_.erase(name);    // ... and whatever W8A8 mark
}

void WeightStore::set_values(const std::string& name, const float* values, size_t n) {
  auto it = map_.find(name);
  if (it == map_.end()) fail(kNotFound, "set_values: the store has no tensor '%s'", name.c_str());
  SD_REQUIRE(n == it->second.numel(), kInvalidArgument, "set_values(%s): %zu values for a tensor of %zu elements", name.c_str(), n, it->second.numel());
  std::copy(values, values + n, it->second.data.begin());
  pal_.erase(name);
  i8_.erase(name);
}

// ---- W8A8 marks ------------------------------------------------------------------------------
const W8A8Mark* WeightStore::w8a8(const std::string& name) const {
  auto it = i8_.find(name);
  return it == i8_.end() ? nullptr : &it->second;
}

double WeightStore::quantize_w8a8(const std::string& name, float act_absmax) {
  auto it = map_.find(name);
  if (it == map_.end()) fail(kNotFound, "quantize_w8a8: the store has no tensor '%s'", name.c_str());
  const HostTensor& t = it->second;
  SD_REQUIRE(t.shape.size() == 4 && t.shape[2] == t.shape[3] && t.numel() > 0, kInvalidArgument,
             "quantize_w8a8(%s): not a conv weight (Cout, Cin, k, k)", name.c_str());
  SD_REQUIRE(!pal_.count(name), kInvalidArgument, "quantize_w8a8(%s): the tensor carries a palette; a tensor is palettized or W8A8, not both",
             name.c_str());
  SD_REQUIRE(w8a8_absmax_ok(act_absmax), kInvalidArgument, "quantize_w8a8(%s): act_absmax = %g, not a positive finite number", name.c_str(),
             (double)act_absmax);
  W8A8Mark m;
  m.act_absmax = act_absmax;
  m.q.resize(t.numel());
  m.w_scale.resize((size_t)t.shape[0]);
  const double err = w8a8_quantize_weight(t.data.data(), (int)t.shape[0], t.numel() / (size_t)t.shape[0], m.q.data(), m.w_scale.data());
  i8_[name] = std::move(m);
  return err;
}

// ---- Einsum marks (activation_quantization.py:205-215, unet.py:45-59) -------------------------
const EinsumMark* WeightStore::einsum(const std::string& name) const {
  auto it = einsum_.find(name);
  return it == einsum_.end() ? nullptr : &it->second;
}

void WeightStore::quantize_einsum(const std::string& name, float q_absmax, float k_absmax, float v_absmax) {
  static const std::string suffix = ".einsum";
  const bool named = name.size() > suffix.size() && name.compare(name.size() - suffix.size(), suffix.size(), suffix) == 0;
  const std::string probe = named ? name.substr(0, name.size() - suffix.size()) + ".to_q.weight" : std::string();
  if (!named || !has(probe))
    fail(kNotFound, "quantize_einsum: '%s' names no attention of the store (<prefix>.einsum beside <prefix>.to_q.weight)", name.c_str());
  SD_REQUIRE(w8a8_absmax_ok(q_absmax) && w8a8_absmax_ok(k_absmax) && w8a8_absmax_ok(v_absmax), kInvalidArgument,
             "quantize_einsum(%s): ranges %g, %g, %g: each must be a positive finite number", name.c_str(), (double)q_absmax, (double)k_absmax,
             (double)v_absmax);
  einsum_[name] = EinsumMark{q_absmax, k_absmax, v_absmax};
}

// ---- palettes --------------------------------------------------------------------------------
static inline uint16_t float_to_half_bits(float f) {
  const _Float16 v = (_Float16)f;
  uint16_t h;
  std::memcpy(&h, &v, 2);
  return h;
}

const Palette* WeightStore::palette(const std::string& name) const {
  auto it = pal_.find(name);
  return it == pal_.end() ? nullptr : &it->second;
}

namespace {
// Optimal partition of n sorted weighted points into k contiguous ranges (least sum of squared distances to the range means).
// dp[m][j] = min_i dp[m-1][i-1] + cost(i, j); the arg min is monotone in j, so a layer is filled by divide and conquer:
// O(k n log n) cost evaluations, each O(1) from float64 prefix sums of count, count * v, count * v^2.  No random start, no
// iteration: the result is the optimum and the same on every run.
struct RangeCost {
  std::vector<double> s0, s1, s2;   // prefix sums, entry i = points [0, i)
  double operator()(int i, int j) const {   // points [i, j], inclusive
    const double c = s0[j + 1] - s0[i], a = s1[j + 1] - s1[i], q = s2[j + 1] - s2[i];
    const double e = q - a * a / c;
    return e > 0.0 ? e : 0.0;
  }
  double mean(int i, int j) const { return (s1[j + 1] - s1[i]) / (s0[j + 1] - s0[i]); }
};

void dp_layer(const RangeCost& cost, const std::vector<double>& prev, std::vector<double>& cur, std::vector<int32_t>& arg, int m, int jlo,
              int jhi, int ilo, int ihi) {
  if (jlo > jhi) return;
  const int j = (jlo + jhi) / 2;
  double best = 1e300;
  int bi = -1;
  // range m (0-based) starts at i >= m (m ranges of at least one point in front of it) and ends at j
  for (int i = std::max(ilo, m), hi = std::min(ihi, j); i <= hi; ++i) {
    const double v = prev[i - 1] + cost(i, j);
    if (v < best) {
      best = v;
      bi = i;
    }
  }
  cur[j] = best;
  arg[j] = bi;
  dp_layer(cost, prev, cur, arg, m, jlo, j - 1, ilo, bi);
  dp_layer(cost, prev, cur, arg, m, j + 1, jhi, bi, ihi);
}
}  // namespace

double WeightStore::palettize(const std::string& name, int nbits) {
  SD_REQUIRE(palette_bits_ok(nbits), kInvalidArgument, "palettize(%s): nbits = %d, not one of 1, 2, 4, 6, 8", name.c_str(), nbits);
  auto it = map_.find(name);
  if (it == map_.end()) fail(kNotFound, "palettize: the store has no tensor '%s'", name.c_str());
  SD_REQUIRE(!i8_.count(name), kInvalidArgument, "palettize(%s): the tensor carries a W8A8 mark; a tensor is palettized or W8A8, not both", name.c_str());
  HostTensor& t = it->second;
  const size_t n_el = t.numel();
  const int k = 1 << nbits;
  // histogram of the fp16-rounded values (the reference clusters weight.astype(float16)); -0 counts as +0
  std::vector<uint16_t> hb(n_el);
  std::vector<uint32_t> count(65536, 0);
  for (size_t e = 0; e < n_el; ++e) {
    uint16_t h = float_to_half_bits(t.data[e]);
    SD_REQUIRE((h & 0x7c00) != 0x7c00, kInvalidArgument, "palettize(%s): element %zu is not finite in fp16", name.c_str(), e);
    if (h == 0x8000) h = 0;
    hb[e] = h;
    ++count[h];
  }
  // distinct values in ascending order: negative patterns downwards, then the non-negative ones upwards
  std::vector<uint16_t> vals;
  for (int h = 0xfbff; h > 0x8000; --h)
    if (count[h]) vals.push_back((uint16_t)h);
  for (int h = 0; h < 0x7c00; ++h)
    if (count[h]) vals.push_back((uint16_t)h);
  const int n = (int)vals.size();
  Palette p;
  p.nbits = nbits;
  p.lut.assign(k, 0);
  std::vector<int> cluster_of(65536, 0);
  if (n <= k) {   // every distinct value gets its own entry (the last one repeated): exact
    for (int i = 0; i < k; ++i) p.lut[i] = n ? vals[std::min(i, n - 1)] : 0;
    for (int i = 0; i < n; ++i) cluster_of[vals[i]] = i;
  } else {
    RangeCost cost;
    cost.s0.assign(n + 1, 0.0);
    cost.s1.assign(n + 1, 0.0);
    cost.s2.assign(n + 1, 0.0);
    for (int i = 0; i < n; ++i) {
      const double v = (double)half_bits_to_float(vals[i]), c = (double)count[vals[i]];
      cost.s0[i + 1] = cost.s0[i] + c;
      cost.s1[i + 1] = cost.s1[i] + c * v;
      cost.s2[i + 1] = cost.s2[i] + c * v * v;
    }
    std::vector<double> prev(n), cur(n);
    std::vector<std::vector<int32_t>> arg(k, std::vector<int32_t>(n, 0));
    for (int j = 0; j < n; ++j) prev[j] = cost(0, j);
    for (int m = 1; m < k; ++m) {
      std::fill(cur.begin(), cur.end(), 1e300);
      dp_layer(cost, prev, cur, arg[m], m, m, n - 1, m, n - 1);
      prev.swap(cur);
    }
    int j = n - 1;
    for (int m = k - 1; m >= 0; --m) {   // walk the range starts back from the last point
      const int i = m == 0 ? 0 : arg[m][j];
      p.lut[m] = float_to_half_bits((float)cost.mean(i, j));
      for (int q = i; q <= j; ++q) cluster_of[vals[q]] = m;
      j = i - 1;
    }
  }
  p.indices.resize(n_el);
  double err = 0.0;
  for (size_t e = 0; e < n_el; ++e) {
    const int c = cluster_of[hb[e]];
    const float v = half_bits_to_float(p.lut[c]);
    const double dlt = (double)half_bits_to_float(hb[e]) - (double)v;
    err += dlt * dlt;
    p.indices[e] = (uint8_t)c;
    t.data[e] = v;
  }
  pal_[name] = std::move(p);
  return err;
}

void WeightStore::add_palettized(const std::string& name, const void* lut_f16, int nbits, const uint8_t* indices, const int64_t* shape,
                                 int ndim) {
  SD_REQUIRE(palette_bits_ok(nbits), kInvalidArgument, "add_palettized(%s): nbits = %d, not one of 1, 2, 4, 6, 8", name.c_str(), nbits);
  SD_REQUIRE(lut_f16 && indices && ndim >= 0 && ndim <= 8, kInvalidArgument, "add_palettized(%s): bad arguments", name.c_str());
  Palette p;
  p.nbits = nbits;
  const uint16_t* l = reinterpret_cast<const uint16_t*>(lut_f16);
  p.lut.assign(l, l + (1 << nbits));
  HostTensor t;
  t.shape.assign(shape, shape + ndim);
  const size_t n_el = t.numel();
  for (size_t e = 0; e < n_el; ++e)
    SD_REQUIRE(indices[e] < (1u << nbits), kInvalidArgument, "add_palettized(%s): index %u at element %zu, the palette has %d entries",
               name.c_str(), (unsigned)indices[e], e, 1 << nbits);
  p.indices.assign(indices, indices + n_el);
  t.data.resize(n_el);
  for (size_t e = 0; e < n_el; ++e) t.data[e] = half_bits_to_float(p.lut[indices[e]]);
  map_[name] = std::move(t);
  pal_[name] = std::move(p);
  i8_.erase(name);   // new values: a W8A8 mark of the old ones is gone
}

// Public SD 1.x / 2.x VAE checkpoints keep the deprecated attention names (query / key / value /
// proj_attn) that diffusers renames at load time; look those up when the current name is absent.
const HostTensor* WeightStore::find(const std::string& name) const {
  auto it = map_.find(name);
  if (it != map_.end()) return &it->second;
  static const char* const kAlias[][2] = {
      {".to_q.", ".query."}, {".to_k.", ".key."}, {".to_v.", ".value."}, {".to_out.0.", ".proj_attn."}};
  for (const auto& a : kAlias) {
    const size_t pos = name.find(a[0]);
    if (pos == std::string::npos) continue;
    std::string old = name;
    old.replace(pos, std::strlen(a[0]), a[1]);
    it = map_.find(old);
    if (it != map_.end()) return &it->second;
  }
  return nullptr;
}

const HostTensor& WeightStore::get(const std::string& name) const {
  const HostTensor* t = find(name);
  if (!t) fail(kNotFound, "checkpoint is missing tensor '%s'", name.c_str());
  return *t;
}

// Minimal safetensors reader: 8-byte LE header length, JSON header
//   {"name": {"dtype": "F16", "shape": [..], "data_offsets": [b, e]}, ..., "__metadata__": {...}}
// followed by the raw little-endian tensor bytes.  The header grammar is a flat two-level object,
// so a small hand-rolled scanner is enough (no JSON dependency).
namespace {
struct Scanner {
  const std::string& s;
  size_t i = 0;
  explicit Scanner(const std::string& str) : s(str) {}
  void ws() {
    while (i < s.size() && (s[i] == ' ' || s[i] == '\n' || s[i] == '\t' || s[i] == '\r')) ++i;
  }
  bool eat(char c) {
    ws();
    if (i < s.size() && s[i] == c) {
      ++i;
      return true;
    }
    return false;
  }
  void expect(char c) {
    if (!eat(c)) fail(kInvalidArgument, "safetensors header: expected '%c' at byte %zu", c, i);
  }
  std::string str() {
    expect('"');
    std::string out;
    while (i < s.size() && s[i] != '"') {
      if (s[i] == '\\' && i + 1 < s.size()) ++i;
      out.push_back(s[i++]);
    }
    expect('"');
    return out;
  }
  int64_t num() {
    ws();
    size_t j = i;
    while (j < s.size() && (isdigit((unsigned char)s[j]) || s[j] == '-')) ++j;
    if (j == i || j - i > 18) fail(kInvalidArgument, "safetensors header: expected a number at byte %zu", i);
    int64_t v = 0;
    try {
      v = std::stoll(s.substr(i, j - i));
    } catch (const std::exception&) {
      fail(kInvalidArgument, "safetensors header: bad number at byte %zu", i);
    }
    i = j;
    return v;
  }
  void skip_value() {   // for __metadata__
    ws();
    if (i >= s.size()) fail(kInvalidArgument, "safetensors header: truncated");
    if (s[i] == '{') {
      int depth = 0;
      bool in_str = false;
      for (; i < s.size(); ++i) {
        if (in_str) {
          if (s[i] == '\\') ++i;
          else if (s[i] == '"') in_str = false;
        } else if (s[i] == '"') in_str = true;
        else if (s[i] == '{') ++depth;
        else if (s[i] == '}' && --depth == 0) {
          ++i;
          return;
        }
      }
    } else if (s[i] == '"') {
      str();
    } else {
      while (i < s.size() && s[i] != ',' && s[i] != '}') ++i;
    }
  }
};
}  // namespace

void WeightStore::load_safetensors(const std::string& path, const std::string& prefix) {
  std::ifstream f(path, std::ios::binary);
  if (!f) fail(kNotFound, "%s not found", path.c_str());
  uint64_t hlen = 0;
  f.read(reinterpret_cast<char*>(&hlen), 8);
  SD_REQUIRE(f && hlen > 0 && hlen < ((uint64_t)1 << 30), kInvalidArgument, "%s: bad safetensors header", path.c_str());
  f.seekg(0, std::ios::end);
  const uint64_t file_size = (uint64_t)f.tellg();
  SD_REQUIRE(8 + hlen <= file_size, kInvalidArgument, "%s: safetensors header (%llu bytes) exceeds the file", path.c_str(),
             (unsigned long long)hlen);
  f.seekg(8);
  std::string header(hlen, '\0');
  f.read(&header[0], (std::streamsize)hlen);
  SD_REQUIRE((bool)f && (uint64_t)f.gcount() == hlen, kInvalidArgument, "%s: truncated safetensors header", path.c_str());
  const uint64_t data_start = 8 + hlen;
  Scanner sc(header);
  sc.expect('{');
  std::vector<char> raw;
  while (true) {
    if (sc.eat('}')) break;
    std::string key = sc.str();
    sc.expect(':');
    if (key == "__metadata__") {
      sc.skip_value();
      sc.eat(',');
      continue;
    }
    std::string dtype;
    std::vector<int64_t> shape;
    int64_t b = 0, e = 0;
    sc.expect('{');
    while (true) {
      std::string field = sc.str();
      sc.expect(':');
      if (field == "dtype") {
        dtype = sc.str();
      } else if (field == "shape") {
        sc.expect('[');
        while (!sc.eat(']')) {
          shape.push_back(sc.num());
          sc.eat(',');
        }
      } else if (field == "data_offsets") {
        sc.expect('[');
        b = sc.num();
        sc.expect(',');
        e = sc.num();
        sc.expect(']');
      } else {
        sc.skip_value();
      }
      if (sc.eat('}')) break;
      sc.expect(',');
    }
    sc.eat(',');
    int dt = dtype == "F16" ? 0 : dtype == "F32" ? 1 : dtype == "BF16" ? 2 : -1;
    if (dt < 0) continue;   // integer buffers etc. are not part of the path
    // never trust the header: offsets inside the file, non-negative dims, byte count == numel * element size
    SD_REQUIRE(b >= 0 && e >= b && data_start + (uint64_t)e <= file_size, kInvalidArgument,
               "%s: tensor '%s' has data_offsets [%lld, %lld) outside the file", path.c_str(), key.c_str(), (long long)b,
               (long long)e);
    SD_REQUIRE(shape.size() <= 8, kInvalidArgument, "%s: tensor '%s' has %zu dims", path.c_str(), key.c_str(), shape.size());
    uint64_t numel = 1;
    for (int64_t dim : shape) {
      SD_REQUIRE(dim >= 0 && (dim == 0 || numel <= ((uint64_t)1 << 40) / (uint64_t)dim), kInvalidArgument,
                 "%s: tensor '%s' has a bad dimension %lld", path.c_str(), key.c_str(), (long long)dim);
      numel *= (uint64_t)dim;
    }
    SD_REQUIRE((uint64_t)(e - b) == numel * (dt == 1 ? 4u : 2u), kInvalidArgument,
               "%s: tensor '%s' stores %lld bytes but its shape needs %llu", path.c_str(), key.c_str(), (long long)(e - b),
               (unsigned long long)(numel * (dt == 1 ? 4u : 2u)));
    raw.resize((size_t)(e - b));
    f.seekg((std::streamoff)(data_start + (uint64_t)b));
    f.read(raw.data(), (std::streamsize)raw.size());
    SD_REQUIRE((bool)f, kInvalidArgument, "%s: truncated tensor '%s'", path.c_str(), key.c_str());
    std::string name = key;
    if (!prefix.empty() && name.compare(0, prefix.size(), prefix) == 0) name = name.substr(prefix.size());
    add(name, raw.data(), dt, shape.data(), (int)shape.size());
  }
}

}  // namespace sd
