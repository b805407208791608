// Host side of the score network (reference UNetModel, ncsnpp.py:71-263): builds the layer table from the flat config,
// prepares weights (layout + dtype), and enqueues the HIP kernels of one evaluation on a stream.
// No host synchronisation happens inside score().
#include "engine.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <thread>

namespace t2p {

static thread_local std::string g_last_error;
void set_last_error(const std::string& msg) { g_last_error = msg; }
const char* get_last_error() { return g_last_error.c_str(); }

int ensure_dynamic_lds(const void* kernel, int bytes) {
  static std::mutex mu;
  static std::map<std::pair<const void*, int>, int> done;     // (kernel, device) -> largest size set so far
  int dev = 0;
  T2P_HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  auto it = done.find({kernel, dev});
  if (it != done.end() && it->second >= bytes) return T2P_OK;
  T2P_HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  done[{kernel, dev}] = bytes;
  return T2P_OK;
}

// ---- development tap (t2p_debug_tap): the output of block number `g_tap_index` of the next evaluations, widened to fp32 ----
static int g_tap_index = -1;
static float* g_tap_dst = nullptr;
static long g_tap_cap = 0;
static long g_tap_shape[4] = {0, 0, 0, 0};     // C, H, W, stored in 16 bits
static int g_tap_counter = 0;
void debug_tap_set(int index, float* dst, long capacity) { g_tap_index = index; g_tap_dst = dst; g_tap_cap = capacity; }
void debug_tap_shape(long out[4]) { for (int i = 0; i < 4; ++i) out[i] = g_tap_shape[i]; }

// ---- per-layer timing (development / bench: t2p_profile_layers_*): HIP events on the launch stream at block boundaries ----
struct LayerRec { std::string label; hipEvent_t e0, e1; };
static bool g_layer_prof = false;
static std::vector<LayerRec> g_layer_recs;
static std::mutex g_layer_mu;      // the records are process-global (a measurement hook): engines on other threads append under the lock
void layer_profile_begin() {
  std::lock_guard<std::mutex> lk(g_layer_mu);
  for (LayerRec& r : g_layer_recs) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
  g_layer_recs.clear();
  g_layer_prof = true;
}
struct LayerScope {
  int idx = -1;
  hipStream_t s;
  LayerScope(const std::string& label, hipStream_t st) : s(st) {
    if (!g_layer_prof) return;
    LayerRec r; r.label = label;
    if (hipEventCreate(&r.e0) != hipSuccess || hipEventCreate(&r.e1) != hipSuccess) return;
    (void)hipEventRecord(r.e0, s);
    std::lock_guard<std::mutex> lk(g_layer_mu);
    idx = (int)g_layer_recs.size();
    g_layer_recs.push_back(r);
  }
  ~LayerScope() {
    if (idx < 0) return;
    std::lock_guard<std::mutex> lk(g_layer_mu);
    if (idx < (int)g_layer_recs.size()) (void)hipEventRecord(g_layer_recs[idx].e1, s);
  }
};
// CSV "label,ms" per record, in launch order
int layer_profile_end(std::string* out) {
  g_layer_prof = false;
  T2P_HIP_CHECK(hipDeviceSynchronize());
  std::lock_guard<std::mutex> lk(g_layer_mu);
  out->clear();
  for (LayerRec& r : g_layer_recs) {
    float ms = 0.f;
    T2P_HIP_CHECK(hipEventElapsedTime(&ms, r.e0, r.e1));
    char buf[64];
    std::snprintf(buf, sizeof buf, ",%.4f\n", ms);
    *out += r.label + buf;
    (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1);
  }
  g_layer_recs.clear();
  return T2P_OK;
}

// ------------------------------------------------------------------------------------------------
DevPool::~DevPool() {
  for (void* p : all_) (void)hipFree(p);
}
static inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
void* DevPool::get(size_t bytes) {
  bytes = round_up(std::max<size_t>(bytes, 256), 256);
  auto it = free_.find(bytes);
  if (it != free_.end()) {
    void* p = it->second;
    free_.erase(it);
    if (lease_depth_) leased_.insert(p);
    return p;
  }
  void* p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess) {
    set_last_error("hipMalloc of " + std::to_string(bytes) + " bytes failed");
    return nullptr;
  }
  size_of_[p] = bytes;
  all_.push_back(p);
  held_ += bytes;
  if (lease_depth_) leased_.insert(p);
  return p;
}
void DevPool::put(void* p) {
  if (!p) return;
  auto it = size_of_.find(p);
  if (it == size_of_.end()) return;
  leased_.erase(p);
  free_.emplace(it->second, p);
}
void DevPool::lease_begin() {
  if (lease_depth_++ == 0) leased_.clear();
}
int DevPool::lease_end() {
  if (--lease_depth_ > 0) return 0;
  lease_depth_ = 0;
  const int n = (int)leased_.size();
  for (void* p : leased_) {
    auto it = size_of_.find(p);
    if (it != size_of_.end()) free_.emplace(it->second, p);
  }
  leased_.clear();
  last_reclaimed_ = n;
  return n;
}
void* DevPool::persistent(size_t bytes) {
  bytes = round_up(std::max<size_t>(bytes, 256), 256);
  void* p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess) {
    set_last_error("hipMalloc of " + std::to_string(bytes) + " bytes failed");
    return nullptr;
  }
  all_.push_back(p);
  held_ += bytes;
  return p;
}

#define POOL_GET(var, type, bytes)                          \
  type var = (type)pool_.get(bytes);                        \
  if (!var) return T2P_ERR_HIP;

// ------------------------------------------------------------------------------------------------
static int gn_groups(int c) { return std::min(c / 4, 32); }  // layers.py:282

Engine::Engine(const t2p_model_config& cfg) : cfg_(cfg) {}
Engine::~Engine() {}

static void add(std::vector<ParamInfo>& v, const std::string& n, std::vector<int64_t> s) { v.push_back({n, std::move(s)}); }

static void res_params(std::vector<ParamInfo>& v, const Layer& l, int td) {
  const std::string& p = l.prefix;
  const int64_t ci = l.in_ch, co = l.out_ch;
  add(v, p + ".GroupNorm_0.weight", {ci}); add(v, p + ".GroupNorm_0.bias", {ci});
  add(v, p + ".Conv_0.weight", {co, ci, 3, 3}); add(v, p + ".Conv_0.bias", {co});
  add(v, p + ".Dense_0.weight", {co, td}); add(v, p + ".Dense_0.bias", {co});
  add(v, p + ".GroupNorm_1.weight", {co}); add(v, p + ".GroupNorm_1.bias", {co});
  add(v, p + ".Conv_1.weight", {co, co, 3, 3}); add(v, p + ".Conv_1.bias", {co});
  if (l.has_conv2) { add(v, p + ".Conv_2.weight", {co, ci, 1, 1}); add(v, p + ".Conv_2.bias", {co}); }
}
static void attn_params(std::vector<ParamInfo>& v, const Layer& l) {
  const int64_t c = l.in_ch;
  add(v, l.prefix + ".GroupNorm_0.weight", {c}); add(v, l.prefix + ".GroupNorm_0.bias", {c});
  for (int i = 0; i < 4; ++i) {
    add(v, l.prefix + ".NIN_" + std::to_string(i) + ".W", {c, c});
    add(v, l.prefix + ".NIN_" + std::to_string(i) + ".b", {c});
  }
}
static void st_params(std::vector<ParamInfo>& v, const Layer& l, int64_t ctx) {
  const std::string& p = l.prefix;
  const std::string t = p + ".transformer_blocks.0";
  const int64_t c = l.in_ch;
  add(v, p + ".norm.weight", {c}); add(v, p + ".norm.bias", {c});
  add(v, p + ".proj_in.weight", {c, c, 1, 1}); add(v, p + ".proj_in.bias", {c});
  add(v, t + ".attn1.to_q.weight", {c, c}); add(v, t + ".attn1.to_k.weight", {c, c});
  add(v, t + ".attn1.to_v.weight", {c, c}); add(v, t + ".attn1.to_out.0.weight", {c, c});
  add(v, t + ".attn1.to_out.0.bias", {c});
  add(v, t + ".ff.net.0.proj.weight", {8 * c, c}); add(v, t + ".ff.net.0.proj.bias", {8 * c});
  add(v, t + ".ff.net.2.weight", {c, 4 * c}); add(v, t + ".ff.net.2.bias", {c});
  add(v, t + ".attn2.to_q.weight", {c, c}); add(v, t + ".attn2.to_k.weight", {c, ctx});
  add(v, t + ".attn2.to_v.weight", {c, ctx}); add(v, t + ".attn2.to_out.0.weight", {c, c});
  add(v, t + ".attn2.to_out.0.bias", {c});
  for (int i = 1; i <= 3; ++i) {
    add(v, t + ".norm" + std::to_string(i) + ".weight", {c});
    add(v, t + ".norm" + std::to_string(i) + ".bias", {c});
  }
  add(v, p + ".proj_out.weight", {c, c, 1, 1}); add(v, p + ".proj_out.bias", {c});
}

int NetArch::build(const t2p_model_config& c) {
  T2P_REQUIRE(c.n_ch_mult >= 1 && c.n_ch_mult <= 8, "ch_mult length");
  T2P_REQUIRE(c.n_attn_resolutions >= 0 && c.n_attn_resolutions <= 8, "attn_resolutions length");
  T2P_REQUIRE(c.nf >= 8 && c.nf % 8 == 0, "nf must be a multiple of 8");
  T2P_REQUIRE(c.num_channels >= 1 && c.num_channels <= 8, "num_channels must be in [1, 8]");
  T2P_REQUIRE(c.max_res_num % (1 << (c.n_ch_mult - 1)) == 0, "max_res_num must be divisible by 2^(levels-1)");
  T2P_REQUIRE(c.n_heads >= 1 && c.context_dim >= 8 && c.context_dim % 8 == 0, "n_heads / context_dim");
  T2P_REQUIRE(c.num_scales >= 2 && c.sigma_min > 0 && c.sigma_max > c.sigma_min, "sigma schedule");
  T2P_REQUIRE(c.compute_dtype >= 0 && c.compute_dtype <= 2, "compute_dtype");
  nf = c.nf;
  temb_dim = 4 * nf;
  const int nres = c.n_ch_mult, nrb = c.num_res_blocks, L = c.max_res_num;
  auto in_attn = [&](int res) {
    for (int i = 0; i < c.n_attn_resolutions; ++i)
      if (c.attn_resolutions[i] == res) return true;
    return false;
  };
  auto mk = [&](int kind, const std::string& prefix, int ci, int co, int up, int down) {
    Layer l;
    l.kind = kind; l.prefix = prefix; l.in_ch = ci; l.out_ch = co; l.up = up; l.down = down;
    l.has_conv2 = (kind == 0) && (ci != co || up || down);
    if (kind == 0) { l.temb_off = temb_total; temb_total += co; }
    return l;
  };
  auto attn_pair = [&](Stage& st, const std::string& prefix, int idx0, int ch) -> int {
    T2P_REQUIRE(ch % 32 == 0 && ch % c.n_heads == 0 && (ch / c.n_heads) % 8 == 0,
                "attention levels need channels % 32 == 0 and head dim % 8 == 0");
    st.layers.push_back(mk(1, prefix + "." + std::to_string(idx0), ch, ch, 0, 0));
    st.layers.push_back(mk(2, prefix + "." + std::to_string(idx0 + 1), ch, ch, 0, 0));
    return T2P_OK;
  };
  std::vector<int> skip_ch{nf};
  int in_ch = nf;
  for (int lvl = 0; lvl < nres; ++lvl) {
    const int res = L >> lvl;
    for (int b = 0; b < nrb; ++b) {
      const int out_ch = nf * c.ch_mult[lvl];
      const std::string prefix = "input_blocks." + std::to_string(input_stages.size());
      Stage st;
      st.layers.push_back(mk(0, prefix + ".0", in_ch, out_ch, 0, 0));
      in_ch = out_ch;
      if (in_attn(res)) T2P_TRY(attn_pair(st, prefix, 1, in_ch));
      input_stages.push_back(std::move(st));
      skip_ch.push_back(in_ch);
    }
    if (lvl != nres - 1) {
      const std::string prefix = "input_blocks." + std::to_string(input_stages.size());
      Stage st;
      st.layers.push_back(mk(0, prefix + ".0", in_ch, in_ch, 0, 1));
      input_stages.push_back(std::move(st));
      skip_ch.push_back(in_ch);
    }
  }
  const int mid = skip_ch.back();
  mid_stage.layers.push_back(mk(0, "mid_blocks.0", mid, mid, 0, 0));
  T2P_TRY(attn_pair(mid_stage, "mid_blocks", 1, mid));
  mid_stage.layers.push_back(mk(0, "mid_blocks.3", mid, mid, 0, 0));
  in_ch = mid;
  for (int lvl = nres - 1; lvl >= 0; --lvl) {
    const int res = L >> lvl;
    for (int b = 0; b <= nrb; ++b) {
      const int out_ch = nf * c.ch_mult[lvl];
      const std::string prefix = "out_blocks." + std::to_string(out_stages.size());
      Stage st;
      st.skip_ch = skip_ch.back();
      skip_ch.pop_back();
      st.layers.push_back(mk(0, prefix + ".0", in_ch + st.skip_ch, out_ch, 0, 0));
      in_ch = out_ch;
      if (in_attn(res)) T2P_TRY(attn_pair(st, prefix, 1, in_ch));
      if (lvl != 0 && b == nrb)
        st.layers.push_back(mk(0, prefix + "." + std::to_string(st.layers.size()), in_ch, in_ch, 1, 0));
      out_stages.push_back(std::move(st));
    }
  }
  T2P_REQUIRE(skip_ch.empty(), "skip stack not consumed");
  final_ch = in_ch;

  // parameter table in reference parameters() order
  const int64_t td = temb_dim, ch = c.num_channels;
  add(params, "pre_blocks.0.weight", {td, nf}); add(params, "pre_blocks.0.bias", {td});
  add(params, "pre_blocks.1.weight", {td, td}); add(params, "pre_blocks.1.bias", {td});
  add(params, "pre_conv.weight", {nf, ch, 3, 3}); add(params, "pre_conv.bias", {nf});
  auto walk = [&](Stage& st) {
    for (Layer& l : st.layers) {
      if (l.kind == 0) res_params(params, l, temb_dim);
      else if (l.kind == 1) attn_params(params, l);
      else st_params(params, l, c.context_dim);
    }
  };
  for (Stage& st : input_stages) walk(st);
  walk(mid_stage);
  for (Stage& st : out_stages) walk(st);
  add(params, "out.0.weight", {final_ch}); add(params, "out.0.bias", {final_ch});
  add(params, "out.2.weight", {ch, final_ch, 3, 3}); add(params, "out.2.bias", {ch});
  return T2P_OK;
}

int Engine::build() {
  T2P_TRY(arch_.build(cfg_));
  total_ = 0;
  for (const ParamInfo& p : arch_.params) {
    int64_t n = 1;
    for (int64_t d : p.shape) n *= d;
    poff_[p.name] = {total_, n};
    total_ += n;
  }
  T2P_HIP_CHECK(hipGetDevice(&device_));
  return T2P_OK;
}

int Engine::load_param(const char* name, const float* data, const int64_t* shape, int ndim) {
  T2P_REQUIRE(name && data && shape && ndim >= 1 && ndim <= 4, "load_param arguments");
  T2P_REQUIRE(!finalized_, "engine already finalized");
  std::string n(name);
  if (n.rfind("module.", 0) == 0) n = n.substr(7);   // DataParallel state dict (score_sde_pytorch/utils.py:8)
  if (n == "sigmas") return T2P_OK;                   // float64 buffer: derived from the config here
  const ParamInfo* info = nullptr;
  for (const ParamInfo& p : arch_.params)
    if (p.name == n) { info = &p; break; }
  if (!info) {   // load_state_dict(strict=False) ignores unknown keys (score_sde_pytorch/utils.py:14)
    return T2P_OK;
  }
  std::vector<int64_t> s(shape, shape + ndim);
  if (s != info->shape) {
    set_last_error("shape mismatch for " + n);
    return T2P_ERR_INVALID;
  }
  int64_t numel = 1;
  for (int64_t d : s) numel *= d;
  HostTensor& t = host_[n];
  t.shape = s;
  t.data.assign(data, data + numel);
  return T2P_OK;
}

// ---- weights ------------------------------------------------------------------------------------------------------------------------
// Engine::pack_weights is the one walk over the network that knows which persistent weight buffers exist, where they live, which
// packing (t2p_kernels.h: WeightPack) fills each and which dtype / width gates apply.  It has two executors that differ only in who runs
// a packing: finalize() runs it on the host from the tensors load_param collected (weight_pack_host below, then an upload);
// load_flat() launches the same packing on the device from a flat fp32 parameter buffer (weightpack.hip).  Both produce the same bits.

// dense [rows][width] fp32 block -> dst at pitch ld, in dtype
static int upload_block(const std::vector<float>& m, int dtype, void* dst, int64_t rows, int64_t width, int64_t ld) {
  const size_t n = m.size(), es = dtype_size(dtype);
  const void* src = m.data();
  std::vector<uint16_t> h;
  if (dtype != DT_F32) {
    h.resize(n);
    if (dtype == DT_BF16) {
      for (size_t i = 0; i < n; ++i) h[i] = f32_to_bf16_bits(m[i]);
    } else {
      for (size_t i = 0; i < n; ++i) {
        _Float16 x = (_Float16)m[i];
        std::memcpy(&h[i], &x, 2);
      }
    }
    src = h.data();
  }
  if (rows == 1 || ld == width) T2P_HIP_CHECK(hipMemcpy(dst, src, n * es, hipMemcpyHostToDevice));
  else T2P_HIP_CHECK(hipMemcpy2D(dst, (size_t)ld * es, src, (size_t)width * es, (size_t)width * es, (size_t)rows, hipMemcpyHostToDevice));
  return T2P_OK;
}

// out[M][N] = A[M][K] B[K][N] (row-major fp32; weight products formed once at load time), rows spread over a few threads
static std::vector<float> host_matmul(const float* A, const float* B, int64_t M, int64_t K, int64_t N) {
  std::vector<float> out((size_t)M * N, 0.f);
  const int nt = (int)std::min<int64_t>(8, std::max<int64_t>(1, M / 16));
  std::vector<std::thread> th;
  for (int t = 0; t < nt; ++t)
    th.emplace_back([&, t] {
      for (int64_t m = M * t / nt; m < M * (t + 1) / nt; ++m) {
        float* o = out.data() + m * N;
        for (int64_t k = 0; k < K; ++k) {
          const float a = A[m * K + k];
          const float* b = B + k * N;
          for (int64_t n = 0; n < N; ++n) o[n] += a * b[n];
        }
      }
    });
  for (auto& x : th) x.join();
  return out;
}

// host twin of launch_weight_pack: the dense block of packing p (p.src = host pointers; p checked by weight_pack_shape).
//   Linear / 1x1 conv : (N, K[,1,1]) as is          NIN : (K, N) transposed
//   3x3 conv          : (N, Cin, 3, 3) -> [N][kh*3+kw][Cin (padded to cin_pad)]
static void weight_pack_host(const WeightPack& p, std::vector<float>* out) {
  const int64_t* d = p.d;
  const float* const* s = p.src;
  std::vector<float>& m = *out;
  switch (p.kind) {
    case WP_COPY:
      m.assign(s[0], s[0] + d[0]);
      if (d[1]) m.insert(m.end(), s[1], s[1] + d[1]);
      if (d[2]) m.insert(m.end(), s[2], s[2] + d[2]);
      break;
    case WP_ROWS:
      m.assign(s[0], s[0] + d[0] * d[1]);
      break;
    case WP_CONV3: {
      const int64_t N = d[0], ci = d[1], cp = d[2];
      m.assign((size_t)N * 9 * cp, 0.f);
      for (int64_t n = 0; n < N; ++n)
        for (int64_t c = 0; c < ci; ++c)
          for (int tap = 0; tap < 9; ++tap) m[(n * 9 + tap) * cp + c] = s[0][(n * ci + c) * 9 + tap];
      break;
    }
    case WP_CONV3_T: {                                         // [tap][C][N]: lanes (= output channels) read contiguously
      const int64_t N = d[0], C = d[1];
      m.resize((size_t)9 * C * N);
      for (int64_t n = 0; n < N; ++n)
        for (int64_t c = 0; c < C; ++c)
          for (int tap = 0; tap < 9; ++tap) m[(tap * C + c) * N + n] = s[0][(n * C + c) * 9 + tap];
      break;
    }
    case WP_NIN: {
      const int64_t K = d[0], N = d[1];
      m.resize((size_t)d[2] * N * K);
      for (int64_t z = 0; z < d[2]; ++z)
        for (int64_t k = 0; k < K; ++k)
          for (int64_t n = 0; n < N; ++n) m[z * N * K + n * K + k] = s[z][k * N + n];
      break;
    }
    case WP_GEGLU: {                                           // rows interleaved (value_j, gate_j) so the GEMM epilogue can gate in registers
      const int64_t inner = d[0], rl = d[1];
      m.resize((size_t)2 * inner * rl);
      for (int64_t j = 0; j < inner; ++j) {
        std::copy(s[0] + j * rl, s[0] + (j + 1) * rl, m.begin() + (2 * j) * rl);
        std::copy(s[0] + (inner + j) * rl, s[0] + (inner + j + 1) * rl, m.begin() + (2 * j + 1) * rl);
      }
      break;
    }
    case WP_UP4: {
      // conv0 of an up block reads the 2x nearest-up-sampled map (layers.py:306-308): output phase (py, px) of pixel
      // (2 yl + py, 2 xl + px) sees source pixel yl + floor((py + kh - 1) / 2) for kernel row kh, i.e. two source rows per
      // phase; the taps that read the same source pixel are summed here (in fp32, before the one rounding to the compute
      // dtype): four 2x2 convolutions on the source map with 4 / 9 of the multiplications
      const int64_t co = d[0], ci = d[1];
      m.assign((size_t)4 * co * 4 * ci, 0.f);
      auto fl2 = [](int f) { return f >= 0 ? f / 2 : -((-f + 1) / 2); };
      for (int py = 0; py < 2; ++py)
        for (int px = 0; px < 2; ++px)
          for (int kh = 0; kh < 3; ++kh)
            for (int kw = 0; kw < 3; ++kw) {
              const int ty = fl2(py + kh - 1) + 1 - py, tx = fl2(px + kw - 1) + 1 - px;     // 0 or 1
              const size_t ph = (size_t)(py * 2 + px), tap = (size_t)(ty * 2 + tx);
              for (int64_t n = 0; n < co; ++n)
                for (int64_t c = 0; c < ci; ++c)
                  m[((ph * co + n) * 4 + tap) * ci + c] += s[0][(((size_t)n * ci + c) * 3 + kh) * 3 + kw];
            }
      break;
    }
    case WP_ADD:
      m.resize((size_t)d[0]);
      for (int64_t i = 0; i < d[0]; ++i) m[i] = s[0][i] + s[1][i];
      break;
    case WP_PRODUCT: {
      const int64_t M = d[0], K = d[1], N = d[2];
      m = host_matmul(s[0], s[1], M, K, N);
      if (s[2])
        for (int64_t i = 0; i < M; ++i)
          for (int64_t n = 0; n < N; ++n) m[i * N + n] += s[2][n];
      if (d[3]) {
        std::vector<float> t((size_t)M * N);
        for (int64_t i = 0; i < M; ++i)
          for (int64_t n = 0; n < N; ++n) t[n * M + i] = m[i * N + n];
        m.swap(t);
      }
      break;
    }
    case WP_DOT64: {
      const int64_t N = d[0], K = d[1];
      m.resize((size_t)N);
      for (int64_t n = 0; n < N; ++n) {
        double acc = s[2][n];
        for (int64_t j = 0; j < K; ++j) acc += (double)s[0][n * K + j] * s[1][j];
        m[n] = (float)acc;
      }
      break;
    }
  }
}

// the persistent buffer behind *slot: allocated by the first load, reused in place by every later one
int Engine::dest(void** slot, size_t bytes) {
  if (!*slot) *slot = pool_.persistent(bytes);
  return *slot ? T2P_OK : T2P_ERR_HIP;
}

// one parameter tensor as the running executor reads it: a host pointer (finalize) or a slice of the flat device buffer (load_flat)
const float* Engine::psrc(const std::string& name, int64_t numel) {
  auto it = poff_.find(name);
  if (it == poff_.end() || it->second.second != numel) {
    set_last_error((it == poff_.end() ? "no parameter " : "unexpected shape for ") + name);
    return nullptr;
  }
  if (flat_) return flat_ + it->second.first;
  auto h = host_.find(name);
  if (h == host_.end() || (int64_t)h->second.data.size() != numel) {
    set_last_error("parameter not loaded: " + name);
    return nullptr;
  }
  return h->second.data.data();
}
#define T2P_SRC(var, name, numel)                         \
  const float* var = psrc((name), (int64_t)(numel));      \
  if (!var) return T2P_ERR_STATE;

int Engine::pack(int kind, void* dst, int64_t off, int dtype, std::initializer_list<const float*> srcs, std::initializer_list<int64_t> dims) {
  WeightPack p;
  p.kind = kind; p.dtype = dtype; p.dst = (char*)dst + (size_t)off * dtype_size(dtype);
  int i = 0;
  for (const float* s : srcs) p.src[i++] = s;
  i = 0;
  for (int64_t d : dims) p.d[i++] = d;
  int64_t rows = 0, width = 0, ld = 0, rd = 0, wr = 0;
  T2P_TRY(weight_pack_shape(p, &rows, &width, &ld));
  weight_pack_bytes(p, rows, width, &rd, &wr);
  load_stats_[0] += rd; load_stats_[1] += wr; load_stats_[2] += 1;
  if (flat_) return launch_weight_pack(p, pack_stream_);
  std::vector<float> m;
  weight_pack_host(p, &m);
  return upload_block(m, dtype, p.dst, rows, width, ld);
}

// fragment-major copy of a packed 16-bit matrix (stfuse.hip), on the stream of the running load
int Engine::pack_frag(void** slot, const void* w, int N, int K) {
  T2P_TRY(dest(slot, (size_t)N * K * 2));
  load_stats_[0] += (int64_t)N * K * 2; load_stats_[1] += (int64_t)N * K * 2; load_stats_[2] += 1;
  return launch_sf_frag_major(cfg_.compute_dtype, w, *slot, N, K, pack_stream_);
}

// the row-resident GEMM's copy of a packed K = 512 projection (rowgemm.hip), on the stream of the running load: a refresh of the
// weights on the device re-makes it from the re-packed matrix
int Engine::pack_rowres(DevLinear* l) {
  T2P_TRY(dest(&l->w_rf, (size_t)l->N * l->K * 2));
  load_stats_[0] += (int64_t)l->N * l->K * 2; load_stats_[1] += (int64_t)l->N * l->K * 2; load_stats_[2] += 1;
  return launch_rowres_pack(cfg_.compute_dtype, l->w, l->K, l->w_rf, l->N, pack_stream_);
}

int Engine::pack_linear(const std::string& wname, const std::string& bname, int N, int K, DevLinear* out, bool conv3x3, bool nin,
                        int force_dtype, int cin_pad) {
  const int dt = force_dtype >= 0 ? force_dtype : cfg_.compute_dtype;
  const int ci = K / 9, cp = cin_pad ? cin_pad : ci;
  const int Kd = conv3x3 ? 9 * cp : K;
  T2P_SRC(w, wname, (int64_t)N * K);
  T2P_TRY(dest(&out->w, (size_t)N * Kd * dtype_size(dt)));
  if (conv3x3) T2P_TRY(pack(WP_CONV3, out->w, 0, dt, {w}, {N, ci, cp, 0}));
  else if (nin) T2P_TRY(pack(WP_NIN, out->w, 0, dt, {w}, {K, N, 1}));
  else T2P_TRY(pack(WP_COPY, out->w, 0, dt, {w}, {(int64_t)N * K}));       // Linear (N, K) and 1x1 convolution (N, K, 1, 1): as they are
  out->N = N;
  out->K = Kd;
  if (!bname.empty()) {
    T2P_SRC(b, bname, N);
    T2P_TRY(dest((void**)&out->b, (size_t)N * 4));
    T2P_TRY(pack(WP_COPY, out->b, 0, DT_F32, {b}, {N}));
  }
  return T2P_OK;
}

int Engine::pack_stack2(const std::string& w0, const std::string& b0, const std::string& w1, const std::string& b1,
                        int N, int K, bool nin, bool has_bias, DevLinear* out) {
  const int dt = cfg_.compute_dtype;
  T2P_SRC(t0, w0, (int64_t)N * K);
  T2P_SRC(t1, w1, (int64_t)N * K);
  T2P_TRY(dest(&out->w, (size_t)2 * N * K * dtype_size(dt)));
  if (nin) T2P_TRY(pack(WP_NIN, out->w, 0, dt, {t0, t1}, {K, N, 2}));
  else T2P_TRY(pack(WP_COPY, out->w, 0, dt, {t0, t1}, {(int64_t)N * K, (int64_t)N * K}));
  out->N = 2 * N;
  out->K = K;
  if (has_bias) {
    T2P_SRC(c0, b0, N);
    T2P_SRC(c1, b1, N);
    T2P_TRY(dest((void**)&out->b, (size_t)2 * N * 4));
    T2P_TRY(pack(WP_COPY, out->b, 0, DT_F32, {c0, c1}, {N, N}));
  }
  return T2P_OK;
}

int Engine::pack_norm(const std::string& prefix, int C, int G, DevNorm* out) {
  T2P_SRC(g, prefix + ".weight", C);
  T2P_SRC(b, prefix + ".bias", C);
  T2P_TRY(dest((void**)&out->gamma, (size_t)C * 4));
  T2P_TRY(dest((void**)&out->beta, (size_t)C * 4));
  T2P_TRY(pack(WP_COPY, out->gamma, 0, DT_F32, {g}, {C}));
  T2P_TRY(pack(WP_COPY, out->beta, 0, DT_F32, {b}, {C}));
  out->C = C;
  out->G = G;
  return T2P_OK;
}

int Engine::pack_weights() {
  load_stats_[0] = load_stats_[1] = load_stats_[2] = 0;
  const int td = arch_.temb_dim, dt = cfg_.compute_dtype, nf = arch_.nf, Cx = cfg_.num_channels;
  const size_t es = dtype_size(dt);
  T2P_TRY(pack_linear("pre_blocks.0.weight", "pre_blocks.0.bias", td, nf, &pre0_, false, false, DT_F32));
  T2P_TRY(pack_linear("pre_blocks.1.weight", "pre_blocks.1.bias", td, td, &pre1_, false, false, DT_F32));
  T2P_TRY(pack_linear("pre_conv.weight", "pre_conv.bias", nf, 9 * Cx, &pre_conv_, true, false, DT_F32, cpad_));
  {
    T2P_SRC(w, "pre_conv.weight", (int64_t)nf * Cx * 9);
    T2P_TRY(dest((void**)&pre_conv_direct_, (size_t)9 * Cx * nf * 4));
    T2P_TRY(pack(WP_CONV3_T, pre_conv_direct_, 0, DT_F32, {w}, {nf, Cx}));       // [tap][C][nf], unpadded
    // the same weights split into two f16 terms each, for the input convolution on the 16-bit matrix pipe (pre_conv_split_kernel).
    // The split form needs |x| inside the f16 range: the state of a VE run stays within a few sigma_max
    if (dt != DT_F32 && (Cx == 5 || Cx == 8) && cfg_.sigma_max <= 4096.0) {
      T2P_TRY(dest(&pre_conv_split_, pre_conv_split_weight_bytes(Cx, nf)));
      T2P_TRY(launch_pre_conv_split_weights(pre_conv_direct_, pre_conv_split_, Cx, nf, pack_stream_));
      load_stats_[0] += (int64_t)9 * Cx * nf * 4; load_stats_[1] += (int64_t)pre_conv_split_weight_bytes(Cx, nf); load_stats_[2] += 1;
    }
  }
  // the time-embedding table: Dense_0 of every residual block, concatenated (one GEMM per evaluation)
  T2P_TRY(dest(&dense_all_.w, (size_t)arch_.temb_total * td * 4));
  T2P_TRY(dest((void**)&dense_all_.b, (size_t)arch_.temb_total * 4));
  dense_all_.N = arch_.temb_total;
  dense_all_.K = td;
  auto each_layer = [&](auto&& fn) -> int {
    for (Stage& st : arch_.input_stages) for (Layer& l : st.layers) T2P_TRY(fn(l));
    for (Layer& l : arch_.mid_stage.layers) T2P_TRY(fn(l));
    for (Stage& st : arch_.out_stages) for (Layer& l : st.layers) T2P_TRY(fn(l));
    return T2P_OK;
  };
  T2P_TRY(each_layer([&](Layer& l) -> int {
    const std::string& p = l.prefix;
    const int ci = l.in_ch, co = l.out_ch;
    if (l.kind == 0) {
      T2P_TRY(pack_norm(p + ".GroupNorm_0", ci, gn_groups(ci), &l.gn0));
      T2P_TRY(pack_norm(p + ".GroupNorm_1", co, gn_groups(co), &l.gn1));
      T2P_TRY(pack_linear(p + ".Conv_0.weight", p + ".Conv_0.bias", co, 9 * ci, &l.conv0, true));
      if (l.up && dt != DT_F32) {                   // conv0 as four 2x2 phase convolutions (WP_UP4)
        T2P_SRC(w, p + ".Conv_0.weight", (int64_t)co * ci * 9);
        T2P_TRY(dest(&l.conv0_up4, (size_t)16 * co * ci * es));
        T2P_TRY(pack(WP_UP4, l.conv0_up4, 0, dt, {w}, {co, ci}));
      }
      T2P_TRY(pack_linear(p + ".Conv_1.weight", p + ".Conv_1.bias", co, 9 * co, &l.conv1, true));
      if (l.has_conv2) T2P_TRY(pack_linear(p + ".Conv_2.weight", p + ".Conv_2.bias", co, ci, &l.conv2));
      if (l.has_conv2 && !l.up && dt != DT_F32 && ci % 64 == 0 && co % 64 == 0) {
        // h + shortcut(x) = [conv1 | conv2] applied to [3x3 window of a1 | x] (layers.py:322-327): one K loop, one fp32 sum
        T2P_SRC(w1, p + ".Conv_1.weight", (int64_t)co * co * 9);
        T2P_SRC(w2, p + ".Conv_2.weight", (int64_t)co * ci);
        T2P_SRC(b1, p + ".Conv_1.bias", co);
        T2P_SRC(b2, p + ".Conv_2.bias", co);
        const int64_t K1 = (int64_t)9 * co, Kx = K1 + ci;
        T2P_TRY(dest(&l.conv1x.w, (size_t)co * Kx * es));
        T2P_TRY(dest((void**)&l.conv1x.b, (size_t)co * 4));
        T2P_TRY(pack(WP_CONV3, l.conv1x.w, 0, dt, {w1}, {co, co, co, Kx}));
        T2P_TRY(pack(WP_ROWS, l.conv1x.w, K1, dt, {w2}, {co, ci, Kx}));
        T2P_TRY(pack(WP_ADD, l.conv1x.b, 0, DT_F32, {b1, b2}, {co}));
        l.conv1x.N = co; l.conv1x.K = (int)Kx;
      }
      T2P_SRC(w, p + ".Dense_0.weight", (int64_t)co * td);
      T2P_SRC(b, p + ".Dense_0.bias", co);
      T2P_TRY(pack(WP_COPY, dense_all_.w, (int64_t)l.temb_off * td, DT_F32, {w}, {(int64_t)co * td}));
      T2P_TRY(pack(WP_COPY, dense_all_.b, l.temb_off, DT_F32, {b}, {co}));
      // fragment-major copies for the small-map convolution kernel: res_block makes them at the block's first use; a later load renews them
      if (l.fm_conv0) {
        const DevLinear& c1 = l.has_conv2 ? l.conv1x : l.conv1;
        T2P_TRY(pack_frag(&l.fm_conv0, l.conv0.w, co, l.conv0.K));
        T2P_TRY(pack_frag(&l.fm_conv1, c1.w, co, c1.K));
      }
    } else if (l.kind == 1) {
      T2P_TRY(pack_norm(p + ".GroupNorm_0", ci, gn_groups(ci), &l.gn0));
      T2P_TRY(pack_stack2(p + ".NIN_0.W", p + ".NIN_0.b", p + ".NIN_1.W", p + ".NIN_1.b", ci, ci, true, true, &l.qk));
      T2P_TRY(pack_linear(p + ".NIN_2.W", p + ".NIN_2.b", ci, ci, &l.v, false, true));
      T2P_TRY(pack_linear(p + ".NIN_3.W", p + ".NIN_3.b", ci, ci, &l.out, false, true));
      if (dt != DT_F32) {
        T2P_SRC(w2, p + ".NIN_2.W", (int64_t)ci * ci);      // NIN: [in][out]
        T2P_SRC(w3, p + ".NIN_3.W", (int64_t)ci * ci);
        T2P_SRC(b2, p + ".NIN_2.b", ci);
        T2P_SRC(b3, p + ".NIN_3.b", ci);
        T2P_TRY(dest(&l.v3.w, (size_t)ci * ci * es));
        T2P_TRY(dest((void**)&l.v3.b, (size_t)ci * 4));
        T2P_TRY(pack(WP_PRODUCT, l.v3.w, 0, dt, {w2, w3}, {ci, ci, ci, 1, 0}));              // (W2 W3)^T
        T2P_TRY(pack(WP_PRODUCT, l.v3.b, 0, DT_F32, {b2, w3, b3}, {1, ci, ci, 0, 0}));       // b2 W3 + b3
        l.v3.N = ci; l.v3.K = ci;
        if (ci == 256 && l.qk.w && l.qk.b) {
          T2P_TRY(pack_frag(&l.fm_qk, l.qk.w, 2 * ci, ci));
          T2P_TRY(pack_frag(&l.fm_v3, l.v3.w, ci, ci));
        }
      }
    } else {
      const std::string t = p + ".transformer_blocks.0";
      const int ctx = cfg_.context_dim;
      T2P_TRY(pack_norm(p + ".norm", ci, 32, &l.gn0));
      T2P_TRY(pack_linear(p + ".proj_in.weight", p + ".proj_in.bias", ci, ci, &l.proj_in));
      T2P_TRY(pack_linear(p + ".proj_out.weight", p + ".proj_out.bias", ci, ci, &l.proj_out));
      T2P_TRY(pack_stack2(t + ".attn1.to_q.weight", "", t + ".attn1.to_k.weight", "", ci, ci, false, false, &l.a1_qk));
      T2P_TRY(pack_linear(t + ".attn1.to_v.weight", "", ci, ci, &l.a1_v));
      if (dt != DT_F32) {      // the fused attention kernel reads V row-major: q | k | v from one GEMM
        const int64_t cc = (int64_t)ci * ci;
        T2P_SRC(wq, t + ".attn1.to_q.weight", cc);
        T2P_SRC(wk, t + ".attn1.to_k.weight", cc);
        T2P_SRC(wv, t + ".attn1.to_v.weight", cc);
        T2P_TRY(dest(&l.a1_qkv.w, (size_t)3 * cc * es));
        T2P_TRY(pack(WP_COPY, l.a1_qkv.w, 0, dt, {wq, wk, wv}, {cc, cc, cc}));
        l.a1_qkv.N = 3 * ci; l.a1_qkv.K = ci; l.a1_qkv.b = nullptr;
      }
      T2P_TRY(pack_linear(t + ".attn1.to_out.0.weight", t + ".attn1.to_out.0.bias", ci, ci, &l.a1_out));
      T2P_TRY(pack_linear(t + ".attn2.to_q.weight", "", ci, ci, &l.a2_q));
      T2P_TRY(pack_linear(t + ".attn2.to_k.weight", "", ci, ctx, &l.a2_k));
      T2P_TRY(pack_linear(t + ".attn2.to_v.weight", "", ci, ctx, &l.a2_v));
      T2P_TRY(pack_linear(t + ".attn2.to_out.0.weight", t + ".attn2.to_out.0.bias", ci, ci, &l.a2_out));
      {   // GEGLU projection with rows interleaved (value_j, gate_j) so the GEMM epilogue can gate in registers
        const int64_t inner = 4 * ci;
        T2P_SRC(w, t + ".ff.net.0.proj.weight", 2 * inner * ci);
        T2P_SRC(b, t + ".ff.net.0.proj.bias", 2 * inner);
        T2P_TRY(dest(&l.ff1.w, (size_t)2 * inner * ci * es));
        T2P_TRY(dest((void**)&l.ff1.b, (size_t)2 * inner * 4));
        T2P_TRY(pack(WP_GEGLU, l.ff1.w, 0, dt, {w}, {inner, ci}));
        T2P_TRY(pack(WP_GEGLU, l.ff1.b, 0, DT_F32, {b}, {inner, 1}));
        l.ff1.N = 8 * ci;
        l.ff1.K = ci;
      }
      T2P_TRY(pack_linear(t + ".ff.net.2.weight", t + ".ff.net.2.bias", ci, 4 * ci, &l.ff2));
      // (C = 512: the chains stream 4x the bytes per workgroup and measured equal to the separate launches: not built)
      if (dt != DT_F32 && ci == 256 && l.a1_qkv.w) {
        // fragment-major copies of the row-chain kernel's weights (1 KiB contiguous per MFMA fragment)
        T2P_TRY(pack_frag(&l.fm_in, l.proj_in.w, ci, ci));
        T2P_TRY(pack_frag(&l.fm_qkv, l.a1_qkv.w, 3 * ci, ci));
        T2P_TRY(pack_frag(&l.fm_out1, l.a1_out.w, ci, ci));
        T2P_TRY(pack_frag(&l.fm_q2, l.a2_q.w, ci, ci));
        if (ci == 256) {                        // (the chains through the feed-forward exist at C = 256 only)
          T2P_TRY(pack_frag(&l.fm_out2, l.a2_out.w, ci, ci));
          T2P_TRY(pack_frag(&l.fm_ff1, l.ff1.w, 8 * ci, ci));
        }
      }
      if (dt != DT_F32 && ci == 512) {
        // the K = 512 projections the row-resident GEMM takes at the 32 x 32 level (plan switch 49)
        for (DevLinear* pl : {&l.proj_in, &l.a1_qkv, &l.a1_out, &l.a2_q, &l.a2_out, &l.ff1})
          if (pl->w && pl->K == 512 && pl->N % 64 == 0) T2P_TRY(pack_rowres(pl));
      }
      if (dt != DT_F32 && ci % 64 == 0) {
        // proj_out(t + ff2(g)) = [W_po W_ff2 | W_po] [g ; t] + (W_po b_ff2 + b_po), the bias accumulated in double
        T2P_SRC(wpo, p + ".proj_out.weight", (int64_t)ci * ci);
        T2P_SRC(bpo, p + ".proj_out.bias", ci);
        T2P_SRC(wf, t + ".ff.net.2.weight", (int64_t)ci * 4 * ci);
        T2P_SRC(bf, t + ".ff.net.2.bias", ci);
        T2P_TRY(dest(&l.ffpo.w, (size_t)ci * 5 * ci * es));
        T2P_TRY(dest((void**)&l.ffpo.b, (size_t)ci * 4));
        T2P_TRY(pack(WP_PRODUCT, l.ffpo.w, 0, dt, {wpo, wf}, {ci, ci, 4 * ci, 0, 5 * ci}));  // [C][4 C | .]
        T2P_TRY(pack(WP_ROWS, l.ffpo.w, 4 * ci, dt, {wpo}, {ci, ci, 5 * ci}));               // [C][. | C]
        T2P_TRY(pack(WP_DOT64, l.ffpo.b, 0, DT_F32, {wpo, bf, bpo}, {ci, ci}));
        l.ffpo.N = ci; l.ffpo.K = 5 * ci;
        if (ci == 256 && l.fm_in) T2P_TRY(pack_frag(&l.fm_ffpo, l.ffpo.w, ci, 5 * ci));      // the row-chain kernel's third product
      }
      T2P_TRY(pack_norm(t + ".norm1", ci, 1, &l.ln1));
      T2P_TRY(pack_norm(t + ".norm2", ci, 1, &l.ln2));
      T2P_TRY(pack_norm(t + ".norm3", ci, 1, &l.ln3));
    }
    return T2P_OK;
  }));
  T2P_TRY(pack_norm("out.0", arch_.final_ch, gn_groups(arch_.final_ch), &head_norm_));
  T2P_TRY(pack_linear("out.2.weight", "out.2.bias", Cx, 9 * arch_.final_ch, &head_conv_, true));

  if (!inv_sigma_) {                       // tables of the config, not of the weights: made by the first load only
    // 1 / sigmas[label]: sigmas = exp(linspace(log sigma_max, log sigma_min, N)) in float64
    // (models/utils.py:50-60); the reference divides by the float64 value (ncsnpp.py:259-261).
    const int N = cfg_.num_scales;
    std::vector<float> inv(N);
    const double a = std::log(cfg_.sigma_max), b = std::log(cfg_.sigma_min);
    for (int i = 0; i < N; ++i) {
      const double s = std::exp(a + (b - a) * (double)i / (double)(N - 1));
      inv[i] = (float)(1.0 / s);
    }
    T2P_TRY(dest((void**)&inv_sigma_, (size_t)N * 4));
    T2P_TRY(dest((void**)&unit_scale_, (size_t)N * 4));
    T2P_TRY(upload_block(inv, DT_F32, inv_sigma_, 1, N, N));
    T2P_TRY(upload_block(std::vector<float>(N, 1.f), DT_F32, unit_scale_, 1, N, N));
  }
  return T2P_OK;
}

int Engine::finalize() {
  T2P_REQUIRE(!finalized_, "engine already finalized");
  for (const ParamInfo& p : arch_.params) {
    if (!host_.count(p.name)) {
      set_last_error("parameter not loaded: " + p.name);
      return T2P_ERR_STATE;
    }
  }
  flat_ = nullptr;
  pack_stream_ = nullptr;
  T2P_TRY(pack_weights());
  T2P_HIP_CHECK(hipStreamSynchronize(nullptr));       // the fragment-major copies and the split input weights
  host_.clear();
  finalized_ = true;
  return T2P_OK;
}

// The weights from a flat fp32 DEVICE buffer in parameters() order (a trainer's parameters or EMA shadow), packed on the device on
// stream s.  On a finalized engine every buffer is overwritten in place: nothing is allocated and no pointer changes, so captured step
// graphs stay valid.  Nothing is waited for; the caller keeps device_flat alive until s has passed this point.
int Engine::load_flat(const float* device_flat, int64_t n, hipStream_t s) {
  T2P_REQUIRE(device_flat, "load_flat: null buffer");
  T2P_REQUIRE(n == total_, "load_flat: n must equal the element count of the engine's parameter table (" + std::to_string(total_) + ")");
  int dev = -1;
  T2P_HIP_CHECK(hipGetDevice(&dev));
  T2P_REQUIRE(dev == device_, "load_flat: the engine lives on device " + std::to_string(device_) + ", the current device is " + std::to_string(dev));
  flat_ = device_flat;
  pack_stream_ = s;
  const int rc = pack_weights();
  flat_ = nullptr;
  pack_stream_ = nullptr;
  T2P_TRY(rc);
  host_.clear();
  finalized_ = true;
  ctx_B_ = 0;      // the cached text keys / values were projected through the old to_k / to_v: score refuses until set_context ran again
  return T2P_OK;
}

// ------------------------------------------------------------------------------------------------
// every GEMM of the engine: lends the split-K workspace (fp32 partial tiles of low-resolution levels)
int Engine::attach_ws(GemmParams& p) {
  if (!splitk_ws_) {
    splitk_ws_bytes_ = (size_t)256 << 20;
    splitk_ws_ = pool_.persistent(splitk_ws_bytes_);
    if (!splitk_ws_) return T2P_ERR_HIP;
  }
  p.ws = splitk_ws_;
  p.ws_bytes = splitk_ws_bytes_;
  return T2P_OK;
}

int Engine::gemm(GemmParams& p, hipStream_t s) {
  T2P_TRY(attach_ws(p));
  return launch_gemm(p, s);
}

int Engine::gemm_stats(GemmParams& p, float** cstats, hipStream_t s) {
  *cstats = nullptr;
  T2P_TRY(attach_ws(p));          // the fuse predicate depends on the split-K decision
  if (g_plan.fuse_gn_stats && (gemm_fuses_col_stats(p) || gemm_fuses_col_stats_lowp(p))) {
    *cstats = (float*)pool_.get((size_t)(p.M / 64) * p.N * 2 * 4);
    if (!*cstats) return T2P_ERR_HIP;
    p.col_stats = *cstats;
  }
  return gemm(p, s);
}

int Engine::linear(const void* a, bool a_is_f32, const DevLinear& w, long rows, void* c, bool c_f32,
                   const float* residual, float alpha, hipStream_t s, bool use_bias, float** cstats, bool r_lowp) {
  GemmParams p;
  p.dtype = dtype();
  p.A0 = a; p.a_f32 = a_is_f32 || p.dtype == DT_F32; p.C0 = w.K; p.lda0 = w.K;
  p.Bw = w.w; p.ldb = w.K; p.Bw_rf = w.w_rf;
  p.M = (int)rows; p.N = w.N;
  p.bias_n = use_bias ? w.b : nullptr;
  p.R = residual; p.ldr = w.N; p.r_lowp = (residual && r_lowp) ? 1 : 0;
  p.alpha = alpha;
  p.C = c; p.c_f32 = c_f32; p.ldc = w.N;
  if (cstats) return gemm_stats(p, cstats, s);
  return gemm(p, s);
}

int Engine::group_norm(const Act& x, const Act* x1, const DevNorm& n, float eps, int silu, int down, int B, void** out,
                       hipStream_t s, void** raw_out) {
  const int C = x.C + (x1 ? x1->C : 0);
  T2P_REQUIRE(C == n.C, "GroupNorm channel mismatch");
  T2P_REQUIRE(!x1 || x1->lowp == x.lowp, "concatenated sources must share a storage type");
  T2P_REQUIRE(!x.lowp || dtype() != DT_F32, "16-bit activations exist in the 16-bit modes only");
  if (x.pre_norm && !x1 && x.pre_for == &n && x.pre_silu == silu && !down && !raw_out) {
    *out = x.pre_norm;              // the producing split-K second pass already applied this norm (GemmParams::gn_out)
    x.pre_norm = nullptr;           // ownership passes to the caller, which returns it to the pool like any norm output
    return T2P_OK;
  }
  {
    // small maps (<= 64 pixels): statistics + apply in one launch instead of two or three latency-bound ones
    GroupNormApplyArgs g;
    g.x0 = (const float*)x.p; g.x1 = x1 ? (const float*)x1->p : nullptr; g.C0 = x.C; g.C1 = x1 ? x1->C : 0;
    g.B = B; g.H = x.H; g.W = x.W; g.G = n.G; g.gamma = n.gamma; g.beta = n.beta; g.silu = silu; g.down = down;
    g.dtype = dtype(); g.x0_lowp = x.lowp; g.eps = eps;
    if (g_plan.gn_small && gn_small_eligible(g)) {
      const size_t bytes = (size_t)B * x.H * x.W * C * dtype_size(dtype());
      POOL_GET(o, void*, bytes);
      g.out = o;
      if (raw_out) {
        *raw_out = pool_.get(bytes);
        if (!*raw_out) return T2P_ERR_HIP;
        g.raw_out = *raw_out;
      }
      T2P_TRY(launch_gn_small(g, s));
      *out = o;
      return T2P_OK;
    }
  }
  GroupNormArgs a;
  a.x0 = x.p; a.x1 = x1 ? x1->p : nullptr; a.C0 = x.C; a.C1 = x1 ? x1->C : 0;
  a.B = B; a.HW = x.H * x.W; a.G = n.G; a.eps = eps;
  const bool have_cols = x.cstats && (!x1 || x1->cstats) && a.HW % 64 == 0;
  if (have_cols && !raw_out) {
    // maps of <= 4096 pixels: fold the column statistics and normalise in one launch
    GroupNormApplyArgs g;
    g.x0 = a.x0; g.x1 = a.x1; g.C0 = a.C0; g.C1 = a.C1; g.B = B; g.H = x.H; g.W = x.W; g.G = n.G;
    g.gamma = n.gamma; g.beta = n.beta; g.silu = silu; g.down = down; g.dtype = dtype(); g.x0_lowp = x.lowp;
    g.cs0 = x.cstats; g.cs1 = x1 ? x1->cstats : nullptr; g.eps = eps;
    if (gn_apply_cols_eligible(g)) {
      POOL_GET(o, void*, (size_t)B * a.HW * C * dtype_size(dtype()));
      g.out = o;
      T2P_TRY(launch_gn_apply_cols(g, s));
      *out = o;
      return T2P_OK;
    }
  }
  const int nparts = gn_num_chunks(a.HW) * ((C + 1023) / 1024);
  POOL_GET(stats, float*, (size_t)B * n.G * 2 * 4);
  float* partial = nullptr;
  if (have_cols) {
    // statistics came with the producing GEMM's epilogue: no pass over the activation
    T2P_TRY(launch_gn_finalize_cols(x.cstats, x1 ? x1->cstats : nullptr, a.C0, a.C1, B, a.HW, n.G, eps, stats, s));
  } else {
    partial = (float*)pool_.get((size_t)B * nparts * n.G * 2 * 4);
    if (!partial) return T2P_ERR_HIP;
    a.partial = partial; a.stats = stats;
    a.lowp_dtype = x.lowp ? dtype() : DT_F32;
    T2P_TRY(launch_gn_stats(a, s));
  }
  GroupNormApplyArgs g;
  g.x0 = a.x0; g.x1 = a.x1; g.C0 = a.C0; g.C1 = a.C1; g.B = B; g.H = x.H; g.W = x.W; g.G = n.G;
  g.stats = stats; g.gamma = n.gamma; g.beta = n.beta; g.silu = silu; g.down = down; g.dtype = dtype();
  g.x0_lowp = x.lowp;
  const size_t opix = (size_t)B * (down ? x.H / 2 : x.H) * (down ? x.W / 2 : x.W);
  POOL_GET(o, void*, opix * C * dtype_size(dtype()));
  g.out = o;
  if (raw_out) {
    *raw_out = pool_.get(opix * C * dtype_size(dtype()));
    if (!*raw_out) return T2P_ERR_HIP;
    g.raw_out = *raw_out;
  }
  T2P_TRY(launch_gn_apply(g, s));
  pool_.put(partial);
  pool_.put(stats);
  *out = o;
  return T2P_OK;
}

// ResnetBlockBigGANpp.forward (layers.py:303-327)
int Engine::res_block(Layer& L, const Act& x, const Act* skip, Act* out, int B, hipStream_t s, NormHint hint) {
  const int Cin = x.C + (skip ? skip->C : 0), Cout = L.out_ch;
  T2P_REQUIRE(Cin == L.in_ch, "res block input channels");
  T2P_REQUIRE(!(L.down && skip), "down block with concat input");
  const int Ho = L.up ? x.H * 2 : (L.down ? x.H / 2 : x.H), Wo = L.up ? x.W * 2 : (L.down ? x.W / 2 : x.W);
  const long rows_out = (long)B * Ho * Wo;
  const int dt = dtype();
  void* a0 = nullptr;
  // the 1x1 shortcut reads the raw block input: in 16-bit modes GroupNorm-apply (which reads it
  // anyway) also emits it in the compute dtype, so the shortcut GEMM takes the LDS-DMA kernel
  void* xraw = nullptr;
  // (a 16-bit residual stream is already in the GEMM operand format: no raw copy)
  const bool want_raw = g_plan.raw_copies && L.has_conv2 && !L.down && dt != DT_F32 && !x.lowp;
  T2P_TRY(group_norm(x, skip, L.gn0, 1e-6f, 1, L.down, B, &a0, s, want_raw ? &xraw : nullptr));
  // ---- 8x8 / 4x4 maps: each convolution with everything around it in ONE launch (small_conv_gn_kernel): a workgroup owns whole
  // samples x whole groups, so GroupNorm_1 + SiLU (conv0) and the first norm of the block that follows (conv1) need no second
  // pass; the 1x1 shortcut rides as an extra K segment, the identity shortcut as the residual
  if (dt != DT_F32 && !L.up && (Ho * Wo == 16 || Ho * Wo == 64) && x.lowp && (!skip || skip->lowp) && (L.has_conv2 ? L.conv1x.w != nullptr : true)) {
    SmallConvArgs c0;
    c0.dtype = dt; c0.A = a0; c0.B = B; c0.H = Ho; c0.W = Wo; c0.C = Cin; c0.N = Cout; c0.Wt = L.conv0.w; c0.ldw = L.conv0.K;
    c0.bias = L.conv0.b; c0.bias_bn = tb_ + L.temb_off; c0.ld_bn = tb_ld_;
    c0.gn_gamma = L.gn1.gamma; c0.gn_beta = L.gn1.beta; c0.groups = L.gn1.G; c0.gn_silu = 1; c0.gn_eps = 1e-6f;
    SmallConvArgs c1;
    c1.dtype = dt; c1.B = B; c1.H = Ho; c1.W = Wo; c1.C = Cout; c1.N = Cout;
    c1.alpha = cfg_.skip_rescale ? 0.70710678118654752440f : 1.f;
    if (L.has_conv2) {
      c1.Wt = L.conv1x.w; c1.ldw = L.conv1x.K; c1.bias = L.conv1x.b;
      c1.CX0 = L.down ? Cin : x.C; c1.CX1 = (!L.down && skip) ? skip->C : 0;
    } else {
      c1.Wt = L.conv1.w; c1.ldw = L.conv1.K; c1.bias = L.conv1.b;
    }
    const bool olp = res_lowp();
    if (hint.norm && olp && hint.norm->C == Cout) { c1.groups = hint.norm->G; c1.gn_silu = hint.silu; }
    // (eligibility is a matter of shapes: probe with placeholders for the buffers allocated below)
    c0.normed = a0; c1.A = a0; c1.out = a0; c1.normed = c1.groups ? a0 : nullptr;
    c1.gn_gamma = c1.groups ? hint.norm->gamma : nullptr; c1.gn_beta = c1.groups ? hint.norm->beta : nullptr;
    if (L.has_conv2) { c1.X0 = a0; c1.X1 = c1.CX1 ? a0 : nullptr; } else { c1.R = a0; }
    if (small_conv_eligible(c0) && small_conv_eligible(c1)) {
      if (g_plan.small_conv_fm && c0.ldw % 32 == 0 && c1.ldw % 32 == 0) {
        // fragment-major weight copies (whole cache lines per fragment load), made the first time the block takes this path
        if (!L.fm_conv0) {
          // never under a stream capture (the conversions would be recorded, not run, and the copies stay uninitialised: every later
          // evaluation would read garbage weights); the pointers are published only after both copies have been enqueued
          hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
          if (s) (void)hipStreamIsCapturing(s, &cap);
          T2P_REQUIRE(cap == hipStreamCaptureStatusNone, "the first evaluation builds per-block weight copies: run one eager step before capturing");
          void* f0 = pool_.persistent((size_t)Cout * c0.ldw * 2);
          void* f1 = pool_.persistent((size_t)Cout * c1.ldw * 2);
          if (!f0 || !f1) return T2P_ERR_HIP;
          T2P_TRY(launch_sf_frag_major(dt, c0.Wt, f0, Cout, (int)c0.ldw, s));
          T2P_TRY(launch_sf_frag_major(dt, c1.Wt, f1, Cout, (int)c1.ldw, s));
          L.fm_conv0 = f0; L.fm_conv1 = f1;
        }
        c0.Wt = L.fm_conv0; c0.w_fm = 1; c1.Wt = L.fm_conv1; c1.w_fm = 1;
      }
      POOL_GET(a1s, void*, (size_t)rows_out * Cout * dtype_size(dt));
      c0.normed = a1s;
      T2P_TRY(launch_small_conv_gn(c0, s));
      pool_.put(a0);
      void* xpooled = nullptr;
      if (L.has_conv2) {
        if (L.down) {                     // the shortcut of a down block reads the 2x2-averaged input (layers.py:313-315)
          xpooled = pool_.get((size_t)rows_out * Cin * dtype_size(dt));
          if (!xpooled) return T2P_ERR_HIP;
          T2P_TRY(launch_pool2x2(x.p, xpooled, dt, B, x.H, x.W, Cin, s, x.lowp));
          c1.X0 = xpooled;
        } else {
          c1.X0 = x.p;
          c1.X1 = skip ? skip->p : nullptr;
        }
      } else {
        c1.R = x.p;
      }
      POOL_GET(o, float*, (size_t)rows_out * Cout * (olp ? dtype_size(dt) : 4));
      float* o_stats = nullptr;
      void* pre = nullptr;
      if (c1.groups) {
        pre = pool_.get((size_t)rows_out * Cout * dtype_size(dt));
        if (!pre) return T2P_ERR_HIP;
      }
      if (Ho * Wo == 64 && g_plan.fuse_gn_stats) {
        o_stats = (float*)pool_.get((size_t)(rows_out / 64) * Cout * 2 * 4);
        if (!o_stats) return T2P_ERR_HIP;
      }
      c1.A = a1s; c1.out = o; c1.out_f32 = olp ? 0 : 1; c1.col_stats = o_stats; c1.normed = pre;
      T2P_TRY(launch_small_conv_gn(c1, s));
      pool_.put(a1s);
      pool_.put(xpooled);
      *out = Act{o, Cout, Ho, Wo, o_stats, olp};
      out->pre_norm = pre; out->pre_for = pre ? hint.norm : nullptr; out->pre_silu = hint.silu;
      return T2P_OK;
    }
  }
  float* h1_stats = nullptr;
  bool h1_lowp = false;
  void* a1_fused = nullptr;
  POOL_GET(h1, float*, (size_t)rows_out * Cout * 4);
  {
    GemmParams p;
    p.dtype = dt; p.A0 = a0; p.a_f32 = dt == DT_F32; p.C0 = Cin; p.lda0 = Cin;
    p.taps = 9; p.H = Ho; p.W = Wo; p.a_up = L.up;
    p.Bw = L.conv0.w; p.ldb = L.conv0.K; p.M = (int)rows_out; p.N = Cout;
    if (L.up && L.conv0_up4 && !skip) { p.Bw4 = L.conv0_up4; p.ldb4 = 4L * Cin; }
    p.bias_n = L.conv0.b; p.bias_bn = tb_ + L.temb_off; p.ld_bn = tb_ld_; p.rows_per_batch = Ho * Wo;
    p.C = h1; p.c_f32 = 1; p.ldc = Cout;
    // h1 is read once more, by GroupNorm_1 only: when its statistics come out of this epilogue
    // (computed from the fp32 values) the tensor itself is stored in the compute dtype
    T2P_TRY(attach_ws(p));
    if (dt != DT_F32 && gemm_fuses_post_gn(p, L.gn1.G)) {
      // split-K convolution: its second pass applies GroupNorm_1 + SiLU itself (h1 is read by nothing else)
      a1_fused = pool_.get((size_t)rows_out * Cout * dtype_size(dt));
      if (!a1_fused) return T2P_ERR_HIP;
      p.gn_gamma = L.gn1.gamma; p.gn_beta = L.gn1.beta; p.gn_groups = L.gn1.G; p.gn_silu = 1; p.gn_eps = 1e-6f; p.gn_out = a1_fused;
      p.C = nullptr;
      T2P_TRY(gemm(p, s));
    } else {
    // (maps of <= 64 pixels go through the single-launch GroupNorm, which takes its own statistics:
    // h1 stays fp32 there so that they are still taken from unrounded values)
    if (g_plan.lowp_h1 && dt != DT_F32 && g_plan.fuse_gn_stats && gemm_fuses_col_stats(p) && (Ho * Wo) % 64 == 0 &&
        !(g_plan.gn_small && Ho * Wo <= 64)) {
      p.c_f32 = 0;
      h1_lowp = gemm_fuses_col_stats_lowp(p);
      if (!h1_lowp) p.c_f32 = 1;
    }
    T2P_TRY(gemm_stats(p, &h1_stats, s));
    if (h1_lowp && !h1_stats) return T2P_ERR_STATE;
    }
  }
  pool_.put(a0);
  Act h1a{h1, Cout, Ho, Wo, h1_stats, h1_lowp};
  void* a1 = a1_fused;
  if (!a1) T2P_TRY(group_norm(h1a, nullptr, L.gn1, 1e-6f, 1, 0, B, &a1, s));
  free_act(h1a);
  // second convolution; set up here because the shortcut may ride in its K loop
  GemmParams pc;
  pc.dtype = dt; pc.A0 = a1; pc.a_f32 = dt == DT_F32; pc.C0 = Cout; pc.lda0 = Cout;
  pc.taps = 9; pc.H = Ho; pc.W = Wo;
  pc.Bw = L.conv1.w; pc.ldb = L.conv1.K; pc.M = (int)rows_out; pc.N = Cout;
  pc.bias_n = L.conv1.b; pc.rows_per_batch = Ho * Wo;
  pc.alpha = cfg_.skip_rescale ? 0.70710678118654752440f : 1.f;
  bool fused_shortcut = false;
  void* xpooled = nullptr;
  if (L.conv1x.w && (L.down || x.lowp || xraw) && x.C % 64 == 0 && (!skip || skip->C % 64 == 0) && gemm_can_fuse_shortcut(pc)) {
    fused_shortcut = true;
    pc.Bw = L.conv1x.w; pc.ldb = L.conv1x.K; pc.bias_n = L.conv1x.b;
    if (L.down) {                     // the shortcut of a down block reads the 2x2-averaged input (layers.py:313-315)
      xpooled = pool_.get((size_t)rows_out * Cin * dtype_size(dt));
      if (!xpooled) return T2P_ERR_HIP;
      T2P_TRY(launch_pool2x2(x.p, xpooled, dt, B, x.H, x.W, Cin, s, x.lowp));
      pc.X0 = xpooled; pc.CX0 = Cin; pc.ldx0 = Cin;
    } else if (xraw) {
      pc.X0 = xraw; pc.CX0 = Cin; pc.ldx0 = Cin;
    } else {
      pc.X0 = x.p; pc.CX0 = x.C; pc.ldx0 = x.C;
      if (skip) { pc.X1 = skip->p; pc.CX1 = skip->C; pc.ldx1 = skip->C; }
    }
  }
  // shortcut branch
  const float* r = x.p;
  float* rbuf = nullptr;
  bool rbuf_lowp = false;
  int r_up = 0;
  if (fused_shortcut) {
    r = nullptr;
  } else if (L.has_conv2) {
    GemmParams p;
    p.dtype = dt; p.a_f32 = dt == DT_F32;
    void* pooled = nullptr;
    long rrows;
    if (L.down) {
      pooled = pool_.get((size_t)rows_out * Cin * dtype_size(dt));
      if (!pooled) return T2P_ERR_HIP;
      T2P_TRY(launch_pool2x2(x.p, pooled, dt, B, x.H, x.W, Cin, s, x.lowp));
      p.A0 = pooled; p.C0 = Cin; p.lda0 = Cin;
      rrows = rows_out;
    } else {
      if (xraw) {
        p.A0 = xraw; p.C0 = Cin; p.lda0 = Cin;
      } else {
        p.a_f32 = x.lowp ? 0 : 1;       // 16-bit stream: the LDS-DMA kernel reads both concat sources in place
        p.A0 = x.p; p.C0 = x.C; p.lda0 = x.C;
        if (skip) { p.A1 = skip->p; p.C1 = skip->C; p.lda1 = skip->C; }
      }
      rrows = (long)B * x.H * x.W;   // for `up` the 1x1 conv runs at the low resolution: it commutes
      r_up = L.up;                   // with nearest up-sampling exactly
    }
    rbuf_lowp = false;   // the shortcut output stays fp32: storing it in 16 bits measured no gain and costs accuracy
    rbuf = (float*)pool_.get((size_t)rrows * Cout * (rbuf_lowp ? dtype_size(dt) : 4));
    if (!rbuf) return T2P_ERR_HIP;
    p.Bw = L.conv2.w; p.ldb = L.conv2.K; p.M = (int)rrows; p.N = Cout; p.bias_n = L.conv2.b;
    p.C = rbuf; p.c_f32 = rbuf_lowp ? 0 : 1; p.ldc = Cout;
    T2P_TRY(gemm(p, s));
    pool_.put(pooled);
    pool_.put(xraw);
    r = rbuf;
  } else {
    T2P_REQUIRE(!skip && Cin == Cout, "identity shortcut needs equal channels");
  }
  const bool olp = res_lowp();           // block output (the residual stream) in the compute dtype
  POOL_GET(o, float*, (size_t)rows_out * Cout * (olp ? dtype_size(dt) : 4));
  float* o_stats = nullptr;
  pc.R = r; pc.ldr = Cout; pc.r_up = r_up;
  pc.r_lowp = (r == x.p ? x.lowp : rbuf_lowp) ? 1 : 0;   // identity shortcut: the block input itself
  pc.C = o; pc.c_f32 = olp ? 0 : 1; pc.ldc = Cout;
  void* pre = nullptr;
  T2P_TRY(attach_ws(pc));
  if (hint.norm && olp && hint.norm->C == Cout && gemm_fuses_post_gn(pc, hint.norm->G)) {
    // the block that follows starts with a GroupNorm of this output alone: the split-K second pass applies it as well, and
    // still writes the output itself (residual stream) with its column statistics (skip connections)
    pre = pool_.get((size_t)rows_out * Cout * dtype_size(dt));
    if (!pre) return T2P_ERR_HIP;
    pc.gn_gamma = hint.norm->gamma; pc.gn_beta = hint.norm->beta; pc.gn_groups = hint.norm->G; pc.gn_silu = hint.silu; pc.gn_eps = 1e-6f;
    if ((Ho * Wo) % 64 == 0 && g_plan.fuse_gn_stats) {
      o_stats = (float*)pool_.get((size_t)(rows_out / 64) * Cout * 2 * 4);
      if (!o_stats) return T2P_ERR_HIP;
      pc.col_stats = o_stats;
    }
    pc.gn_out = pre;
    T2P_TRY(gemm(pc, s));
  } else {
    T2P_TRY(gemm_stats(pc, &o_stats, s));
  }
  pool_.put(a1);
  pool_.put(rbuf);
  if (fused_shortcut) { pool_.put(xraw); pool_.put(xpooled); }
  *out = Act{o, Cout, Ho, Wo, o_stats, olp};
  out->pre_norm = pre; out->pre_for = hint.norm; out->pre_silu = hint.silu;
  return T2P_OK;
}

// softmax(q k^T * scale) v for [B][heads]; q,k row-major with head h at column h*d; vt = v^T
int Engine::attention(const void* q, long ldq, const void* k, long ldk, const void* vt, long ldvt, void* out, int B,
                      int heads, int nq, int nk, int d, float scale, hipStream_t s) {
  const int dt = dtype();
  if (g_plan.flash_attention && attention_flash_eligible(dt, d, ldq, ldk, ldvt, (long)heads * d))
    return launch_attention_flash(dt, q, ldq, k, ldk, vt, ldvt, out, B, heads, nq, nk, d, scale, s);
  if (attention_strip_eligible(dt, heads, nq, nk, d, ldq, ldk, ldvt, d))
    return launch_attention_strip(dt, q, ldq, k, ldk, vt, ldvt, out, d, B, nq, d, scale, s);
  const long nkp = (long)round_up((size_t)nk, 8);
  const long rows = (long)B * heads * nq;
  POOL_GET(S, float*, (size_t)rows * nkp * 4);
  POOL_GET(P, void*, (size_t)rows * nkp * dtype_size(dt));
  GemmParams p;
  p.dtype = dt; p.a_f32 = dt == DT_F32;
  p.A0 = q; p.C0 = d; p.lda0 = ldq; p.M = nq; p.N = nk;
  p.Bw = k; p.ldb = ldk;
  p.nz0 = B; p.nz1 = heads;
  p.sA_z0 = (long)nq * ldq; p.sA_z1 = d; p.sB_z0 = (long)nk * ldk; p.sB_z1 = d;
  p.C = S; p.c_f32 = 1; p.ldc = nkp; p.sC_z0 = (long)heads * nq * nkp; p.sC_z1 = (long)nq * nkp;
  T2P_TRY(gemm(p, s));
  T2P_TRY(launch_softmax(S, nkp, P, nkp, dt, rows, nk, scale, s));
  GemmParams r;
  r.dtype = dt; r.a_f32 = dt == DT_F32;
  r.A0 = P; r.C0 = nk; r.lda0 = nkp; r.M = nq; r.N = d;
  r.Bw = vt; r.ldb = ldvt;
  r.nz0 = B; r.nz1 = heads;
  r.sA_z0 = (long)heads * nq * nkp; r.sA_z1 = (long)nq * nkp; r.sB_z0 = (long)heads * d * ldvt; r.sB_z1 = (long)d * ldvt;
  r.C = out; r.c_f32 = 0; r.ldc = (long)heads * d; r.sC_z0 = (long)nq * heads * d; r.sC_z1 = d;
  T2P_TRY(launch_gemm(r, s));
  pool_.put(S);
  pool_.put(P);
  return T2P_OK;
}

// v^T[b] = W_v a_b^T : [C][n] (row stride npad) -- the projection is written transposed so that
// P V is a plain "A row-major, B = [N][K]" GEMM with no transposing loads.
static int project_vt(int dt, const DevLinear& wv, const void* a, long lda, int B, int n, long npad, void* vt,
                      hipStream_t s) {
  GemmParams p;
  p.dtype = dt; p.a_f32 = dt == DT_F32;
  p.A0 = wv.w; p.C0 = wv.K; p.lda0 = wv.K; p.M = wv.N; p.N = n;
  p.Bw = a; p.ldb = lda;
  p.nz0 = B; p.sA_z0 = 0; p.sB_z0 = (long)n * lda;
  p.bias_m = wv.b;
  p.C = vt; p.c_f32 = 0; p.ldc = npad; p.sC_z0 = (long)wv.N * npad;
  return launch_gemm(p, s);
}

// AttnBlockpp.forward (layers.py:160-176)
int Engine::attn_block(Layer& L, const Act& x, Act* out, int B, hipStream_t s) {
  const int C = x.C, n = x.H * x.W, dt = dtype();
  const size_t es = dtype_size(dt);
  const long rows = (long)B * n, npad = (long)round_up((size_t)n, 8);
  const bool olp = res_lowp();
  const bool merged = g_plan.attn_merged && L.v3.w && attention_strip_eligible(dt, 1, n, n, C, 2 * C, 2 * C, npad, C) && (!x.lowp || olp);
  if (merged && x.lowp && L.fm_qk && g_plan.attn_proj) {
    // C = 256: GroupNorm apply, q | k and the transposed value projection as ONE launch over 32-row blocks (attn_proj_kernel)
    AttnProjArgs e;
    e.dtype = dt; e.B = B; e.n = n; e.C = C; e.npad = npad;
    const bool normed = x.pre_norm && x.pre_for == &L.gn0 && x.pre_silu == 0;
    e.x = normed ? x.pre_norm : (const void*)x.p;
    e.cstats = normed ? nullptr : x.cstats;
    e.gn_gamma = L.gn0.gamma; e.gn_beta = L.gn0.beta; e.groups = L.gn0.G; e.gn_eps = 1e-6f;
    e.w_qk = L.fm_qk; e.b_qk = L.qk.b; e.w_v = L.fm_v3;
    if ((normed || x.cstats) && attn_proj_eligible(e)) {
      POOL_GET(qk2, char*, (size_t)rows * 2 * C * es);
      POOL_GET(vt2, void*, (size_t)B * C * npad * es);
      e.qk = qk2; e.vt = vt2;
      void* kfm2 = nullptr;
      if (g_plan.attn_fm && npad == n && attention_strip_frag_major_ok(dt, n, C)) {     // K and V^T in the order the attention kernel streams them
        kfm2 = pool_.get((size_t)rows * C * es);
        if (!kfm2) return T2P_ERR_HIP;
        e.k_fm = kfm2;
      }
      T2P_TRY(launch_attn_proj(e, s));
      if (normed) { pool_.put(x.pre_norm); x.pre_norm = nullptr; }
      const float att_scale2 = 1.f / std::sqrt((float)C);
      POOL_GET(y, float*, (size_t)rows * C * (olp ? es : 4));
      float* y_stats = nullptr;
      if (g_plan.fuse_gn_stats && n % 64 == 0) {
        y_stats = (float*)pool_.get((size_t)(rows / 64) * C * 2 * 4);
        if (!y_stats) return T2P_ERR_HIP;
      }
      StripEpilogue ep;
      ep.bias = L.v3.b; ep.residual = x.p; ep.r_lowp = 1; ep.ldr = C; ep.alpha = cfg_.skip_rescale ? 0.70710678118654752440f : 1.f;
      ep.out_f32 = olp ? 0 : 1; ep.col_stats = y_stats;
      ep.frag_major = kfm2 ? 1 : 0;
      if (kfm2) T2P_TRY(launch_attention_strip(dt, qk2, 2 * C, kfm2, C, vt2, npad, y, C, B, n, C, att_scale2, s, &ep));
      else T2P_TRY(launch_attention_strip(dt, qk2, 2 * C, qk2 + (size_t)C * es, 2 * C, vt2, npad, y, C, B, n, C, att_scale2, s, &ep));
      pool_.put(kfm2);
      pool_.put(qk2);
      pool_.put(vt2);
      *out = Act{y, C, x.H, x.W, y_stats, olp};
      return T2P_OK;
    }
  }
  void* a = nullptr;
  T2P_TRY(group_norm(x, nullptr, L.gn0, 1e-6f, 0, 0, B, &a, s));
  POOL_GET(qk, char*, (size_t)rows * 2 * C * es);
  // q | k projection; where the wide-head attention kernel takes fragment-major operands (plan switch 45: the 32 x 32 level of the
  // C = 512 configurations) the k columns and the transposed values are written that way by the products' epilogues
  GemmParams pq;
  pq.dtype = dt; pq.A0 = a; pq.a_f32 = dt == DT_F32; pq.C0 = C; pq.lda0 = C; pq.Bw = L.qk.w; pq.ldb = C; pq.M = (int)rows; pq.N = 2 * C;
  pq.bias_n = L.qk.b; pq.C = qk; pq.c_f32 = 0; pq.ldc = 2 * C;
  T2P_TRY(attach_ws(pq));
  void* kfm = nullptr;
  GemmParams pv;      // the transposed value projection of the merged path (project_vt's parameters), probed for the same option
  pv.dtype = dt; pv.a_f32 = dt == DT_F32; pv.A0 = L.v3.w; pv.C0 = C; pv.lda0 = C; pv.M = C; pv.N = n; pv.Bw = a; pv.ldb = C;
  pv.nz0 = B; pv.sA_z0 = 0; pv.sB_z0 = (long)n * C; pv.c_f32 = 0; pv.ldc = npad; pv.sC_z0 = (long)C * npad;
  T2P_TRY(attach_ws(pv));
  bool fm = false;
  if (merged && g_plan.attn_fm && npad == n && attention_strip_frag_major_ok(dt, n, C)) {
    GemmParams tq = pq, tv = pv;
    tq.rows_per_batch = n; tq.frag_col0 = C; tq.frag_ns = C / 32; tq.frag_bstride = (long)n * C; tq.c_frag = qk;     // (placeholder pointers)
    tv.frag_col0 = 0; tv.frag_ns = n / 32; tv.frag_bstride = (long)n * C; tv.c_frag = qk; tv.C = qk;
    fm = gemm_writes_frag_major(tq) && gemm_writes_frag_major(tv);
    if (fm) {
      kfm = pool_.get((size_t)rows * C * es);
      if (!kfm) return T2P_ERR_HIP;
      tq.c_frag = kfm;
      pq = tq;
      pv = tv;
    }
  }
  T2P_TRY(launch_gemm(pq, s));
  POOL_GET(vt, void*, (size_t)B * C * npad * es);
  const float att_scale = 1.f / std::sqrt((float)C);
  const float out_alpha = cfg_.skip_rescale ? 0.70710678118654752440f : 1.f;
  if (merged) {
    // NIN_2 and NIN_3 as one projection (Layer::v3): the attention kernel's epilogue adds b2 W3 + b3 and the block input and
    // scales by 1 / sqrt 2 -- (x + NIN_3(softmax(q k^T) v)) / sqrt 2, layers.py:170-176 -- no output-projection GEMM
    if (fm) {
      pv.C = vt; pv.c_frag = vt;           // every column fragment-major: C itself receives nothing
      T2P_TRY(launch_gemm(pv, s));
    } else {
      DevLinear nob = L.v3;
      nob.b = nullptr;
      T2P_TRY(project_vt(dt, nob, a, C, B, n, npad, vt, s));
    }
    pool_.put(a);
    POOL_GET(y, float*, (size_t)rows * C * (olp ? es : 4));
    float* y_stats = nullptr;
    if (g_plan.fuse_gn_stats && n % 64 == 0) {
      y_stats = (float*)pool_.get((size_t)(rows / 64) * C * 2 * 4);
      if (!y_stats) return T2P_ERR_HIP;
    }
    StripEpilogue ep;
    ep.bias = L.v3.b; ep.residual = x.p; ep.r_lowp = x.lowp ? 1 : 0; ep.ldr = C; ep.alpha = out_alpha; ep.out_f32 = olp ? 0 : 1;
    ep.col_stats = y_stats;
    ep.frag_major = fm ? 1 : 0;
    if (fm) T2P_TRY(launch_attention_strip(dt, qk, 2 * C, kfm, C, vt, npad, y, C, B, n, C, att_scale, s, &ep));
    else T2P_TRY(launch_attention_strip(dt, qk, 2 * C, qk + (size_t)C * es, 2 * C, vt, npad, y, C, B, n, C, att_scale, s, &ep));
    pool_.put(kfm);
    pool_.put(qk);
    pool_.put(vt);
    *out = Act{y, C, x.H, x.W, y_stats, olp};
    return T2P_OK;
  }
  T2P_TRY(project_vt(dt, L.v, a, C, B, n, npad, vt, s));
  pool_.put(a);
  POOL_GET(o, void*, (size_t)rows * C * es);
  T2P_TRY(attention(qk, 2 * C, qk + (size_t)C * es, 2 * C, vt, npad, o, B, 1, n, n, C, att_scale, s));
  pool_.put(qk);
  pool_.put(vt);
  POOL_GET(y, float*, (size_t)rows * C * (olp ? es : 4));
  float* y_stats = nullptr;
  T2P_TRY(linear(o, false, L.out, rows, y, !olp, x.p, out_alpha, s, true, &y_stats, x.lowp));
  pool_.put(o);
  *out = Act{y, C, x.H, x.W, y_stats, olp};
  return T2P_OK;
}

// SpatialTransformer.forward with one BasicTransformerBlock (attention.py:208-215, 250-263)
// plan switch 40: the chain after the cross-attention (to_out + residual -> LayerNorm_3 -> ff.net.0 with GEGLU) on the row-block kernel
// too: every workgroup streams 1.15 MB of weights for it, which pays only when the launch fills the chip (>= 8192 rows: cfg3
// 16.26 -> 16.19 ms per step; at cfg5's 4096 rows 10.53 -> 10.55, so the three separate launches stay there).  With row-major weights
// (half of every fetched line unused, each line fetched twice) the chain was slower everywhere: 16.83 -> 16.88 ms at cfg3.
// development key 43: fewest rows for which the block's last chain (with the third product) is taken; without the third product
// (plan switch 42 off) the chain needs twice as many (measured at cfg5's 4096 rows: +0.02 ms without, -0.06 ms with it)
int Engine::st_block(Layer& L, const Act& x, Act* out, int B, hipStream_t s) {
  const int C = x.C, n = x.H * x.W, dt = dtype(), heads = cfg_.n_heads, d = C / heads;
  const size_t es = dtype_size(dt);
  const long rows = (long)B * n, npad = (long)round_up((size_t)n, 8);
  const float scale = 1.f / std::sqrt((float)d);
  T2P_REQUIRE(L.ctx_k && L.ctx_vt && ctx_B_ == B, "set_context must be called with the same batch before score");
  // the block's own residual stream t: fp32, or the compute dtype together with the stream between blocks
  const bool tl = res_lowp();
  POOL_GET(t, float*, (size_t)rows * C * (tl ? es : 4));
  const bool qkv_flash = g_plan.qkv_fused && L.a1_qkv.w && g_plan.flash_attention && attention_flash_eligible(dt, d, 3 * C, 3 * C, 3 * C, C);
  // GroupNorm -> proj_in -> LayerNorm_1 -> q | k | v as ONE launch where the row-block kernel applies (stfuse.hip)
  char* qkv_pre = nullptr;
  // the block's last launch (plan switch 42): to_out + residual -> LayerNorm_3 -> ff.net.0 (GEGLU) -> [g | t] W_ffpo + x in one kernel;
  // its column sums are accumulated by pairs of workgroups into a buffer the entry kernel zeroes
  const bool mega = tl && x.lowp && qkv_flash && g_plan.st_tail && g_plan.st_ffpo && g_plan.ffpo_merged && L.fm_ffpo && L.fm_ff1 && rows >= g_plan.st_tail_rows && n % 64 == 0 &&
                    g_plan.fuse_geglu && L.a2_out.b && L.ff1.b;
  float* y2 = nullptr;
  float* y2_stats = nullptr;
  if (tl && x.lowp && qkv_flash) {
    StEntryArgs e;
    e.dtype = dt; e.B = B; e.n = n; e.C = C;
    const bool normed = x.pre_norm && x.pre_for == &L.gn0 && x.pre_silu == 0;
    e.x = normed ? x.pre_norm : (const void*)x.p;
    e.cstats = normed ? nullptr : x.cstats;
    e.gn_gamma = L.gn0.gamma; e.gn_beta = L.gn0.beta; e.groups = L.gn0.G; e.gn_eps = 1e-6f;
    e.w_in = L.fm_in; e.b_in = L.proj_in.b;
    e.ln_gamma = L.ln1.gamma; e.ln_beta = L.ln1.beta; e.ln_eps = 1e-5f;
    e.w_qkv = L.fm_qkv; e.n2 = 3 * C;
    // (no column sums and no producer-side norm -- the 4 x 4 level: the GroupNorm as its own small launch, the rest of the chain here)
    void* a_small = nullptr;
    if (!normed && !x.cstats && L.proj_in.b && L.fm_in && g_plan.st_fuse) {
      StEntryArgs probe = e;
      probe.x = x.p; probe.cstats = nullptr;
      if (st_entry_eligible(probe)) {
        T2P_TRY(group_norm(x, nullptr, L.gn0, 1e-6f, 0, 0, B, &a_small, s));
        e.x = a_small; e.cstats = nullptr;
      }
    }
    if ((normed || x.cstats || a_small) && L.proj_in.b && L.fm_in && st_entry_eligible(e)) {
      qkv_pre = (char*)pool_.get((size_t)rows * 3 * C * es);
      if (!qkv_pre) return T2P_ERR_HIP;
      if (mega) {
        y2 = (float*)pool_.get((size_t)rows * C * es);
        if (!y2) return T2P_ERR_HIP;
        if (g_plan.fuse_gn_stats) {
          y2_stats = (float*)pool_.get((size_t)(rows / 64) * C * 2 * 4);
          if (!y2_stats) return T2P_ERR_HIP;
          e.zero = y2_stats; e.zero_n = (long)(rows / 64) * C * 2;
        }
      }
      e.t = t; e.qkv = qkv_pre;
      T2P_TRY(launch_st_entry(e, s));
      if (normed) { pool_.put(x.pre_norm); x.pre_norm = nullptr; }
    }
    pool_.put(a_small);
  }
  if (!qkv_pre) {
    void* a = nullptr;
    T2P_TRY(group_norm(x, nullptr, L.gn0, 1e-6f, 0, 0, B, &a, s));
    T2P_TRY(linear(a, false, L.proj_in, rows, t, !tl, nullptr, 1.f, s));
    pool_.put(a);
  }
  POOL_GET(ln, void*, (size_t)rows * C * es);
  POOL_GET(o, void*, (size_t)rows * C * es);
  // attn1: self-attention
  if (!qkv_pre) T2P_TRY(launch_layernorm(t, L.ln1.gamma, L.ln1.beta, ln, dt, rows, C, 1e-5f, s, tl));
  if (qkv_flash) {
    char* qkv = qkv_pre;
    if (!qkv) {
      qkv = (char*)pool_.get((size_t)rows * 3 * C * es);
      if (!qkv) return T2P_ERR_HIP;
      T2P_TRY(linear(ln, false, L.a1_qkv, rows, qkv, false, nullptr, 1.f, s, false));
    }
    T2P_TRY(launch_attention_flash(dt, qkv, 3 * C, qkv + (size_t)C * es, 3 * C, qkv + (size_t)2 * C * es, 3 * C, o, B, heads, n, n, d, scale, s,
                                   true));
    pool_.put(qkv);
  } else {
    POOL_GET(qk, char*, (size_t)rows * 2 * C * es);
    T2P_TRY(linear(ln, false, L.a1_qk, rows, qk, false, nullptr, 1.f, s, false));
    POOL_GET(vt, void*, (size_t)B * C * npad * es);
    T2P_TRY(project_vt(dt, L.a1_v, ln, C, B, n, npad, vt, s));
    T2P_TRY(attention(qk, 2 * C, qk + (size_t)C * es, 2 * C, vt, npad, o, B, heads, n, n, d, scale, s));
    pool_.put(qk);
    pool_.put(vt);
  }
  // attn2: cross-attention to the cached text keys / values.  t += to_out(o) -> LayerNorm_2 -> to_q: one launch where the row-block
  // kernel applies (the first product's residual and output are both t: a workgroup's rows are its own)
  {
    POOL_GET(q, void*, (size_t)rows * C * es);
    StEntryArgs e;
    e.dtype = dt; e.B = B; e.n = n; e.C = C; e.x = o; e.w_in = L.fm_out1; e.b_in = L.a1_out.b; e.res = t;
    e.ln_gamma = L.ln2.gamma; e.ln_beta = L.ln2.beta; e.ln_eps = 1e-5f; e.w_qkv = L.fm_q2; e.n2 = C; e.t = t; e.qkv = q;
    if (tl && qkv_pre && L.a1_out.b && !L.a2_q.b && st_entry_eligible(e)) {
      T2P_TRY(launch_st_entry(e, s));
    } else {
      T2P_TRY(linear(o, false, L.a1_out, rows, t, !tl, t, 1.f, s, true, nullptr, tl));
      T2P_TRY(launch_layernorm(t, L.ln2.gamma, L.ln2.beta, ln, dt, rows, C, 1e-5f, s, tl));
      T2P_TRY(linear(ln, false, L.a2_q, rows, q, false, nullptr, 1.f, s, false));
    }
    T2P_TRY(attention(q, C, L.ctx_k, C, L.ctx_vt, ctx_Tpad_, o, B, heads, n, ctx_T_, d, scale, s));
    pool_.put(q);
  }
  // feed-forward with GEGLU.  t += to_out(o) -> LayerNorm_3 -> ff.net.0 (GEGLU): one launch where the row-block kernel applies
  {
    POOL_GET(g, void*, (size_t)rows * 4 * C * es);
    GemmParams p;
    p.dtype = dt; p.A0 = ln; p.a_f32 = dt == DT_F32; p.C0 = C; p.lda0 = C;
    p.Bw = L.ff1.w; p.ldb = C; p.Bw_rf = L.ff1.w_rf; p.M = (int)rows; p.N = 8 * C; p.bias_n = L.ff1.b;
    p.C = g; p.c_f32 = 0; p.ldc = 4 * C; p.geglu = 1;
    T2P_TRY(attach_ws(p));
    StEntryArgs e;
    e.dtype = dt; e.B = B; e.n = n; e.C = C; e.x = o; e.w_in = L.fm_out2; e.b_in = L.a2_out.b; e.res = t;
    e.ln_gamma = L.ln3.gamma; e.ln_beta = L.ln3.beta; e.ln_eps = 1e-5f; e.w_qkv = L.fm_ff1; e.b2 = L.ff1.b; e.n2 = 8 * C; e.geglu = 1;
    e.t = t; e.qkv = g;
    const bool tail_chain = tl && qkv_pre && g_plan.st_tail && (y2 || rows >= 2 * g_plan.st_tail_rows) && L.fm_ff1 && g_plan.fuse_geglu && gemm_fuses_geglu(p) && L.a2_out.b && L.ff1.b && st_entry_eligible(e);
    if (tail_chain && y2) {
      e.w3 = L.fm_ffpo; e.b3 = L.ffpo.b; e.res3 = x.p; e.y = y2; e.y_stats = y2_stats; e.qkv = nullptr;
      T2P_REQUIRE(st_entry_eligible(e), "row chain with the third product");
      T2P_TRY(launch_st_entry(e, s));
      pool_.put(g); pool_.put(o); pool_.put(ln); pool_.put(t);
      *out = Act{y2, C, x.H, x.W, y2_stats, true};
      return T2P_OK;
    }
    if (y2) { pool_.put(y2); pool_.put(y2_stats); y2 = nullptr; y2_stats = nullptr; }     // (entry chain taken, tail not: unused)
    if (tail_chain) {
      T2P_TRY(launch_st_entry(e, s));
    } else {
      T2P_TRY(linear(o, false, L.a2_out, rows, t, !tl, t, 1.f, s, true, nullptr, tl));
      T2P_TRY(launch_layernorm(t, L.ln3.gamma, L.ln3.beta, ln, dt, rows, C, 1e-5f, s, tl));
    }
    if (tail_chain) {
    } else if (g_plan.fuse_geglu && gemm_fuses_geglu(p)) {
      T2P_TRY(gemm(p, s));                       // value * gelu(gate) in the GEMM epilogue
    } else {
      POOL_GET(u, float*, (size_t)rows * 8 * C * 4);
      T2P_TRY(linear(ln, false, L.ff1, rows, u, true, nullptr, 1.f, s));
      T2P_TRY(launch_geglu(u, g, dt, rows, 4 * C, s, 1));
      pool_.put(u);
    }
    if (g_plan.ffpo_merged && tl && L.ffpo.w) {
      // ff.net.2 and proj_out as ONE product over [g | t] (Layer::ffpo): x + proj_out(t + ff2(g)), attention.py:213-215, 259-263
      pool_.put(o);
      const bool olp2 = res_lowp();
      POOL_GET(y2, float*, (size_t)rows * C * (olp2 ? es : 4));
      float* y2_stats = nullptr;
      GemmParams q;
      q.dtype = dt; q.a_f32 = 0; q.A0 = g; q.C0 = 4 * C; q.lda0 = 4 * C; q.A1 = t; q.C1 = C; q.lda1 = C;
      q.Bw = L.ffpo.w; q.ldb = L.ffpo.K; q.M = (int)rows; q.N = C; q.bias_n = L.ffpo.b;
      q.R = x.p; q.ldr = C; q.r_lowp = x.lowp ? 1 : 0;
      q.C = y2; q.c_f32 = olp2 ? 0 : 1; q.ldc = C; q.rows_per_batch = n;
      T2P_TRY(gemm_stats(q, &y2_stats, s));
      pool_.put(g);
      pool_.put(ln);
      pool_.put(t);
      *out = Act{y2, C, x.H, x.W, y2_stats, olp2};
      return T2P_OK;
    }
    T2P_TRY(linear(g, false, L.ff2, rows, t, !tl, t, 1.f, s, true, nullptr, tl));
    pool_.put(g);
  }
  pool_.put(o);
  const bool olp = res_lowp();
  POOL_GET(y, float*, (size_t)rows * C * (olp ? es : 4));
  float* y_stats = nullptr;
  if (tl) {                                              // t already is a GEMM operand
    T2P_TRY(linear(t, false, L.proj_out, rows, y, !olp, x.p, 1.f, s, true, &y_stats, x.lowp));
  } else if (dt != DT_F32 && g_plan.raw_copies) {
    T2P_TRY(launch_convert(t, ln, dt, rows * C, s));     // residual stream -> compute dtype (reuses the LN buffer)
    T2P_TRY(linear(ln, false, L.proj_out, rows, y, !olp, x.p, 1.f, s, true, &y_stats, x.lowp));
  } else {
    T2P_TRY(linear(t, true, L.proj_out, rows, y, !olp, x.p, 1.f, s, true, &y_stats, x.lowp));
  }
  pool_.put(ln);
  pool_.put(t);
  *out = Act{y, C, x.H, x.W, y_stats, olp};
  return T2P_OK;
}

// the first norm of `l` when it reads its input alone at full resolution (what a producer may apply ahead of time)
static NormHint first_norm_of(const Layer* l, bool concat_input) {
  NormHint h;
  if (!l || concat_input || l->down) return h;
  h.norm = &l->gn0;
  h.silu = l->kind == 0 ? 1 : 0;
  return h;
}

int Engine::run_stage(Stage& st, Act& h, const Act* skip, int B, hipStream_t s, const Layer* next_after) {
  Act cur = h;
  bool own = false;   // cur was produced inside this stage
  for (size_t i = 0; i < st.layers.size(); ++i) {
    Layer& L = st.layers[i];
    Act nxt;
    LayerScope scope(L.prefix + (L.kind == 0 ? (L.up ? ",res_up," : L.down ? ",res_down," : ",res,") : L.kind == 1 ? ",attn," : ",st,") +
                     std::to_string(cur.H) + "," + std::to_string(L.in_ch) + "," + std::to_string(L.out_ch), s);
    const Layer* nextL = i + 1 < st.layers.size() ? &st.layers[i + 1] : next_after;
    if (L.kind == 0) T2P_TRY(res_block(L, cur, i == 0 ? skip : nullptr, &nxt, B, s, res_lowp() ? first_norm_of(nextL, false) : NormHint()));
    else if (L.kind == 1) T2P_TRY(attn_block(L, cur, &nxt, B, s));
    else T2P_TRY(st_block(L, cur, &nxt, B, s));
    if (g_tap_index >= 0 && g_tap_counter++ == g_tap_index) {
      const long n = (long)B * nxt.H * nxt.W * nxt.C;
      g_tap_shape[0] = nxt.C; g_tap_shape[1] = nxt.H; g_tap_shape[2] = nxt.W; g_tap_shape[3] = nxt.lowp;
      float* dst = g_tap_dst;
      const long cap = g_tap_cap;
      g_tap_index = -1; g_tap_dst = nullptr; g_tap_cap = 0;      // one capture per arming: a later evaluation never writes to a buffer the caller may have freed
      T2P_REQUIRE(dst && n <= cap, "tap buffer too small");
      T2P_TRY(launch_widen(nxt.p, nxt.lowp ? dtype() : DT_F32, dst, n, s));
    }
    drop_pre_norm(cur);              // (only if this layer did not take it)
    if (own) free_act(cur);
    cur = nxt;
    own = true;
  }
  h = cur;
  return T2P_OK;
}

int Engine::set_context(const float* ctx, int B, int T, hipStream_t s) {
  T2P_REQUIRE(finalized_, "finalize the engine first");
  T2P_REQUIRE(ctx && B > 0 && T > 0, "set_context arguments");
  const int dt = dtype(), D = cfg_.context_dim;
  const size_t es = dtype_size(dt);
  const long Tpad = (long)round_up((size_t)T, 8);
  const bool realloc = (B != ctx_cap_B_ || T != ctx_cap_T_);   // (a weight refresh clears ctx_B_, not the buffers: they keep their addresses)
  const void* cx = ctx;
  void* conv = nullptr;
  PoolLease lease(pool_);                              // (the per-layer key / value caches are handed over with keep())
  if (dt != DT_F32) {
    conv = pool_.get((size_t)B * T * D * es);
    if (!conv) return T2P_ERR_HIP;
    T2P_TRY(launch_convert(ctx, conv, dt, (long)B * T * D, s));
    cx = conv;
  }
  auto each = [&](Layer& l) -> int {
    if (l.kind != 2) return T2P_OK;
    const int C = l.in_ch;
    if (realloc || !l.ctx_k) {
      pool_.put(l.ctx_k);
      pool_.put(l.ctx_vt);
      l.ctx_k = pool_.get((size_t)B * T * C * es);
      l.ctx_vt = pool_.get((size_t)B * C * Tpad * es);
      pool_.keep(l.ctx_k);
      pool_.keep(l.ctx_vt);
      if (!l.ctx_k || !l.ctx_vt) return T2P_ERR_HIP;
    }
    T2P_TRY(linear(cx, false, l.a2_k, (long)B * T, l.ctx_k, false, nullptr, 1.f, s, false));
    T2P_TRY(project_vt(dt, l.a2_v, cx, D, B, T, Tpad, l.ctx_vt, s));
    return T2P_OK;
  };
  for (Stage& st : arch_.input_stages) for (Layer& l : st.layers) T2P_TRY(each(l));
  for (Layer& l : arch_.mid_stage.layers) T2P_TRY(each(l));
  for (Stage& st : arch_.out_stages) for (Layer& l : st.layers) T2P_TRY(each(l));
  pool_.put(conv);
  ctx_B_ = ctx_cap_B_ = B; ctx_T_ = ctx_cap_T_ = T; ctx_Tpad_ = (int)Tpad;
  return T2P_OK;
}

// UNetModel.forward (ncsnpp.py:220-263)
int Engine::score(const float* x, const int* labels, const int* step_counter, float* out, int B, hipStream_t s,
                  const float* labels_f, const int* label_table, const float* label_f_table) {
  T2P_REQUIRE(finalized_, "finalize the engine first");
  T2P_REQUIRE(x && out && B > 0 && (labels || step_counter), "score arguments");
  const int L = cfg_.max_res_num, HW = L * L, Cx = cfg_.num_channels, N = cfg_.num_scales;
  const int R = labels ? B : 1;
  PoolLease lease(pool_);                              // whatever an early return below leaves checked out goes back to the pool
  g_tap_counter = 0;
  std::unique_ptr<LayerScope> pre_scope(new LayerScope("pre,pre," + std::to_string(L) + "," + std::to_string(Cx) + "," + std::to_string(arch_.nf), s));
  POOL_GET(emb, float*, (size_t)R * arch_.nf * 4);
  POOL_GET(t1, float*, (size_t)R * arch_.temb_dim * 4);
  POOL_GET(t2, float*, (size_t)R * arch_.temb_dim * 4);
  POOL_GET(tb, float*, (size_t)R * arch_.temb_total * 4);
  T2P_REQUIRE(!labels_f || labels, "fractional labels come with integer labels (sigma index)");
  T2P_REQUIRE(!label_table || (!labels && step_counter), "a label table goes with the device step counter");
  T2P_REQUIRE(!label_f_table || label_table, "the fractional label table goes with the integer one (sigma index)");
  T2P_TRY(launch_timestep_embedding(labels, labels_f, step_counter, emb, R, arch_.nf, s, label_table, N, label_f_table));
  T2P_TRY(launch_small_linear(emb, (const float*)pre0_.w, pre0_.b, t1, R, arch_.nf, arch_.temb_dim, 0, s));
  T2P_TRY(launch_small_linear(t1, (const float*)pre1_.w, pre1_.b, t2, R, arch_.temb_dim, arch_.temb_dim, 0, s));
  T2P_TRY(launch_small_linear(t2, (const float*)dense_all_.w, dense_all_.b, tb, R, arch_.temb_dim, arch_.temb_total, 1, s));
  tb_ = tb;
  tb_ld_ = labels ? arch_.temb_total : 0;
  POOL_GET(scale, float*, (size_t)B * 4);
  // without scale_by_sigma the same gather reads a table of ones: no host copy, nothing for the stream to wait on
  T2P_TRY(launch_gather_label(labels, step_counter, cfg_.scale_by_sigma ? inv_sigma_ : unit_scale_, scale, B, N, s, label_table));
  const bool hlp = res_lowp() && (Cx == 5 || Cx == 8) && pre_conv_direct_;   // the residual stream starts here
  POOL_GET(h0, float*, (size_t)B * HW * arch_.nf * (hlp ? dtype_size(dtype()) : 4));
  float* h0_stats = nullptr;
  if ((Cx == 5 || Cx == 8) && pre_conv_direct_) {
    // 16-bit modes: the GroupNorm column statistics of h0 (read by the first block and, through the skip stack, by the last
    // stage) come out of the input convolution instead of two passes over the tensor
    if (hlp && g_plan.fuse_gn_stats && pre_conv_fuses_col_stats(L, arch_.nf) && !(g_plan.gn_small && HW <= 64)) {
      h0_stats = (float*)pool_.get((size_t)B * (HW / 64) * arch_.nf * 2 * 4);
      if (!h0_stats) return T2P_ERR_HIP;
    }
    if (hlp && pre_conv_split_ && pre_conv_split_ok(dtype(), Cx, L, L, arch_.nf))
      T2P_TRY(launch_pre_conv_split(x, pre_conv_split_, pre_conv_.b, h0, dtype(), B, Cx, L, L, arch_.nf, s, h0_stats));
    else
      T2P_TRY(launch_pre_conv(x, pre_conv_direct_, pre_conv_.b, h0, hlp ? dtype() : DT_F32, B, Cx, L, L, arch_.nf, s, h0_stats));
  } else {
    POOL_GET(xin, float*, (size_t)B * HW * cpad_ * 4);
    T2P_TRY(launch_nchw_to_nhwc(x, xin, B, Cx, HW, cpad_, s));
    GemmParams p;   // pre_conv always in exact fp32: the input has the dynamic range of sigma_max
    p.dtype = DT_F32; p.a_f32 = 1; p.A0 = xin; p.C0 = cpad_; p.lda0 = cpad_;
    p.taps = 9; p.H = L; p.W = L;
    p.Bw = pre_conv_.w; p.ldb = pre_conv_.K; p.M = B * HW; p.N = arch_.nf; p.bias_n = pre_conv_.b;
    p.rows_per_batch = HW;
    p.C = h0; p.c_f32 = 1; p.ldc = arch_.nf;
    T2P_TRY(gemm(p, s));
    pool_.put(xin);
  }
  bool h0_lowp = hlp;
  if (res_lowp() && !hlp) {              // generic input-conv path: bring the stream to its storage type
    POOL_GET(h0c, float*, (size_t)B * HW * arch_.nf * dtype_size(dtype()));
    T2P_TRY(launch_convert(h0, h0c, dtype(), (long)B * HW * arch_.nf, s));
    pool_.put(h0);
    h0 = h0c;
    h0_lowp = true;
  }
  pool_.put(emb); pool_.put(t1); pool_.put(t2);
  pre_scope.reset();

  std::vector<Act> hs;
  Act h{h0, arch_.nf, L, L, h0_stats, h0_lowp};
  hs.push_back(h);
  for (size_t i = 0; i < arch_.input_stages.size(); ++i) {
    // the stage's last block may apply the first norm of the block that follows it (next input stage, or the mid stage)
    // (run_stage owns the pre-applied norm its input carries: the first block takes it, or it is dropped there)
    const Layer* next = i + 1 < arch_.input_stages.size() ? &arch_.input_stages[i + 1].layers[0] : &arch_.mid_stage.layers[0];
    T2P_TRY(run_stage(arch_.input_stages[i], h, nullptr, B, s, next));
    hs.push_back(h);
    hs.back().pre_norm = nullptr;      // the skip-stack copy does not own the pre-applied norm
  }
  // mid stage: its input stays on the skip stack
  T2P_TRY(run_stage(arch_.mid_stage, h, nullptr, B, s));
  for (Stage& st : arch_.out_stages) {
    Act skip = hs.back();
    hs.pop_back();
    T2P_REQUIRE(skip.C == st.skip_ch && skip.H == h.H, "skip stack mismatch");
    Act in = h;
    in.pre_norm = nullptr;
    T2P_TRY(run_stage(st, h, &skip, B, s));
    free_act(in);
    free_act(skip);
  }
  T2P_REQUIRE(hs.empty(), "skip stack not consumed");
  // head: GroupNorm -> SiLU -> conv3x3 (nf -> C), stored NCHW and divided by sigma[label]
  LayerScope head_scope("head,head," + std::to_string(L) + "," + std::to_string(arch_.final_ch) + "," + std::to_string(Cx), s);
  void* a = nullptr;
  {
    GemmParams p;
    p.dtype = dtype(); p.a_f32 = p.dtype == DT_F32; p.C0 = arch_.final_ch; p.lda0 = arch_.final_ch;
    p.taps = 9; p.H = L; p.W = L;
    p.Bw = head_conv_.w; p.ldb = head_conv_.K; p.M = B * HW; p.N = Cx; p.bias_n = head_conv_.b;
    p.rows_per_batch = HW;
    p.C = out; p.c_f32 = 1; p.c_nchw = 1; p.row_scale = scale;
    p.A0 = h.p;
    float* hstats = nullptr;
    if (h.lowp && h.cstats && HW % 64 == 0 && gemm_applies_a_norm(p)) {
      // GroupNorm + SiLU of the head inside the convolution's halo staging: the statistics come from the column sums of the last
      // block's epilogue (one small launch), the 134 - 268 MB normalised copy of the map is never written
      hstats = (float*)pool_.get((size_t)B * head_norm_.G * 2 * 4);
      if (!hstats) return T2P_ERR_HIP;
      T2P_TRY(launch_gn_finalize_cols(h.cstats, nullptr, h.C, 0, B, HW, head_norm_.G, 1e-6f, hstats, s));
      p.an_stats = hstats; p.an_gamma = head_norm_.gamma; p.an_beta = head_norm_.beta; p.an_groups = head_norm_.G; p.an_silu = 1;
      T2P_TRY(gemm(p, s));
      pool_.put(hstats);
      free_act(h);
    } else {
      T2P_TRY(group_norm(h, nullptr, head_norm_, 1e-6f, 1, 0, B, &a, s));
      free_act(h);
      p.A0 = a;
      T2P_TRY(gemm(p, s));
    }
  }
  pool_.put(a);
  pool_.put(scale);
  pool_.put(tb);
  tb_ = nullptr;
  return T2P_OK;
}

}  // namespace t2p
