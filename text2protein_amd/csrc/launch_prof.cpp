// The launch-profiling registry behind t2p_profile_* and the scope the launchers time a launch with (launch_prof.h).
#include <array>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "launch_prof.h"

namespace t2p {

// ---- optional per-launch timing (bench.py roofline leg): HIP events on the launch stream -----------
static bool g_prof_on = false;
static std::vector<ProfRec> g_prof;
// the 3x3-convolution instantiation with the largest total time of the last profiled region
static std::string g_dom_name;
static double g_dom[4] = {0, 0, 0, 0};

// fused-attention launches of the profiled region (attention.hip: records of kind 3)
static std::vector<ProfRec> g_prof_attn;
static double g_attn[3] = {0, 0, 0};
bool prof_on() { return g_prof_on; }
int profile_attention(double out[3]) {
  out[0] = g_attn[0]; out[1] = g_attn[1]; out[2] = g_attn[2];
  return T2P_OK;
}

static std::map<std::string, std::array<double, 3>> g_shapes;    // "kind,M,N,K,taps,z" -> {launches, ms, flops} of the last region
// the launches of the region closed by the last profile_end, one line per operand shape:
// kind,M,N,K,taps (negative: gathered from the half-resolution map),batch,launches,ms,flops
int profile_shapes(char* buf, int len) {
  std::string t = "kind,M,N,K,taps,batch,launches,ms,flops\n";
  for (auto& kv : g_shapes) {
    char line[256];
    std::snprintf(line, sizeof line, "%s,%.0f,%.4f,%.6g\n", kv.first.c_str(), kv.second[0], kv.second[1], kv.second[2]);
    t += line;
  }
  if ((int)t.size() + 1 > len) { set_last_error("profile_shapes: buffer too small"); return T2P_ERR_INVALID; }
  std::memcpy(buf, t.c_str(), t.size() + 1);
  return T2P_OK;
}
// the 3x3-convolution launches of the last region on the LDS-DMA kernels, one line per (instantiation, operand shape):
// kernel;M;N;K;launches  (the kernel name as profile_dominant prints it; it holds commas, hence the semicolons)
static std::map<std::string, int> g_conv_kernels;
int profile_conv_kernels(char* buf, int len) {
  std::string t = "kernel;M;N;K;launches\n";
  for (auto& kv : g_conv_kernels) t += kv.first + ";" + std::to_string(kv.second) + "\n";
  if ((int)t.size() + 1 > len) { set_last_error("profile_conv_kernels: buffer too small"); return T2P_ERR_INVALID; }
  std::memcpy(buf, t.c_str(), t.size() + 1);
  return T2P_OK;
}
void profile_begin() {
  for (ProfRec& r : g_prof_attn) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
  g_prof_attn.clear();
  for (ProfRec& r : g_prof) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
  g_prof.clear();
  g_prof_on = true;
}
// out[kind][0..2] = {milliseconds, flops, launches}; kind 0 = 3x3 convolutions on the LDS-DMA
// kernel (the dominant kernel), 1 = other GEMMs, 2 = 3x3 convolutions on the register-staged kernel
// (pre_conv in fp32, the 5-channel head, tiny maps)
int profile_end(double out[3][3]) {
  g_prof_on = false;
  for (int k = 0; k < 3; ++k) out[k][0] = out[k][1] = out[k][2] = 0;
  std::map<std::string, std::array<double, 4>> per;
  g_shapes.clear();
  g_conv_kernels.clear();
  for (ProfRec& r : g_prof) {
    T2P_HIP_CHECK(hipEventSynchronize(r.b));
    float ms = 0.f;
    T2P_HIP_CHECK(hipEventElapsedTime(&ms, r.a, r.b));
    out[r.kind][0] += ms; out[r.kind][1] += r.flops; out[r.kind][2] += 1;
    {
      char key[128];
      if (r.K >= 1000000) std::snprintf(key, sizeof key, "%d,%d,%d,%d+%d,%d,%d", r.kind, r.M, r.N, r.K / 1000000, r.K % 1000000, r.taps, r.z);
      else std::snprintf(key, sizeof key, "%d,%d,%d,%d,%d,%d", r.kind, r.M, r.N, r.K, r.taps, r.z);
      auto& e = g_shapes[key];
      e[0] += 1; e[1] += ms; e[2] += r.flops;
    }
    if (r.kind == 0 && r.name) {
      auto& e = per[r.name];
      e[0] += ms; e[1] += r.flops; e[2] += 1; e[3] += r.bytes;
      g_conv_kernels[std::string(r.name) + ";" + std::to_string(r.M) + ";" + std::to_string(r.N) + ";" + std::to_string(r.K)] += 1;
    }
    (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b);
  }
  g_prof.clear();
  g_attn[0] = g_attn[1] = g_attn[2] = 0;
  for (ProfRec& r : g_prof_attn) {
    T2P_HIP_CHECK(hipEventSynchronize(r.b));
    float ms = 0.f;
    T2P_HIP_CHECK(hipEventElapsedTime(&ms, r.a, r.b));
    g_attn[0] += ms; g_attn[1] += r.flops; g_attn[2] += 1;
    (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b);
  }
  g_prof_attn.clear();
  g_dom_name.clear();
  g_dom[0] = g_dom[1] = g_dom[2] = g_dom[3] = 0;
  for (auto& kv : per)
    if (kv.second[0] > g_dom[0]) { g_dom_name = kv.first; for (int i = 0; i < 4; ++i) g_dom[i] = kv.second[i]; }
  return T2P_OK;
}

// {milliseconds, flops, launches, algorithmic bytes} and the kernel name (as rocprofv3 prints it, without the
// argument list) of the dominant 3x3-convolution instantiation of the region closed by the last profile_end.
// Algorithmic bytes of a launch: every input element, weight, residual element once + the output once.
int profile_dominant(double out[4], const char** name) {
  out[0] = g_dom[0]; out[1] = g_dom[1]; out[2] = g_dom[2]; out[3] = g_dom[3];
  *name = g_dom_name.c_str();
  return T2P_OK;
}

int ProfScope::open(hipStream_t stream) {
  if (!on_) return T2P_OK;
  stream_ = stream;
  T2P_HIP_CHECK(hipEventCreate(&rec.a));
  T2P_HIP_CHECK(hipEventCreate(&rec.b));
  T2P_HIP_CHECK(hipEventRecord(rec.a, stream));
  return T2P_OK;
}
int ProfScope::close() {
  if (!on_) return T2P_OK;
  T2P_HIP_CHECK(hipEventRecord(rec.b, stream_));
  return T2P_OK;
}
void ProfScope::commit() {
  if (!on_) return;
  (rec.kind == 3 ? g_prof_attn : g_prof).push_back(rec);
  rec.a = rec.b = nullptr;                              // the registry destroys them (profile_end / profile_begin)
}
ProfScope::~ProfScope() {
  if (rec.a) (void)hipEventDestroy(rec.a);
  if (rec.b) (void)hipEventDestroy(rec.b);
}

}  // namespace t2p
