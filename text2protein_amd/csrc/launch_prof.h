// Per-launch timing of the GEMM, convolution and fused-attention launches (bench.py roofline leg, t2p_profile_*): HIP events on
// the launch stream, collected between profile_begin and profile_end.
#pragma once
#include "t2p_common.h"

namespace t2p {

// kind 0 = 3x3 convolutions on the LDS-DMA kernels, 1 = other GEMMs, 2 = 3x3 convolutions on the register-staged / thin-output
// kernels, 3 = fused attention (reported by profile_attention)
struct ProfRec { hipEvent_t a = nullptr, b = nullptr; double flops = 0; int kind = 1; const char* name = nullptr; double bytes = 0; int M = 0, N = 0, K = 0, taps = 0, z = 0; };
inline void prof_shape(ProfRec& r, const GemmParams& p) {
  r.M = p.M; r.N = p.N; r.K = p.C0 + p.C1; r.taps = p.a_up ? -p.taps : p.taps; r.z = p.nz0 * p.nz1;
  if (p.CX0 + p.CX1) r.K = r.K * 1000000 + p.CX0 + p.CX1;      // shortcut segment: printed as K+KX
}

void profile_begin();
int profile_end(double out[3][3]);
int profile_dominant(double out[4], const char** name);
int profile_shapes(char* buf, int len);
int profile_conv_kernels(char* buf, int len);
int profile_attention(double out[3]);
bool prof_on();

// One timed launch.  Inside a profiled region (on()) the launcher fills `rec`; open() creates the two events and records the first on
// the stream, close() records the second, commit() hands the record to the registry.  close and commit are separate calls: a launcher
// may time its main kernel only and commit after the work that follows it.  Outside a region every call returns without a HIP call.
// The events of a scope that is never committed (an error return in between) are destroyed with it.
class ProfScope {
 public:
  ProfRec rec;
  ProfScope() : on_(prof_on()) {}
  ~ProfScope();
  ProfScope(const ProfScope&) = delete;
  ProfScope& operator=(const ProfScope&) = delete;
  bool on() const { return on_; }
  int open(hipStream_t stream);
  int close();
  void commit();

 private:
  const bool on_;
  hipStream_t stream_ = nullptr;
};

}  // namespace t2p
