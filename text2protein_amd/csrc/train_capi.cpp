// extern "C" surface of the training step (declarations and reference citations: include/t2p.h, "training step").
#include <algorithm>
#include <new>

#include "train.h"

using namespace t2p;

#define API_BEGIN try {
#define API_END                                        \
  }                                                    \
  catch (const std::bad_alloc&) {                      \
    set_last_error("out of host memory");              \
    return T2P_ERR_STATE;                              \
  }                                                    \
  catch (const std::exception& e) {                    \
    set_last_error(std::string("exception: ") + e.what()); \
    return T2P_ERR_STATE;                              \
  }

// the arguments of t2p_op_tgemm / t2p_op_tgemm16 (include/t2p.h) as the launchers take them
static TGemmArgs op_tgemm_args(const float* A, int64_t sAm, int64_t sAk, const float* B, int64_t sBk, int64_t sBn, float* C, int64_t ldc, int M,
                               int N, int K, int nz, int64_t sAz, int64_t sBz, int64_t sCz, float alpha, float beta, const float* bias_n,
                               int ksplit, int conv, int H, int W, int conv_C) {
  TGemmArgs a;
  a.A = A; a.sAm = sAm; a.sAk = sAk; a.sAz0 = sAz;
  a.B = B; a.sBk = sBk; a.sBn = sBn; a.sBz0 = sBz;
  a.C = C; a.ldc = ldc; a.sCz0 = sCz; a.M = M; a.N = N; a.K = K; a.nz0 = nz; a.nz1 = 1;
  a.alpha = alpha; a.beta = beta; a.bias_n = bias_n; a.ksplit = ksplit;
  if (conv) { a.conv_b = 1; a.H = H; a.W = W; a.conv_C = conv_C; a.ldx = sBz; a.sBz0 = 0; }
  return a;
}

extern "C" {

int t2p_train_create(const t2p_model_config* model, const t2p_train_config* train, t2p_trainer** out) {
  API_BEGIN
  T2P_REQUIRE(model && train && out, "null argument");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    set_last_error("no HIP device: the training step has no CPU fallback");
    return T2P_ERR_HIP;
  }
  t2p_trainer* t = new t2p_trainer(*model, *train);
  const int rc = t->impl.build();
  if (rc != T2P_OK) {
    delete t;
    return rc;
  }
  *out = t;
  return T2P_OK;
  API_END
}

void t2p_train_destroy(t2p_trainer* t) { delete t; }

int t2p_train_num_params(const t2p_trainer* t) { return t ? (int)t->impl.params().size() : -1; }

int t2p_train_param_info(const t2p_trainer* t, int i, const char** name, int64_t shape[4], int* ndim) {
  API_BEGIN
  T2P_REQUIRE(t && name && shape && ndim && i >= 0 && i < (int)t->impl.params().size(), "param_info arguments");
  const TParam& p = t->impl.params()[i];
  *name = p.name.c_str();
  *ndim = (int)p.shape.size();
  for (int d = 0; d < 4; ++d) shape[d] = d < *ndim ? p.shape[d] : 1;
  return T2P_OK;
  API_END
}

int t2p_train_load_param(t2p_trainer* t, const char* name, const float* host_data, const int64_t* shape, int ndim) {
  API_BEGIN
  T2P_REQUIRE(t, "null trainer");
  return t->impl.load_param(name, host_data, shape, ndim);
  API_END
}

int t2p_train_read(t2p_trainer* t, int which, const char* name, float* host_out) {
  API_BEGIN
  T2P_REQUIRE(t, "null trainer");
  return t->impl.read_tensor(which, name, host_out);
  API_END
}

int t2p_train_write(t2p_trainer* t, int which, const char* name, const float* host_in) {
  API_BEGIN
  T2P_REQUIRE(t, "null trainer");
  return t->impl.write_tensor(which, name, host_in);
  API_END
}

int t2p_train_set_step(t2p_trainer* t, int64_t step, int64_t adam_updates, int64_t ema_updates) {
  API_BEGIN
  T2P_REQUIRE(t, "null trainer");
  return t->impl.set_step(step, adam_updates, ema_updates);
  API_END
}

int t2p_train_get_step(const t2p_trainer* t, int64_t out3[3]) {
  API_BEGIN
  T2P_REQUIRE(t && out3, "get_step arguments");
  return t->impl.get_step(out3);
  API_END
}

int t2p_train_set_sde(t2p_trainer* t, int sde, double beta_min, double beta_max, const float* std_table) {
  API_BEGIN
  T2P_REQUIRE(t, "null trainer");
  return t->impl.set_sde(sde, beta_min, beta_max, std_table);
  API_END
}

int t2p_train_set_ploss(t2p_trainer* t, int loss_type, int timesteps, const float* sqrt_alphas_cumprod,
                        const float* sqrt_one_minus_alphas_cumprod) {
  API_BEGIN
  T2P_REQUIRE(t, "null trainer");
  return t->impl.set_ploss(loss_type, timesteps, sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod);
  API_END
}

int t2p_train_set_dropout_masks(t2p_trainer* t, const uint8_t* const* device_masks, int n) {
  API_BEGIN
  T2P_REQUIRE(t && n >= 0, "set_dropout_masks arguments");
  return t->impl.set_dropout_masks(device_masks, n);
  API_END
}

int t2p_train_set_ss_blocks(t2p_trainer* t, const int32_t* host_blocks, int n, const uint8_t* host_drop, double p) {
  API_BEGIN
  T2P_REQUIRE(t, "null trainer");
  return t->impl.set_ss_blocks(host_blocks, n, host_drop, p);
  API_END
}

int t2p_train_set_inpaint_draw(t2p_trainer* t, const int32_t* host_len_lo_hi, int B, double random_p, double contiguous_p) {
  API_BEGIN
  T2P_REQUIRE(t, "null trainer");
  return t->impl.set_inpaint_draw(host_len_lo_hi, B, random_p, contiguous_p);
  API_END
}

int t2p_train_set_context_drop(t2p_trainer* t, const uint8_t* host_drop, int B, double p) {
  API_BEGIN
  T2P_REQUIRE(t, "null trainer");
  return t->impl.set_context_drop(host_drop, B, p);
  API_END
}

int t2p_train_loss(t2p_trainer* t, const t2p_train_batch* batch, int backward, float* loss_host, float* score_out, void* stream) {
  API_BEGIN
  T2P_REQUIRE(t && batch, "null argument");
  return t->impl.loss(*batch, backward != 0, false, loss_host, score_out, (hipStream_t)stream);
  API_END
}

int t2p_train_step(t2p_trainer* t, const t2p_train_batch* batch, float* loss_host, void* stream) {
  API_BEGIN
  T2P_REQUIRE(t && batch, "null argument");
  return t->impl.step(*batch, loss_host, (hipStream_t)stream);
  API_END
}

int t2p_train_apply(t2p_trainer* t, void* stream) {
  API_BEGIN
  T2P_REQUIRE(t, "null trainer");
  return t->impl.apply((hipStream_t)stream);
  API_END
}

int t2p_train_grad_buffer(t2p_trainer* t, float** device_ptr, int64_t* n) {
  API_BEGIN
  T2P_REQUIRE(t && device_ptr && n, "grad_buffer arguments");
  *device_ptr = t->impl.grad_buffer();
  *n = (int64_t)t->impl.num_elements();
  return T2P_OK;
  API_END
}

int t2p_train_buffer(t2p_trainer* t, int which, float** device_ptr, int64_t* n) {
  API_BEGIN
  T2P_REQUIRE(t, "null trainer");
  return t->impl.buffer(which, device_ptr, n);
  API_END
}

int t2p_train_copy(t2p_trainer* t, int dst, int src, void* stream) {
  API_BEGIN
  T2P_REQUIRE(t, "null trainer");
  return t->impl.copy(dst, src, (hipStream_t)stream);
  API_END
}

// t2p_train_buffer + t2p_engine_load_flat; every mismatch is refused before anything is written
int t2p_engine_load_from_trainer(t2p_engine* e, t2p_trainer* t, int which, void* stream) {
  API_BEGIN
  T2P_REQUIRE(e && t, "null argument");
  T2P_REQUIRE(which == 0 || which == 2, "load_from_trainer: which is 0 (parameters) or 2 (EMA shadow), got " + std::to_string(which));
  const auto& ep = e->impl.params();
  const auto& tp = t->impl.params();
  T2P_REQUIRE(ep.size() == tp.size(), "load_from_trainer: the trainer has " + std::to_string(tp.size()) + " parameter tensors, the engine " +
                                          std::to_string(ep.size()));
  for (size_t i = 0; i < ep.size(); ++i) {
    T2P_REQUIRE(ep[i].name == tp[i].name, "load_from_trainer: parameter " + std::to_string(i) + " is " + tp[i].name + " in the trainer, " +
                                              ep[i].name + " in the engine");
    T2P_REQUIRE(ep[i].shape == tp[i].shape, "load_from_trainer: the shape of " + ep[i].name + " differs between the trainer and the engine");
  }
  T2P_REQUIRE(e->impl.device() == t->impl.device(), "load_from_trainer: the trainer lives on device " + std::to_string(t->impl.device()) +
                                                        ", the engine on device " + std::to_string(e->impl.device()));
  float* p = nullptr;
  int64_t n = 0;
  T2P_TRY(t->impl.buffer(which, &p, &n));
  return e->impl.load_flat(p, n, (hipStream_t)stream);
  API_END
}

int t2p_train_eval_loss(t2p_trainer* t, const t2p_train_batch* batch, float* loss_host, void* stream) {
  API_BEGIN
  T2P_REQUIRE(t && batch, "null argument");
  return t->impl.loss(*batch, false, true, loss_host, nullptr, (hipStream_t)stream);
  API_END
}

int64_t t2p_train_device_bytes(const t2p_trainer* t) { return t ? t->impl.device_bytes() : -1; }

int t2p_op_tgemm(const float* A, int64_t sAm, int64_t sAk, const float* B, int64_t sBk, int64_t sBn, float* C, int64_t ldc, int M, int N,
                 int K, int nz, int64_t sAz, int64_t sBz, int64_t sCz, float alpha, float beta, const float* bias_n, int ksplit, int conv,
                 int H, int W, int conv_C, void* stream) {
  API_BEGIN
  return launch_tgemm(op_tgemm_args(A, sAm, sAk, B, sBk, sBn, C, ldc, M, N, K, nz, sAz, sBz, sCz, alpha, beta, bias_n, ksplit, conv, H, W, conv_C),
                      (hipStream_t)stream);
  API_END
}

int t2p_op_tgemm16(int dtype, const float* A, int64_t sAm, int64_t sAk, const float* B, int64_t sBk, int64_t sBn, float* C, int64_t ldc,
                   int M, int N, int K, int nz, int64_t sAz, int64_t sBz, int64_t sCz, float alpha, float beta, const float* bias_n, int ksplit,
                   int conv, int H, int W, int conv_C, void* stream) {
  API_BEGIN
  const TGemmArgs a = op_tgemm_args(A, sAm, sAk, B, sBk, sBn, C, ldc, M, N, K, nz, sAz, sBz, sCz, alpha, beta, bias_n, ksplit, conv, H, W, conv_C);
  T2P_REQUIRE(M > 0 && N > 0 && K > 0 && nz >= 1 && ksplit >= 0, "tgemm16 shapes");
  hipStream_t s = (hipStream_t)stream;
  const long n = tgemm16_ws_floats(a);
  float* ws = nullptr;
  if (n > 0) T2P_HIP_CHECK(hipMalloc(&ws, (size_t)n * 4));
  int rc = launch_tgemm16(a, dtype, ws, s);
  if (ws) {
    (void)hipStreamSynchronize(s);
    (void)hipFree(ws);
  }
  return rc;
  API_END
}

// scratch of one operator call: hipMalloc blocks, all held until the call ends (put is a no-op), then freed after the stream has drained --
// whichever way the call ends
struct OpScratch {
  explicit OpScratch(hipStream_t stream) : s(stream) {}
  ~OpScratch() {
    if (blocks.empty()) return;
    (void)hipStreamSynchronize(s);
    for (void* p : blocks) (void)hipFree(p);
  }
  OpScratch(const OpScratch&) = delete;
  OpScratch& operator=(const OpScratch&) = delete;
  void* get(size_t bytes) {
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, std::max(bytes, (size_t)16));
    if (e != hipSuccess) {
      set_last_error(std::string("operator scratch: hipMalloc: ") + hipGetErrorString(e));
      return nullptr;
    }
    blocks.push_back(p);
    return p;
  }
  hipStream_t s;
  std::vector<void*> blocks;
};

int t2p_op_train_conv3x3(int dtype, const float* x, const float* w, const float* bias, const float* tbias, int batch, int H, int W, int Ci,
                         int Co, int Cip, int Cop, float* y, const float* dy, float* dx, float* dw, float* dbias, float* dtbias,
                         int fixed_order, void* stream) {
  API_BEGIN
  T2P_REQUIRE(dtype == DT_F32 || dtype == DT_BF16 || dtype == DT_F16, "train_conv3x3: dtype is 0 (f32), 1 (bf16) or 2 (f16)");
  T2P_REQUIRE(x && w && bias && y && batch > 0 && H > 0 && W > 0 && Ci > 0 && Co > 0, "train_conv3x3 arguments");
  const int vec = dtype == DT_F32 ? 4 : 8;
  T2P_REQUIRE(Cip >= Ci && Cop >= Co && Cip % vec == 0 && Cop % vec == 0, "train_conv3x3: Cip / Cop pad Ci / Co to the kernels' vector width");
  T2P_REQUIRE(!tbias || Cop == Co, "train_conv3x3: the time-embedding bias needs Cop == Co");
  T2P_REQUIRE(!dy || (dw && dbias && (dtbias != nullptr) == (tbias != nullptr)), "train_conv3x3: the backward takes dw, dbias and (with tbias) dtbias");
  T2P_REQUIRE((long)batch * H * W < (1L << 31), "train_conv3x3: rows");
  hipStream_t s = (hipStream_t)stream;
  OpScratch mem(s);
  ConvScratch sc;
  sc.get = [&mem](size_t bytes) { return mem.get(bytes); };
  sc.put = [](void*) {};
  const bool need_dx = dy && dx;
  const size_t nf = (size_t)Co * 9 * Cip, nd = (size_t)Ci * 9 * Cop;
  ConvW c;
  c.Co = Co; c.Ci = Ci; c.Cip = Cip; c.Cop = Cop;
  float* wf = (float*)mem.get(nf * 4);
  float* wd = need_dx ? (float*)mem.get(nd * 4) : nullptr;            // (the network input's convolution has none either)
  if (!wf || (need_dx && !wd)) return T2P_ERR_HIP;
  T2P_TRY(launch_conv_w_prep(w, wf, wd, Co, Ci, Cip, Cop, s));
  c.wf = wf; c.wd = wd;
  if (dtype != DT_F32) {
    void* wf16 = mem.get(nf * 2);
    void* wd16 = need_dx ? mem.get(nd * 2) : nullptr;
    if (!wf16 || (need_dx && !wd16)) return T2P_ERR_HIP;
    T2P_TRY(launch_convert(wf, wf16, dtype, (long)nf, s));
    if (need_dx) T2P_TRY(launch_convert(wd, wd16, dtype, (long)nd, s));
    c.wf16 = wf16; c.wd16 = wd16;
  }
  T2P_TRY(train_conv3x3_forward(dtype, c, x, batch, H, W, bias, tbias, y, sc, s));
  if (!dy) return T2P_OK;
  float* dwc = (float*)mem.get(nf * 4);
  if (!dwc) return T2P_ERR_HIP;
  return train_conv3x3_backward(dtype, fixed_order != 0, c, x, dy, batch, H, W, dx, dwc, dw, dbias, dtbias, sc, s);
  API_END
}

// block_dropout alone, through the two kernels of the training pass: the residue flags, then dsm_perturb with an all-false pair mask
// (every element takes the select's fallback branch, perturbed = the dropped x)
int t2p_op_ss_block_dropout(const float* x, float* out, int batch, int C, int L, const int32_t* host_blocks, int n, const uint8_t* host_drop,
                            double p, uint64_t seed, uint64_t stream_id, uint8_t* drop_out_device, void* stream) {
  API_BEGIN
  T2P_REQUIRE(x && out && batch > 0 && L > 0 && n >= 0 && (n == 0 || host_blocks), "ss_block_dropout arguments");
  T2P_REQUIRE(C >= 7, "ss_block_dropout: channels 4:7 need the 8-channel layout (C >= 7)");
  T2P_REQUIRE(p >= 0.0 && p <= 1.0, "ss_block_dropout: the dropout probability must lie in [0, 1]");
  for (int k = 0; k < n; ++k) {
    const int32_t* b = host_blocks + 3 * k;
    T2P_REQUIRE(b[0] >= 0 && b[0] < batch, "ss_block_dropout: block " + std::to_string(k) + " names a sample outside the batch");
    T2P_REQUIRE(b[1] >= 0 && b[2] >= 0, "ss_block_dropout: block " + std::to_string(k) + " has a negative start or end");
  }
  hipStream_t s = (hipStream_t)stream;
  const size_t HW = (size_t)L * L, nx = (size_t)batch * C * HW;
  if (n == 0) {
    if (out != x) T2P_HIP_CHECK(hipMemcpyAsync(out, x, nx * 4, hipMemcpyDeviceToDevice, s));
    return T2P_OK;
  }
  // one scratch allocation: a copy of x when out aliases it (the kernel's pointers are __restrict__: it never runs in place), [std |
  // num_elem] floats, blocks, then the byte tables (pair mask = 0, rows, decisions, the mask output)
  const size_t o_std = out == x ? nx * 4 : 0, o_blocks = o_std + (size_t)batch * 8, o_pair = o_blocks + (size_t)n * 12, o_rows = o_pair + batch * HW,
               o_drop = o_rows + (size_t)batch * L, o_mask = o_drop + n, total = o_mask + nx;
  char* ws = nullptr;
  T2P_HIP_CHECK(hipMalloc(&ws, total));
  int rc = T2P_OK;
  hipError_t e = hipMemsetAsync(ws + o_std, 0, o_rows - o_std, s);       // std = 0, pair mask = all false
  const float* src = x;
  if (e == hipSuccess && out == x) {
    e = hipMemcpyAsync(ws, x, nx * 4, hipMemcpyDeviceToDevice, s);
    src = (const float*)ws;
  }
  if (e == hipSuccess) e = hipMemcpyAsync(ws + o_blocks, host_blocks, (size_t)n * 12, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && host_drop) e = hipMemcpyAsync(ws + o_drop, host_drop, (size_t)n, hipMemcpyHostToDevice, s);
  if (e != hipSuccess) {
    set_last_error(std::string("ss_block_dropout: ") + hipGetErrorString(e));
    rc = T2P_ERR_HIP;
  }
  if (rc == T2P_OK)
    rc = launch_ss_block_rows((const int*)(ws + o_blocks), n, host_drop ? (const unsigned char*)(ws + o_drop) : nullptr, (float)p, seed, stream_id,
                              batch, L, (unsigned char*)(ws + o_rows), drop_out_device, s);
  if (rc == T2P_OK)                                                      // z is never read (the mask is false everywhere): any valid buffer
    rc = launch_dsm_perturb(src, src, (const float*)(ws + o_std), nullptr, (const unsigned char*)(ws + o_pair), nullptr, 0, batch, C, L, out,
                            (unsigned char*)(ws + o_mask), (float*)(ws + o_std) + batch, s, (const unsigned char*)(ws + o_rows));
  (void)hipStreamSynchronize(s);                                         // host_blocks / host_drop and the scratch are free after the call
  (void)hipFree(ws);
  return rc;
  API_END
}

// context dropout alone, through the two kernels of the training pass: the decisions (given or drawn), then the row zeroing in place
int t2p_op_context_drop(float* x, int batch, int64_t row_floats, const uint8_t* host_drop, double p, uint64_t seed, uint64_t stream_id,
                        uint8_t* drop_out_device, void* stream) {
  API_BEGIN
  T2P_REQUIRE(x && batch > 0 && batch <= 65535 && row_floats > 0, "context_drop arguments");
  T2P_REQUIRE(row_floats % 4 == 0, "context_drop: row_floats must be a multiple of 4 (16-byte stores)");
  T2P_REQUIRE(((uintptr_t)x & 15) == 0, "context_drop: x must be 16-byte aligned");
  T2P_REQUIRE(p >= 0.0 && p <= 1.0, "context_drop: the dropout probability must lie in [0, 1]");
  hipStream_t s = (hipStream_t)stream;
  unsigned char* drop = nullptr;
  T2P_HIP_CHECK(hipMalloc(&drop, (size_t)batch));
  int rc = T2P_OK;
  hipError_t e = hipSuccess;
  if (host_drop) e = hipMemcpyAsync(drop, host_drop, (size_t)batch, hipMemcpyHostToDevice, s);
  else rc = launch_context_drop_draw(batch, (float)p, seed, stream_id, drop, s);
  if (rc == T2P_OK && e == hipSuccess) rc = launch_zero_sample_rows(x, nullptr, batch, (long)row_floats, drop, s);
  if (rc == T2P_OK && e == hipSuccess && drop_out_device) e = hipMemcpyAsync(drop_out_device, drop, (size_t)batch, hipMemcpyDeviceToDevice, s);
  const hipError_t e2 = hipStreamSynchronize(s);                         // host_drop and the scratch are free after the call
  (void)hipFree(drop);
  if (rc != T2P_OK) return rc;
  if (e != hipSuccess || e2 != hipSuccess) {
    set_last_error(std::string("context_drop: ") + hipGetErrorString(e != hipSuccess ? e : e2));
    return T2P_ERR_HIP;
  }
  return T2P_OK;
  API_END
}

// the integer timesteps of the p_loss objective alone, through the device function of the training pass
int t2p_op_ploss_draw_t(uint64_t seed, uint64_t stream_id, int B, int timesteps, int32_t* out_dev, void* stream) {
  API_BEGIN
  T2P_REQUIRE(out_dev && B > 0, "ploss_draw_t arguments");
  T2P_REQUIRE(timesteps >= 1 && timesteps <= (1 << 24), "ploss_draw_t: timesteps must lie in [1, 2^24]");
  return launch_ploss_draw_t(B, timesteps, seed, stream_id, out_dev, (hipStream_t)stream);
  API_END
}

// random_mask_batch's draw alone, through the kernel of the training pass.  Drawn into scratch and copied out after the kernel completed, so
// a call that fails leaves flags_out / pair_out / mode_out_host as they were
int t2p_op_inpaint_mask_draw(const int32_t* host_len_lo_hi, int B, int L, double random_p, double contiguous_p, uint64_t seed, uint64_t stream_id,
                             int force_mode, uint8_t* flags_out, uint8_t* pair_out, int* mode_out_host, void* stream) {
  API_BEGIN
  T2P_REQUIRE(host_len_lo_hi && B > 0 && B <= 65535 && L > 0 && flags_out && pair_out, "inpaint_mask_draw arguments");
  T2P_REQUIRE(L <= 256, "inpaint_mask_draw: the device draw counts ranks in LDS, L <= 256");
  T2P_REQUIRE(force_mode >= -1 && force_mode <= 2, "inpaint_mask_draw: force_mode is -1 (drawn), 0 (none), 1 (random) or 2 (contiguous)");
  T2P_TRY(check_inpaint_draw("inpaint_mask_draw", host_len_lo_hi, B, L, random_p, contiguous_p));
  hipStream_t s = (hipStream_t)stream;
  const size_t n_flags = (size_t)B * L, n_pair = n_flags * L, o_flags = 16, o_pair = o_flags + ((n_flags + 15) & ~(size_t)15),
               o_llh = o_pair + ((n_pair + 15) & ~(size_t)15), total = o_llh + (size_t)B * 12;     // [mode | flags | pair | (l, lo, hi)]
  char* ws = nullptr;
  T2P_HIP_CHECK(hipMalloc(&ws, total));
  int rc = T2P_OK, mode = -1;
  hipError_t e = hipMemcpyAsync(ws + o_llh, host_len_lo_hi, (size_t)B * 12, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) {
    rc = launch_inpaint_mask_draw((const int*)(ws + o_llh), B, L, (float)random_p, (float)(1.0 - contiguous_p), seed, stream_id, force_mode,
                                  (unsigned char*)(ws + o_flags), (unsigned char*)(ws + o_pair), (int*)ws, s);
    if (rc == T2P_OK) e = hipMemcpyAsync(&mode, ws, 4, hipMemcpyDeviceToHost, s);
    if (rc == T2P_OK && e == hipSuccess) e = hipStreamSynchronize(s);
    if (rc == T2P_OK && e == hipSuccess) e = hipMemcpyAsync(flags_out, ws + o_flags, n_flags, hipMemcpyDeviceToDevice, s);
    if (rc == T2P_OK && e == hipSuccess) e = hipMemcpyAsync(pair_out, ws + o_pair, n_pair, hipMemcpyDeviceToDevice, s);
  }
  const hipError_t e2 = hipStreamSynchronize(s);                         // host_len_lo_hi and the scratch are free after the call
  (void)hipFree(ws);
  if (rc != T2P_OK) return rc;
  if (e != hipSuccess || e2 != hipSuccess) {
    set_last_error(std::string("inpaint_mask_draw: ") + hipGetErrorString(e != hipSuccess ? e : e2));
    return T2P_ERR_HIP;
  }
  if (mode_out_host) *mode_out_host = mode;
  return T2P_OK;
  API_END
}

// the op-level backward entry points take eps and recompute the forward statistics themselves (tests hold no engine state)
static int op_groupnorm_backward(const float* x, const float* dy, const float* gamma, const float* beta, int silu, int batch, int HW, int C,
                                 int groups, float eps, float* dx, float* dgamma, float* dbeta, bool fixed_order, hipStream_t s) {
  T2P_REQUIRE(x && dy && gamma && beta && dx && dgamma && dbeta && batch > 0 && HW > 0 && C > 0 && groups > 0 && C % groups == 0, "groupnorm_backward arguments");
  float *stats = nullptr, *partial = nullptr, *ws = nullptr;
  const int nparts = gn_num_chunks(HW) * ((C + 1023) / 1024);
  int rc = T2P_OK;
  hipError_t e = hipMalloc(&stats, (size_t)batch * groups * 2 * 4);
  if (e == hipSuccess) e = hipMalloc(&partial, (size_t)batch * nparts * groups * 2 * 4);
  if (e == hipSuccess) e = hipMalloc(&ws, (size_t)gn_bwd_ws_floats(batch, HW, C, groups) * 4);
  if (e != hipSuccess) {
    set_last_error(std::string("groupnorm_backward: hipMalloc: ") + hipGetErrorString(e));
    rc = T2P_ERR_HIP;
  }
  GroupNormArgs a;
  a.x0 = x; a.C0 = C; a.B = batch; a.HW = HW; a.G = groups; a.eps = eps; a.partial = partial; a.stats = stats;
  if (rc == T2P_OK) rc = launch_gn_stats(a, s);
  if (rc == T2P_OK) rc = launch_gn_backward(x, dy, stats, gamma, beta, silu, batch, HW, C, groups, dx, dgamma, dbeta, ws, fixed_order, s);
  (void)hipStreamSynchronize(s);
  (void)hipFree(stats); (void)hipFree(partial); (void)hipFree(ws);   // hipFree(nullptr) is a no-op: one cleanup path, whichever step failed
  return rc;
}

int t2p_op_groupnorm_backward(const float* x, const float* dy, const float* gamma, const float* beta, int silu, int batch, int HW, int C,
                              int groups, float eps, float* dx, float* dgamma, float* dbeta, void* stream) {
  API_BEGIN
  return op_groupnorm_backward(x, dy, gamma, beta, silu, batch, HW, C, groups, eps, dx, dgamma, dbeta, false, (hipStream_t)stream);
  API_END
}

int t2p_op_groupnorm_backward_form(const float* x, const float* dy, const float* gamma, const float* beta, int silu, int batch, int HW, int C,
                                   int groups, float eps, float* dx, float* dgamma, float* dbeta, int fixed_order, void* stream) {
  API_BEGIN
  return op_groupnorm_backward(x, dy, gamma, beta, silu, batch, HW, C, groups, eps, dx, dgamma, dbeta, fixed_order != 0, (hipStream_t)stream);
  API_END
}

int t2p_op_layernorm_backward(const float* x, const float* dy, const float* gamma, int64_t rows, int C, float eps, float* dx, float* dgamma,
                              float* dbeta, void* stream) {
  API_BEGIN
  return launch_ln_backward(x, dy, gamma, rows, C, eps, dx, dgamma, dbeta, nullptr, (hipStream_t)stream);
  API_END
}

// the fixed-order forms take a workspace: allocated here from the launcher's own size function, freed after the stream has drained
static int op_ws_alloc(const char* what, long floats, float** ws) {
  const hipError_t e = hipMalloc(ws, (size_t)std::max(floats, 1L) * 4);
  if (e == hipSuccess) return T2P_OK;
  *ws = nullptr;
  set_last_error(std::string(what) + ": hipMalloc: " + hipGetErrorString(e));
  return T2P_ERR_HIP;
}

int t2p_op_layernorm_backward_form(const float* x, const float* dy, const float* gamma, int64_t rows, int C, float eps, float* dx,
                                   float* dgamma, float* dbeta, int fixed_order, void* stream) {
  API_BEGIN
  hipStream_t s = (hipStream_t)stream;
  if (!fixed_order) return launch_ln_backward(x, dy, gamma, rows, C, eps, dx, dgamma, dbeta, nullptr, s);
  T2P_REQUIRE(rows > 0 && C > 0, "layernorm_backward arguments");
  float* ws = nullptr;
  T2P_TRY(op_ws_alloc("layernorm_backward", ln_bwd_ws_floats(rows, C), &ws));
  const int rc = launch_ln_backward(x, dy, gamma, rows, C, eps, dx, dgamma, dbeta, ws, s);
  (void)hipStreamSynchronize(s);
  (void)hipFree(ws);
  return rc;
  API_END
}

int t2p_op_colsum(const float* dy, int nz, int64_t rows_per_z, int N, int64_t ld, float* out, int64_t ld_out, int accumulate, int fixed_order,
                  void* stream) {
  API_BEGIN
  hipStream_t s = (hipStream_t)stream;
  if (!fixed_order) return launch_colsum(dy, nz, rows_per_z, N, ld, out, ld_out, accumulate, nullptr, s);
  T2P_REQUIRE(nz > 0 && rows_per_z > 0 && N > 0, "colsum arguments");
  float* ws = nullptr;
  T2P_TRY(op_ws_alloc("colsum", colsum_ws_floats(nz, rows_per_z, N), &ws));
  const int rc = launch_colsum(dy, nz, rows_per_z, N, ld, out, ld_out, accumulate, ws, s);
  (void)hipStreamSynchronize(s);
  (void)hipFree(ws);
  return rc;
  API_END
}

int t2p_op_sumsq(const float* g, int64_t n, int fixed_order, double* result_host, void* stream) {
  API_BEGIN
  T2P_REQUIRE(g && n > 0 && result_host, "sumsq arguments");
  hipStream_t s = (hipStream_t)stream;
  double* buf = nullptr;                  // [0]: the result, [1 .. 1024]: the partials of the fixed-order form
  const hipError_t e = hipMalloc(&buf, (size_t)1025 * 8);
  if (e != hipSuccess) {
    set_last_error(std::string("sumsq: hipMalloc: ") + hipGetErrorString(e));
    return T2P_ERR_HIP;
  }
  int rc = T2P_OK;
  if (hipMemsetAsync(buf, 0, 8, s) != hipSuccess) rc = T2P_ERR_HIP;      // the atomic form accumulates
  if (rc == T2P_OK) rc = launch_sumsq(g, n, fixed_order ? buf + 1 : nullptr, buf, s);
  if (rc == T2P_OK && (hipStreamSynchronize(s) != hipSuccess || hipMemcpy(result_host, buf, 8, hipMemcpyDeviceToHost) != hipSuccess)) {
    set_last_error("sumsq: reading the result back failed");
    rc = T2P_ERR_HIP;
  }
  (void)hipStreamSynchronize(s);
  (void)hipFree(buf);
  return rc;
  API_END
}

int t2p_op_seed_scale(const float* x, int64_t n, float target, float* s2_host, void* stream) {
  API_BEGIN
  T2P_REQUIRE(x && n > 0 && s2_host && target > 0.f, "seed_scale arguments");
  hipStream_t s = (hipStream_t)stream;
  float* buf = nullptr;                   // [0 .. 1]: {S, 1 / S}, [2]: the absmax word
  const hipError_t e = hipMalloc(&buf, 3 * 4);
  if (e != hipSuccess) {
    set_last_error(std::string("seed_scale: hipMalloc: ") + hipGetErrorString(e));
    return T2P_ERR_HIP;
  }
  int rc = launch_seed_scale(x, n, target, (unsigned int*)(buf + 2), buf, s);
  if (rc == T2P_OK && (hipStreamSynchronize(s) != hipSuccess || hipMemcpy(s2_host, buf, 8, hipMemcpyDeviceToHost) != hipSuccess)) {
    set_last_error("seed_scale: reading the result back failed");
    rc = T2P_ERR_HIP;
  }
  (void)hipStreamSynchronize(s);
  (void)hipFree(buf);
  return rc;
  API_END
}

int t2p_op_softmax_backward(const float* P, float* dP_inout, int64_t rows, int n, float scale, void* stream) {
  API_BEGIN
  return launch_softmax_backward(P, dP_inout, rows, n, scale, (hipStream_t)stream);
  API_END
}

int t2p_op_geglu_backward(const float* u, const float* dy, float* du, int64_t rows, int inner, void* stream) {
  API_BEGIN
  return launch_geglu_backward(u, dy, du, rows, inner, (hipStream_t)stream);
  API_END
}

}  // extern "C"
