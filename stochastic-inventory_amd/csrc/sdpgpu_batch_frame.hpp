// sdpgpu_batch_frame.hpp -- BatchFrame: the ONE place a batch keeps its error text, its stream, the timing events of a sweep, the
// staging block of sdpgpu_batch_initial and the scratch block and events of its rollouts.  An sdpgpu_batch owns one by value
// (sdpgpu_batch.hip); a batch of the STAFF family (sdpgpu_staffbatch.hip) works on the frame of the sdpgpu_batch that holds it.
// The owners keep what is theirs -- layout, tables, plans, kernels, the loop of a sweep -- and call the frame around it:
//   open(N)                            no device: refused; the stream unless the caller gave one, ev0 / ev1, the staging block
//   sweep_begin()                      the period events when profiling, ev0
//   period_mark(t)                     before the launches of period index t; period_mark(-1) behind the last period's
//   sweep_end(sync)                    ev1, the flags, the optional synchronise
//   read_check / read_row              the refusals of a row read-out, and the read-out
//   initial_download                   the staging block (N doubles, then N int32) behind the owner's initial kernel
//   solve_ms / period_ms / synchronize / set_stream / close
// It is also the owner the shared rollout helpers see (sim_scratch, RolloutFrame: d_sim_scratch, sim_scratch_bytes, stream,
// sim_fail, sim_events).  Internal, header only.
#pragma once
#include "sdpgpu_sim_host.hpp"

namespace sdpgpu_detail {

// the one formatter of an error text; returns `code`
inline int vfail_to(std::string* sink, int code, const char* fmt, va_list ap) {
  char buf[640];
  vsnprintf(buf, sizeof buf, fmt, ap);
  if (sink) *sink = buf;
  return code;
}
inline int fail_to(std::string* sink, int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfail_to(sink, code, fmt, ap);
  va_end(ap);
  return code;
}

struct BatchFrame {
  std::string err;  // sdpgpu_batch_last_error
  int device = -1;
  int32_t T = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false, stream_given = false;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::vector<hipEvent_t> ev_period;  // [T + 1] when profiling
  bool profiling = false, timed = false, periods_timed = false;
  char* d_ini_out = nullptr;      // N doubles, then N int32
  char* d_sim_scratch = nullptr;  // sim_scratch of sdpgpu_sim_host.hpp: grow-only
  size_t sim_scratch_bytes = 0;
  hipEvent_t sim_ev0 = nullptr, sim_ev1 = nullptr;

  template <class... A>
  int fail(int code, const char* fmt, A... a) {
    return fail_to(&err, code, fmt, a...);
  }

  int open(int32_t N);
  int set_stream(void* hip_stream);
  int sweep_begin();
  int period_mark(int t);
  int sweep_end(bool sync);
  int synchronize(bool allocated);
  int read_row(void* dst, const void* dev_src, size_t bytes);
  double* ini_value() const { return reinterpret_cast<double*>(d_ini_out); }
  int32_t* ini_action(int32_t N) const { return reinterpret_cast<int32_t*>(d_ini_out + (size_t)N * 8); }
  int initial_download(double* out_value, int32_t* out_action_index, int32_t N);
  int solve_ms(double* out);
  double period_ms(int32_t period);
  void close(bool drain, std::initializer_list<void*> owner_buffers, const std::vector<void*>& more = {});
};

// the error sink and the timing events of the shared host helpers (guarded, no_device, sim_scratch, RolloutFrame)
template <class... A>
int sim_fail(BatchFrame* f, int code, const char* fmt, A... a) {
  return f->fail(code, fmt, a...);
}
inline hipError_t sim_events(BatchFrame* f, hipEvent_t* ev0, hipEvent_t* ev1) {
  hipError_t e = hipSuccess;
  if (!f->sim_ev0 && (e = hipEventCreate(&f->sim_ev0)) != hipSuccess) return e;
  if (!f->sim_ev1 && (e = hipEventCreate(&f->sim_ev1)) != hipSuccess) return e;
  *ev0 = f->sim_ev0;
  *ev1 = f->sim_ev1;
  return hipSuccess;
}

inline int BatchFrame::open(int32_t N) {
  if (const int rc = no_device(this, nullptr)) return rc;
  if (!stream && !stream_given) {
    SIM_TRY(this, hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    own_stream = true;
  }
  SIM_TRY(this, hipEventCreate(&ev0));
  SIM_TRY(this, hipEventCreate(&ev1));
  SIM_TRY(this, hipMalloc((void**)&d_ini_out, (size_t)N * 12));
  return SDPGPU_OK;
}

inline int BatchFrame::set_stream(void* hip_stream) {
  if (own_stream && stream) {
    DeviceScope dev;
    SIM_TRY(this, dev.enter(device));
    (void)hipStreamSynchronize(stream);
    (void)hipStreamDestroy(stream);
  }
  stream = (hipStream_t)hip_stream;
  own_stream = false;
  stream_given = true;
  return SDPGPU_OK;
}

inline int BatchFrame::sweep_begin() {
  if (profiling && ev_period.empty()) {
    ev_period.assign((size_t)T + 1, nullptr);
    for (hipEvent_t& e : ev_period) SIM_TRY(this, hipEventCreate(&e));
  }
  periods_timed = false;
  SIM_TRY(this, hipEventRecord(ev0, stream));
  return SDPGPU_OK;
}

// period t was launched between the events t + 1 and t (the sweep runs t = T - 1 .. 0)
inline int BatchFrame::period_mark(int t) {
  if (profiling) SIM_TRY(this, hipEventRecord(ev_period[(size_t)(t + 1)], stream));
  return SDPGPU_OK;
}

inline int BatchFrame::sweep_end(bool sync) {
  SIM_TRY(this, hipEventRecord(ev1, stream));
  timed = true;
  periods_timed = profiling;
  if (sync) SIM_TRY(this, hipStreamSynchronize(stream));
  return SDPGPU_OK;
}

inline int BatchFrame::synchronize(bool allocated) {
  if (!allocated) return SDPGPU_OK;
  DeviceScope dev;
  SIM_TRY(this, dev.enter(device));
  SIM_TRY(this, hipStreamSynchronize(stream));
  return SDPGPU_OK;
}

// The refusals of a row read-out (sdpgpu_batch_values, _policy, _gy), in the order each family has always reported them: a
// batch of the staff family looks at `solved` before the output arguments (solved_first), a backorder batch after.  nx: the
// row's length (anything when instance or period is out of range); states: the end of the "bad output" sentence.
inline int read_check(BatchFrame* f, const char* who, int32_t instance, int32_t N, int32_t period, const void* out, int64_t n, int64_t nx,
                      const char* states, bool solved, bool solved_first, bool ping_pong_values) {
  if (instance < 0 || instance >= N) return f->fail(SDPGPU_ERR_ARG, "%s: instance %d outside 0 .. %d", who, instance, N - 1);
  if (period < 1 || period > f->T) return f->fail(SDPGPU_ERR_ARG, "%s: period %d outside 1 .. %d", who, period, f->T);
  if (solved_first && !solved) return f->fail(SDPGPU_ERR_STATE, "%s before sdpgpu_batch_solve", who);
  if (!out || n < 0 || n > nx) return f->fail(SDPGPU_ERR_ARG, "%s: bad output (n = %lld, %s)", who, (long long)n, states);
  if (!solved) return f->fail(SDPGPU_ERR_STATE, "%s before sdpgpu_batch_solve", who);
  if (ping_pong_values && period > 2)
    return f->fail(SDPGPU_ERR_STATE, "%s: V_%d was overwritten (store_all_values = 0 keeps two ping-pong tables: periods 1 and 2 survive)", who, period);
  return SDPGPU_OK;
}

inline int BatchFrame::read_row(void* dst, const void* dev_src, size_t bytes) {
  DeviceScope dev;
  SIM_TRY(this, dev.enter(device));
  SIM_TRY(this, hipStreamSynchronize(stream));
  SIM_TRY(this, hipMemcpy(dst, dev_src, bytes, hipMemcpyDeviceToHost));
  return SDPGPU_OK;
}

inline int BatchFrame::initial_download(double* out_value, int32_t* out_action_index, int32_t N) {
  std::vector<char> host((size_t)N * 12);
  SIM_TRY(this, hipMemcpyAsync(host.data(), d_ini_out, host.size(), hipMemcpyDeviceToHost, stream));
  SIM_TRY(this, hipStreamSynchronize(stream));
  std::memcpy(out_value, host.data(), (size_t)N * 8);
  std::memcpy(out_action_index, host.data() + (size_t)N * 8, (size_t)N * 4);
  return SDPGPU_OK;
}

// *out stays as it is until a sweep has been timed
inline int BatchFrame::solve_ms(double* out) {
  if (!timed) return SDPGPU_OK;
  DeviceScope dev;
  SIM_TRY(this, dev.enter(device));
  SIM_TRY(this, hipEventSynchronize(ev1));
  float ms = 0;
  SIM_TRY(this, hipEventElapsedTime(&ms, ev0, ev1));
  *out = ms;
  return SDPGPU_OK;
}

inline double BatchFrame::period_ms(int32_t period) {
  if (period < 1 || period > T || !periods_timed) {
    (void)fail(SDPGPU_ERR_STATE, "sdpgpu_batch_period_ms: period %d has no timing (sdpgpu_batch_set_profiling before the solve)", period);
    return -1.0;
  }
  DeviceScope dev;
  if (dev.enter(device) != hipSuccess) return -1.0;
  // period t was launched between the events t and t - 1 (the sweep runs t = T .. 1)
  if (hipEventSynchronize(ev_period[(size_t)period - 1]) != hipSuccess) return -1.0;
  float ms = 0;
  if (hipEventElapsedTime(&ms, ev_period[(size_t)period], ev_period[(size_t)period - 1]) != hipSuccess) return -1.0;
  return ms;
}

// drain: something was allocated, so the stream may still hold work on it.  The owner's device buffers (a list, and a vector of
// further ones) go between the drain and the stream.  Allocates nothing: it runs in sdpgpu_batch_destroy, outside every barrier.
inline void BatchFrame::close(bool drain, std::initializer_list<void*> owner_buffers, const std::vector<void*>& more) {
  DeviceScope dev;
  if (drain) {
    (void)dev.enter(device);
    if (stream) (void)hipStreamSynchronize(stream);
  }
  if (ev0) (void)hipEventDestroy(ev0);
  if (ev1) (void)hipEventDestroy(ev1);
  for (hipEvent_t e : ev_period)
    if (e) (void)hipEventDestroy(e);
  for (void* p : owner_buffers)
    if (p) (void)hipFree(p);
  for (void* p : more)
    if (p) (void)hipFree(p);
  if (d_ini_out) (void)hipFree(d_ini_out);
  if (d_sim_scratch) (void)hipFree(d_sim_scratch);
  if (sim_ev0) (void)hipEventDestroy(sim_ev0);
  if (sim_ev1) (void)hipEventDestroy(sim_ev1);
  if (stream && own_stream) (void)hipStreamDestroy(stream);
}

}  // namespace sdpgpu_detail
