// api_common.h -- what every host unit of the C-ABI (*_api.hip) shares: the error path, the device allocation and upload
// helpers, the event-pair timer of the tlfea_*_time_* entry points and the readers of the environment switches.  Private to csrc/.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/tlfea_c.h"
#include "tlfea_internal.h"

#define HIP_TRY(expr)                                                                                \
  do {                                                                                               \
    hipError_t _e = (expr);                                                                          \
    if (_e != hipSuccess)                                                                            \
      return tlfea::fail(std::string(hipGetErrorString(_e)) + " in " + __FILE__ + ":" + std::to_string(__LINE__)); \
  } while (0)
#define TRY(x)           \
  do {                   \
    if (int _r = (x)) return _r; \
  } while (0)
#define NEED_SETUP(h, what) \
  if (!(h) || !(h)->is_setup) return tlfea::fail(std::string("GPU_FEAT10_Data must be set up before ") + what)
#define D2H(dst, src, n) HIP_TRY(hipMemcpy(dst, src, (size_t)(n) * sizeof(*(dst)), hipMemcpyDeviceToHost))

namespace tlfea {

// the message of tlfea_last_error() (thread-local, tlfea_api.hip); api_fail (tlfea_internal.h) sets it
std::string& api_error();

inline int fail(const std::string& msg) { return api_fail(msg); }

template <typename T>
int dmalloc(T** p, size_t n) {
  *p = nullptr;
  if (n == 0) n = 1;
  HIP_TRY(hipMalloc((void**)p, n * sizeof(T)));
  return 0;
}

template <typename T>
void dfree(T*& p) {
  if (p) (void)hipFree(p);
  p = nullptr;
}

template <typename T>
int upload_vec(T** dst, const std::vector<T>& v) {
  TRY(dmalloc(dst, std::max<size_t>(1, v.size())));
  if (!v.empty()) HIP_TRY(hipMemcpy(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}

// Milliseconds per call over `reps` calls fn(0), ..., fn(reps - 1) between one pair of events on `st`.  fn returns 0 to
// go on, kStopReps to end the repetitions there (the time is still divided by reps), or an error code (> 0), which
// time_reps hands back once its events are released.
constexpr int kStopReps = -1;
template <typename F>
int time_reps(hipStream_t st, int reps, double* ms_per_call, F&& fn) {
  hipEvent_t ev[2] = {nullptr, nullptr};
  float ms = 0.f;
  int rc = 0;
  hipError_t e = hipEventCreate(&ev[0]);
  if (e == hipSuccess) e = hipEventCreate(&ev[1]);
  if (e == hipSuccess) e = hipEventRecord(ev[0], st);
  for (int r = 0; e == hipSuccess && rc == 0 && r < reps; r++) rc = fn(r);
  if (e == hipSuccess && rc <= 0) e = hipEventRecord(ev[1], st);
  if (e == hipSuccess && rc <= 0) e = hipEventSynchronize(ev[1]);
  if (e == hipSuccess && rc <= 0) e = hipEventElapsedTime(&ms, ev[0], ev[1]);
  for (hipEvent_t x : ev)
    if (x) (void)hipEventDestroy(x);
  if (rc > 0) return rc;
  HIP_TRY(e);
  *ms_per_call = ms / reps;
  return 0;
}

// environment switches: the value when the variable is set, dflt when it is not
inline int env_int(const char* name, int dflt) { const char* e = std::getenv(name); return e ? std::atoi(e) : dflt; }
inline long long env_ll(const char* name, long long dflt) { const char* e = std::getenv(name); return e ? std::atoll(e) : dflt; }
inline double env_double(const char* name, double dflt) { const char* e = std::getenv(name); return e ? std::atof(e) : dflt; }
// set: any integer but 0 is on
inline bool env_flag(const char* name, bool dflt) { const char* e = std::getenv(name); return e ? std::atoi(e) != 0 : dflt; }
// forced on (1), forced off (0) or not set (-1: the code chooses)
inline int env_tristate(const char* name) { const char* e = std::getenv(name); return e ? (std::atoi(e) != 0 ? 1 : 0) : -1; }

}  // namespace tlfea
