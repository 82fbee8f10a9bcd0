// rccl_api.hip -- C-ABI (include/tlfea_c.h, tlfea_rccl_*) of the built-in RCCL collectives (opt-in): librccl.so resolved at
// run time, communicator create / destroy with a watchdog, the all-reduce and halo-exchange callbacks a partitioned solver
// is handed, and the self-check that decides whether the partitioned CG iteration may be replayed from a hipGraph.
#include <dlfcn.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <thread>

#include "newton_handle.h"

using namespace tlfea;

struct RcclUniqueId {  // == ncclUniqueId (rccl.h): 128 opaque bytes, passed BY VALUE to ncclCommInitRank
  char internal[128];
};

// ---- built-in RCCL all-reduce (opt-in): the collective is enqueued from C++ on the stream the solver launches on -------
// stream the built-in callbacks enqueue on: the null stream on the boundary-sum path (its launch stream once an interface
// is set), the solver's own stream on the overlapping-partition path (set by the engine around every call)
thread_local hipStream_t tlfea::g_rccl_stream = nullptr;
namespace {
struct RcclApi {
  void* lib = nullptr;
  int (*get_unique_id)(void*) = nullptr;
  int (*comm_init_rank)(void**, int, RcclUniqueId, int) = nullptr;
  int (*all_reduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*comm_destroy)(void*) = nullptr;
  const char* (*error_string)(int) = nullptr;
  int (*send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*group_start)() = nullptr;
  int (*group_end)() = nullptr;
};
RcclApi& rccl_api() {
  static RcclApi a;
  if (a.lib) return a;
  for (const char* name : {"librccl.so", "librccl.so.1"}) {
    a.lib = dlopen(name, RTLD_NOW | RTLD_NOLOAD);  // the copy the process already uses (torch's), if any
    if (a.lib) break;
  }
  if (!a.lib)
    for (const char* name : {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"}) {
      a.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (a.lib) break;
    }
  if (!a.lib) return a;
  a.get_unique_id = (int (*)(void*))dlsym(a.lib, "ncclGetUniqueId");
  a.comm_init_rank = (int (*)(void**, int, RcclUniqueId, int))dlsym(a.lib, "ncclCommInitRank");
  a.all_reduce = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))dlsym(a.lib, "ncclAllReduce");
  a.comm_destroy = (int (*)(void*))dlsym(a.lib, "ncclCommDestroy");
  a.error_string = (const char* (*)(int))dlsym(a.lib, "ncclGetErrorString");
  a.send = (int (*)(const void*, size_t, int, int, void*, hipStream_t))dlsym(a.lib, "ncclSend");
  a.recv = (int (*)(void*, size_t, int, int, void*, hipStream_t))dlsym(a.lib, "ncclRecv");
  a.group_start = (int (*)())dlsym(a.lib, "ncclGroupStart");
  a.group_end = (int (*)())dlsym(a.lib, "ncclGroupEnd");
  if (!a.get_unique_id || !a.comm_init_rank || !a.all_reduce || !a.comm_destroy) a.lib = nullptr;
  return a;
}
int rccl_fail(const char* what, int rc) {
  RcclApi& a = rccl_api();
  return fail(std::string(what) + ": " + (a.error_string ? a.error_string(rc) : "RCCL error " + std::to_string(rc)));
}
int rccl_allreduce_cb(void* comm, double* d_buf, int n) {  // sum of n doubles in place
  RcclApi& a = rccl_api();
  const int rc = a.all_reduce(d_buf, d_buf, (size_t)n, /*ncclDouble*/ 8, /*ncclSum*/ 0, comm, g_rccl_stream);
  return rc == 0 ? 0 : 1;
}
// one group of send / recv pairs per ghost refresh (ncclGroup makes the pairs deadlock-free in any order)
int rccl_halo_exchange_cb(void* comm, const void* d_send, void* d_recv, int n_peers, const int* peers,
                          const long long* so, const long long* ro) {
  RcclApi& a = rccl_api();
  if (!a.send || !a.recv || !a.group_start || !a.group_end) return 1;
  int rc = a.group_start();
  for (int k = 0; k < n_peers && rc == 0; k++) {
    const long long ns = so[k + 1] - so[k], nr = ro[k + 1] - ro[k];
    if (ns > 0) rc = a.send((const char*)d_send + so[k], (size_t)ns, /*ncclInt8*/ 0, peers[k], comm, g_rccl_stream);
    if (rc == 0 && nr > 0) rc = a.recv((char*)d_recv + ro[k], (size_t)nr, /*ncclInt8*/ 0, peers[k], comm, g_rccl_stream);
  }
  const int rc2 = a.group_end();
  return (rc == 0 && rc2 == 0) ? 0 : 1;
}
}  // namespace

extern "C" int tlfea_rccl_unique_id(char* id128) {
  RcclApi& a = rccl_api();
  if (!a.lib) return fail("tlfea_rccl: librccl.so could not be resolved");
  RcclUniqueId id;
  const int rc = a.get_unique_id(&id);
  if (rc) return rccl_fail("ncclGetUniqueId", rc);
  std::memcpy(id128, id.internal, 128);
  return 0;
}
extern "C" int tlfea_rccl_comm_create(const char* id128, int rank, int world, void** comm_out) {
  RcclApi& a = rccl_api();
  if (!a.lib) return fail("tlfea_rccl: librccl.so could not be resolved");
  RcclUniqueId id;
  std::memcpy(id.internal, id128, 128);
  void* comm = nullptr;
  const int rc = a.comm_init_rank(&comm, world, id, rank);
  if (rc) return rccl_fail("ncclCommInitRank", rc);
  *comm_out = comm;
  return 0;
}
extern "C" int tlfea_rccl_comm_destroy(void* comm) {
  RcclApi& a = rccl_api();
  if (!a.lib || !comm) return 0;
  HIP_TRY(hipDeviceSynchronize());
  const int rc = a.comm_destroy(comm);
  return rc ? rccl_fail("ncclCommDestroy", rc) : 0;
}
extern "C" tlfea_allreduce_fn tlfea_rccl_allreduce_fn(void) { return rccl_allreduce_cb; }

extern "C" tlfea_halo_exchange_fn tlfea_rccl_halo_exchange_fn(void) { return rccl_halo_exchange_cb; }

// A collective that never completes cannot be abandoned: the watchdog reports and ends the process (exit code 97), so the
// launcher sees a failed rank instead of a hang.
[[noreturn]] static void rccl_watchdog_abort(const char* what, int rank, double timeout_s) {
  std::fprintf(stderr, "tlfea: rank %d: %s did not complete within %.0f s -- giving up (exit 97)\n", rank, what, timeout_s);
  std::fflush(stderr);
  _exit(97);
}
extern "C" int tlfea_rccl_comm_create_timeout(const char* id128, int rank, int world, double timeout_s, void** comm_out) {
  RcclApi& a = rccl_api();
  if (!a.lib) return fail("tlfea_rccl: librccl.so could not be resolved");
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  std::atomic<int> done{0};
  int rc = 0;
  void* comm = nullptr;
  RcclUniqueId id;
  std::memcpy(id.internal, id128, 128);
  std::thread t([&] {
    (void)hipSetDevice(dev);
    rc = a.comm_init_rank(&comm, world, id, rank);
    done.store(1);
  });
  const auto t0 = std::chrono::steady_clock::now();
  while (!done.load()) {
    std::this_thread::sleep_for(std::chrono::milliseconds(20));
    if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s) {
      t.detach();
      rccl_watchdog_abort("ncclCommInitRank", rank, timeout_s);
    }
  }
  t.join();
  if (rc) return rccl_fail("ncclCommInitRank", rc);
  *comm_out = comm;
  return 0;
}
extern "C" int tlfea_rccl_self_check(void* comm, int rank, int world, double timeout_s) {
  RcclApi& a = rccl_api();
  if (!a.lib || !comm) return fail("tlfea_rccl_self_check: no communicator");
  hipStream_t st = nullptr;
  HIP_TRY(hipStreamCreate(&st));
  double* d = nullptr;
  HIP_TRY(hipMalloc((void**)&d, 8 * sizeof(double)));
  // all-reduce: sum over ranks of (rank + 1) and of (rank + 1)^2; ring: every rank sends 1000 + rank to rank + 1
  double h[8] = {rank + 1.0, (rank + 1.0) * (rank + 1.0), 1000.0 + rank, 0, -1.0, 0, 0, 0};
  HIP_TRY(hipMemcpy(d, h, sizeof(h), hipMemcpyHostToDevice));
  auto collectives = [&]() -> int {  // enqueued on st: eagerly here, under capture below
    int rc = rccl_allreduce_cb(comm, d, 2);
    if (rc == 0 && world > 1) {
      const int next = (rank + 1) % world, prev = (rank + world - 1) % world;
      rc = a.group_start();
      if (rc == 0) rc = a.send(d + 2, sizeof(double), 0, next, comm, st);
      if (rc == 0) rc = a.recv(d + 4, sizeof(double), 0, prev, comm, st);
      const int rc2 = a.group_end();
      rc = rc ? rc : rc2;
    }
    return rc;
  };
  auto wait = [&](const char* what) {  // for st to drain; the watchdog ends the process when it does not
    const auto t0 = std::chrono::steady_clock::now();
    while (hipStreamQuery(st) == hipErrorNotReady) {
      std::this_thread::sleep_for(std::chrono::milliseconds(5));
      if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s)
        rccl_watchdog_abort(what, rank, timeout_s);
    }
  };
  g_rccl_stream = st;
  const int rc = collectives();
  g_rccl_stream = nullptr;
  if (rc) {
    (void)hipFree(d);
    (void)hipStreamDestroy(st);
    return fail("tlfea_rccl_self_check: RCCL refused the check collectives");
  }
  wait("the RCCL self-check (all-reduce + ring send/recv)");
  HIP_TRY(hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost));
  const double s1 = world * (world + 1.0) / 2.0, s2 = world * (world + 1.0) * (2.0 * world + 1.0) / 6.0;
  const double ring = world > 1 ? 1000.0 + (rank + world - 1) % world : -1.0;
  if (h[0] != s1 || h[1] != s2 || h[4] != ring) {
    std::fprintf(stderr, "tlfea: rank %d: RCCL self-check WRONG ANSWER: all-reduce %.17g %.17g (expected %.17g %.17g), ring %.17g "
                 "(expected %.17g) -- giving up (exit 97)\n", rank, h[0], h[1], s1, s2, h[4], ring);
    std::fflush(stderr);
    _exit(97);
  }
  // The same collectives once more, captured in a hipGraph and replayed -- what the solver does with its CG iteration.
  // A capture RCCL refuses, or a replay with the wrong answer, switches the partitioned solve to eager launches on EVERY
  // rank (agreed with an eager all-reduce); a replay that never finishes ends the job through the watchdog.
  double ok = 1.0;
  if (halo_graph_wanted()) {
    const double h2[8] = {rank + 1.0, (rank + 1.0) * (rank + 1.0), 1000.0 + rank, 0, -1.0, 0, 0, 0};
    double hr[8];
    HIP_TRY(hipMemcpy(d, h2, sizeof(h2), hipMemcpyHostToDevice));
    hipGraph_t g = nullptr;
    hipGraphExec_t ge = nullptr;
    g_rccl_stream = st;
    bool captured = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess;
    if (captured) {
      const int rc3 = collectives();
      captured = hipStreamEndCapture(st, &g) == hipSuccess && rc3 == 0 && g &&
                 hipGraphInstantiate(&ge, g, nullptr, nullptr, 0) == hipSuccess;
    }
    g_rccl_stream = nullptr;
    (void)hipGetLastError();
    if (captured && hipGraphLaunch(ge, st) == hipSuccess) {
      wait("the hipGraph replay of the RCCL self-check (set TLFEA_HALO_GRAPH=0 to run the partitioned solve without graph "
           "capture)");
      HIP_TRY(hipMemcpy(hr, d, sizeof(hr), hipMemcpyDeviceToHost));
      if (hr[0] != s1 || hr[1] != s2 || hr[4] != ring) ok = 0.0;
    } else {
      ok = 0.0;
    }
    if (ge) (void)hipGraphExecDestroy(ge);
    if (g) (void)hipGraphDestroy(g);
    (void)hipGetLastError();
    // agree: every rank replays graphs, or none does
    HIP_TRY(hipMemcpy(d, &ok, sizeof(double), hipMemcpyHostToDevice));
    g_rccl_stream = st;
    const int rc5 = rccl_allreduce_cb(comm, d, 1);
    g_rccl_stream = nullptr;
    if (rc5) return fail("tlfea_rccl_self_check: RCCL refused the agreement all-reduce");
    wait("the RCCL self-check (agreement all-reduce)");
    double sum = 0.0;
    HIP_TRY(hipMemcpy(&sum, d, sizeof(double), hipMemcpyDeviceToHost));
    if (sum != (double)world) {
      halo_graph_give_up();
      if (rank == 0)
        std::fprintf(stderr, "tlfea: RCCL collectives could not be captured / replayed in a hipGraph on %d of %d ranks: the "
                     "partitioned CG iteration runs with eager launches\n", world - (int)sum, world);
    }
  }
  (void)hipFree(d);
  (void)hipStreamDestroy(st);
  return 0;
}
