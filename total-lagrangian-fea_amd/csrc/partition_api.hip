// partition_api.hip -- the partition plumbing of the Newton solver: the boundary-node interface and the overlapping
// partition (ghost-layer plans and refreshes), the sums over ranks through the caller's collectives, and the norms and
// scalar read-backs built on them.
#include "newton_handle.h"

using namespace tlfea;

extern "C" int tlfea_newton_set_interface(tlfea_newton_t s, const int* iface_nodes, const int* iface_slots,
                                          int n_local, int n_global, const double* node_weight,
                                          tlfea_allreduce_fn fn, void* user, int sync_before_callback) {
  // every rejection comes before anything is released: a caller that catches the error keeps a working solver
  if (!s) return fail("tlfea_newton_set_interface: null solver");
  if (s->d->d_emat)
    return fail("tlfea_newton_set_interface: per-element materials are not supported on the partitioned path");
  if (s->d->obs.n > 0)
    return fail("tlfea_newton_set_interface: rigid obstacles are not supported on the partitioned path (clear them first)");
  if (s->d->loads_on())
    return fail("tlfea_newton_set_interface: distributed loads are not supported on the partitioned path (clear them first)");
  if (s->pmg.tried)
    return fail("tlfea_newton_set_interface: set the interface before the first linear solve (the p-multigrid hierarchy "
                "is partitioned with it)");
  if (fn) {
    if (s->d->cons_mode == 2)
      return fail("tlfea_newton_set_interface: general linear constraints are not supported on the multi-GPU path");
    if (n_local < 0 || n_global < 0 || (n_local > 0 && (!iface_nodes || !iface_slots)) || !node_weight)
      return fail("tlfea_newton_set_interface: null / negative argument");
    for (int k = 0; k < n_local; k++)
      if (iface_nodes[k] < 0 || iface_nodes[k] >= s->N || iface_slots[k] < 0 || iface_slots[k] >= n_global)
        return fail("tlfea_newton_set_interface: index out of range");
  }
  HIP_TRY(hipStreamSynchronize(s->stream));  // launches that read the old lists may still be in flight
  HIP_TRY(hipDeviceSynchronize());
  void** ptrs[] = {(void**)&s->d_if_node, (void**)&s->d_if_slot, (void**)&s->d_ibuf, (void**)&s->d_w,
                   (void**)&s->d_nw, (void**)&s->d_wc};
  for (void** p : ptrs)
    if (*p) {
      (void)hipFree(*p);
      *p = nullptr;
    }
  s->n_if_loc = n_local;
  s->n_if_glob = n_global;
  s->ar = fn;
  s->ar_user = user;
  s->sync_before_cb = sync_before_callback != 0;
  s->n_constraints_global = s->n_constraints;
  s->stream = fn ? nullptr : s->stream_own;
  if (s->d_own) {
    (void)hipFree(s->d_own);
    s->d_own = nullptr;
  }
  if (!fn) {
    s->n_if_loc = s->n_if_glob = 0;
    return 0;
  }
  tlfea_t10_t d = s->d;
  const size_t N = s->N;
  TRY(dmalloc(&s->d_if_node, (size_t)std::max(1, n_local)));
  TRY(dmalloc(&s->d_if_slot, (size_t)std::max(1, n_local)));
  TRY(dmalloc(&s->d_ibuf, (size_t)9 * std::max(1, n_global) + 2 * kNPart));
  TRY(dmalloc(&s->d_w, 3 * N));
  TRY(dmalloc(&s->d_nw, N));
  if (n_local) {
    HIP_TRY(hipMemcpy(s->d_if_node, iface_nodes, (size_t)n_local * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->d_if_slot, iface_slots, (size_t)n_local * sizeof(int), hipMemcpyHostToDevice));
  }
  s->h_if_node.assign(iface_nodes, iface_nodes + n_local);
  s->h_if_slot.assign(iface_slots, iface_slots + n_local);
  s->h_nw.assign(node_weight, node_weight + N);
  {
    std::vector<int> bs(N, -1);
    for (int k = 0; k < n_local; k++) bs[iface_nodes[k]] = iface_slots[k];
    if (s->d_bslot_f) (void)hipFree(s->d_bslot_f);
    TRY(dmalloc(&s->d_bslot_f, N));
    HIP_TRY(hipMemcpy(s->d_bslot_f, bs.data(), N * sizeof(int), hipMemcpyHostToDevice));
  }
  std::vector<double> w3(3 * N);
  for (size_t i = 0; i < N; i++) w3[3 * i] = w3[3 * i + 1] = w3[3 * i + 2] = node_weight[i];
  HIP_TRY(hipMemcpy(s->d_w, w3.data(), 3 * N * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(s->d_nw, node_weight, N * sizeof(double), hipMemcpyHostToDevice));
  if (d->n_constraint > 0) {
    std::vector<double> wc((size_t)d->n_constraint);
    for (int k = 0; k < d->n_constraint; k++) wc[k] = node_weight[d->h_fixed[k / 3]];
    TRY(dmalloc(&s->d_wc, wc.size()));
    HIP_TRY(hipMemcpy(s->d_wc, wc.data(), wc.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  // every rank must take the same branches of the ALM loop: agree on whether ANY rank has constraints
  double cnt = d->n_constraint;
  HIP_TRY(hipMemcpy(s->d_ibuf, &cnt, sizeof(double), hipMemcpyHostToDevice));
  if (fn(user, s->d_ibuf, 1)) return fail("interface all-reduce callback failed");
  HIP_TRY(hipMemcpy(&cnt, s->d_ibuf, sizeof(double), hipMemcpyDeviceToHost));
  s->n_constraints_global = (int)(cnt + 0.5);
  return 0;
}

// ---- overlapping partition ------------------------------------------------------------------------------------------------
// hipGraph replay of the partitioned CG iteration (collectives included): on unless TLFEA_HALO_GRAPH=0, and off for the
// process once the self-check (rccl_api.hip) or a failed capture of the iteration finds that RCCL cannot be captured /
// replayed here
static bool g_rccl_graph_ok = true;
bool tlfea::halo_graph_wanted() {
  static const bool on = env_flag("TLFEA_HALO_GRAPH", true);
  return on && g_rccl_graph_ok;
}
void tlfea::halo_graph_give_up() { g_rccl_graph_ok = false; }
// Ghost layers on which the CG residual must be exact when the preconditioner starts: the V-cycle's ks pre-smoothing
// passes give up one layer each and must leave layer 1 (restriction) and layer ks - 1 (the post-smoother's own-row
// operands); the polynomial fallback refreshes its direction before every step instead.  The direction z is refreshed
// one layer deeper (the CG's SpMV gives up one).
int tlfea::halo_dr(tlfea_newton_t s) {
  if (precond_eff(s) != 2) return 0;
  const int ks = pmg_ks(s);
  return std::max(ks + 1, 2 * ks - 1);
}

void tlfea::halo_free_plans(tlfea_newton_s::HaloLevel& L) {
  for (auto& kv : L.plans) {
    if (kv.second.d_sidx) (void)hipFree(kv.second.d_sidx);
    if (kv.second.d_ridx) (void)hipFree(kv.second.d_ridx);
  }
  L.plans.clear();
}

extern "C" int tlfea_newton_set_halo(tlfea_newton_t s, const int* node_layer, int depth, const tlfea_halo_lists* lists,
                                     tlfea_allreduce_fn allreduce, tlfea_halo_exchange_fn exchange, void* user,
                                     int sync_before_callback) {
  if (!s || !node_layer || !lists || !allreduce || !exchange) return fail("tlfea_newton_set_halo: null argument");
  if (s->d->d_emat) return fail("tlfea_newton_set_halo: per-element materials are not supported on the partitioned path");
  if (s->d->obs.n > 0)
    return fail("tlfea_newton_set_halo: rigid obstacles are not supported on the partitioned path (clear them first)");
  if (s->d->loads_on())
    return fail("tlfea_newton_set_halo: distributed loads are not supported on the partitioned path (clear them first)");
  if (s->pmg.tried || s->ar)
    return fail("tlfea_newton_set_halo: set the halo on a fresh solver, before the first linear solve and instead of "
                "tlfea_newton_set_interface");
  tlfea_t10_t d = s->d;
  if (d->cons_mode == 2) return fail("tlfea_newton_set_halo: general linear constraints are not supported on the multi-GPU path");
  if (d->kind != kT10) return fail("tlfea_newton_set_halo: T10 meshes only");
  if (depth < 3) return fail("tlfea_newton_set_halo: depth must be at least 3");
  const int N = s->N, P = lists->n_peers;
  if (P < 0 || (P > 0 && (!lists->peers || !lists->send_off || !lists->recv_off)))
    return fail("tlfea_newton_set_halo: peer lists missing");
  for (int i = 0; i < N; i++)
    if (node_layer[i] < 0 || node_layer[i] > depth || (i > 0 && node_layer[i] < node_layer[i - 1]))
      return fail("tlfea_newton_set_halo: node_layer must be non-decreasing in 0..depth (owned nodes first, ghosts by layer)");
  auto& h = s->halo;
  auto& L = h.lv[0];
  for (int k = 0; k < P; k++) {
    const int s0 = lists->send_off[k], s1 = lists->send_off[k + 1], r0 = lists->recv_off[k], r1 = lists->recv_off[k + 1];
    if (s0 < 0 || s1 < s0 || r0 < 0 || r1 < r0) return fail("tlfea_newton_set_halo: offsets must be non-decreasing");
    for (int t = s0; t < s1; t++) {
      const int n = lists->send_nodes[t], l = lists->send_layer[t];
      if (n < 0 || n >= N || node_layer[n] != 0 || l < 1 || l > depth || (t > s0 && l < lists->send_layer[t - 1]))
        return fail("tlfea_newton_set_halo: send list must hold owned nodes ordered by their layer on the peer (1..depth)");
    }
    for (int t = r0; t < r1; t++) {
      const int n = lists->recv_nodes[t];
      if (n < 0 || n >= N || node_layer[n] < 1 || (t > r0 && node_layer[n] < node_layer[lists->recv_nodes[t - 1]]))
        return fail("tlfea_newton_set_halo: recv list must hold ghost nodes ordered by layer");
    }
  }
  HIP_TRY(hipStreamSynchronize(s->stream));
  h.on = true;
  h.native = exchange == tlfea_rccl_halo_exchange_fn() && allreduce == tlfea_rccl_allreduce_fn();
  h.depth = depth;
  h.rank = lists->rank;
  h.world = lists->world;
  h.peers.assign(lists->peers, lists->peers + P);
  h.layer.assign(node_layer, node_layer + N);
  h.n_upto.assign(depth + 1, 0);
  for (int k = 0; k <= depth; k++)
    h.n_upto[k] = (int)(std::upper_bound(h.layer.begin(), h.layer.end(), k) - h.layer.begin());
  halo_free_plans(L);
  L.send_off.assign(lists->send_off, lists->send_off + P + 1);
  L.recv_off.assign(lists->recv_off, lists->recv_off + P + 1);
  L.send_nodes.assign(lists->send_nodes, lists->send_nodes + L.send_off[P]);
  L.send_layer.assign(lists->send_layer, lists->send_layer + L.send_off[P]);
  L.recv_nodes.assign(lists->recv_nodes, lists->recv_nodes + L.recv_off[P]);
  L.recv_layer.resize(L.recv_nodes.size());
  for (size_t t = 0; t < L.recv_nodes.size(); t++) L.recv_layer[t] = node_layer[L.recv_nodes[t]];
  h.xfn = exchange;
  h.arfn = allreduce;
  h.user = user;
  h.sync_cb = sync_before_callback != 0;
  if (!h.d_red) TRY(dmalloc(&h.d_red, (size_t)2 * kNPart));
  if (!h.ev0) {
    HIP_TRY(hipEventCreate(&h.ev0));
    HIP_TRY(hipEventCreate(&h.ev1));
  }
  // dot products: owned DOFs 1, ghosts 0; the assembly takes no shares (d_nw stays null: every row is complete)
  if (s->d_w) (void)hipFree(s->d_w);
  if (s->d_wc) (void)hipFree(s->d_wc);
  s->d_w = s->d_wc = nullptr;
  std::vector<double> w3(3 * (size_t)N);
  for (int i = 0; i < N; i++) w3[3 * (size_t)i] = w3[3 * (size_t)i + 1] = w3[3 * (size_t)i + 2] = node_layer[i] == 0 ? 1.0 : 0.0;
  TRY(dmalloc(&s->d_w, w3.size()));
  HIP_TRY(hipMemcpy(s->d_w, w3.data(), w3.size() * sizeof(double), hipMemcpyHostToDevice));
  s->h_nw.assign((size_t)N, 0.0);
  for (int i = 0; i < N; i++) s->h_nw[i] = node_layer[i] == 0 ? 1.0 : 0.0;
  if (d->n_constraint > 0) {
    std::vector<double> wc((size_t)d->n_constraint);
    for (int k = 0; k < d->n_constraint; k++) wc[k] = s->h_nw[d->h_fixed[k / 3]];
    TRY(dmalloc(&s->d_wc, wc.size()));
    HIP_TRY(hipMemcpy(s->d_wc, wc.data(), wc.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  s->pcg_fused = 0;  // the fused direction update would read p of ghost columns nobody wrote
  // every rank must take the same branches of the ALM loop: agree on whether ANY rank OWNS a constraint
  double cnt = 0.0;
  for (int k = 0; k < d->n_constraint; k++) cnt += s->h_nw[d->h_fixed[k / 3]];
  HIP_TRY(hipMemcpy(h.d_red, &cnt, sizeof(double), hipMemcpyHostToDevice));
  g_rccl_stream = s->stream;
  if (h.arfn(h.user, h.d_red, 1)) return fail("tlfea_newton_set_halo: all-reduce callback failed");
  HIP_TRY(hipStreamSynchronize(s->stream));
  HIP_TRY(hipMemcpy(&cnt, h.d_red, sizeof(double), hipMemcpyDeviceToHost));
  s->n_constraints_global = (int)(cnt + 0.5);
  return 0;
}

// the plan "ghost layers <= D" of a level (built on first use)
static int halo_plan(tlfea_newton_t s, int level, int D, tlfea_newton_s::HaloPlan** out) {
  auto& h = s->halo;
  auto& L = h.lv[level];
  D = std::max(0, std::min(D, h.depth));
  auto it = L.plans.find(D);
  if (it != L.plans.end()) {
    *out = &it->second;
    return 0;
  }
  tlfea_newton_s::HaloPlan pl;
  const int P = (int)h.peers.size();
  std::vector<int> sidx, ridx;
  pl.soff.assign(P + 1, 0);
  pl.roff.assign(P + 1, 0);
  for (int k = 0; k < P; k++) {
    for (int t = L.send_off[k]; t < L.send_off[k + 1] && L.send_layer[t] <= D; t++) sidx.push_back(L.send_nodes[t]);
    for (int t = L.recv_off[k]; t < L.recv_off[k + 1] && L.recv_layer[t] <= D; t++) ridx.push_back(L.recv_nodes[t]);
    pl.soff[k + 1] = (long long)sidx.size();
    pl.roff[k + 1] = (long long)ridx.size();
  }
  pl.n_send = (int)sidx.size();
  pl.n_recv = (int)ridx.size();
  if (sidx.empty()) sidx.push_back(0);
  if (ridx.empty()) ridx.push_back(0);
  TRY(upload_vec(&pl.d_sidx, sidx));
  TRY(upload_vec(&pl.d_ridx, ridx));
  auto ins = L.plans.emplace(D, std::move(pl));
  *out = &ins.first->second;
  return 0;
}

static int halo_exchange_bytes(tlfea_newton_t s, const tlfea_newton_s::HaloPlan& pl, size_t item) {
  auto& h = s->halo;
  const int P = (int)h.peers.size();
  h.so_b.resize(P + 1);
  h.ro_b.resize(P + 1);
  for (int k = 0; k <= P; k++) {
    h.so_b[k] = pl.soff[k] * (long long)item;
    h.ro_b[k] = pl.roff[k] * (long long)item;
  }
  if (h.sync_cb) HIP_TRY(hipStreamSynchronize(s->stream));
  if (s->profiling) (void)hipEventRecord(h.ev0, s->stream);
  g_rccl_stream = s->stream;
  if (h.xfn(h.user, h.d_sbuf, h.d_rbuf, P, h.peers.data(), h.so_b.data(), h.ro_b.data()))
    return fail("halo exchange callback failed");
  if (s->profiling) {
    (void)hipEventRecord(h.ev1, s->stream);
    (void)hipEventSynchronize(h.ev1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, h.ev0, h.ev1);
    h.comm_ms += ms;
  }
  h.n_exch++;
  h.n_exch_cg += h.in_cg ? 1 : 0;
  h.bytes_exch += (double)pl.n_send * item;
  return 0;
}
static int halo_reserve(tlfea_newton_t s, size_t bs, size_t br) {
  auto& h = s->halo;
  if (bs > h.cap_s) {
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (h.d_sbuf) (void)hipFree(h.d_sbuf);
    h.cap_s = bs + bs / 4 + 256;
    HIP_TRY(hipMalloc(&h.d_sbuf, h.cap_s));
  }
  if (br > h.cap_r) {
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (h.d_rbuf) (void)hipFree(h.d_rbuf);
    h.cap_r = br + br / 4 + 256;
    HIP_TRY(hipMalloc(&h.d_rbuf, h.cap_r));
  }
  return 0;
}
// ghost layers <= D of up to three fp64 / fp32 nodal fields (dim values per node) take their owners' values
template <typename T>
static int halo_refresh(tlfea_newton_t s, int level, int D, int dim, T* a, T* b, T* c) {
  if (!s->halo.on || s->halo.peers.empty()) return 0;
  tlfea_newton_s::HaloPlan* pl = nullptr;
  TRY(halo_plan(s, level, D, &pl));
  if (pl->n_send == 0 && pl->n_recv == 0) return 0;
  const int nvec = c ? 3 : (b ? 2 : 1);
  const size_t item = (size_t)dim * nvec * sizeof(T);
  TRY(halo_reserve(s, pl->n_send * item, pl->n_recv * item));
  launch_halo_pack(s->stream, pl->n_send, pl->d_sidx, dim, nvec, a, b, c, (T*)s->halo.d_sbuf);
  TRY(halo_exchange_bytes(s, *pl, item));
  launch_halo_unpack(s->stream, pl->n_recv, pl->d_ridx, dim, nvec, (const T*)s->halo.d_rbuf, a, b, c);
  return 0;
}
int tlfea::halo_refresh_f64(tlfea_newton_t s, int level, int D, int dim, double* a, double* b, double* c) {
  return halo_refresh(s, level, D, dim, a, b, c);
}
int tlfea::halo_refresh_f32(tlfea_newton_t s, int level, int D, int dim, float* a, float* b, float* c) {
  return halo_refresh(s, level, D, dim, a, b, c);
}

// Which of the replicated partition-boundary nodes this rank OWNS (exactly one owner per node over all ranks; interior
// nodes are owned by definition).  With owners set, the polynomial preconditioner becomes rank-local: each rank
// applies it to the block of the matrix on its own nodes with no exchange inside, and ONE packed all-reduce per CG
// iteration sums the result on the boundary (block-Jacobi over ranks; the CG around it restores the coupling).  Without
// owners every polynomial step exchanges its SpMV result (deg-1 collectives per CG iteration instead of one).
extern "C" int tlfea_newton_set_interface_owners(tlfea_newton_t s, const int* owned) {
  if (!s || !owned) return fail("null argument");
  if (!s->ar) return fail("tlfea_newton_set_interface_owners: set the interface first");
  if (!s->d_own) TRY(dmalloc(&s->d_own, (size_t)s->N));
  if (!s->d_sc_mask) TRY(dmalloc(&s->d_sc_mask, 3 * (size_t)s->N));
  HIP_TRY(hipMemcpy(s->d_own, owned, (size_t)s->N * sizeof(int), hipMemcpyHostToDevice));
  s->lam_max_loc = 0.0;
  return 0;
}

int tlfea::call_allreduce(tlfea_newton_t s, double* d_buf, int n) {
  s->n_collectives++;
  if (s->halo.on) {
    auto& h = s->halo;
    if (h.sync_cb) HIP_TRY(hipStreamSynchronize(s->stream));
    if (s->profiling) (void)hipEventRecord(h.ev0, s->stream);
    g_rccl_stream = s->stream;
    if (h.arfn(h.user, d_buf, n)) return fail("all-reduce callback failed");
    if (s->profiling) {
      (void)hipEventRecord(h.ev1, s->stream);
      (void)hipEventSynchronize(h.ev1);
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, h.ev0, h.ev1);
      h.comm_ms += ms;
    }
    h.n_allred++;
    h.n_allred_cg += h.in_cg ? 1 : 0;
    h.bytes_allred += 8.0 * n;
    return 0;
  }
  if (s->sync_before_cb) HIP_TRY(hipStreamSynchronize(s->stream));
  g_rccl_stream = nullptr;
  if (s->ar(s->ar_user, d_buf, n)) return fail("interface all-reduce callback failed");
  return 0;
}

// host doubles summed over ranks through a device buffer (set-up only: synchronises)
int tlfea::allreduce_host(tlfea_newton_t s, double* d_buf, double* h, size_t n) {
  HIP_TRY(hipMemcpy(d_buf, h, n * sizeof(double), hipMemcpyHostToDevice));
  TRY(call_allreduce(s, d_buf, (int)n));
  HIP_TRY(hipStreamSynchronize(s->stream));
  HIP_TRY(hipMemcpy(h, d_buf, n * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}
// Sum over ranks of the partition-boundary entries of a nodal field with `dim` values per node (3 for
// vectors, 9 for diagonal blocks), optionally fused with `n_extra` reduction slots (one collective).
int tlfea::iface_sum(tlfea_newton_t s, double* d_vec, int dim, double* d_extra, int n_extra,
                     double* d_extra2) {
  return iface_sum_lvl(s, s->iface(), d_vec, dim, d_extra, n_extra, d_extra2);
}
// the same for any level of the multigrid hierarchy (its own boundary node / slot lists)
int tlfea::iface_sum_lvl(tlfea_newton_t s, const LevelIface& I, double* d_vec, int dim, double* d_extra, int n_extra,
                         double* d_extra2) {
  if (!s->ar) return 0;
  const int nb = dim * I.n_glob;
  if (nb) HIP_TRY(hipMemsetAsync(s->d_ibuf, 0, (size_t)nb * sizeof(double), s->stream));
  launch_pack(s->stream, I.n_loc, dim, I.d_node, I.d_slot, d_vec, s->d_ibuf);
  int total = nb;
  if (d_extra) {
    HIP_TRY(hipMemcpyAsync(s->d_ibuf + total, d_extra, (size_t)n_extra * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
    total += n_extra;
  }
  if (d_extra2) {
    HIP_TRY(hipMemcpyAsync(s->d_ibuf + total, d_extra2, (size_t)n_extra * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
    total += n_extra;
  }
  if (total == 0) return 0;
  TRY(call_allreduce(s, s->d_ibuf, total));
  launch_unpack(s->stream, I.n_loc, dim, I.d_node, I.d_slot, s->d_ibuf, d_vec);
  int o = nb;
  if (d_extra) {
    HIP_TRY(hipMemcpyAsync(d_extra, s->d_ibuf + o, (size_t)n_extra * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
    o += n_extra;
  }
  if (d_extra2)
    HIP_TRY(hipMemcpyAsync(d_extra2, s->d_ibuf + o, (size_t)n_extra * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
  return 0;
}
// sum over ranks of reduction slots only (element-wise), so every rank re-adds identical partials
int tlfea::parts_sum(tlfea_newton_t s, double* d_a, double* d_b) {
  if (!dist_on(s)) return 0;
  double* buf = s->halo.on ? s->halo.d_red : s->d_ibuf;
  HIP_TRY(hipMemcpyAsync(buf, d_a, (size_t)kNPart * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
  if (d_b) HIP_TRY(hipMemcpyAsync(buf + kNPart, d_b, (size_t)kNPart * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
  TRY(call_allreduce(s, buf, d_b ? 2 * kNPart : kNPart));
  HIP_TRY(hipMemcpyAsync(d_a, buf, (size_t)kNPart * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
  if (d_b) HIP_TRY(hipMemcpyAsync(d_b, buf + kNPart, (size_t)kNPart * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
  return 0;
}


// sum of squares (over ranks) left in s->d_scal[0]; no host synchronisation on the single-GPU path
int tlfea::device_sumsq_async(tlfea_newton_t s, const double* d_vec, const double* w, int n) {
  launch_norm2(s->stream, d_vec, w, n, part(s, 5), s->d_scal);
  if (dist_on(s)) {
    TRY(parts_sum(s, part(s, 5)));
    launch_sum_parts(s->stream, part(s, 5), s->d_scal);
  }
  return 0;
}
// one device scalar to the host through the pinned staging word
int tlfea::fetch_scalar(tlfea_newton_t s, const double* d_src, double* out) {
  HIP_TRY(hipMemcpyAsync(s->h_pin, d_src, sizeof(double), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  *out = s->h_pin[0];
  return 0;
}
int tlfea::fetch_scalar2(tlfea_newton_t s, const double* d_src, double* out0, double* out1) {
  HIP_TRY(hipMemcpyAsync(s->h_pin, d_src, 2 * sizeof(double), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  *out0 = s->h_pin[0];
  *out1 = s->h_pin[1];
  return 0;
}
int tlfea::device_norm(tlfea_newton_t s, const double* d_vec, const double* w, int n, double* out) {
  TRY(device_sumsq_async(s, d_vec, w, n));
  double ss = 0.0;
  TRY(fetch_scalar(s, s->d_scal, &ss));
  *out = std::sqrt(ss);
  return 0;
}

extern "C" int tlfea_newton_l2_norm(tlfea_newton_t s, const double* d_vec, int n, double* out) {
  return device_norm(s, d_vec, nullptr, n, out);
}

extern "C" long tlfea_newton_collectives(tlfea_newton_t s) { return s ? s->n_collectives : -1; }
extern "C" int tlfea_newton_get_comm_stats(tlfea_newton_t s, double* out8) {
  if (!s || !out8) return fail("null argument");
  const auto& h = s->halo;
  out8[0] = (double)h.n_exch;
  out8[1] = h.on ? (double)h.n_allred : (double)s->n_collectives;
  out8[2] = h.bytes_exch;
  out8[3] = h.bytes_allred;
  out8[4] = h.comm_ms;
  out8[5] = (double)h.n_cg_iters;
  out8[6] = (double)h.n_exch_cg;
  out8[7] = (double)h.n_allred_cg;
  return 0;
}
