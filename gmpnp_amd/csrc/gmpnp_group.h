// Mesh-partitioned Newton solve inside the library (include/gmpnp.h, "mesh-partitioned solve").
// Included at the end of gmpnp_api.hip: uses the handle type and the launch helpers defined there.
//
// One handle per rank on the rank's local mesh (owned + one ghost layer).  Per BiCGStab half-iteration and rank (half_of: which
// sums it all-reduces, which ghost rows it sends):
//     coarse kernel (scalars + coarse solve from all-reduced sums)  ->  tile kernel on the owned tiles (SpMV + vector updates)
//     ->  per-rank sums  ->  ONE all-reduce  +  ONE grouped send/recv of the ghost rows  ->  unpacking in the next coarse kernel
// in one routine per form (group_half; on the peer transport peer_half, or peer_half_x where the exchange rides in front of the
// next launch).  Every rank launches the same bursts (the burst schedule depends only on all-reduced quantities), so the
// collectives pair up.
//
// Transports: peer mailboxes (one process per rank; every collective is ONE k_peer_exchange launch that stores into the other
// ranks' IPC-mapped mailboxes — over xGMI between GPUs — and waits on its own flags: gmpnp_dist_kernels.h); RCCL (ncclAllReduce /
// grouped ncclSend+ncclRecv on the solver's stream, librccl.so loaded with dlopen on first use); host-staged callbacks; or, for
// a group that holds ALL ranks of the partition in one process, device copies between the handles on one shared stream.
#pragma once
#include <dlfcn.h>
#include <tuple>
#include <rccl/rccl.h>

namespace {

struct RcclApi {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
};

RcclApi* rccl_api(std::string* why) {
  static RcclApi api;
  static bool tried = false;
  static std::string err;
  if (!tried) {
    tried = true;
    // One RCCL per HIP runtime — and it has to be the one that sits on the HIP runtime THIS library is bound to.  A process
    // that imports PyTorch holds PyTorch's own libamdhip64.so and librccl.so next to the system's (same sonames): whichever
    // HIP runtime was loaded first serves this library, and an RCCL bound to the other one fails in ncclCommInitRank
    // ("unhandled cuda error").  So: find the file our HIP symbols come from and take the librccl.so in ITS directory
    // (torch/lib for PyTorch's pair, /opt/rocm/lib for the system's); by path, because a name or soname would match
    // whichever copy happens to be loaded already.
    std::string dir;
    { Dl_info info{};
      if (dladdr((void*)&hipGetDeviceCount, &info) && info.dli_fname) {
        dir = info.dli_fname;
        const size_t slash = dir.find_last_of('/');
        dir = slash == std::string::npos ? std::string() : dir.substr(0, slash);
      } }
    if (!dir.empty())
      for (const char* name : {"/librccl.so", "/librccl.so.1"}) {
        api.lib = dlopen((dir + name).c_str(), RTLD_NOW | RTLD_LOCAL);
        if (api.lib) break;
      }
    if (!api.lib)
      for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
        api.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
        if (api.lib) break;
      }
    if (!api.lib) err = std::string("librccl.so could not be loaded: ") + (dlerror() ? dlerror() : "?");
    else {
      auto sym = [&](const char* n) { void* p = dlsym(api.lib, n); if (!p && err.empty()) err = std::string("librccl.so lacks ") + n; return p; };
      api.GetUniqueId = (decltype(api.GetUniqueId))sym("ncclGetUniqueId");
      api.CommInitRank = (decltype(api.CommInitRank))sym("ncclCommInitRank");
      api.CommDestroy = (decltype(api.CommDestroy))sym("ncclCommDestroy");
      api.AllReduce = (decltype(api.AllReduce))sym("ncclAllReduce");
      api.Send = (decltype(api.Send))sym("ncclSend");
      api.Recv = (decltype(api.Recv))sym("ncclRecv");
      api.GroupStart = (decltype(api.GroupStart))sym("ncclGroupStart");
      api.GroupEnd = (decltype(api.GroupEnd))sym("ncclGroupEnd");
      api.GetErrorString = (decltype(api.GetErrorString))sym("ncclGetErrorString");
    }
  }
  if (!err.empty()) { if (why) *why = err; return nullptr; }
  return &api;
}

#define NCCL_TRY(api, expr)                                                                        \
  do {                                                                                             \
    ncclResult_t r__ = (expr);                                                                     \
    if (r__ != ncclSuccess)                                                                        \
      return fail(GMPNP_ERR_HIP, std::string(#expr) + ": " + ((api)->GetErrorString ? (api)->GetErrorString(r__) : "RCCL error")); \
  } while (0)

}  // namespace

struct gmpnp_comm {
  ncclComm_t comm = nullptr;
  int rank = 0, size = 1, device = 0;
};

struct gmpnp_group {
  std::vector<gmpnp_solver*> dom;       // local handles, ascending rank
  gmpnp_comm* comm = nullptr;           // RCCL transport (exactly one local handle) or nullptr (all ranks in this process)
  std::vector<hipStream_t> own_stream;  // in-process mode: the handles' own streams, given back at destroy
  std::vector<std::vector<int>> peer_slot;  // in-process mode: peer_slot[d][j] = index of d in the neighbour list of d's neighbour j
  GroupBurstHint burst; GroupCoarseReuse coarse;   // gmpnp_host_rules.h: first-burst sizing, cadence of the coarse operator (identical on every rank)
  // peer-mailbox transport (gmpnp_group_peer_begin / _connect): one k_peer_exchange launch per collective, no library, no host step
  bool peer = false, peer_connected = false;
  unsigned* peer_counter = nullptr;                        // arrival counter of k_dist_reduce_exchange (device)
  // exchange as the prologue of the next half-iteration's launch (k_half_a_x / k_half_b_x): possible when the launch WITH its exchange
  // workgroups is resident at once; exchange_form 0 = use it when possible, 1 = separate exchange launches (gmpnp_group_set_exchange_form)
  bool prologue_ok = false; int exchange_form = 0;
  size_t ll_red_off = 0, ll_halo_off = 0;   // flagged-word areas of the mailbox (gmpnp_dist_kernels.h, XchArgs)
  unsigned llseq = 0;                        // their sequence number (same on every rank: one per k_half_*_x launch)
  unsigned char* box = nullptr; size_t box_bytes = 0;   // own mailbox (uncached device memory)
  void* peer_map[kPeerMax] = {};                          // the other ranks' mailboxes as mapped here (IPC)
  PeerArgs pa{};
  int32_t* h_peer_err = nullptr;                          // pinned
  // caller-provided transport (gmpnp_group_create_hosted): collectives staged through pinned host memory
  bool hosted = false; gmpnp_host_transport_t host{};
  double* h_stage = nullptr; size_t h_stage_n = 0;   // pinned: [send | recv] or the all-reduce buffer
  std::vector<int64_t> off_s, cnt_s, off_r, cnt_r;
  // multilevel term (gmpnp_group_attach_coarse_group): the group of the next-coarser level's handles, and whether this group IS such
  // a level (driven by the finest group's solve, never by a solve of its own)
  gmpnp_group* ml_next = nullptr; bool ml_level = false;
};

namespace {

// ghost nodes a handle sends / receives
inline int n_send(const gmpnp_solver* s) { return s->send_ptr.empty() ? 0 : s->send_ptr.back(); }
inline int n_recv(const gmpnp_solver* s) { return s->recv_ptr.empty() ? 0 : s->recv_ptr.back(); }

// the peer transport's usability: connected, and no rank's flag late (the device reports that in pinned memory)
int peer_check(gmpnp_group* g) {
  if (!g->peer) return GMPNP_OK;
  if (!g->peer_connected) return fail(GMPNP_ERR_INVALID, "peer transport: gmpnp_group_peer_connect has not been called");
  if (*g->h_peer_err) return fail(GMPNP_ERR_HIP, "peer transport: a rank's flag did not arrive within 5 s (rank gone, or its process ended with an error)");
  return GMPNP_OK;
}

// ---- peer-mailbox transport: one launch = all-reduce of `n_red` doubles (in place) and / or the ghost rows (`per` doubles a node) ----
int peer_exchange(gmpnp_group* g, double* red, int n_red, size_t per) {
  gmpnp_solver* s = g->dom[0];
  if (int rc = peer_check(g)) return rc;
  if (n_red > g->pa.red_cap) return fail(GMPNP_ERR_INVALID, "peer transport: all-reduce larger than the mailbox slot");
  if ((int)per > g->pa.wmax) return fail(GMPNP_ERR_INVALID, "peer transport: ghost rows wider than the mailbox unit");
  g->pa.seq++;
  hipLaunchKernelGGL(k_peer_exchange, dim3(1), dim3(1024), 0, s->stream, g->pa, (const double*)red, n_red, red,
                     (const double*)s->sendbuf.p, s->recvbuf.p, (int)per);
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

// ---- flagged-word exchange (exchange-prologue launches, gmpnp_dist_kernels.h): whether the peer transport uses it, the arguments of
// the next one, and what its readers poll ----
inline bool flagged_words(const gmpnp_group* g) { return g->peer && g->prologue_ok && g->exchange_form != 1 && g->dom[0]->fused_half; }
// `h`: the half-iteration whose sums and rows it exchanges; `nsn` of its ghost nodes are sent
XchArgs make_xch_args(gmpnp_group* g, const Half& h, int par, int nsn) {
  gmpnp_solver* s = g->dom[0];
  XchArgs x{};
  const PeerArgs& a = g->pa;
  for (int q = 0; q < kPeerMax; ++q) x.box[q] = a.box[q];
  x.me = a.me; x.size = a.size; x.seq = ++g->llseq; x.ll_red_off = g->ll_red_off; x.ll_halo_off = g->ll_halo_off; x.red_cap = a.red_cap;
  x.n_nb = a.n_nb;
  for (int j = 0; j < a.n_nb; ++j) { x.nb_rank[j] = a.nb_rank[j]; x.peer_recv_ptr[j] = a.peer_recv_ptr[j]; }
  for (int j = 0; j <= a.n_nb; ++j) x.send_ptr[j] = a.send_ptr[j];
  x.phase = h.phase; x.par = par; x.nout = h.nout; x.nvec = h.nvec; x.nsn = nsn; x.nx = xch_workgroups(h.nout, nsn, h.nvec, s->nf);
  x.vecs = read_only(h.vecs); x.send_nodes = s->send_nodes.p;
  return x;
}
Ctx xch_ctx(gmpnp_group* g, const XchArgs& x) {
  gmpnp_solver* s = g->dom[0];
  Ctx cc = s->c;
  cc.xseq = x.seq; cc.xsize = x.size; cc.xcap = x.red_cap; cc.tile_cols_x = s->tile_cols_x.p;
  cc.xll_red = reinterpret_cast<const unsigned long long*>(g->box + g->ll_red_off);
  cc.xll_halo = reinterpret_cast<const unsigned long long*>(g->box + g->ll_halo_off);
  return cc;
}

// ---- collectives over the local handles ------------------------------------------------------------------------------------
template <class F>
int group_allreduce(gmpnp_group* g, F buf_of, int n) {
  if (g->peer) return peer_exchange(g, buf_of(g->dom[0]), n, 0);
  if (g->hosted) {
    gmpnp_solver* s = g->dom[0];
    if ((size_t)n > g->h_stage_n) return fail(GMPNP_ERR_INVALID, "hosted transport: staging buffer too small");
    HIP_TRY(hipMemcpyAsync(g->h_stage, buf_of(s), (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (g->host.allreduce(g->host.user, g->h_stage, n) != 0) return fail(GMPNP_ERR_HIP, "hosted transport: allreduce callback failed");
    HIP_TRY(hipMemcpyAsync(buf_of(s), g->h_stage, (size_t)n * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));   // the staging buffer is reused by the next collective
    return GMPNP_OK;
  }
  if (g->comm) {
    RcclApi* api = rccl_api(nullptr);
    gmpnp_solver* s = g->dom[0];
    NCCL_TRY(api, api->AllReduce(buf_of(s), buf_of(s), (size_t)n, ncclDouble, ncclSum, g->comm->comm, s->stream));
    return GMPNP_OK;
  }
  PtrList pl{};
  for (size_t d = 0; d < g->dom.size(); ++d) pl.p[d] = buf_of(g->dom[d]);
  hipLaunchKernelGGL(k_local_allreduce, dim3(grid_for(n, 256)), dim3(256), 0, g->dom[0]->stream, pl, (int)g->dom.size(), n);
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

// Ghost rows of up to four nodal arrays (`width` doubles per node) from their owners: pack, one message per neighbour, unpack.
// The messages themselves: what every rank packed into its send buffer (`per` doubles per node) travels to the neighbours'
// receive buffers — RCCL, host-staged callbacks, or device copies between the handles of one process.
int group_transfer(gmpnp_group* g, size_t per) {
  if (g->peer) return peer_exchange(g, nullptr, 0, per);
  if (g->hosted) {
    gmpnp_solver* s = g->dom[0];
    const size_t nb = s->nb_rank.size();
    if (nb) {
      const size_t ns = (size_t)n_send(s) * per, nr = (size_t)n_recv(s) * per;
      if (ns + nr > g->h_stage_n) return fail(GMPNP_ERR_INVALID, "hosted transport: staging buffer too small");
      double* hs = g->h_stage; double* hr = g->h_stage + ns;
      g->off_s.resize(nb); g->cnt_s.resize(nb); g->off_r.resize(nb); g->cnt_r.resize(nb);
      for (size_t j = 0; j < nb; ++j) {
        g->off_s[j] = (int64_t)s->send_ptr[j] * per; g->cnt_s[j] = (int64_t)(s->send_ptr[j + 1] - s->send_ptr[j]) * per;
        g->off_r[j] = (int64_t)s->recv_ptr[j] * per; g->cnt_r[j] = (int64_t)(s->recv_ptr[j + 1] - s->recv_ptr[j]) * per;
      }
      HIP_TRY(hipMemcpyAsync(hs, s->sendbuf.p, ns * sizeof(double), hipMemcpyDeviceToHost, s->stream));
      HIP_TRY(hipStreamSynchronize(s->stream));
      if (g->host.exchange(g->host.user, (int32_t)nb, s->nb_rank.data(), g->off_s.data(), g->cnt_s.data(), hs, g->off_r.data(), g->cnt_r.data(), hr) != 0)
        return fail(GMPNP_ERR_HIP, "hosted transport: exchange callback failed");
      HIP_TRY(hipMemcpyAsync(s->recvbuf.p, hr, nr * sizeof(double), hipMemcpyHostToDevice, s->stream));
      HIP_TRY(hipStreamSynchronize(s->stream));
    }
  } else if (g->comm) {
    RcclApi* api = rccl_api(nullptr);
    gmpnp_solver* s = g->dom[0];
    if (!s->nb_rank.empty()) {
      NCCL_TRY(api, api->GroupStart());
      for (size_t j = 0; j < s->nb_rank.size(); ++j) {
        const size_t ns = (size_t)(s->send_ptr[j + 1] - s->send_ptr[j]) * per, nr = (size_t)(s->recv_ptr[j + 1] - s->recv_ptr[j]) * per;
        if (ns) NCCL_TRY(api, api->Send(s->sendbuf.p + (size_t)s->send_ptr[j] * per, ns, ncclDouble, s->nb_rank[j], g->comm->comm, s->stream));
        if (nr) NCCL_TRY(api, api->Recv(s->recvbuf.p + (size_t)s->recv_ptr[j] * per, nr, ncclDouble, s->nb_rank[j], g->comm->comm, s->stream));
      }
      NCCL_TRY(api, api->GroupEnd());
    }
  } else {
    for (size_t d = 0; d < g->dom.size(); ++d) {
      gmpnp_solver* s = g->dom[d];
      for (size_t j = 0; j < s->nb_rank.size(); ++j) {
        gmpnp_solver* q = g->dom[s->nb_rank[j]];
        const int jj = g->peer_slot[d][j];
        const size_t ns = (size_t)(s->send_ptr[j + 1] - s->send_ptr[j]) * per;
        if (ns) HIP_TRY(hipMemcpyAsync(q->recvbuf.p + (size_t)q->recv_ptr[jj] * per, s->sendbuf.p + (size_t)s->send_ptr[j] * per,
                                       ns * sizeof(double), hipMemcpyDeviceToDevice, g->dom[0]->stream));
      }
    }
  }
  return GMPNP_OK;
}

// the all-reduce AND the ghost rows of a BiCGStab half-iteration: one launch on the peer transport, two collectives otherwise
template <class F>
int group_reduce_transfer(gmpnp_group* g, F buf_of, int n, size_t per) {
  if (g->peer) return peer_exchange(g, buf_of(g->dom[0]), n, per);
  int r = group_allreduce(g, buf_of, n); if (r) return r;
  return group_transfer(g, per);
}

inline VecListW one_vec(double* p) { VecListW w{}; w.p[0] = p; return w; }
template <class F>
int group_exchange(gmpnp_group* g, int width, int nvec, F vecs_of) {
  for (gmpnp_solver* s : g->dom) {
    const int nsn = n_send(s);
    if (nsn == 0) continue;
    hipLaunchKernelGGL(k_halo_pack, dim3(grid_for(nsn * nvec * width, 256)), dim3(256), 0, s->stream, read_only(vecs_of(s)), nvec, width,
                       (const int32_t*)s->send_nodes.p, nsn, s->sendbuf.p);
  }
  HIP_TRY(hipGetLastError());
  { int rt = group_transfer(g, (size_t)nvec * width); if (rt) return rt; }
  for (gmpnp_solver* s : g->dom) {
    const int nrn = n_recv(s);
    if (nrn == 0) continue;
    hipLaunchKernelGGL(k_halo_unpack, dim3(grid_for(nrn * nvec * width, 256)), dim3(256), 0, s->stream, vecs_of(s), nvec, width,
                       (const int32_t*)s->recv_nodes.p, nrn, (const double*)s->recvbuf.p);
  }
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

// all-reduces the first n doubles of every handle's red_norm and reads them into dom[0]'s h_red (synchronises the stream)
int group_sums_to_host(gmpnp_group* g, int n) {
  int rc = group_allreduce(g, [](gmpnp_solver* s) { return s->red_norm.p; }, n); if (rc) return rc;
  gmpnp_solver* s0 = g->dom[0];
  HIP_TRY(hipMemcpyAsync(s0->h_red, s0->red_norm.p, n * sizeof(double), hipMemcpyDeviceToHost, s0->stream));
  HIP_TRY(hipStreamSynchronize(s0->stream));
  return peer_check(g);
}

// (a, b), (a, a), (b, b) over all ranks' owned rows into dom[0]'s h_red; prep(s) launches what comes first on each handle
template <int NF, class F>
int group_dots3(gmpnp_group* g, DevBuf<double> gmpnp_solver::*a, DevBuf<double> gmpnp_solver::*b, F prep) {
  for (gmpnp_solver* s : g->dom) {
    int rc = prep(s); if (rc) return rc;
    hipLaunchKernelGGL(k_dots3, dim3(s->n_resblocks), dim3(kVecBlock), 0, s->stream, (const double*)(s->*a).p, (const double*)(s->*b).p, s->c.part_f,
                       (int)s->ndof, s->n_resblocks, s->t.own_node0 * NF, s->t.own_node1 * NF);
    hipLaunchKernelGGL(k_dots3_reduce, dim3(1), dim3(256), 0, s->stream, (const double*)s->c.part_f, s->n_resblocks, s->red_norm.p);
  }
  HIP_TRY(hipGetLastError());
  return group_sums_to_host(g, 3);
}

// ---- residual: ||b||_2 over all ranks' owned rows and the OR of the status bits -----------------------------------------------
template <int DIM, int NF>
int group_residual(gmpnp_group* g, double* norm, int* flags) {
  for (gmpnp_solver* s : g->dom) {
    int rc = launch_element<DIM, NF>(s, true); if (rc) return rc;
    rc = launch_res_gather<DIM, NF>(s); if (rc) return rc;
    hipLaunchKernelGGL(k_norm_reduce, dim3(1), dim3(256), 0, s->stream, (const double*)s->c.part_f, s->n_resblocks,
                       (const int32_t*)s->status.p, s->red_norm.p);
  }
  int rc = group_sums_to_host(g, 5); if (rc) return rc;
  gmpnp_solver* s0 = g->dom[0];
  *norm = std::sqrt(s0->h_red[0]);
  int f = 0;
  for (int b = 0; b < 4; ++b) if (s0->h_red[1 + b] > 0.0) f |= 1 << b;
  *flags = f;
  return GMPNP_OK;
}

// ---- preconditioner of the partitioned operator: node-block Jacobi (ghost blocks from their owners) + GLOBAL slab coarse space ----
template <int NF>
int group_setup(gmpnp_group* g, int mode, bool rebuild_coarse = true) {
  const int use_coarse = (mode == GMPNP_LINEAR_BICGSTAB_TWOLEVEL) ? 1 : 0;
  for (gmpnp_solver* s : g->dom) {
    s->c.use_coarse = use_coarse;
    hipLaunchKernelGGL((k_block_inverse<NF>), dim3(grid_for(s->t.nv, 4)), dim3(64), 0, s->stream, s->c);
  }
  // As = J Dinv needs the owners' inverse blocks at the ghost COLUMNS (the local ghost rows are identity rows)
  int rc = group_exchange(g, NF * NF, 1, [](gmpnp_solver* s) { return one_vec(s->Dinv.p); }); if (rc) return rc;
  for (gmpnp_solver* s : g->dom)
    hipLaunchKernelGGL((k_scale_columns<NF>), dim3(grid_for(s->c.n_work * kWave, kVecBlock)), dim3(kVecBlock), 0, s->stream, s->c);
  if (use_coarse && rebuild_coarse) {
    for (gmpnp_solver* s : g->dom) {
      const int n = s->ncoarse;
      launch_coarse_galerkin<NF>(s, s->c, s->stream);
      hipLaunchKernelGGL(k_zero_foreign_rows, dim3(grid_for(n * n, 256)), dim3(256), 0, s->stream, s->Ac.p, n, s->t.own_agg0 * NF, s->t.own_agg1 * NF);
    }
    const int n = g->dom[0]->ncoarse;
    rc = group_allreduce(g, [](gmpnp_solver* s) { return s->Ac.p; }, n * n); if (rc) return rc;   // ONE all-reduce per set-up
    for (gmpnp_solver* s : g->dom)
      hipLaunchKernelGGL((k_coarse_invert<NF>), dim3(1), dim3(512), coarse_lds_bytes(n, NF), s->stream, s->c);
  }
  HIP_TRY(hipGetLastError());
  for (gmpnp_solver* s : g->dom) { s->precond_valid = true; s->precond_mode = mode; }
  return GMPNP_OK;
}

// ---- multilevel term across the partitions (gmpnp_multilevel.h; serial form: gmpnp_api.hip ml_setup / ml_level_apply) ----------
// Every level is a group of partition handles of the same ranks (gmpnp_group_attach_coarse_group) over the finest group's
// transport; each level's collectives run over its own group, its launches in the finest handle's stream.  The transfers act on
// the OWNED rows (the existing kernels on the owned range): the restriction of an owned coarse vertex reads its children, local on
// the finer level, after a halo exchange of the finer vector; the prolongation of an owned fine vertex reads both parents, local on
// the coarser level (transfer ghosts), after a halo exchange of the coarser vector.  Ghost dofs are identity rows of a partition
// handle, so the finer side of a restriction masks with the TRUE Dirichlet flags (ml_tbc, k_pml_flags).  Every rank runs the same
// sequence of collectives (the V-cycle has a fixed shape), so the lock-step of the partitioned solve holds.
struct LevelStreams {   // the coarser levels' launches go to the finest handle's stream for the duration (as ml_setup does)
  std::vector<std::pair<gmpnp_solver*, hipStream_t>> keep;
  explicit LevelStreams(gmpnp_group* g) {
    hipStream_t st = g->dom[0]->stream;
    for (gmpnp_group* l = g->ml_next; l; l = l->ml_next)
      for (gmpnp_solver* s : l->dom) { keep.emplace_back(s, s->stream); s->stream = st; }
  }
  ~LevelStreams() { for (auto& k : keep) k.first->stream = k.second; }
};

// dst = scale_dst * dst + scale_x * M^-1 src on every handle's owned rows, (src, dst, scale_x) = io(s); M^-1 = Dinv (I + P Aci P^T)
// with the coarse sums all-reduced (`coarse`), Dinv alone otherwise
template <int NF, class F>
int group_minv(gmpnp_group* g, bool coarse, double scale_dst, F io) {
  if (coarse) {
    for (gmpnp_solver* s : g->dom) {
      hipLaunchKernelGGL((k_restrict<NF>), dim3(s->t.own_ntiles), dim3(kVecBlock), 0, s->stream, s->c, std::get<0>(io(s)), s->cpart_v0.p);
      hipLaunchKernelGGL(k_dist_reduce, dim3(s->ncoarse), dim3(256), 0, s->stream, s->c, 3, 0, s->red_i.p);
    }
    HIP_TRY(hipGetLastError());
    int rc = group_allreduce(g, [](gmpnp_solver* s) { return s->red_i.p; }, g->dom[0]->ncoarse); if (rc) return rc;
  }
  for (gmpnp_solver* s : g->dom) {
    const auto [src, dst, scale_x] = io(s);
    hipLaunchKernelGGL((k_minv_apply<NF>), dim3(s->t.own_ntiles), dim3(kKrylovThreads), 0, s->stream, s->c, src, (const double*)s->cpart_v0.p, dst,
                       scale_dst, scale_x, NewtonUpdate{nullptr, nullptr, 0.0, 0.0, 0.0}, (const double*)s->red_i.p);
  }
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

// true Dirichlet flags of a finer level's local dofs (the mask of its restriction), ghost rows from their owners
template <int NF>
int pml_masks(gmpnp_group* F) {
  for (gmpnp_solver* s : F->dom)
    hipLaunchKernelGGL(k_pml_flags, dim3(grid_for(s->ndof, 256)), dim3(256), 0, s->stream, (const uint8_t*)s->c.bcflag, s->t.own_node0 * NF,
                       s->t.own_node1 * NF, s->ml_tbd.p, (int)s->ndof);
  HIP_TRY(hipGetLastError());
  int rc = group_exchange(F, NF, 1, [](gmpnp_solver* s) { return one_vec(s->ml_tbd.p); }); if (rc) return rc;
  for (gmpnp_solver* s : F->dom)
    hipLaunchKernelGGL(k_pml_flags_bytes, dim3(grid_for(s->ndof, 256)), dim3(256), 0, s->stream, (const double*)s->ml_tbd.p, s->ml_tbc.p, (int)s->ndof);
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

// Once per preconditioner set-up: the state goes down by injection (owned rows, then the ghost rows from their owners), every level
// assembles its Jacobian and sets up its node-block inverse (ghost blocks from their owners); the coarsest level also its GLOBAL slab
// operator (one all-reduce), rebuilt with the finest level's cadence (`rebuild`: GroupCoarseReuse, identical on all ranks).
template <int DIM, int NF>
int group_ml_setup(gmpnp_group* g, bool rebuild) {
  for (gmpnp_group* F = g; F->ml_next; F = F->ml_next) {
    gmpnp_group* C = F->ml_next;
    int rc = pml_masks<NF>(F); if (rc) return rc;
    for (size_t d = 0; d < F->dom.size(); ++d) {
      gmpnp_solver* f = F->dom[d]; gmpnp_solver* c = C->dom[d];
      const int c0 = c->t.own_node0, nown = (c->t.own_node1 - c0) * NF;
      hipLaunchKernelGGL((k_ml_inject<NF>), dim3(grid_for(nown, 256)), dim3(256), 0, f->stream, (const double*)f->u.p, (const int32_t*)f->ml_copy.p + c0,
                         c->u.p + (size_t)c0 * NF, nown);
    }
    HIP_TRY(hipGetLastError());
    rc = group_exchange(C, NF, 1, [](gmpnp_solver* s) { return one_vec(s->u.p); }); if (rc) return rc;
    for (gmpnp_solver* c : C->dom) {
      rc = launch_element<DIM, NF>(c, true); if (rc) return rc;
      rc = launch_jac_gather<DIM, NF>(c); if (rc) return rc;
      c->jacobian_valid = true;
    }
    // intermediate levels smooth with node-block Jacobi alone (ml_mid_jacobi): no slab operator there
    rc = group_setup<NF>(C, C->ml_next ? GMPNP_LINEAR_BICGSTAB_JACOBI : GMPNP_LINEAR_BICGSTAB_TWOLEVEL, rebuild); if (rc) return rc;
  }
  return GMPNP_OK;
}

// ml_r of the next-coarser level's owned rows = mask_c P^T mask_f src (src: ghost rows current)
template <int NF, class F>
int pml_restrict(gmpnp_group* Fg, F src_of) {
  gmpnp_group* C = Fg->ml_next;
  for (size_t d = 0; d < Fg->dom.size(); ++d) {
    gmpnp_solver* f = Fg->dom[d]; gmpnp_solver* c = C->dom[d];
    const int c0 = c->t.own_node0, nown = (c->t.own_node1 - c0) * NF;
    hipLaunchKernelGGL((k_ml_restrict<NF>), dim3(grid_for(nown, 256)), dim3(256), 0, f->stream, src_of(f), (const uint8_t*)f->ml_tbc.p,
                       (const int32_t*)f->ml_child_ptr.p + c0, (const int32_t*)f->ml_child.p, (const uint8_t*)c->c.bcflag + (size_t)c0 * NF,
                       c->ml_r.p + (size_t)c0 * NF, nown);
  }
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

// L's handles hold the restricted residual in ml_r (owned rows); leaves ml_w = S_L ml_r on the owned rows: the V(1,1) cycle of
// ml_level_apply.  Collectives per cycle: a halo exchange in front of every SpMV, restriction and prolongation that reads ghost rows;
// one all-reduce per application of the coarsest level's slab coarse space.
template <int NF>
int pml_level_apply(gmpnp_group* L) {
  auto smooth = [&](bool from_r, double scale_dst) -> int {   // ml_w = scale_dst * ml_w + omega * M_L^-1 src, owned rows
    if (L->ml_next) {
      for (gmpnp_solver* s : L->dom) {
        const size_t o = (size_t)s->t.own_node0 * NF; const int nown = (s->t.own_node1 - s->t.own_node0) * NF;
        const double* src = from_r ? s->ml_r.p : s->ks.p;
        hipLaunchKernelGGL((k_ml_jacobi<NF>), dim3(grid_for(nown, 256)), dim3(256), 0, s->stream, (const double*)s->c.Dinv + o * NF, src + o,
                           s->ml_w.p + o, scale_dst, s->ml_omega, nown);
      }
      HIP_TRY(hipGetLastError());
      return GMPNP_OK;
    }
    return group_minv<NF>(L, true, scale_dst, [from_r](gmpnp_solver* s) {
      return std::make_tuple(from_r ? (const double*)s->ml_r.p : (const double*)s->ks.p, s->ml_w.p, s->ml_omega); });
  };
  auto residual = [&]() -> int {   // ks = ml_r - J_L ml_w on the owned rows (ghost columns of ml_w from their owners)
    int rc = group_exchange(L, NF, 1, [](gmpnp_solver* s) { return one_vec(s->ml_w.p); }); if (rc) return rc;
    for (gmpnp_solver* s : L->dom)
      hipLaunchKernelGGL((k_spmv_residual<NF>), dim3(s->t.own_ntiles), dim3(kKrylovThreads), 0, s->stream, s->c, (const double*)s->ml_w.p,
                         (const double*)s->ml_r.p, s->ks.p);
    HIP_TRY(hipGetLastError());
    return GMPNP_OK;
  };
  int rc = smooth(true, 0.0); if (rc) return rc;
  if (gmpnp_group* C = L->ml_next) {
    rc = residual(); if (rc) return rc;
    rc = group_exchange(L, NF, 1, [](gmpnp_solver* s) { return one_vec(s->ks.p); }); if (rc) return rc;
    rc = pml_restrict<NF>(L, [](gmpnp_solver* s) { return (const double*)s->ks.p; }); if (rc) return rc;
    rc = pml_level_apply<NF>(C); if (rc) return rc;
    rc = group_exchange(C, NF, 1, [](gmpnp_solver* s) { return one_vec(s->ml_w.p); }); if (rc) return rc;
    for (size_t d = 0; d < L->dom.size(); ++d) {
      gmpnp_solver* s = L->dom[d]; gmpnp_solver* c = C->dom[d];
      const int o = s->t.own_node0, nown = (s->t.own_node1 - o) * NF;
      hipLaunchKernelGGL((k_ml_prolong_add<NF>), dim3(grid_for(nown, 256)), dim3(256), 0, s->stream, (const double*)c->ml_w.p, (const int32_t*)s->ml_par.p + 2 * (size_t)o,
                         (const uint8_t*)s->c.bcflag + (size_t)o * NF, s->ml_w.p + (size_t)o * NF, nown);
    }
    HIP_TRY(hipGetLastError());
    rc = residual(); if (rc) return rc;
    rc = smooth(false, 1.0); if (rc) return rc;
  } else {
    for (int k = 1; k < L->dom[0]->ml_sweeps; ++k) { rc = residual(); if (rc) return rc; rc = smooth(false, 1.0); if (rc) return rc; }
  }
  return GMPNP_OK;
}

// coarse part of T src on the finest level (src: ghost rows current): leaves S P^T src in the next level's ml_w, ghost rows included
template <int NF, class F>
int pml_correction(gmpnp_group* g, F src_of) {
  int rc = pml_restrict<NF>(g, src_of); if (rc) return rc;
  rc = pml_level_apply<NF>(g->ml_next); if (rc) return rc;
  return group_exchange(g->ml_next, NF, 1, [](gmpnp_solver* s) { return one_vec(s->ml_w.p); });
}

// z = vec + theta D T vec on the owned rows (k_ml_stage masks the ghost rows, whose D is an identity block here), then z's ghost
// rows from their owners: the operand the materialised tile kernel stages
template <int NF, class F>
int pml_stage(gmpnp_group* g, F vec_of) {
  int rc = pml_correction<NF>(g, vec_of); if (rc) return rc;
  for (size_t d = 0; d < g->dom.size(); ++d) {
    gmpnp_solver* s = g->dom[d];
    hipLaunchKernelGGL((k_ml_stage<NF>), dim3(grid_for(s->ndof, kMlStageNodes * NF)), dim3(kMlStageNodes * NF), 0, s->stream, s->c,
                       (const double*)g->ml_next->dom[d]->ml_w.p, (const int32_t*)s->ml_par.p, vec_of(s), s->ml_z.p, s->ml_theta);
  }
  HIP_TRY(hipGetLastError());
  return group_exchange(g, NF, 1, [](gmpnp_solver* s) { return one_vec(s->ml_z.p); });
}

// ---- BiCGStab across the ranks: one half-iteration (H: A = 0, B = 1; half_of says what it all-reduces and sends) per form ----------
// Over the transport's own collectives, per rank: [coarse kernel + unpacking of the ghost rows the previous half sent], tile kernel,
// [per-rank sums + packing of the ghost rows to send]; then the all-reduce and the grouped send/recv.  With a multilevel term the
// tile kernel is the materialised one (launch_half): k_vec_* writes the vector, and the staged operand z = vec + theta D T vec
// comes out of the V-cycle across the partitioned levels (pml_stage).
template <int NF, int H>
int group_half(gmpnp_group* g, int k) {
  const int par = k & 1;
  const unsigned cg = std::max(1, g->dom[0]->t.nagg);
  auto tile_pack = [&](gmpnp_solver* s) {
    Ctx cc = s->c;
    if (g->ml_next) {
      (H == 0 ? cc.stage_a : cc.stage_b) = s->ml_z.p;
      if (H == 0) hipLaunchKernelGGL((k_bicg_a_mat<NF>), dim3(s->t.own_ntiles), dim3(kKrylovThreads), 0, s->stream, cc, k);
      else hipLaunchKernelGGL((k_bicg_b_mat<NF>), dim3(s->t.own_ntiles), dim3(kKrylovThreads), 0, s->stream, cc, k);
    } else if (H == 0) hipLaunchKernelGGL((k_bicg_a<NF>), dim3(s->t.own_ntiles), dim3(kKrylovThreads), 0, s->stream, cc, k);
    else hipLaunchKernelGGL((k_bicg_b<NF>), dim3(s->t.own_ntiles), dim3(kKrylovThreads), 0, s->stream, cc, k);
    const Half out = half_of(s, H, par);
    const int nsn = n_send(s);
    hipLaunchKernelGGL(k_dist_reduce_pack, dim3(out.nout + grid_for(nsn * out.nvec * NF, 256)), dim3(256), 0, s->stream, s->c, out.phase, par, out.red,
                       out.nout, read_only(out.vecs), out.nvec, (const int32_t*)s->send_nodes.p, nsn, s->sendbuf.p, NF);
  };
  for (gmpnp_solver* s : g->dom) {
    const Half in = half_of(s, 1 - H, par);
    const int un = (H == 1 || k > 0) ? n_recv(s) : 0;   // (nothing pending before the first iteration)
    const dim3 ug(cg + grid_for(un * in.nvec * NF, kCoarseThreads));
    if (H == 0) hipLaunchKernelGGL((k_coarse_a_unpack<NF>), ug, dim3(kCoarseThreads), 0, s->stream, s->c, k, in.vecs, in.nvec, (const int32_t*)s->recv_nodes.p, un,
                                   (const double*)s->recvbuf.p);
    else hipLaunchKernelGGL((k_coarse_b_unpack<NF>), ug, dim3(kCoarseThreads), 0, s->stream, s->c, k, in.vecs, in.nvec, (const int32_t*)s->recv_nodes.p, un,
                            (const double*)s->recvbuf.p);
    if (!g->ml_next) tile_pack(s);
    else if (H == 0) hipLaunchKernelGGL(k_vec_a, dim3(grid_for(s->ndof, 256)), dim3(256), 0, s->stream, s->c, k);
    else hipLaunchKernelGGL(k_vec_b, dim3(grid_for(s->ndof, 256)), dim3(256), 0, s->stream, s->c, k);
  }
  if (g->ml_next) {
    HIP_TRY(hipGetLastError());
    int rc = pml_stage<NF>(g, [par](gmpnp_solver* s) { return H == 0 ? (const double*)s->c.kp[par] : (const double*)s->ks.p; }); if (rc) return rc;
    for (gmpnp_solver* s : g->dom) tile_pack(s);
  }
  const Half out = half_of(g->dom[0], H, par);
  return group_reduce_transfer(g, [par](gmpnp_solver* s) { return half_of(s, H, par).red; }, out.nout, (size_t)out.nvec * NF);
}

// Peer transport, separate launches: coarse kernel and tile kernel (one launch where the coarse workgroups ride in front of the
// tile workgroups), then ONE k_dist_reduce_exchange: the sums, the ghost rows and their exchange; the received rows are in place and
// the sums all-reduced when it ends.  No library call.
template <int NF, int H>
int peer_half(gmpnp_group* g, int k) {
  gmpnp_solver* s = g->dom[0];
  const int par = k & 1, nsn = n_send(s);
  const dim3 cg(std::max(1, s->t.nagg)), fg(s->t.nagg + s->t.own_ntiles);
  if (s->fused_half) {
    if (H == 0) hipLaunchKernelGGL((k_half_a<NF>), fg, dim3(kKrylovThreads), 0, s->stream, s->c, k, (unsigned)(++s->fused_seq));
    else hipLaunchKernelGGL((k_half_b<NF>), fg, dim3(kKrylovThreads), 0, s->stream, s->c, k, (unsigned)(++s->fused_seq));
  } else if (H == 0) {
    hipLaunchKernelGGL((k_coarse_a<NF>), cg, dim3(kCoarseThreads), 0, s->stream, s->c, k);
    hipLaunchKernelGGL((k_bicg_a<NF>), dim3(s->t.own_ntiles), dim3(kKrylovThreads), 0, s->stream, s->c, k);
  } else {
    hipLaunchKernelGGL((k_coarse_b<NF>), cg, dim3(kCoarseThreads), 0, s->stream, s->c, k);
    hipLaunchKernelGGL((k_bicg_b<NF>), dim3(s->t.own_ntiles), dim3(kKrylovThreads), 0, s->stream, s->c, k);
  }
  const Half out = half_of(s, H, par);
  g->pa.seq++;
  hipLaunchKernelGGL(k_dist_reduce_exchange, dim3(out.nout + grid_for(nsn * out.nvec * NF, 256)), dim3(256), 0, s->stream, s->c, out.phase, par, out.red,
                     out.nout, out.vecs, out.nvec, NF, (const int32_t*)s->send_nodes.p, nsn, (const int32_t*)s->recv_nodes.p, g->pa, g->peer_counter);
  return GMPNP_OK;
}

// Peer transport, flagged words: ONE launch per half-iteration, the exchange of the previous half's sums and boundary rows riding in
// front of its coarse workgroups (gmpnp_dist_kernels.h, "exchange as the prologue").  A(0) needs nothing exchanged (the start-up
// collectives did it).
template <int NF, int H>
int peer_half_x(gmpnp_group* g, int k) {
  gmpnp_solver* s = g->dom[0];
  const unsigned fg = s->t.nagg + s->t.own_ntiles;
  if (H == 0 && k == 0) {
    hipLaunchKernelGGL((k_half_a<NF>), dim3(fg), dim3(kKrylovThreads), 0, s->stream, s->c, k, (unsigned)(++s->fused_seq));
    return GMPNP_OK;
  }
  const XchArgs x = make_xch_args(g, half_of(s, 1 - H, k & 1), k & 1, n_send(s));
  const Ctx cc = xch_ctx(g, x);
  if (H == 0) hipLaunchKernelGGL((k_half_a_x<NF>), dim3(x.nx + fg), dim3(kKrylovThreads), 0, s->stream, cc, k, (unsigned)(++s->fused_seq), x);
  else hipLaunchKernelGGL((k_half_b_x<NF>), dim3(x.nx + fg), dim3(kKrylovThreads), 0, s->stream, cc, k, (unsigned)(++s->fused_seq), x);
  return GMPNP_OK;
}

// rhs in kr (owned rows; k_res_gather left it there), ||rhs|| = bnorm (global); leaves y in ky.  Nothing of the loop runs on the host
// except the launches; the host reads the device's verdict once per burst.
// random_shadow: the shadow vector of this pass is each handle's krand (filled by the caller) and (rhat, r_0) = shadow_rho0
template <int NF>
int group_krylov(gmpnp_group* g, int mode, double bnorm, double rtol, double atol, int maxit, gmpnp_linear_stats_t* st, bool sized_by_previous = true,
                 bool random_shadow = false, double shadow_rho0 = 0.0, int predicted = 0) {
  const int use_coarse = (mode == GMPNP_LINEAR_BICGSTAB_TWOLEVEL) ? 1 : 0;
  const int n = g->dom[0]->ncoarse;
  const KrylovScalars init = krylov_start(random_shadow ? shadow_rho0 : bnorm * bnorm, bnorm, rtol, atol, maxit);
  for (gmpnp_solver* s : g->dom) {
    s->c.use_coarse = use_coarse;
    hipLaunchKernelGGL((k_krylov_init<NF>), dim3(s->t.own_ntiles), dim3(kVecBlock), 0, s->stream, s->c,
                       random_shadow ? (const double*)s->krand.p : (const double*)nullptr, init, s->cpart_v1.p);
    if (use_coarse) hipLaunchKernelGGL(k_dist_reduce, dim3(n), dim3(256), 0, s->stream, s->c, 0, 0, s->red_i.p);
  }
  HIP_TRY(hipGetLastError());
  int rc;
  if (use_coarse) { rc = group_allreduce(g, [](gmpnp_solver* s) { return s->red_i.p; }, n); if (rc) return rc; }
  rc = group_exchange(g, NF, 1, [](gmpnp_solver* s) { return one_vec(s->kr.p); }); if (rc) return rc;   // p_0 = r_0 at the ghost columns
  const bool flagged = flagged_words(g);
  KrylovScalars res = init;
  int k = 0;
  auto iteration = [&]() -> int {
    int r = peer_check(g);
    if (!r) r = flagged ? peer_half_x<NF, 0>(g, k) : g->peer ? peer_half<NF, 0>(g, k) : group_half<NF, 0>(g, k);
    if (!r) r = flagged ? peer_half_x<NF, 1>(g, k) : g->peer ? peer_half<NF, 1>(g, k) : group_half<NF, 1>(g, k);
    if (r) return r;
    ++k;
    HIP_TRY(hipGetLastError());
    return GMPNP_OK;
  };
  if (!res.done) {
    // Bursts: every rank launches the SAME number of iterations (the schedule depends only on earlier solves' counts and
    // on `done`, both identical on all ranks), then reads the device's verdict.  Iterations launched behind the end of the
    // solve exit at their first instruction; their collectives still pair up.
    int burst = g->burst.first(predicted, sized_by_previous);
    gmpnp_solver* s0 = g->dom[0];
    while (true) {
      for (int it = 0; it < burst; ++it) { rc = iteration(); if (rc) return rc; }
      HIP_TRY(hipMemcpyAsync(&s0->h_scal[0], s0->scal.p, sizeof(KrylovScalars), hipMemcpyDeviceToHost, s0->stream));
      for (gmpnp_solver* s : g->dom) HIP_TRY(hipStreamSynchronize(s->stream));
      rc = peer_check(g); if (rc) return rc;
      res = s0->h_scal[0];
      if (res.done) break;
      if (k > maxit + 8) break;
      burst = 4;
    }
  }
  g->burst.solve_done(res.iters);
  for (gmpnp_solver* s : g->dom) s->last_done = res.done;
  return krylov_verdict(res, bnorm, st, "partitioned BiCGStab");
}

// x = Dinv (I + P Aci P^T) y on the owned rows, ghost rows from their owners, then u -= omega x on every local row
template <int NF>
int group_update(gmpnp_group* g, int mode, double omega, bool add_to_start) {
  int rc = group_minv<NF>(g, mode == GMPNP_LINEAR_BICGSTAB_TWOLEVEL, add_to_start ? 1.0 : 0.0,
                          [](gmpnp_solver* s) { return std::make_tuple((const double*)s->ky.p, s->kx.p, 1.0); });
  if (rc) return rc;
  if (g->ml_next) {   // x += theta T y on the owned rows (the multilevel term of M^-1 applied to the Krylov solution), as the serial solve does
    rc = group_exchange(g, NF, 1, [](gmpnp_solver* s) { return one_vec(s->ky.p); }); if (rc) return rc;
    rc = pml_correction<NF>(g, [](gmpnp_solver* s) { return (const double*)s->ky.p; }); if (rc) return rc;
    for (size_t d = 0; d < g->dom.size(); ++d) {
      gmpnp_solver* s = g->dom[d];
      hipLaunchKernelGGL((k_ml_add_solution<NF>), dim3(grid_for(s->ndof, 256)), dim3(256), 0, s->stream, s->c, (const double*)g->ml_next->dom[d]->ml_w.p,
                         (const int32_t*)s->ml_par.p, s->kx.p, s->ml_theta);
    }
  }
  rc = group_exchange(g, NF, 1, [](gmpnp_solver* s) { return one_vec(s->kx.p); }); if (rc) return rc;
  for (gmpnp_solver* s : g->dom)
    hipLaunchKernelGGL(k_axpy, dim3(grid_for(s->ndof, 256)), dim3(256), 0, s->stream, s->u.p, (const double*)s->kx.p, -omega, (int)s->ndof);
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

// The linear solve of one Newton iteration (J dx = F, ||F|| = r, preconditioner set up): dx is left for group_update, `warm` says
// whether it adds to the predicted start in kx.  Counts the BiCGStab iterations into st and `iters`, also those of a failed solve.
struct GroupLinearStep { bool warm = false; int iters = 0; };

template <int NF>
int group_linear_step(gmpnp_group* g, const gmpnp_newton_options_t& o, gmpnp_newton_stats_t& st, double r, GroupLinearStep* out) {
  int rc = GMPNP_OK;
  gmpnp_linear_stats_t ls{};
  // Warm start, as in the single-GPU Newton: the predicted start (gmpnp_host_rules.h) is accepted when it removes at least half
  // of the residual (one SpMV, three all-reduced dot products, a decision identical on every rank), and BiCGStab then only
  // has to remove b - J x0, to the SAME absolute target.
  const double tol_abs = std::max(o.krylov_relative_tolerance * r, o.krylov_absolute_tolerance);
  const std::pair<double, double> w = predicted_start(g->dom[0]->cfg.warm_start, 1.0 - o.relaxation_parameter, st.iterations);
  bool warm = false; double rstart = r;
  if ((w.first != 0.0 || w.second != 0.0) && r > 0.0) {
    rc = group_dots3<NF>(g, &gmpnp_solver::kt, &gmpnp_solver::kb, [&](gmpnp_solver* s) -> int {
      hipLaunchKernelGGL(k_warm_start, dim3(grid_for(s->ndof, 256)), dim3(256), 0, s->stream, s->kx.p, s->kxp.p, w.first, w.second, (int)s->ndof);
      hipLaunchKernelGGL((k_spmv_plain<NF>), dim3(s->t.own_ntiles), dim3(kKrylovThreads), 0, s->stream, s->c, (const double*)s->kx.p, s->kt.p);
      return GMPNP_OK;
    });
    if (rc) return rc;
    const double* h = g->dom[0]->h_red;
    if (accept_predicted_start(h[0], h[1], h[2], &rstart)) {
      for (gmpnp_solver* s : g->dom)
        hipLaunchKernelGGL(k_start_residual, dim3(grid_for(s->ndof, 256)), dim3(256), 0, s->stream, s->kr.p, (const double*)s->kb.p, (const double*)s->kt.p, (int)s->ndof);
      warm = true;
    }
  }
  int kry_total = 0;
  if (warm && rstart <= tol_abs) { ls.converged = 1; ls.residual_norm = rstart; for (gmpnp_solver* s : g->dom) HIP_TRY(hipMemsetAsync(s->ky.p, 0, s->ndof * sizeof(double), s->stream)); }
  else {
    // BiCGStab can break down, or spike past 1e5 times its starting residual, on one (right-hand side, shadow vector) pair
    // and run smoothly on another: such a pass is thrown away and repeated with a pseudo-random shadow vector — the
    // second time also without the predicted start — as the single-GPU solver does (gmpnp_api.hip, linear_solve).  The
    // verdict comes from all-reduced sums, so every rank takes the same branch.
    bool random_shadow = false; double rho0 = 0.0;
    for (int attempt = 0;; ++attempt) {
      const int hist = g->burst.predicted(attempt, g->dom[0]->state_jumped, st.iterations);
      rc = group_krylov<NF>(g, o.linear_solver, rstart, warm ? 0.0 : o.krylov_relative_tolerance, warm ? tol_abs : o.krylov_absolute_tolerance,
                            o.krylov_maximum_iterations, &ls, st.iterations > 0 && attempt == 0, random_shadow, rho0, hist);
      g->burst.record(attempt, rc == GMPNP_OK, st.iterations, ls.iterations);
      kry_total += ls.iterations;
      if (rc != GMPNP_ERR_LINEAR || attempt >= 4 || g->dom[0]->last_done != 3) break;
      if (warm && attempt >= 1) { warm = false; rstart = r; }
      const int r2 = group_dots3<NF>(g, &gmpnp_solver::krand, &gmpnp_solver::kr, [&](gmpnp_solver* s) -> int {
        const int nd = s->ndof;
        HIP_TRY(hipMemsetAsync(s->status.p, 0, sizeof(int32_t), s->stream));
        if (warm) {   // kr = b - J x0 again (kt was a work vector of the lost pass)
          hipLaunchKernelGGL((k_spmv_plain<NF>), dim3(s->t.own_ntiles), dim3(kKrylovThreads), 0, s->stream, s->c, (const double*)s->kx.p, s->kt.p);
          hipLaunchKernelGGL(k_start_residual, dim3(grid_for(nd, 256)), dim3(256), 0, s->stream, s->kr.p, (const double*)s->kb.p, (const double*)s->kt.p, nd);
        } else HIP_TRY(hipMemcpyAsync(s->kr.p, s->kb.p, nd * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
        hipLaunchKernelGGL(k_fill_hash, dim3(grid_for(nd, 256)), dim3(256), 0, s->stream, s->krand.p, (unsigned)((attempt + 1) * 2654435761u), nd);
        return GMPNP_OK;
      });
      if (r2) return r2;
      rho0 = g->dom[0]->h_red[0]; random_shadow = true;   // (rhat, r_0) of the new shadow vector, over all ranks' owned rows
    }
    ls.iterations = kry_total;
  }
  if (st.iterations < GMPNP_MAX_NEWTON_HISTORY) st.krylov_per_iteration[st.iterations] = ls.iterations;
  st.krylov_iterations += ls.iterations;
  out->warm = warm; out->iters = ls.iterations;
  return rc;
}

template <int DIM, int NF>
int group_newton(gmpnp_group* g, const gmpnp_newton_options_t& o, gmpnp_newton_stats_t& st) {
  const double t0 = now_ms();
  for (gmpnp_solver* s : g->dom) HIP_TRY(hipMemsetAsync(s->status.p, 0, sizeof(int32_t), s->stream));
  // ghost values of u and u_n are the owners' values from here on (the caller's scatter normally made them so already)
  int rc = group_exchange(g, NF, 2, [](gmpnp_solver* s) { VecListW w{}; w.p[0] = s->u.p; w.p[1] = s->un.p; return w; }); if (rc) return rc;
  double r = 0.0; int flags = 0;
  rc = group_residual<DIM, NF>(g, &r, &flags); if (rc) return rc;
  NewtonJudge judge(o, st, g->dom[0]->cfg.strict_steric != 0);   // r and flags are all-reduced: the same verdict on every rank
  NewtonJudge::Verdict v = judge.first(r, flags);
  const bool two_level = o.linear_solver == GMPNP_LINEAR_BICGSTAB_TWOLEVEL;
  while (v == NewtonJudge::go_on) {
    for (gmpnp_solver* s : g->dom) { rc = launch_jac_gather<DIM, NF>(s); if (rc) return rc; s->jacobian_valid = true; }
    const bool rebuild = two_level && g->coarse.rebuild(st.iterations, g->dom[0]->state_jumped);
    rc = group_setup<NF>(g, o.linear_solver, rebuild); if (rc) return rc;
    if (g->ml_next) { rc = group_ml_setup<DIM, NF>(g, rebuild); if (rc) return rc; }
    GroupLinearStep lin;
    rc = group_linear_step<NF>(g, o, st, r, &lin); if (rc) return rc;
    if (two_level) g->coarse.solved(rebuild, lin.iters);
    rc = group_update<NF>(g, o.linear_solver, o.relaxation_parameter, lin.warm); if (rc) return rc;
    st.iterations++;
    rc = group_residual<DIM, NF>(g, &r, &flags); if (rc) return rc;
    v = judge.next(r, flags);
  }
  if (v == NewtonJudge::failed) return fail(judge.code, judge.message);
  for (gmpnp_solver* s : g->dom) { s->state_jumped = false; s->x0.left(false); }
  st.ms_total = now_ms() - t0;
  return v == NewtonJudge::converged ? GMPNP_OK : fail(judge.code, judge.message);
}

}  // namespace

extern "C" {

int gmpnp_comm_unique_id(char id[GMPNP_COMM_ID_BYTES]) {
  static_assert(GMPNP_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "id size");
  if (!id) return fail(GMPNP_ERR_INVALID, "NULL argument");
  std::string why;
  RcclApi* api = rccl_api(&why);
  if (!api) return fail(GMPNP_ERR_HIP, why);
  ncclUniqueId u;
  NCCL_TRY(api, api->GetUniqueId(&u));
  std::memcpy(id, u.internal, NCCL_UNIQUE_ID_BYTES);
  return GMPNP_OK;
}

int gmpnp_comm_create(const char id[GMPNP_COMM_ID_BYTES], int32_t rank, int32_t size, int32_t device_id, gmpnp_comm** out) {
  if (!id || !out || size < 1 || rank < 0 || rank >= size) return fail(GMPNP_ERR_INVALID, "bad arguments");
  *out = nullptr;
  std::string why;
  RcclApi* api = rccl_api(&why);
  if (!api) return fail(GMPNP_ERR_HIP, why);
  HIP_TRY(hipSetDevice(device_id));
  ncclUniqueId u;
  std::memcpy(u.internal, id, NCCL_UNIQUE_ID_BYTES);
  std::unique_ptr<gmpnp_comm> c(new gmpnp_comm);
  c->rank = rank; c->size = size; c->device = device_id;
  NCCL_TRY(api, api->CommInitRank(&c->comm, size, u, rank));
  *out = c.release();
  return GMPNP_OK;
}

// Round trip through every RCCL entry point the partitioned solve uses, on this rank alone: n doubles sent to OUR OWN rank
// and received back inside one group (RCCL pairs a send-to-self with the matching receive), then all-reduced.  A single-GPU
// box cannot host a second rank (RCCL refuses two ranks on one device), so this is how the send/receive bindings get
// exercised there.  Collective in the sense that every rank of the communicator has to call it (the all-reduce).
int gmpnp_comm_selftest(gmpnp_comm* c, int32_t n, double* max_error) {
  if (!c || n < 1 || !max_error) return fail(GMPNP_ERR_INVALID, "bad arguments");
  RcclApi* api = rccl_api(nullptr);
  if (!api) return fail(GMPNP_ERR_HIP, "RCCL not loaded");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st; HIP_TRY(hipStreamCreate(&st));
  DevBuf<double> a, b;
  HIP_TRY(a.alloc(n)); HIP_TRY(b.alloc(n));
  std::vector<double> h(n), back(n);
  for (int i = 0; i < n; ++i) h[i] = 0.25 * i - 3.0 + c->rank;
  HIP_TRY(hipMemcpyAsync(a.p, h.data(), n * sizeof(double), hipMemcpyHostToDevice, st));
  NCCL_TRY(api, api->GroupStart());
  NCCL_TRY(api, api->Send(a.p, (size_t)n, ncclDouble, c->rank, c->comm, st));
  NCCL_TRY(api, api->Recv(b.p, (size_t)n, ncclDouble, c->rank, c->comm, st));
  NCCL_TRY(api, api->GroupEnd());
  NCCL_TRY(api, api->AllReduce(b.p, b.p, (size_t)n, ncclDouble, ncclSum, c->comm, st));
  HIP_TRY(hipMemcpyAsync(back.data(), b.p, n * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  (void)hipStreamDestroy(st);
  double err = 0.0;
  for (int i = 0; i < n; ++i) {   // sum over ranks r of (0.25 i - 3 + r)
    const double want = c->size * (0.25 * i - 3.0) + 0.5 * c->size * (c->size - 1);
    err = std::max(err, std::fabs(back[i] - want));
  }
  *max_error = err;
  return GMPNP_OK;
}

void gmpnp_comm_destroy(gmpnp_comm* c) {
  if (!c) return;
  RcclApi* api = rccl_api(nullptr);
  if (api && c->comm) { (void)hipSetDevice(c->device); (void)api->CommDestroy(c->comm); }
  delete c;
}

int gmpnp_group_create(int32_t n_local, gmpnp_solver* const* handles, gmpnp_comm* comm, gmpnp_group** out) {
  if (n_local < 1 || !handles || !out) return fail(GMPNP_ERR_INVALID, "bad arguments");
  *out = nullptr;
  std::unique_ptr<gmpnp_group> g(new gmpnp_group);
  for (int d = 0; d < n_local; ++d) {
    gmpnp_solver* s = handles[d];
    if (!s || !s->partitioned) return fail(GMPNP_ERR_INVALID, "group members must come from gmpnp_create_partition");
    g->dom.push_back(s);
  }
  gmpnp_solver* s0 = g->dom[0];
  for (gmpnp_solver* s : g->dom)
    if (s->part_size != s0->part_size || s->ncoarse != s0->ncoarse || s->nf != s0->nf || s->opts.device_id != s0->opts.device_id)
      return fail(GMPNP_ERR_INVALID, "group members disagree on partition size, coarse space, fields or device");
  if (comm) {
    if (n_local != 1) return fail(GMPNP_ERR_INVALID, "with a communicator a process drives exactly one partition handle");
    if (comm->size != s0->part_size || comm->rank != s0->part_rank) return fail(GMPNP_ERR_INVALID, "communicator rank/size differ from the partition's");
    g->comm = comm;
  } else {
    if (n_local != s0->part_size || n_local > 8) return fail(GMPNP_ERR_INVALID, "without a communicator the group must hold every rank of the partition (at most 8)");
    for (int d = 0; d < n_local; ++d) if (g->dom[d]->part_rank != d) return fail(GMPNP_ERR_INVALID, "handles must be given in rank order");
    g->peer_slot.resize(n_local);
    for (int d = 0; d < n_local; ++d) {
      gmpnp_solver* s = g->dom[d];
      for (size_t j = 0; j < s->nb_rank.size(); ++j) {
        gmpnp_solver* q = g->dom[s->nb_rank[j]];
        int jj = -1;
        for (size_t z = 0; z < q->nb_rank.size(); ++z) if (q->nb_rank[z] == d) jj = (int)z;
        if (jj < 0 || (q->recv_ptr[jj + 1] - q->recv_ptr[jj]) != (s->send_ptr[j + 1] - s->send_ptr[j]))
          return fail(GMPNP_ERR_INVALID, "halo plans of two neighbouring ranks do not match");
        g->peer_slot[d].push_back(jj);
      }
    }
    // one stream for all handles of the process: their launches and the copies between them are ordered without events
    HIP_TRY(hipSetDevice(s0->opts.device_id));
    g->own_stream.resize(n_local, nullptr);
    for (int d = 1; d < n_local; ++d) {
      HIP_TRY(hipStreamSynchronize(g->dom[d]->stream));
      g->own_stream[d] = g->dom[d]->stream; g->dom[d]->stream = s0->stream;
    }
  }
  *out = g.release();
  return GMPNP_OK;
}

int gmpnp_group_create_hosted(gmpnp_solver* handle, const gmpnp_host_transport_t* t, gmpnp_group** out) {
  if (!handle || !t || !out || !t->allreduce || !t->exchange) return fail(GMPNP_ERR_INVALID, "bad arguments");
  *out = nullptr;
  if (!handle->partitioned) return fail(GMPNP_ERR_INVALID, "group members must come from gmpnp_create_partition");
  if (t->size != handle->part_size || t->rank != handle->part_rank) return fail(GMPNP_ERR_INVALID, "transport rank/size differ from the partition's");
  std::unique_ptr<gmpnp_group> g(new gmpnp_group);
  g->dom.push_back(handle);
  g->hosted = true; g->host = *t;
  const size_t n = (size_t)handle->ncoarse;
  g->h_stage_n = std::max<size_t>({handle->sendbuf.n + handle->recvbuf.n, n * n, 2 + 3 * n, (size_t)64});
  HIP_TRY(hipSetDevice(handle->opts.device_id));
  HIP_TRY(hipHostMalloc((void**)&g->h_stage, g->h_stage_n * sizeof(double)));
  *out = g.release();
  return GMPNP_OK;
}

// Peer-mailbox transport, step 1: allocate this rank's mailbox and hand out its IPC handle.  The caller gathers the handles of
// all ranks (any channel: the Python driver uses torch.distributed.all_gather) and calls gmpnp_group_peer_connect.
int gmpnp_group_peer_begin(gmpnp_solver* handle, gmpnp_group** out, char ipc_handle[GMPNP_PEER_HANDLE_BYTES]) {
  static_assert(GMPNP_PEER_HANDLE_BYTES == sizeof(hipIpcMemHandle_t), "IPC handle size");
  if (!handle || !out || !ipc_handle) return fail(GMPNP_ERR_INVALID, "NULL argument");
  *out = nullptr;
  if (!handle->partitioned) return fail(GMPNP_ERR_INVALID, "group members must come from gmpnp_create_partition");
  if (handle->part_size > kPeerMax) return fail(GMPNP_ERR_INVALID, "peer transport: at most 8 ranks");
  if (handle->nb_rank.size() > (size_t)kPeerNbMax) return fail(GMPNP_ERR_INVALID, "peer transport: at most 8 neighbours per rank");
  std::unique_ptr<gmpnp_group> g(new gmpnp_group);
  g->dom.push_back(handle);
  g->peer = true;
  HIP_TRY(hipSetDevice(handle->opts.device_id));
  PeerArgs& a = g->pa;
  a.me = handle->part_rank; a.size = handle->part_size; a.seq = 0;
  const size_t n = (size_t)handle->ncoarse;
  a.red_cap = (int)std::max<size_t>({n * n, 2 + 3 * n, (size_t)8});
  a.red_cap = (a.red_cap + 15) & ~15;
  a.wmax = handle->nf * handle->nf;
  // mailbox layout (every offset the same on every rank; only the last area's size differs): flags | table | all-reduce contributions
  // | flagged-word sums [kLLSlots][size][red_cap] | flagged-word ghost rows [kLLHaloNodes][kLLSlots][kLLRow] (16 bytes a double) |
  // ghost rows of the flag-based exchanges (2 parities, wmax doubles per node)
  g->ll_red_off = kPeerRedOff + (size_t)2 * a.size * a.red_cap * sizeof(double);
  g->ll_halo_off = g->ll_red_off + (size_t)kLLSlots * a.size * a.red_cap * 16;
  a.halo_off = g->ll_halo_off + (size_t)kLLHaloNodes * kLLSlots * kLLRow * 16;
  a.n_nb = (int)handle->nb_rank.size();
  for (int j = 0; j < a.n_nb; ++j) a.nb_rank[j] = handle->nb_rank[j];
  for (int j = 0; j <= a.n_nb; ++j) { a.send_ptr[j] = handle->send_ptr[j]; a.recv_ptr[j] = handle->recv_ptr[j]; }
  g->box_bytes = a.halo_off + (size_t)2 * std::max(1, n_recv(handle)) * a.wmax * sizeof(double);
  // uncached: a peer's stores (and this rank's polls of them) must not meet a stale line in this GPU's L2
  HIP_TRY(hipExtMallocWithFlags((void**)&g->box, g->box_bytes, hipDeviceMallocUncached));
  HIP_TRY(hipMemset(g->box, 0, g->box_bytes));
  // where each neighbour's rows start in THIS rank's ghost-row area: the neighbour reads its entry after mapping the mailbox
  std::vector<int32_t> table(kPeerMax, -1);
  for (int j = 0; j < a.n_nb; ++j) table[a.nb_rank[j]] = a.recv_ptr[j];
  HIP_TRY(hipMemcpy(g->box + kPeerTableOff, table.data(), kPeerMax * sizeof(int32_t), hipMemcpyHostToDevice));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMalloc((void**)&g->peer_counter, sizeof(unsigned)));
  HIP_TRY(hipMemset(g->peer_counter, 0, sizeof(unsigned)));
  if (handle->fused_half && handle->nf == 9) {
    // the exchange may ride in front of the next launch's coarse workgroups where that launch is STILL resident at once
    int occ_a = 0, occ_b = 0, cus = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ_a, k_half_a_x<9>, kKrylovThreads, 0));
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ_b, k_half_b_x<9>, kKrylovThreads, 0));
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, handle->opts.device_id));
    const int nsn = n_send(handle);
    const Half ha = half_of(handle, 0, 0), hb = half_of(handle, 1, 0);
    const int nx = std::max(xch_workgroups(ha.nout, nsn, ha.nvec, 9), xch_workgroups(hb.nout, nsn, hb.nvec, 9));
    g->prologue_ok = handle->t.own_ntiles + handle->t.nagg + nx <= std::min(occ_a, occ_b) * cus && n_recv(handle) <= kLLHaloNodes;
  }
  HIP_TRY(hipHostMalloc((void**)&g->h_peer_err, sizeof(int32_t)));
  *g->h_peer_err = 0;
  a.err = g->h_peer_err;
  int clock_khz = 0;   // wall_clock64 rate of THIS device (100 MHz on gfx950, not assumed)
  if (hipDeviceGetAttribute(&clock_khz, hipDeviceAttributeWallClockRate, handle->opts.device_id) != hipSuccess || clock_khz <= 0) clock_khz = 100000;
  a.budget = 5ull * 1000ull * (unsigned long long)clock_khz;
  hipIpcMemHandle_t h;
  HIP_TRY(hipIpcGetMemHandle(&h, g->box));
  std::memcpy(ipc_handle, &h, sizeof h);
  *out = g.release();
  return GMPNP_OK;
}

// Step 2: map the other ranks' mailboxes (all_handles: [size][GMPNP_PEER_HANDLE_BYTES], rank order).  Every rank must have
// returned from gmpnp_group_peer_begin before any rank calls this (the gather of the handles is that point).
int gmpnp_group_peer_connect(gmpnp_group* g, const char* all_handles) {
  if (!g || !all_handles || !g->peer) return fail(GMPNP_ERR_INVALID, "bad arguments");
  if (g->peer_connected) return GMPNP_OK;
  gmpnp_solver* s = g->dom[0];
  HIP_TRY(hipSetDevice(s->opts.device_id));
  PeerArgs& a = g->pa;
  for (int q = 0; q < a.size; ++q) {
    if (q == a.me) { a.box[q] = g->box; continue; }
    hipIpcMemHandle_t h;
    std::memcpy(&h, all_handles + (size_t)q * GMPNP_PEER_HANDLE_BYTES, sizeof h);
    HIP_TRY(hipIpcOpenMemHandle(&g->peer_map[q], h, hipIpcMemLazyEnablePeerAccess));
    a.box[q] = (unsigned char*)g->peer_map[q];
  }
  for (int j = 0; j < a.n_nb; ++j) {
    int32_t off = -1;
    HIP_TRY(hipMemcpy(&off, a.box[a.nb_rank[j]] + kPeerTableOff + (size_t)a.me * sizeof(int32_t), sizeof off, hipMemcpyDeviceToHost));
    if (off < 0) return fail(GMPNP_ERR_INVALID, "peer transport: a neighbour's plan has no segment for this rank");
    a.peer_recv_ptr[j] = off;
  }
  g->peer_connected = true;
  return GMPNP_OK;
}

void gmpnp_group_destroy(gmpnp_group* g) {
  if (!g) return;
  if (g->peer) {   // (the caller has made sure that no rank is still inside an exchange: a barrier of its own)
    if (!g->dom.empty()) { (void)hipSetDevice(g->dom[0]->opts.device_id); (void)hipStreamSynchronize(g->dom[0]->stream); }
    for (int q = 0; q < kPeerMax; ++q) if (g->peer_map[q]) (void)hipIpcCloseMemHandle(g->peer_map[q]);
    if (g->box) (void)hipFree(g->box);
    if (g->peer_counter) (void)hipFree(g->peer_counter);
    if (g->h_peer_err) (void)hipHostFree(g->h_peer_err);
  }
  if (g->h_stage) (void)hipHostFree(g->h_stage);
  if (!g->dom.empty()) { (void)hipSetDevice(g->dom[0]->opts.device_id); (void)hipStreamSynchronize(g->dom[0]->stream); }
  for (size_t d = 1; d < g->own_stream.size(); ++d) if (g->own_stream[d]) g->dom[d]->stream = g->own_stream[d];
  delete g;
}

int gmpnp_group_newton_solve(gmpnp_group* g, const gmpnp_newton_options_t* o, gmpnp_newton_stats_t* stats) {
  if (!g || !o) return fail(GMPNP_ERR_INVALID, "NULL argument");
  if (o->maximum_iterations < 0 || o->krylov_maximum_iterations < 1) return fail(GMPNP_ERR_INVALID, "bad iteration limits");
  if (o->linear_solver != GMPNP_LINEAR_BICGSTAB_TWOLEVEL && o->linear_solver != GMPNP_LINEAR_BICGSTAB_JACOBI)
    return fail(GMPNP_ERR_INVALID, "the partitioned solve uses BiCGStab (two-level or Jacobi)");
  if (o->step_fraction != 0.0)   // the group transports all-reduce sums, the limiter needs a minimum over the ranks
    return fail(GMPNP_ERR_INVALID, "step_fraction: the step limiter is not available in the partitioned solve (set it to 0)");
  gmpnp_newton_stats_t local{};
  gmpnp_newton_stats_t& st = stats ? *stats : local;
  st = fresh_newton_stats();
  HIP_TRY(hipSetDevice(g->dom[0]->opts.device_id));
  if (g->ml_level) return fail(GMPNP_ERR_INVALID, "this group is a coarse level of a multilevel term: the finest level's group drives it");
  if (g->dom[0]->ml_coarse && !g->ml_next)
    return fail(GMPNP_ERR_INVALID, "multilevel term: the coarse level's group is not attached (gmpnp_group_attach_coarse_group)");
  if (g->ml_next && o->linear_solver != GMPNP_LINEAR_BICGSTAB_TWOLEVEL)
    return fail(GMPNP_ERR_INVALID, "multilevel term: the partitioned solve runs it with the two-level preconditioner");
  LevelStreams keep(g);
  return group_newton<3, 9>(g, *o, st);
}

// Multilevel term of partitioned handles: `coarse` holds the coarse levels (gmpnp_attach_coarse_level) of `fine`'s handles, handle
// by handle, over the same kind of transport; it carries that level's collectives from now on.
int gmpnp_group_attach_coarse_group(gmpnp_group* fine, gmpnp_group* coarse) {
  if (!fine || !coarse || fine == coarse) return fail(GMPNP_ERR_INVALID, "bad arguments");
  if (fine->peer || coarse->peer)
    return fail(GMPNP_ERR_INVALID, "multilevel term: not over the peer-mailbox transport (its mailbox and sequence numbers serve one halo plan; "
                                   "use the in-process, host-staged or RCCL transport)");
  auto kind = [](const gmpnp_group* g) { return g->hosted ? "host-staged" : (g->comm ? "RCCL" : "in-process"); };
  if (fine->hosted != coarse->hosted || (fine->comm != nullptr) != (coarse->comm != nullptr))
    return fail(GMPNP_ERR_INVALID, std::string("multilevel term: the coarse group's transport (") + kind(coarse) + ") differs from the fine group's (" + kind(fine) + ")");
  if (fine->comm && fine->comm != coarse->comm) return fail(GMPNP_ERR_INVALID, "multilevel term: the coarse group must use the fine group's communicator");
  if (fine->dom.size() != coarse->dom.size() || fine->dom[0]->part_size != coarse->dom[0]->part_size)
    return fail(GMPNP_ERR_INVALID, "multilevel term: the coarse group holds another number of ranks than the fine group");
  for (size_t d = 0; d < fine->dom.size(); ++d)
    if (fine->dom[d]->ml_coarse != coarse->dom[d])
      return fail(GMPNP_ERR_INVALID, "multilevel term: a handle of the coarse group is not the level attached to the fine group's handle of its rank (gmpnp_attach_coarse_level)");
  if (fine->ml_next || coarse->ml_level) return fail(GMPNP_ERR_INVALID, "multilevel term: a group serves one finer level and has one coarser level");
  fine->ml_next = coarse; coarse->ml_level = true;
  return GMPNP_OK;
}

// One pass of each collective of the partitioned solve over the group's OWN transport (peer mailboxes, RCCL, host-staged or the
// in-process copies), with contents every rank can check by itself: a 5-double all-reduce of (rank + 1)(i + 1), and a ghost-row
// message per neighbour whose k-th value is sender * 1e6 + k.  Collective: every rank of the group calls it; *max_error = largest
// deviation seen by THIS process.  What the bench runs before it trusts a transport between physical GPUs with a timed solve.
int gmpnp_group_selftest(gmpnp_group* g, double* max_error) {
  if (!g || !max_error) return fail(GMPNP_ERR_INVALID, "NULL argument");
  HIP_TRY(hipSetDevice(g->dom[0]->opts.device_id));
  const int size = g->dom[0]->part_size;
  for (gmpnp_solver* s : g->dom) {
    double red[5];
    for (int i = 0; i < 5; ++i) red[i] = (double)(s->part_rank + 1) * (i + 1);
    HIP_TRY(hipMemcpyAsync(s->red_norm.p, red, sizeof red, hipMemcpyHostToDevice, s->stream));
    const int nsn = n_send(s);
    std::vector<double> h((size_t)std::max(nsn, 1));
    for (size_t j = 0; j < s->nb_rank.size(); ++j)
      for (int k = s->send_ptr[j]; k < s->send_ptr[j + 1]; ++k) h[k] = 1e6 * s->part_rank + (k - s->send_ptr[j]);
    if (nsn) HIP_TRY(hipMemcpyAsync(s->sendbuf.p, h.data(), (size_t)nsn * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));   // (h leaves scope)
  }
  int rc = group_reduce_transfer(g, [](gmpnp_solver* s) { return s->red_norm.p; }, 5, 1); if (rc) return rc;
  double err = 0.0;
  for (gmpnp_solver* s : g->dom) {
    // in-process groups run every handle on dom[0]'s stream
    double red[5];
    HIP_TRY(hipMemcpyAsync(red, s->red_norm.p, sizeof red, hipMemcpyDeviceToHost, g->dom[0]->stream));
    const int nrn = n_recv(s);
    std::vector<double> h((size_t)std::max(nrn, 1), 0.0);
    if (nrn) HIP_TRY(hipMemcpyAsync(h.data(), s->recvbuf.p, (size_t)nrn * sizeof(double), hipMemcpyDeviceToHost, g->dom[0]->stream));
    HIP_TRY(hipStreamSynchronize(g->dom[0]->stream));
    for (int i = 0; i < 5; ++i) err = std::max(err, std::fabs(red[i] - 0.5 * size * (size + 1) * (i + 1)));
    for (size_t j = 0; j < s->nb_rank.size(); ++j)
      for (int k = s->recv_ptr[j]; k < s->recv_ptr[j + 1]; ++k) err = std::max(err, std::fabs(h[k] - (1e6 * s->nb_rank[j] + (k - s->recv_ptr[j]))));
  }
  rc = peer_check(g); if (rc) return rc;
  if (flagged_words(g)) {
    // ... and the flagged-word areas the exchange-prologue launches of a solve use (k_xch_selftest), over the same mapping
    gmpnp_solver* s = g->dom[0];
    XchArgs x = make_xch_args(g, Half{}, 0, 0);
    Ctx cc = xch_ctx(g, x);
    HIP_TRY(hipMemsetAsync(s->status.p, 0, sizeof(int32_t), s->stream));
    hipLaunchKernelGGL(k_xch_selftest, dim3(1), dim3(kKrylovThreads), 0, s->stream, cc, x, g->pa, s->red_norm.p);
    HIP_TRY(hipGetLastError());
    double xerr = 0.0; int32_t st = 0;
    HIP_TRY(hipMemcpyAsync(&xerr, s->red_norm.p, sizeof xerr, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipMemcpyAsync(&st, s->status.p, sizeof st, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipMemsetAsync(s->status.p, 0, sizeof(int32_t), s->stream));
    if (st & 8) return fail(GMPNP_ERR_HIP, "peer transport: a flagged word of another rank did not arrive within 12 s");
    err = std::max(err, xerr);
  }
  *max_error = err;
  return GMPNP_OK;
}

int gmpnp_group_set_exchange_form(gmpnp_group* g, int32_t form) {
  if (!g || (form != 0 && form != 1)) return fail(GMPNP_ERR_INVALID, "bad arguments");
  g->exchange_form = form;
  return GMPNP_OK;
}
int32_t gmpnp_group_exchange_form(const gmpnp_group* g) {
  if (!g) return -1;
  return flagged_words(g) ? 2 : (g->peer ? 1 : 0);
}

int gmpnp_group_assign_previous(gmpnp_group* g) {
  if (!g) return fail(GMPNP_ERR_INVALID, "NULL argument");
  HIP_TRY(hipSetDevice(g->dom[0]->opts.device_id));
  for (gmpnp_solver* s : g->dom) HIP_TRY(hipMemcpyAsync(s->un.p, s->u.p, s->ndof * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
  return GMPNP_OK;
}

}  // extern "C"
