// Ensemble of independent 1D problems on one mesh (include/gmpnp.h, "ensemble of 1D problems").
// Included at the end of gmpnp_api.hip: uses the handle type and the helpers defined there.
//
// One Newton iteration of B members is ONE launch chain: Jacobian gather, block-tridiagonal extraction, the cyclic reduction
// down (one launch per level), the tail (one wave per member), the reduction up, the update, and the residual (element kernel +
// gather) at the new iterate.  Every launch carries all ACTIVE members: blockIdx.y (the tail: blockIdx.x) indexes the active list,
// the member's Ctx / TriLevel pyramid / status word come from a per-member table in device memory.  The batched kernels call the
// single handle's code (the bodies of k_element and k_jac_gather, res_gather_body, tri_extract_entry, bcr_forward_row,
// bcr_top_row, bcr_backward_entry, tri_apply_entry), so a member computes exactly what its handle computes alone.  Members are
// independent: nothing waits inside a launch, the launch boundaries are the only ordering.  One host synchronisation per
// iteration: the residual partials of every member land in that member's pinned buffer, the host forms the norms and decides
// per member with the one Newton rule (NewtonJudge, gmpnp_host_rules.h), then uploads the next active list.
#pragma once

namespace gmpnp {

constexpr int kEnsMaxMembers = 64;   // gmpnp_ensemble_create refuses more
constexpr int kEnsMaxLevels = 32;    // cyclic-reduction levels: ceil(log2(n_vertices)) + 1

struct EnsMember {
  Ctx c;
  TriLevel tri[kEnsMaxLevels];
  int32_t* status;
  const int32_t* tri_kpos;
};

template <int DIM, int NF>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(GMPNP_ELEMENT_WAVES, GMPNP_ELEMENT_WAVES))) void k_element_ens(
    const EnsMember* __restrict__ tab, const int32_t* __restrict__ act) {
  constexpr bool WANT_J = true, STAGED = false;
  const Ctx& c = tab[act[blockIdx.y]].c;   // (a copy of the context here costs 864 bytes of scratch per lane; the gather's copy costs none)
#include "gmpnp_element_body.inc"
}
template <int DIM, int NF>
__global__ __launch_bounds__(kVecBlock) void k_res_gather_ens(const EnsMember* __restrict__ tab, const int32_t* __restrict__ act) {
  res_gather_body<DIM, NF>(tab[act[blockIdx.y]].c);
}
template <int DIM, int NF>
__global__ __launch_bounds__(kVecBlock) void k_jac_gather_ens(const EnsMember* __restrict__ tab, const int32_t* __restrict__ act) {
  const Ctx c = tab[act[blockIdx.y]].c;
#include "gmpnp_jac_gather_body.inc"
}
template <int NF>
__global__ __launch_bounds__(kVecBlock) void k_tri_extract_ens(const EnsMember* __restrict__ tab, const int32_t* __restrict__ act) {
  const EnsMember& M = tab[act[blockIdx.y]];
  const TriLevel l0 = M.tri[0];
  tri_extract_entry<NF>(M.c, l0, M.tri_kpos, M.c.F, blockIdx.x * kVecBlock + threadIdx.x);
}
template <int NF>
__global__ __launch_bounds__(64) void k_bcr_forward_ens(const EnsMember* __restrict__ tab, const int32_t* __restrict__ act, const int l) {
  const EnsMember& M = tab[act[blockIdx.y]];
  const TriLevel lo = M.tri[l], hi = M.tri[l + 1];
  bcr_forward_row<NF>(lo, hi, M.status, blockIdx.x * 4 + ((int)threadIdx.x >> 4));
}
// k_bcr_tail of one member per workgroup (one wave each): levels l0 .. l0 + nlev - 1
template <int NF>
__global__ __launch_bounds__(kBcrTailThreads) void k_bcr_tail_ens(const EnsMember* __restrict__ tab, const int32_t* __restrict__ act,
                                                                  const int l0, const int nlev) {
  const EnsMember& M = tab[act[blockIdx.x]];
  const TriLevel* lv = M.tri + l0;
  int32_t* status = M.status;
  const int t = threadIdx.x;
  for (int l = 0; l + 1 < nlev; ++l) {
    const TriLevel lo = lv[l], hi = lv[l + 1];
    for (int ih0 = 0; ih0 < hi.n; ih0 += kBcrTailThreads / 16) bcr_forward_row<NF>(lo, hi, status, ih0 + (t >> 4));
    __syncthreads();
  }
  {
    const TriLevel top = lv[nlev - 1];
    if (t < 64) bcr_top_row<NF>(top, status);
  }
  __syncthreads();
  for (int l = nlev - 2; l >= 0; --l) {
    const TriLevel lo = lv[l], hi = lv[l + 1];
    for (int q = t; q < lo.n * NF; q += kBcrTailThreads) bcr_backward_entry<NF>(lo, hi, q);
    __syncthreads();
  }
}
template <int NF>
__global__ __launch_bounds__(kVecBlock) void k_bcr_backward_ens(const EnsMember* __restrict__ tab, const int32_t* __restrict__ act, const int l) {
  const EnsMember& M = tab[act[blockIdx.y]];
  const TriLevel lo = M.tri[l], hi = M.tri[l + 1];
  bcr_backward_entry<NF>(lo, hi, blockIdx.x * kVecBlock + threadIdx.x);
}
// u <- u - omega x (tri_apply of the single handle with scale_dst = 1, scale_x = -omega)
template <int NF>
__global__ __launch_bounds__(kVecBlock) void k_tri_apply_ens(const EnsMember* __restrict__ tab, const int32_t* __restrict__ act, const double scale_x) {
  const EnsMember& M = tab[act[blockIdx.y]];
  const TriLevel l0 = M.tri[0];
  tri_apply_entry<NF>(l0, M.c.u, 1.0, scale_x, M.c.ndof, blockIdx.x * kVecBlock + threadIdx.x);
}
// u_n <- u of member blockIdx.y (all members)
__global__ __launch_bounds__(256) void k_ens_assign(const EnsMember* __restrict__ tab, const int ndof) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= ndof) return;
  const Ctx& c = tab[blockIdx.y].c;
  c.un[i] = c.u[i];
}
// dst[m][i] = u of member m (internal order)
__global__ __launch_bounds__(256) void k_ens_gather_u(const EnsMember* __restrict__ tab, double* __restrict__ dst, const int ndof) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= ndof) return;
  dst[(size_t)blockIdx.y * ndof + i] = tab[blockIdx.y].c.u[i];
}

}  // namespace gmpnp

struct gmpnp_ensemble {
  std::vector<gmpnp_solver*> m;   // owned by the caller
  int device = 0, ndof = 0, nv = 0;
  hipStream_t stream = nullptr;
  DevBuf<EnsMember> tab; DevBuf<int32_t> act; DevBuf<double> ustage;
  EnsMember* h_tab = nullptr;   // pinned [n]: staging of the member table
  int32_t* h_act = nullptr;     // pinned [2][kEnsMaxMembers]: active lists, alternating
  double* h_u = nullptr;        // pinned [n][ndof]
  int act_slot = 0;
  std::vector<std::string> err;   // last failure of each member ("" = none)
  ~gmpnp_ensemble() {
    if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
    if (h_tab) (void)hipHostFree(h_tab);
    if (h_act) (void)hipHostFree(h_act);
    if (h_u) (void)hipHostFree(h_u);
  }
};

namespace {

// every member's own stream drained: what a member call queued (gmpnp_assign_previous) is done before the ensemble reads its state
int ens_drain_members(gmpnp_ensemble* e) {
  for (gmpnp_solver* s : e->m) HIP_TRY(hipStreamSynchronize(s->stream));
  return GMPNP_OK;
}

// the configuration an ensemble solve supports, per member: checked at create and again before every solve (SUPG can be set later)
int ens_check_member(const gmpnp_solver* s, const gmpnp_solver* s0, int k) {
  char buf[200];
  auto bad = [&](const char* why) { snprintf(buf, sizeof buf, "ensemble member %d: %s", k, why); return fail(GMPNP_ERR_INVALID, buf); };
  if (!s) return bad("NULL handle");
  if (s->dim != 1 || s->nf != 7) return bad("ensembles hold 1D problems (6 species + potential); 3D ensembles are not supported");
  if (s->partitioned) return bad("partitioned handles cannot join an ensemble");
  if (!s->tri_ok) return bad("the block-tridiagonal solver needs a 1D mesh in path order");
  if (s->c.supg_rho) return bad("SUPG terms are set (gmpnp_set_supg): not supported in an ensemble");
  if ((int)s->tri.size() > kEnsMaxLevels) return bad("mesh too large for the ensemble's level table");
  if (s->c.n_robin != 0) return bad("Robin terms are not part of the 1D model");
  if (s == s0) return GMPNP_OK;
  if (s->opts.device_id != s0->opts.device_id) return bad("members live on different devices");
  const Topology& a = s->t; const Topology& b = s0->t;
  if (a.nv != b.nv || a.nc != b.nc || a.perm != b.perm || a.cells != b.cells || s->ndof != s0->ndof || a.nslices != b.nslices ||
      s->c.n_work != s0->c.n_work || s->c.wl_run_blocks != s0->c.wl_run_blocks || s->n_resblocks != s0->n_resblocks ||
      s->tri.size() != s0->tri.size())
    return bad("topology differs from member 0 (mesh, vertex order, cells or storage layout)");
  return GMPNP_OK;
}

int ens_upload_table(gmpnp_ensemble* e) {
  const int n = (int)e->m.size();
  for (int k = 0; k < n; ++k) {
    gmpnp_solver* s = e->m[k];
    EnsMember rec{};
    rec.c = s->c;
    for (size_t l = 0; l < s->tri.size(); ++l) rec.tri[l] = s->tri[l];
    rec.status = s->status.p; rec.tri_kpos = s->tri_kpos.p;
    std::memcpy(&e->h_tab[k], &rec, sizeof rec);
  }
  HIP_TRY(hipMemcpyAsync(e->tab.p, e->h_tab, (size_t)n * sizeof(EnsMember), hipMemcpyHostToDevice, e->stream));
  return GMPNP_OK;
}

// the active list of the next launches: stream-ordered copy from a pinned slot the host does not touch again before the copy ran
// (the slots alternate, and every iteration ends with a synchronisation of the stream)
int ens_upload_active(gmpnp_ensemble* e, const std::vector<int32_t>& act) {
  int32_t* src = e->h_act + (size_t)e->act_slot * kEnsMaxMembers;
  e->act_slot ^= 1;
  std::memcpy(src, act.data(), act.size() * sizeof(int32_t));
  HIP_TRY(hipMemcpyAsync(e->act.p, src, act.size() * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
  return GMPNP_OK;
}

// element kernel + residual gather of the active members at their current u (leaves F and the element Jacobian records)
int ens_residual(gmpnp_ensemble* e, int nact) {
  gmpnp_solver* s0 = e->m[0];
  hipLaunchKernelGGL((k_element_ens<1, 7>), dim3(grid_for(s0->t.nc, 64), nact), dim3(64), 0, e->stream, (const EnsMember*)e->tab.p,
                     (const int32_t*)e->act.p);
  hipLaunchKernelGGL((k_res_gather_ens<1, 7>), dim3(s0->n_resblocks, nact), dim3(kVecBlock), 0, e->stream, (const EnsMember*)e->tab.p,
                     (const int32_t*)e->act.p);
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

// J dx = F by block cyclic reduction and u <- u - omega dx for the active members (gather, tri_solve and tri_apply of newton())
int ens_update(gmpnp_ensemble* e, int nact, double omega) {
  gmpnp_solver* s0 = e->m[0];
  const EnsMember* tab = e->tab.p; const int32_t* act = e->act.p;
  constexpr int NF = 7;
  hipLaunchKernelGGL((k_jac_gather_ens<1, NF>), dim3(grid_for(s0->c.n_work * kWave, kVecBlock), nact), dim3(kVecBlock), 0, e->stream, tab, act);
  hipLaunchKernelGGL((k_tri_extract_ens<NF>), dim3(grid_for(s0->t.nv * NF * NF, kVecBlock), nact), dim3(kVecBlock), 0, e->stream, tab, act);
  const int nl = (int)s0->tri.size(), l0 = bcr_tail_first_level(s0);
  for (int l = 0; l < l0; ++l)
    hipLaunchKernelGGL((k_bcr_forward_ens<NF>), dim3(grid_for(s0->tri[l + 1].n, 4), nact), dim3(64), 0, e->stream, tab, act, l);
  hipLaunchKernelGGL((k_bcr_tail_ens<NF>), dim3(nact), dim3(kBcrTailThreads), 0, e->stream, tab, act, l0, nl - l0);
  for (int l = l0 - 1; l >= 0; --l)
    hipLaunchKernelGGL((k_bcr_backward_ens<NF>), dim3(grid_for(s0->tri[l].n * NF, kVecBlock), nact), dim3(kVecBlock), 0, e->stream, tab, act, l);
  hipLaunchKernelGGL((k_tri_apply_ens<NF>), dim3(grid_for(s0->ndof, kVecBlock), nact), dim3(kVecBlock), 0, e->stream, tab, act, -omega);
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

}  // namespace

extern "C" {

int gmpnp_ensemble_create(int32_t n, gmpnp_solver* const* members, gmpnp_ensemble** out) {
  if (!members || !out) return fail(GMPNP_ERR_INVALID, "NULL argument");
  *out = nullptr;
  if (n < 1 || n > kEnsMaxMembers) return fail(GMPNP_ERR_INVALID, "ensemble size must be 1 ... 64");
  for (int k = 0; k < n; ++k) { int rc = ens_check_member(members[k], members[0], k); if (rc) return rc; }
  for (int k = 0; k < n; ++k)
    for (int j = 0; j < k; ++j)
      if (members[j] == members[k]) return fail(GMPNP_ERR_INVALID, "a handle appears twice in the ensemble");
  std::unique_ptr<gmpnp_ensemble> e(new gmpnp_ensemble);
  e->m.assign(members, members + n);
  e->device = members[0]->opts.device_id; e->ndof = members[0]->ndof; e->nv = members[0]->t.nv;
  e->err.assign(n, std::string());
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamCreate(&e->stream));
  HIP_TRY(e->tab.alloc(n)); HIP_TRY(e->act.alloc(kEnsMaxMembers)); HIP_TRY(e->ustage.alloc((size_t)n * e->ndof));
  HIP_TRY(hipHostMalloc((void**)&e->h_tab, (size_t)n * sizeof(EnsMember)));
  HIP_TRY(hipHostMalloc((void**)&e->h_act, 2 * kEnsMaxMembers * sizeof(int32_t)));
  HIP_TRY(hipHostMalloc((void**)&e->h_u, (size_t)n * e->ndof * sizeof(double)));
  int rc = ens_upload_table(e.get()); if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));
  *out = e.release();
  return GMPNP_OK;
}

void gmpnp_ensemble_destroy(gmpnp_ensemble* e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  delete e;
}

int32_t gmpnp_ensemble_size(const gmpnp_ensemble* e) { return e ? (int32_t)e->m.size() : 0; }

const char* gmpnp_ensemble_member_error(const gmpnp_ensemble* e, int32_t k) {
  if (!e || k < 0 || k >= (int32_t)e->m.size()) return "";
  return e->err[k].c_str();
}

int gmpnp_ensemble_newton_solve(gmpnp_ensemble* e, const gmpnp_newton_options_t* o, gmpnp_newton_stats_t* stats, int32_t* status) {
  if (!e || !o || !stats || !status) return fail(GMPNP_ERR_INVALID, "NULL argument");
  if (o->maximum_iterations < 0 || o->krylov_maximum_iterations < 1) return fail(GMPNP_ERR_INVALID, "bad iteration limits");
  if (o->linear_solver != GMPNP_LINEAR_BLOCK_TRIDIAGONAL)
    return fail(GMPNP_ERR_INVALID, "ensembles solve with GMPNP_LINEAR_BLOCK_TRIDIAGONAL only");
  const int n = (int)e->m.size();
  for (int k = 0; k < n; ++k) { int rc = ens_check_member(e->m[k], e->m[0], k); if (rc) return rc; }
  HIP_TRY(hipSetDevice(e->device));
  const double t0 = now_ms();
  { int rc = ens_drain_members(e); if (rc) return rc; }
  // the member table is rebuilt for every solve: a gmpnp_set_* call may have re-allocated member storage since the last one
  { int rc = ens_upload_table(e); if (rc) return rc; }
  std::vector<char> live(n, 1);
  std::vector<NewtonJudge> judge; judge.reserve(n);   // one per member: the single handle's rule (gmpnp_host_rules.h)
  for (int k = 0; k < n; ++k) {
    stats[k] = gmpnp_newton_stats_t{}; status[k] = GMPNP_OK; e->err[k].clear();
    judge.emplace_back(*o, stats[k], e->m[k]->cfg.strict_steric != 0);
    HIP_TRY(hipMemsetAsync(e->m[k]->status.p, 0, sizeof(int32_t), e->stream));
  }
  // member k's residual is in its pinned buffer: the verdict, mapped to status[k] / err[k] / live[k] (a member that fails keeps
  // its message and the others go on; a member that ends its solve ends as newton() does)
  auto settle = [&](int k, bool first) {
    gmpnp_solver* s = e->m[k];
    const double r = std::sqrt(sum_partials(s, 0));
    const NewtonJudge::Verdict v = first ? judge[k].first(r, *s->h_status) : judge[k].next(r, *s->h_status);
    if (v == NewtonJudge::go_on) return;
    live[k] = 0;
    if (v != NewtonJudge::failed) { s->state_jumped = false; stats[k].ms_total = now_ms() - t0; }
    if (v != NewtonJudge::converged) { status[k] = judge[k].code; e->err[k] = judge[k].message; }
  };
  std::vector<int32_t> act(n);
  for (int k = 0; k < n; ++k) act[k] = k;
  { int rc = ens_upload_active(e, act); if (rc) return rc; }
  { int rc = ens_residual(e, n); if (rc) return rc; }
  HIP_TRY(hipStreamSynchronize(e->stream));
  for (int k = 0; k < n; ++k) settle(k, true);
  for (;;) {
    act.clear();
    for (int k = 0; k < n; ++k) if (live[k]) act.push_back(k);
    if (act.empty()) break;
    const int nact = (int)act.size();
    int rc = ens_upload_active(e, act); if (rc) return rc;
    rc = ens_update(e, nact, o->relaxation_parameter); if (rc) return rc;
    rc = ens_residual(e, nact); if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));   // the one host synchronisation of the iteration
    for (int k : act) {
      e->m[k]->jacobian_valid = true;
      stats[k].iterations++;
      settle(k, false);
    }
  }
  for (int k = 0; k < n; ++k)
    if (status[k] != GMPNP_OK) { g_err = "ensemble member " + std::to_string(k) + ": " + e->err[k]; return status[k]; }
  return GMPNP_OK;
}

int gmpnp_ensemble_assign_previous(gmpnp_ensemble* e) {
  if (!e) return fail(GMPNP_ERR_INVALID, "NULL handle");
  HIP_TRY(hipSetDevice(e->device));
  int rc = ens_drain_members(e); if (rc) return rc;
  // u / u_n of a handle are allocated once at create: the table of the last upload addresses them
  hipLaunchKernelGGL(k_ens_assign, dim3(grid_for(e->ndof, 256), (unsigned)e->m.size()), dim3(256), 0, e->stream, (const EnsMember*)e->tab.p, e->ndof);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->stream));   // blocking: a member call on the member's own stream sees u_n afterwards
  return GMPNP_OK;
}

int gmpnp_ensemble_get_state(gmpnp_ensemble* e, double* u_out) {
  if (!e || !u_out) return fail(GMPNP_ERR_INVALID, "NULL argument");
  HIP_TRY(hipSetDevice(e->device));
  int rc = ens_drain_members(e); if (rc) return rc;
  const int n = (int)e->m.size(), nf = 7, nv = e->nv, ndof = e->ndof;
  hipLaunchKernelGGL(k_ens_gather_u, dim3(grid_for(ndof, 256), n), dim3(256), 0, e->stream, (const EnsMember*)e->tab.p, e->ustage.p, ndof);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(e->h_u, e->ustage.p, (size_t)n * ndof * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  for (int k = 0; k < n; ++k) {
    const int32_t* perm = e->m[k]->t.perm.data();
    const double* src = e->h_u + (size_t)k * ndof;
    double* dst = u_out + (size_t)k * ndof;
    for (int i = 0; i < nv; ++i) std::memcpy(&dst[(size_t)perm[i] * nf], &src[(size_t)i * nf], nf * sizeof(double));
  }
  return GMPNP_OK;
}

}  // extern "C"
