// Adaptive time stepping of an ensemble's members, every member on its own clock (include/gmpnp.h: gmpnp_ensemble_set_time_step,
// gmpnp_ensemble_time_error, gmpnp_ensemble_time_advance).  The kernels of gmpnp_time_step.h with a list of
// members per launch: blockIdx.y (the reduce: blockIdx.x) indexes the list, the member's arguments come from a per-call table
// (EnsTimeRec, indexed by member).
//
//   k_time_error_ens    (workgroups of 256 nodes, listed members): the body of k_time_error, as text (gmpnp_time_error_body.inc),
//                       on the member's u, u_n, u_nm1, Dirichlet flags, partials and its own ratio, scale, inv_h, rtol, atol[]
//   k_time_reduce_ens   one workgroup per listed member: the body of k_time_reduce (fixed-order sums, its tie rule); the report goes
//                       to the member's row of ONE pinned array owned by the ensemble
//   k_time_advance_ens  (workgroups of 256 dofs, listed members), per member: accept = the one-pass shift of k_time_shift, reject =
//                       u <- u_n
// u_nm1 and the partials are each member's own (time_prepare): the history is shared with the single-handle calls.  The table is
// staged in pinned memory, two alternating slots; every call here ends with a synchronisation of the ensemble's stream, so a
// queued launch never sees the table or the list change under it.  No atomics on data.  Included behind gmpnp_ensemble.h and
// gmpnp_time_step.h.
#pragma once

namespace gmpnp {

struct EnsTimeRec {
  TimeErrorIo io;                     // the estimator's arguments of the member (k_time_error_ens)
  TimeReport* report;                 // the member's row of the ensemble's pinned reports (k_time_reduce_ens)
  double* u; double* un; double* unm1;   // k_time_advance_ens
  int32_t action;                     // 1 accept, 2 reject
};

template <int NF>
__global__ __launch_bounds__(kVecBlock) void k_time_error_ens(const EnsTimeRec* __restrict__ tab, const int32_t* __restrict__ act) {
  const TimeErrorIo& io = tab[act[blockIdx.y]].io;
#include "gmpnp_time_error_body.inc"
}

template <int NF>
__global__ __launch_bounds__(kVecBlock) void k_time_reduce_ens(const EnsTimeRec* __restrict__ tab, const int32_t* __restrict__ act) {
  const EnsTimeRec& M = tab[act[blockIdx.x]];
  time_reduce_body<NF>(M.io.part, M.io.part_max, M.io.part_dof, M.io.part_bad, M.io.nblk, M.report);
}

__global__ __launch_bounds__(kVecBlock) void k_time_advance_ens(const EnsTimeRec* __restrict__ tab, const int32_t* __restrict__ act,
                                                                const int ndof) {
  const int i = blockIdx.x * kVecBlock + threadIdx.x;
  if (i >= ndof) return;
  const EnsTimeRec& M = tab[act[blockIdx.y]];
  if (M.action == 1) {          // k_time_shift
    const double a = M.u[i], b = M.un[i];
    M.un[i] = a; M.unm1[i] = b;
  } else if (M.action == 2) {   // gmpnp_time_reject's copy
    M.u[i] = M.un[i];
  }
}

}  // namespace gmpnp

namespace {

int ens_time_prepare(gmpnp_ensemble* e) {
  if (e->tstep) return GMPNP_OK;
  std::unique_ptr<gmpnp_ens_time> T(new gmpnp_ens_time);
  HIP_TRY(hipMalloc((void**)&T->d_rec, (size_t)kEnsMaxMembers * sizeof(EnsTimeRec)));
  HIP_TRY(hipMemset(T->d_rec, 0, (size_t)kEnsMaxMembers * sizeof(EnsTimeRec)));
  HIP_TRY(hipHostMalloc((void**)&T->h_rec, (size_t)2 * kEnsMaxMembers * sizeof(EnsTimeRec)));
  std::memset((void*)T->h_rec, 0, (size_t)2 * kEnsMaxMembers * sizeof(EnsTimeRec));
  HIP_TRY(hipHostMalloc((void**)&T->h_report, (size_t)kEnsMaxMembers * sizeof(TimeReport), hipHostMallocCoherent | hipHostMallocMapped));
  std::memset((void*)T->h_report, 0, (size_t)kEnsMaxMembers * sizeof(TimeReport));
  { void* dp = nullptr; HIP_TRY(hipHostGetDevicePointer(&dp, T->h_report, 0)); T->d_report = (TimeReport*)dp; }
  HIP_TRY(hipHostMalloc((void**)&T->h_model, e->m.size() * sizeof(gmpnp_model_t)));
  e->tstep = std::move(T);
  return GMPNP_OK;
}

// what gmpnp_ensemble_newton_solve re-checks, for the calls of this family
int ens_time_check(gmpnp_ensemble* e, const char* what) {
  const int n = (int)e->m.size();
  for (int k = 0; k < n; ++k) { int rc = ens_check_member(e->m[k], e->m[0], k); if (rc) return rc; }
  for (int k = 0; k < n; ++k)
    if (e->m[k]->partitioned) return fail(GMPNP_ERR_INVALID, std::string(what) + ": partition handles have no adaptive time stepping");
  return GMPNP_OK;
}

// the records of the listed members and the list, staged in the slot of this call and copied in the ensemble's stream
int ens_time_upload(gmpnp_ensemble* e, const std::vector<EnsTimeRec>& rec, const std::vector<int32_t>& list) {
  gmpnp_ens_time* T = e->tstep.get();
  EnsTimeRec* src = T->h_rec + (size_t)T->slot * kEnsMaxMembers;
  T->slot ^= 1;
  for (int k : list) std::memcpy((void*)&src[k], &rec[k], sizeof(EnsTimeRec));
  // (one copy of the members' span: a row outside the list is never indexed)
  HIP_TRY(hipMemcpyAsync(T->d_rec, src, e->m.size() * sizeof(EnsTimeRec), hipMemcpyHostToDevice, e->stream));
  e->act_slot ^= 1;
  return ens_upload_list(e, L_TIME, list);
}

}  // namespace

extern "C" {

int gmpnp_ensemble_set_time_step(gmpnp_ensemble* e, const double* inv_dt) {
  if (!e || !inv_dt) return fail(GMPNP_ERR_INVALID, "gmpnp_ensemble_set_time_step: NULL argument");
  const int n = (int)e->m.size();
  for (int k = 0; k < n; ++k)
    if (!time_step_valid(inv_dt[k]))
      return fail(GMPNP_ERR_INVALID, "gmpnp_ensemble_set_time_step: ensemble member " + std::to_string(k) + ": inv_dt must be finite and >= 0 (0 = steady form)");
  { int rc = ens_time_check(e, "gmpnp_ensemble_set_time_step"); if (rc) return rc; }
  HIP_TRY(hipSetDevice(e->device));
  { int rc = ens_time_prepare(e); if (rc) return rc; }
  { int rc = ens_drain_members(e); if (rc) return rc; }   // idle streams unless a member call was queued
  gmpnp_ens_time* T = e->tstep.get();
  for (int k = 0; k < n; ++k) {
    gmpnp_solver* s = e->m[k];   // (ens_check_member: no coarse level below a member)
    s->model.inv_dt = inv_dt[k];
    std::memcpy(&T->h_model[k], &s->model, sizeof(gmpnp_model_t));
    HIP_TRY(hipMemcpyAsync(s->d_model.p, &T->h_model[k], sizeof(gmpnp_model_t), hipMemcpyHostToDevice, e->stream));
    s->jacobian_valid = false; s->precond_valid = false;
  }
  HIP_TRY(hipStreamSynchronize(e->stream));   // the one synchronisation for the whole ensemble
  return GMPNP_OK;
}

int gmpnp_ensemble_time_error(gmpnp_ensemble* e, const double* h, const double* h_prev, const gmpnp_time_tol_t* tol, const int32_t* mask,
                              gmpnp_time_error_t* out) {
  if (!e || !h || !h_prev || !tol || !out) return fail(GMPNP_ERR_INVALID, "gmpnp_ensemble_time_error: NULL argument");
  const int n = (int)e->m.size();
  { int rc = ens_time_check(e, "gmpnp_ensemble_time_error"); if (rc) return rc; }
  std::vector<int32_t> list;
  for (int k = 0; k < n; ++k) {
    if (mask && !mask[k]) continue;
    if (const char* why = time_error_invalid(h[k], h_prev[k], tol[k], e->m[k]->nf))
      return fail(GMPNP_ERR_INVALID, "gmpnp_ensemble_time_error: ensemble member " + std::to_string(k) + ": " + why);
    list.push_back(k);
  }
  HIP_TRY(hipSetDevice(e->device));
  for (int k : list) { int rc = time_prepare(e->m[k], "gmpnp_ensemble_time_error"); if (rc) return rc; }
  { int rc = ens_time_prepare(e); if (rc) return rc; }
  for (int k = 0; k < n; ++k) out[k] = gmpnp_time_error_t{};
  if (list.empty()) return GMPNP_OK;
  { int rc = ens_drain_members(e); if (rc) return rc; }
  gmpnp_ens_time* T = e->tstep.get();
  std::vector<EnsTimeRec> rec(n);
  std::vector<char> history(n, 0);
  for (int k : list) {
    gmpnp_solver* s = e->m[k];
    history[k] = s->stepper->has_history && h_prev[k] > 0.0;
    rec[k] = EnsTimeRec{};
    rec[k].io = time_error_io(s, h[k], h_prev[k], history[k] != 0, tol[k]);
    rec[k].report = T->d_report + k;
  }
  { int rc = ens_time_upload(e, rec, list); if (rc) return rc; }
  gmpnp_solver* s0 = e->m[0];
  const unsigned nl = (unsigned)list.size();
  const int nblk = e->m[list[0]]->stepper->nblk;   // one mesh: one count
  const EnsTimeRec* tab = T->d_rec; const int32_t* act = ens_list(e, L_TIME);
  if (s0->nf == 9) {
    hipLaunchKernelGGL((k_time_error_ens<9>), dim3(nblk, nl), dim3(kVecBlock), 0, e->stream, tab, act);
    hipLaunchKernelGGL((k_time_reduce_ens<9>), dim3(nl), dim3(kVecBlock), 0, e->stream, tab, act);
  } else {
    hipLaunchKernelGGL((k_time_error_ens<7>), dim3(nblk, nl), dim3(kVecBlock), 0, e->stream, tab, act);
    hipLaunchKernelGGL((k_time_reduce_ens<7>), dim3(nl), dim3(kVecBlock), 0, e->stream, tab, act);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->stream));   // the one host synchronisation of the call
  for (int k : list) out[k] = time_report_result(e->m[k], T->h_report[k], history[k] != 0);
  return GMPNP_OK;
}

int gmpnp_ensemble_time_advance(gmpnp_ensemble* e, const int32_t* action) {
  if (!e || !action) return fail(GMPNP_ERR_INVALID, "gmpnp_ensemble_time_advance: NULL argument");
  const int n = (int)e->m.size();
  std::vector<int32_t> list;
  for (int k = 0; k < n; ++k) {
    if (action[k] < 0 || action[k] > 2)
      return fail(GMPNP_ERR_INVALID, "gmpnp_ensemble_time_advance: ensemble member " + std::to_string(k) + ": action must be 0 (leave), 1 (accept) or 2 (reject)");
    if (action[k]) list.push_back(k);
  }
  { int rc = ens_time_check(e, "gmpnp_ensemble_time_advance"); if (rc) return rc; }
  HIP_TRY(hipSetDevice(e->device));
  for (int k : list) { int rc = time_prepare(e->m[k], "gmpnp_ensemble_time_advance"); if (rc) return rc; }
  { int rc = ens_time_prepare(e); if (rc) return rc; }
  if (list.empty()) return GMPNP_OK;
  { int rc = ens_drain_members(e); if (rc) return rc; }
  gmpnp_ens_time* T = e->tstep.get();
  std::vector<EnsTimeRec> rec(n);
  for (int k : list) {
    gmpnp_solver* s = e->m[k];
    rec[k] = EnsTimeRec{};
    rec[k].u = s->u.p; rec[k].un = s->un.p; rec[k].unm1 = s->stepper->unm1.p; rec[k].action = action[k];
  }
  { int rc = ens_time_upload(e, rec, list); if (rc) return rc; }
  hipLaunchKernelGGL(k_time_advance_ens, dim3(grid_for(e->ndof, kVecBlock), (unsigned)list.size()), dim3(kVecBlock), 0, e->stream,
                     (const EnsTimeRec*)T->d_rec, ens_list(e, L_TIME), e->ndof);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->stream));   // complete when it returns, like every ensemble call
  for (int k : list) {
    gmpnp_solver* s = e->m[k];
    if (action[k] == 1) s->stepper->accepted();                            // gmpnp_time_accept
    else { s->state_jumped = true; s->jacobian_valid = false; }            // gmpnp_time_reject
  }
  return GMPNP_OK;
}

}  // extern "C"
