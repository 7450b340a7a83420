// Adaptive time stepping on the device (include/gmpnp.h: gmpnp_set_time_step, gmpnp_time_error, gmpnp_time_accept, gmpnp_time_reject;
// the accept / reject rule is host code: gmpnp_host_rules.h, next_time_step).  Over the FREE dofs (I, f) (bcflag = 0: a Dirichlet
// dof's change between steps is boundary data moving, not truncation error), with h the step just solved and h_prev the accepted
// step before it:
//     p = u_n + (h / h_prev)(u_n - u_nm1)         linear extrapolation through the last two accepted states
//     d = (u - p) h / (2h + h_prev)               backward Euler's local error: u - p = 1/2 u'' h (2h + h_prev) + O(h^3)
//     w = atol_f + rtol max(|u|, |u_n|)
//     err_f = sqrt(sum_I (d/w)^2 / n_free_f)      rate_f = sqrt(sum_I ((u - u_n)/h)^2 / n_free_f)
//
//   k_time_error   one lane per node, shaped like k_step_limit: the workgroup's 256 node blocks of u, u_n and u_nm1 come through LDS
//                  (coalesced loads of the AoS rows in internal order), the lane forms its NF terms, fixed-order workgroup sums ->
//                  ONE partial row per workgroup (per field: sum (d/w)^2, sum of the squared rates, free count; max |d/w| with its
//                  internal dof; a flag for a NaN / Inf in u) in storage of the estimator's own (part_f may be in use by the side stream)
//   k_time_reduce  ONE workgroup sums the partial rows in workgroup order (two calls give equal bits), takes the maximum (ties: the
//                  smaller internal dof) and leaves the report in pinned host memory
//   k_time_shift   the accept as one pass: reads u and u_n, writes u_n and u_nm1
// The reject is a device copy.  No atomics on data.  The batched forms for ensembles: gmpnp_time_step_ens.h.  u_nm1, the partials and the report are allocated by the first call of the
// family: a handle that never asks keeps the buffers and launches it had.  Included at the end of gmpnp_api.hip.
// Second order (variable-step BDF2: its set-up, its estimator and the three-deep shift gmpnp_time_accept launches on an order-2
// handle): gmpnp_time_order.h, included behind this file.
#pragma once

namespace gmpnp {

constexpr int kTimeCols = 3;   // per field: sum (d/w)^2, sum ((u - u_n)/h)^2, free dofs

// what k_time_reduce leaves for the host (pinned memory)
struct TimeReport {
  double sum_err[GMPNP_MAX_SPECIES + 1], sum_rate[GMPNP_MAX_SPECIES + 1], n_free[GMPNP_MAX_SPECIES + 1];
  double worst;      // max |d/w|, -1 = no free dof
  int32_t dof;       // its internal dof, -1 = none
  int32_t bad;       // u held a NaN / Inf
};

struct TimeErrorIo {
  const double* u; const double* un; const double* unm1;   // [nv][NF] internal order
  const uint8_t* bcflag;                                   // [nv][NF]
  double* part;                                            // [kTimeCols * NF][nblk]
  double* part_max; int32_t* part_dof; int32_t* part_bad;  // [nblk]
  int32_t nv, nblk;
  double ratio;     // h / h_prev (0 without history: p = u_n)
  double scale;     // h / (2h + h_prev)
  double inv_h;
  double rtol, atol[GMPNP_MAX_SPECIES + 1];
};

// maximum over the wave with its index, result in every lane; equal values: the smaller index (-1 = no index counts as the largest)
__device__ __forceinline__ void wave_max_index(double& v, int& idx) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o);
    const int oi = __shfl_xor(idx, o);
    if (ov > v || (ov == v && (unsigned)oi < (unsigned)idx)) { v = ov; idx = oi; }
  }
}

template <int NF>
__global__ __launch_bounds__(kVecBlock) void k_time_error(const TimeErrorIo io) {
#include "gmpnp_time_error_body.inc"
}

// one workgroup; thread c < kTimeCols * NF sums column c over the workgroups in their order, thread 64 takes the maximum
// (the body is k_time_reduce_ens's too, gmpnp_time_step_ens.h: additions in one order and comparisons only)
template <int NF>
__device__ __forceinline__ void time_reduce_body(const double* part, const double* part_max, const int32_t* part_dof,
                                                 const int32_t* part_bad, int nblk, TimeReport* out) {
  constexpr int K = kTimeCols * NF;
  const int t = threadIdx.x;
  if (t < K) {
    const double* p = part + (size_t)t * nblk;
    double s = 0.0;
    for (int i = 0; i < nblk; ++i) s += p[i];
    const int f = t % NF;
    if (t < NF) out->sum_err[f] = s;
    else if (t < 2 * NF) out->sum_rate[f] = s;
    else out->n_free[f] = s;
  } else if (t == kWave) {
    double worst = -1.0; int dof = -1, bad = 0;
    for (int i = 0; i < nblk; ++i) {
      if (part_max[i] > worst) { worst = part_max[i]; dof = part_dof[i]; }   // the workgroups' dofs ascend: a tie keeps the smaller
      bad |= part_bad[i];
    }
    out->worst = worst; out->dof = dof; out->bad = bad;
  }
}
template <int NF>
__global__ __launch_bounds__(kVecBlock) void k_time_reduce(const double* part, const double* part_max, const int32_t* part_dof,
                                                           const int32_t* part_bad, int nblk, TimeReport* out) {
  time_reduce_body<NF>(part, part_max, part_dof, part_bad, nblk, out);
}

__global__ __launch_bounds__(kVecBlock) void k_time_shift(const double* u, double* un, double* unm1, int ndof) {
  const int i = blockIdx.x * kVecBlock + threadIdx.x;
  if (i < ndof) {
    const double a = u[i], b = un[i];
    un[i] = a; unm1[i] = b;
  }
}

}  // namespace gmpnp

namespace {

int time_prepare(gmpnp_solver* s, const char* what) {
  if (s->partitioned) return fail(GMPNP_ERR_INVALID, std::string(what) + ": partition handles have no adaptive time stepping (the groups' transports all-reduce sums; the estimator's maximum is not one)");
  if (!(s->nf == 7 || s->nf == 9)) return fail(GMPNP_ERR_INVALID, "unsupported (dim, n_fields)");
  HIP_TRY(hipSetDevice(s->opts.device_id));
  if (s->stepper) return GMPNP_OK;
  std::unique_ptr<gmpnp_time_stepper> T(new gmpnp_time_stepper);
  T->nblk = std::max(1, grid_for(s->t.nv, kVecBlock));
  HIP_TRY(T->unm1.alloc((size_t)s->ndof));
  HIP_TRY(T->part.alloc((size_t)kTimeCols * s->nf * T->nblk));
  HIP_TRY(T->part_max.alloc((size_t)T->nblk)); HIP_TRY(T->part_dof.alloc((size_t)T->nblk)); HIP_TRY(T->part_bad.alloc((size_t)T->nblk));
  HIP_TRY(hipHostMalloc((void**)&T->h_report, sizeof(TimeReport), hipHostMallocCoherent | hipHostMallocMapped));
  std::memset(T->h_report, 0, sizeof(TimeReport));
  { void* dp = nullptr; HIP_TRY(hipHostGetDevicePointer(&dp, T->h_report, 0)); T->d_report = (TimeReport*)dp; }
  s->stepper = std::move(T);
  return GMPNP_OK;
}

// the estimator's arguments of one handle; without history u_nm1 is not read as a state (ratio = 0: p = u_n)
TimeErrorIo time_error_io(const gmpnp_solver* s, double h, double h_prev, bool history, const gmpnp_time_tol_t& tol) {
  const gmpnp_time_stepper* T = s->stepper.get();
  TimeErrorIo io{};
  io.u = s->u.p; io.un = s->un.p; io.unm1 = history ? T->unm1.p : s->un.p; io.bcflag = s->bcflag.p;
  io.part = T->part.p; io.part_max = T->part_max.p; io.part_dof = T->part_dof.p; io.part_bad = T->part_bad.p;
  io.nv = s->t.nv; io.nblk = T->nblk;
  io.ratio = history ? h / h_prev : 0.0;
  io.scale = history ? h / (2.0 * h + h_prev) : 0.0;
  io.inv_h = 1.0 / h;
  io.rtol = tol.rtol;
  for (int f = 0; f < s->nf; ++f) io.atol[f] = tol.atol[f];
  return io;
}

// estimator + reduce on the handle's stream
template <int NF>
int time_error_launch(gmpnp_solver* s, double h, double h_prev, bool history, const gmpnp_time_tol_t& tol) {
  gmpnp_time_stepper* T = s->stepper.get();
  const TimeErrorIo io = time_error_io(s, h, h_prev, history, tol);
  hipLaunchKernelGGL((k_time_error<NF>), dim3(T->nblk), dim3(kVecBlock), 0, s->stream, io);
  hipLaunchKernelGGL((k_time_reduce<NF>), dim3(1), dim3(kVecBlock), 0, s->stream, (const double*)T->part.p, (const double*)T->part_max.p,
                     (const int32_t*)T->part_dof.p, (const int32_t*)T->part_bad.p, T->nblk, T->d_report);
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

int time_shift3_launch(gmpnp_solver* s);   // gmpnp_time_order.h

int time_shift_launch(gmpnp_solver* s) {
  hipLaunchKernelGGL(k_time_shift, dim3(grid_for(s->ndof, kVecBlock)), dim3(kVecBlock), 0, s->stream, (const double*)s->u.p, s->un.p,
                     s->stepper->unm1.p, s->ndof);
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

// gmpnp_time_kernel(22): estimator + reduce + shift.  The shift moves u into u_n, so the timing hook saves u_n and u_nm1 in front
// of its launches and restores them behind (time_kernel_begin / _end below).
int time_launch_any(gmpnp_solver* s) {
  gmpnp_time_tol_t tol{}; tol.rtol = 1e-2;
  for (int f = 0; f <= GMPNP_MAX_SPECIES; ++f) tol.atol[f] = 1e-4;
  int rc;
  if (s->nf == 9) rc = time_error_launch<9>(s, 1.0, 1.0, true, tol); else rc = time_error_launch<7>(s, 1.0, 1.0, true, tol);
  if (rc) return rc;
  return time_shift_launch(s);
}

// the timing hook's bracket: u_n and u_nm1 as they were, history flag untouched
int time_kernel_begin(gmpnp_solver* s, DevBuf<double>& keep) {
  int rc = time_prepare(s, "gmpnp_time_kernel"); if (rc) return rc;
  HIP_TRY(keep.alloc((size_t)2 * s->ndof, false));
  HIP_TRY(hipMemcpyAsync(keep.p, s->un.p, (size_t)s->ndof * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(keep.p + s->ndof, s->stepper->unm1.p, (size_t)s->ndof * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
  return GMPNP_OK;
}
int time_kernel_end(gmpnp_solver* s, DevBuf<double>& keep) {
  HIP_TRY(hipMemcpyAsync(s->un.p, keep.p, (size_t)s->ndof * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(s->stepper->unm1.p, keep.p + s->ndof, (size_t)s->ndof * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return GMPNP_OK;
}

// model.inv_dt of the handle and of every coarse level below it (gmpnp_attach_coarse_level): the time term is the diagonal of the
// species blocks
int time_step_apply(gmpnp_solver* s, double inv_dt) {
  for (gmpnp_solver* l = s; l; l = l->ml_coarse) {
    HIP_TRY(hipSetDevice(l->opts.device_id));
    HIP_TRY(hipStreamSynchronize(l->stream));
    if (l->stream2) HIP_TRY(hipStreamSynchronize(l->stream2));
    l->model.inv_dt = inv_dt;
    HIP_TRY(hipMemcpy(l->d_model.p, &l->model, sizeof(gmpnp_model_t), hipMemcpyHostToDevice));
    l->jacobian_valid = false; l->precond_valid = false;
    tangent_drop(l);
  }
  return GMPNP_OK;
}

// the argument rules of gmpnp_time_error (nullptr = fine, else the message without its prefix)
const char* time_error_invalid(double h, double h_prev, const gmpnp_time_tol_t& tol, int nf) {
  if (!(h > 0.0) || std::isinf(h) || h_prev != h_prev || std::isinf(h_prev)) return "h must be positive and finite, h_prev finite";
  if (!(tol.rtol >= 0.0) || std::isinf(tol.rtol)) return "rtol must be finite and >= 0";
  for (int f = 0; f < nf; ++f)
    if (!(tol.atol[f] > 0.0) || std::isinf(tol.atol[f])) return "every field's atol must be positive and finite";
  return nullptr;
}

// what the caller gets from the device's report
gmpnp_time_error_t time_report_result(const gmpnp_solver* s, const TimeReport& r, bool history) {
  const int nf = s->nf;
  gmpnp_time_error_t e{};
  e.has_history = history ? 1 : 0; e.nonfinite = r.bad ? 1 : 0;
  e.worst_dof = -1;
  bool nan_err = false, nan_rate = false;
  for (int f = 0; f < nf; ++f) {
    const double n = r.n_free[f];
    e.err_field[f] = (history && n > 0.0) ? std::sqrt(r.sum_err[f] / n) : 0.0;
    e.rate_field[f] = n > 0.0 ? std::sqrt(r.sum_rate[f] / n) : 0.0;
    if (r.bad) { e.err_field[f] = NAN; e.rate_field[f] = NAN; }
    nan_err |= e.err_field[f] != e.err_field[f]; nan_rate |= e.rate_field[f] != e.rate_field[f];
    if (e.err_field[f] > e.err) e.err = e.err_field[f];
    if (e.rate_field[f] > e.rate) e.rate = e.rate_field[f];
  }
  if (nan_err) e.err = NAN;      // a NaN never wins a comparison
  if (nan_rate) e.rate = NAN;
  if (!r.bad && history && r.dof >= 0) e.worst_dof = (int64_t)s->t.perm[r.dof / nf] * nf + r.dof % nf;
  return e;
}

}  // namespace

extern "C" {

int gmpnp_set_time_step(gmpnp_solver* s, double inv_dt) {
  if (!s) return fail(GMPNP_ERR_INVALID, "NULL handle");
  if (s->partitioned) return fail(GMPNP_ERR_INVALID, "gmpnp_set_time_step: partition handles have no adaptive time stepping");
  if (!time_step_valid(inv_dt)) return fail(GMPNP_ERR_INVALID, "gmpnp_set_time_step: inv_dt must be finite and >= 0 (0 = steady form)");
  time_read_un(s);   // a backward Euler step: the time term reads u_n (it may have read u* since gmpnp_set_time_step_bdf2)
  return time_step_apply(s, inv_dt);
}

int gmpnp_time_error(gmpnp_solver* s, double h, double h_prev, const gmpnp_time_tol_t* tol, gmpnp_time_error_t* out) {
  if (!s || !tol || !out) return fail(GMPNP_ERR_INVALID, "gmpnp_time_error: NULL argument");
  if (const char* why = time_error_invalid(h, h_prev, *tol, 0)) return fail(GMPNP_ERR_INVALID, std::string("gmpnp_time_error: ") + why);
  int rc = time_prepare(s, "gmpnp_time_error"); if (rc) return rc;
  const int nf = s->nf;
  if (const char* why = time_error_invalid(h, h_prev, *tol, nf)) return fail(GMPNP_ERR_INVALID, std::string("gmpnp_time_error: ") + why);
  gmpnp_time_stepper* T = s->stepper.get();
  const bool history = T->has_history && h_prev > 0.0;
  if (nf == 9) rc = time_error_launch<9>(s, h, h_prev, history, *tol); else rc = time_error_launch<7>(s, h, h_prev, history, *tol);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  *out = time_report_result(s, *T->h_report, history);
  return GMPNP_OK;
}

int gmpnp_time_accept(gmpnp_solver* s) {
  if (!s) return fail(GMPNP_ERR_INVALID, "NULL handle");
  int rc = time_prepare(s, "gmpnp_time_accept"); if (rc) return rc;
  // stream-ordered like gmpnp_assign_previous: whatever reads u_n / u_nm1 next is launched behind the pass
  rc = s->stepper->order == 2 ? time_shift3_launch(s) : time_shift_launch(s); if (rc) return rc;
  s->stepper->accepted();
  if (galvanostat_on(s)) return galvanostat_shift(s, true);
  return GMPNP_OK;
}

int gmpnp_time_reject(gmpnp_solver* s) {
  if (!s) return fail(GMPNP_ERR_INVALID, "NULL handle");
  int rc = time_prepare(s, "gmpnp_time_reject"); if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(s->u.p, s->un.p, (size_t)s->ndof * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
  s->state_jumped = true; s->jacobian_valid = false;
  tangent_drop(s);
  if (galvanostat_on(s)) return galvanostat_shift(s, false);
  return GMPNP_OK;
}

}  // extern "C"
