// Second-order adaptive time stepping on the device: variable-step BDF2 (include/gmpnp.h: gmpnp_set_time_order,
// gmpnp_set_time_step_bdf2, gmpnp_time_error_bdf2, gmpnp_time_history_levels, gmpnp_get_time_history; the coefficients and the
// accept / reject rule are host code: gmpnp_host_rules.h).  The time term of the element pass and of the budgets is
// inv_dt M (u - c.un); a BDF2 step of length h after an accepted step h_prev, omega = h / h_prev, has exactly that shape:
//     (alpha0 / h) M (u - u*)      alpha0 = (1 + 2 omega)/(1 + omega)      u* = ((1 + omega)^2 u_n - omega^2 u_nm1)/(1 + 2 omega)
// so no element, gather, Jacobian, preconditioner or solver kernel knows about the order: the set-up writes alpha0 inv_dt into the
// model, forms u* and points c.un at it.  The estimator, over the free dofs as at order 1 (gmpnp_time_step.h):
//     p = wn u_n + wm1 u_nm1 + wm2 u_nm2          the quadratic through the last three accepted states, at t + h
//     d = (u - p) kappa                           kappa = c / (h + h1 + h2 + c), c = h / alpha0: BDF2's share of u - p
//     w = atol_f + rtol max(|u|, |u_n|)           err_f, rate_f, worst_dof and the NaN flag as at order 1
//
//   k_time_history   u* = a u_n - b u_nm1, one pass
//   k_time_error2    k_time_error with p formed while the rows stream in (gmpnp_time_error2_body.inc): LDS holds u, u_n and p, the
//                    order-1 footprint; its partial rows go to k_time_reduce unchanged
//   k_time_shift3    the accept as one pass: u_nm2 <- u_nm1 <- u_n <- u
// u_nm2 and u* are allocated by the first call that asks for order 2; a handle that never does keeps the buffers, launches and
// branches of order 1.  Included at the end of gmpnp_api.hip, behind gmpnp_time_step.h.
#pragma once

namespace gmpnp {

struct TimeError2Io {
  const double* u; const double* un; const double* unm1; const double* unm2;   // [nv][NF] internal order
  const uint8_t* bcflag;                                                       // [nv][NF]
  double* part;                                                                // [kTimeCols * NF][nblk]
  double* part_max; int32_t* part_dof; int32_t* part_bad;                      // [nblk]
  int32_t nv, nblk;
  double wn, wm1, wm2;   // the predictor's weights (1, 0, 0 without history: p = u_n)
  double kappa;          // 0 without history
  double inv_h;
  double rtol, atol[GMPNP_MAX_SPECIES + 1];
};

__global__ __launch_bounds__(kVecBlock) void k_time_history(const double* __restrict__ un, const double* __restrict__ unm1,
                                                            double* __restrict__ ustar, double a, double b, int ndof) {
  const int i = blockIdx.x * kVecBlock + threadIdx.x;
  if (i < ndof) ustar[i] = a * un[i] - b * unm1[i];
}

template <int NF>
__global__ __launch_bounds__(kVecBlock) void k_time_error2(const TimeError2Io io) {
#include "gmpnp_time_error2_body.inc"
}

__global__ __launch_bounds__(kVecBlock) void k_time_shift3(const double* u, double* un, double* unm1, double* unm2, int ndof) {
  const int i = blockIdx.x * kVecBlock + threadIdx.x;
  if (i < ndof) {
    const double a = u[i], b = un[i], c = unm1[i];
    un[i] = a; unm1[i] = b; unm2[i] = c;
  }
}

}  // namespace gmpnp

namespace {

// the order-1 storage (time_prepare) and the two vectors of order 2
int time_order_prepare(gmpnp_solver* s, const char* what) {
  int rc = time_prepare(s, what); if (rc) return rc;
  gmpnp_time_stepper* T = s->stepper.get();
  if (!T->unm2.p) HIP_TRY(T->unm2.alloc((size_t)s->ndof));
  if (!T->ustar.p) { HIP_TRY(T->ustar.alloc((size_t)s->ndof)); T->star_formed = false; }
  return GMPNP_OK;
}

int time_history_launch(gmpnp_solver* s, double omega) {
  gmpnp_time_stepper* T = s->stepper.get();
  const std::pair<double, double> ab = bdf2_history_weights(omega);
  hipLaunchKernelGGL(k_time_history, dim3(grid_for(s->ndof, kVecBlock)), dim3(kVecBlock), 0, s->stream, (const double*)s->un.p,
                     (const double*)T->unm1.p, T->ustar.p, ab.first, ab.second, s->ndof);
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

// the estimator's arguments; without history neither u_nm1 nor u_nm2 is read as a state (p = u_n, kappa = 0)
TimeError2Io time_error2_io(const gmpnp_solver* s, double h, double h1, double h2, bool history, const gmpnp_time_tol_t& tol) {
  const gmpnp_time_stepper* T = s->stepper.get();
  TimeError2Io io{};
  io.u = s->u.p; io.un = s->un.p; io.unm1 = history ? T->unm1.p : s->un.p; io.unm2 = history ? T->unm2.p : s->un.p;
  io.bcflag = s->bcflag.p;
  io.part = T->part.p; io.part_max = T->part_max.p; io.part_dof = T->part_dof.p; io.part_bad = T->part_bad.p;
  io.nv = s->t.nv; io.nblk = T->nblk;
  if (history) {
    const TimePredictor w = bdf2_predictor_weights(h, h1, h2);
    io.wn = w.wn; io.wm1 = w.wm1; io.wm2 = w.wm2; io.kappa = bdf2_error_share(h, h1, h2);
  } else { io.wn = 1.0; io.wm1 = 0.0; io.wm2 = 0.0; io.kappa = 0.0; }
  io.inv_h = 1.0 / h;
  io.rtol = tol.rtol;
  for (int f = 0; f < s->nf; ++f) io.atol[f] = tol.atol[f];
  return io;
}

// estimator + reduce on the handle's stream
template <int NF>
int time_error2_launch(gmpnp_solver* s, double h, double h1, double h2, bool history, const gmpnp_time_tol_t& tol) {
  gmpnp_time_stepper* T = s->stepper.get();
  const TimeError2Io io = time_error2_io(s, h, h1, h2, history, tol);
  hipLaunchKernelGGL((k_time_error2<NF>), dim3(T->nblk), dim3(kVecBlock), 0, s->stream, io);
  hipLaunchKernelGGL((k_time_reduce<NF>), dim3(1), dim3(kVecBlock), 0, s->stream, (const double*)T->part.p, (const double*)T->part_max.p,
                     (const int32_t*)T->part_dof.p, (const int32_t*)T->part_bad.p, T->nblk, T->d_report);
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

int time_shift3_launch(gmpnp_solver* s) {
  gmpnp_time_stepper* T = s->stepper.get();
  hipLaunchKernelGGL(k_time_shift3, dim3(grid_for(s->ndof, kVecBlock)), dim3(kVecBlock), 0, s->stream, (const double*)s->u.p, s->un.p,
                     T->unm1.p, T->unm2.p, s->ndof);
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

// gmpnp_time_kernel(23): history + estimator + reduce + three-deep shift, between a bracket that keeps u_n, u_nm1 and u_nm2 (the
// order, the levels and c.un stay as they are: u* is written, not read)
int time_launch_any2(gmpnp_solver* s) {
  gmpnp_time_tol_t tol{}; tol.rtol = 1e-2;
  for (int f = 0; f <= GMPNP_MAX_SPECIES; ++f) tol.atol[f] = 1e-4;
  int rc = time_history_launch(s, 1.0); if (rc) return rc;
  if (s->nf == 9) rc = time_error2_launch<9>(s, 1.0, 1.0, 1.0, true, tol); else rc = time_error2_launch<7>(s, 1.0, 1.0, 1.0, true, tol);
  if (rc) return rc;
  return time_shift3_launch(s);
}
int time_kernel_begin2(gmpnp_solver* s, DevBuf<double>& keep) {
  int rc = time_order_prepare(s, "gmpnp_time_kernel"); if (rc) return rc;
  const size_t n = (size_t)s->ndof, bytes = n * sizeof(double);
  HIP_TRY(keep.alloc(3 * n, false));
  HIP_TRY(hipMemcpyAsync(keep.p, s->un.p, bytes, hipMemcpyDeviceToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(keep.p + n, s->stepper->unm1.p, bytes, hipMemcpyDeviceToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(keep.p + 2 * n, s->stepper->unm2.p, bytes, hipMemcpyDeviceToDevice, s->stream));
  return GMPNP_OK;
}
int time_kernel_end2(gmpnp_solver* s, DevBuf<double>& keep) {
  const size_t n = (size_t)s->ndof, bytes = n * sizeof(double);
  HIP_TRY(hipMemcpyAsync(s->un.p, keep.p, bytes, hipMemcpyDeviceToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(s->stepper->unm1.p, keep.p + n, bytes, hipMemcpyDeviceToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(s->stepper->unm2.p, keep.p + 2 * n, bytes, hipMemcpyDeviceToDevice, s->stream));
  s->stepper->star_formed = false;   // u* holds the hook's vector
  HIP_TRY(hipStreamSynchronize(s->stream));
  return GMPNP_OK;
}

}  // namespace

extern "C" {

int gmpnp_set_time_order(gmpnp_solver* s, int32_t order) {
  if (!s) return fail(GMPNP_ERR_INVALID, "NULL handle");
  if (order != 1 && order != 2) return fail(GMPNP_ERR_INVALID, "gmpnp_set_time_order: the order is 1 (backward Euler) or 2 (variable-step BDF2)");
  if (order == 1 && !s->stepper && !s->partitioned) return GMPNP_OK;   // nothing to undo: the handle stays as it was
  if (order == 2 && galvanostat_on(s)) return fail(GMPNP_ERR_INVALID, "gmpnp_set_time_order: the galvanostat is on (gmpnp_set_galvanostat): p_M has no second-order history");
  int rc = order == 2 ? time_order_prepare(s, "gmpnp_set_time_order") : time_prepare(s, "gmpnp_set_time_order"); if (rc) return rc;
  gmpnp_time_stepper* T = s->stepper.get();
  T->order = order;
  if (order == 1) {
    if (s->c.un != s->un.p) { s->jacobian_valid = false; time_read_un(s); }
    T->levels = std::min(T->levels, 1);
  }
  return GMPNP_OK;
}

int gmpnp_time_history_levels(gmpnp_solver* s, int32_t* levels) {
  if (!s || !levels) return fail(GMPNP_ERR_INVALID, "gmpnp_time_history_levels: NULL argument");
  if (s->partitioned) return fail(GMPNP_ERR_INVALID, "gmpnp_time_history_levels: partition handles have no adaptive time stepping");
  *levels = s->stepper ? s->stepper->levels : 0;
  return GMPNP_OK;
}

int gmpnp_set_time_step_bdf2(gmpnp_solver* s, double inv_dt, double ratio) {
  if (!s) return fail(GMPNP_ERR_INVALID, "NULL handle");
  if (s->partitioned) return fail(GMPNP_ERR_INVALID, "gmpnp_set_time_step_bdf2: partition handles have no adaptive time stepping");
  if (!time_step_valid(inv_dt)) return fail(GMPNP_ERR_INVALID, "gmpnp_set_time_step_bdf2: inv_dt must be finite and >= 0");
  if (!time_ratio_valid(ratio)) return fail(GMPNP_ERR_INVALID, "gmpnp_set_time_step_bdf2: ratio = h / h_prev must be finite and > 0");
  if (!s->stepper || s->stepper->order != 2) return fail(GMPNP_ERR_INVALID, "gmpnp_set_time_step_bdf2: the handle is not at order 2 (gmpnp_set_time_order)");
  if (s->stepper->levels < 1) return fail(GMPNP_ERR_INVALID, "gmpnp_set_time_step_bdf2: an order-2 step needs an accepted state before u_n (gmpnp_time_accept)");
  HIP_TRY(hipSetDevice(s->opts.device_id));
  int rc = time_history_launch(s, ratio); if (rc) return rc;
  rc = time_step_apply(s, bdf2_alpha0(ratio) * inv_dt); if (rc) return rc;   // (synchronises the stream: u* is formed)
  s->c.un = s->stepper->ustar.p; s->stepper->star_formed = true;
  return GMPNP_OK;
}

int gmpnp_time_error_bdf2(gmpnp_solver* s, double h, double h_prev, double h_prev2, const gmpnp_time_tol_t* tol, gmpnp_time_error_t* out) {
  if (!s || !tol || !out) return fail(GMPNP_ERR_INVALID, "gmpnp_time_error_bdf2: NULL argument");
  if (h_prev2 != h_prev2 || std::isinf(h_prev2)) return fail(GMPNP_ERR_INVALID, "gmpnp_time_error_bdf2: h_prev2 must be finite");
  if (const char* why = time_error_invalid(h, h_prev, *tol, 0)) return fail(GMPNP_ERR_INVALID, std::string("gmpnp_time_error_bdf2: ") + why);
  int rc = time_prepare(s, "gmpnp_time_error_bdf2"); if (rc) return rc;
  const int nf = s->nf;
  if (const char* why = time_error_invalid(h, h_prev, *tol, nf)) return fail(GMPNP_ERR_INVALID, std::string("gmpnp_time_error_bdf2: ") + why);
  gmpnp_time_stepper* T = s->stepper.get();
  const bool history = T->levels >= 2 && h_prev > 0.0 && h_prev2 > 0.0;
  if (nf == 9) rc = time_error2_launch<9>(s, h, h_prev, h_prev2, history, *tol); else rc = time_error2_launch<7>(s, h, h_prev, h_prev2, history, *tol);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  *out = time_report_result(s, *T->h_report, history);
  return GMPNP_OK;
}

int gmpnp_get_time_history(gmpnp_solver* s, double* out) {
  if (!s || !out) return fail(GMPNP_ERR_INVALID, "gmpnp_get_time_history: NULL argument");
  if (s->partitioned) return fail(GMPNP_ERR_INVALID, "gmpnp_get_time_history: partition handles have no adaptive time stepping");
  if (!s->stepper || !s->stepper->star_formed) return fail(GMPNP_ERR_INVALID, "gmpnp_get_time_history: no u* was formed (gmpnp_set_time_step_bdf2)");
  HIP_TRY(hipSetDevice(s->opts.device_id));
  return download_vec(s, s->stepper->ustar.p, out);
}

}  // extern "C"
