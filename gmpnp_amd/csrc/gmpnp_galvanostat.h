// Galvanostatic mode on the device: gmpnp_set_galvanostat / gmpnp_galvanostat_report / gmpnp_galvanostat_terms (include/gmpnp.h),
// rule in gmpnp_host_rules.h (galvanostat_step).
//
// The electrode potential p_M is one more unknown and G = ln(I / I_target) = 0 one more equation (I = sum_r weight_r I_r, I_r the
// integrated rates of gmpnp_kinetics.h).  One Newton iteration by block elimination, sign convention u <- u - omega dx:
//     J y = F,  J z = b,  dp = (G - c.y) / (d - c.z),  dx = y - dp z,  u -= omega alpha dx,  p_M -= omega alpha dp
//     b = dF/dp_M   Stern rows: 1D g / lam, 3D sum over the node's Stern facets in list order of g(eps_f) |f| / (3 lam)
//                   kinetic rows: -w_I sum_r nu[r][i] alpha_r rate_r;  0 on every Dirichlet row and everywhere else
//     c = dG/du     at boundary node I: column reactant_r: weight_r w_I k_r E_r / I,  column p: weight_r w_I alpha_r rate_r / I
//     d = dG/dp_M = -sum_r weight_r alpha_r I_r / I
//
//   k_galv_rhs        one lane per boundary node (the Stern nodes and the kinetics' nodes are one ascending list): its Stern facets in
//                     list order -> b[p row], its rates -> b[species rows]; the Dirichlet flags are read at run time (such a row: 0)
//   k_galv_reduce     one workgroup, fixed order: I_r, and with `full` c.y and c.z, straight from u, y and z; thread 0 then forms I,
//                     G, d and dp by the host + device rule and writes the device scalars and the pinned report.  Without `full`: I_r,
//                     I and G alone, for the convergence test at a new state (queued in front of the residual evaluation, read behind
//                     ITS synchronisation).  A verdict that is not ok: status bit 128, dp = 0.
//   k_galv_direction  kx = y - dp z (zero where the verdict was not ok: the update that follows applies nothing)
//   k_galv_potential  p_M -= omega alpha dp, alpha from the step limiter's report where the limiter is on; the new value also goes
//                     into the kinetics' device option (an ordinary store), which k_kinetics_* read, and into the report
// p_M lives in scal[0], its value at u_n in scal[1]; the Stern kernels read scal[0] through SternTab::p_M_dev.  Every sum is a gather
// in a fixed order (no floating-point atomics): two calls on one state give equal bits.  The reactant's entry of y and z is picked by
// selects out of unrolled loops, not by indexing a register array.  No synchronisation of its own per iteration.
// Included at the end of gmpnp_api.hip.
#pragma once

namespace gmpnp {

constexpr int kGalvScalars = 8;   // 0: p_M  1: p_M at u_n  2: dp  3: verdict (1 ok)  4, 5: dp and verdict of the hooks' reduce

// what thread 0 of k_galv_reduce and k_galv_potential leave for the host (pinned memory)
struct GalvReport {
  double p_M, p_M_n;
  double I_r[GMPNP_MAX_SURFACE_REACTIONS];
  double I, G, cy, cz, d, dp, alpha;
  int32_t bad, pad_;
};

struct GalvIo {
  double target;
  double weight[GMPNP_MAX_SURFACE_REACTIONS];
  const double* y; const double* z;   // [nv][NF] internal order (full only)
  double* scal;                       // the galvanostat's device scalars
  int32_t slot;                       // where dp and the verdict go: 2 (the solve) or 4 (the hooks)
  int32_t full;
  GalvReport* report;
  int32_t* status;
};

template <int DIM, int NF>
__global__ __launch_bounds__(kVecBlock) void k_galv_rhs(const Ctx c, const KinTab t, const SternTab st, const int stern, double* __restrict__ b) {
  constexpr int NS = NF - 1;
  const int n = blockIdx.x * kVecBlock + threadIdx.x;
  if (n >= t.n_nodes) return;
  const size_t row0 = (size_t)t.node[n] * NF;
  double uu[NF];
#pragma unroll
  for (int j = 0; j < NF; ++j) uu[j] = c.u[row0 + j];
  KinRate R[GMPNP_MAX_SURFACE_REACTIONS];
  kinetics_rates<NF>(t, uu, R);
  const gmpnp_kinetics_t* o = t.opt;
  const int nr = o->n_reactions;
  const double w = t.w[n];
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    double term = 0.0;
    bool driven = false;
#pragma unroll
    for (int r = 0; r < GMPNP_MAX_SURFACE_REACTIONS; ++r)
      if (r < nr) { const double nu = o->nu[r][i]; term += nu * R[r].d_p; driven = driven || nu != 0.0; }   // d_p = alpha rate
    b[row0 + i] = (driven && !c.bcflag[row0 + i]) ? -(w * term) : 0.0;
  }
  double sb = 0.0;
  if (stern && !c.bcflag[row0 + NS]) {   // (st.node[n] == t.node[n]: checked when the option is set)
    for (int k = st.nf_ptr[n]; k < st.nf_ptr[n + 1]; ++k) {
      const SternFacet<DIM, NF> F(c, st, st.nf_ent[k] >> 2);
      sb += F.G.g * (DIM == 3 ? F.area / 3.0 : 1.0) / st.lam;
    }
  }
  b[row0 + NS] = sb;
}

template <int NF>
__global__ __launch_bounds__(kVecBlock) void k_galv_reduce(const Ctx c, const KinTab t, const GalvIo g) {
  constexpr int NS = NF - 1, K = GMPNP_MAX_SURFACE_REACTIONS + 2;
  __shared__ double lds[4 * K];
  const gmpnp_kinetics_t* o = t.opt;
  const int nr = o->n_reactions;
  double v[K];
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = 0.0;
  for (int n = threadIdx.x; n < t.n_nodes; n += kVecBlock) {
    const size_t row0 = (size_t)t.node[n] * NF;
    double uu[NF];
#pragma unroll
    for (int j = 0; j < NF; ++j) uu[j] = c.u[row0 + j];
    KinRate R[GMPNP_MAX_SURFACE_REACTIONS];
    kinetics_rates<NF>(t, uu, R);
    const double w = t.w[n];
#pragma unroll
    for (int r = 0; r < GMPNP_MAX_SURFACE_REACTIONS; ++r) v[r] += w * R[r].rate;
    if (g.full) {
      double yy[NF], zz[NF];
#pragma unroll
      for (int j = 0; j < NF; ++j) { yy[j] = g.y[row0 + j]; zz[j] = g.z[row0 + j]; }
      double cy = 0.0, cz = 0.0;
#pragma unroll
      for (int r = 0; r < GMPNP_MAX_SURFACE_REACTIONS; ++r)
        if (r < nr) {
          const int re = o->reactant[r];
          double yr = 0.0, zr = 0.0;
#pragma unroll
          for (int j = 0; j < NS; ++j) { yr = (j == re) ? yy[j] : yr; zr = (j == re) ? zz[j] : zr; }
          const double du = re >= 0 ? R[r].d_u : 0.0;
          cy += g.weight[r] * (du * yr + R[r].d_p * yy[NS]);
          cz += g.weight[r] * (du * zr + R[r].d_p * zz[NS]);
        }
      v[GMPNP_MAX_SURFACE_REACTIONS] += w * cy;
      v[GMPNP_MAX_SURFACE_REACTIONS + 1] += w * cz;
    }
  }
  block_sum<K>(v, lds);
  if (threadIdx.x != 0) return;
  double I = 0.0, A = 0.0;
#pragma unroll
  for (int r = 0; r < GMPNP_MAX_SURFACE_REACTIONS; ++r)
    if (r < nr) { I += g.weight[r] * v[r]; A += g.weight[r] * (o->alpha[r] * v[r]); }
  GalvReport* rep = g.report;
  GalvStep s;
  if (g.full) {
    const double cy = v[GMPNP_MAX_SURFACE_REACTIONS] / I, cz = v[GMPNP_MAX_SURFACE_REACTIONS + 1] / I, d = -A / I;
    s = galvanostat_step(I, g.target, cy, cz, d);
    rep->cy = cy; rep->cz = cz; rep->d = d; rep->dp = s.dp;
    g.scal[g.slot] = s.ok ? s.dp : 0.0;
    g.scal[g.slot + 1] = s.ok ? 1.0 : 0.0;
  } else {
    s = galvanostat_constraint(I, g.target);
  }
#pragma unroll
  for (int r = 0; r < GMPNP_MAX_SURFACE_REACTIONS; ++r) rep->I_r[r] = v[r];
  rep->I = I; rep->G = s.G; rep->bad = s.ok ? 0 : 1;
  rep->p_M = g.scal[0]; rep->p_M_n = g.scal[1];
  if (!s.ok) atomicOr(g.status, 128);
}

__global__ __launch_bounds__(kVecBlock) void k_galv_direction(double* __restrict__ kx, const double* __restrict__ y, const double* __restrict__ z,
                                                              const double* __restrict__ scal, int slot, int n) {
  const int i = blockIdx.x * kVecBlock + threadIdx.x;
  if (i >= n) return;
  const double dp = scal[slot];
  kx[i] = scal[slot + 1] != 0.0 ? y[i] - dp * z[i] : 0.0;
}

// limiter: the step limiter's report (its alpha is NaN where it applied nothing), or nullptr: alpha = 1
__global__ void k_galv_potential(double* __restrict__ scal, int slot, gmpnp_kinetics_t* __restrict__ opt, GalvReport* __restrict__ report,
                                 const StepReport* limiter, double omega) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double alpha = limiter ? limiter->alpha : 1.0;
  const double step = alpha == alpha ? omega * alpha : 0.0;
  const double p = scal[0] - step * scal[slot];
  scal[0] = p;
  opt->p_electrode = p;
  report->p_M = p; report->alpha = alpha;
}

}  // namespace gmpnp

namespace {

GalvIo galvanostat_io(gmpnp_solver* s, bool full, const double* y, const double* z, int slot, int which_report, int32_t* status) {
  gmpnp_galvanostat* G = s->galvanostat.get();
  GalvIo g{};
  g.target = G->opt.target;
  for (int r = 0; r < GMPNP_MAX_SURFACE_REACTIONS; ++r) g.weight[r] = G->opt.weight[r];
  g.y = y; g.z = z; g.scal = G->scal.p; g.slot = slot; g.full = full ? 1 : 0;
  g.report = G->d_report + which_report; g.status = status;
  return g;
}

int galvanostat_launch_rhs(gmpnp_solver* s, int32_t* status) {
  const KinTab t = kinetics_tab(s, status);
  const int stern = stern_on(s) ? 1 : 0;
  SternTab st{};
  if (stern) st = stern_tab(s, status);
  GMPNP_DISPATCH(s, hipLaunchKernelGGL((k_galv_rhs<DIM, NF>), dim3(grid_for(t.n_nodes, kVecBlock)), dim3(kVecBlock), 0, s->stream, s->c, t, st, stern,
                                       s->galvanostat->b.p));
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

int galvanostat_launch_reduce(gmpnp_solver* s, bool full, const double* y, const double* z, int slot, int which_report, int32_t* status) {
  const KinTab t = kinetics_tab(s, status);
  const GalvIo g = galvanostat_io(s, full, y, z, slot, which_report, status);
  GMPNP_DISPATCH(s, hipLaunchKernelGGL((k_galv_reduce<NF>), dim3(1), dim3(kVecBlock), 0, s->stream, s->c, t, g));
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

int galvanostat_launch_direction(gmpnp_solver* s, double* kx, int slot) {
  gmpnp_galvanostat* G = s->galvanostat.get();
  hipLaunchKernelGGL(k_galv_direction, dim3(grid_for(s->ndof, kVecBlock)), dim3(kVecBlock), 0, s->stream, kx, (const double*)G->y.p, (const double*)G->z.p,
                     (const double*)G->scal.p, slot, (int)s->ndof);
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

int galvanostat_launch_potential(gmpnp_solver* s, int slot, int which_report, bool limited, double omega) {
  gmpnp_galvanostat* G = s->galvanostat.get();
  hipLaunchKernelGGL(k_galv_potential, dim3(1), dim3(kWave), 0, s->stream, G->scal.p, slot, s->kineticist->d_opt.p, G->d_report + which_report,
                     limited ? (const StepReport*)s->limiter->d_report : (const StepReport*)nullptr, omega);
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

// y = J^-1 F and z = J^-1 b with the Jacobian the stream holds (||F|| = r)
template <int DIM, int NF>
int galvanostat_solves(gmpnp_solver* s, const gmpnp_newton_options_t& o, gmpnp_newton_stats_t& st, double r) {
  gmpnp_galvanostat* G = s->galvanostat.get();
  const size_t bytes = (size_t)s->ndof * sizeof(double);
  if constexpr (DIM == 1) {
    int rc = tri_solve<NF>(s, s->F.p); if (rc) return rc;
    rc = tri_apply<NF>(s, G->y.p, 0.0, 1.0); if (rc) return rc;
    rc = tri_solve<NF>(s, G->b.p); if (rc) return rc;
    return tri_apply<NF>(s, G->z.p, 0.0, 1.0);
  } else {
    HIP_TRY(hipMemcpyAsync(s->kb.p, s->F.p, bytes, hipMemcpyDeviceToDevice, s->stream));
    int rc = band_factor<NF>(s); if (rc) return rc;
    const char* wild = "galvanostat: block-banded LU: the residual of a solve is not finite";
    double rn = 0.0;
    rc = band_refined_substitute<NF>(s, std::max(o.krylov_relative_tolerance * r, o.krylov_absolute_tolerance), &rn); if (rc) return rc;
    if (!rule_finite(rn)) return fail(GMPNP_ERR_LINEAR, wild);
    HIP_TRY(hipMemcpy(s->h_status, s->status.p, sizeof(int32_t), hipMemcpyDeviceToHost));
    if (*s->h_status & 2) return fail(GMPNP_ERR_LINEAR, "galvanostat: block-banded LU: singular pivot block");
    HIP_TRY(hipMemcpyAsync(G->y.p, s->kx.p, bytes, hipMemcpyDeviceToDevice, s->stream));
    // ||b||: the partial sums of b - 0
    HIP_TRY(hipMemcpyAsync(s->kb.p, G->b.p, bytes, hipMemcpyDeviceToDevice, s->stream));
    hipLaunchKernelGGL(k_true_residual, dim3(s->n_resblocks), dim3(kVecBlock), 0, s->stream, (const double*)s->kb.p, (const double*)G->zero.p, s->kr.p,
                       s->c.part_f, (int)s->ndof);
    HIP_TRY(hipStreamSynchronize(s->stream));
    const double bn = std::sqrt(sum_partials(s, 0));
    rc = band_refined_substitute<NF>(s, std::max(o.krylov_relative_tolerance * bn, o.krylov_absolute_tolerance), &rn); if (rc) return rc;
    if (!rule_finite(rn)) return fail(GMPNP_ERR_LINEAR, wild);
    HIP_TRY(hipMemcpyAsync(G->z.p, s->kx.p, bytes, hipMemcpyDeviceToDevice, s->stream));
    st.direct_solves++; s->x0.left(false);
    return GMPNP_OK;
  }
}

// the galvanostat's launches of one iteration apart from the two solves, on a zero step (gmpnp_time_kernel 26): the state and p_M stay
int galvanostat_launch_iteration(gmpnp_solver* s) {
  gmpnp_galvanostat* G = s->galvanostat.get();
  int32_t* st = G->status.p;
  int rc = galvanostat_launch_rhs(s, st); if (rc) return rc;
  rc = galvanostat_launch_reduce(s, true, G->y.p, G->z.p, 4, 1, st); if (rc) return rc;
  rc = galvanostat_launch_direction(s, G->x.p, 4); if (rc) return rc;
  rc = galvanostat_launch_potential(s, 4, 1, false, 0.0); if (rc) return rc;
  return galvanostat_launch_reduce(s, false, nullptr, nullptr, 4, 1, st);
}

// p_M -> its twin at u_n (assign_previous, accept), or back (reject); stream-ordered like the copies of u beside it
int galvanostat_shift(gmpnp_solver* s, bool to_previous) {
  gmpnp_galvanostat* G = s->galvanostat.get();
  double* sc = G->scal.p;
  if (to_previous) {
    HIP_TRY(hipMemcpyAsync(sc + 1, sc, sizeof(double), hipMemcpyDeviceToDevice, s->stream));
  } else {
    HIP_TRY(hipMemcpyAsync(sc, sc + 1, sizeof(double), hipMemcpyDeviceToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(&s->kineticist->d_opt.p->p_electrode, sc + 1, sizeof(double), hipMemcpyDeviceToDevice, s->stream));
  }
  return GMPNP_OK;
}

// gmpnp_newton_solve with the option on: newton()'s loop with the bordered step.  The residual the judge sees is sqrt(||F||^2 + G^2);
// G comes from a reduce queued in front of every residual evaluation and is read behind that evaluation's synchronisation.
template <int DIM, int NF>
int newton_galvanostat(gmpnp_solver* s, const gmpnp_newton_options_t& o, gmpnp_newton_stats_t& st) {
  gmpnp_galvanostat* G = s->galvanostat.get();
  const double t0 = now_ms();
  HIP_TRY(hipMemsetAsync(s->status.p, 0, sizeof(int32_t), s->stream));
  double r = 0.0; int flags = 0;
  auto bordered = [&](double* rr) -> int {
    int rc = galvanostat_launch_reduce(s, false, nullptr, nullptr, 2, 0, s->status.p); if (rc) return rc;
    rc = residual<DIM, NF>(s, true, &r, &flags); if (rc) return rc;   // synchronises the stream: the report has landed
    const double g = G->h_report->G;
    *rr = std::sqrt(r * r + g * g);
    return GMPNP_OK;
  };
  double rr = 0.0;
  const double ta = now_ms();
  int rc = bordered(&rr); if (rc) return rc;
  st.ms_assemble += now_ms() - ta;
  NewtonJudge judge(o, st, s->cfg.strict_steric != 0);
  NewtonJudge::Verdict v = judge.first(rr, flags);
  const bool limited = o.step_fraction != 0.0;
  if (limited) { rc = step_prepare(s); if (rc) return rc; }
  while (v == NewtonJudge::go_on) {
    rc = mark_phase(s, 0); if (rc) return rc;
    rc = launch_jac_gather<DIM, NF>(s); if (rc) return rc;   // element records: left by the last residual evaluation
    s->jacobian_valid = true;
    rc = mark_phase(s, 1); if (rc) return rc;
    rc = galvanostat_launch_rhs(s, s->status.p); if (rc) return rc;
    rc = mark_phase(s, 2); if (rc) return rc;
    rc = galvanostat_solves<DIM, NF>(s, o, st, r); if (rc) return rc;
    rc = galvanostat_launch_reduce(s, true, G->y.p, G->z.p, 2, 0, s->status.p); if (rc) return rc;
    rc = galvanostat_launch_direction(s, s->kx.p, 2); if (rc) return rc;
    if (limited) rc = step_launch<NF>(s, s->kx.p, s->kxp.p, o.relaxation_parameter, o.step_fraction, s->status.p);
    else hipLaunchKernelGGL(k_axpy, dim3(grid_for(s->ndof, 256)), dim3(256), 0, s->stream, s->u.p, (const double*)s->kx.p, -o.relaxation_parameter, (int)s->ndof);
    if (rc) return rc;
    rc = galvanostat_launch_potential(s, 2, 0, limited, o.relaxation_parameter); if (rc) return rc;
    rc = mark_phase(s, 3); if (rc) return rc;
    st.iterations++;
    rc = bordered(&rr); if (rc) return rc;
    if (limited) record_step(st, st.iterations - 1, s->limiter->h_report->alpha);
    rc = collect_phases(s, st); if (rc) return rc;
    v = judge.next(rr, flags);
  }
  s->x0.left(false);
  if (v == NewtonJudge::failed) return fail(judge.code, judge.message);
  s->state_jumped = false;
  st.ms_total = now_ms() - t0;
  return v == NewtonJudge::converged ? GMPNP_OK : fail(judge.code, judge.message);
}

// the current p_M of the device into the two options' host records (the stream is idle)
int galvanostat_read_p_M(gmpnp_solver* s, double* p) {
  HIP_TRY(hipStreamSynchronize(s->stream));
  HIP_TRY(hipMemcpy(p, s->galvanostat->scal.p, sizeof(double), hipMemcpyDeviceToHost));
  return GMPNP_OK;
}

}  // namespace

extern "C" {

int gmpnp_set_galvanostat(gmpnp_solver* s, const gmpnp_galvanostat_t* o) {
  if (!s || !o) return fail(GMPNP_ERR_INVALID, "galvanostat: NULL argument");
  if (!o->on && !s->galvanostat) return GMPNP_OK;   // never on: the handle stays as it was
  tangent_drop(s);
  HIP_TRY(hipSetDevice(s->opts.device_id));
  if (!o->on) {
    if (!galvanostat_on(s)) return GMPNP_OK;
    // the potential that was found goes into both options: a potentiostatic continuation holds it, by value again
    double p = 0.0;
    int rc = galvanostat_read_p_M(s, &p); if (rc) return rc;
    s->galvanostat->opt.on = 0;
    s->kineticist->opt.p_electrode = p;
    HIP_TRY(hipMemcpy(s->kineticist->d_opt.p, &s->kineticist->opt, sizeof(gmpnp_kinetics_t), hipMemcpyHostToDevice));
    if (s->sterner) s->sterner->opt.p_electrode = p;
    s->jacobian_valid = false; s->precond_valid = false;
    return GMPNP_OK;
  }
  if (s->partitioned) return fail(GMPNP_ERR_INVALID, "galvanostat: partition handles and groups are not supported");
  if (s->ml_coarse || s->ml_is_coarse) return fail(GMPNP_ERR_INVALID, "galvanostat: not with a multilevel coarse level attached");
  if (!kinetics_on(s)) return fail(GMPNP_ERR_INVALID, "galvanostat: the surface kinetics must be on (gmpnp_set_kinetics)");
  if (!galvanostat_options_valid(*o)) return fail(GMPNP_ERR_INVALID, "galvanostat: a finite target > 0 and finite weights that are not all zero");
  if (s->stepper && s->stepper->order == 2) return fail(GMPNP_ERR_INVALID, "galvanostat: not with order-2 time stepping (gmpnp_set_time_order)");
  HIP_TRY(hipStreamSynchronize(s->stream));
  const bool was_on = galvanostat_on(s);
  double p = s->kineticist->opt.p_electrode;
  if (was_on) { int rc = galvanostat_read_p_M(s, &p); if (rc) return rc; }   // a new target keeps the potential the handle is at
  else if (stern_on(s) && s->sterner->opt.p_electrode != p)
    return fail(GMPNP_ERR_INVALID, "galvanostat: the Stern option's p_electrode differs from the kinetics' (one electrode potential)");
  if (stern_on(s) && s->sterner->n_nodes != s->kineticist->n_nodes)
    return fail(GMPNP_ERR_INVALID, "galvanostat: the Stern boundary and the kinetics' boundary differ");
  if (!s->galvanostat) {
    std::unique_ptr<gmpnp_galvanostat> G(new gmpnp_galvanostat);
    HIP_TRY(G->scal.alloc(kGalvScalars)); HIP_TRY(G->status.alloc(1));
    HIP_TRY(G->b.alloc((size_t)s->ndof)); HIP_TRY(G->y.alloc((size_t)s->ndof)); HIP_TRY(G->z.alloc((size_t)s->ndof));
    HIP_TRY(G->x.alloc((size_t)s->ndof)); HIP_TRY(G->zero.alloc((size_t)s->ndof));
    HIP_TRY(hipHostMalloc((void**)&G->h_report, 2 * sizeof(GalvReport), hipHostMallocCoherent | hipHostMallocMapped));
    std::memset(G->h_report, 0, 2 * sizeof(GalvReport));
    { void* dp = nullptr; HIP_TRY(hipHostGetDevicePointer(&dp, G->h_report, 0)); G->d_report = (GalvReport*)dp; }
    s->galvanostat = std::move(G);
  }
  gmpnp_galvanostat* G = s->galvanostat.get();
  G->opt = *o;
  if (!was_on) {
    double sc[kGalvScalars] = {p, p, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    HIP_TRY(hipMemcpy(G->scal.p, sc, sizeof sc, hipMemcpyHostToDevice));
    std::memset(G->h_report, 0, 2 * sizeof(GalvReport));
    G->h_report[0].p_M = G->h_report[0].p_M_n = p;
  }
  s->jacobian_valid = false; s->precond_valid = false;
  return GMPNP_OK;
}

int gmpnp_galvanostat_report(gmpnp_solver* s, gmpnp_galvanostat_report_t* out) {
  if (!s || !out) return fail(GMPNP_ERR_INVALID, "galvanostat: NULL argument");
  if (!galvanostat_on(s)) return fail(GMPNP_ERR_INVALID, "galvanostat: the option is off (gmpnp_set_galvanostat)");
  HIP_TRY(hipSetDevice(s->opts.device_id));
  gmpnp_galvanostat* G = s->galvanostat.get();
  // currents and G at the u the stream holds, into the hooks' report; the last iteration's terms are the solve's
  int rc = galvanostat_launch_reduce(s, false, nullptr, nullptr, 4, 1, G->status.p); if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  const GalvReport now = G->h_report[1], last = G->h_report[0];
  out->p_electrode = now.p_M; out->p_electrode_n = now.p_M_n;
  for (int r = 0; r < GMPNP_MAX_SURFACE_REACTIONS; ++r) out->I_r[r] = now.I_r[r];
  out->I = now.I; out->G = now.G;
  out->cy = last.cy; out->cz = last.cz; out->d = last.d; out->dp = last.dp; out->alpha = last.alpha;
  return GMPNP_OK;
}

int gmpnp_galvanostat_terms(gmpnp_solver* s, const double* x, double* b_out, double* scalars) {
  if (!s || !scalars) return fail(GMPNP_ERR_INVALID, "galvanostat: NULL argument");
  if (!galvanostat_on(s)) return fail(GMPNP_ERR_INVALID, "galvanostat: the option is off (gmpnp_set_galvanostat)");
  HIP_TRY(hipSetDevice(s->opts.device_id));
  gmpnp_galvanostat* G = s->galvanostat.get();
  int32_t* st = G->status.p;
  HIP_TRY(hipMemsetAsync(st, 0, sizeof(int32_t), s->stream));
  if (x) { int rc = upload_vec(s, x, G->x.p); if (rc) return rc; }
  else HIP_TRY(hipMemsetAsync(G->x.p, 0, (size_t)s->ndof * sizeof(double), s->stream));
  int rc = galvanostat_launch_rhs(s, st); if (rc) return rc;
  rc = galvanostat_launch_reduce(s, true, G->x.p, G->zero.p, 4, 1, st); if (rc) return rc;
  int32_t flags = 0;
  HIP_TRY(hipMemcpyAsync(s->h_status, st, sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  flags = *s->h_status;
  const GalvReport rep = G->h_report[1];
  scalars[0] = rep.G; scalars[1] = rep.d; scalars[2] = rep.I; scalars[3] = rep.cy;
  if (b_out) { rc = download_vec(s, G->b.p, b_out); if (rc) return rc; }
  if (flags & (32 | 64 | 128)) return fail(GMPNP_ERR_NUMERIC, status_message(flags));
  return GMPNP_OK;
}

}  // extern "C"
