// Potential programmes on the device: gmpnp_set_electrode_potential and the electrode trace (include/gmpnp.h "potential programmes"),
// rule in gmpnp_host_rules.h (electrode_record_combine).
//
//   k_electrode_record   one workgroup, fixed order, behind k_stern_residual (and k_kinetics_residual) at the current u.  Over the
//                        nodes of the Stern boundary, ascending (the list of SternTab, which is the kinetics' list too):
//                            D        the sum of k_stern_sum: bnd_dyn - bndF on the potential rows
//                            I[r]     the sum of k_kinetics_sum: w_I rate_r straight from u (kinetics on)
//                            means    sum_I w_I u_{I,f} and sum_I w_I
//                        each lane adds its nodes n = lane, lane + 256, ... in the statements of those two kernels and block_sum adds
//                        the lanes component by component, so D and I carry the bits gmpnp_stern_displacement and
//                        gmpnp_kinetics_currents return.  Lane 0 applies electrode_record_combine to the accumulators the device
//                        keeps (D_prev, Q, Q_D) and writes the record's slot: no host synchronisation, no copy, no floating-point
//                        atomics.  The sums are picked out of the register array with constant indices (unrolled loops).
// The weights are the kinetics' own array while that option is on, otherwise the trace's copy (boundary_weights, gmpnp_kinetics.h).
// Included at the end of gmpnp_api.hip.
#pragma once

namespace gmpnp {

struct TraceTab {
  const double* w;                  // [n_nodes] w_I of the Stern nodes
  gmpnp_electrode_record_t* rec;    // the slot to write
  ElectrodeAccum* acc;              // D_prev, Q, Q_D
  double t, h, p_M;
  int32_t kinetics, pad_;           // 1: the kinetic option is on (KinTab is valid)
};

template <int DIM, int NF>
__global__ __launch_bounds__(kVecBlock) void k_electrode_record(const Ctx c, const SternTab st, const KinTab kt, const TraceTab tr) {
  constexpr int NS = NF - 1, R = GMPNP_MAX_SURFACE_REACTIONS, U0 = 1 + R, W0 = U0 + NF, K = W0 + 1;
  __shared__ double lds[4 * K];
  double v[K];
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = 0.0;
  for (int n = threadIdx.x; n < st.n_nodes; n += kVecBlock) {
    const size_t row0 = (size_t)st.node[n] * NF;
    v[0] += st.bnd_dyn[row0 + NS] - st.bndF[row0 + NS];
    double uu[NF];
#pragma unroll
    for (int j = 0; j < NF; ++j) uu[j] = c.u[row0 + j];
    const double w = tr.w[n];
    if (tr.kinetics) {
      KinRate Rr[R];
      kinetics_rates<NF>(kt, uu, Rr);
#pragma unroll
      for (int r = 0; r < R; ++r) v[1 + r] += w * Rr[r].rate;
    }
#pragma unroll
    for (int j = 0; j < NF; ++j) v[U0 + j] += w * uu[j];
    v[W0] += w;
  }
  block_sum<K>(v, lds);
  if (threadIdx.x != 0) return;
  ElectrodeAccum a = *tr.acc;
  const double I[R] = {v[1], v[2], v[3], v[4]};
  const double dD_dt = electrode_record_combine(a, tr.h, v[0], I);
  *tr.acc = a;
  gmpnp_electrode_record_t* o = tr.rec;
  const double ws = v[W0];
  bool ok = rule_finite(tr.t) && rule_finite(tr.h) && rule_finite(tr.p_M) && rule_finite(v[0]) && rule_finite(dD_dt) && rule_finite(a.Q_D);
  o->t = tr.t; o->h = tr.h; o->p_M = tr.p_M;
  const double pb = v[U0 + NS] / ws;
  o->p_boundary = pb; ok = ok && rule_finite(pb);
  o->D = v[0]; o->dD_dt = dD_dt;
#pragma unroll
  for (int r = 0; r < R; ++r) { o->I[r] = I[r]; o->Q[r] = a.Q[r]; ok = ok && rule_finite(I[r]) && rule_finite(a.Q[r]); }
  o->Q_D = a.Q_D;
#pragma unroll
  for (int j = 0; j < GMPNP_MAX_SPECIES; ++j) {
    const double m = j < NS ? v[U0 + (j < NS ? j : 0)] / ws : 0.0;
    o->u_boundary[j] = m; ok = ok && rule_finite(m);
  }
  o->status = ok ? 0 : 1; o->pad_ = 0;
}

}  // namespace gmpnp

namespace {

const char* trace_refusal(const gmpnp_solver* s) {
  if (!stern_on(s)) return "electrode trace: the Stern boundary condition is off (gmpnp_set_stern)";
  if (s->partitioned) return "electrode trace: partition handles and groups are not supported";
  if (s->ml_coarse || s->ml_is_coarse) return "electrode trace: not with a multilevel coarse level attached";
  if (galvanostat_on(s)) return "electrode trace: the galvanostat is on (gmpnp_set_galvanostat): the potential is its unknown";
  return nullptr;
}

// w_I of the Stern nodes in ascending internal order: the kinetics' weights, for a handle whose kinetics are off
int trace_build_weights(gmpnp_solver* s, gmpnp_tracer* T) {
  std::vector<double> wv, w;
  std::vector<uint8_t> on;
  boundary_weights(s, wv, on);
  for (int I = 0; I < s->t.nv; ++I) if (on[I]) w.push_back(wv[I]);
  if ((int)w.size() != s->sterner->n_nodes) return fail(GMPNP_ERR_INVALID, "electrode trace: the Stern boundary's node list does not match its weights");
  HIP_TRY(T->w.upload(w));
  return GMPNP_OK;
}

// the launches of one append into slot `slot` with the accumulators acc[which]
int trace_launch(gmpnp_solver* s, double t, double h, int slot, int which) {
  gmpnp_tracer* T = s->tracer.get();
  int rc = stern_launch_residual(s, T->status.p); if (rc) return rc;   // (the trace's own word: the solver's stays what it was)
  const bool kin = kinetics_on(s);
  if (kin) { rc = kinetics_launch_residual(s, T->status.p); if (rc) return rc; }
  const SternTab st = stern_tab(s, T->status.p);
  const KinTab kt = kin ? kinetics_tab(s, T->status.p) : KinTab{};
  TraceTab tr{};
  tr.w = kin ? s->kineticist->w.p : T->w.p;
  tr.rec = T->rec.p + slot; tr.acc = T->acc.p + which;
  tr.t = t; tr.h = h; tr.p_M = s->sterner->opt.p_electrode; tr.kinetics = kin ? 1 : 0;
  GMPNP_DISPATCH(s, hipLaunchKernelGGL((k_electrode_record<DIM, NF>), dim3(1), dim3(kVecBlock), 0, s->stream, s->c, st, kt, tr));
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

bool trace_is_open(const gmpnp_solver* s) { return s->tracer && s->tracer->open; }

// gmpnp_time_kernel 29: the slot behind the buffer and the second set of accumulators, so the trace stays what it was
int trace_time_append(gmpnp_solver* s) {
  const char* why = trace_refusal(s);
  if (why) return fail(GMPNP_ERR_INVALID, why);
  return trace_launch(s, 0.0, 1.0, s->tracer->capacity, 1);
}

}  // namespace

extern "C" {

int gmpnp_set_electrode_potential(gmpnp_solver* s, double p) {
  if (!s) return fail(GMPNP_ERR_INVALID, "electrode potential: NULL argument");
  if (!rule_finite(p)) return fail(GMPNP_ERR_INVALID, "electrode potential: the value must be finite");
  if (!stern_on(s)) return fail(GMPNP_ERR_INVALID, "electrode potential: the Stern boundary condition is off (gmpnp_set_stern)");
  if (galvanostat_on(s)) return fail(GMPNP_ERR_INVALID, "electrode potential: the galvanostat is on (gmpnp_set_galvanostat) and owns it");
  HIP_TRY(hipSetDevice(s->opts.device_id));
  HIP_TRY(hipStreamSynchronize(s->stream));
  tangent_drop(s);
  s->sterner->opt.p_electrode = p;
  if (kinetics_on(s)) {
    s->kineticist->opt.p_electrode = p;
    HIP_TRY(hipMemcpy(s->kineticist->d_opt.p, &s->kineticist->opt, sizeof(gmpnp_kinetics_t), hipMemcpyHostToDevice));
  }
  s->jacobian_valid = false; s->precond_valid = false;
  return boundary_rebind(s);
}

int gmpnp_electrode_trace_open(gmpnp_solver* s, int32_t capacity) {
  if (!s) return fail(GMPNP_ERR_INVALID, "electrode trace: NULL argument");
  const char* why = trace_refusal(s);
  if (why) return fail(GMPNP_ERR_INVALID, why);
  if (capacity < 1) return fail(GMPNP_ERR_INVALID, "electrode trace: capacity must be at least 1");
  HIP_TRY(hipSetDevice(s->opts.device_id));
  if (!s->tracer) {
    std::unique_ptr<gmpnp_tracer> T(new gmpnp_tracer);
    int rc = trace_build_weights(s, T.get()); if (rc) return rc;
    HIP_TRY(T->acc.alloc(2)); HIP_TRY(T->status.alloc(1));
    s->tracer = std::move(T);
  }
  gmpnp_tracer* T = s->tracer.get();
  T->open = false;
  if (T->capacity != capacity) {
    HIP_TRY(hipStreamSynchronize(s->stream));
    T->capacity = 0;   // (alloc frees the old buffer first: an allocation that fails leaves no capacity a later open could take for a buffer)
    HIP_TRY(T->rec.alloc((size_t)capacity + 1));
    T->capacity = capacity;
  }
  T->count = 0;
  // D_prev = D at the current u; Q = Q_D = 0
  int rc = stern_launch_residual(s, T->status.p); if (rc) return rc;
  rc = stern_launch_sum(s, nullptr); if (rc) return rc;
  HIP_TRY(hipMemsetAsync(T->acc.p, 0, 2 * sizeof(ElectrodeAccum), s->stream));
  HIP_TRY(hipMemcpyAsync(&T->acc.p[0].D_prev, s->sterner->sum.p, sizeof(double), hipMemcpyDeviceToDevice, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  T->open = true;
  return GMPNP_OK;
}

int gmpnp_electrode_trace_append(gmpnp_solver* s, double t, double h) {
  if (!s) return fail(GMPNP_ERR_INVALID, "electrode trace: NULL argument");
  const char* why = trace_refusal(s);
  if (why) return fail(GMPNP_ERR_INVALID, why);
  if (!trace_is_open(s)) return fail(GMPNP_ERR_INVALID, "electrode trace: no trace is open (gmpnp_electrode_trace_open)");
  if (!electrode_trace_step_valid(t, h)) return fail(GMPNP_ERR_INVALID, "electrode trace: t finite, h finite and > 0");
  gmpnp_tracer* T = s->tracer.get();
  if (T->count >= T->capacity) return fail(GMPNP_ERR_INVALID, "electrode trace: the buffer is full (read the records and open the trace again)");
  HIP_TRY(hipSetDevice(s->opts.device_id));
  int rc = trace_launch(s, t, h, T->count, 0); if (rc) return rc;
  T->count += 1;
  return GMPNP_OK;
}

int gmpnp_electrode_trace_read(gmpnp_solver* s, int32_t first, int32_t n, gmpnp_electrode_record_t* out) {
  if (!s || !out) return fail(GMPNP_ERR_INVALID, "electrode trace: NULL argument");
  if (!trace_is_open(s)) return fail(GMPNP_ERR_INVALID, "electrode trace: no trace is open (gmpnp_electrode_trace_open)");
  gmpnp_tracer* T = s->tracer.get();
  if (first < 0 || n < 1 || (int64_t)first + n > T->count) return fail(GMPNP_ERR_INVALID, "electrode trace: the records asked for have not been written");
  HIP_TRY(hipSetDevice(s->opts.device_id));
  HIP_TRY(hipMemcpyAsync(out, T->rec.p + first, (size_t)n * sizeof(gmpnp_electrode_record_t), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return GMPNP_OK;
}

int gmpnp_electrode_trace_close(gmpnp_solver* s) {
  if (!s) return fail(GMPNP_ERR_INVALID, "electrode trace: NULL argument");
  if (!trace_is_open(s)) return fail(GMPNP_ERR_INVALID, "electrode trace: no trace is open (gmpnp_electrode_trace_open)");
  s->tracer->open = false;
  return GMPNP_OK;
}

}  // extern "C"
