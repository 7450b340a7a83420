// Potential programmes on the device: gmpnp_set_electrode_potential and the electrode trace (include/gmpnp.h "potential programmes"),
// rule in gmpnp_host_rules.h (electrode_record_combine).  Also the one home of what the trace and the wall profile (gmpnp_wall_profile.h)
// share: the boundary sum of a record on the device, the refusals and the weights of the Stern nodes on the host.
//
//   boundary_record_sums    over entries of the Stern boundary's node list (the list of SternTab, which is the kinetics' list too), ascending:
//                               v[0]        D: the sum of k_stern_sum, bnd_dyn - bndF on the potential rows
//                               v[1 + r]    I[r]: the sum of k_kinetics_sum, w_I rate_r straight from u (kinetics on)
//                               v[U0 + f]   sum_I w_I u_{I,f}
//                               v[W0]       sum_I w_I
//                           each lane adds its entries e0 + lane, e0 + lane + 256, ... in the statements of those two kernels; block_sum
//                           then adds the lanes component by component, so D and I carry the bits gmpnp_stern_displacement and
//                           gmpnp_kinetics_currents return, whichever kernel asks.  `pos` names the entries' positions in the node list
//                           (nullptr: entry e is position e).
//   boundary_record_means   the means of the potential and of the species over the summed weight, 0 beyond the species, and whether all
//                           of them are finite.
//   k_electrode_record      one workgroup, fixed order, behind k_stern_residual (and k_kinetics_residual) at the current u, over the whole
//                           list.  Lane 0 applies electrode_record_combine to the accumulators the device keeps (D_prev, Q, Q_D) and
//                           writes the record's slot: no host synchronisation, no copy, no floating-point atomics.
// The sums are picked out of the register array with constant indices (unrolled loops): a dynamic index would put v[] into scratch.
// The weights are the kinetics' own array while that option is on, otherwise the trace's copy (boundary_weights, gmpnp_kinetics.h).
// Included at the end of gmpnp_api.hip.
#pragma once

namespace gmpnp {

template <int NF>
struct BoundarySums {
  static constexpr int NS = NF - 1, R = GMPNP_MAX_SURFACE_REACTIONS, U0 = 1 + R, W0 = U0 + NF, K = W0 + 1;
};

template <int NF>
__device__ __forceinline__ void boundary_record_sums(const Ctx& c, const SternTab& st, const KinTab& kt, const double* w, int kinetics, int e0, int e1,
                                                     const int32_t* pos, double (&v)[BoundarySums<NF>::K]) {
  using B = BoundarySums<NF>;
  constexpr int NS = B::NS, R = B::R;
#pragma unroll
  for (int k = 0; k < B::K; ++k) v[k] = 0.0;
  for (int e = e0 + (int)threadIdx.x; e < e1; e += kVecBlock) {
    const int n = pos ? pos[e] : e;
    const size_t row0 = (size_t)st.node[n] * NF;
    v[0] += st.bnd_dyn[row0 + NS] - st.bndF[row0 + NS];
    double uu[NF];
#pragma unroll
    for (int j = 0; j < NF; ++j) uu[j] = c.u[row0 + j];
    const double wn = w[n];
    if (kinetics) {
      KinRate Rr[R];
      kinetics_rates<NF>(kt, uu, Rr);
#pragma unroll
      for (int r = 0; r < R; ++r) v[1 + r] += wn * Rr[r].rate;
    }
#pragma unroll
    for (int j = 0; j < NF; ++j) v[B::U0 + j] += wn * uu[j];
    v[B::W0] += wn;
  }
}

// lane 0, behind block_sum: the means and whether every one of them is finite
struct BoundaryMeans { double p, u[GMPNP_MAX_SPECIES]; bool ok; };
template <int NF>
__device__ __forceinline__ BoundaryMeans boundary_record_means(const double (&v)[BoundarySums<NF>::K]) {
  using B = BoundarySums<NF>;
  constexpr int NS = B::NS;
  const double ws = v[B::W0];
  BoundaryMeans m;
  m.p = v[B::U0 + NS] / ws;
  m.ok = rule_finite(m.p);
#pragma unroll
  for (int j = 0; j < GMPNP_MAX_SPECIES; ++j) {
    m.u[j] = j < NS ? v[B::U0 + (j < NS ? j : 0)] / ws : 0.0;
    m.ok = m.ok && rule_finite(m.u[j]);
  }
  return m;
}

struct TraceTab {
  const double* w;                  // [n_nodes] w_I of the Stern nodes
  gmpnp_electrode_record_t* rec;    // the slot to write
  ElectrodeAccum* acc;              // D_prev, Q, Q_D
  double t, h, p_M;
  int32_t kinetics, pad_;           // 1: the kinetic option is on (KinTab is valid)
};

template <int DIM, int NF>
__global__ __launch_bounds__(kVecBlock) void k_electrode_record(const Ctx c, const SternTab st, const KinTab kt, const TraceTab tr) {
  constexpr int R = GMPNP_MAX_SURFACE_REACTIONS, K = BoundarySums<NF>::K;
  __shared__ double lds[4 * K];
  double v[K];
  boundary_record_sums<NF>(c, st, kt, tr.w, tr.kinetics, 0, st.n_nodes, nullptr, v);
  block_sum<K>(v, lds);
  if (threadIdx.x != 0) return;
  ElectrodeAccum a = *tr.acc;
  const double I[R] = {v[1], v[2], v[3], v[4]};
  const double dD_dt = electrode_record_combine(a, tr.h, v[0], I);
  *tr.acc = a;
  gmpnp_electrode_record_t* o = tr.rec;
  bool ok = rule_finite(tr.t) && rule_finite(tr.h) && rule_finite(tr.p_M) && rule_finite(v[0]) && rule_finite(dD_dt) && rule_finite(a.Q_D);
  o->t = tr.t; o->h = tr.h; o->p_M = tr.p_M;
  o->D = v[0]; o->dD_dt = dD_dt;
#pragma unroll
  for (int r = 0; r < R; ++r) { o->I[r] = I[r]; o->Q[r] = a.Q[r]; ok = ok && rule_finite(I[r]) && rule_finite(a.Q[r]); }
  o->Q_D = a.Q_D;
  const BoundaryMeans m = boundary_record_means<NF>(v);
  o->p_boundary = m.p; ok = ok && m.ok;
#pragma unroll
  for (int j = 0; j < GMPNP_MAX_SPECIES; ++j) o->u_boundary[j] = m.u[j];
  o->status = ok ? 0 : 1; o->pad_ = 0;
}

}  // namespace gmpnp

namespace {

// refuses a handle that keeps no records of its Stern boundary (the trace, the wall profile)
int boundary_record_refuse(const gmpnp_solver* s, const RecordNouns& w) {
  const char* why = !stern_on(s) ? "the Stern boundary condition is off (gmpnp_set_stern)"
                    : s->partitioned ? "partition handles and groups are not supported"
                    : (s->ml_coarse || s->ml_is_coarse) ? "not with a multilevel coarse level attached"
                    : galvanostat_on(s) ? "the galvanostat is on (gmpnp_set_galvanostat): the potential is its unknown" : nullptr;
  return why ? fail(GMPNP_ERR_INVALID, w.say(why)) : GMPNP_OK;
}

// w_I of the Stern nodes in ascending internal order (the kinetics' weights, for a handle whose kinetics are off) and, with `z`, their
// third coordinates
void stern_node_weights(const gmpnp_solver* s, std::vector<double>& w, std::vector<double>* z) {
  std::vector<double> wv;
  std::vector<uint8_t> on;
  boundary_weights(s, wv, on);
  for (int I = 0; I < s->t.nv; ++I)
    if (on[I]) { w.push_back(wv[I]); if (z) z->push_back(s->t.coords[(size_t)I * 3 + 2]); }
}

// the launches of one append into the row `rec` with the accumulators acc[which]
int trace_launch(gmpnp_solver* s, double t, double h, gmpnp_electrode_record_t* rec, int which) {
  gmpnp_tracer* T = s->tracer.get();
  int rc = stern_launch_residual(s, T->status.p); if (rc) return rc;   // (the trace's own word: the solver's stays what it was)
  const bool kin = kinetics_on(s);
  if (kin) { rc = kinetics_launch_residual(s, T->status.p); if (rc) return rc; }
  const SternTab st = stern_tab(s, T->status.p);
  const KinTab kt = kin ? kinetics_tab(s, T->status.p) : KinTab{};
  TraceTab tr{};
  tr.w = kin ? s->kineticist->w.p : T->w.p;
  tr.rec = rec; tr.acc = T->acc.p + which;
  tr.t = t; tr.h = h; tr.p_M = s->sterner->opt.p_electrode; tr.kinetics = kin ? 1 : 0;
  GMPNP_DISPATCH(s, hipLaunchKernelGGL((k_electrode_record<DIM, NF>), dim3(1), dim3(kVecBlock), 0, s->stream, s->c, st, kt, tr));
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

bool trace_is_open(const gmpnp_solver* s) { return s->tracer && s->tracer->rec.open; }

// gmpnp_time_kernel 29: the row behind the buffer and the second set of accumulators, so the trace stays what it was
int trace_time_append(gmpnp_solver* s) {
  if (int rc = boundary_record_refuse(s, kTraceNouns)) return rc;
  return trace_launch(s, 0.0, 1.0, s->tracer->rec.hook_row(), 1);
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
  if (int rc = boundary_record_refuse(s, kTraceNouns)) return rc;
  if (capacity < 1) return fail(GMPNP_ERR_INVALID, "electrode trace: capacity must be at least 1");
  HIP_TRY(hipSetDevice(s->opts.device_id));
  if (!s->tracer) {
    std::unique_ptr<gmpnp_tracer> T(new gmpnp_tracer);
    std::vector<double> w;
    stern_node_weights(s, w, nullptr);
    if ((int)w.size() != s->sterner->n_nodes) return fail(GMPNP_ERR_INVALID, "electrode trace: the Stern boundary's node list does not match its weights");
    HIP_TRY(T->w.upload(w));
    HIP_TRY(T->acc.alloc(2)); HIP_TRY(T->status.alloc(1));
    s->tracer = std::move(T);
  }
  gmpnp_tracer* T = s->tracer.get();
  T->rec.close();
  int rc = T->rec.reserve(capacity, 1, s->stream); if (rc) return rc;
  // D_prev = D at the current u; Q = Q_D = 0
  rc = stern_launch_residual(s, T->status.p); if (rc) return rc;
  rc = stern_launch_sum(s, nullptr); if (rc) return rc;
  HIP_TRY(hipMemsetAsync(T->acc.p, 0, 2 * sizeof(ElectrodeAccum), s->stream));
  HIP_TRY(hipMemcpyAsync(&T->acc.p[0].D_prev, s->sterner->sum.p, sizeof(double), hipMemcpyDeviceToDevice, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  T->rec.open = true;
  return GMPNP_OK;
}

int gmpnp_electrode_trace_append(gmpnp_solver* s, double t, double h) {
  if (!s) return fail(GMPNP_ERR_INVALID, "electrode trace: NULL argument");
  if (int rc = boundary_record_refuse(s, kTraceNouns)) return rc;
  if (!trace_is_open(s)) return fail(GMPNP_ERR_INVALID, kTraceNouns.not_open());
  if (!record_step_valid(t, h)) return fail(GMPNP_ERR_INVALID, "electrode trace: t finite, h finite and > 0");
  gmpnp_tracer* T = s->tracer.get();
  if (T->rec.full()) return T->rec.refuse_full();
  HIP_TRY(hipSetDevice(s->opts.device_id));
  int rc = trace_launch(s, t, h, T->rec.row(T->rec.count), 0); if (rc) return rc;
  T->rec.count += 1;
  return GMPNP_OK;
}

int gmpnp_electrode_trace_read(gmpnp_solver* s, int32_t first, int32_t n, gmpnp_electrode_record_t* out) {
  if (!s || !out) return fail(GMPNP_ERR_INVALID, "electrode trace: NULL argument");
  if (!trace_is_open(s)) return fail(GMPNP_ERR_INVALID, kTraceNouns.not_open());
  HIP_TRY(hipSetDevice(s->opts.device_id));
  return s->tracer->rec.read(first, n, out, s->stream);
}

int gmpnp_electrode_trace_close(gmpnp_solver* s) {
  if (!s) return fail(GMPNP_ERR_INVALID, "electrode trace: NULL argument");
  if (!trace_is_open(s)) return fail(GMPNP_ERR_INVALID, kTraceNouns.not_open());
  s->tracer->rec.close();
  return GMPNP_OK;
}

}  // extern "C"
