// The wall profile on the device: the electrode record resolved along the axis of the 3D pore (include/gmpnp.h "wall profile"), rule in
// gmpnp_host_rules.h (wall_bin, wall_bins_valid, wall_profile_charge).
//
//   k_wall_profile   one workgroup per axial bin, fixed order, behind k_stern_residual (and k_kinetics_residual) at the current u.  The
//                    bin's entries are positions in the Stern node list (SternTab::node, ascending), ascending; lane l takes entries
//                    l, l + kVecBlock, ... and adds, in the statements of k_electrode_record,
//                        D        bnd_dyn - bndF on the potential row
//                        I[r]     w_I rate_r straight from u (kinetics on)
//                        means    w_I u_{I,f} and w_I
//                    block_sum adds the lanes component by component, so with one bin over the whole wall D and I carry the bits of
//                    gmpnp_electrode_record_t.  Lane 0 applies wall_profile_charge to the bin's charges, divides the means by the bin's
//                    area, checks every value for finiteness and writes the bin's slot with ordinary stores: no host synchronisation, no
//                    copy, no floating-point atomics, no barrier across workgroups.  A bin's workgroup touches that bin's slot and
//                    charges only.  The sums are picked out of the register array with constant indices (unrolled loops).
// The weights are the profile's own copy of boundary_weights (gmpnp_kinetics.h): the bits the kinetics hold.
// Included at the end of gmpnp_api.hip.
#pragma once

namespace gmpnp {

struct WallProfileTab {
  const double* w;                      // [n_nodes] w_I of the Stern nodes
  const int32_t* bin_ptr;               // [n_bins + 1]
  const int32_t* bin_pos;               // positions in the Stern node list
  const double* edges;                  // [n_bins + 1]
  gmpnp_wall_profile_record_t* rec;     // the step's row of n_bins slots
  double* Q;                            // [n_bins][4] the charges of the bins
  double t, h;
  int32_t kinetics, pad_;               // 1: the kinetic option is on (KinTab is valid)
};

template <int NF>
__global__ __launch_bounds__(kVecBlock) void k_wall_profile(const Ctx c, const SternTab st, const KinTab kt, const WallProfileTab pt) {
  constexpr int NS = NF - 1, R = GMPNP_MAX_SURFACE_REACTIONS, U0 = 1 + R, W0 = U0 + NF, K = W0 + 1;
  __shared__ double lds[4 * K];
  const int b = blockIdx.x;
  const int e0 = pt.bin_ptr[b], e1 = pt.bin_ptr[b + 1];
  double v[K];
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = 0.0;
  for (int e = e0 + (int)threadIdx.x; e < e1; e += kVecBlock) {
    const int n = pt.bin_pos[e];
    const size_t row0 = (size_t)st.node[n] * NF;
    v[0] += st.bnd_dyn[row0 + NS] - st.bndF[row0 + NS];
    double uu[NF];
#pragma unroll
    for (int j = 0; j < NF; ++j) uu[j] = c.u[row0 + j];
    const double w = pt.w[n];
    if (pt.kinetics) {
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
  double* Qb = pt.Q + (size_t)b * R;
  double Q[R] = {Qb[0], Qb[1], Qb[2], Qb[3]};
  const double I[R] = {v[1], v[2], v[3], v[4]};
  wall_profile_charge(Q, pt.h, I);
  gmpnp_wall_profile_record_t* o = pt.rec + b;
  const double ws = v[W0];
  bool ok = rule_finite(pt.t) && rule_finite(pt.h) && rule_finite(v[0]) && rule_finite(ws);
  o->t = pt.t; o->h = pt.h; o->z_lo = pt.edges[b]; o->z_hi = pt.edges[b + 1];
  o->area = ws; o->D = v[0];
#pragma unroll
  for (int r = 0; r < R; ++r) { Qb[r] = Q[r]; o->I[r] = I[r]; o->Q[r] = Q[r]; ok = ok && rule_finite(I[r]) && rule_finite(Q[r]); }
  const double pm = v[U0 + NS] / ws;
  o->p_mean = pm; ok = ok && rule_finite(pm);
#pragma unroll
  for (int j = 0; j < GMPNP_MAX_SPECIES; ++j) {
    const double m = j < NS ? v[U0 + (j < NS ? j : 0)] / ws : 0.0;
    o->u_mean[j] = m; ok = ok && rule_finite(m);
  }
  o->count = e1 - e0; o->status = ok ? 0 : 1;
}

}  // namespace gmpnp

namespace {

const char* wall_profile_refusal(const gmpnp_solver* s) {
  if (s->dim != 3) return "wall profile: 3D handles only (the electrode record is the profile of a 1D handle)";
  if (!stern_on(s)) return "wall profile: the Stern boundary condition is off (gmpnp_set_stern)";
  if (s->partitioned) return "wall profile: partition handles and groups are not supported";
  if (s->ml_coarse || s->ml_is_coarse) return "wall profile: not with a multilevel coarse level attached";
  if (galvanostat_on(s)) return "wall profile: the galvanostat is on (gmpnp_set_galvanostat): the potential is its unknown";
  return nullptr;
}

// the Stern nodes (ascending internal order, the list of SternTab) sorted into the bins by their z: CSR of positions in that list
int wall_profile_build_bins(gmpnp_solver* s, gmpnp_wall_profiler* P, int n_bins, const double* edges, bool first) {
  std::vector<double> wv, w, z;
  std::vector<uint8_t> on;
  boundary_weights(s, wv, on);
  for (int I = 0; I < s->t.nv; ++I) if (on[I]) { w.push_back(wv[I]); z.push_back(s->t.coords[(size_t)I * 3 + 2]); }
  const int nn = (int)w.size();
  if (nn != s->sterner->n_nodes) return fail(GMPNP_ERR_INVALID, "wall profile: the Stern boundary's node list does not match its weights");
  std::vector<int32_t> bin((size_t)nn), ptr((size_t)n_bins + 1, 0), pos;
  for (int n = 0; n < nn; ++n) { bin[n] = wall_bin(z[n], edges, n_bins); if (bin[n] >= 0) ptr[bin[n] + 1]++; }
  for (int b = 0; b < n_bins; ++b) {
    if (ptr[b + 1] == 0)
      return fail(GMPNP_ERR_INVALID, "wall profile: bin " + std::to_string(b) + " of " + std::to_string(n_bins) + " holds no node of the wall: ask for fewer bins");
    ptr[b + 1] += ptr[b];
  }
  pos.resize((size_t)ptr[n_bins]);
  { std::vector<int32_t> fill(ptr.begin(), ptr.end() - 1);
    for (int n = 0; n < nn; ++n) if (bin[n] >= 0) pos[fill[bin[n]]++] = n; }   // n ascending: ascending inside a bin
  HIP_TRY(hipStreamSynchronize(s->stream));   // (no launch of an earlier profile reads the lists any more)
  if (first) HIP_TRY(P->w.upload(w));
  HIP_TRY(P->bin_ptr.upload(ptr)); HIP_TRY(P->bin_pos.upload(pos));
  HIP_TRY(P->edges.upload(std::vector<double>(edges, edges + n_bins + 1)));
  P->h_edges.assign(edges, edges + n_bins + 1);
  return GMPNP_OK;
}

// the launches of one append into row `slot` with the charges Q[which]
int wall_profile_launch(gmpnp_solver* s, double t, double h, int slot, int which) {
  gmpnp_wall_profiler* P = s->wall_profiler.get();
  int rc = stern_launch_residual(s, P->status.p); if (rc) return rc;   // (the profile's own word: the solver's stays what it was)
  const bool kin = kinetics_on(s);
  if (kin) { rc = kinetics_launch_residual(s, P->status.p); if (rc) return rc; }
  const SternTab st = stern_tab(s, P->status.p);
  const KinTab kt = kin ? kinetics_tab(s, P->status.p) : KinTab{};
  WallProfileTab pt{};
  pt.w = P->w.p; pt.bin_ptr = P->bin_ptr.p; pt.bin_pos = P->bin_pos.p; pt.edges = P->edges.p;
  pt.rec = P->rec.p + (size_t)slot * P->n_bins;
  pt.Q = P->Q.p + (size_t)which * P->n_bins * GMPNP_MAX_SURFACE_REACTIONS;
  pt.t = t; pt.h = h; pt.kinetics = kin ? 1 : 0;
  hipLaunchKernelGGL((k_wall_profile<9>), dim3(P->n_bins), dim3(kVecBlock), 0, s->stream, s->c, st, kt, pt);
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

bool wall_profile_is_open(const gmpnp_solver* s) { return s->wall_profiler && s->wall_profiler->open; }

// gmpnp_time_kernel 32: the row behind the buffer and the second set of charges, so the profile stays what it was
int wall_profile_time_append(gmpnp_solver* s) {
  const char* why = wall_profile_refusal(s);
  if (why) return fail(GMPNP_ERR_INVALID, why);
  return wall_profile_launch(s, 0.0, 1.0, s->wall_profiler->capacity, 1);
}

}  // namespace

extern "C" {

int gmpnp_wall_profile_open(gmpnp_solver* s, int32_t n_bins, const double* edges, int32_t capacity) {
  if (!s) return fail(GMPNP_ERR_INVALID, "wall profile: NULL argument");
  const char* why = wall_profile_refusal(s);
  if (why) return fail(GMPNP_ERR_INVALID, why);
  if (s->nf != 9) return fail(GMPNP_ERR_INVALID, "wall profile: 3D pore problems (9 fields)");
  if (!wall_bins_valid(edges, n_bins)) return fail(GMPNP_ERR_INVALID, "wall profile: 1 ... 256 bins with n_bins + 1 finite, strictly ascending edges");
  if (capacity < 1) return fail(GMPNP_ERR_INVALID, "wall profile: capacity must be at least 1");
  HIP_TRY(hipSetDevice(s->opts.device_id));
  const bool first = !s->wall_profiler;
  std::unique_ptr<gmpnp_wall_profiler> fresh;
  if (first) { fresh.reset(new gmpnp_wall_profiler); HIP_TRY(fresh->status.alloc(1)); }
  gmpnp_wall_profiler* P = first ? fresh.get() : s->wall_profiler.get();
  P->open = false;
  const bool same_bins = !first && P->n_bins == n_bins && std::equal(P->h_edges.begin(), P->h_edges.end(), edges);
  if (!same_bins) {
    P->n_bins = 0; P->capacity = 0;   // (a refusal or a failed upload below leaves nothing a later open could take for valid lists)
    int rc = wall_profile_build_bins(s, P, n_bins, edges, first); if (rc) return rc;
    HIP_TRY(P->Q.alloc((size_t)2 * n_bins * GMPNP_MAX_SURFACE_REACTIONS));
    P->n_bins = n_bins;
  }
  if (first) s->wall_profiler = std::move(fresh);
  if (P->capacity != capacity) {
    HIP_TRY(hipStreamSynchronize(s->stream));
    P->capacity = 0;
    HIP_TRY(P->rec.alloc(((size_t)capacity + 1) * n_bins));
    P->capacity = capacity;
  }
  P->count = 0;
  HIP_TRY(hipMemsetAsync(P->Q.p, 0, (size_t)2 * n_bins * GMPNP_MAX_SURFACE_REACTIONS * sizeof(double), s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  P->open = true;
  return GMPNP_OK;
}

int gmpnp_wall_profile_append(gmpnp_solver* s, double t, double h) {
  if (!s) return fail(GMPNP_ERR_INVALID, "wall profile: NULL argument");
  const char* why = wall_profile_refusal(s);
  if (why) return fail(GMPNP_ERR_INVALID, why);
  if (!wall_profile_is_open(s)) return fail(GMPNP_ERR_INVALID, "wall profile: no profile is open (gmpnp_wall_profile_open)");
  if (!wall_profile_step_valid(t, h)) return fail(GMPNP_ERR_INVALID, "wall profile: t finite, h finite and > 0");
  gmpnp_wall_profiler* P = s->wall_profiler.get();
  if (P->count >= P->capacity) return fail(GMPNP_ERR_INVALID, "wall profile: the buffer is full (read the records and open the profile again)");
  HIP_TRY(hipSetDevice(s->opts.device_id));
  int rc = wall_profile_launch(s, t, h, P->count, 0); if (rc) return rc;
  P->count += 1;
  return GMPNP_OK;
}

int gmpnp_wall_profile_read(gmpnp_solver* s, int32_t first, int32_t n, gmpnp_wall_profile_record_t* out) {
  if (!s || !out) return fail(GMPNP_ERR_INVALID, "wall profile: NULL argument");
  if (!wall_profile_is_open(s)) return fail(GMPNP_ERR_INVALID, "wall profile: no profile is open (gmpnp_wall_profile_open)");
  gmpnp_wall_profiler* P = s->wall_profiler.get();
  if (first < 0 || n < 1 || (int64_t)first + n > P->count) return fail(GMPNP_ERR_INVALID, "wall profile: the records asked for have not been written");
  HIP_TRY(hipSetDevice(s->opts.device_id));
  HIP_TRY(hipMemcpyAsync(out, P->rec.p + (size_t)first * P->n_bins, (size_t)n * P->n_bins * sizeof(gmpnp_wall_profile_record_t), hipMemcpyDeviceToHost,
                         s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return GMPNP_OK;
}

int gmpnp_wall_profile_close(gmpnp_solver* s) {
  if (!s) return fail(GMPNP_ERR_INVALID, "wall profile: NULL argument");
  if (!wall_profile_is_open(s)) return fail(GMPNP_ERR_INVALID, "wall profile: no profile is open (gmpnp_wall_profile_open)");
  s->wall_profiler->open = false;
  return GMPNP_OK;
}

}  // extern "C"
