// The wall profile on the device: the electrode record resolved along the axis of the 3D pore (include/gmpnp.h "wall profile"), rule in
// gmpnp_host_rules.h (wall_bin, wall_bins_valid, wall_profile_charge).
//
//   k_wall_profile   one workgroup per axial bin, fixed order, behind k_stern_residual (and k_kinetics_residual) at the current u.  The
//                    bin's entries are positions in the Stern node list (SternTab::node, ascending), ascending; the workgroup adds them
//                    with boundary_record_sums (gmpnp_trace.h), the function k_electrode_record adds the whole list with, so with one
//                    bin over the whole wall D and I carry the bits of gmpnp_electrode_record_t.  Lane 0 applies wall_profile_charge
//                    to the bin's charges, divides the means by the bin's area (boundary_record_means), checks every value for
//                    finiteness and writes the bin's slot with ordinary stores: no host synchronisation, no copy, no floating-point
//                    atomics, no barrier across workgroups.  A bin's workgroup touches that bin's slot and charges only.
// The weights are the profile's own copy of boundary_weights (gmpnp_kinetics.h): the bits the kinetics hold.
// Included at the end of gmpnp_api.hip, behind gmpnp_trace.h.
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
  constexpr int R = GMPNP_MAX_SURFACE_REACTIONS, K = BoundarySums<NF>::K;
  __shared__ double lds[4 * K];
  const int b = blockIdx.x;
  const int e0 = pt.bin_ptr[b], e1 = pt.bin_ptr[b + 1];
  double v[K];
  __builtin_assume(pt.bin_pos != nullptr);   // (no second loop for the identity list)
  boundary_record_sums<NF>(c, st, kt, pt.w, pt.kinetics, e0, e1, pt.bin_pos, v);
  block_sum<K>(v, lds);
  if (threadIdx.x != 0) return;
  double* Qb = pt.Q + (size_t)b * R;
  double Q[R] = {Qb[0], Qb[1], Qb[2], Qb[3]};
  const double I[R] = {v[1], v[2], v[3], v[4]};
  wall_profile_charge(Q, pt.h, I);
  gmpnp_wall_profile_record_t* o = pt.rec + b;
  const double ws = v[BoundarySums<NF>::W0];
  bool ok = rule_finite(pt.t) && rule_finite(pt.h) && rule_finite(v[0]) && rule_finite(ws);
  o->t = pt.t; o->h = pt.h; o->z_lo = pt.edges[b]; o->z_hi = pt.edges[b + 1];
  o->area = ws; o->D = v[0];
#pragma unroll
  for (int r = 0; r < R; ++r) { Qb[r] = Q[r]; o->I[r] = I[r]; o->Q[r] = Q[r]; ok = ok && rule_finite(I[r]) && rule_finite(Q[r]); }
  const BoundaryMeans m = boundary_record_means<NF>(v);
  o->p_mean = m.p; ok = ok && m.ok;
#pragma unroll
  for (int j = 0; j < GMPNP_MAX_SPECIES; ++j) o->u_mean[j] = m.u[j];
  o->count = e1 - e0; o->status = ok ? 0 : 1;
}

}  // namespace gmpnp

namespace {

int wall_profile_refuse(const gmpnp_solver* s) {
  if (s->dim != 3) return fail(GMPNP_ERR_INVALID, "wall profile: 3D handles only (the electrode record is the profile of a 1D handle)");
  return boundary_record_refuse(s, kWallProfileNouns);
}

// the Stern nodes (ascending internal order, the list of SternTab) sorted into the bins by their z: CSR of positions in that list
int wall_profile_build_bins(gmpnp_solver* s, gmpnp_wall_profiler* P, int n_bins, const double* edges, bool first) {
  std::vector<double> w, z;
  stern_node_weights(s, w, &z);
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

// the launches of one append into the row `rec` with the charges Q[which]
int wall_profile_launch(gmpnp_solver* s, double t, double h, gmpnp_wall_profile_record_t* rec, int which) {
  gmpnp_wall_profiler* P = s->wall_profiler.get();
  int rc = stern_launch_residual(s, P->status.p); if (rc) return rc;   // (the profile's own word: the solver's stays what it was)
  const bool kin = kinetics_on(s);
  if (kin) { rc = kinetics_launch_residual(s, P->status.p); if (rc) return rc; }
  const SternTab st = stern_tab(s, P->status.p);
  const KinTab kt = kin ? kinetics_tab(s, P->status.p) : KinTab{};
  WallProfileTab pt{};
  pt.w = P->w.p; pt.bin_ptr = P->bin_ptr.p; pt.bin_pos = P->bin_pos.p; pt.edges = P->edges.p;
  pt.rec = rec;
  pt.Q = P->Q.p + (size_t)which * P->n_bins * GMPNP_MAX_SURFACE_REACTIONS;
  pt.t = t; pt.h = h; pt.kinetics = kin ? 1 : 0;
  hipLaunchKernelGGL((k_wall_profile<9>), dim3(P->n_bins), dim3(kVecBlock), 0, s->stream, s->c, st, kt, pt);
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

bool wall_profile_is_open(const gmpnp_solver* s) { return s->wall_profiler && s->wall_profiler->rec.open; }

// gmpnp_time_kernel 32: the row behind the buffer and the second set of charges, so the profile stays what it was
int wall_profile_time_append(gmpnp_solver* s) {
  if (int rc = wall_profile_refuse(s)) return rc;
  return wall_profile_launch(s, 0.0, 1.0, s->wall_profiler->rec.hook_row(), 1);
}

}  // namespace

extern "C" {

int gmpnp_wall_profile_open(gmpnp_solver* s, int32_t n_bins, const double* edges, int32_t capacity) {
  if (!s) return fail(GMPNP_ERR_INVALID, "wall profile: NULL argument");
  if (int rc = wall_profile_refuse(s)) return rc;
  if (s->nf != 9) return fail(GMPNP_ERR_INVALID, "wall profile: 3D pore problems (9 fields)");
  if (!wall_bins_valid(edges, n_bins)) return fail(GMPNP_ERR_INVALID, "wall profile: 1 ... 256 bins with n_bins + 1 finite, strictly ascending edges");
  if (capacity < 1) return fail(GMPNP_ERR_INVALID, "wall profile: capacity must be at least 1");
  HIP_TRY(hipSetDevice(s->opts.device_id));
  const bool first = !s->wall_profiler;
  std::unique_ptr<gmpnp_wall_profiler> fresh;
  if (first) { fresh.reset(new gmpnp_wall_profiler); HIP_TRY(fresh->status.alloc(1)); }
  gmpnp_wall_profiler* P = first ? fresh.get() : s->wall_profiler.get();
  P->rec.close();
  const bool same_bins = !first && P->n_bins == n_bins && std::equal(P->h_edges.begin(), P->h_edges.end(), edges);
  if (!same_bins) {
    P->n_bins = 0;   // (a refusal or a failed upload below leaves nothing a later open could take for valid lists)
    int rc = wall_profile_build_bins(s, P, n_bins, edges, first); if (rc) return rc;
    HIP_TRY(P->Q.alloc((size_t)2 * n_bins * GMPNP_MAX_SURFACE_REACTIONS));
    P->n_bins = n_bins;
  }
  if (first) s->wall_profiler = std::move(fresh);
  int rc = P->rec.reserve(capacity, n_bins, s->stream); if (rc) return rc;
  HIP_TRY(hipMemsetAsync(P->Q.p, 0, (size_t)2 * n_bins * GMPNP_MAX_SURFACE_REACTIONS * sizeof(double), s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  P->rec.open = true;
  return GMPNP_OK;
}

int gmpnp_wall_profile_append(gmpnp_solver* s, double t, double h) {
  if (!s) return fail(GMPNP_ERR_INVALID, "wall profile: NULL argument");
  if (int rc = wall_profile_refuse(s)) return rc;
  if (!wall_profile_is_open(s)) return fail(GMPNP_ERR_INVALID, kWallProfileNouns.not_open());
  if (!record_step_valid(t, h)) return fail(GMPNP_ERR_INVALID, "wall profile: t finite, h finite and > 0");
  gmpnp_wall_profiler* P = s->wall_profiler.get();
  if (P->rec.full()) return P->rec.refuse_full();
  HIP_TRY(hipSetDevice(s->opts.device_id));
  int rc = wall_profile_launch(s, t, h, P->rec.row(P->rec.count), 0); if (rc) return rc;
  P->rec.count += 1;
  return GMPNP_OK;
}

int gmpnp_wall_profile_read(gmpnp_solver* s, int32_t first, int32_t n, gmpnp_wall_profile_record_t* out) {
  if (!s || !out) return fail(GMPNP_ERR_INVALID, "wall profile: NULL argument");
  if (!wall_profile_is_open(s)) return fail(GMPNP_ERR_INVALID, kWallProfileNouns.not_open());
  HIP_TRY(hipSetDevice(s->opts.device_id));
  return s->wall_profiler->rec.read(first, n, out, s->stream);
}

int gmpnp_wall_profile_close(gmpnp_solver* s) {
  if (!s) return fail(GMPNP_ERR_INVALID, "wall profile: NULL argument");
  if (!wall_profile_is_open(s)) return fail(GMPNP_ERR_INVALID, kWallProfileNouns.not_open());
  s->wall_profiler->rec.close();
  return GMPNP_OK;
}

}  // extern "C"
