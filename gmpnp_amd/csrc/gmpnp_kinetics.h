// Potential-dependent surface kinetics on the device: gmpnp_set_kinetics / gmpnp_kinetics_currents (include/gmpnp.h), rule in
// gmpnp_host_rules.h (surface_rate).
//
// At every node I of the Stern boundary (1D: the point vertices, 3D: the vertices of the wall facets), with p_M the option's own
// p_electrode and w_I = 1 (1D) or the sum over the wall facets holding I of |f| / 3 in list order (3D):
//     E_r = exp(-alpha_r (p_M - p_I - p_eq_r))        rate_r = k_r (reactant_r >= 0 ? u_{I,reactant_r} : 1) E_r
//     F[(I,i)] += w_I sum_r nu[r][i] rate_r           J[(I,i),(I,reactant_r)] += w_I nu[r][i] k_r E_r
//                                                     J[(I,i),(I,p)]          += w_I nu[r][i] alpha_r rate_r
//
//   k_kinetics_residual   one lane per boundary node: its NF state values once, the <= 4 rates, bnd_dyn[(I,i)] = bndF[(I,i)] + term_i on
//                         the species rows (bndF alone on a Dirichlet row and on a species no reaction drives).  In front of every
//                         residual gather, beside k_stern_residual: the two write disjoint rows of the handle's one bnd_dyn.
//   k_kinetics_jacobian   one lane per (boundary node, species row): adds into that row of the node's own diagonal SELL block, at an
//                         address precomputed on the host (SternTab::addr with J = I); entries that are identically zero are skipped.
//                         Behind k_jac_gather / k_robin_add / k_stern_jacobian.
//   k_kinetics_sum        one workgroup, fixed order: the <= 4 integrated rates and the integrated kinetic flux per species (0 on a
//                         Dirichlet row), straight from u; the fluxes are added to the species rows' wall / point entries of a
//                         budget table when one is given.
// Every sum is a gather in a fixed order (no floating-point atomics): two calls on one state give equal bits.  The Dirichlet flags
// are read at run time.  A rate that is not finite: status bit 64.  The reactant and the rows are picked by selects out of unrolled
// loops, not by indexing a register array (an indexed array goes to scratch).
// Included at the end of gmpnp_api.hip.
#pragma once

namespace gmpnp {

struct KinTab {
  int32_t n_nodes, pad_;
  const gmpnp_kinetics_t* opt;   // device copy of the option
  const int32_t* node;           // [n_nodes] internal node, ascending
  const double* w;               // [n_nodes] w_I
  const int64_t* addr;           // [n_nodes] address in vals of J[(I,0),(I,0)]: entry (row i, column j) is addr + j * kWave + i
  const double* bndF;            // the constant boundary vector (rebuild_boundary)
  double* bnd_dyn;               // what the context's bndF points at
  int32_t* status;
};

// the rates of one boundary node from its state values uu[NF] (status bit 64 where one is not finite)
template <int NF>
__device__ __forceinline__ void kinetics_rates(const KinTab& t, const double (&uu)[NF], KinRate (&R)[GMPNP_MAX_SURFACE_REACTIONS]) {
  constexpr int NS = NF - 1;
  const gmpnp_kinetics_t* o = t.opt;
  const int nr = o->n_reactions;
  bool bad = false;
#pragma unroll
  for (int r = 0; r < GMPNP_MAX_SURFACE_REACTIONS; ++r) {
    R[r] = KinRate{0.0, 0.0, 0.0, 1};
    if (r < nr) {
      const int re = o->reactant[r];
      double ur = 0.0;
#pragma unroll
      for (int j = 0; j < NS; ++j) ur = (j == re) ? uu[j] : ur;
      R[r] = surface_rate(o->k[r], o->alpha[r], o->p_eq[r], o->p_electrode, uu[NS], re >= 0, ur);
      bad = bad || !R[r].ok;
    }
  }
  if (bad) atomicOr(t.status, 64);
}

template <int NF>
__global__ __launch_bounds__(kVecBlock) void k_kinetics_residual(const Ctx c, const KinTab t) {
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
      if (r < nr) { const double nu = o->nu[r][i]; term += nu * R[r].rate; driven = driven || nu != 0.0; }
    const double b = t.bndF[row0 + i];
    t.bnd_dyn[row0 + i] = (driven && !c.bcflag[row0 + i]) ? b + w * term : b;
  }
}

template <int NF>
__global__ __launch_bounds__(kVecBlock) void k_kinetics_jacobian(const Ctx c, const KinTab t) {
  constexpr int NS = NF - 1;
  const int wk = blockIdx.x * kVecBlock + threadIdx.x;
  if (wk >= t.n_nodes * NS) return;
  const int n = wk / NS, i = wk - n * NS;
  const size_t row0 = (size_t)t.node[n] * NF;
  if (c.bcflag[row0 + i]) return;
  const gmpnp_kinetics_t* o = t.opt;
  const int nr = o->n_reactions;
  const double p = c.u[row0 + NS], w = t.w[n];
  double* blk = c.vals + t.addr[n] + i;   // row i of the node's diagonal block: column j at blk[j * kWave]
  double vp = 0.0;
  bool any_p = false;
  for (int r = 0; r < nr; ++r) {
    const double nu = o->nu[r][i];
    if (nu == 0.0) continue;
    const int re = o->reactant[r];
    const double ur = re >= 0 ? c.u[row0 + re] : 0.0;
    const KinRate R = surface_rate(o->k[r], o->alpha[r], o->p_eq[r], o->p_electrode, p, re >= 0, ur);
    if (re >= 0) blk[(size_t)re * kWave] += w * (nu * R.d_u);   // one lane owns the row: reactions sharing a column add in order
    if (o->alpha[r] != 0.0) { vp += nu * R.d_p; any_p = true; }
  }
  if (any_p) blk[(size_t)NS * kWave] += w * vp;
}

// out[r] = sum_I w_I rate_r (r < 4), out[4 + i] = sum over the rows (I,i) that are not Dirichlet of w_I sum_r nu[r][i] rate_r; one
// workgroup, fixed order.  table != nullptr: out[4 + i] is added to table[i][column] (the species rows' wall / point entries).
template <int NF>
__global__ __launch_bounds__(kVecBlock) void k_kinetics_sum(const Ctx c, const KinTab t, double* __restrict__ out, double* __restrict__ table, int column) {
  constexpr int NS = NF - 1, K = GMPNP_MAX_SURFACE_REACTIONS + NS;
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
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      double term = 0.0;
#pragma unroll
      for (int r = 0; r < GMPNP_MAX_SURFACE_REACTIONS; ++r)
        if (r < nr) term += o->nu[r][i] * R[r].rate;
      v[GMPNP_MAX_SURFACE_REACTIONS + i] += c.bcflag[row0 + i] ? 0.0 : w * term;
    }
  }
  block_sum<K>(v, lds);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] = v[k];
    if (table)
#pragma unroll
      for (int i = 0; i < NS; ++i) table[i * GMPNP_BUDGET_COLUMNS + column] += v[GMPNP_MAX_SURFACE_REACTIONS + i];
  }
}

}  // namespace gmpnp

namespace {

// w_I of every vertex (0 off the Stern boundary) and the flags of the boundary's vertices: geometry only (also gmpnp_trace.h)
void boundary_weights(const gmpnp_solver* s, std::vector<double>& wv, std::vector<uint8_t>& on) {
  const Topology& t = s->t;
  wv.assign((size_t)t.nv, 0.0);
  on.assign((size_t)t.nv, 0);
  if (s->dim == 3) {
    for (size_t k = 0; k + 2 < s->wall_f.size(); k += 3) {
      const int32_t* f = &s->wall_f[k];
      const double* a = &t.coords[(size_t)f[0] * 3]; const double* b = &t.coords[(size_t)f[1] * 3]; const double* c = &t.coords[(size_t)f[2] * 3];
      const double ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2], vx = c[0] - a[0], vy = c[1] - a[1], vz = c[2] - a[2];
      const double cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
      const double ar = 0.5 * std::sqrt(cx * cx + cy * cy + cz * cz);
      for (int q = 0; q < 3; ++q) { wv[f[q]] += ar / 3.0; on[f[q]] = 1; }
    }
  } else {
    for (int v : s->point_v) { wv[v] += 1.0; on[v] = 1; }
  }
}

// the boundary nodes in ascending internal order, their weights and the addresses of their diagonal blocks: geometry only
int kinetics_build(gmpnp_solver* s, gmpnp_kineticist* K) {
  const Topology& t = s->t;
  const int nf = s->nf;
  std::vector<double> wv;
  std::vector<uint8_t> on;
  boundary_weights(s, wv, on);
  std::vector<int32_t> node; std::vector<double> w; std::vector<int64_t> addr;
  for (int I = 0; I < t.nv; ++I) {
    if (!on[I]) continue;
    const int32_t* b = t.cols.data() + t.rowptr[I]; const int32_t* e = t.cols.data() + t.rowptr[I + 1];
    const int32_t* hit = std::lower_bound(b, e, I);
    if (hit == e || *hit != I) return fail(GMPNP_ERR_INVALID, "surface kinetics: a boundary node has no diagonal block");
    const int kpos = t.sellk[(int)(hit - t.cols.data())];
    const int sl = t.node_slice[I], il = I - t.slice_node0[sl];
    node.push_back(I); w.push_back(wv[I]);
    addr.push_back(t.slice_off[sl] + (int64_t)(kpos * nf) * kWave + il * nf);
  }
  if (node.empty()) return fail(GMPNP_ERR_INVALID, "surface kinetics: the mesh has no Stern boundary (wall facets in 3D, point vertices in 1D)");
  K->n_nodes = (int)node.size();
  HIP_TRY(K->node.upload(node)); HIP_TRY(K->w.upload(w)); HIP_TRY(K->addr.upload(addr));
  HIP_TRY(K->d_opt.alloc(1)); HIP_TRY(K->status.alloc(1)); HIP_TRY(K->sum.alloc(GMPNP_MAX_SURFACE_REACTIONS + GMPNP_MAX_SPECIES));
  return GMPNP_OK;
}

KinTab kinetics_tab(gmpnp_solver* s, int32_t* status) {
  gmpnp_kineticist* K = s->kineticist.get();
  KinTab t{};
  t.n_nodes = K->n_nodes; t.opt = K->d_opt.p; t.node = K->node.p; t.w = K->w.p; t.addr = K->addr.p;
  t.bndF = s->bndF.p; t.bnd_dyn = s->bnd_dyn.p; t.status = status;
  return t;
}

int kinetics_launch_residual(gmpnp_solver* s, int32_t* status) {
  const KinTab t = kinetics_tab(s, status);
  GMPNP_DISPATCH(s, hipLaunchKernelGGL((k_kinetics_residual<NF>), dim3(grid_for(t.n_nodes, kVecBlock)), dim3(kVecBlock), 0, s->stream, s->c, t));
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

int kinetics_launch_jacobian(gmpnp_solver* s) {
  const KinTab t = kinetics_tab(s, s->status.p);
  GMPNP_DISPATCH(s, hipLaunchKernelGGL((k_kinetics_jacobian<NF>), dim3(grid_for(t.n_nodes * (s->nf - 1), kVecBlock)), dim3(kVecBlock), 0, s->stream, s->c, t));
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

// the integrated rates and fluxes at the u the stream holds -> kineticist->sum (the fluxes also into the budget table, if given)
int kinetics_launch_sum(gmpnp_solver* s, int32_t* status, double* table) {
  const KinTab t = kinetics_tab(s, status);
  GMPNP_DISPATCH(s, hipLaunchKernelGGL((k_kinetics_sum<NF>), dim3(1), dim3(kVecBlock), 0, s->stream, s->c, t, s->kineticist->sum.p, table,
                                       (int)(DIM == 3 ? GMPNP_BUDGET_WALL : GMPNP_BUDGET_POINT)));
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

}  // namespace

extern "C" {

int gmpnp_set_kinetics(gmpnp_solver* s, const gmpnp_kinetics_t* o) {
  if (!s || !o) return fail(GMPNP_ERR_INVALID, "surface kinetics: NULL argument");
  if (!kinetics_options_valid(*o, s->nf - 1))
    return fail(GMPNP_ERR_INVALID, "surface kinetics: n_reactions in 0 ... 4, finite k, alpha, p_eq, nu and p_electrode, reactant in -1 ... n_species - 1");
  if (o->n_reactions == 0 && !s->kineticist) return GMPNP_OK;   // never on: the handle stays as it was
  if (o->n_reactions == 0 && galvanostat_on(s)) return fail(GMPNP_ERR_INVALID, "surface kinetics: the galvanostat is on (gmpnp_set_galvanostat) and needs them; switch it off first");
  if (o->n_reactions != 0) {
    if (s->partitioned) return fail(GMPNP_ERR_INVALID, "surface kinetics: partition handles and groups are not supported");
    if (s->ml_coarse || s->ml_is_coarse) return fail(GMPNP_ERR_INVALID, "surface kinetics: not with a multilevel coarse level attached");
    if (s->c.supg_rho) return fail(GMPNP_ERR_INVALID, "surface kinetics: not with SUPG terms set (gmpnp_set_supg)");
  }
  HIP_TRY(hipSetDevice(s->opts.device_id));
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (!s->kineticist) {
    std::unique_ptr<gmpnp_kineticist> K(new gmpnp_kineticist);
    int rc = kinetics_build(s, K.get()); if (rc) return rc;
    s->kineticist = std::move(K);
  }
  tangent_drop(s);
  s->kineticist->opt = *o;
  if (galvanostat_on(s))   // the galvanostat's p_M stays (the stream is idle: its last update has landed)
    HIP_TRY(hipMemcpy(&s->kineticist->opt.p_electrode, s->galvanostat->scal.p, sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(s->kineticist->d_opt.p, &s->kineticist->opt, sizeof(gmpnp_kinetics_t), hipMemcpyHostToDevice));
  s->jacobian_valid = false; s->precond_valid = false;
  return boundary_rebind(s);
}

int gmpnp_kinetics_currents(gmpnp_solver* s, double* out) {
  if (!s || !out) return fail(GMPNP_ERR_INVALID, "surface kinetics: NULL argument");
  if (!kinetics_on(s)) return fail(GMPNP_ERR_INVALID, "surface kinetics: the option is off (gmpnp_set_kinetics)");
  HIP_TRY(hipSetDevice(s->opts.device_id));
  int32_t* st = s->kineticist->status.p;   // (a rate that is not finite shows in the result; the solver's status word stays what it was)
  int rc = kinetics_launch_residual(s, st); if (rc) return rc;
  rc = kinetics_launch_sum(s, st, nullptr); if (rc) return rc;
  const int nr = s->kineticist->opt.n_reactions;
  HIP_TRY(hipMemcpyAsync(s->h_stage, s->kineticist->sum.p, nr * sizeof(double), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  for (int r = 0; r < nr; ++r) out[r] = s->h_stage[r];
  return GMPNP_OK;
}

}  // extern "C"
