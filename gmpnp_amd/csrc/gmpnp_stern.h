// Stern-layer boundary condition on the device: gmpnp_set_stern / gmpnp_stern_displacement (include/gmpnp.h), rule in gmpnp_host_rules.h.
//
// On the Stern boundary the potential row gains  int g(eps) (p_M - p) / lam v ds  (1D: at the point vertices with eps at the vertex;
// 3D: per wall facet with eps at the facet mean of u and (p_M - p) as P1 with the facet mass matrix |f| (1 + delta_ab) / 12):
//     1D   F[p_v] += g (p_M - p_v) / lam          J[p_v, p_v] += -g / lam            J[p_v, u_{v,j}] += g' epsc_j (p_M - p_v) / lam
//     3D   w_a = |f| (p_M / 3 - (p_0 + p_1 + p_2 + p_a) / 12)
//          F[p_a] += g w_a / lam                  J[p_a, p_b] += -g Mf_ab / lam      J[p_a, u_{b,j}] += g' (epsc_j / 3) w_a / lam
//
//   k_stern_residual   one lane per Stern node: its incident Stern facets in list order -> bnd_dyn[p row] = bndF[p row] + term.  The
//                      other rows of bnd_dyn are a copy of bndF made on the host side of gmpnp_set_stern / rebuild_boundary, and the
//                      context's bndF pointer is bnd_dyn while the option is on: res_gather_body and the budget's row pass read it
//                      unchanged, and the constant bndF is never written.
//   k_stern_jacobian   one lane per (ordered Stern node pair sharing a facet, column of the potential row): the facets holding both
//                      nodes in list order, added to the SELL value at an address precomputed like rob_addr (every pair shares an
//                      element, so the pattern holds the block).  Behind k_jac_gather / k_robin_add.
//   k_stern_sum        one workgroup: the integrated term, sum over the Stern nodes of bnd_dyn - bndF, fixed order
// Every sum is a gather in list order (no floating-point atomics): two calls on one state give equal bits.  A potential row with a
// Dirichlet flag is skipped by all three, as k_robin_add skips Dirichlet rows.  eps <= 0 (BDM): status bit 32, g = g' = 0.
// bnd_dyn is the handle's one dynamic boundary vector (boundary_rebind, gmpnp_api.hip), shared with the surface kinetics
// (gmpnp_kinetics.h), which write the species rows only.
// Included at the end of gmpnp_api.hip.
#pragma once

namespace gmpnp {

struct SternTab {
  int32_t n_nodes, n_pairs, model, pad_;
  double p_M, lam, eps_s;
  const double* p_M_dev;    // the galvanostat's p_M on the device (gmpnp_galvanostat.h); nullptr: p_M above, by value
  const int32_t* node;      // [n_nodes] internal node
  const int32_t* nf_ptr;    // [n_nodes+1] CSR over the Stern nodes of (facet << 2 | local position)
  const int32_t* nf_ent;
  const int32_t* fnodes;    // [n_facets][FN] internal nodes (FN = 3 in 3D, 1 in 1D)
  const double* area;       // [n_facets] |f| (1D: 1)
  const int32_t* pair_row;  // [n_pairs] row node I of the pair (I, J)
  const int32_t* pf_ptr;    // [n_pairs+1] CSR over the pairs of (facet << 4 | a << 2 | b)
  const int32_t* pf_ent;
  const int64_t* addr;      // [n_pairs][NF] address in vals of J[p_I, (J, column)]
  const double* bndF;       // the constant boundary vector (rebuild_boundary)
  double* bnd_dyn;          // what the context's bndF points at
  int32_t* status;
};

// one Stern facet at the current u: nodal potentials, g and g' at its permittivity (status bit 32 where eps <= 0 under BDM)
template <int DIM, int NF>
struct SternFacet {
  static constexpr int FN = DIM == 3 ? 3 : 1;
  double p[FN], psum, area, pM;
  SternG G;
  __device__ __forceinline__ SternFacet(const Ctx& c, const SternTab& t, int f) {
    constexpr int NS = NF - 1;
    const gmpnp_model_t* m = c.model;
    int nd[FN];
    psum = 0.0;
#pragma unroll
    for (int a = 0; a < FN; ++a) { nd[a] = t.fnodes[f * FN + a]; p[a] = c.u[(size_t)nd[a] * NF + NS]; psum += p[a]; }
    double eps = m->eps0;
    for (int j = 0; j < NS; ++j) {
      double us = 0.0;
#pragma unroll
      for (int a = 0; a < FN; ++a) us += c.u[(size_t)nd[a] * NF + j];
      eps += m->epsc[j] * (us / FN);
    }
    area = t.area[f];
    pM = t.p_M_dev ? *t.p_M_dev : t.p_M;
    G = stern_g(t.model, eps, t.eps_s);
    if (!G.ok) atomicOr(t.status, 32);
  }
  // w_a = int (p_M - p) phi_a ds
  __device__ __forceinline__ double w(const SternTab& t, int a) const {
    if constexpr (DIM == 3) {
      const double pa = a == 0 ? p[0] : a == 1 ? p[1] : p[2];   // (a select, not an index: the array stays in registers)
      return area * (pM / 3.0 - (psum + pa) / 12.0);
    } else return pM - p[0];
  }
  __device__ __forceinline__ double mass(int a, int b) const {
    if constexpr (DIM == 3) return area * (a == b ? 2.0 : 1.0) / 12.0;
    else return 1.0;
  }
};

template <int DIM, int NF>
__global__ __launch_bounds__(kVecBlock) void k_stern_residual(const Ctx c, const SternTab t) {
  const int n = blockIdx.x * kVecBlock + threadIdx.x;
  if (n >= t.n_nodes) return;
  const int row = t.node[n] * NF + (NF - 1);
  double term = 0.0;
  for (int k = t.nf_ptr[n]; k < t.nf_ptr[n + 1]; ++k) {
    const int ent = t.nf_ent[k];
    const SternFacet<DIM, NF> F(c, t, ent >> 2);
    term += F.G.g * F.w(t, ent & 3) / t.lam;
  }
  const double b = t.bndF[row];
  t.bnd_dyn[row] = c.bcflag[row] ? b : b + term;
}

template <int DIM, int NF>
__global__ __launch_bounds__(kVecBlock) void k_stern_jacobian(const Ctx c, const SternTab t) {
  constexpr int NS = NF - 1;
  const int w = blockIdx.x * kVecBlock + threadIdx.x;
  if (w >= t.n_pairs * NF) return;
  const int pr = w / NF, col = w - pr * NF;
  if (c.bcflag[t.pair_row[pr] * NF + NS]) return;
  const gmpnp_model_t* m = c.model;
  double v = 0.0;
  for (int k = t.pf_ptr[pr]; k < t.pf_ptr[pr + 1]; ++k) {
    const int ent = t.pf_ent[k];
    const int a = (ent >> 2) & 3, b = ent & 3;
    const SternFacet<DIM, NF> F(c, t, ent >> 4);
    if (col == NS) v += -F.G.g * F.mass(a, b) / t.lam;
    else v += F.G.dg * (m->epsc[col] / SternFacet<DIM, NF>::FN) * F.w(t, a) / t.lam;
  }
  c.vals[t.addr[w]] += v;
}

// out[0] = sum over the Stern nodes of (bnd_dyn - bndF) on the potential rows (0 on a Dirichlet row); one workgroup, fixed order.
// table != nullptr: the value also goes there (the potential row's wall / point entry of the budget table).
template <int NF>
__global__ __launch_bounds__(kVecBlock) void k_stern_sum(const SternTab t, double* __restrict__ out, double* __restrict__ table) {
  __shared__ double lds[4];
  double v[1] = {0.0};
  for (int n = threadIdx.x; n < t.n_nodes; n += kVecBlock) {
    const int row = t.node[n] * NF + (NF - 1);
    v[0] += t.bnd_dyn[row] - t.bndF[row];
  }
  block_sum<1>(v, lds);
  if (threadIdx.x == 0) { out[0] = v[0]; if (table) table[0] = v[0]; }
}

}  // namespace gmpnp

namespace {

// gather lists of the Stern boundary (internal node ids): geometry only, the Dirichlet flags are read at run time
int stern_build(gmpnp_solver* s, gmpnp_sterner* S) {
  const Topology& t = s->t;
  const int nf = s->nf, fn = s->dim == 3 ? 3 : 1;
  std::vector<int32_t> fnodes; std::vector<double> area;
  if (s->dim == 3) {
    for (size_t k = 0; k + 2 < s->wall_f.size(); k += 3) {
      const int32_t* f = &s->wall_f[k];
      const double* a = &t.coords[(size_t)f[0] * 3]; const double* b = &t.coords[(size_t)f[1] * 3]; const double* c = &t.coords[(size_t)f[2] * 3];
      const double ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2], vx = c[0] - a[0], vy = c[1] - a[1], vz = c[2] - a[2];
      const double cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
      fnodes.insert(fnodes.end(), f, f + 3); area.push_back(0.5 * std::sqrt(cx * cx + cy * cy + cz * cz));
    }
  } else {
    for (int v : s->point_v) { fnodes.push_back(v); area.push_back(1.0); }
  }
  const int nfac = (int)area.size();
  if (nfac == 0) return fail(GMPNP_ERR_INVALID, "Stern boundary condition: the mesh has no Stern boundary (wall facets in 3D, point vertices in 1D)");
  // Stern nodes in ascending internal order, each with its incident facets in list order
  std::vector<int32_t> slot((size_t)t.nv, -1), node;
  for (int v : fnodes) if (slot[v] < 0) { slot[v] = 0; }
  for (int I = 0; I < t.nv; ++I) if (slot[I] == 0) { slot[I] = (int32_t)node.size(); node.push_back(I); }
  const int nn = (int)node.size();
  std::vector<int32_t> nf_ptr((size_t)nn + 1, 0), nf_ent;
  for (int f = 0; f < nfac; ++f) for (int a = 0; a < fn; ++a) nf_ptr[slot[fnodes[f * fn + a]] + 1]++;
  for (int n = 0; n < nn; ++n) nf_ptr[n + 1] += nf_ptr[n];
  nf_ent.resize(nf_ptr[nn]);
  { std::vector<int32_t> fill(nf_ptr.begin(), nf_ptr.end() - 1);
    for (int f = 0; f < nfac; ++f) for (int a = 0; a < fn; ++a) nf_ent[fill[slot[fnodes[f * fn + a]]]++] = (f << 2) | a; }
  // ordered pairs (I, J) sharing a facet, sorted by (I, J); the facets of a pair stay in list order (stable sort)
  struct PE { int32_t I, J, ent; };
  std::vector<PE> pe;
  for (int f = 0; f < nfac; ++f)
    for (int a = 0; a < fn; ++a)
      for (int b = 0; b < fn; ++b) pe.push_back({fnodes[f * fn + a], fnodes[f * fn + b], (f << 4) | (a << 2) | b});
  std::stable_sort(pe.begin(), pe.end(), [](const PE& x, const PE& y) { return x.I != y.I ? x.I < y.I : x.J < y.J; });
  std::vector<int32_t> pair_row, pf_ptr(1, 0), pf_ent; std::vector<int64_t> addr;
  for (size_t k = 0; k < pe.size();) {
    size_t j = k;
    while (j < pe.size() && pe[j].I == pe[k].I && pe[j].J == pe[k].J) pf_ent.push_back(pe[j++].ent);
    const int I = pe[k].I, J = pe[k].J;
    const int32_t* b = t.cols.data() + t.rowptr[I]; const int32_t* e = t.cols.data() + t.rowptr[I + 1];
    const int32_t* hit = std::lower_bound(b, e, J);
    if (hit == e || *hit != J) return fail(GMPNP_ERR_INVALID, "Stern boundary condition: a boundary facet is not the face of a cell");
    const int kpos = t.sellk[(int)(hit - t.cols.data())];
    const int sl = t.node_slice[I], il = I - t.slice_node0[sl];
    for (int jf = 0; jf < nf; ++jf) addr.push_back(t.slice_off[sl] + (int64_t)(kpos * nf + jf) * kWave + il * nf + (nf - 1));
    pair_row.push_back(I); pf_ptr.push_back((int32_t)pf_ent.size());
    k = j;
  }
  S->n_nodes = nn; S->n_pairs = (int)pair_row.size();
  HIP_TRY(S->node.upload(node)); HIP_TRY(S->nf_ptr.upload(nf_ptr)); HIP_TRY(S->nf_ent.upload(nf_ent)); HIP_TRY(S->fnodes.upload(fnodes));
  HIP_TRY(S->area.upload(area)); HIP_TRY(S->pair_row.upload(pair_row)); HIP_TRY(S->pf_ptr.upload(pf_ptr)); HIP_TRY(S->pf_ent.upload(pf_ent));
  HIP_TRY(S->addr.upload(addr));
  HIP_TRY(S->sum.alloc(1));
  return GMPNP_OK;
}

SternTab stern_tab(gmpnp_solver* s, int32_t* status) {
  gmpnp_sterner* S = s->sterner.get();
  SternTab t{};
  t.n_nodes = S->n_nodes; t.n_pairs = S->n_pairs; t.model = S->opt.model;
  t.p_M = S->opt.p_electrode; t.lam = S->opt.lam; t.eps_s = S->opt.eps_surface;
  t.p_M_dev = galvanostat_p_M(s);
  t.node = S->node.p; t.nf_ptr = S->nf_ptr.p; t.nf_ent = S->nf_ent.p; t.fnodes = S->fnodes.p; t.area = S->area.p;
  t.pair_row = S->pair_row.p; t.pf_ptr = S->pf_ptr.p; t.pf_ent = S->pf_ent.p; t.addr = S->addr.p;
  t.bndF = s->bndF.p; t.bnd_dyn = s->bnd_dyn.p; t.status = status;
  return t;
}

int stern_launch_residual(gmpnp_solver* s, int32_t* status) {
  const SternTab t = stern_tab(s, status);
  GMPNP_DISPATCH(s, hipLaunchKernelGGL((k_stern_residual<DIM, NF>), dim3(grid_for(t.n_nodes, kVecBlock)), dim3(kVecBlock), 0, s->stream, s->c, t));
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

int stern_launch_jacobian(gmpnp_solver* s) {
  const SternTab t = stern_tab(s, s->status.p);
  GMPNP_DISPATCH(s, hipLaunchKernelGGL((k_stern_jacobian<DIM, NF>), dim3(grid_for(t.n_pairs * s->nf, kVecBlock)), dim3(kVecBlock), 0, s->stream, s->c, t));
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

// the integrated term of the bnd_dyn the stream holds -> S->sum (and the budget table's entry, if given)
int stern_launch_sum(gmpnp_solver* s, double* table_entry) {
  const SternTab t = stern_tab(s, s->status.p);
  GMPNP_DISPATCH(s, hipLaunchKernelGGL((k_stern_sum<NF>), dim3(1), dim3(kVecBlock), 0, s->stream, t, s->sterner->sum.p, table_entry));
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

}  // namespace

extern "C" {

int gmpnp_set_stern(gmpnp_solver* s, const gmpnp_stern_t* o) {
  if (!s || !o) return fail(GMPNP_ERR_INVALID, "Stern boundary condition: NULL argument");
  if (!stern_options_valid(*o)) return fail(GMPNP_ERR_INVALID, "Stern boundary condition: model 0 / 1 / 2, a finite p_electrode, lam > 0 and (BDM) eps_surface > 0");
  if (o->model == 0 && !s->sterner) return GMPNP_OK;   // never on: the handle stays as it was
  if (o->model != 0) {
    if (s->partitioned) return fail(GMPNP_ERR_INVALID, "Stern boundary condition: partition handles and groups are not supported");
    if (s->ml_coarse || s->ml_is_coarse) return fail(GMPNP_ERR_INVALID, "Stern boundary condition: not with a multilevel coarse level attached");
  }
  HIP_TRY(hipSetDevice(s->opts.device_id));
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (!s->sterner) {
    std::unique_ptr<gmpnp_sterner> S(new gmpnp_sterner);
    int rc = stern_build(s, S.get()); if (rc) return rc;
    s->sterner = std::move(S);
  }
  tangent_drop(s);
  s->sterner->opt = *o;   // (with the galvanostat on the kernels read ITS p_M: p_electrode is what on = 0 writes back)
  s->jacobian_valid = false; s->precond_valid = false;
  return boundary_rebind(s);
}

int gmpnp_stern_displacement(gmpnp_solver* s, double* out) {
  if (!s || !out) return fail(GMPNP_ERR_INVALID, "Stern boundary condition: NULL argument");
  if (!stern_on(s)) return fail(GMPNP_ERR_INVALID, "Stern boundary condition: the option is off (gmpnp_set_stern)");
  HIP_TRY(hipSetDevice(s->opts.device_id));
  int rc = stern_launch_residual(s, s->status.p); if (rc) return rc;
  rc = stern_launch_sum(s, nullptr); if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(s->h_stage, s->sterner->sum.p, sizeof(double), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  *out = s->h_stage[0];
  return GMPNP_OK;
}

}  // extern "C"
