// Species budgets and consistent boundary fluxes on the device: gmpnp_species_budget / gmpnp_group_species_budget (include/gmpnp.h).
//
// P1 test functions sum to one, so the RAW residual rows of one field (before the Dirichlet replacement) sum to that field's integrated
// balance: every term whose test-function factor is a gradient (diffusion, migration, steric, SUPG) drops out of the sum.  Per field
// one row of GMPNP_BUDGET_COLUMNS doubles with
//     storage + reaction + wall + exit + point  =  dirichlet + closure        (to rounding, for any state)
// the left side from closed-form P1 integrals (MDEN / KAPPA monomials, the element body's own), the right side from the gathered
// element rows plus the boundary terms, binned by the Dirichlet flag.  The two sides share no arithmetic: the identity is the check.
//
//   k_budget_cells   one lane per cell: per local node the shares of inventory / storage / reaction, added only where the node's row
//                    is OWNED (own_node0 <= I < own_node1) — a partition counts every row once without a cell-ownership rule, because
//                    cut cells are assembled on both sides and owned rows are complete
//   k_budget_rows    one lane per owned dof: the raw row as res_gather_body forms it (bndF, incident EF rows, Robin entries) without the
//                    Dirichlet replacement -> dirichlet | closure; wall / exit / point from geometry-only facet tables (bndF merges them)
//   k_budget_final   one workgroup: the workgroup partials of both passes in a fixed order -> table[field][column]
// With the Stern boundary condition on (gmpnp_stern.h) k_stern_residual refreshes the term at the current u in front of the row pass
// (c.bndF is then bnd_dyn) and k_stern_sum writes the integrated term into the potential row's wall (3D) / point (1D) entry.
// With the surface kinetics on (gmpnp_kinetics.h) k_kinetics_residual does the same for the species rows and k_kinetics_sum adds
// the integrated kinetic flux of every species to its wall / point entry.
// Reductions are fixed-order sums of per-workgroup partials (no floating-point atomics): two calls on one state give equal bits.
// The element residual is evaluated at the current u by k_element<.., WANT_J = false> into a buffer of the budget's own, with a status
// word of its own: u, u_n, F, EF, kr / kb, the Jacobian, the preconditioner and the device status stay what they were.
// Included at the end of gmpnp_api.hip (after gmpnp_group.h, whose group_allreduce the group form uses).
#pragma once

namespace gmpnp {

constexpr int kBudgetCellCols = 3;   // inventory, storage, reaction      (cell pass)
constexpr int kBudgetRowCols = 5;    // wall, exit, point, dirichlet, closure   (row pass)
static_assert(kBudgetCellCols + kBudgetRowCols == GMPNP_BUDGET_COLUMNS, "the two passes fill the table");

// geometry-only boundary tables in internal node order (built on first use; they do not depend on the model)
struct BudgetGeo {
  const double* wall_w;     // [nv] sum over the ds(2) facets at the node of |f| / 3
  const double* exit_w;     // [nv] the same over ds(3)
  const int32_t* exit_ptr;  // [nv+1] CSR over nodes of the ds(3) facet mass matrix
  const int32_t* exit_col;  // column node
  const double* exit_val;   // |f| (1 + delta_ab) / 12
  const double* point_w;    // [nv] times the node is listed as a point vertex (1D)
};

template <int DIM, int NF>
__global__ __launch_bounds__(kVecBlock) void k_budget_cells(const Ctx c, double* __restrict__ part /* [3][NF][gridDim.x] */) {
  using L = Lay<DIM, NF>;
  constexpr int NS = L::NS, NN = L::NN;
  __shared__ gmpnp_model_t m;
  __shared__ double lds[4 * kBudgetCellCols * NF];
  {
    static_assert(sizeof(gmpnp_model_t) % 4 == 0, "word-wise staging");
    const uint32_t* gm = reinterpret_cast<const uint32_t*>(c.model);
    uint32_t* lm = reinterpret_cast<uint32_t*>(&m);
    for (int w = threadIdx.x; w < (int)(sizeof(gmpnp_model_t) / 4); w += kVecBlock) lm[w] = gm[w];
  }
  __syncthreads();
  const int e_raw = blockIdx.x * kVecBlock + threadIdx.x;
  const bool on = e_raw < c.nc;
  const int e = min(e_raw, c.nc - 1);   // every lane stays for the reduction (surplus lanes redo the last cell, masked)
  int nd[NN];
  double X[NN][DIM], U[NN][NF], dU[NN][NS];
#pragma unroll
  for (int a = 0; a < NN; ++a) {
    nd[a] = c.cells[e * NN + a];
#pragma unroll
    for (int d = 0; d < DIM; ++d) X[a][d] = c.coords[(size_t)nd[a] * DIM + d];
#pragma unroll
    for (int f = 0; f < NF; ++f) U[a][f] = c.u[(size_t)nd[a] * NF + f];
#pragma unroll
    for (int i = 0; i < NS; ++i) dU[a][i] = U[a][i] - c.un[(size_t)nd[a] * NF + i];
  }
  double vol;
  if constexpr (DIM == 1) {
    vol = fabs(X[1][0] - X[0][0]);
  } else {
    double T[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int d = 0; d < 3; ++d) T[r][d] = X[r + 1][d] - X[0][d];
    const double det = T[0][0] * (T[1][1] * T[2][2] - T[1][2] * T[2][1]) + T[0][1] * (T[1][2] * T[2][0] - T[1][0] * T[2][2]) +
                       T[0][2] * (T[1][0] * T[2][1] - T[1][1] * T[2][0]);
    vol = fabs(det) * (1.0 / 6.0);
  }
  double usum[NF], dusum[NS];
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    double s = 0.0;
#pragma unroll
    for (int a = 0; a < NN; ++a) s += U[a][f];
    usum[f] = s;
  }
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    double s = 0.0;
#pragma unroll
    for (int a = 0; a < NN; ++a) s += dU[a][i];
    dusum[i] = s;
  }
  // bilinear monomials int u_x u_y phi_a = |K| kappa (XY + x_a Y + X y_a + D + 2 x_a y_a)   (gmpnp_element_body.inc)
  double mono[GMPNP_MAX_BILINEAR][NN];
  for (int t = 0; t < m.n_bilinear; ++t) {
    const int bj = m.bil_j[t], bk = m.bil_k[t];
    double xs[NN], ys[NN], Xs = 0.0, Ys = 0.0, D = 0.0;
#pragma unroll
    for (int a = 0; a < NN; ++a) {
      double xv = 0.0, yv = 0.0;
#pragma unroll
      for (int j = 0; j < NS; ++j) { xv = (j == bj) ? U[a][j] : xv; yv = (j == bk) ? U[a][j] : yv; }
      xs[a] = xv; ys[a] = yv; Xs += xv; Ys += yv; D += xv * yv;
    }
#pragma unroll
    for (int a = 0; a < NN; ++a) mono[t][a] = vol * L::KAPPA * (Xs * Ys + xs[a] * Ys + Xs * ys[a] + D + 2.0 * xs[a] * ys[a]);
  }
  double acc[kBudgetCellCols * NF];
#pragma unroll
  for (int k = 0; k < kBudgetCellCols * NF; ++k) acc[k] = 0.0;
#pragma unroll
  for (int a = 0; a < NN; ++a) {
    const bool mine = on && nd[a] >= c.own_node0 && nd[a] < c.own_node1;
    double mass[NF];   // int u_f phi_a = |K| MDEN (sum_b u_b + u_a)
#pragma unroll
    for (int f = 0; f < NF; ++f) mass[f] = vol * L::MDEN * (usum[f] + U[a][f]);
    double charge = 0.0;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      double r = m.rc0[i] * vol * (1.0 / NN);
#pragma unroll
      for (int j = 0; j < NS; ++j) r += m.rc1[i][j] * mass[j];
      for (int t = 0; t < m.n_bilinear; ++t) r += m.rc2[i][t] * mono[t][a];
      const double st = m.inv_dt * vol * L::MDEN * (dusum[i] + dU[a][i]);
      acc[0 * NF + i] += mine ? mass[i] : 0.0;
      acc[1 * NF + i] += mine ? st : 0.0;
      acc[2 * NF + i] += mine ? r : 0.0;
      charge += m.qzb[i] * mass[i];
    }
    acc[0 * NF + NS] += mine ? mass[NS] : 0.0;
    acc[2 * NF + NS] += mine ? charge : 0.0;   // potential row: the space-charge term (its storage stays 0)
  }
  block_sum<kBudgetCellCols * NF>(acc, lds);
  if (threadIdx.x < kBudgetCellCols * NF) {
    double v = 0.0;
#pragma unroll
    for (int k = 0; k < kBudgetCellCols * NF; ++k) v = ((int)threadIdx.x == k) ? acc[k] : v;
    part[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = v;
  }
}

template <int DIM, int NF>
__global__ __launch_bounds__(kVecBlock) void k_budget_rows(const Ctx c, const double* __restrict__ EF, const BudgetGeo g,
                                                           double* __restrict__ part /* [5][NF][gridDim.x] */) {
  using L = Lay<DIM, NF>;
  constexpr int NS = NF - 1;
  __shared__ double sh[kBudgetRowCols][kVecBlock];
  const int r0 = blockIdx.x * kVecBlock, r = r0 + (int)threadIdx.x;
  double wall = 0.0, exitv = 0.0, point = 0.0, raw = 0.0;
  bool dirichlet = false;
  if (r < c.ndof) {
    const int I = r / NF, i = r - I * NF;
    if (I >= c.own_node0 && I < c.own_node1) {   // ghost rows of a partitioned handle: the owner's rank counts them
      double s = c.bndF[r];
      for (int k = c.n2e_ptr[I]; k < c.n2e_ptr[I + 1]; ++k) {
        const int pk = c.n2e[k];
        const int e = pk / L::NN, a = pk - e * L::NN;
        s += EF[(size_t)e * L::EF_STRIDE + a * NF + i];
      }
      for (int k = c.robF_ptr[r]; k < c.robF_ptr[r + 1]; ++k) s += c.rob_val[k] * c.u[c.rob_col[k]];
      raw = s;
      dirichlet = c.bcflag[r] != 0;
      if (i < NS) {
        const gmpnp_model_t* m = c.model;
        wall = m->wall_flux[i] * g.wall_w[I];
        point = m->point_flux[i] * g.point_w[I];
        double mu = 0.0;   // int_S3 u_i phi_I ds
        for (int k = g.exit_ptr[I]; k < g.exit_ptr[I + 1]; ++k) mu += g.exit_val[k] * c.u[(size_t)g.exit_col[k] * NF + i];
        exitv = m->exit_kappa[i] * (mu - g.exit_w[I]);
      }
    }
  }
  sh[0][threadIdx.x] = wall; sh[1][threadIdx.x] = exitv; sh[2][threadIdx.x] = point;
  sh[3][threadIdx.x] = dirichlet ? raw : 0.0; sh[4][threadIdx.x] = dirichlet ? 0.0 : raw;
  __syncthreads();
  // thread (column q, field f): the workgroup's rows of field f in ascending order
  if (threadIdx.x < kBudgetRowCols * NF) {
    const int q = threadIdx.x / NF, f = threadIdx.x - q * NF;
    const int first = (f - r0 % NF + NF) % NF;   // first lane of the workgroup whose dof has field f
    double s = 0.0;
    for (int j = first; j < kVecBlock; j += NF) s += sh[q][j];
    part[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = s;
  }
}

// table[f][column] = fixed-order sums of the partials: wave w takes the entries w, w + 4, ...
template <int NF>
__global__ __launch_bounds__(kVecBlock) void k_budget_final(const double* __restrict__ part_c, int nblk_c, const double* __restrict__ part_r, int nblk_r,
                                                            double* __restrict__ table /* [NF][GMPNP_BUDGET_COLUMNS] */) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int k = w; k < GMPNP_BUDGET_COLUMNS * NF; k += kVecBlock / 64) {
    const int col = k / NF, f = k - col * NF;
    const bool cell = col < kBudgetCellCols;
    const double* p = cell ? part_c + (size_t)(col * NF + f) * nblk_c : part_r + (size_t)((col - kBudgetCellCols) * NF + f) * nblk_r;
    const int n = cell ? nblk_c : nblk_r;
    double v = 0.0;
    for (int i = lane; i < n; i += 64) v += p[i];
    v = wave_sum(v);
    if (lane == 0) table[f * GMPNP_BUDGET_COLUMNS + col] = v;
  }
}

}  // namespace gmpnp

namespace {

// geometry-only facet tables of the handle (first call)
int budget_geometry(gmpnp_solver* s, gmpnp_budgeter* b) {
  const Topology& t = s->t;
  const int nv = t.nv;
  std::vector<double> wall_w((size_t)nv, 0.0), exit_w((size_t)nv, 0.0), point_w((size_t)nv, 0.0);
  auto area = [&](const int32_t* f) {
    const double* a = &t.coords[(size_t)f[0] * 3]; const double* bb = &t.coords[(size_t)f[1] * 3];
    const double* cc = &t.coords[(size_t)f[2] * 3];
    const double ux = bb[0] - a[0], uy = bb[1] - a[1], uz = bb[2] - a[2];
    const double vx = cc[0] - a[0], vy = cc[1] - a[1], vz = cc[2] - a[2];
    const double cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
    return 0.5 * std::sqrt(cx * cx + cy * cy + cz * cz);
  };
  struct Ent { int row, col; double v; };
  std::vector<Ent> ents;
  if (s->dim == 3) {
    for (size_t k = 0; k + 2 < s->wall_f.size(); k += 3) {
      const int32_t* f = &s->wall_f[k]; const double ar = area(f);
      for (int a = 0; a < 3; ++a) wall_w[f[a]] += ar / 3.0;
    }
    for (size_t k = 0; k + 2 < s->exit_f.size(); k += 3) {
      const int32_t* f = &s->exit_f[k]; const double ar = area(f);
      for (int a = 0; a < 3; ++a) {
        exit_w[f[a]] += ar / 3.0;
        for (int c2 = 0; c2 < 3; ++c2) ents.push_back({f[a], f[c2], ar * (a == c2 ? 2.0 : 1.0) / 12.0});
      }
    }
  }
  for (int v : s->point_v) point_w[v] += 1.0;
  std::stable_sort(ents.begin(), ents.end(), [](const Ent& a, const Ent& c2) { return a.row != c2.row ? a.row < c2.row : a.col < c2.col; });
  std::vector<int32_t> ptr((size_t)nv + 1, 0), col; std::vector<double> val;
  for (size_t k = 0; k < ents.size();) {
    size_t j = k; double v = 0.0;
    while (j < ents.size() && ents[j].row == ents[k].row && ents[j].col == ents[k].col) v += ents[j++].v;
    col.push_back(ents[k].col); val.push_back(v); ptr[ents[k].row + 1]++;
    k = j;
  }
  for (int I = 0; I < nv; ++I) ptr[I + 1] += ptr[I];
  HIP_TRY(b->wall_w.upload(wall_w)); HIP_TRY(b->exit_w.upload(exit_w)); HIP_TRY(b->point_w.upload(point_w));
  HIP_TRY(b->exit_ptr.upload(ptr)); HIP_TRY(b->exit_col.upload(col)); HIP_TRY(b->exit_val.upload(val));
  return GMPNP_OK;
}

// queues the three passes of one handle on its stream: the handle's table lands in budgeter->table (device)
template <int DIM, int NF>
int budget_launch(gmpnp_solver* s) {
  using L = Lay<DIM, NF>;
  HIP_TRY(hipSetDevice(s->opts.device_id));
  if (!s->budgeter) {
    std::unique_ptr<gmpnp_budgeter> b(new gmpnp_budgeter);
    int rc = budget_geometry(s, b.get()); if (rc) return rc;
    b->nblk_c = std::max(1, grid_for(s->t.nc, kVecBlock));
    b->nblk_r = std::max(1, grid_for(s->ndof, kVecBlock));
    HIP_TRY(b->EF.alloc((size_t)s->t.nc * L::EF_STRIDE, false));
    HIP_TRY(b->part_c.alloc((size_t)kBudgetCellCols * NF * b->nblk_c));
    HIP_TRY(b->part_r.alloc((size_t)kBudgetRowCols * NF * b->nblk_r));
    HIP_TRY(b->table.alloc((size_t)NF * GMPNP_BUDGET_COLUMNS));
    HIP_TRY(b->status.alloc(1));
    HIP_TRY(hipHostMalloc((void**)&b->h_table, sizeof(double) * GMPNP_BUDGET_COLUMNS * (GMPNP_MAX_SPECIES + 1)));
    s->budgeter = std::move(b);
  }
  gmpnp_budgeter* b = s->budgeter.get();
  Ctx c = s->c;
  c.EF = b->EF.p; c.status = b->status.p;   // the element pass writes nothing the solver reads
  hipLaunchKernelGGL((k_element<DIM, NF, false>), dim3(grid_for(s->t.nc, 64)), dim3(64), 0, s->stream, c);
  hipLaunchKernelGGL((k_budget_cells<DIM, NF>), dim3(b->nblk_c), dim3(kVecBlock), 0, s->stream, c, b->part_c.p);
  if (stern_on(s)) { int rc = stern_launch_residual(s, b->status.p); if (rc) return rc; }   // the Stern term at THIS u, for the row pass
  if (kinetics_on(s)) { int rc = kinetics_launch_residual(s, b->status.p); if (rc) return rc; }   // and the kinetic term of the species rows
  BudgetGeo g{b->wall_w.p, b->exit_w.p, b->exit_ptr.p, b->exit_col.p, b->exit_val.p, b->point_w.p};
  hipLaunchKernelGGL((k_budget_rows<DIM, NF>), dim3(b->nblk_r), dim3(kVecBlock), 0, s->stream, c, (const double*)b->EF.p, g, b->part_r.p);
  hipLaunchKernelGGL((k_budget_final<NF>), dim3(1), dim3(kVecBlock), 0, s->stream, (const double*)b->part_c.p, b->nblk_c, (const double*)b->part_r.p,
                     b->nblk_r, b->table.p);
  if (stern_on(s)) {   // the integrated Stern term: the potential row's wall (3D) / point (1D) entry, so that row still closes
    int rc = stern_launch_sum(s, b->table.p + (size_t)(NF - 1) * GMPNP_BUDGET_COLUMNS + (DIM == 3 ? GMPNP_BUDGET_WALL : GMPNP_BUDGET_POINT));
    if (rc) return rc;
  }
  if (kinetics_on(s)) {   // the integrated kinetic fluxes: added to the species rows' wall (3D) / point (1D) entries, so those rows still close
    int rc = kinetics_launch_sum(s, b->status.p, b->table.p); if (rc) return rc;
  }
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

int budget_launch_any(gmpnp_solver* s) {
  GMPNP_DISPATCH(s, return (budget_launch<DIM, NF>(s)));
  return GMPNP_OK;
}

}  // namespace

extern "C" {

int gmpnp_species_budget(gmpnp_solver* s, double* out) {
  if (!s || !out) return fail(GMPNP_ERR_INVALID, "species budget: NULL argument");
  int rc = budget_launch_any(s); if (rc) return rc;
  gmpnp_budgeter* b = s->budgeter.get();
  const size_t n = (size_t)s->nf * GMPNP_BUDGET_COLUMNS;
  HIP_TRY(hipMemcpyAsync(b->h_table, b->table.p, n * sizeof(double), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  std::memcpy(out, b->h_table, n * sizeof(double));
  return GMPNP_OK;
}

int gmpnp_group_species_budget(gmpnp_group* g, double* out) {
  if (!g || !out) return fail(GMPNP_ERR_INVALID, "species budget: NULL argument");
  if (g->ml_level) return fail(GMPNP_ERR_INVALID, "this group is a coarse level of a multilevel term");
  for (gmpnp_solver* s : g->dom) { int rc = budget_launch_any(s); if (rc) return rc; }
  gmpnp_solver* s0 = g->dom[0];
  const size_t n = (size_t)s0->nf * GMPNP_BUDGET_COLUMNS;
  // the ranks' owned-row tables summed over the group's transport, in pieces its staging holds (as the column select does)
  const size_t cap = g->peer ? (size_t)g->pa.red_cap : g->hosted ? g->h_stage_n : ~(size_t)0;
  for (size_t off = 0; off < n; off += cap) {
    const int m = (int)std::min(cap, n - off);
    int rc = group_allreduce(g, [off](gmpnp_solver* s) { return s->budgeter->table.p + off; }, m); if (rc) return rc;
  }
  for (gmpnp_solver* s : g->dom)
    HIP_TRY(hipMemcpyAsync(s->budgeter->h_table, s->budgeter->table.p, n * sizeof(double), hipMemcpyDeviceToHost, s0->stream));
  HIP_TRY(hipStreamSynchronize(s0->stream));
  { int rc = peer_check(g); if (rc) return rc; }
  for (gmpnp_solver* s : g->dom)   // every local rank holds the same bits
    if (std::memcmp(s->budgeter->h_table, s0->budgeter->h_table, n * sizeof(double)) != 0)
      return fail(GMPNP_ERR_HIP, "species budget: the ranks of this process hold different all-reduced tables");
  std::memcpy(out, s0->budgeter->h_table, n * sizeof(double));
  return GMPNP_OK;
}

}  // extern "C"
