// Transient sensitivities on the device: gmpnp_sensitivity_open / _step / _read / _columns / _set_columns / _close (include/gmpnp.h
// "transient sensitivities").
//
// The exact discrete forward sensitivity of a marched potential programme, one recursion per accepted step (J = K + inv_dt M, the
// backward-Euler time term linear in u_n):
//     J(u^{n+1}) s_k^{n+1} = -c_k(u^{n+1}) + inv_dt M s_k^n        (Dirichlet rows: 0)
//
//   k_galv_rhs / k_response_rhs / k_tan_columns      the columns c_k = dF/dtheta_k, by the electrode tangent's own kernels
//   k_sens_rhs        one lane per (chain column, field, vertex): -c_k + inv_dt (M s_k) with M the consistent P1 mass of a free species
//                     row (species_mass_1d: the entries towards I - 1, I, I + 1), written straight into level 0 of the multi-column
//                     chain's right-hand sides, [column][field][vertex] (what k_tan_extract does for the tangent); zero beyond the
//                     columns in use
//   k_bcr_forward_cols / k_bcr_tail_cols / k_bcr_backward_cols / k_tan_apply      the tangent's chain (tangent_chain<7, 2 | 8>) over
//                     right-hand-side levels of the sensitivities' own: a region of 8 columns and one of 2 per level, so that the
//                     chain of columns 9 and 10 leaves the right-hand sides of the first eight where gmpnp_sensitivity_columns reads
//                     them.  The solution replaces S.
//   k_sens_record     one workgroup, the columns one after the other: max |J s - rhs| and max |rhs| over all rows (J s by k_spmv_plain in
//                     front), the tangent's functionals of S (tan_functional_sums and block_sum: the statements and the order of
//                     k_tan_functional, so dD, dI_r and dp_boundary carry its bits), then lane 0 applies electrode_record_combine to
//                     the derivatives with the accumulators the device keeps (dD_prev, dQ, dQ_D) and writes the column's record: no host
//                     synchronisation, no copy, no floating-point atomics; the sums are picked out of the register array with constant
//                     indices.  `init`: gmpnp_sensitivity_open's launch, which only takes dD as dD_prev and zeroes dQ and dQ_D.
// A column's numbers never meet another column's: its records and S do not depend on which other columns are carried.
// The records' buffer is a RecordStream of width n (gmpnp_api.hip; rule: gmpnp_host_rules.h "record streams"), as the electrode trace's
// and the wall profile's are; the refusal of a handle goes through tangent_refusal.
// Included at the end of gmpnp_api.hip.
#pragma once

namespace gmpnp {

constexpr int kSensSingular = 2, kSensAssembly = 4;   // gmpnp_sensitivity_record_t.status beside kTangentNonFinite

struct SensTab {
  int32_t n, ndof, nv, init;
  int32_t param[kTangentMaxColumns];
  const double* S;                   // [n][ndof]
  const double* Jz;                  // [n][ndof] J s_k
  const double* b8;                  // level-0 right-hand sides of the chain of 8, [8][NF][nv]
  const double* b2;                  // ... of the chain of 2
  gmpnp_sensitivity_record_t* rec;   // [n]: the step's row
  ElectrodeAccum* acc;               // [kTangentMaxColumns]
  const int32_t* word;               // the solver's status word (the chain's pivots, the assembly)
  const int32_t* own;                // the word of the column launches
  double t, h;
};

// where column k's right-hand side sits: at most 2 columns run in the chain of 2, otherwise 0 ... 7 in the chain of 8 and 8, 9 in the chain of 2
__device__ __host__ inline const double* sens_rhs_of(const double* b8, const double* b2, int n, int k, int nf, int nv) {
  if (n <= 2) return b2 + (size_t)k * nf * nv;
  return k < 8 ? b8 + (size_t)k * nf * nv : b2 + (size_t)(k - 8) * nf * nv;
}

template <int NF>
__global__ __launch_bounds__(kVecBlock) void k_sens_rhs(const double* __restrict__ c, const double* __restrict__ S, const double* __restrict__ mass,
                                                        const uint8_t* __restrict__ bcflag, double* __restrict__ b0, int nv, int ndof, int col0,
                                                        int used, int M, double inv_dt) {
  GMPNP_RULE_NO_CONTRACT
  constexpr int NS = NF - 1;
  const int idx = blockIdx.x * kVecBlock + threadIdx.x;
  if (idx >= M * NF * nv) return;
  const int mf = idx / nv, I = idx - mf * nv, m = mf / NF, f = mf - m * NF;
  double v = 0.0;
  if (m < used) {
    const size_t row = (size_t)I * NF + f;
    const double* s = S + (size_t)(col0 + m) * ndof;
    v = -c[(size_t)(col0 + m) * ndof + row];
    if (f < NS && !bcflag[row]) {
      double ms = mass[(size_t)nv + I] * s[row];
      if (I > 0) ms = ms + mass[I] * s[row - NF];
      if (I + 1 < nv) ms = ms + mass[(size_t)2 * nv + I] * s[row + NF];
      v = v + inv_dt * ms;
    }
  }
  b0[idx] = v;
}

template <int DIM, int NF>
__global__ __launch_bounds__(kVecBlock) void k_sens_record(const Ctx c, const KinTab kt, const SternTab st, const int kinetics, const SensTab t) {
  GMPNP_RULE_NO_CONTRACT
  constexpr int R = GMPNP_MAX_SURFACE_REACTIONS, K = 3 + R;
  __shared__ double lds[4 * K];
  __shared__ double mx[2 * 4];
  const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
  for (int k = 0; k < t.n; ++k) {
    const int param = t.param[k];
    const double* z = t.S + (size_t)k * t.ndof;
    double rmax = 0.0, bmax = 0.0;
    bool wild = false;
    if (!t.init) {
      const double* Jz = t.Jz + (size_t)k * t.ndof;
      const double* b = sens_rhs_of(t.b8, t.b2, t.n, k, NF, t.nv);
      for (int idx = threadIdx.x; idx < t.ndof; idx += kVecBlock) {
        const int I = idx / NF, f = idx - I * NF;
        const double bi = b[(size_t)f * t.nv + I], v = Jz[idx] - bi, zi = z[idx];
        wild = wild || !rule_finite(v) || !rule_finite(zi);
        rmax = fmax(rmax, fabs(v)); bmax = fmax(bmax, fabs(bi));
      }
    }
    double v[K];
    tan_functional_sums<DIM, NF>(c, kt, st, kinetics, param, z, v);
    block_sum<K>(v, lds);
    double a = wild ? -1.0 : rmax, b = bmax;   // -1 marks a value that is not finite (every true maximum is >= 0)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double a2 = __shfl_xor(a, o), b2 = __shfl_xor(b, o);
      a = (a < 0.0 || a2 < 0.0) ? -1.0 : fmax(a, a2);
      b = fmax(b, b2);
    }
    if (ln == 0) { mx[wv] = a; mx[4 + wv] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
      ElectrodeAccum acc = t.acc[k];
      if (t.init) {
        acc.D_prev = v[0];
#pragma unroll
        for (int r = 0; r < R; ++r) acc.Q[r] = 0.0;
        acc.Q_D = 0.0;
        t.acc[k] = acc;
      } else {
        bool w2 = false;
        double ra = 0.0, rb = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) { w2 = w2 || mx[q] < 0.0; ra = fmax(ra, mx[q]); rb = fmax(rb, mx[4 + q]); }
        const double dI[R] = {kinetics ? v[1] : 0.0, kinetics ? v[2] : 0.0, kinetics ? v[3] : 0.0, kinetics ? v[4] : 0.0};
        const double d_dD_dt = electrode_record_combine(acc, t.h, v[0], dI);
        t.acc[k] = acc;
        gmpnp_sensitivity_record_t* o = t.rec + k;
        const double den = v[2 + R];
        const double dpb = den != 0.0 ? v[1 + R] / den : 0.0;
        bool fin = rule_finite(t.t) && rule_finite(t.h) && rule_finite(v[0]) && rule_finite(d_dD_dt) && rule_finite(acc.Q_D) && rule_finite(dpb);
        o->t = t.t; o->h = t.h; o->param = param; o->pad0_ = 0;
        o->dD = v[0]; o->d_dD_dt = d_dD_dt;
#pragma unroll
        for (int r = 0; r < R; ++r) { o->dI[r] = dI[r]; o->dQ[r] = acc.Q[r]; fin = fin && rule_finite(dI[r]) && rule_finite(acc.Q[r]); }
        o->dQ_D = acc.Q_D;
        o->dp_boundary = dpb;
        o->residual = w2 ? __longlong_as_double(0x7ff8000000000000ll) : (rb > 0.0 ? ra / rb : ra);
        const int32_t word = *t.word, own = *t.own;
        o->status = ((w2 || !fin) ? kTangentNonFinite : 0) | ((word & 2) ? kSensSingular : 0) | (((word | own) & (32 | 64)) ? kSensAssembly : 0);
        o->pad_ = 0;
      }
    }
    // (the next column's block_sum synchronises before it writes lds, and twice before mx is written again)
  }
}

}  // namespace gmpnp

namespace {

struct SensLevels { std::vector<TriCols> c8, c2; };

// the right-hand-side levels of the sensitivities: per level of the pyramid b, bi, x with 8 columns, then b, bi, x with 2
SensLevels sens_levels(gmpnp_solver* s) {
  SensLevels L;
  double* p = s->sensitizer->store.p;
  const size_t nf = (size_t)s->nf;
  for (const TriLevel& l : s->tri) {
    for (int M : {8, 2}) {
      TriCols c{};
      c.b = p; p += (size_t)M * nf * l.n;
      c.bi = p; p += (size_t)M * nf * l.n;
      c.x = p; p += (size_t)M * nf * l.n;
      (M == 8 ? L.c8 : L.c2).push_back(c);
    }
  }
  return L;
}

const char* sens_refusal(const gmpnp_solver* s) {
  if (s->dim != 1) return "1D handles only (3D needs the tetrahedron mass product and n band substitutions per step)";
  return tangent_refusal(s);
}

// right-hand side, elimination and application of one chain of M columns: columns col0 ... col0 + used - 1 of S
template <int NF, int M>
int sens_solve_chain(gmpnp_solver* s, double* S, const std::vector<TriCols>& cl, int col0, int used) {
  gmpnp_sensitizer* Z = s->sensitizer.get();
  const int nv = s->t.nv;
  hipLaunchKernelGGL((k_sens_rhs<NF>), dim3(grid_for(M * NF * nv, kVecBlock)), dim3(kVecBlock), 0, s->stream, (const double*)Z->c.p, (const double*)S,
                     (const double*)Z->mass.p, (const uint8_t*)s->c.bcflag, cl[0].b, nv, (int)s->ndof, col0, used, M, s->model.inv_dt);
  int rc = tangent_chain<NF, M>(s, cl); if (rc) return rc;
  hipLaunchKernelGGL((k_tan_apply<NF>), dim3(grid_for(used * s->ndof, kVecBlock)), dim3(kVecBlock), 0, s->stream, (const double*)cl[0].x, S, nv, (int)s->ndof,
                     col0, used);
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

SensTab sens_tab(gmpnp_solver* s, const SensLevels& L, const double* S, gmpnp_sensitivity_record_t* rec, int which) {
  gmpnp_sensitizer* Z = s->sensitizer.get();
  SensTab t{};
  t.n = Z->n; t.ndof = (int32_t)s->ndof; t.nv = s->t.nv;
  for (int k = 0; k < Z->n; ++k) t.param[k] = Z->param[k];
  t.S = S; t.Jz = Z->Jz.p; t.b8 = L.c8[0].b; t.b2 = L.c2[0].b;
  t.rec = rec; t.acc = Z->acc.p + (size_t)which * kTangentMaxColumns;
  t.word = s->status.p; t.own = Z->status.p;
  return t;
}

// the launches of one step on the sensitivities `S`, into the row `rec` of the records with the accumulators acc[which]: nothing waits
int sens_launch(gmpnp_solver* s, double t, double h, double* S, gmpnp_sensitivity_record_t* rec, int which) {
  constexpr int DIM = 1, NF = 7;
  gmpnp_sensitizer* Z = s->sensitizer.get();
  const size_t ndof = (size_t)s->ndof;
  const int n = Z->n;
  tangent_drop(s);
  // F and J at the current u, as gmpnp_electrode_tangent assembles them (residual() without its synchronisation)
  HIP_TRY(hipMemsetAsync(s->status.p, 0, sizeof(int32_t), s->stream));
  HIP_TRY(hipMemsetAsync(Z->status.p, 0, sizeof(int32_t), s->stream));
  int rc = launch_element<DIM, NF>(s, true); if (rc) return rc;
  rc = stern_launch_residual(s, s->status.p); if (rc) return rc;
  const int kin = kinetics_on(s) ? 1 : 0;
  if (kin) { rc = kinetics_launch_residual(s, s->status.p); if (rc) return rc; }
  rc = launch_res_gather<DIM, NF>(s); if (rc) return rc;
  rc = launch_jac_gather<DIM, NF>(s); if (rc) return rc;
  s->jacobian_valid = true; s->precond_valid = false;
  // the columns
  TanTab tt{};
  tt.n = n; tt.ndof = (int32_t)ndof;
  int col_pM = -1;
  for (int k = 0; k < n; ++k) { tt.param[k] = Z->param[k]; if (Z->param[k] == 0) col_pM = k; }
  tt.c = Z->c.p; tt.z = S; tt.Jz = Z->Jz.p; tt.out = nullptr;
  const SternTab st = stern_tab(s, Z->status.p);
  KinTab kt{};
  if (kin) kt = kinetics_tab(s, Z->status.p);
  HIP_TRY(hipMemsetAsync(Z->c.p, 0, (size_t)n * ndof * sizeof(double), s->stream));
  if (col_pM >= 0) {
    double* b = Z->c.p + (size_t)col_pM * ndof;
    if (kin) hipLaunchKernelGGL((k_galv_rhs<DIM, NF>), dim3(grid_for(kt.n_nodes, kVecBlock)), dim3(kVecBlock), 0, s->stream, s->c, kt, st, 1, b);
    else hipLaunchKernelGGL((k_response_rhs<DIM, NF>), dim3(grid_for(st.n_nodes, kVecBlock)), dim3(kVecBlock), 0, s->stream, s->c, st, b);
  }
  hipLaunchKernelGGL((k_tan_columns<DIM, NF>), dim3(grid_for(st.n_nodes, kVecBlock)), dim3(kVecBlock), 0, s->stream, s->c, kt, st, kin, tt);
  HIP_TRY(hipGetLastError());
  // the solves: the matrix levels once, then the chain(s)
  const SensLevels L = sens_levels(s);
  hipLaunchKernelGGL((k_tri_extract<NF>), dim3(grid_for(s->t.nv * NF * NF, kVecBlock)), dim3(kVecBlock), 0, s->stream, s->c, s->tri[0], s->tri_kpos.p,
                     (const double*)Z->c.p);
  if (n <= 2) rc = sens_solve_chain<NF, 2>(s, S, L.c2, 0, n);
  else {
    rc = sens_solve_chain<NF, 8>(s, S, L.c8, 0, std::min(n, 8));
    if (!rc && n > 8) rc = sens_solve_chain<NF, 2>(s, S, L.c2, 8, n - 8);
  }
  if (rc) return rc;
  for (int k = 0; k < n; ++k)
    hipLaunchKernelGGL((k_spmv_plain<NF>), dim3(s->t.own_ntiles), dim3(kKrylovThreads), 0, s->stream, s->c, (const double*)(S + (size_t)k * ndof),
                       Z->Jz.p + (size_t)k * ndof);
  SensTab t_ = sens_tab(s, L, S, rec, which);
  t_.t = t; t_.h = h; t_.init = 0;
  hipLaunchKernelGGL((k_sens_record<DIM, NF>), dim3(1), dim3(kVecBlock), 0, s->stream, s->c, kt, st, kin, t_);
  HIP_TRY(hipGetLastError());
  Z->stepped = true;
  return GMPNP_OK;
}

bool sensitivity_is_open(const gmpnp_solver* s) { return s->sensitizer && s->sensitizer->rec.open; }

// gmpnp_time_kernel 31: the second S, the row behind the buffer and the second set of accumulators, so the march stays what it was
int sensitivity_time_step(gmpnp_solver* s) {
  if (const char* why = sens_refusal(s)) return fail(GMPNP_ERR_INVALID, std::string("sensitivities: ") + why);
  if (!s->sensitizer->S_hook.p) HIP_TRY(s->sensitizer->S_hook.alloc((size_t)kTangentMaxColumns * s->ndof));   // (zeroed)
  return sens_launch(s, 0.0, 1.0, s->sensitizer->S_hook.p, s->sensitizer->rec.hook_row(), 1);
}

}  // namespace

extern "C" {

int gmpnp_sensitivity_open(gmpnp_solver* s, int32_t n, const int32_t* param, int32_t start, int32_t capacity) {
  if (!s || !param) return fail(GMPNP_ERR_INVALID, "sensitivities: NULL argument");
  if (const char* why = sens_refusal(s)) return fail(GMPNP_ERR_INVALID, std::string("sensitivities: ") + why);
  if (!tangent_count_valid(n)) return fail(GMPNP_ERR_INVALID, "sensitivities: n must lie in 1 ... 10");
  const int nr = kinetics_on(s) ? s->kineticist->opt.n_reactions : 0;
  for (int k = 0; k < n; ++k) {
    const int kind = tangent_param_kind(param[k]);
    if (kind < 0) return fail(GMPNP_ERR_INVALID, "sensitivities: unknown parameter (0 = p_M, 16 + r = ln k_r, 32 + r = alpha_r, 48 = ln lam)");
    if ((kind == 1 || kind == 2) && nr == 0) return fail(GMPNP_ERR_INVALID, "sensitivities: a kinetic parameter needs the surface kinetics on (gmpnp_set_kinetics)");
    if (!tangent_param_valid(param[k], nr)) return fail(GMPNP_ERR_INVALID, "sensitivities: a kinetic parameter names a reaction >= n_reactions");
    for (int q = 0; q < k; ++q)
      if (param[q] == param[k]) return fail(GMPNP_ERR_INVALID, "sensitivities: a parameter is repeated");
  }
  if (capacity < 1) return fail(GMPNP_ERR_INVALID, "sensitivities: capacity must be at least 1");
  if (start < 0 || start > 2) return fail(GMPNP_ERR_INVALID, "sensitivities: start is 0 (S = 0), 1 (S = the tangent's columns) or 2 (S and the accumulators stay)");
  gmpnp_sensitizer* Z = s->sensitizer.get();
  if (start == 2) {
    bool same = Z && Z->n == n;
    for (int k = 0; same && k < n; ++k) same = Z->param[k] == param[k];
    if (!same) return fail(GMPNP_ERR_INVALID, "sensitivities: start = 2 goes on with the columns of the open before (the same n and param)");
  }
  const gmpnp_tangenter* T = s->tangenter.get();
  int at[kTangentMaxColumns] = {};
  if (start == 1) {
    if (!T || !T->cols_fresh)
      return fail(GMPNP_ERR_INVALID, "sensitivities: start = 1 needs a tangent computed at the present state, potential and options (gmpnp_electrode_tangent)");
    for (int k = 0; k < n; ++k) {
      at[k] = -1;
      for (int q = 0; q < T->last_n; ++q) at[k] = (T->param[q] == param[k]) ? q : at[k];
      if (at[k] < 0) return fail(GMPNP_ERR_INVALID, "sensitivities: a parameter is not among those of the last gmpnp_electrode_tangent call");
      if (T->col_status[at[k]] != 0) return fail(GMPNP_ERR_INVALID, "sensitivities: a requested column of the last gmpnp_electrode_tangent call is not finite");
    }
  }
  HIP_TRY(hipSetDevice(s->opts.device_id));
  const size_t ndof = (size_t)s->ndof;
  if (!Z) {
    std::unique_ptr<gmpnp_sensitizer> N(new gmpnp_sensitizer);
    HIP_TRY(N->c.alloc(kTangentMaxColumns * ndof)); HIP_TRY(N->Jz.alloc(kTangentMaxColumns * ndof));
    HIP_TRY(N->S.alloc(kTangentMaxColumns * ndof));   // (S_hook: by the first hook call)
    HIP_TRY(N->mass.upload(species_mass_1d(s)));
    size_t total = 0;
    for (const TriLevel& l : s->tri) total += (size_t)3 * (8 + 2) * s->nf * l.n;
    HIP_TRY(N->store.alloc(total));
    HIP_TRY(N->acc.alloc(2 * kTangentMaxColumns)); HIP_TRY(N->status.alloc(1));
    s->sensitizer = std::move(N);
    Z = s->sensitizer.get();
  }
  Z->rec.close();
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (int rc = Z->rec.reserve(capacity, n, s->stream)) return rc;
  if (start == 2) { Z->rec.open = true; return GMPNP_OK; }
  Z->n = n;
  for (int k = 0; k < n; ++k) Z->param[k] = param[k];
  Z->stepped = false;
  HIP_TRY(hipMemsetAsync(Z->S.p, 0, kTangentMaxColumns * ndof * sizeof(double), s->stream));
  if (Z->S_hook.p) HIP_TRY(hipMemsetAsync(Z->S_hook.p, 0, kTangentMaxColumns * ndof * sizeof(double), s->stream));
  HIP_TRY(hipMemsetAsync(Z->acc.p, 0, 2 * kTangentMaxColumns * sizeof(ElectrodeAccum), s->stream));
  if (start == 1)
    for (int k = 0; k < n; ++k)
      HIP_TRY(hipMemcpyAsync(Z->S.p + (size_t)k * ndof, T->z.p + (size_t)at[k] * ndof, ndof * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
  // dD of S at the current u and options becomes dD_prev
  {
    const int kin = kinetics_on(s) ? 1 : 0;
    HIP_TRY(hipMemsetAsync(Z->status.p, 0, sizeof(int32_t), s->stream));
    const SternTab st = stern_tab(s, Z->status.p);
    KinTab kt{};
    if (kin) kt = kinetics_tab(s, Z->status.p);
    SensTab t_ = sens_tab(s, sens_levels(s), Z->S.p, Z->rec.row(0), 0);
    t_.t = 0.0; t_.h = 1.0; t_.init = 1;
    hipLaunchKernelGGL((k_sens_record<1, 7>), dim3(1), dim3(kVecBlock), 0, s->stream, s->c, kt, st, kin, t_);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipStreamSynchronize(s->stream));
  Z->rec.open = true;
  return GMPNP_OK;
}

int gmpnp_sensitivity_step(gmpnp_solver* s, double t, double h) {
  if (!s) return fail(GMPNP_ERR_INVALID, "sensitivities: NULL argument");
  if (const char* why = sens_refusal(s)) return fail(GMPNP_ERR_INVALID, std::string("sensitivities: ") + why);
  if (!sensitivity_is_open(s)) return fail(GMPNP_ERR_INVALID, kSensNouns.not_open());
  if (!record_step_valid(t, h)) return fail(GMPNP_ERR_INVALID, "sensitivities: t finite, h finite and > 0");
  gmpnp_sensitizer* Z = s->sensitizer.get();
  const int nr = kinetics_on(s) ? s->kineticist->opt.n_reactions : 0;
  for (int k = 0; k < Z->n; ++k)
    if (!tangent_param_valid(Z->param[k], nr)) return fail(GMPNP_ERR_INVALID, "sensitivities: a kinetic parameter of the open buffer names a reaction the kinetics no longer hold");
  if (Z->rec.full()) return Z->rec.refuse_full();
  HIP_TRY(hipSetDevice(s->opts.device_id));
  int rc = sens_launch(s, t, h, Z->S.p, Z->rec.row(Z->rec.count), 0); if (rc) return rc;
  Z->rec.count += 1;
  return GMPNP_OK;
}

int gmpnp_sensitivity_read(gmpnp_solver* s, int32_t first, int32_t n_steps, gmpnp_sensitivity_record_t* out) {
  if (!s || !out) return fail(GMPNP_ERR_INVALID, "sensitivities: NULL argument");
  if (!sensitivity_is_open(s)) return fail(GMPNP_ERR_INVALID, kSensNouns.not_open());
  HIP_TRY(hipSetDevice(s->opts.device_id));
  return s->sensitizer->rec.read(first, n_steps, out, s->stream);
}

int gmpnp_sensitivity_columns(gmpnp_solver* s, int32_t which, double* out) {
  if (!s || !out) return fail(GMPNP_ERR_INVALID, "sensitivities: NULL argument");
  if (!sensitivity_is_open(s)) return fail(GMPNP_ERR_INVALID, kSensNouns.not_open());
  if (which != 0 && which != 1) return fail(GMPNP_ERR_INVALID, "sensitivities: which is 0 (S) or 1 (the right-hand sides of the last step)");
  gmpnp_sensitizer* Z = s->sensitizer.get();
  if (which == 1 && !Z->stepped) return fail(GMPNP_ERR_INVALID, "sensitivities: no step has been made since the buffer was opened");
  HIP_TRY(hipSetDevice(s->opts.device_id));
  const size_t ndof = (size_t)s->ndof;
  const int nv = s->t.nv, nf = s->nf;
  if (which == 0) {
    for (int k = 0; k < Z->n; ++k) { int rc = download_vec(s, Z->S.p + (size_t)k * ndof, out + (size_t)k * ndof); if (rc) return rc; }
    return GMPNP_OK;
  }
  const SensLevels L = sens_levels(s);
  std::vector<double> b(ndof);
  for (int k = 0; k < Z->n; ++k) {   // [field][vertex] -> file order
    HIP_TRY(hipMemcpyAsync(b.data(), sens_rhs_of(L.c8[0].b, L.c2[0].b, Z->n, k, nf, nv), ndof * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    for (int I = 0; I < nv; ++I)
      for (int f = 0; f < nf; ++f) out[(size_t)k * ndof + (size_t)s->t.perm[I] * nf + f] = b[(size_t)f * nv + I];
  }
  return GMPNP_OK;
}

int gmpnp_sensitivity_set_columns(gmpnp_solver* s, const double* in) {
  if (!s || !in) return fail(GMPNP_ERR_INVALID, "sensitivities: NULL argument");
  if (!sensitivity_is_open(s)) return fail(GMPNP_ERR_INVALID, kSensNouns.not_open());
  gmpnp_sensitizer* Z = s->sensitizer.get();
  HIP_TRY(hipSetDevice(s->opts.device_id));
  for (int k = 0; k < Z->n; ++k) { int rc = upload_vec(s, in + (size_t)k * s->ndof, Z->S.p + (size_t)k * s->ndof); if (rc) return rc; }
  return GMPNP_OK;
}

int gmpnp_sensitivity_close(gmpnp_solver* s) {
  if (!s) return fail(GMPNP_ERR_INVALID, "sensitivities: NULL argument");
  if (!sensitivity_is_open(s)) return fail(GMPNP_ERR_INVALID, kSensNouns.not_open());
  s->sensitizer->rec.close();
  return GMPNP_OK;
}

}  // extern "C"
