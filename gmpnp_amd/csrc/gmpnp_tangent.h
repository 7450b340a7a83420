// Electrode tangent on the device: gmpnp_electrode_tangent / gmpnp_electrode_advance / gmpnp_parameter_advance / gmpnp_tangent_columns /
// gmpnp_get_electrode_options (include/gmpnp.h), rule in
// gmpnp_host_rules.h (tangent_param_kind, tangent_rate_explicit, tangent_stern_explicit, tangent_current_term).
//
// At the handle's current u, p_M and model.inv_dt, for up to ten parameters theta_k (p_M, ln k_r, alpha_r, ln lam):
//     J z_k = -c_k,  c_k = dF/dtheta_k        dD = dD/dtheta + (dD/du).z        dI_r = dI_r/dtheta + (dI_r/du).z
//
//   k_galv_rhs / k_response_rhs   the p_M column: the galvanostat's b, by the galvanostat's own kernels (kinetics on / Stern alone)
//   k_tan_columns     one lane per boundary node (the Stern nodes and the kinetics' nodes are one ascending list): the node's rates once,
//                     then per column the species rows (ln k_r: w nu[r][i] rate_r, alpha_r: -w nu[r][i] rate_r eta_r) or the potential
//                     row (ln lam: minus the Stern term, its facets in list order).  The Dirichlet flags are read at run time (such a
//                     row: 0); every other entry of a column is zero (the columns are cleared in front).
//   k_tan_extract / k_bcr_forward_cols / k_bcr_tail_cols / k_bcr_backward_cols / k_tan_apply
//                     1D: block cyclic reduction of J with M right-hand sides at once, M = 2 or 8.  The augmented row of the block
//                     elimination is [D | L | U | b_1 ... b_M]; the matrix levels are the handle's own (tri_solve's storage), the
//                     levels of b, bi and x are the tangent's, [column][field][row].  The pivots depend on D alone and every column
//                     sees the operations tri_group_solve applies to its one right-hand side, in the same order: column k carries the
//                     bits of gmpnp_linear_solve(-c_k, GMPNP_LINEAR_BLOCK_TRIDIAGONAL), whatever the other columns hold.  n <= 2: one
//                     M = 2 chain; n <= 8: one M = 8 chain; n = 9, 10: an M = 8 chain and an M = 2 chain.
//   k_tan_functional  one workgroup per column: max |J z + c| and max |c| over all rows (J z by k_spmv_plain in front), dD, dI_r and the
//                     weighted mean of z's potential entry from the boundary nodes (block_sum, fixed order), the column's status word.
//   k_tan_scale / k_step_limit / k_tan_advance     gmpnp_electrode_advance: u += alpha dp z_0 without FMA contraction; with tau != 0 the
//                     step limiter's partials of the direction -dp z_0 come first and every workgroup re-reduces them to alpha.
//   k_par_advance     gmpnp_parameter_advance: the same in several columns at once (pointers and coefficients by value), both passes: the
//                     direction -(dtheta_0 z_0 + ...) for the step limiter, and u += (alpha dtheta_0) z_0 + ... with k_tan_advance's reduction.
// Every sum is a gather in a fixed order (no floating-point atomics): two calls on one state give equal bits.  The reactant's entry and
// the rate of a column's reaction are picked by selects out of unrolled loops, not by indexing a register array.
// Included at the end of gmpnp_api.hip.
#pragma once

namespace gmpnp {

// what k_tan_functional leaves per column
struct TanOut {
  double dD;
  double dI[GMPNP_MAX_SURFACE_REACTIONS];
  double dp_boundary, residual;
  int32_t status, pad_;
};

struct TanTab {
  int32_t n, ndof;
  int32_t param[kTangentMaxColumns];
  double* c;          // [n][ndof] dF/dtheta_k, internal order
  const double* z;    // [n][ndof] the tangents
  const double* Jz;   // [n][ndof] J z_k
  TanOut* out;        // [n]
};

// the right-hand sides of one level: [M][NF][n] each, beside the TriLevel of the same index
struct TriCols { double *b, *bi, *x; };

// tri_group_solve with M right-hand sides in the place of one: W[0..NF) = Dm row, W[NF..3NF) = Lm | Um, W[3NF..3NF+M) = the columns
template <int NF, int M>
__device__ inline bool tri_group_solve_cols(const TriLevel& lv, const TriCols& cl, int j, bool on, int r, double (&W)[3 * NF + M]) {
  constexpr int NC = 3 * NF + M;
  static_assert(NF <= 8, "one lane per row of an 8-lane group");
  const bool rowon = on && r < NF;
  const int jc = on ? j : 0, rc = r < NF ? r : 0;
#pragma unroll
  for (int cI = 0; cI < NF; ++cI) {
    const size_t off = (size_t)(rc * NF + cI) * lv.n + jc;
    W[cI] = lv.D[off]; W[NF + cI] = lv.L[off]; W[2 * NF + cI] = lv.U[off];
  }
#pragma unroll
  for (int m = 0; m < M; ++m) W[3 * NF + m] = cl.b[(size_t)(m * NF + rc) * lv.n + jc];
  if (!rowon) {
#pragma unroll
    for (int cI = 0; cI < NC; ++cI) W[cI] = (cI == r && r < NF) ? 1.0 : 0.0;
  }
  bool bad = false, used = r >= NF;
  int home = r;
#pragma unroll
  for (int k = 0; k < NF; ++k) {
    unsigned long long key = used ? 0ull : (((unsigned long long)__double_as_longlong(fabs(W[k])) & ~7ull) | (unsigned long long)(7 - r));
#pragma unroll
    for (int o = 4; o > 0; o >>= 1) {
      const int olo = __shfl_xor((int)(unsigned)key, o, 8), ohi = __shfl_xor((int)(unsigned)(key >> 32), o, 8);
      const unsigned long long ok_ = ((unsigned long long)(unsigned)ohi << 32) | (unsigned)olo;
      key = ok_ > key ? ok_ : key;
    }
    const int p = 7 - (int)(key & 7ull);
    bad |= (key >> 3) == 0ull;
    const double ip = 1.0 / __shfl(W[k], p, 8);
    const double f = (r == p) ? 0.0 : W[k] * ip;
#pragma unroll
    for (int cI = k + 1; cI < NC; ++cI) {
      const double from_p = __shfl(W[cI], p, 8);
      W[cI] = (r == p) ? W[cI] * ip : W[cI] - f * from_p;
    }
    W[k] = (r == p) ? 1.0 : 0.0;
    used = used || (r == p);
    home = (r == k) ? p : home;
  }
#pragma unroll
  for (int cI = NF; cI < NC; ++cI) W[cI] = __shfl(W[cI], home, 8);
  return !(on && bad);
}

// bcr_forward_row with M right-hand sides
template <int NF, int M>
__device__ __forceinline__ void bcr_forward_row_cols(const TriLevel& lo, const TriLevel& hi, const TriCols& clo, const TriCols& chi, int32_t* status,
                                                     const int ih_raw) {
  constexpr int NC = 3 * NF + M;
  const int t = threadIdx.x;
  const int side = (t >> 3) & 1, r = t & 7;
  const bool rowok = ih_raw < hi.n;
  const int ih = rowok ? ih_raw : 0, i = 2 * ih;
  const int j = side == 0 ? i - 1 : i + 1;
  const bool on = rowok && j >= 0 && j < lo.n;
  const int rc = r < NF ? r : 0;
  double W[NC];
  double cr[NF], dr[NF], br[M];
  const double* C = side == 0 ? lo.L : lo.U;
#pragma unroll
  for (int mI = 0; mI < NF; ++mI) { cr[mI] = C[(size_t)(rc * NF + mI) * lo.n + i]; dr[mI] = lo.D[(size_t)(rc * NF + mI) * lo.n + i]; }
#pragma unroll
  for (int m = 0; m < M; ++m) br[m] = clo.b[(size_t)(m * NF + rc) * lo.n + i];
  const bool ok = tri_group_solve_cols<NF, M>(lo, clo, j, on, r, W);
  double pL[NF], pU[NF], pb[M];
#pragma unroll
  for (int cI = 0; cI < NF; ++cI) { pL[cI] = 0.0; pU[cI] = 0.0; }
#pragma unroll
  for (int m = 0; m < M; ++m) pb[m] = 0.0;
#pragma unroll
  for (int mI = 0; mI < NF; ++mI) {
    const double cm = on ? cr[mI] : 0.0;
#pragma unroll
    for (int cI = 0; cI < NF; ++cI) { pL[cI] += cm * __shfl(W[NF + cI], mI, 8); pU[cI] += cm * __shfl(W[2 * NF + cI], mI, 8); }
#pragma unroll
    for (int m = 0; m < M; ++m) pb[m] += cm * __shfl(W[3 * NF + m], mI, 8);
  }
  double dmine[NF], dother[NF], pbo[M];
#pragma unroll
  for (int cI = 0; cI < NF; ++cI) { dmine[cI] = side == 0 ? pU[cI] : pL[cI]; dother[cI] = __shfl_xor(dmine[cI], 8, 16); }
#pragma unroll
  for (int m = 0; m < M; ++m) pbo[m] = __shfl_xor(pb[m], 8, 16);
  if (rowok && r < NF) {
    if (side == 0) {
#pragma unroll
      for (int cI = 0; cI < NF; ++cI) {
        hi.L[(size_t)(r * NF + cI) * hi.n + ih] = -pL[cI];
        hi.D[(size_t)(r * NF + cI) * hi.n + ih] = (dr[cI] - dmine[cI]) - dother[cI];
      }
    } else {
#pragma unroll
      for (int cI = 0; cI < NF; ++cI) hi.U[(size_t)(r * NF + cI) * hi.n + ih] = -pU[cI];
#pragma unroll
      for (int m = 0; m < M; ++m) chi.b[(size_t)(m * NF + r) * hi.n + ih] = (br[m] - pbo[m]) - pb[m];
      if (on) {
#pragma unroll
        for (int cI = 0; cI < NF; ++cI) {
          lo.Li[(size_t)(r * NF + cI) * lo.n + j] = W[NF + cI];
          lo.Ui[(size_t)(r * NF + cI) * lo.n + j] = W[2 * NF + cI];
        }
#pragma unroll
        for (int m = 0; m < M; ++m) clo.bi[(size_t)(m * NF + r) * lo.n + j] = W[3 * NF + m];
      }
    }
  }
  if (!ok) atomicOr(status, 2);
}
template <int NF, int M>
__global__ __launch_bounds__(64) void k_bcr_forward_cols(TriLevel lo, TriLevel hi, TriCols clo, TriCols chi, int32_t* status) {
  bcr_forward_row_cols<NF, M>(lo, hi, clo, chi, status, blockIdx.x * 4 + ((int)threadIdx.x >> 4));
}

template <int NF, int M>
__device__ __forceinline__ void bcr_top_row_cols(const TriLevel& top, const TriCols& ct, int32_t* status) {
  constexpr int NC = 3 * NF + M;
  const int t = threadIdx.x, r = t & 7;
  double W[NC];
  const bool ok = tri_group_solve_cols<NF, M>(top, ct, 0, t < 8, r, W);
  if (t < NF) {
#pragma unroll
    for (int m = 0; m < M; ++m) ct.x[m * NF + t] = W[3 * NF + m];
  }
  if (!ok) atomicOr(status, 2);
}

// bcr_backward_entry per (column, field, row): q in [0, M NF n)
template <int NF, int M>
__device__ __forceinline__ void bcr_backward_entry_cols(const TriLevel& lo, const TriLevel& hi, const TriCols& clo, const TriCols& chi, const int q) {
  if (q >= lo.n * NF * M) return;
  const int mr = q / lo.n, j = q - mr * lo.n;   // j fastest
  const int m = mr / NF, r = mr - m * NF;
  const double* xh = chi.x + (size_t)m * NF * hi.n;
  double* xl_ = clo.x + (size_t)m * NF * lo.n;
  if ((j & 1) == 0) { xl_[(size_t)r * lo.n + j] = xh[(size_t)r * hi.n + (j >> 1)]; return; }
  const bool has_r = (j + 1 < lo.n);
  double li[NF], ui[NF], xl[NF], xr[NF];
#pragma unroll
  for (int cI = 0; cI < NF; ++cI) {
    li[cI] = lo.Li[(size_t)(r * NF + cI) * lo.n + j]; ui[cI] = lo.Ui[(size_t)(r * NF + cI) * lo.n + j];
    xl[cI] = xh[(size_t)cI * hi.n + ((j - 1) >> 1)];
    xr[cI] = has_r ? xh[(size_t)cI * hi.n + ((j + 1) >> 1)] : 0.0;
  }
  double sacc = clo.bi[(size_t)(m * NF + r) * lo.n + j];
#pragma unroll
  for (int cI = 0; cI < NF; ++cI) sacc -= li[cI] * xl[cI] + ui[cI] * xr[cI];
  xl_[(size_t)r * lo.n + j] = sacc;
}
template <int NF, int M>
__global__ __launch_bounds__(kVecBlock) void k_bcr_backward_cols(TriLevel lo, TriLevel hi, TriCols clo, TriCols chi) {
  bcr_backward_entry_cols<NF, M>(lo, hi, clo, chi, blockIdx.x * kVecBlock + threadIdx.x);
}

struct TriTailCols { TriLevel lv[kBcrTailLevels + 1]; TriCols cl[kBcrTailLevels + 1]; int nlev; };
template <int NF, int M>
__global__ __launch_bounds__(kBcrTailThreads) void k_bcr_tail_cols(const TriTailCols tt, int32_t* status) {
  const int t = threadIdx.x;
  for (int l = 0; l + 1 < tt.nlev; ++l) {
    for (int ih0 = 0; ih0 < tt.lv[l + 1].n; ih0 += kBcrTailThreads / 16)
      bcr_forward_row_cols<NF, M>(tt.lv[l], tt.lv[l + 1], tt.cl[l], tt.cl[l + 1], status, ih0 + (t >> 4));
    __syncthreads();
  }
  if (t < 64) bcr_top_row_cols<NF, M>(tt.lv[tt.nlev - 1], tt.cl[tt.nlev - 1], status);
  __syncthreads();
  for (int l = tt.nlev - 2; l >= 0; --l) {
    for (int q = t; q < tt.lv[l].n * NF * M; q += kBcrTailThreads) bcr_backward_entry_cols<NF, M>(tt.lv[l], tt.lv[l + 1], tt.cl[l], tt.cl[l + 1], q);
    __syncthreads();
  }
}

// level-0 right-hand sides: column m of the chain = -c[col0 + m] (zero beyond the columns in use), [m][field][vertex]
template <int NF>
__global__ __launch_bounds__(kVecBlock) void k_tan_extract(const double* __restrict__ c, double* __restrict__ b0, int nv, int ndof, int col0, int used, int M) {
  const int idx = blockIdx.x * kVecBlock + threadIdx.x;
  if (idx >= M * NF * nv) return;
  const int mf = idx / nv, I = idx - mf * nv, m = mf / NF, f = mf - m * NF;
  b0[idx] = m < used ? -c[(size_t)(col0 + m) * ndof + (size_t)I * NF + f] : 0.0;
}
// z[col0 + m][I NF + f] = x[m][f][I] (tri_apply's 0 + 1 x)
template <int NF>
__global__ __launch_bounds__(kVecBlock) void k_tan_apply(const double* __restrict__ x0, double* __restrict__ z, int nv, int ndof, int col0, int used) {
  const int idx = blockIdx.x * kVecBlock + threadIdx.x;
  if (idx >= used * ndof) return;
  const int m = idx / ndof, r = idx - m * ndof, I = r / NF, f = r - I * NF;
  z[(size_t)(col0 + m) * ndof + r] = 0.0 + x0[(size_t)(m * NF + f) * nv + I];
}

template <int DIM, int NF>
__global__ __launch_bounds__(kVecBlock) void k_tan_columns(const Ctx c, const KinTab kt, const SternTab st, const int kinetics, const TanTab t) {
  GMPNP_RULE_NO_CONTRACT
  constexpr int NS = NF - 1;
  const int n = blockIdx.x * kVecBlock + threadIdx.x;
  if (n >= st.n_nodes) return;
  const size_t row0 = (size_t)st.node[n] * NF;
  double uu[NF];
#pragma unroll
  for (int j = 0; j < NF; ++j) uu[j] = c.u[row0 + j];
  KinRate R[GMPNP_MAX_SURFACE_REACTIONS];
#pragma unroll
  for (int r = 0; r < GMPNP_MAX_SURFACE_REACTIONS; ++r) R[r] = KinRate{0.0, 0.0, 0.0, 1};
  if (kinetics) kinetics_rates<NF>(kt, uu, R);
  for (int k = 0; k < t.n; ++k) {
    const int param = t.param[k], kind = tangent_param_kind(param);
    double* col = t.c + (size_t)k * t.ndof;
    if (kind == 1 || kind == 2) {
      const gmpnp_kinetics_t* o = kt.opt;
      const int r = tangent_param_reaction(param);
      double rate = 0.0, d_p = 0.0;
#pragma unroll
      for (int q = 0; q < GMPNP_MAX_SURFACE_REACTIONS; ++q) { rate = (q == r) ? R[q].rate : rate; d_p = (q == r) ? R[q].d_p : d_p; }
      const double eta = o->p_electrode - uu[NS] - o->p_eq[r];
      const double e = tangent_rate_explicit(param, r, rate, d_p, eta);
      const double w = kt.w[n];
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        const double nu = o->nu[r][i];
        col[row0 + i] = (nu != 0.0 && !c.bcflag[row0 + i]) ? w * (nu * e) : 0.0;
      }
    } else if (kind == 3) {
      double term = 0.0;
      if (!c.bcflag[row0 + NS]) {
        for (int q = st.nf_ptr[n]; q < st.nf_ptr[n + 1]; ++q) {
          const int ent = st.nf_ent[q];
          const SternFacet<DIM, NF> F(c, st, ent >> 2);
          term += F.G.g * F.w(st, ent & 3) / st.lam;
        }
      }
      col[row0 + NS] = -term;
    }
  }
}

// the boundary sums of one column's functionals, each lane its nodes n = lane, lane + 256, ...: v[0] = dD, v[1 + r] = dI_r, then the
// weighted sum of z's potential entry and the sum of the weights (k_tan_functional and gmpnp_sensitivity.h's k_sens_record add the lanes
// with block_sum)
template <int DIM, int NF>
__device__ __forceinline__ void tan_functional_sums(const Ctx& c, const KinTab& kt, const SternTab& st, const int kinetics, const int param,
                                                    const double* __restrict__ z, double (&v)[3 + GMPNP_MAX_SURFACE_REACTIONS]) {
  GMPNP_RULE_NO_CONTRACT
  constexpr int NS = NF - 1, K = 3 + GMPNP_MAX_SURFACE_REACTIONS, FN = SternFacet<DIM, NF>::FN;
#pragma unroll
  for (int q = 0; q < K; ++q) v[q] = 0.0;
  const gmpnp_model_t* m = c.model;
  for (int n = threadIdx.x; n < st.n_nodes; n += kVecBlock) {
    const size_t row0 = (size_t)st.node[n] * NF;
    double zz[NF];
#pragma unroll
    for (int j = 0; j < NF; ++j) zz[j] = z[row0 + j];
    double wn = 0.0, dd = 0.0;
    for (int q = st.nf_ptr[n]; q < st.nf_ptr[n + 1]; ++q) {
      const int ent = st.nf_ent[q], f = ent >> 2, a = ent & 3;
      const SternFacet<DIM, NF> F(c, st, f);
      const double share = DIM == 3 ? F.area / 3.0 : 1.0;
      wn += share;
      if (c.bcflag[row0 + NS]) continue;
      const double wa = F.w(st, a);
      const double slope = F.G.g * share / st.lam, term = F.G.g * wa / st.lam;
      double acc = tangent_stern_explicit(param, slope, term);
      // the Stern row of J applied to z: the facet's nodes b
#pragma unroll
      for (int b = 0; b < FN; ++b) {
        const size_t rb = (size_t)st.fnodes[f * FN + b] * NF;
        double se = 0.0;
        for (int j = 0; j < NS; ++j) se += m->epsc[j] * z[rb + j];
        acc += F.G.dg * (se / FN) * wa / st.lam - F.G.g * F.mass(a, b) / st.lam * z[rb + NS];
      }
      dd += acc;
    }
    v[0] += dd;
    v[1 + GMPNP_MAX_SURFACE_REACTIONS] += wn * zz[NS];
    v[2 + GMPNP_MAX_SURFACE_REACTIONS] += wn;
    if (kinetics) {
      double uu[NF];
#pragma unroll
      for (int j = 0; j < NF; ++j) uu[j] = c.u[row0 + j];
      KinRate R[GMPNP_MAX_SURFACE_REACTIONS];
      kinetics_rates<NF>(kt, uu, R);
      const gmpnp_kinetics_t* o = kt.opt;
      const double w = kt.w[n];
#pragma unroll
      for (int r = 0; r < GMPNP_MAX_SURFACE_REACTIONS; ++r)
        if (r < o->n_reactions) {
          const int re = o->reactant[r];
          double zu = 0.0;
#pragma unroll
          for (int j = 0; j < NS; ++j) zu = (j == re) ? zz[j] : zu;
          const double eta = o->p_electrode - uu[NS] - o->p_eq[r];
          const double e = tangent_rate_explicit(param, r, R[r].rate, R[r].d_p, eta);
          v[1 + r] += tangent_current_term(w, re >= 0 ? R[r].d_u : 0.0, R[r].d_p, zu, zz[NS], e);
        }
    }
  }
}

template <int DIM, int NF>
__global__ __launch_bounds__(kVecBlock) void k_tan_functional(const Ctx c, const KinTab kt, const SternTab st, const int kinetics, const TanTab t) {
  GMPNP_RULE_NO_CONTRACT
  constexpr int K = 3 + GMPNP_MAX_SURFACE_REACTIONS;
  __shared__ double lds[4 * K];
  __shared__ double mx[2 * 4];
  const int k = blockIdx.x;
  const int param = t.param[k];
  const double* z = t.z + (size_t)k * t.ndof;
  const double* Jz = t.Jz + (size_t)k * t.ndof;
  const double* col = t.c + (size_t)k * t.ndof;
  double rmax = 0.0, bmax = 0.0;
  bool wild = false;
  for (int idx = threadIdx.x; idx < t.ndof; idx += kVecBlock) {
    const double ci = col[idx], v = Jz[idx] + ci, zi = z[idx];
    wild = wild || !rule_finite(v) || !rule_finite(zi);
    rmax = fmax(rmax, fabs(v)); bmax = fmax(bmax, fabs(ci));
  }
  double v[K];
  tan_functional_sums<DIM, NF>(c, kt, st, kinetics, param, z, v);
  block_sum<K>(v, lds);
  const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
  double a = wild ? -1.0 : rmax, b = bmax;   // -1 marks a value that is not finite (every true maximum is >= 0)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double a2 = __shfl_xor(a, o), b2 = __shfl_xor(b, o);
    a = (a < 0.0 || a2 < 0.0) ? -1.0 : fmax(a, a2);
    b = fmax(b, b2);
  }
  if (ln == 0) { mx[wv] = a; mx[4 + wv] = b; }
  __syncthreads();
  if (threadIdx.x != 0) return;
  bool w2 = false;
  double ra = 0.0, rb = 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) { w2 = w2 || mx[q] < 0.0; ra = fmax(ra, mx[q]); rb = fmax(rb, mx[4 + q]); }
  TanOut* out = t.out + k;
  bool fin = rule_finite(v[0]);
  out->dD = v[0];
#pragma unroll
  for (int r = 0; r < GMPNP_MAX_SURFACE_REACTIONS; ++r) { out->dI[r] = v[1 + r]; fin = fin && rule_finite(v[1 + r]); }
  const double den = v[2 + GMPNP_MAX_SURFACE_REACTIONS];
  out->dp_boundary = den != 0.0 ? v[1 + GMPNP_MAX_SURFACE_REACTIONS] / den : 0.0;
  fin = fin && rule_finite(out->dp_boundary);
  out->residual = w2 ? __longlong_as_double(0x7ff8000000000000ll) : (rb > 0.0 ? ra / rb : ra);
  out->status = (w2 || !fin) ? kTangentNonFinite : 0;
  out->pad_ = 0;
}

// dx = -(dp z): the direction the step limiter looks at
__global__ __launch_bounds__(kVecBlock) void k_tan_scale(double* __restrict__ dx, const double* __restrict__ z, double dp, int n) {
  GMPNP_RULE_NO_CONTRACT
  const int i = blockIdx.x * kVecBlock + threadIdx.x;
  if (i < n) dx[i] = -(dp * z[i]);
}

// u += alpha dp z; part != nullptr: alpha from the step limiter's partials (step_update_body's reduction and rule), written to
// alpha_out by workgroup 0; a NaN / Inf in the direction: nothing is applied, alpha = NaN
__global__ __launch_bounds__(kVecBlock) void k_tan_advance(double* __restrict__ u, const double* __restrict__ z, double dp, double tau,
                                                           const double* __restrict__ part, const int32_t* __restrict__ part_node, int nblk,
                                                           double* __restrict__ alpha_out, int n) {
  GMPNP_RULE_NO_CONTRACT
  __shared__ double s_lam;
  __shared__ int s_bad;
  double alpha = 1.0;
  int bad = 0;
  if (part) {
    if (threadIdx.x < kWave) {
      double lam = INFINITY; int node = -1, b = 0;
      for (int i = threadIdx.x; i < nblk; i += kWave) {
        const double v = part[i];
        const int nd = part_node[i];
        if (nd == kStepBad) b = 1;
        else if (v < lam) { lam = v; node = nd; }
      }
      wave_min_index(lam, node);
      const int any_bad = __ballot(b) != 0 ? 1 : 0;
      if (threadIdx.x == 0) { s_lam = lam; s_bad = any_bad; }
    }
    __syncthreads();
    alpha = s_lam < 1.0 ? tau * s_lam : 1.0;
    bad = s_bad;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *alpha_out = bad ? NAN : alpha;
  if (bad) return;
  const int i = blockIdx.x * kVecBlock + threadIdx.x;
  if (i < n) u[i] = u[i] + (alpha * dp) * z[i];
}

// gmpnp_parameter_advance: the columns of a step in several parameters and their coefficients, by value
struct ParCols {
  int32_t n, pad_;
  const double* z[kTangentMaxColumns];
  double dtheta[kTangentMaxColumns];
};

// Both passes of gmpnp_parameter_advance, sums left to right in the order of `pc`, every product and sum rounded on its own:
//   dx != nullptr   dx = -(dtheta_0 z_0 + dtheta_1 z_1 + ...): the direction the step limiter looks at
//   dx == nullptr   u += (alpha dtheta_0) z_0 + (alpha dtheta_1) z_1 + ...; alpha as k_tan_advance finds it (part != nullptr: every
//                   workgroup re-reduces the step limiter's partials; a NaN / Inf in the direction: nothing is applied, alpha = NaN)
// One column is k_tan_scale's and k_tan_advance's expression.
__global__ __launch_bounds__(kVecBlock) void k_par_advance(double* __restrict__ u, double* __restrict__ dx, const ParCols pc, double tau,
                                                           const double* __restrict__ part, const int32_t* __restrict__ part_node, int nblk,
                                                           double* __restrict__ alpha_out, int n) {
  GMPNP_RULE_NO_CONTRACT
  __shared__ double s_lam;
  __shared__ int s_bad;
  const int i = blockIdx.x * kVecBlock + threadIdx.x;
  if (dx) {
    if (i >= n) return;
    double d = pc.dtheta[0] * pc.z[0][i];
    for (int k = 1; k < pc.n; ++k) d = d + pc.dtheta[k] * pc.z[k][i];
    dx[i] = -d;
    return;
  }
  double alpha = 1.0;
  int bad = 0;
  if (part) {
    if (threadIdx.x < kWave) {
      double lam = INFINITY; int node = -1, b = 0;
      for (int q = threadIdx.x; q < nblk; q += kWave) {
        const double v = part[q];
        const int nd = part_node[q];
        if (nd == kStepBad) b = 1;
        else if (v < lam) { lam = v; node = nd; }
      }
      wave_min_index(lam, node);
      const int any_bad = __ballot(b) != 0 ? 1 : 0;
      if (threadIdx.x == 0) { s_lam = lam; s_bad = any_bad; }
    }
    __syncthreads();
    alpha = s_lam < 1.0 ? tau * s_lam : 1.0;
    bad = s_bad;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *alpha_out = bad ? NAN : alpha;
  if (bad || i >= n) return;
  double d = (alpha * pc.dtheta[0]) * pc.z[0][i];
  for (int k = 1; k < pc.n; ++k) d = d + (alpha * pc.dtheta[k]) * pc.z[k][i];
  u[i] = u[i] + d;
}

}  // namespace gmpnp

namespace {

constexpr int kTanChainMax = 8;  // columns of the widest chain

// the tangent's right-hand-side levels (the storage holds kTanChainMax columns per level; a chain of M columns uses the first M)
std::vector<TriCols> tangent_levels(gmpnp_solver* s) {
  std::vector<TriCols> cl;
  double* p = s->tangenter->cols_store.p;
  const size_t nf = (size_t)s->nf;
  for (const TriLevel& l : s->tri) {
    TriCols c{};
    c.b = p; p += (size_t)kTanChainMax * nf * l.n;
    c.bi = p; p += (size_t)kTanChainMax * nf * l.n;
    c.x = p; p += (size_t)kTanChainMax * nf * l.n;
    cl.push_back(c);
  }
  return cl;
}

// the elimination of J (the Jacobian the stream holds) with the M right-hand sides level 0 of the tangent's storage holds
template <int NF, int M>
int tangent_chain(gmpnp_solver* s, const std::vector<TriCols>& cl) {
  const int nl = (int)s->tri.size(), l0 = bcr_tail_first_level(s);
  for (int l = 0; l < l0; ++l)
    hipLaunchKernelGGL((k_bcr_forward_cols<NF, M>), dim3(grid_for(s->tri[l + 1].n, 4)), dim3(64), 0, s->stream, s->tri[l], s->tri[l + 1], cl[l], cl[l + 1],
                       s->status.p);
  {
    TriTailCols tt{};
    tt.nlev = nl - l0;
    for (int l = l0; l < nl; ++l) { tt.lv[l - l0] = s->tri[l]; tt.cl[l - l0] = cl[l]; }
    hipLaunchKernelGGL((k_bcr_tail_cols<NF, M>), dim3(1), dim3(kBcrTailThreads), 0, s->stream, tt, s->status.p);
  }
  for (int l = l0 - 1; l >= 0; --l)
    hipLaunchKernelGGL((k_bcr_backward_cols<NF, M>), dim3(grid_for(s->tri[l].n * NF * M, kVecBlock)), dim3(kVecBlock), 0, s->stream, s->tri[l], s->tri[l + 1],
                       cl[l], cl[l + 1]);
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

// one chain of M columns: columns col0 ... col0 + used - 1 of c -> z.  The matrix levels are extracted by k_tri_extract (tri_solve's).
template <int NF, int M>
int tangent_solve_chain(gmpnp_solver* s, int col0, int used) {
  gmpnp_tangenter* T = s->tangenter.get();
  const int nv = s->t.nv;
  const std::vector<TriCols> cl = tangent_levels(s);
  hipLaunchKernelGGL((k_tri_extract<NF>), dim3(grid_for(nv * NF * NF, kVecBlock)), dim3(kVecBlock), 0, s->stream, s->c, s->tri[0], s->tri_kpos.p,
                     (const double*)T->c.p);
  hipLaunchKernelGGL((k_tan_extract<NF>), dim3(grid_for(M * NF * nv, kVecBlock)), dim3(kVecBlock), 0, s->stream, (const double*)T->c.p, cl[0].b, nv,
                     (int)s->ndof, col0, used, M);
  int rc = tangent_chain<NF, M>(s, cl); if (rc) return rc;
  hipLaunchKernelGGL((k_tan_apply<NF>), dim3(grid_for(used * s->ndof, kVecBlock)), dim3(kVecBlock), 0, s->stream, (const double*)cl[0].x, T->z.p, nv,
                     (int)s->ndof, col0, used);
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

// gmpnp_time_kernel(28): the chain(s) of the last call, extraction and application included
int tangent_time_chain(gmpnp_solver* s) {
  const int n = s->tangenter->last_n;
  if (n <= 2) return tangent_solve_chain<7, 2>(s, 0, n);
  int rc = tangent_solve_chain<7, 8>(s, 0, std::min(n, 8)); if (rc) return rc;
  if (n > 8) return tangent_solve_chain<7, 2>(s, 8, n - 8);
  return GMPNP_OK;
}
bool tangent_has_chain(const gmpnp_solver* s) { return s->tangenter && s->tangenter->last_n > 0 && s->dim == 1 && s->jacobian_valid; }

// 3D: one band-LU factorisation of the Jacobian the stream holds and n substitutions, each refined (band_refined_substitute);
// the storage of the factorisation is band_prepare's, under its memory cap
template <int NF>
int tangent_band_solves(gmpnp_solver* s, int n) {
  gmpnp_tangenter* T = s->tangenter.get();
  const size_t ndof = (size_t)s->ndof, bytes = ndof * sizeof(double);
  int rc = band_factor<NF>(s); if (rc) return rc;
  HIP_TRY(hipMemsetAsync(T->Jz.p, 0, bytes, s->stream));   // (a zero vector for the norm of the right-hand side; J z is formed afterwards)
  for (int k = 0; k < n; ++k) {
    hipLaunchKernelGGL(k_tan_scale, dim3(grid_for((int)ndof, kVecBlock)), dim3(kVecBlock), 0, s->stream, s->kb.p, (const double*)(T->c.p + k * ndof), 1.0, (int)ndof);
    hipLaunchKernelGGL(k_true_residual, dim3(s->n_resblocks), dim3(kVecBlock), 0, s->stream, (const double*)s->kb.p, (const double*)T->Jz.p, s->kr.p,
                       s->c.part_f, (int)ndof);
    HIP_TRY(hipStreamSynchronize(s->stream));
    const double bn = std::sqrt(sum_partials(s, 0));
    double rn = 0.0;
    rc = band_refined_substitute<NF>(s, std::max(1e-10 * bn, 0.0), &rn); if (rc) return rc;
    if (!rule_finite(rn)) return fail(GMPNP_ERR_LINEAR, "galvanostat: block-banded LU: the residual of a solve is not finite");   // (the text this refusal has always had)
    HIP_TRY(hipMemcpyAsync(T->z.p + k * ndof, s->kx.p, bytes, hipMemcpyDeviceToDevice, s->stream));
  }
  return GMPNP_OK;
}

const char* tangent_refusal(const gmpnp_solver* s) {
  if (s->partitioned) return "electrode tangent: partition handles and groups are not supported";
  if (s->ml_coarse || s->ml_is_coarse) return "electrode tangent: not with a multilevel coarse level attached";
  if (s->c.supg_rho) return "electrode tangent: not with SUPG terms set (gmpnp_set_supg)";
  if (!stern_on(s)) return "electrode tangent: the Stern option must be on (gmpnp_set_stern): p_M is then a parameter of F";
  if (galvanostat_on(s)) return "electrode tangent: the galvanostat is on; switch it off first (gmpnp_set_galvanostat keeps the potential it found)";
  if (kinetics_on(s) && s->kineticist->opt.p_electrode != s->sterner->opt.p_electrode)
    return "electrode tangent: the Stern option's p_electrode differs from the kinetics' (one electrode potential)";
  // (the Stern nodes and the kinetics' nodes are built from the same boundary list: one ascending list, gmpnp_kinetics.h)
  if (s->dim == 1 && (!s->tri_ok || s->nf != 7)) return "electrode tangent: a 1D handle needs the block-tridiagonal solver (a mesh in path order with 6 species)";
  if (s->dim == 3 && s->nf != 9) return "electrode tangent: a 3D handle needs the block-banded LU (8 species)";
  return nullptr;
}

}  // namespace

extern "C" {

int gmpnp_electrode_tangent(gmpnp_solver* s, int32_t n, const int32_t* param, gmpnp_tangent_t* out, double* z_out) {
  if (!s || !param || !out) return fail(GMPNP_ERR_INVALID, "electrode tangent: NULL argument");
  if (const char* why = tangent_refusal(s)) return fail(GMPNP_ERR_INVALID, why);
  if (!tangent_count_valid(n)) return fail(GMPNP_ERR_INVALID, "electrode tangent: n must lie in 1 ... 10");
  const int nr = kinetics_on(s) ? s->kineticist->opt.n_reactions : 0;
  int col_pM = -1;
  for (int k = 0; k < n; ++k) {
    const int kind = tangent_param_kind(param[k]);
    if (kind < 0) return fail(GMPNP_ERR_INVALID, "electrode tangent: unknown parameter (0 = p_M, 16 + r = ln k_r, 32 + r = alpha_r, 48 = ln lam)");
    if ((kind == 1 || kind == 2) && nr == 0) return fail(GMPNP_ERR_INVALID, "electrode tangent: a kinetic parameter needs the surface kinetics on (gmpnp_set_kinetics)");
    if (!tangent_param_valid(param[k], nr)) return fail(GMPNP_ERR_INVALID, "electrode tangent: a kinetic parameter names a reaction >= n_reactions");
    for (int q = 0; q < k; ++q)
      if (param[q] == param[k]) return fail(GMPNP_ERR_INVALID, "electrode tangent: a parameter is repeated");
    if (kind == 0) col_pM = k;
  }
  HIP_TRY(hipSetDevice(s->opts.device_id));
  const size_t ndof = (size_t)s->ndof;
  if (!s->tangenter) {
    std::unique_ptr<gmpnp_tangenter> T(new gmpnp_tangenter);
    HIP_TRY(T->c.alloc(kTangentMaxColumns * ndof)); HIP_TRY(T->z.alloc(kTangentMaxColumns * ndof)); HIP_TRY(T->Jz.alloc(kTangentMaxColumns * ndof));
    HIP_TRY(T->out.alloc(kTangentMaxColumns)); HIP_TRY(T->status.alloc(1)); HIP_TRY(T->alpha.alloc(1));
    size_t total = 0;
    if (s->dim == 1) for (const TriLevel& l : s->tri) total += (size_t)3 * kTanChainMax * s->nf * l.n;
    HIP_TRY(T->cols_store.alloc(total));
    HIP_TRY(hipHostMalloc((void**)&T->h_out, kTangentMaxColumns * sizeof(TanOut), hipHostMallocDefault));
    s->tangenter = std::move(T);
  }
  gmpnp_tangenter* T = s->tangenter.get();
  T->fresh = false; T->cols_fresh = false; T->last_n = 0;
  // F and J at the current u, as the first iteration of gmpnp_newton_solve assembles them
  HIP_TRY(hipMemsetAsync(s->status.p, 0, sizeof(int32_t), s->stream));
  HIP_TRY(hipMemsetAsync(T->status.p, 0, sizeof(int32_t), s->stream));
  double r = 0.0; int flags = 0;
  int rc;
  GMPNP_DISPATCH(s, rc = (residual<DIM, NF>(s, true, &r, &flags))); if (rc) return rc;
  GMPNP_DISPATCH(s, rc = (launch_jac_gather<DIM, NF>(s))); if (rc) return rc;
  s->jacobian_valid = true; s->precond_valid = false;
  if (flags & (32 | 64)) return fail(GMPNP_ERR_NUMERIC, "electrode tangent: " + status_message(flags & (32 | 64)));
  if (!rule_finite(r)) return fail(GMPNP_ERR_NUMERIC, "electrode tangent: the residual at the current state is not finite");
  // the columns
  TanTab t{};
  t.n = n; t.ndof = (int32_t)ndof;
  for (int k = 0; k < n; ++k) t.param[k] = param[k];
  t.c = T->c.p; t.z = T->z.p; t.Jz = T->Jz.p; t.out = T->out.p;
  const SternTab st = stern_tab(s, T->status.p);
  const int kin = kinetics_on(s) ? 1 : 0;
  KinTab kt{};
  if (kin) kt = kinetics_tab(s, T->status.p);
  HIP_TRY(hipMemsetAsync(T->c.p, 0, (size_t)n * ndof * sizeof(double), s->stream));
  if (col_pM >= 0) {
    double* b = T->c.p + (size_t)col_pM * ndof;
    if (kin) GMPNP_DISPATCH(s, hipLaunchKernelGGL((k_galv_rhs<DIM, NF>), dim3(grid_for(kt.n_nodes, kVecBlock)), dim3(kVecBlock), 0, s->stream, s->c, kt, st, 1, b));
    else GMPNP_DISPATCH(s, hipLaunchKernelGGL((k_response_rhs<DIM, NF>), dim3(grid_for(st.n_nodes, kVecBlock)), dim3(kVecBlock), 0, s->stream, s->c, st, b));
  }
  GMPNP_DISPATCH(s, hipLaunchKernelGGL((k_tan_columns<DIM, NF>), dim3(grid_for(st.n_nodes, kVecBlock)), dim3(kVecBlock), 0, s->stream, s->c, kt, st, kin, t));
  HIP_TRY(hipGetLastError());
  // the solves
  T->last_n = n;
  if (s->dim == 1) rc = tangent_time_chain(s); else rc = tangent_band_solves<9>(s, n);
  if (rc) return rc;
  for (int k = 0; k < n; ++k)
    GMPNP_DISPATCH(s, hipLaunchKernelGGL((k_spmv_plain<NF>), dim3(s->t.own_ntiles), dim3(kKrylovThreads), 0, s->stream, s->c,
                                         (const double*)(T->z.p + (size_t)k * ndof), T->Jz.p + (size_t)k * ndof));
  GMPNP_DISPATCH(s, hipLaunchKernelGGL((k_tan_functional<DIM, NF>), dim3(n), dim3(kVecBlock), 0, s->stream, s->c, kt, st, kin, t));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(T->h_out, T->out.p, (size_t)n * sizeof(TanOut), hipMemcpyDeviceToHost, s->stream));
  int32_t own = 0, word = 0;
  HIP_TRY(hipStreamSynchronize(s->stream));
  HIP_TRY(hipMemcpy(&own, T->status.p, sizeof(int32_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(&word, s->status.p, sizeof(int32_t), hipMemcpyDeviceToHost));
  if (own & (32 | 64)) return fail(GMPNP_ERR_NUMERIC, "electrode tangent: " + status_message(own & (32 | 64)));
  if (word & 2) return fail(GMPNP_ERR_LINEAR, "electrode tangent: " + status_message(word & 2));
  for (int k = 0; k < n; ++k) {
    const TanOut& o = T->h_out[k];
    gmpnp_tangent_t& q = out[k];
    q.param = param[k];
    q.dD = o.dD;
    for (int rr = 0; rr < GMPNP_MAX_SURFACE_REACTIONS; ++rr) q.dI[rr] = kin ? o.dI[rr] : 0.0;
    q.dp_boundary = o.dp_boundary; q.residual = o.residual; q.status = o.status;
  }
  if (z_out)
    for (int k = 0; k < n; ++k) { rc = download_vec(s, T->z.p + (size_t)k * ndof, z_out + (size_t)k * ndof); if (rc) return rc; }
  if (col_pM >= 0 && out[col_pM].status == 0) { T->fresh = true; T->col_pM = col_pM; }
  for (int k = 0; k < n; ++k) { T->param[k] = param[k]; T->col_status[k] = out[k].status; }
  T->cols_fresh = true;
  return GMPNP_OK;
}

int gmpnp_tangent_columns(gmpnp_solver* s, double* c_out) {
  if (!s || !c_out) return fail(GMPNP_ERR_INVALID, "electrode tangent: NULL argument");
  if (!s->tangenter || s->tangenter->last_n < 1) return fail(GMPNP_ERR_INVALID, "electrode tangent: no call has been made (gmpnp_electrode_tangent)");
  HIP_TRY(hipSetDevice(s->opts.device_id));
  for (int k = 0; k < s->tangenter->last_n; ++k) {
    int rc = download_vec(s, s->tangenter->c.p + (size_t)k * s->ndof, c_out + (size_t)k * s->ndof); if (rc) return rc;
  }
  return GMPNP_OK;
}

int gmpnp_electrode_advance(gmpnp_solver* s, double dp, double tau, double* alpha_out) {
  if (!s) return fail(GMPNP_ERR_INVALID, "electrode tangent: NULL handle");
  if (const char* why = tangent_refusal(s)) return fail(GMPNP_ERR_INVALID, why);
  if (!rule_finite(dp)) return fail(GMPNP_ERR_INVALID, "electrode tangent: dp must be finite");
  if (!step_fraction_valid(tau)) return fail(GMPNP_ERR_INVALID, "electrode tangent: tau must be 0 (no damping) or lie in (0, 1)");
  gmpnp_tangenter* T = s->tangenter.get();
  if (!T || !T->fresh)
    return fail(GMPNP_ERR_INVALID, "electrode tangent: the advance needs a tangent whose p_M column was computed at the present state, potential and options (gmpnp_electrode_tangent)");
  HIP_TRY(hipSetDevice(s->opts.device_id));
  const int ndof = (int)s->ndof;
  const double* z = T->z.p + (size_t)T->col_pM * s->ndof;
  const double* part = nullptr; const int32_t* part_node = nullptr; int nblk = 0;
  if (tau != 0.0) {
    int rc = step_prepare(s); if (rc) return rc;
    gmpnp_step_limiter* L = s->limiter.get();
    hipLaunchKernelGGL(k_tan_scale, dim3(grid_for(ndof, kVecBlock)), dim3(kVecBlock), 0, s->stream, L->dx.p, z, dp, ndof);
    GMPNP_DISPATCH(s, hipLaunchKernelGGL((k_step_limit<NF>), dim3(L->nblk), dim3(kVecBlock), 0, s->stream, step_limit_io(s, L->dx.p)));
    part = L->part.p; part_node = L->part_node.p; nblk = L->nblk;
  }
  hipLaunchKernelGGL(k_tan_advance, dim3(grid_for(ndof, kVecBlock)), dim3(kVecBlock), 0, s->stream, s->u.p, z, dp, tau, part, part_node, nblk, T->alpha.p, ndof);
  HIP_TRY(hipGetLastError());
  double alpha = 0.0;
  HIP_TRY(hipMemcpyAsync(s->h_stage, T->alpha.p, sizeof(double), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  alpha = s->h_stage[0];
  tangent_drop(s);
  if (!(alpha == alpha)) return fail(GMPNP_ERR_NUMERIC, "electrode tangent: " + status_message(16));
  // the potential takes the whole dp
  s->sterner->opt.p_electrode += dp;
  if (kinetics_on(s)) {
    s->kineticist->opt.p_electrode = s->sterner->opt.p_electrode;
    HIP_TRY(hipMemcpy(s->kineticist->d_opt.p, &s->kineticist->opt, sizeof(gmpnp_kinetics_t), hipMemcpyHostToDevice));
  }
  s->state_jumped = true;
  s->jacobian_valid = false; s->precond_valid = false;
  if (alpha_out) *alpha_out = alpha;
  return GMPNP_OK;
}

int gmpnp_parameter_advance(gmpnp_solver* s, int32_t n, const int32_t* param, const double* dtheta, double tau, double* alpha_out) {
  if (!s || !param || !dtheta) return fail(GMPNP_ERR_INVALID, "parameter advance: NULL argument");
  if (const char* why = tangent_refusal(s)) return fail(GMPNP_ERR_INVALID, std::string("parameter advance: ") + why);
  gmpnp_tangenter* T = s->tangenter.get();
  if (!T || !T->cols_fresh)
    return fail(GMPNP_ERR_INVALID, "parameter advance: it needs a tangent computed at the present state, potential and options (gmpnp_electrode_tangent)");
  if (const char* why = parameter_advance_refusal(n, param, dtheta, tau, T->last_n, T->param, T->col_status))
    return fail(GMPNP_ERR_INVALID, std::string("parameter advance: ") + why);
  // the moved options, validated before anything is changed
  const bool kin = kinetics_on(s);
  gmpnp_stern_t stern = s->sterner->opt;
  gmpnp_kinetics_t kinetics{};
  if (kin) kinetics = s->kineticist->opt;
  if (!parameter_move(stern, kinetics, s->nf - 1, n, param, dtheta))
    return fail(GMPNP_ERR_INVALID, "parameter advance: the moved parameters are not valid options (a finite p_electrode, k and alpha, lam > 0)");
  HIP_TRY(hipSetDevice(s->opts.device_id));
  const int ndof = (int)s->ndof;
  ParCols pc{};
  pc.n = n;
  for (int k = 0; k < n; ++k) {
    int at = 0;
    for (int q = 0; q < T->last_n; ++q) at = (T->param[q] == param[k]) ? q : at;
    pc.z[k] = T->z.p + (size_t)at * s->ndof;
    pc.dtheta[k] = dtheta[k];
  }
  const double* part = nullptr; const int32_t* part_node = nullptr; int nblk = 0;
  if (tau != 0.0) {
    int rc = step_prepare(s); if (rc) return rc;
    gmpnp_step_limiter* L = s->limiter.get();
    hipLaunchKernelGGL(k_par_advance, dim3(grid_for(ndof, kVecBlock)), dim3(kVecBlock), 0, s->stream, (double*)nullptr, L->dx.p, pc, tau, part, part_node, 0,
                       (double*)nullptr, ndof);
    GMPNP_DISPATCH(s, hipLaunchKernelGGL((k_step_limit<NF>), dim3(L->nblk), dim3(kVecBlock), 0, s->stream, step_limit_io(s, L->dx.p)));
    part = L->part.p; part_node = L->part_node.p; nblk = L->nblk;
  }
  hipLaunchKernelGGL(k_par_advance, dim3(grid_for(ndof, kVecBlock)), dim3(kVecBlock), 0, s->stream, s->u.p, (double*)nullptr, pc, tau, part, part_node, nblk,
                     T->alpha.p, ndof);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(s->h_stage, T->alpha.p, sizeof(double), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  const double alpha = s->h_stage[0];
  tangent_drop(s);
  if (!(alpha == alpha)) return fail(GMPNP_ERR_NUMERIC, "parameter advance: " + status_message(16));
  // the parameters take the whole step
  s->sterner->opt = stern;
  if (kin) {
    s->kineticist->opt = kinetics;
    HIP_TRY(hipMemcpy(s->kineticist->d_opt.p, &s->kineticist->opt, sizeof(gmpnp_kinetics_t), hipMemcpyHostToDevice));
  }
  s->state_jumped = true;
  s->jacobian_valid = false; s->precond_valid = false;
  if (alpha_out) *alpha_out = alpha;
  return GMPNP_OK;
}

int gmpnp_get_electrode_options(gmpnp_solver* s, gmpnp_stern_t* stern_out, gmpnp_kinetics_t* kinetics_out) {
  if (!s) return fail(GMPNP_ERR_INVALID, "electrode options: NULL handle");
  double p_M = 0.0;
  const bool galv = galvanostat_on(s);
  if (galv) {   // the galvanostat holds p_M on the device
    HIP_TRY(hipSetDevice(s->opts.device_id));
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipMemcpy(&p_M, s->galvanostat->scal.p, sizeof(double), hipMemcpyDeviceToHost));
  }
  if (stern_out) {
    gmpnp_stern_t o{};
    if (stern_on(s)) { o = s->sterner->opt; if (galv) o.p_electrode = p_M; }
    *stern_out = o;
  }
  if (kinetics_out) {
    gmpnp_kinetics_t o{};
    if (kinetics_on(s)) { o = s->kineticist->opt; if (galv) o.p_electrode = p_M; }
    *kinetics_out = o;
  }
  return GMPNP_OK;
}

}  // extern "C"
