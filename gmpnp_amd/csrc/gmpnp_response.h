// Small-signal frequency response of the 1D handle on the device: gmpnp_frequency_response (include/gmpnp.h), rule in
// gmpnp_host_rules.h (response_capacitance_term, response_current_term, response_chunk).
//
// At the handle's current u and p_M, per unit of p_M and with i sigma in the place of inv_dt:
//     (K + i sigma M) x = -b        K = J(u) at inv_dt = 0,  M = the consistent P1 mass on the free species rows,  b = dF/dp_M
//     C(sigma) = dD/dp_M + (dD/du).x        dI_r(sigma) = dI_r/dp_M + (dI_r/du).x
// K, M and b are real and the same for every frequency; a spectrum is n independent complex block-tridiagonal systems.
//
//   set-up (once per call)   model.inv_dt = 0 on the device, one residual evaluation + Jacobian gather, k_galv_rhs (kinetics on) or
//                     k_response_rhs (Stern alone) for b, k_tri_extract into the response's OWN level-0 SoA blocks, then the model is
//                     put back and the residual (and the Jacobian, where the handle held a valid one) is evaluated again: F, J and the
//                     flags are what they were, bit for bit.  The mass vector [3][nv] comes from the path-ordered coordinates.
//   k_response_solve  complex block Thomas, EIGHT LANES per frequency (lane r < NF holds row r of the 7 x 7 blocks, as
//                     tri_group_solve does) and eight frequencies per 64-lane workgroup; the sweep over the vertices is sequential.
//                     Vertex j: D' = D_j - L_j X_{j-1}[U], b' = -b_j - L_j X_{j-1}[b], then Gauss-Jordan with partial pivoting inside
//                     the block on [D' | U_j | b'] (pivot key |re| + |im|, rows stay where they are, ties to the lower lane);
//                     X_j = D'^-1 [U_j | b'] goes to the workspace [frequency][vertex][8 columns][8 lanes] complex in HBM and stays in
//                     registers for the next vertex.  The way back x_j = X_j[b] - X_j[U] x_{j+1} reads the workspace again.  The
//                     rows of vertex j + 1 are requested before vertex j is eliminated.  No LDS, no atomics: a group's arithmetic
//                     does not depend on its neighbours in the wave, so the bits of a frequency do not depend on n or on the chunk.
//   k_response_functional   one workgroup per frequency: max |(K + i sigma M) x + b| and max |b| over all rows from the real blocks
//                     and the mass vector (a maximum: any order gives the same bits), C and dI_r from the boundary nodes' entries
//                     (block_sum, fixed order), the per-frequency status word.
// A pivot that is (all but) zero sets bit 256 of that frequency's status, a value that is not finite bit 512; the other frequencies
// are not touched.  One host synchronisation per chunk; the chunk is sized from a memory cap (response_chunk).
// Included at the end of gmpnp_api.hip.
#pragma once

namespace gmpnp {

constexpr int kRespGroup = 8;                      // lanes per frequency
constexpr int kRespPerBlock = kWave / kRespGroup;  // frequencies per workgroup (one wave)

// what k_response_functional leaves per frequency
struct RespOut {
  double C[2];
  double dI[GMPNP_MAX_SURFACE_REACTIONS][2];
  double residual;
  int32_t status, pad_;
};

struct RespTab {
  int32_t nv, nfreq;            // vertices; frequencies of this chunk
  const double* sigma;          // [nfreq]
  TriLevel k;                   // level-0 SoA blocks of K (L, D, U) and b, the response's own storage
  const double* mass;           // [3][nv]: the species rows' mass entries towards I - 1, I, I + 1
  double2* ws;                  // [nfreq][nv][8][8] X = D'^-1 [U | b'], column-major inside a vertex, lane fastest
  double2* x;                   // [nfreq][nv][8]    the solution, internal order, one padding entry per vertex
  int32_t* fstat;               // [nfreq] what k_response_solve found
  RespOut* out;                 // [nfreq]
};

__device__ __forceinline__ Cx resp_shfl(Cx v, int src) { return Cx{__shfl(v.re, src, kRespGroup), __shfl(v.im, src, kRespGroup)}; }

template <int NF>
__global__ __launch_bounds__(kWave) void k_response_solve(const Ctx c, const RespTab t) {
  GMPNP_RULE_NO_CONTRACT   // the elimination's operations are those of the rule and of the model, one rounding each
  constexpr int NS = NF - 1, NX = NF + 1, NC = 2 * NF + 1;   // NX columns kept per vertex: U and the right-hand side
  static_assert(NF <= kRespGroup, "one lane per row of an 8-lane group");
  const int lane = threadIdx.x, r = lane & 7;
  const int f_raw = blockIdx.x * kRespPerBlock + (lane >> 3);
  const bool on = f_raw < t.nfreq;
  const int f = on ? f_raw : t.nfreq - 1;          // an idle group repeats the last frequency and stores nothing
  const bool rowon = r < NF;
  const int rc = rowon ? r : 0;
  const int nv = t.nv;
  const double sigma = t.sigma[f];
  double2* ws = t.ws + (size_t)f * nv * (NX * kRespGroup);
  double2* xo = t.x + (size_t)f * nv * kRespGroup;

  // rows of one vertex: real blocks, b and the imaginary diagonal sigma M of a free species row
  double lr[NF], dr[NF], ur[NF], br, ml, md, mu;
  auto load = [&](int j, double (&L)[NF], double (&D)[NF], double (&U)[NF], double& B, double& mL, double& mD, double& mU) {
#pragma unroll
    for (int cI = 0; cI < NF; ++cI) {
      const size_t off = (size_t)(rc * NF + cI) * nv + j;
      L[cI] = t.k.L[off]; D[cI] = t.k.D[off]; U[cI] = t.k.U[off];
    }
    B = t.k.b[(size_t)rc * nv + j];
    const double w = (rowon && r < NS && !c.bcflag[(size_t)j * NF + rc]) ? sigma : 0.0;
    mL = w * t.mass[j]; mD = w * t.mass[(size_t)nv + j]; mU = w * t.mass[(size_t)2 * nv + j];
  };
  load(0, lr, dr, ur, br, ml, md, mu);

  Cx X[NX];   // X_{j-1}: row r of D'^-1 [U | b'] of the vertex before
#pragma unroll
  for (int q = 0; q < NX; ++q) X[q] = Cx{0.0, 0.0};
  bool bad = false;

  for (int j = 0; j < nv; ++j) {
    // the next vertex's rows: requested now, used after this vertex's elimination
    double lr2[NF], dr2[NF], ur2[NF], br2, ml2, md2, mu2;
    load(j + 1 < nv ? j + 1 : j, lr2, dr2, ur2, br2, ml2, md2, mu2);

    Cx W[NC];   // [D' | U | b']
#pragma unroll
    for (int cI = 0; cI < NF; ++cI) {
      W[cI] = Cx{dr[cI], cI == r ? md : 0.0};
      W[NF + cI] = Cx{ur[cI], cI == r ? mu : 0.0};
    }
    W[2 * NF] = Cx{-br, 0.0};
    // minus L_j X_{j-1}: X row m sits in lane m
#pragma unroll
    for (int m = 0; m < NF; ++m) {
      const Cx l = Cx{lr[m], m == r ? ml : 0.0};
#pragma unroll
      for (int cI = 0; cI < NF; ++cI) W[cI] = cx_sub(W[cI], cx_mul(l, resp_shfl(X[cI], m)));
      W[2 * NF] = cx_sub(W[2 * NF], cx_mul(l, resp_shfl(X[NF], m)));
    }
    if (!rowon) {   // identity row: never a pivot of another column
#pragma unroll
      for (int cI = 0; cI < NC; ++cI) W[cI] = Cx{0.0, 0.0};
    }
    // Gauss-Jordan, partial pivoting inside the block (tri_group_solve's scheme on complex rows)
    bool used = !rowon;
    int home = r;
#pragma unroll
    for (int k = 0; k < NF; ++k) {
      unsigned long long key = used ? 0ull : (((unsigned long long)__double_as_longlong(response_pivot_key(W[k])) & ~7ull) | (unsigned long long)(7 - r));
#pragma unroll
      for (int o = 4; o > 0; o >>= 1) {
        const int olo = __shfl_xor((int)(unsigned)key, o, kRespGroup), ohi = __shfl_xor((int)(unsigned)(key >> 32), o, kRespGroup);
        const unsigned long long ok_ = ((unsigned long long)(unsigned)ohi << 32) | (unsigned)olo;
        key = ok_ > key ? ok_ : key;
      }
      const int p = 7 - (int)(key & 7ull);
      bad |= (key >> 3) == 0ull;   // the largest candidate is (all but) zero
      const Cx ip = cx_inv(resp_shfl(W[k], p));
      const Cx fac = (r == p) ? Cx{0.0, 0.0} : cx_mul(W[k], ip);
#pragma unroll
      for (int cI = k + 1; cI < NC; ++cI) {
        const Cx from_p = resp_shfl(W[cI], p);
        W[cI] = (r == p) ? cx_mul(W[cI], ip) : cx_sub(W[cI], cx_mul(fac, from_p));
      }
      used = used || (r == p);
      home = (r == k) ? p : home;
    }
    double2* wj = ws + (size_t)j * (NX * kRespGroup);
#pragma unroll
    for (int q = 0; q < NX; ++q) {
      X[q] = resp_shfl(W[NF + q], home);
      if (on) wj[q * kRespGroup + r] = make_double2(X[q].re, X[q].im);   // (lane 7 writes the zeros of its padding row)
    }
#pragma unroll
    for (int cI = 0; cI < NF; ++cI) { lr[cI] = lr2[cI]; dr[cI] = dr2[cI]; ur[cI] = ur2[cI]; }
    br = br2; ml = ml2; md = md2; mu = mu2;
  }

  // the way back: x_{nv-1} = X[b]; x_j = X_j[b] - X_j[U] x_{j+1}
  Cx xr = X[NF];
  bool wild = !(rule_finite(xr.re) && rule_finite(xr.im));
  if (on) xo[(size_t)(nv - 1) * kRespGroup + r] = make_double2(xr.re, xr.im);
  double2 nx[NX];
  if (nv > 1) {
    const double2* wj = ws + (size_t)(nv - 2) * (NX * kRespGroup);
#pragma unroll
    for (int q = 0; q < NX; ++q) nx[q] = on ? wj[q * kRespGroup + r] : make_double2(0.0, 0.0);
  }
  for (int j = nv - 2; j >= 0; --j) {
    double2 cur[NX];
#pragma unroll
    for (int q = 0; q < NX; ++q) cur[q] = nx[q];
    if (j > 0) {
      const double2* wj = ws + (size_t)(j - 1) * (NX * kRespGroup);
#pragma unroll
      for (int q = 0; q < NX; ++q) nx[q] = on ? wj[q * kRespGroup + r] : make_double2(0.0, 0.0);
    }
    Cx acc = Cx{cur[NF].x, cur[NF].y};
#pragma unroll
    for (int m = 0; m < NF; ++m) acc = cx_sub(acc, cx_mul(Cx{cur[m].x, cur[m].y}, resp_shfl(xr, m)));
    xr = acc;
    wild = wild || !(rule_finite(xr.re) && rule_finite(xr.im));
    if (on) xo[(size_t)j * kRespGroup + r] = make_double2(xr.re, xr.im);
  }
  int st = (bad ? kResponseSingular : 0) | ((wild && rowon) ? kResponseNonFinite : 0);
#pragma unroll
  for (int o = 4; o > 0; o >>= 1) st |= __shfl_xor(st, o, kRespGroup);
  if (on && r == 0) t.fstat[f] = st;
}

// b = dF/dp_M with the kinetics off: the Stern rows alone (k_galv_rhs's statement); every other entry of b stays zero
template <int DIM, int NF>
__global__ __launch_bounds__(kVecBlock) void k_response_rhs(const Ctx c, const SternTab st, double* __restrict__ b) {
  constexpr int NS = NF - 1;
  const int n = blockIdx.x * kVecBlock + threadIdx.x;
  if (n >= st.n_nodes) return;
  const size_t row0 = (size_t)st.node[n] * NF;
  double sb = 0.0;
  if (!c.bcflag[row0 + NS]) {
    for (int k = st.nf_ptr[n]; k < st.nf_ptr[n + 1]; ++k) {
      const SternFacet<DIM, NF> F(c, st, st.nf_ent[k] >> 2);
      sb += F.G.g * (DIM == 3 ? F.area / 3.0 : 1.0) / st.lam;
    }
  }
  b[row0 + NS] = sb;
}

template <int NF>
__global__ __launch_bounds__(kVecBlock) void k_response_functional(const Ctx c, const RespTab t, const SternTab st, const KinTab kt, const int kinetics) {
  GMPNP_RULE_NO_CONTRACT
  constexpr int NS = NF - 1, K = 2 + 2 * GMPNP_MAX_SURFACE_REACTIONS;
  __shared__ double lds[4 * K];
  __shared__ double mx[2 * 4];
  const int f = blockIdx.x, nv = t.nv;
  const double sigma = t.sigma[f];
  const double2* x = t.x + (size_t)f * nv * kRespGroup;
  // residual max |(K + i sigma M) x + b| and max |b|: one row per thread and trip, vertex fastest
  double rmax = 0.0, bmax = 0.0;
  bool wild = false;
  for (int idx = threadIdx.x; idx < nv * NF; idx += kVecBlock) {
    const int i = idx / nv, I = idx - i * nv;
    const double bi = t.k.b[idx];
    double re = bi, im = 0.0;
#pragma unroll
    for (int cI = 0; cI < NF; ++cI) {
      const size_t off = (size_t)(i * NF + cI) * nv + I;
      const double l = t.k.L[off], d = t.k.D[off], u = t.k.U[off];
      const double2 xl = I > 0 ? x[(size_t)(I - 1) * kRespGroup + cI] : make_double2(0.0, 0.0);
      const double2 xd = x[(size_t)I * kRespGroup + cI];
      const double2 xu = I + 1 < nv ? x[(size_t)(I + 1) * kRespGroup + cI] : make_double2(0.0, 0.0);
      re += l * xl.x + d * xd.x + u * xu.x;
      im += l * xl.y + d * xd.y + u * xu.y;
    }
    if (i < NS && !c.bcflag[(size_t)I * NF + i]) {
      const double2 xl = I > 0 ? x[(size_t)(I - 1) * kRespGroup + i] : make_double2(0.0, 0.0);
      const double2 xd = x[(size_t)I * kRespGroup + i];
      const double2 xu = I + 1 < nv ? x[(size_t)(I + 1) * kRespGroup + i] : make_double2(0.0, 0.0);
      const double mr = t.mass[I] * xl.x + t.mass[(size_t)nv + I] * xd.x + t.mass[(size_t)2 * nv + I] * xu.x;
      const double mi = t.mass[I] * xl.y + t.mass[(size_t)nv + I] * xd.y + t.mass[(size_t)2 * nv + I] * xu.y;
      re -= sigma * mi; im += sigma * mr;
    }
    const double mod = sqrt(re * re + im * im);
    wild = wild || !rule_finite(mod);
    rmax = fmax(rmax, mod); bmax = fmax(bmax, fabs(bi));
  }
  // C and dI_r from the boundary nodes (the Stern nodes and the kinetics' nodes are one ascending list)
  double v[K];
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = 0.0;
  for (int n = threadIdx.x; n < st.n_nodes; n += kVecBlock) {
    const size_t node = (size_t)st.node[n], row0 = node * NF;
    Cx xx[NF];
#pragma unroll
    for (int jf = 0; jf < NF; ++jf) { const double2 q = x[node * kRespGroup + jf]; xx[jf] = Cx{q.x, q.y}; }
    if (!c.bcflag[row0 + NS]) {
      Cx se = Cx{0.0, 0.0};
#pragma unroll
      for (int jf = 0; jf < NS; ++jf) { const double e = c.model->epsc[jf]; se.re += e * xx[jf].re; se.im += e * xx[jf].im; }
      for (int k = st.nf_ptr[n]; k < st.nf_ptr[n + 1]; ++k) {
        const SternFacet<1, NF> F(c, st, st.nf_ent[k] >> 2);
        const Cx term = response_capacitance_term(F.G.g, F.G.dg, st.lam, F.pM, F.p[0], xx[NS], se);
        v[0] += term.re; v[1] += term.im;
      }
    }
    if (kinetics) {
      double uu[NF];
#pragma unroll
      for (int jf = 0; jf < NF; ++jf) uu[jf] = c.u[row0 + jf];
      KinRate R[GMPNP_MAX_SURFACE_REACTIONS];
      kinetics_rates<NF>(kt, uu, R);
      const gmpnp_kinetics_t* o = kt.opt;
      const double w = kt.w[n];
#pragma unroll
      for (int rr = 0; rr < GMPNP_MAX_SURFACE_REACTIONS; ++rr)
        if (rr < o->n_reactions) {
          const int re_ = o->reactant[rr];
          Cx xu = Cx{0.0, 0.0};
#pragma unroll
          for (int jf = 0; jf < NS; ++jf) { xu.re = (jf == re_) ? xx[jf].re : xu.re; xu.im = (jf == re_) ? xx[jf].im : xu.im; }
          const Cx term = response_current_term(w, re_ >= 0 ? R[rr].d_u : 0.0, R[rr].d_p, xu, xx[NS]);
          v[2 + 2 * rr] += term.re; v[3 + 2 * rr] += term.im;
        }
    }
  }
  block_sum<K>(v, lds);
  // the two maxima and the flag
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
  RespOut* out = t.out + f;
  int status = t.fstat[f];
  bool fin = rule_finite(v[0]) && rule_finite(v[1]);
  out->C[0] = v[0]; out->C[1] = v[1];
#pragma unroll
  for (int rr = 0; rr < GMPNP_MAX_SURFACE_REACTIONS; ++rr) {
    out->dI[rr][0] = v[2 + 2 * rr]; out->dI[rr][1] = v[3 + 2 * rr];
    fin = fin && rule_finite(v[2 + 2 * rr]) && rule_finite(v[3 + 2 * rr]);
  }
  if (w2 || !fin) status |= kResponseNonFinite;
  out->residual = w2 ? __longlong_as_double(0x7ff8000000000000ll) : (rb > 0.0 ? ra / rb : ra);
  out->status = status; out->pad_ = 0;
}

}  // namespace gmpnp

namespace {

RespTab response_tab(gmpnp_solver* s, int nfreq) {
  gmpnp_responder* R = s->responder.get();
  const size_t nv = (size_t)s->t.nv, nf = (size_t)s->nf;
  RespTab t{};
  t.nv = (int)nv; t.nfreq = nfreq; t.sigma = R->sigma.p;
  t.k = TriLevel{};
  t.k.n = (int)nv;
  t.k.L = R->blocks.p; t.k.D = t.k.L + nf * nf * nv; t.k.U = t.k.D + nf * nf * nv; t.k.b = t.k.U + nf * nf * nv;
  t.mass = R->mass.p; t.ws = R->ws.p; t.x = R->x.p; t.fstat = R->fstat.p; t.out = R->out.p;
  return t;
}

// the two launches of one chunk whose sigma the device holds
int response_launch_chunk(gmpnp_solver* s, int nfreq) {
  gmpnp_responder* R = s->responder.get();
  const RespTab t = response_tab(s, nfreq);
  const SternTab st = stern_tab(s, R->status.p);
  const int kin = kinetics_on(s) ? 1 : 0;
  KinTab kt{};
  if (kin) kt = kinetics_tab(s, R->status.p);
  hipLaunchKernelGGL((k_response_solve<7>), dim3(grid_for(nfreq, kRespPerBlock)), dim3(kWave), 0, s->stream, s->c, t);
  hipLaunchKernelGGL((k_response_functional<7>), dim3(nfreq), dim3(kVecBlock), 0, s->stream, s->c, t, st, kt, kin);
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

int response_time_chunk(gmpnp_solver* s) { return response_launch_chunk(s, s->responder->last_chunk); }
bool response_has_chunk(const gmpnp_solver* s) { return s->responder && s->responder->last_chunk > 0; }

// the mass entries [3][nv] of a species row towards I - 1, I, I + 1 (k_jac_gather's Mab, summed over the vertex's two cells in element
// order): the consistent P1 mass M of J = K + inv_dt M on the free species rows (gmpnp_sensitivity.h reads the same vector)
std::vector<double> species_mass_1d(const gmpnp_solver* s) {
  const int nv = s->t.nv;
  std::vector<double> m((size_t)3 * nv, 0.0);
  constexpr double MDEN = Lay<1, 7>::MDEN;
  for (int I = 0; I + 1 < nv; ++I) {
    const double vol = std::fabs(s->t.coords[(size_t)I + 1] - s->t.coords[(size_t)I]);   // (1D: one coordinate per vertex, internal = path order)
    m[(size_t)2 * nv + I] += vol * MDEN;          // I -> I + 1
    m[(size_t)I + 1] += vol * MDEN;               // I + 1 -> I
    m[(size_t)nv + I] += vol * MDEN * 2.0; m[(size_t)nv + I + 1] += vol * MDEN * 2.0;
  }
  return m;
}

// K, b and the mass vector of the current state into the response's own storage; the handle's F, J and flags are put back
int response_setup(gmpnp_solver* s) {
  gmpnp_responder* R = s->responder.get();
  const int nv = s->t.nv, nf = s->nf;
  {
    const std::vector<double> m = species_mass_1d(s);
    HIP_TRY(hipMemcpy(R->mass.p, m.data(), m.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  HIP_TRY(hipStreamSynchronize(s->stream));
  const bool was_valid = s->jacobian_valid;
  int32_t word = 0;
  HIP_TRY(hipMemcpy(&word, s->status.p, sizeof(int32_t), hipMemcpyDeviceToHost));
  const int32_t host_word = *s->h_status;
  gmpnp_model_t steady = s->model;
  steady.inv_dt = 0.0;
  HIP_TRY(hipMemcpy(s->d_model.p, &steady, sizeof(gmpnp_model_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemsetAsync(s->status.p, 0, sizeof(int32_t), s->stream));
  HIP_TRY(hipMemsetAsync(R->status.p, 0, sizeof(int32_t), s->stream));
  HIP_TRY(hipMemsetAsync(R->b.p, 0, (size_t)s->ndof * sizeof(double), s->stream));
  double r = 0.0; int flags = 0;
  int rc = residual<1, 7>(s, true, &r, &flags);
  if (!rc) rc = launch_jac_gather<1, 7>(s);
  if (!rc) {
    const SternTab st = stern_tab(s, R->status.p);
    if (kinetics_on(s)) {
      const KinTab kt = kinetics_tab(s, R->status.p);
      hipLaunchKernelGGL((k_galv_rhs<1, 7>), dim3(grid_for(kt.n_nodes, kVecBlock)), dim3(kVecBlock), 0, s->stream, s->c, kt, st, 1, R->b.p);
    } else {
      hipLaunchKernelGGL((k_response_rhs<1, 7>), dim3(grid_for(st.n_nodes, kVecBlock)), dim3(kVecBlock), 0, s->stream, s->c, st, R->b.p);
    }
    hipLaunchKernelGGL((k_tri_extract<7>), dim3(grid_for(nv * nf * nf, kVecBlock)), dim3(kVecBlock), 0, s->stream, s->c, response_tab(s, 0).k,
                       s->tri_kpos.p, (const double*)R->b.p);
    if (hipGetLastError() != hipSuccess) rc = fail(GMPNP_ERR_HIP, "frequency response: a set-up launch failed");
  }
  // the handle as it was: the model, then F (and J where it was valid) at the model's own inv_dt, then the status words
  int32_t own = 0;
  hipError_t e = hipStreamSynchronize(s->stream);
  if (e == hipSuccess) e = hipMemcpy(&own, R->status.p, sizeof(int32_t), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(s->d_model.p, &s->model, sizeof(gmpnp_model_t), hipMemcpyHostToDevice);
  if (e != hipSuccess) return fail(GMPNP_ERR_HIP, std::string("frequency response: ") + hipGetErrorString(e));
  const std::string msg = g_err;
  double r2 = 0.0; int flags2 = 0;
  int rc2 = residual<1, 7>(s, was_valid, &r2, &flags2);
  if (!rc2 && was_valid) { rc2 = launch_jac_gather<1, 7>(s); if (!rc2) HIP_TRY(hipStreamSynchronize(s->stream)); }
  HIP_TRY(hipMemcpy(s->status.p, &word, sizeof(int32_t), hipMemcpyHostToDevice));
  *s->h_status = host_word;
  if (rc) { g_err = msg; return rc; }
  if (rc2) return rc2;
  if ((flags | own) & (32 | 64)) return fail(GMPNP_ERR_NUMERIC, "frequency response: " + status_message((flags | own) & (32 | 64)));
  if (!rule_finite(r)) return fail(GMPNP_ERR_NUMERIC, "frequency response: the residual at the current state is not finite");
  return GMPNP_OK;
}

}  // namespace

extern "C" {

int gmpnp_frequency_response(gmpnp_solver* s, int32_t n, const double* sigma, gmpnp_response_t* out, double* x_out) {
  if (!s || !sigma || !out) return fail(GMPNP_ERR_INVALID, "frequency response: NULL argument");
  if (s->partitioned) return fail(GMPNP_ERR_INVALID, "frequency response: partition handles and groups are not supported");
  if (s->ml_coarse || s->ml_is_coarse) return fail(GMPNP_ERR_INVALID, "frequency response: not with a multilevel coarse level attached");
  if (s->dim != 1) return fail(GMPNP_ERR_INVALID, "frequency response: 1D handles only (3D needs a complex band LU)");
  if (s->c.supg_rho) return fail(GMPNP_ERR_INVALID, "frequency response: not with SUPG terms set (gmpnp_set_supg)");
  if (!stern_on(s)) return fail(GMPNP_ERR_INVALID, "frequency response: the Stern option must be on (gmpnp_set_stern): p_M is then a parameter of F");
  if (galvanostat_on(s)) return fail(GMPNP_ERR_INVALID, "frequency response: the galvanostat is on; switch it off first (gmpnp_set_galvanostat keeps the potential it found)");
  if (!response_count_valid(n)) return fail(GMPNP_ERR_INVALID, "frequency response: n must lie in 1 ... 4096");
  for (int k = 0; k < n; ++k)
    if (!response_sigma_valid(sigma[k])) return fail(GMPNP_ERR_INVALID, "frequency response: every sigma must be finite and >= 0");
  if (!s->tri_ok || s->nf != 7) return fail(GMPNP_ERR_INVALID, "frequency response: needs a 1D mesh in path order with 6 species");
  if (kinetics_on(s) && s->kineticist->opt.p_electrode != s->sterner->opt.p_electrode)
    return fail(GMPNP_ERR_INVALID, "frequency response: the Stern option's p_electrode differs from the kinetics' (one electrode potential)");
  if (kinetics_on(s) && s->kineticist->n_nodes != s->sterner->n_nodes)
    return fail(GMPNP_ERR_INVALID, "frequency response: the Stern boundary and the kinetics' boundary differ");
  HIP_TRY(hipSetDevice(s->opts.device_id));
  const int nv = s->t.nv, nf = s->nf;
  double cap_mb = 1024.0;
  if (const char* env = std::getenv("GMPNP_RESPONSE_CAP_MB")) { const double v = std::atof(env); if (v > 0.0) cap_mb = v; }
  const int chunk = response_chunk(n, nv, cap_mb * 1048576.0);
  if (!s->responder) {
    std::unique_ptr<gmpnp_responder> R(new gmpnp_responder);
    HIP_TRY(R->blocks.alloc((size_t)nv * (3 * nf * nf + nf))); HIP_TRY(R->b.alloc((size_t)s->ndof)); HIP_TRY(R->mass.alloc((size_t)3 * nv));
    HIP_TRY(R->status.alloc(1));
    s->responder = std::move(R);
  }
  gmpnp_responder* R = s->responder.get();
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (R->cap_freq < (size_t)chunk) {
    R->last_chunk = 0;
    HIP_TRY(R->ws.alloc((size_t)chunk * nv * (nf + 1) * kRespGroup, false)); HIP_TRY(R->x.alloc((size_t)chunk * nv * kRespGroup, false));
    HIP_TRY(R->sigma.alloc((size_t)chunk)); HIP_TRY(R->fstat.alloc((size_t)chunk)); HIP_TRY(R->out.alloc((size_t)chunk));
    if (R->h_out) { (void)hipHostFree(R->h_out); R->h_out = nullptr; }
    HIP_TRY(hipHostMalloc((void**)&R->h_out, (size_t)chunk * sizeof(RespOut), hipHostMallocDefault));
    R->cap_freq = (size_t)chunk;
  }
  if (x_out && R->h_x_freq < (size_t)chunk) {
    if (R->h_x) { (void)hipHostFree(R->h_x); R->h_x = nullptr; R->h_x_freq = 0; }
    HIP_TRY(hipHostMalloc((void**)&R->h_x, (size_t)chunk * nv * kRespGroup * 2 * sizeof(double), hipHostMallocDefault));
    R->h_x_freq = (size_t)chunk;
  }
  int rc = response_setup(s); if (rc) return rc;
  const bool kin = kinetics_on(s);
  for (int k0 = 0; k0 < n; k0 += chunk) {
    const int m = std::min(chunk, n - k0);
    HIP_TRY(hipMemcpyAsync(R->sigma.p, sigma + k0, (size_t)m * sizeof(double), hipMemcpyHostToDevice, s->stream));
    rc = response_launch_chunk(s, m); if (rc) return rc;
    R->last_chunk = m;
    HIP_TRY(hipMemcpyAsync(R->h_out, R->out.p, (size_t)m * sizeof(RespOut), hipMemcpyDeviceToHost, s->stream));
    if (x_out) HIP_TRY(hipMemcpyAsync(R->h_x, R->x.p, (size_t)m * nv * kRespGroup * 2 * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));   // the chunk's one synchronisation
    for (int k = 0; k < m; ++k) {
      const RespOut& o = R->h_out[k];
      gmpnp_response_t& q = out[k0 + k];
      q.sigma = sigma[k0 + k];
      q.C[0] = o.C[0]; q.C[1] = o.C[1];
      for (int r = 0; r < GMPNP_MAX_SURFACE_REACTIONS; ++r) { q.dI[r][0] = kin ? o.dI[r][0] : 0.0; q.dI[r][1] = kin ? o.dI[r][1] : 0.0; }
      q.residual = o.residual; q.status = o.status;
      if (x_out) {
        const double* src = R->h_x + (size_t)k * nv * kRespGroup * 2;
        double* dst = x_out + (size_t)(k0 + k) * s->ndof * 2;
        for (int I = 0; I < nv; ++I)
          std::memcpy(dst + (size_t)s->t.perm[I] * nf * 2, src + (size_t)I * kRespGroup * 2, (size_t)nf * 2 * sizeof(double));
      }
    }
  }
  return GMPNP_OK;
}

}  // extern "C"
