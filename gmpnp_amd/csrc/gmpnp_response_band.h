// Small-signal frequency response of the 3D handle on the device: gmpnp_frequency_response_3d (include/gmpnp.h), rule in
// gmpnp_host_rules.h (response_facet_term, response_band_chunk, response_block_inverse; tangent_current_term, tangent_rate_explicit).
//
// gmpnp_response.h's system on the block band of gmpnp_band_lu.h: per unit of p_M and with i sigma in the place of inv_dt
//     (K + i sigma M) x = -b        K = J(u) at inv_dt = 0,  M = the consistent P1 mass on the free species rows,  b = dF/dp_M
//     C(sigma) = dD/dp_M + (dD/du).x        dI_r(sigma) = dI_r/dp_M + (dI_r/du).x
// K, M and b are real and the same for every frequency; a spectrum is n independent complex block-banded systems, and a chunk of them
// goes through ONE chain of launches: the frequency is the last grid dimension of every kernel below, and the batch member of
// gmpnp_band_lu.h's kernels, which do the elimination and the substitution on (re, im) pairs (policy BandComplex; the launch chains
// are gmpnp_api.hip's band_launch_factor / band_launch_substitute, the ones of the real solver).  What is the response's own:
//
//   set-up (once per call)   gmpnp_response.h's sequence: model.inv_dt = 0 on the device, residual + Jacobian gather, k_galv_rhs /
//                     k_response_rhs for b, the SELL values of K copied into the response's OWN storage, k_cband_mass (one double per
//                     node block from the element records' volumes, vol MDEN (1 + delta_ab) as the gather forms it), then the model
//                     back and the residual (and the gather, where the handle held a valid Jacobian) again.
//   k_cband_scatter   SELL values of K -> complex band, plus i sigma m_pq on the (i, i) entries of block (p, q) for free species rows i
//   k_cband_init / k_cband_axpy / k_cband_residual / k_cband_judge   refinement WITHOUT the host: the complex residual
//                     -(K + i sigma M) x - b from the real SELL values and the mass, its maximum per frequency, and a per-frequency
//                     `live` word (the band kernels' BandView::live): band_refine_again (gmpnp_host_rules.h, the real solver's rule)
//                     against 1e-10 max |b|.  The launches of a round are always made; the workgroups of a frequency that is done
//                     leave at once.
//   k_cband_functional   one workgroup per frequency: C and dI_r from the boundary nodes (k_tan_functional's node and facet terms on
//                     Re x and Im x, block_sum in fixed order), the residual and the status word.
// No floating-point atomics, no grid barriers, no spins; a frequency's workgroups read and write that frequency's storage alone, so its
// bits do not depend on n or on the chunk.  Status bit 256: a pivot block was singular (the pivot workgroups' BandView::status_bit, one
// word per frequency); 512: a value that is not finite.
// One host synchronisation per chunk.  Included at the end of gmpnp_api.hip.
#pragma once

namespace gmpnp {

using CBand = BandView<BandComplex>;   // band [nfreq][n][2b+1][NF][NF], dinv [nfreq][n][NF][NF]: (re, im) pairs

// what the refinement keeps per frequency
struct CBandState {
  double rn, best, bmax;   // max |residual| of the present x; the one before; max |b|
  int32_t live, rounds;    // 1: the next round's launches work on this frequency
};

struct CBandVec {
  int32_t ndof, nslices;
  const double* sigma;     // [nfreq]
  const double* mass;      // [nb] one double per node block of the Jacobian's pattern
  const double* b;         // [ndof] internal order
  double2* x;              // [nfreq][ndof] internal order
  double2* r;              // [nfreq][ndof] residual -(K + i sigma M) x - b (the first right-hand side: -b)
  double2* dx;             // [nfreq][ndof] what a substitution leaves
  double* rmax;            // [nfreq][nslices] max |r| per slice, -1: a value that is not finite
  CBandState* st;          // [nfreq]
  int32_t* fstat;          // [nfreq] bit 256 from the pivot workgroups
  RespOut* out;            // [nfreq]
};

// mass[k] of node block k: the gather's Mab summed over the block's element contributions in list order
template <int DIM, int NF>
__global__ __launch_bounds__(kVecBlock) void k_cband_mass(const Ctx c, double* __restrict__ mass) {
  using L = Lay<DIM, NF>;
  const int k = blockIdx.x * kVecBlock + threadIdx.x;
  if (k >= c.nb) return;
  double s = 0.0;
  for (int q = c.cptr[k]; q < c.cptr[k + 1]; ++q) {
    const int pk = c.contrib[q];
    s += c.EJ[(size_t)(pk >> 4) * L::EJ_STRIDE + L::O_VOL] * L::MDEN * (((pk >> 2) & 3) == (pk & 3) ? 2.0 : 1.0);
  }
  mass[k] = s;
}

// grid (nslices, nfreq); c.vals = the response's copy of K
template <int NF>
__global__ __launch_bounds__(64) void k_cband_scatter(const Ctx c, const CBand lu, const CBandVec v) {
  constexpr int NS = NF - 1;
  const int s = blockIdx.x, f = blockIdx.y, lane = threadIdx.x;
  if (lane >= c.slice_nn[s] * NF) return;
  const int il = lane / NF, i = lane - il * NF;
  const int I = c.slice_node0[s] + il, p = lu.lu_pos[I];
  const int cb = c.slice_colbase[s], mx = c.slice_colbase[s + 1] - cb;
  const double* val = c.vals + c.slice_off[s] + lane;
  const double sg = (i < NS && !c.bcflag[(size_t)I * NF + i]) ? v.sigma[f] : 0.0;
  for (int kp = 0; kp < mx; ++kp) {
    const size_t rec = (size_t)(cb + kp) * kSlicePad + il;
    const int blk = c.sell_blk[rec];
    if (blk < 0) continue;
    const int q = lu.lu_pos[c.sell_cols[rec] & 0xffffff];
    double2* dst = band_at<NF>(lu, f, p, q) + i * NF;
    const double im = sg * v.mass[blk];
#pragma unroll
    for (int j = 0; j < NF; ++j) dst[j] = make_double2(val[(size_t)(kp * NF + j) * kWave], j == i ? im : 0.0);
  }
}

// ---- refinement -------------------------------------------------------------------------------------------------------------------
// grid (nfreq): x = 0, r = -b, the frequency's state (live; max |b|)
__global__ __launch_bounds__(kVecBlock) void k_cband_init(const CBandVec v) {
  __shared__ double mx[4];
  const int f = blockIdx.x;
  double bmax = 0.0;
  for (int idx = threadIdx.x; idx < v.ndof; idx += kVecBlock) {
    const double bi = v.b[idx];
    v.x[(size_t)f * v.ndof + idx] = make_double2(0.0, 0.0);
    v.r[(size_t)f * v.ndof + idx] = make_double2(-bi, 0.0);
    bmax = fmax(bmax, fabs(bi));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bmax = fmax(bmax, __shfl_xor(bmax, o));
  if ((threadIdx.x & 63) == 0) mx[threadIdx.x >> 6] = bmax;
  __syncthreads();
  if (threadIdx.x == 0) v.st[f] = CBandState{0.0, 0.0, fmax(fmax(mx[0], mx[1]), fmax(mx[2], mx[3])), 1, 0};
}

// grid (ceil(ndof / 256), nfreq): x += dx
__global__ __launch_bounds__(kVecBlock) void k_cband_axpy(const CBandVec v) {
  const int f = blockIdx.y;
  if (!v.st[f].live) return;
  const int idx = blockIdx.x * kVecBlock + threadIdx.x;
  if (idx >= v.ndof) return;
  const size_t at = (size_t)f * v.ndof + idx;
  const double2 a = v.x[at], d = v.dx[at];
  v.x[at] = make_double2(a.x + d.x, a.y + d.y);
}

// grid (nslices, nfreq); c.vals = the response's copy of K.  r = -((K + i sigma M) x + b), rmax[slice] = max |r| (-1: not finite)
template <int NF>
__global__ __launch_bounds__(64) void k_cband_residual(const Ctx c, const CBandVec v) {
  constexpr int NS = NF - 1;
  const int s = blockIdx.x, f = blockIdx.y, lane = threadIdx.x;
  if (!v.st[f].live) return;
  const bool on = lane < c.slice_nn[s] * NF;
  double mod = 0.0;
  if (on) {
    const int il = lane / NF, i = lane - il * NF;
    const int I = c.slice_node0[s] + il;
    const size_t row = (size_t)I * NF + i;
    const int cb = c.slice_colbase[s], mxp = c.slice_colbase[s + 1] - cb;
    const double* val = c.vals + c.slice_off[s] + lane;
    const double2* x = v.x + (size_t)f * v.ndof;
    const double sg = (i < NS && !c.bcflag[row]) ? v.sigma[f] : 0.0;
    double re = v.b[row], im = 0.0;
    for (int kp = 0; kp < mxp; ++kp) {
      const size_t rec = (size_t)(cb + kp) * kSlicePad + il;
      const int blk = c.sell_blk[rec];
      if (blk < 0) continue;
      const size_t col0 = (size_t)(c.sell_cols[rec] & 0xffffff) * NF;
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        const double a = val[(size_t)(kp * NF + j) * kWave];
        const double2 xj = x[col0 + j];
        re += a * xj.x; im += a * xj.y;
      }
      const double m = sg * v.mass[blk];
      const double2 xi = x[col0 + i];
      re -= m * xi.y; im += m * xi.x;
    }
    v.r[(size_t)f * v.ndof + row] = make_double2(-re, -im);
    mod = sqrt(re * re + im * im);
    if (!rule_finite(mod)) mod = -1.0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double m2 = __shfl_xor(mod, o);
    mod = (mod < 0.0 || m2 < 0.0) ? -1.0 : fmax(mod, m2);
  }
  if (lane == 0) v.rmax[(size_t)f * v.nslices + s] = mod;
}

// grid (nfreq), one wave: band_refine_again on the residual of the x just formed.  Round 0 is the plain solve.
__global__ __launch_bounds__(kWave) void k_cband_judge(const CBandVec v, const int round) {
  const int f = blockIdx.x;
  CBandState st = v.st[f];
  if (!st.live) return;
  double mod = 0.0;
  for (int s = threadIdx.x; s < v.nslices; s += kWave) {
    const double m2 = v.rmax[(size_t)f * v.nslices + s];
    mod = (mod < 0.0 || m2 < 0.0) ? -1.0 : fmax(mod, m2);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double m2 = __shfl_xor(mod, o);
    mod = (mod < 0.0 || m2 < 0.0) ? -1.0 : fmax(mod, m2);
  }
  if (threadIdx.x != 0) return;
  const bool fin = mod >= 0.0;
  const bool live = band_refine_again(round, fin, mod, st.best, 1e-10 * st.bmax);
  st.rn = fin ? mod : __longlong_as_double(0x7ff8000000000000ll);
  st.best = st.rn; st.live = live ? 1 : 0; st.rounds = round;
  v.st[f] = st;
}

// grid (nfreq): C and dI_r of x (k_tan_functional's node and facet terms on the real and on the imaginary part)
template <int DIM, int NF>
__global__ __launch_bounds__(kVecBlock) void k_cband_functional(const Ctx c, const KinTab kt, const SternTab st, const int kinetics, const CBandVec v) {
  GMPNP_RULE_NO_CONTRACT
  constexpr int NS = NF - 1, K = 2 + 2 * GMPNP_MAX_SURFACE_REACTIONS, FN = SternFacet<DIM, NF>::FN;
  __shared__ double lds[4 * K];
  const int f = blockIdx.x;
  const double2* x = v.x + (size_t)f * v.ndof;
  double acc[K];
#pragma unroll
  for (int q = 0; q < K; ++q) acc[q] = 0.0;
  bool wild = false;
  for (int idx = threadIdx.x; idx < v.ndof; idx += kVecBlock) { const double2 q = x[idx]; wild = wild || !rule_finite(q.x) || !rule_finite(q.y); }
  const gmpnp_model_t* m = c.model;
  for (int n = threadIdx.x; n < st.n_nodes; n += kVecBlock) {
    const size_t row0 = (size_t)st.node[n] * NF;
    double ddr = 0.0, ddi = 0.0;
    if (!c.bcflag[row0 + NS]) {
      for (int q = st.nf_ptr[n]; q < st.nf_ptr[n + 1]; ++q) {
        const int ent = st.nf_ent[q], fc = ent >> 2, a = ent & 3;
        const SternFacet<DIM, NF> F(c, st, fc);
        const double share = DIM == 3 ? F.area / 3.0 : 1.0;
        const double wa = F.w(st, a);
        double ar = F.G.g * share / st.lam, ai = 0.0;   // the explicit d/dp_M part: the real part alone
#pragma unroll
        for (int b = 0; b < FN; ++b) {
          const size_t rb = (size_t)st.fnodes[fc * FN + b] * NF;
          double ser = 0.0, sei = 0.0;
          for (int j = 0; j < NS; ++j) { const double2 xj = x[rb + j]; ser += m->epsc[j] * xj.x; sei += m->epsc[j] * xj.y; }
          const double2 xp = x[rb + NS];
          ar += response_facet_term(F.G.g, F.G.dg, st.lam, wa, F.mass(a, b), ser / FN, xp.x);
          ai += response_facet_term(F.G.g, F.G.dg, st.lam, wa, F.mass(a, b), sei / FN, xp.y);
        }
        ddr += ar; ddi += ai;
      }
    }
    acc[0] += ddr; acc[1] += ddi;
    if (kinetics) {
      double uu[NF];
      double2 zz[NF];
#pragma unroll
      for (int j = 0; j < NF; ++j) { uu[j] = c.u[row0 + j]; zz[j] = x[row0 + j]; }
      KinRate R[GMPNP_MAX_SURFACE_REACTIONS];
      kinetics_rates<NF>(kt, uu, R);
      const gmpnp_kinetics_t* o = kt.opt;
      const double w = kt.w[n];
#pragma unroll
      for (int r = 0; r < GMPNP_MAX_SURFACE_REACTIONS; ++r)
        if (r < o->n_reactions) {
          const int re = o->reactant[r];
          double zur = 0.0, zui = 0.0;
#pragma unroll
          for (int j = 0; j < NS; ++j) { zur = (j == re) ? zz[j].x : zur; zui = (j == re) ? zz[j].y : zui; }
          const double eta = o->p_electrode - uu[NS] - o->p_eq[r];
          const double e = tangent_rate_explicit(0, r, R[r].rate, R[r].d_p, eta);
          acc[2 + 2 * r] += tangent_current_term(w, re >= 0 ? R[r].d_u : 0.0, R[r].d_p, zur, zz[NS].x, e);
          acc[3 + 2 * r] += tangent_current_term(w, re >= 0 ? R[r].d_u : 0.0, R[r].d_p, zui, zz[NS].y, 0.0);
        }
    }
  }
  block_sum<K>(acc, lds);
  const int any_wild = __syncthreads_or(wild ? 1 : 0);
  if (threadIdx.x != 0) return;
  const CBandState s = v.st[f];
  RespOut* out = v.out + f;
  bool fin = rule_finite(s.rn);
  out->C[0] = acc[0]; out->C[1] = acc[1];
  fin = fin && rule_finite(acc[0]) && rule_finite(acc[1]);
#pragma unroll
  for (int r = 0; r < GMPNP_MAX_SURFACE_REACTIONS; ++r) {
    out->dI[r][0] = acc[2 + 2 * r]; out->dI[r][1] = acc[3 + 2 * r];
    fin = fin && rule_finite(acc[2 + 2 * r]) && rule_finite(acc[3 + 2 * r]);
  }
  out->residual = s.bmax > 0.0 ? s.rn / s.bmax : s.rn;
  out->status = v.fstat[f] | ((any_wild || !fin) ? kResponseNonFinite : 0);
  out->pad_ = 0;
}

}  // namespace gmpnp

namespace {

// the chunk's bands as gmpnp_band_lu.h's batch: one member per frequency, its `live` word in the refinement's state, its pivot word in fstat
CBand cband_tab(gmpnp_solver* s) {
  gmpnp_band_responder* R = s->band_responder.get();
  CBand lu{};
  lu.band = R->band.p; lu.dinv = R->dinv.p; lu.lu_pos = R->pos.p; lu.lu_node = R->node.p; lu.n = R->n; lu.b = R->b;
  lu.band_stride = (size_t)R->n * (2 * R->b + 1) * 81; lu.dinv_stride = (size_t)R->n * 81;
  lu.vec_stride = (size_t)s->ndof; lu.part_stride = (size_t)kBandPanel * kBandChunks * 9;
  lu.live = &R->st.p->live; lu.live_stride = (int32_t)(sizeof(CBandState) / sizeof(int32_t));
  lu.status = R->fstat.p; lu.status_stride = 1; lu.status_bit = kResponseSingular;
  return lu;
}
CBandVec cband_vec(gmpnp_solver* s) {
  gmpnp_band_responder* R = s->band_responder.get();
  CBandVec v{};
  v.ndof = (int32_t)s->ndof; v.nslices = s->t.nslices;
  v.sigma = R->sigma.p; v.mass = R->mass.p; v.b = R->rhs.p;
  v.x = R->x.p; v.r = R->r.p; v.dx = R->dx.p; v.rmax = R->rmax.p;
  v.st = R->st.p; v.fstat = R->fstat.p; v.out = R->out.p;
  return v;
}

// every launch of one chunk whose sigma the device holds: scatter, factorisation, solve, three rounds of refinement, functionals
int cband_launch_chunk(gmpnp_solver* s, int m) {
  constexpr int NF = 9;
  gmpnp_band_responder* R = s->band_responder.get();
  const CBand lu = cband_tab(s);
  const CBandVec v = cband_vec(s);
  Ctx ck = s->c;
  ck.vals = R->kvals.p;
  const SternTab st = stern_tab(s, R->status.p);
  const int kin = kinetics_on(s) ? 1 : 0;
  KinTab kt{};
  if (kin) kt = kinetics_tab(s, R->status.p);
  HIP_TRY(hipMemsetAsync(lu.band, 0, (size_t)m * lu.band_stride * sizeof(double2), s->stream));
  HIP_TRY(hipMemsetAsync(R->fstat.p, 0, (size_t)m * sizeof(int32_t), s->stream));
  hipLaunchKernelGGL((k_cband_scatter<NF>), dim3(s->t.nslices, m), dim3(64), 0, s->stream, ck, lu, v);
  hipLaunchKernelGGL(k_cband_init, dim3(m), dim3(kVecBlock), 0, s->stream, v);
  int rc = band_launch_factor<NF>(s->stream, lu, m); if (rc) return rc;
  for (int round = 0; round <= 3; ++round) {
    rc = band_launch_substitute<NF>(s->stream, lu, m, (const double2*)v.r, R->y.p, R->part.p, v.dx); if (rc) return rc;   // every live frequency: r -> dx
    hipLaunchKernelGGL(k_cband_axpy, dim3(grid_for((int)s->ndof, kVecBlock), m), dim3(kVecBlock), 0, s->stream, v);
    hipLaunchKernelGGL((k_cband_residual<NF>), dim3(s->t.nslices, m), dim3(64), 0, s->stream, ck, v);
    hipLaunchKernelGGL(k_cband_judge, dim3(m), dim3(kWave), 0, s->stream, v, round);
  }
  hipLaunchKernelGGL((k_cband_functional<3, NF>), dim3(m), dim3(kVecBlock), 0, s->stream, s->c, kt, st, kin, v);
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

int response_band_time_chunk(gmpnp_solver* s) { return cband_launch_chunk(s, s->band_responder->last_chunk); }
// (the functional kernel reads the Stern tables of the handle's present option: with the option switched off since the call there is
// nothing to time)
bool response_band_has_chunk(const gmpnp_solver* s) { return s->band_responder && s->band_responder->last_chunk > 0 && stern_on(s); }

// K (SELL values), the mass and b of the current state into the response's own storage; the handle's F, J and flags are put back
// (response_setup's sequence on the 3D handle)
int cband_setup(gmpnp_solver* s) {
  gmpnp_band_responder* R = s->band_responder.get();
  HIP_TRY(hipStreamSynchronize(s->stream));
  const bool was_valid = s->jacobian_valid;
  int32_t word = 0;
  HIP_TRY(hipMemcpy(&word, s->status.p, sizeof(int32_t), hipMemcpyDeviceToHost));
  const int32_t host_word = *s->h_status;
  gmpnp_model_t steady = s->model;
  steady.inv_dt = 0.0;
  HIP_TRY(hipMemcpy(s->d_model.p, &steady, sizeof(gmpnp_model_t), hipMemcpyHostToDevice));
  // from here to the restore below nothing returns early: whatever fails, the model goes back to the device
  double r = 0.0; int flags = 0;
  int rc = GMPNP_OK;
  {
    hipError_t e0 = hipMemsetAsync(s->status.p, 0, sizeof(int32_t), s->stream);
    if (e0 == hipSuccess) e0 = hipMemsetAsync(R->status.p, 0, sizeof(int32_t), s->stream);
    if (e0 == hipSuccess) e0 = hipMemsetAsync(R->rhs.p, 0, (size_t)s->ndof * sizeof(double), s->stream);
    if (e0 != hipSuccess) rc = fail(GMPNP_ERR_HIP, std::string("frequency response (3D): ") + hipGetErrorString(e0));
  }
  if (!rc) rc = residual<3, 9>(s, true, &r, &flags);
  if (!rc) rc = launch_jac_gather<3, 9>(s);
  if (!rc) {
    const SternTab st = stern_tab(s, R->status.p);
    if (kinetics_on(s)) {
      const KinTab kt = kinetics_tab(s, R->status.p);
      hipLaunchKernelGGL((k_galv_rhs<3, 9>), dim3(grid_for(kt.n_nodes, kVecBlock)), dim3(kVecBlock), 0, s->stream, s->c, kt, st, 1, R->rhs.p);
    } else {
      hipLaunchKernelGGL((k_response_rhs<3, 9>), dim3(grid_for(st.n_nodes, kVecBlock)), dim3(kVecBlock), 0, s->stream, s->c, st, R->rhs.p);
    }
    hipLaunchKernelGGL((k_cband_mass<3, 9>), dim3(grid_for(s->nb, kVecBlock)), dim3(kVecBlock), 0, s->stream, s->c, R->mass.p);
    if (hipGetLastError() != hipSuccess) rc = fail(GMPNP_ERR_HIP, "frequency response (3D): a set-up launch failed");
    else if (hipMemcpyAsync(R->kvals.p, s->c.vals, R->kvals.n * sizeof(double), hipMemcpyDeviceToDevice, s->stream) != hipSuccess)
      rc = fail(GMPNP_ERR_HIP, "frequency response (3D): the copy of K failed");
  }
  // the handle as it was: the model, then F (and J where it was valid) at the model's own inv_dt, then the status words
  int32_t own = 0;
  const std::string msg0 = g_err;
  hipError_t e = hipStreamSynchronize(s->stream);
  if (e == hipSuccess) e = hipMemcpy(&own, R->status.p, sizeof(int32_t), hipMemcpyDeviceToHost);
  const hipError_t e_model = hipMemcpy(s->d_model.p, &s->model, sizeof(gmpnp_model_t), hipMemcpyHostToDevice);   // whatever came before
  if (e == hipSuccess) e = e_model;
  if (e != hipSuccess) { if (rc) { g_err = msg0; return rc; } return fail(GMPNP_ERR_HIP, std::string("frequency response (3D): ") + hipGetErrorString(e)); }
  const std::string msg = g_err;
  double r2 = 0.0; int flags2 = 0;
  int rc2 = residual<3, 9>(s, was_valid, &r2, &flags2);
  if (!rc2 && was_valid) { rc2 = launch_jac_gather<3, 9>(s); if (!rc2) HIP_TRY(hipStreamSynchronize(s->stream)); }
  HIP_TRY(hipMemcpy(s->status.p, &word, sizeof(int32_t), hipMemcpyHostToDevice));
  *s->h_status = host_word;
  if (rc) { g_err = msg; return rc; }
  if (rc2) return rc2;
  if ((flags | own) & (32 | 64)) return fail(GMPNP_ERR_NUMERIC, "frequency response (3D): " + status_message((flags | own) & (32 | 64)));
  if (!rule_finite(r)) return fail(GMPNP_ERR_NUMERIC, "frequency response (3D): the residual at the current state is not finite");
  return GMPNP_OK;
}

}  // namespace

extern "C" {

int gmpnp_band_lu_shape(gmpnp_solver* s, int32_t* n_blocks, int32_t* band) {
  if (!s || !n_blocks || !band) return fail(GMPNP_ERR_INVALID, "band LU shape: NULL argument");
  if (s->dim != 3) return fail(GMPNP_ERR_INVALID, "band LU shape: 3D handles only (the block-banded LU is the 3D direct solver)");
  *n_blocks = s->t.nv;
  *band = std::max(s->t.lu_band, kBandPanel - 1);
  return GMPNP_OK;
}

int gmpnp_frequency_response_3d(gmpnp_solver* s, int32_t n, const double* sigma, gmpnp_response_t* out, double* x_out) {
  if (!s || !sigma || !out) return fail(GMPNP_ERR_INVALID, "frequency response (3D): NULL argument");
  if (s->partitioned) return fail(GMPNP_ERR_INVALID, "frequency response (3D): partition handles and groups are not supported");
  if (s->ml_coarse || s->ml_is_coarse) return fail(GMPNP_ERR_INVALID, "frequency response (3D): not with a multilevel coarse level attached");
  if (s->dim != 3 || s->nf != 9) return fail(GMPNP_ERR_INVALID, "frequency response (3D): 3D handles with 8 species only (1D handles: gmpnp_frequency_response)");
  if (!stern_on(s)) return fail(GMPNP_ERR_INVALID, "frequency response (3D): the Stern option must be on (gmpnp_set_stern): p_M is then a parameter of F");
  if (galvanostat_on(s)) return fail(GMPNP_ERR_INVALID, "frequency response (3D): the galvanostat is on; switch it off first (gmpnp_set_galvanostat keeps the potential it found)");
  if (!response_count_valid(n)) return fail(GMPNP_ERR_INVALID, "frequency response (3D): n must lie in 1 ... 4096");
  for (int k = 0; k < n; ++k)
    if (!response_sigma_valid(sigma[k])) return fail(GMPNP_ERR_INVALID, "frequency response (3D): every sigma must be finite and >= 0");
  if (kinetics_on(s) && s->kineticist->opt.p_electrode != s->sterner->opt.p_electrode)
    return fail(GMPNP_ERR_INVALID, "frequency response (3D): the Stern option's p_electrode differs from the kinetics' (one electrode potential)");
  const int nv = s->t.nv, nf = s->nf, b = std::max(s->t.lu_band, kBandPanel - 1);
  const double per = response_band_bytes_per_frequency(nv, b, nf);
  if (per / 1e9 > s->cfg.lu_max_gb) {
    char buf[240];
    snprintf(buf, sizeof buf, "frequency response (3D): the complex band of one frequency needs %.2f GB (%d node blocks, band %d), above gmpnp_options_t.band_lu_max_gb = %.2f",
             per / 1e9, nv, b, s->cfg.lu_max_gb);
    return fail(GMPNP_ERR_INVALID, buf);
  }
  HIP_TRY(hipSetDevice(s->opts.device_id));
  const int chunk = response_band_chunk(n, nv, b, nf, s->cfg.lu_max_gb * 1e9);
  const size_t ndof = (size_t)s->ndof;
  if (!s->band_responder) {
    std::unique_ptr<gmpnp_band_responder> R(new gmpnp_band_responder);
    R->n = nv; R->b = b;
    HIP_TRY(R->mass.alloc((size_t)s->nb)); HIP_TRY(R->rhs.alloc(ndof)); HIP_TRY(R->kvals.alloc(s->vals.n, false)); HIP_TRY(R->status.alloc(1));
    HIP_TRY(R->pos.upload(s->t.lu_pos)); HIP_TRY(R->node.upload(s->t.lu_node));
    s->band_responder = std::move(R);
  }
  gmpnp_band_responder* R = s->band_responder.get();
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (R->cap_freq < (size_t)chunk) {
    const size_t c = (size_t)chunk;
    R->last_chunk = 0; R->cap_freq = 0;
    HIP_TRY(R->band.alloc(c * nv * (2 * (size_t)b + 1) * nf * nf, false)); HIP_TRY(R->dinv.alloc(c * nv * nf * nf));
    for (DevBuf<double2>* q : {&R->x, &R->r, &R->dx, &R->y}) HIP_TRY(q->alloc(c * ndof));
    HIP_TRY(R->part.alloc(c * kBandPanel * kBandChunks * nf)); HIP_TRY(R->rmax.alloc(c * s->t.nslices));
    HIP_TRY(R->sigma.alloc(c)); HIP_TRY(R->fstat.alloc(c)); HIP_TRY(R->st.alloc(c)); HIP_TRY(R->out.alloc(c));
    if (R->h_out) { (void)hipHostFree(R->h_out); R->h_out = nullptr; }
    HIP_TRY(hipHostMalloc((void**)&R->h_out, c * sizeof(RespOut), hipHostMallocDefault));
    R->cap_freq = c;
  }
  int rc = cband_setup(s); if (rc) return rc;
  const bool kin = kinetics_on(s);
  std::vector<double> hx;
  if (x_out) hx.resize((size_t)chunk * ndof * 2);
  for (int k0 = 0; k0 < n; k0 += chunk) {
    const int m = std::min(chunk, n - k0);
    HIP_TRY(hipMemcpyAsync(R->sigma.p, sigma + k0, (size_t)m * sizeof(double), hipMemcpyHostToDevice, s->stream));
    rc = cband_launch_chunk(s, m); if (rc) return rc;
    R->last_chunk = m;
    HIP_TRY(hipMemcpyAsync(R->h_out, R->out.p, (size_t)m * sizeof(RespOut), hipMemcpyDeviceToHost, s->stream));
    if (x_out) HIP_TRY(hipMemcpyAsync(hx.data(), R->x.p, (size_t)m * ndof * 2 * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));   // the chunk's one synchronisation
    for (int k = 0; k < m; ++k) {
      const RespOut& o = R->h_out[k];
      gmpnp_response_t& q = out[k0 + k];
      q.sigma = sigma[k0 + k];
      q.C[0] = o.C[0]; q.C[1] = o.C[1];
      for (int r = 0; r < GMPNP_MAX_SURFACE_REACTIONS; ++r) { q.dI[r][0] = kin ? o.dI[r][0] : 0.0; q.dI[r][1] = kin ? o.dI[r][1] : 0.0; }
      q.residual = o.residual; q.status = o.status;
      if (x_out) {
        const double* src = hx.data() + (size_t)k * ndof * 2;
        double* dst = x_out + (size_t)(k0 + k) * ndof * 2;
        for (int I = 0; I < nv; ++I)
          std::memcpy(dst + (size_t)s->t.perm[I] * nf * 2, src + (size_t)I * nf * 2, (size_t)nf * 2 * sizeof(double));
      }
    }
  }
  return GMPNP_OK;
}

}  // extern "C"
