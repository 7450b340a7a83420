// Periodic steady state of a potential programme: the device side of the accelerated cycle map (include/gmpnp.h "periodic steady
// state"; the host rules anderson_weights and cycle_verdict: gmpnp_host_rules.h; the driver: gmpnp_amd/periodic.py).
// The cycle map Phi takes u_n at the start of one period to u_n at its end.  The handle keeps a window of at most depth + 1 pairs
// (x_j, g_j = Phi(x_j)) in window order (oldest first, k = the newest) and a weight vector frozen at the open.  With r_j = g_j - x_j
// and d_j = r_{j+1} - r_j, over the FREE dofs i (bcflag = 0):
//     err^2 n_free = sum_i (r_k / w)^2        A_ij = sum (d_i / w)(d_j / w)  (i <= j)        b_i = sum (d_i / w)(r_k / w)
//
//   k_cycle_weights    w = atol_f + rtol |u_n| per dof (the open)
//   k_cycle_residual   workgroups of 256 nodes as k_time_error has them.  Every term is a per-dof expression (the weights carry the
//                      field), so the workgroup walks its 256 NF dofs with consecutive lanes on consecutive doubles and no row is
//                      staged in LDS (the 18 rows of a full window would take 2 x 9 x 256 x NF x 8 B > 160 KiB).  Per dof the lane
//                      forms the window's r_j, then r_k / w and the differences d_j / w — differences FIRST, then the products: a Gram
//                      matrix of the r_j would cancel where successive residuals differ in the third digit — and adds the 36 + 8
//                      products, (r_k / w)^2 and the free count to its K sums; block_sum -> ONE partial row per workgroup, [K][nblk];
//                      max |r_k / w| with its internal dof (ties: the smaller dof); a flag for a NaN / Inf in any vector of the window or in
//                      the weights (gmpnp_cycle_mix is refused behind such a report).
//                      The window's entries are picked by selects out of unrolled loops (no indexed register array, no scratch).
//   k_cycle_reduce     ONE workgroup sums the partial rows in workgroup order, takes the maximum and leaves the report in pinned memory
//   k_cycle_mix        free rows: u = u_n = g_k + alpha (sum_j gamma_j g_j - g_k), j in window order, every product and sum rounded on
//                      its own; Dirichlet rows: g_k.  One pass over the <= 9 stored g_j.  With tau != 0 a first pass writes the
//                      direction dx = -(sum_j gamma_j g_j - g_k) (0 on Dirichlet rows), k_step_limit looks at it at the state g_k, and
//                      every workgroup of the second pass re-reduces the limiter's partials (k_tan_advance's reduction and rule).
// No floating-point atomics, fixed summation order: two calls give equal bits.  All of it is allocated by gmpnp_cycle_open: a handle
// that never calls it keeps the buffers and launches it had.  Included at the end of gmpnp_api.hip.
#pragma once

namespace gmpnp {

constexpr int kCycleDepth = GMPNP_CYCLE_MAX_DEPTH;          // differences of a full window
constexpr int kCyclePairs = kCycleDepth + 1;                // pairs of a full window
constexpr int kCycleTri = kCycleDepth * (kCycleDepth + 1) / 2;
constexpr int kCycleCols = kCycleTri + kCycleDepth + 2;     // A (upper triangle by rows), b, sum (r_k / w)^2, free dofs

// what k_cycle_reduce leaves for the host (pinned memory)
struct CycleReport {
  double sum[kCycleCols];
  double worst;      // max |r_k / w|, -1 = no free dof
  int32_t dof;       // its internal dof, -1 = none
  int32_t bad;       // a vector of the window held a NaN / Inf
};

struct CycleWeightIo {
  const double* un; double* w;
  int32_t ndof, nf;
  double rtol, atol[GMPNP_MAX_SPECIES + 1];
};

struct CycleResidualIo {
  const double* x[kCyclePairs]; const double* g[kCyclePairs];   // window order; entries m ... are not read
  const double* w; const uint8_t* bcflag;                       // [nv][NF] internal order
  double* part;                                                 // [kCycleCols][nblk]
  double* part_max; int32_t* part_dof; int32_t* part_bad;       // [nblk]
  int32_t nv, nblk, m, pad_;                                    // m: pairs in the window, 1 ... 9
};

struct CycleMixIo {
  const double* g[kCyclePairs]; double gamma[kCyclePairs];      // window order; entries n ... are not read
  const uint8_t* bcflag;
  double* u; double* un;                                        // the apply pass writes both
  double* dx;                                                   // != nullptr: the direction pass (u, u_n untouched)
  const double* part; const int32_t* part_node;                 // the step limiter's partials (tau != 0), else nullptr
  double* alpha_out;
  double tau;
  int32_t nv, nblk_limit, n, pad_;
};

__device__ __forceinline__ int cycle_nonfinite(double x) { return ((__double2hiint(x) & 0x7ff00000) == 0x7ff00000) ? 1 : 0; }

__global__ __launch_bounds__(kVecBlock) void k_cycle_weights(const CycleWeightIo io) {
  GMPNP_RULE_NO_CONTRACT
  const int i = blockIdx.x * kVecBlock + threadIdx.x;
  if (i >= io.ndof) return;
  const int f = i % io.nf;
  double a = 0.0;
#pragma unroll
  for (int k = 0; k <= GMPNP_MAX_SPECIES; ++k) if (k == f) a = io.atol[k];
  io.w[i] = a + io.rtol * fabs(io.un[i]);
}

template <int NF>
__global__ __launch_bounds__(kVecBlock) void k_cycle_residual(const CycleResidualIo io) {
  GMPNP_RULE_NO_CONTRACT
  constexpr int P = kCyclePairs, D = kCycleDepth, K = kCycleCols;
  __shared__ double red[4 * K];
  __shared__ double wl[kVecBlock / kWave];
  __shared__ int wd[kVecBlock / kWave];
  const int t = threadIdx.x, n0 = blockIdx.x * kVecBlock;
  const int cnt = min(kVecBlock, io.nv - n0) * NF;   // doubles of this workgroup's node blocks (gridDim.x = ceil(nv / 256): cnt > 0)
  const size_t base = (size_t)n0 * NF;
  const int m = io.m;
  double v[K];
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = 0.0;
  double worst = -1.0; int dof = -1, bad = 0;
#pragma unroll 1
  for (int k = t; k < cnt; k += kVecBlock) {   // the lane's dofs ascend
    const size_t i = base + k;
    double r[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
      r[j] = 0.0;
      if (j < m) {
        const double xv = io.x[j][i], gv = io.g[j][i];
        bad |= cycle_nonfinite(xv) | cycle_nonfinite(gv);
        r[j] = gv - xv;
      }
    }
    const double w = io.w[i];
    bad |= cycle_nonfinite(w);   // (u_n was not finite at the open)
    if (io.bcflag[i]) continue;
    double rk = 0.0;
#pragma unroll
    for (int j = 0; j < P; ++j) if (j == m - 1) rk = r[j];
    const double qk = rk / w;
    double q[D];
#pragma unroll
    for (int j = 0; j < D; ++j) q[j] = (j + 1 < m) ? (r[j + 1] - r[j]) / w : 0.0;
    int c = 0;
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int b = a; b < D; ++b) { v[c] = v[c] + q[a] * q[b]; ++c; }
#pragma unroll
    for (int a = 0; a < D; ++a) v[kCycleTri + a] = v[kCycleTri + a] + q[a] * qk;
    v[kCycleTri + D] = v[kCycleTri + D] + qk * qk;
    v[kCycleTri + D + 1] = v[kCycleTri + D + 1] + 1.0;
    if (fabs(qk) > worst) { worst = fabs(qk); dof = (int)i; }   // a tie keeps the smaller dof
  }
  const int any_bad = __syncthreads_or(bad);
  block_sum<K>(v, red);
  wave_max_index(worst, dof);
  if ((t & (kWave - 1)) == 0) { wl[t >> 6] = worst; wd[t >> 6] = dof; }
  __syncthreads();
  if (t == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) io.part[(size_t)k * io.nblk + blockIdx.x] = v[k];
#pragma unroll
    for (int w = 1; w < kVecBlock / kWave; ++w)
      if (wl[w] > worst || (wl[w] == worst && (unsigned)wd[w] < (unsigned)dof)) { worst = wl[w]; dof = wd[w]; }
    io.part_max[blockIdx.x] = worst;
    io.part_dof[blockIdx.x] = dof;
    io.part_bad[blockIdx.x] = any_bad;
  }
}

// one workgroup; thread c < kCycleCols sums column c over the workgroups in their order, thread 64 takes the maximum
__global__ __launch_bounds__(kVecBlock) void k_cycle_reduce(const double* part, const double* part_max, const int32_t* part_dof,
                                                            const int32_t* part_bad, int nblk, CycleReport* out) {
  const int t = threadIdx.x;
  if (t < kCycleCols) {
    const double* p = part + (size_t)t * nblk;
    double s = 0.0;
    for (int i = 0; i < nblk; ++i) s += p[i];
    out->sum[t] = s;
  } else if (t == kWave) {
    double worst = -1.0; int dof = -1, bad = 0;
    for (int i = 0; i < nblk; ++i) {
      if (part_max[i] > worst) { worst = part_max[i]; dof = part_dof[i]; }   // the workgroups' dofs ascend: a tie keeps the smaller
      bad |= part_bad[i];
    }
    out->worst = worst; out->dof = dof; out->bad = bad;
  }
}

template <int NF>
__global__ __launch_bounds__(kVecBlock) void k_cycle_mix(const CycleMixIo io) {
  GMPNP_RULE_NO_CONTRACT
  constexpr int P = kCyclePairs;
  __shared__ double s_lam;
  __shared__ int s_bad;
  double alpha = 1.0;
  int bad = 0;
  if (io.part) {   // k_tan_advance's reduction of the step limiter's partials, by every workgroup
    if (threadIdx.x < kWave) {
      double lam = INFINITY; int node = -1, b = 0;
      for (int i = threadIdx.x; i < io.nblk_limit; i += kWave) {
        const double pv = io.part[i];
        const int nd = io.part_node[i];
        if (nd == kStepBad) b = 1;
        else if (pv < lam) { lam = pv; node = nd; }
      }
      wave_min_index(lam, node);
      const int any_bad = __ballot(b) != 0 ? 1 : 0;
      if (threadIdx.x == 0) { s_lam = lam; s_bad = any_bad; }
    }
    __syncthreads();
    alpha = s_lam < 1.0 ? io.tau * s_lam : 1.0;
    bad = s_bad;
  }
  if (!io.dx && blockIdx.x == 0 && threadIdx.x == 0) *io.alpha_out = bad ? NAN : alpha;
  if (bad) return;
  const int n0 = blockIdx.x * kVecBlock;
  const int cnt = min(kVecBlock, io.nv - n0) * NF;
  const size_t base = (size_t)n0 * NF;
  const int n = io.n;
#pragma unroll 1
  for (int k = threadIdx.x; k < cnt; k += kVecBlock) {
    const size_t i = base + k;
    double acc = 0.0, gk = 0.0;
#pragma unroll
    for (int j = 0; j < P; ++j) {
      if (j < n) {
        const double gv = io.g[j][i];
        const double term = io.gamma[j] * gv;
        acc = j == 0 ? term : acc + term;
        if (j == n - 1) gk = gv;
      }
    }
    const double p = acc - gk;
    const bool bc = io.bcflag[i] != 0;
    if (io.dx) { io.dx[i] = bc ? 0.0 : -p; continue; }
    const double val = bc ? gk : gk + alpha * p;
    io.u[i] = val; io.un[i] = val;
  }
}

}  // namespace gmpnp

namespace {

const char* cycle_refusal(const gmpnp_solver* s) {
  if (s->partitioned) return "cycle: partition handles and groups are not supported";
  if (s->ml_coarse || s->ml_is_coarse) return "cycle: not with a multilevel coarse level attached, nor on a handle that serves as one";
  if (galvanostat_on(s)) return "cycle: the galvanostat is on (gmpnp_set_galvanostat): p_M would be part of the cycle map's state";
  if (s->stepper && s->stepper->order == 2) return "cycle: not with order-2 time stepping (gmpnp_set_time_order): u_nm1 would be part of the cycle map's state";
  if (!(s->nf == 7 || s->nf == 9)) return "cycle: unsupported (dim, n_fields)";
  return nullptr;
}

inline bool cycle_is_open(const gmpnp_solver* s) { return s->cycler && s->cycler->open; }
inline int cycle_slot(const gmpnp_cycler* C, int j) { return (C->start + j) % C->cap; }

CycleResidualIo cycle_residual_io(const gmpnp_solver* s) {
  const gmpnp_cycler* C = s->cycler.get();
  CycleResidualIo io{};
  for (int j = 0; j < kCyclePairs; ++j) {
    const size_t off = (size_t)cycle_slot(C, j < C->window ? j : 0) * s->ndof;
    io.x[j] = C->X.p + off; io.g[j] = C->G.p + off;
  }
  io.w = C->w.p; io.bcflag = s->bcflag.p;
  io.part = C->part.p; io.part_max = C->part_max.p; io.part_dof = C->part_dof.p; io.part_bad = C->part_bad.p;
  io.nv = s->t.nv; io.nblk = C->nblk; io.m = C->window;
  return io;
}

// k_cycle_residual + k_cycle_reduce on the handle's stream
int cycle_residual_launch(gmpnp_solver* s) {
  gmpnp_cycler* C = s->cycler.get();
  const CycleResidualIo io = cycle_residual_io(s);
  if (s->nf == 9) hipLaunchKernelGGL((k_cycle_residual<9>), dim3(C->nblk), dim3(kVecBlock), 0, s->stream, io);
  else hipLaunchKernelGGL((k_cycle_residual<7>), dim3(C->nblk), dim3(kVecBlock), 0, s->stream, io);
  hipLaunchKernelGGL(k_cycle_reduce, dim3(1), dim3(kVecBlock), 0, s->stream, (const double*)C->part.p, (const double*)C->part_max.p,
                     (const int32_t*)C->part_dof.p, (const int32_t*)C->part_bad.p, C->nblk, C->d_report);
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

// the launches of one mix: u = u_n = g_k + alpha (sum_j gamma_j g_j - g_k); alpha lands in C->alpha
int cycle_mix_launch(gmpnp_solver* s, int n, const double* gamma, double tau) {
  gmpnp_cycler* C = s->cycler.get();
  CycleMixIo io{};
  for (int j = 0; j < kCyclePairs; ++j) {
    io.g[j] = C->G.p + (size_t)cycle_slot(C, j < n ? j : 0) * s->ndof;
    io.gamma[j] = j < n ? gamma[j] : 0.0;
  }
  io.bcflag = s->bcflag.p; io.u = s->u.p; io.un = s->un.p; io.alpha_out = C->alpha.p;
  io.tau = tau; io.nv = s->t.nv; io.n = n;
  auto launch = [&](const CycleMixIo& a) {
    if (s->nf == 9) hipLaunchKernelGGL((k_cycle_mix<9>), dim3(C->nblk), dim3(kVecBlock), 0, s->stream, a);
    else hipLaunchKernelGGL((k_cycle_mix<7>), dim3(C->nblk), dim3(kVecBlock), 0, s->stream, a);
  };
  if (tau != 0.0) {
    int rc = step_prepare(s); if (rc) return rc;
    gmpnp_step_limiter* L = s->limiter.get();
    CycleMixIo dir = io; dir.dx = L->dx.p;
    launch(dir);
    const StepLimitIo lim{io.g[n - 1], L->dx.p, s->d_model.p, L->part.p, L->part_node.p, s->t.nv};   // the limiter's rule at the state g_k
    if (s->nf == 9) hipLaunchKernelGGL((k_step_limit<9>), dim3(L->nblk), dim3(kVecBlock), 0, s->stream, lim);
    else hipLaunchKernelGGL((k_step_limit<7>), dim3(L->nblk), dim3(kVecBlock), 0, s->stream, lim);
    io.part = L->part.p; io.part_node = L->part_node.p; io.nblk_limit = L->nblk;
  }
  launch(io);
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

// gmpnp_time_kernel 33: residual + reduce + mix (gamma = the newest pair alone, tau = 0.9: both passes and the limiter) between a
// bracket that keeps u and u_n; the window, the flags of the handle and its history are not touched
bool cycle_has_window(const gmpnp_solver* s) { return cycle_is_open(s) && s->cycler->window >= 1 && !s->cycler->begun; }
int cycle_time_launch(gmpnp_solver* s) {
  gmpnp_cycler* C = s->cycler.get();
  int rc = cycle_residual_launch(s); if (rc) return rc;
  double gamma[kCyclePairs] = {};
  gamma[C->window - 1] = 1.0;
  return cycle_mix_launch(s, C->window, gamma, 0.9);
}
int cycle_kernel_begin(gmpnp_solver* s, DevBuf<double>& keep) {
  if (const char* why = cycle_refusal(s)) return fail(GMPNP_ERR_INVALID, why);
  const size_t n = (size_t)s->ndof, bytes = n * sizeof(double);
  HIP_TRY(keep.alloc(2 * n, false));
  HIP_TRY(hipMemcpyAsync(keep.p, s->u.p, bytes, hipMemcpyDeviceToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(keep.p + n, s->un.p, bytes, hipMemcpyDeviceToDevice, s->stream));
  return GMPNP_OK;
}
int cycle_kernel_end(gmpnp_solver* s, DevBuf<double>& keep) {
  const size_t n = (size_t)s->ndof, bytes = n * sizeof(double);
  HIP_TRY(hipMemcpyAsync(s->u.p, keep.p, bytes, hipMemcpyDeviceToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(s->un.p, keep.p + n, bytes, hipMemcpyDeviceToDevice, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return GMPNP_OK;
}

// what the caller gets from the device's report
gmpnp_cycle_report_t cycle_report_result(const gmpnp_solver* s, const CycleReport& r, int window) {
  gmpnp_cycle_report_t o{};
  const double n_free = r.sum[kCycleTri + kCycleDepth + 1];
  o.n_free = (int64_t)n_free;
  o.window = window; o.nonfinite = r.bad ? 1 : 0;
  o.err = n_free > 0.0 ? std::sqrt(r.sum[kCycleTri + kCycleDepth] / n_free) : 0.0;
  o.err_max = r.worst >= 0.0 ? r.worst : 0.0;
  if (r.bad) { o.err = NAN; o.err_max = NAN; }
  o.worst_dof = (!r.bad && r.dof >= 0) ? (int64_t)s->t.perm[r.dof / s->nf] * s->nf + r.dof % s->nf : -1;
  int c = 0;
  for (int a = 0; a < kCycleDepth; ++a)
    for (int b = a; b < kCycleDepth; ++b) { o.A[a * kCycleDepth + b] = r.sum[c]; o.A[b * kCycleDepth + a] = r.sum[c]; ++c; }
  for (int a = 0; a < kCycleDepth; ++a) o.b[a] = r.sum[kCycleTri + a];
  return o;
}

}  // namespace

extern "C" {

int gmpnp_cycle_open(gmpnp_solver* s, int32_t depth, const gmpnp_time_tol_t* tol) {
  if (!s || !tol) return fail(GMPNP_ERR_INVALID, "cycle: NULL argument");
  if (const char* why = cycle_refusal(s)) return fail(GMPNP_ERR_INVALID, why);
  if (depth < 1 || depth > GMPNP_CYCLE_MAX_DEPTH) return fail(GMPNP_ERR_INVALID, "cycle: depth is 1 ... 8");
  if (const char* why = time_error_invalid(1.0, 0.0, *tol, s->nf)) return fail(GMPNP_ERR_INVALID, std::string("cycle: ") + why);
  HIP_TRY(hipSetDevice(s->opts.device_id));
  if (!s->cycler) {
    std::unique_ptr<gmpnp_cycler> C(new gmpnp_cycler);
    C->nblk = std::max(1, grid_for(s->t.nv, kVecBlock));
    HIP_TRY(C->w.alloc((size_t)s->ndof));
    HIP_TRY(C->part.alloc((size_t)kCycleCols * C->nblk));
    HIP_TRY(C->part_max.alloc((size_t)C->nblk)); HIP_TRY(C->part_dof.alloc((size_t)C->nblk)); HIP_TRY(C->part_bad.alloc((size_t)C->nblk));
    HIP_TRY(C->alpha.alloc(1));
    HIP_TRY(hipHostMalloc((void**)&C->h_report, sizeof(CycleReport), hipHostMallocCoherent | hipHostMallocMapped));
    std::memset(C->h_report, 0, sizeof(CycleReport));
    { void* dp = nullptr; HIP_TRY(hipHostGetDevicePointer(&dp, C->h_report, 0)); C->d_report = (CycleReport*)dp; }
    s->cycler = std::move(C);
  }
  gmpnp_cycler* C = s->cycler.get();
  C->open = false;
  if (C->cap != depth + 1) {
    HIP_TRY(hipStreamSynchronize(s->stream));
    C->cap = 0;
    HIP_TRY(C->X.alloc((size_t)(depth + 1) * s->ndof)); HIP_TRY(C->G.alloc((size_t)(depth + 1) * s->ndof));
    C->cap = depth + 1;
  }
  C->depth = depth; C->start = 0; C->window = 0; C->begun = false; C->ended = false;
  CycleWeightIo io{};
  io.un = s->un.p; io.w = C->w.p; io.ndof = s->ndof; io.nf = s->nf; io.rtol = tol->rtol;
  for (int f = 0; f < s->nf; ++f) io.atol[f] = tol->atol[f];
  hipLaunchKernelGGL(k_cycle_weights, dim3(grid_for(s->ndof, kVecBlock)), dim3(kVecBlock), 0, s->stream, io);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s->stream));
  C->open = true;
  return GMPNP_OK;
}

int gmpnp_cycle_begin(gmpnp_solver* s) {
  if (!s) return fail(GMPNP_ERR_INVALID, "cycle: NULL argument");
  if (const char* why = cycle_refusal(s)) return fail(GMPNP_ERR_INVALID, why);
  if (!cycle_is_open(s)) return fail(GMPNP_ERR_INVALID, "cycle: no cycle is open (gmpnp_cycle_open)");
  gmpnp_cycler* C = s->cycler.get();
  HIP_TRY(hipSetDevice(s->opts.device_id));
  if (!C->begun && C->window == C->cap) { C->start = (C->start + 1) % C->cap; C->window -= 1; }   // the oldest pair leaves a full window
  HIP_TRY(hipMemcpyAsync(C->X.p + (size_t)cycle_slot(C, C->window) * s->ndof, s->un.p, (size_t)s->ndof * sizeof(double),
                         hipMemcpyDeviceToDevice, s->stream));
  C->begun = true; C->ended = false;
  return GMPNP_OK;
}

int gmpnp_cycle_end(gmpnp_solver* s, gmpnp_cycle_report_t* report) {
  if (!s || !report) return fail(GMPNP_ERR_INVALID, "cycle: NULL argument");
  if (const char* why = cycle_refusal(s)) return fail(GMPNP_ERR_INVALID, why);
  if (!cycle_is_open(s)) return fail(GMPNP_ERR_INVALID, "cycle: no cycle is open (gmpnp_cycle_open)");
  gmpnp_cycler* C = s->cycler.get();
  if (!C->begun) return fail(GMPNP_ERR_INVALID, "cycle: gmpnp_cycle_end without gmpnp_cycle_begin");
  HIP_TRY(hipSetDevice(s->opts.device_id));
  HIP_TRY(hipMemcpyAsync(C->G.p + (size_t)cycle_slot(C, C->window) * s->ndof, s->un.p, (size_t)s->ndof * sizeof(double),
                         hipMemcpyDeviceToDevice, s->stream));
  C->window += 1; C->begun = false; C->ended = true;
  int rc = cycle_residual_launch(s); if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  *report = cycle_report_result(s, *C->h_report, C->window);
  C->report_bad = report->nonfinite != 0;
  return GMPNP_OK;
}

int gmpnp_cycle_mix(gmpnp_solver* s, int32_t n, const double* gamma, double tau, double* alpha_out) {
  if (!s || !gamma) return fail(GMPNP_ERR_INVALID, "cycle: NULL argument");
  if (const char* why = cycle_refusal(s)) return fail(GMPNP_ERR_INVALID, why);
  if (!cycle_is_open(s)) return fail(GMPNP_ERR_INVALID, "cycle: no cycle is open (gmpnp_cycle_open)");
  gmpnp_cycler* C = s->cycler.get();
  if (!C->ended) return fail(GMPNP_ERR_INVALID, "cycle: gmpnp_cycle_mix needs the report of a gmpnp_cycle_end (mix before end)");
  if (trace_is_open(s) || sensitivity_is_open(s) || wall_profile_is_open(s))
    return fail(GMPNP_ERR_INVALID, "cycle: an electrode trace, sensitivity session or wall profile is open: close it, mix and open it again (its accumulators start at the mixed state)");
  if (C->report_bad)   // (with tau = 0 no pass of the mix looks for such a value: it would reach u and u_n)
    return fail(GMPNP_ERR_INVALID, "cycle: the last report met a value that is not finite in the window or the weights: restart (gmpnp_cycle_restart) or open again");
  if (n != C->window) return fail(GMPNP_ERR_INVALID, "cycle: n must equal the window of the last report");
  if (!cycle_gamma_valid(n, gamma)) return fail(GMPNP_ERR_INVALID, "cycle: every gamma finite and |sum gamma - 1| <= 1e-12");
  if (!step_fraction_valid(tau)) return fail(GMPNP_ERR_INVALID, "cycle: tau must be 0 (no limiter) or lie in (0, 1)");
  HIP_TRY(hipSetDevice(s->opts.device_id));
  int rc = cycle_mix_launch(s, n, gamma, tau); if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(s->h_stage, C->alpha.p, sizeof(double), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  const double alpha = s->h_stage[0];
  if (alpha_out) *alpha_out = alpha;
  if (!(alpha == alpha)) return fail(GMPNP_ERR_NUMERIC, "cycle: " + status_message(16));   // nothing was applied
  // the handle is where gmpnp_set_state(u, u) leaves it
  C->ended = false;
  tangent_drop(s);
  s->state_jumped = true;
  s->jacobian_valid = false; s->precond_valid = false;
  if (s->stepper) s->stepper->dropped();
  time_read_un(s);
  return GMPNP_OK;
}

int gmpnp_cycle_restart(gmpnp_solver* s) {
  if (!s) return fail(GMPNP_ERR_INVALID, "cycle: NULL argument");
  if (!cycle_is_open(s)) return fail(GMPNP_ERR_INVALID, "cycle: no cycle is open (gmpnp_cycle_open)");
  gmpnp_cycler* C = s->cycler.get();
  C->start = 0; C->window = 0; C->begun = false; C->ended = false;
  return GMPNP_OK;
}

int gmpnp_cycle_vectors(gmpnp_solver* s, int32_t which, double* out) {
  if (!s || !out) return fail(GMPNP_ERR_INVALID, "cycle: NULL argument");
  if (!cycle_is_open(s)) return fail(GMPNP_ERR_INVALID, "cycle: no cycle is open (gmpnp_cycle_open)");
  if (which < 0 || which > 2) return fail(GMPNP_ERR_INVALID, "cycle: which is 0 (x), 1 (g) or 2 (the weights)");
  gmpnp_cycler* C = s->cycler.get();
  HIP_TRY(hipSetDevice(s->opts.device_id));
  if (which == 2) return download_vec(s, C->w.p, out);
  const double* src = which == 0 ? C->X.p : C->G.p;
  for (int j = 0; j < C->window; ++j) {
    int rc = download_vec(s, src + (size_t)cycle_slot(C, j) * s->ndof, out + (size_t)j * s->ndof); if (rc) return rc;
  }
  return GMPNP_OK;
}

int gmpnp_cycle_close(gmpnp_solver* s) {
  if (!s) return fail(GMPNP_ERR_INVALID, "cycle: NULL argument");
  if (!cycle_is_open(s)) return fail(GMPNP_ERR_INVALID, "cycle: no cycle is open (gmpnp_cycle_open)");
  gmpnp_cycler* C = s->cycler.get();
  C->open = false; C->window = 0; C->start = 0; C->begun = false; C->ended = false;
  return GMPNP_OK;
}

}  // extern "C"
