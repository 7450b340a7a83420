// Fraction-to-boundary step limiter of the Newton update (include/gmpnp.h, gmpnp_newton_options_t.step_fraction = tau; the rule is
// restated in gmpnp_host_rules.h).  For the correction dx (J dx = b) at the state u:
//     S_I = sum_j a_j u_{I,j}      dS_I = sum_j a_j dx_{I,j}          (j ascending, plain fp64 sums, no fused multiply-add)
//     lambda = min over the nodes with dS_I < 0 and S_I < 1 of (1 - S_I) / (-dS_I)       (+inf: no such node)
//     alpha  = tau lambda if lambda < 1, else 1                     u <- u - omega alpha dx
// S is P1, so admissible vertices give admissible quadrature points: one pass over the nodes, no element pass.
//
//   k_step_limit      one lane per node: the workgroup's 256 node blocks of u and dx come through LDS (coalesced loads of the AoS rows in
//                     internal order), the lane forms its ratio, wave and workgroup minimum (ties: the smaller node) -> ONE partial per
//                     workgroup (ratio, internal node), in storage of the limiter's own (part_f may be in use by the side stream)
//   k_limited_update  every workgroup re-reduces the partials in the same fixed order to alpha, applies u -= omega alpha dx and leaves
//                     dx in kxp; workgroup 0 writes (alpha, lambda, node) into pinned host memory, which the host reads behind the
//                     synchronisation of the next residual evaluation: no synchronisation of its own
// A minimum does not depend on the order it is taken in: no atomics, two calls give equal bits.  A NaN / Inf in dx marks the
// workgroup's partial; the update is then NOT applied and bit 16 of the device status word is raised (GMPNP_ERR_NUMERIC).
// Included by gmpnp_api.hip behind gmpnp_kernels.h (newton() launches the kernels); the 1D ensemble (gmpnp_ensemble.h) runs the same
// bodies per member (blockIdx.y), every member with its own partials, alpha and report.
#pragma once

namespace gmpnp {

constexpr int kStepBad = -2;   // node entry of a partial whose workgroup met a non-finite entry of dx

// what workgroup 0 of the update leaves for the host (pinned memory)
struct StepReport {
  double alpha, lambda;   // alpha: NaN when `bad`
  int32_t node;           // internal index of the limiting node, -1 = none
  int32_t bad;            // dx held a NaN / Inf: nothing was applied
};

struct StepLimitIo {
  const double* u; const double* dx;   // [nv][NF] internal order
  const gmpnp_model_t* model;
  double* part; int32_t* part_node;    // [gridDim.x]
  int32_t nv;
};

struct StepUpdateIo {
  double* u; const double* dx; double* xp;   // u -= omega alpha dx, xp = dx
  const double* part; const int32_t* part_node;
  int32_t nblk, ndof;
  double omega, tau;
  StepReport* report;
  int32_t* status;   // device status word (bit 16), or nullptr
};

// minimum over the wave with its index, result in every lane; equal values: the smaller index (-1 = no index counts as the largest)
__device__ __forceinline__ void wave_min_index(double& v, int& idx) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o);
    const int oi = __shfl_xor(idx, o);
    if (ov < v || (ov == v && (unsigned)oi < (unsigned)idx)) { v = ov; idx = oi; }
  }
}

template <int NF>
__device__ __forceinline__ void step_limit_body(const StepLimitIo& io) {
  constexpr int NS = NF - 1;
  __shared__ double su[kVecBlock * NF], sd[kVecBlock * NF];
  __shared__ double wl[kVecBlock / kWave];
  __shared__ int wn[kVecBlock / kWave];
  const int t = threadIdx.x, n0 = blockIdx.x * kVecBlock;
  const int cnt = min(kVecBlock, io.nv - n0) * NF;   // doubles of this workgroup's node blocks (gridDim.x = ceil(nv / 256): cnt > 0)
  const size_t base = (size_t)n0 * NF;
  int bad = 0;
  for (int k = t; k < cnt; k += kVecBlock) {
    const double d = io.dx[base + k];
    su[k] = io.u[base + k]; sd[k] = d;
    bad |= ((__double2hiint(d) & 0x7ff00000) == 0x7ff00000) ? 1 : 0;   // NaN or Inf
  }
  const int any_bad = __syncthreads_or(bad);
  double lam = INFINITY; int node = -1;
  if (n0 + t < io.nv) {
#pragma clang fp contract(off)
    double S = 0.0, dS = 0.0;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      const double a = io.model->a[j];
      S = S + a * su[t * NF + j];
      dS = dS + a * sd[t * NF + j];
    }
    if (dS < 0.0 && S < 1.0) { lam = (1.0 - S) / (-dS); node = n0 + t; }
  }
  wave_min_index(lam, node);
  if ((t & (kWave - 1)) == 0) { wl[t >> 6] = lam; wn[t >> 6] = node; }
  __syncthreads();
  if (t == 0) {
#pragma unroll
    for (int w = 1; w < kVecBlock / kWave; ++w)
      if (wl[w] < lam) { lam = wl[w]; node = wn[w]; }   // the waves' nodes ascend: a tie keeps the smaller
    io.part[blockIdx.x] = lam;
    io.part_node[blockIdx.x] = any_bad ? kStepBad : node;
  }
}

// UPDATE = false: the report alone (gmpnp_step_limit), one workgroup
template <bool UPDATE>
__device__ __forceinline__ void step_update_body(const StepUpdateIo& io) {
  __shared__ double s_lam;
  __shared__ int s_node, s_bad;
  if (threadIdx.x < kWave) {
    double lam = INFINITY; int node = -1, bad = 0;
    for (int i = threadIdx.x; i < io.nblk; i += kWave) {
      const double v = io.part[i];
      const int nd = io.part_node[i];
      if (nd == kStepBad) bad = 1;
      else if (v < lam) { lam = v; node = nd; }
    }
    wave_min_index(lam, node);
    const int any_bad = __ballot(bad) != 0 ? 1 : 0;
    if (threadIdx.x == 0) { s_lam = lam; s_node = node; s_bad = any_bad; }
  }
  __syncthreads();
  const double lam = s_lam;
  const int bad = s_bad;
  const double alpha = lam < 1.0 ? io.tau * lam : 1.0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    io.report->alpha = bad ? NAN : alpha;
    io.report->lambda = lam;
    io.report->node = lam < INFINITY ? s_node : -1;
    io.report->bad = bad;
    if (bad && io.status) atomicOr(io.status, 16);
  }
  if (!UPDATE || bad) return;
  const int i = blockIdx.x * kVecBlock + threadIdx.x;
  if (i < io.ndof) {
    const double d = io.dx[i];
    io.u[i] -= (io.omega * alpha) * d;
    io.xp[i] = d;
  }
}

template <int NF>
__global__ __launch_bounds__(kVecBlock) void k_step_limit(const StepLimitIo io) { step_limit_body<NF>(io); }
__global__ __launch_bounds__(kVecBlock) void k_limited_update(const StepUpdateIo io) { step_update_body<true>(io); }
__global__ __launch_bounds__(kVecBlock) void k_step_report(const StepUpdateIo io) { step_update_body<false>(io); }

}  // namespace gmpnp
