// Block-banded LU of the node-block Jacobian on gfx950: the DIRECT linear solver of the 3D path, for real and for complex scalars.
//
// The reference solves every Newton system with MUMPS (3D/MPNP_CO2ER_pore.py:792, PETSc KSP preonly + LU).  The fast
// path of this library is the two-level BiCGStab; this file is what takes over when that Krylov solve does not converge
// (the stiff systems of the thinnest pores), and what `GMPNP_LINEAR_BAND_LU` selects explicitly.  The same kernels on
// (re, im) pairs solve the systems (K + i sigma M) x = -b of the 3D frequency response (gmpnp_response_band.h).
//
// Elimination order = the caller's slab order (vertices sorted along the pore axis): in that order the pattern is a
// band of b node blocks (182 on L_50_R_5), which the elimination fills completely, so the factor is stored as a dense
// block band (BandView below).  No MFMA: the update is a rank-NF (9) product per pivot, HBM-bound.
//
// ONE kernel set, template <int NF, class S>: S is the scalar policy (BandReal, BandComplex: storage and value type, the
// arithmetic, the column chunk and the dot batch), and a BATCH of independent bands goes through one chain of launches: the
// batch member is the last grid dimension of every kernel (the Newton path: extent 1, and S::kBatched = false makes the member
// index the constant 0, which takes the stride arithmetic out of its 4000 back-to-back launches; the response: a chunk of frequencies).
// A member's workgroups read and write that member's storage alone, so its bits depend neither on the extent nor on the others.
//
//   k_band_scatter  SELL values -> band storage (real; the response has its own, which adds i sigma M: k_cband_scatter)
//   k_band_step     pivot k: A_pq -= A_pk (D_k^-1 A_kq) for the (<= b)^2 window behind it; one extra workgroup: D_{k+1}^-1.  Row k and
//                   column k are only READ (they are the factors: L_pk = A_pk, U_kq = D_k^-1 A_kq with unit diagonal),
//                   everything written lies strictly behind them: no hazard inside a launch, one launch per pivot.
//   k_band_gather / k_band_panel / k_band_tri   forward and backward substitution in panels of 16 block rows (see below)
//
// Pivoting is partial INSIDE the NF x NF pivot block only; the caller checks the answer with the true residual
// b - J x and refines (gmpnp_api.hip: band_refined_substitute; the response: k_cband_judge; one rule: band_refine_again).
#pragma once
#include "gmpnp_kernels.h"
#include "gmpnp_host_rules.h"

namespace gmpnp {

constexpr int kBandThreads = 512;
constexpr int kBandColChunk = 16;   // pivot-row blocks one workgroup multiplies by D_k^-1 and keeps in LDS
constexpr int kCBandColChunk = 8;   // the same on (re, im) pairs (10.4 KB; 16 would double the operand registers)
constexpr int kBandDotBatch = 16;   // band-row entries per lane requested together (clamped indices, masks afterwards); complex: half

// ---- the two scalar policies ----------------------------------------------------------------------------------------
// mac / nmac are the elimination's and the substitution's acc + a b and acc - a b, contraction allowed.  The inv_* operations
// are the ONLY arithmetic of group16_inverse: a lexical pragma cannot depend on S, so whether they fuse is theirs to say.  The
// real ones fuse (f mine - f p is one fma); the complex ones are the host rule's cx_inv / cx_mul / cx_sub, every product and sum
// rounded on its own, because response_block_inverse (gmpnp_host_rules.h) is the statement of that inverse.
struct BandReal {
  using Store = double;
  using Val = double;
  static constexpr int kColChunk = kBandColChunk, kDotBatch = kBandDotBatch;
  static constexpr bool kTriangleInRegisters = true;   // k_band_tri: the whole in-panel triangle requested before the chain starts
  static constexpr bool kBatched = false;   // launched with a batch of one alone: the member index is the constant 0 and no stride is ever multiplied
  static __device__ __forceinline__ Val ld(const Store* p) { return *p; }
  static __device__ __forceinline__ void st(Store* p, Val v) { *p = v; }
  static __device__ __forceinline__ Val real(double v) { return v; }
  static __device__ __forceinline__ Val add(Val a, Val b) { return a + b; }
  static __device__ __forceinline__ Val sub(Val a, Val b) { return a - b; }
  static __device__ __forceinline__ Val mac(Val acc, Val a, Val b) { return acc + a * b; }
  static __device__ __forceinline__ Val nmac(Val acc, Val a, Val b) { return acc - a * b; }
  // one masked term of a dot product: the product is rounded, a masked lane adds 0
  static __device__ __forceinline__ Val dot(Val acc, bool on, Val a, Val b) { return acc + (on ? a * b : 0.0); }
  static __device__ __forceinline__ Val wsum(Val v) { return wave_sum(v); }
  static __device__ __forceinline__ Val shfl16(Val v, int src) { return __shfl(v, src, 16); }
  static __device__ __forceinline__ double inv_key(Val v) { return fabs(v); }
  static __device__ __forceinline__ Val inv_recip(Val v) { return 1.0 / v; }
  static __device__ __forceinline__ Val inv_mul(Val a, Val b) { return a * b; }
  static __device__ __forceinline__ Val inv_nmac(Val acc, Val a, Val b) { return acc - a * b; }
};

struct BandComplex {
  using Store = double2;   // (re, im): a lane moves 16 bytes
  using Val = Cx;
  static constexpr int kColChunk = kCBandColChunk, kDotBatch = kBandDotBatch / 2;
  static constexpr bool kTriangleInRegisters = false;   // k_band_tri: the in-panel entries of block row s + 1 requested while row s is solved
  static constexpr bool kBatched = true;
  static __device__ __forceinline__ Val ld(const Store* p) { const double2 v = *p; return Cx{v.x, v.y}; }
  static __device__ __forceinline__ void st(Store* p, Val v) { *p = make_double2(v.re, v.im); }
  static __device__ __forceinline__ Val real(double v) { return Cx{v, 0.0}; }
  static __device__ __forceinline__ Val add(Val a, Val b) { return cx_add(a, b); }
  static __device__ __forceinline__ Val sub(Val a, Val b) { return cx_sub(a, b); }
  static __device__ __forceinline__ Val mac(Val acc, Val a, Val b) { return Cx{acc.re + a.re * b.re - a.im * b.im, acc.im + a.re * b.im + a.im * b.re}; }
  static __device__ __forceinline__ Val nmac(Val acc, Val a, Val b) { return Cx{acc.re - a.re * b.re + a.im * b.im, acc.im - a.re * b.im - a.im * b.re}; }
  static __device__ __forceinline__ Val dot(Val acc, bool on, Val a, Val b) { return on ? mac(acc, a, b) : acc; }
  static __device__ __forceinline__ Val wsum(Val v) { return Cx{wave_sum(v.re), wave_sum(v.im)}; }
  static __device__ __forceinline__ Val shfl16(Val v, int src) { return Cx{__shfl(v.re, src, 16), __shfl(v.im, src, 16)}; }
  static __device__ __forceinline__ double inv_key(Val v) { return response_pivot_key(v); }
  static __device__ __forceinline__ Val inv_recip(Val v) { return cx_inv(v); }
  static __device__ __forceinline__ Val inv_mul(Val a, Val b) { return cx_mul(a, b); }
  static __device__ __forceinline__ Val inv_nmac(Val acc, Val a, Val b) { return cx_sub(acc, cx_mul(a, b)); }
};

// A batch of block-banded LUs in the elimination order of Topology::lu_node.  Block (p, q), |p - q| <= b, of member f lives at
// band[f * band_stride + (p * (2b+1) + (q - p + b)) * NF*NF], row major.  The vectors of the substitution (right-hand side, y, x) and
// its partial sums are the kernels' own arguments; member f's lie vec_stride / part_stride entries further per member.
template <class S>
struct BandView {
  typename S::Store* band;   // [batch][n][2b+1][NF][NF]
  typename S::Store* dinv;   // [batch][n][NF][NF] inverses of the pivot blocks
  const int32_t* lu_pos;     // [nv] internal node -> position
  const int32_t* lu_node;    // [nv] position -> internal node
  int32_t n, b;
  size_t band_stride, dinv_stride, vec_stride, part_stride;   // entries per member (S::kBatched false: never read)
  const int32_t* live;       // member f's substitution launches work while live[f * live_stride] != 0; null: always
  int32_t live_stride;
  int32_t* status;           // a singular pivot block of member f: status[f * status_stride] |= status_bit
  int32_t status_stride, status_bit;
};

template <class S>
__device__ __forceinline__ bool band_live(const BandView<S>& lu, int f) { return !lu.live || lu.live[(size_t)f * lu.live_stride] != 0; }

template <int NF, class S>
__device__ __forceinline__ typename S::Store* band_at(const BandView<S>& lu, int f, int p, int q) {
  return lu.band + (size_t)f * lu.band_stride + ((size_t)p * (2 * lu.b + 1) + (size_t)(q - p + lu.b)) * (NF * NF);
}

template <int NF>
__global__ __launch_bounds__(64) void k_band_scatter(const Ctx c, const BandView<BandReal> lu) {
  const int s = blockIdx.x, lane = threadIdx.x;
  if (lane >= c.slice_nn[s] * NF) return;
  const int il = lane / NF, i = lane - il * NF;
  const int I = c.slice_node0[s] + il, p = lu.lu_pos[I];
  const int cb = c.slice_colbase[s], mx = c.slice_colbase[s + 1] - cb;
  const double* v = c.vals + c.slice_off[s] + lane;
  for (int kp = 0; kp < mx; ++kp) {
    const size_t rec = (size_t)(cb + kp) * kSlicePad + il;
    if (c.sell_blk[rec] < 0) continue;
    const int q = lu.lu_pos[c.sell_cols[rec] & 0xffffff];
    double* dst = band_at<NF>(lu, 0, p, q) + i * NF;
#pragma unroll
    for (int j = 0; j < NF; ++j) dst[j] = v[(size_t)(kp * NF + j) * kWave];
  }
}

// Gauss-Jordan inverse of one NF x NF block by a 16-lane group: lane r (< NF) holds row r of [A | I].
// Partial pivoting (key: S::inv_key); returns true when a pivot column was all zero / NaN.
template <int NF, class S>
__device__ inline bool group16_inverse(typename S::Val (&row)[2 * NF], int r) {
  using V = typename S::Val;
  bool bad = false;
#pragma unroll
  for (int k = 0; k < NF; ++k) {
    double v = (r < NF && r >= k) ? S::inv_key(row[k]) : -1.0; int idx = r;
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
      const double ov = __shfl_xor(v, o, 16); const int oi = __shfl_xor(idx, o, 16);
      if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
    }
    bad |= !(v > 0.0);
    const V ip = S::inv_recip(S::shfl16(row[k], idx));
    const V oldk_k = S::shfl16(row[k], k);
    const V f = S::inv_mul((r == idx) ? oldk_k : row[k], ip);
#pragma unroll
    for (int j = k + 1; j < 2 * NF; ++j) {
      const V from_p = S::shfl16(row[j], idx), from_k = S::shfl16(row[j], k);
      const V mine = (r == idx) ? from_k : row[j];
      row[j] = (r == k) ? S::inv_mul(from_p, ip) : S::inv_nmac(mine, f, from_p);
    }
    row[k] = S::real((r == k) ? 1.0 : 0.0);
  }
  return bad;
}

// grid (ceil(w / QC), 1 + ceil(w / G), batch), w = min(b, n-1-k), QC = S::kColChunk; k = -1: grid (1, 1, batch).  The FIRST grid row is
// one extra workgroup (blockIdx.x = 0; the others of that row leave at once) that owns block (k+1, k+1): it applies pivot k to that one
// block, stores it and inverts it — the NEXT launch's pivot — while the window is being updated by everybody else.  Done at
// the end of the launch by the workgroup that holds the block, the dependent inverse (4 us of 16-lane shuffles) was a tail
// every launch waited for.  k = -1: only D_0^-1.
template <int NF, class S>
__global__ __launch_bounds__(kBandThreads) void k_band_step(const BandView<S> lu, const int k) {
  using T = typename S::Store;
  using V = typename S::Val;
  constexpr int BB = NF * NF, G = kBandThreads / BB, QC = S::kColChunk;
  __shared__ T sU[QC * BB];
  __shared__ T sD[BB];
  const int f = S::kBatched ? blockIdx.z : 0;
  const int t = threadIdx.x, g = t / BB, e = t - g * BB, i = e / NF, j = e - i * NF;
  T* dinv = lu.dinv + (size_t)f * lu.dinv_stride;
  if (blockIdx.y == 0) {   // the pivot workgroup: FIRST grid row, so that it is dispatched with the first workgroups whatever the window size
    if (blockIdx.x != 0) return;
    V entry = S::real(0.0);
    if (k >= 0) {
      const int tc = min(t, BB - 1), ic = tc / NF, jc = tc - ic * NF;
      V a9[NF], l9[NF];
      const T* Ak = band_at<NF>(lu, f, k, k + 1);
      const T* Lp = band_at<NF>(lu, f, k + 1, k) + ic * NF;
#pragma unroll
      for (int m = 0; m < NF; ++m) { a9[m] = S::ld(Ak + m * NF + jc); l9[m] = S::ld(Lp + m); }
      T* Cd = band_at<NF>(lu, f, k + 1, k + 1) + tc;
      V acc = S::ld(Cd);
      if (t < BB) sD[t] = dinv[(size_t)k * BB + t];
      __syncthreads();
      V u = S::real(0.0);   // same operation order as the window update below
#pragma unroll
      for (int ll = 0; ll < NF; ++ll) u = S::mac(u, S::ld(sD + ic * NF + ll), a9[ll]);
      if (t < BB) S::st(sU + t, u);
      __syncthreads();
#pragma unroll
      for (int m = 0; m < NF; ++m) acc = S::nmac(acc, l9[m], S::ld(sU + m * NF + jc));
      if (t < BB) S::st(Cd, acc);
      entry = acc;
    } else if (t < BB) {
      entry = S::ld(band_at<NF>(lu, f, 0, 0) + t);
    }
    if (k + 1 >= lu.n) return;
    // D_{k+1}^-1 (sD is free: its last readers passed the barrier above)
    if (t < BB) S::st(sD + t, entry);
    __syncthreads();
    if (t < kWave) {   // wave 0: its four 16-lane groups all do the same work, group 0 writes
      const int r = t & 15;
      V row[2 * NF];
#pragma unroll
      for (int jj = 0; jj < NF; ++jj) {
        row[jj] = (r < NF) ? S::ld(sD + (r < NF ? r : 0) * NF + jj) : S::real(0.0);
        row[NF + jj] = S::real((jj == r) ? 1.0 : 0.0);
      }
      const bool bad = group16_inverse<NF, S>(row, r);
      if (t < NF) {
        T* o = dinv + ((size_t)(k + 1) * NF + t) * NF;
#pragma unroll
        for (int jj = 0; jj < NF; ++jj) S::st(o + jj, row[NF + jj]);
      }
      if (t == 0 && bad) atomicOr(lu.status + (size_t)f * lu.status_stride, lu.status_bit);
    }
    return;
  }
  const int w = min(lu.b, lu.n - 1 - k);
  const int q0 = k + 1 + blockIdx.x * QC, p = k + 1 + ((int)blockIdx.y - 1) * G + g;
  const int nq = min(QC, k + w + 1 - q0);
  // every global operand is requested before the first barrier (clamped indices, masks afterwards): one memory
  // latency per launch instead of three dependent ones; the launches of a factorisation run back to back
  constexpr int UP = (QC * BB + kBandThreads - 1) / kBandThreads;   // U' entries per thread
  const bool act = g < G && p <= k + w;
  const int pc = min(p, k + w);
  const T dk = dinv[(size_t)k * BB + min(t, BB - 1)];
  const T* Ak = band_at<NF>(lu, f, k, q0);
  V a[UP][NF];
#pragma unroll
  for (int u = 0; u < UP; ++u) {
    const int idx = min(t + u * kBandThreads, nq * BB - 1), qq = idx / BB, ee = idx - qq * BB, jj = ee % NF;
#pragma unroll
    for (int l = 0; l < NF; ++l) a[u][l] = S::ld(Ak + (size_t)qq * BB + l * NF + jj);
  }
  const T* Lp = band_at<NF>(lu, f, pc, k) + i * NF;
  V l[NF];
#pragma unroll
  for (int m = 0; m < NF; ++m) l[m] = S::ld(Lp + m);
  T* C = band_at<NF>(lu, f, pc, q0) + e;
  V cv[QC];
#pragma unroll
  for (int qq = 0; qq < QC; ++qq) cv[qq] = S::ld(C + (size_t)min(qq, nq - 1) * BB);
  if (t < BB) sD[t] = dk;
  __syncthreads();
#pragma unroll
  for (int u = 0; u < UP; ++u) {
    const int idx = t + u * kBandThreads;
    const int ic = min(idx, nq * BB - 1), qq = ic / BB, ee = ic - qq * BB, m = ee / NF;
    V acc = S::real(0.0);
#pragma unroll
    for (int ll = 0; ll < NF; ++ll) acc = S::mac(acc, S::ld(sD + m * NF + ll), a[u][ll]);
    if (idx < nq * BB) S::st(sU + idx, acc);
  }
  __syncthreads();
  if (act) {
    const bool pivot_block = (p == k + 1 && q0 == k + 1);   // (k+1, k+1) belongs to the pivot workgroup
#pragma unroll
    for (int qq = 0; qq < QC; ++qq) {
      V acc = cv[qq];
#pragma unroll
      for (int m = 0; m < NF; ++m) acc = S::nmac(acc, l[m], S::ld(sU + min(qq, nq - 1) * BB + m * NF + j));
      if (qq < nq && !(pivot_block && qq == 0)) S::st(C + (size_t)qq * BB, acc);
    }
  }
}

// ---- substitution: panels of kBandPanel block rows, two launches per panel -----------------------------------------
// x = U^-1 L^-1 rhs with y_k = D_k^-1 (rhs_k - sum_{q<k} A_kq y_q) and x_k = y_k - D_k^-1 sum_{q>k} A_kq x_q.  The chain
// over the n block rows is what one workgroup used to walk alone (118 KB of band row per step through one CU: 27 ms on
// L_50_R_5).  Now the band row of a block row is split at the panel boundary:
//   k_band_panel   everything OUTSIDE the panel (blocks solved by earlier panels): one workgroup per (block row, chunk of
//                  the band row), NF waves = the NF rows of the block, partial sums to `part` (summed in fixed order by the
//                  next kernel: bitwise repeatable, no atomics);
//   k_band_tri     the kBandPanel x kBandPanel block triangle INSIDE the panel: one workgroup per member, D_k^-1 and the
//                  panel's vectors in LDS; a step is products -> wave sums -> barrier -> D_k^-1 (NF threads) -> barrier.  The
//                  triangle comes in as the policy says (S::kTriangleInRegisters): whole, before the chain starts (real: 48
//                  doubles per lane), or one block row ahead of the chain (complex: the whole would be 96).
// y holds rhs in elimination order on entry of the forward sweep, y after it and x (elimination order) after the backward
// sweep, which also scatters x to internal node order.
constexpr int kBandPanel = 16;
constexpr int kBandChunks = 4;      // chunks of the outside part of a band row (one workgroup each)

// grid (ceil(n NF / 256), batch): y = rhs in elimination order
template <int NF, class S>
__global__ __launch_bounds__(256) void k_band_gather(const BandView<S> lu, const typename S::Store* __restrict__ rhs, typename S::Store* __restrict__ y) {
  const int f = S::kBatched ? blockIdx.y : 0;
  if (!band_live(lu, f)) return;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= lu.n * NF) return;
  const int k = idx / NF;
  y[(size_t)f * lu.vec_stride + idx] = rhs[(size_t)f * lu.vec_stride + (size_t)lu.lu_node[k] * NF + (idx - k * NF)];
}

// grid (K1 - K0, kBandChunks, batch).  FWD: blocks [max(0, k-b), K0) of block row k; backward: blocks [K1, min(k+b, n-1)].
template <int NF, class S, bool FWD>
__global__ __launch_bounds__(NF * kWave) void k_band_panel(const BandView<S> lu, const typename S::Store* __restrict__ y, typename S::Store* __restrict__ part,
                                                            const int K0, const int K1) {
  using T = typename S::Store;
  using V = typename S::Val;
  constexpr int U = S::kDotBatch, BB = NF * NF;
  const int f = S::kBatched ? blockIdx.z : 0;
  if (!band_live(lu, f)) return;
  const int t = threadIdx.x, wv = t / kWave, lane = t - wv * kWave;
  const int kk = blockIdx.x, ch = blockIdx.y, k = K0 + kk;
  const int q_lo = FWD ? max(0, k - lu.b) : K1, q_hi = FWD ? K0 : min(k + lu.b, lu.n - 1) + 1;
  const int nblk = max(q_hi - q_lo, 0), per = (nblk + kBandChunks - 1) / kBandChunks;
  const int c_lo = q_lo + ch * per, c_hi = min(c_lo + per, q_hi);
  const int count = max(c_hi - c_lo, 0) * NF, last = max(count - 1, 0);
  V acc = S::real(0.0);
  if (count > 0) {   // uniform per workgroup
    const T* row = band_at<NF>(lu, f, k, c_lo) + wv * NF;                      // row wv of the blocks: NF entries every BB
    const T* yv = y + (size_t)f * lu.vec_stride + (size_t)c_lo * NF;           // entry (qo, j) of the row meets y[(c_lo + qo) * NF + j]
    for (int base = 0; base < count; base += U * kWave) {
      V w[U], z[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int idx = min(base + u * kWave + lane, last), qo = idx / NF, jj = idx - qo * NF;
        w[u] = S::ld(row + (size_t)qo * BB + jj); z[u] = S::ld(yv + idx);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) acc = S::dot(acc, base + u * kWave + lane < count, w[u], z[u]);
    }
  }
  acc = S::wsum(acc);
  if (lane == kWave - 1) S::st(part + (size_t)f * lu.part_stride + ((size_t)kk * kBandChunks + ch) * NF + wv, acc);
}

// grid (batch): one workgroup per member; np = K1 - K0 <= kBandPanel block rows.  Step s solves block row K0 + s (forward) /
// K1 - 1 - s (backward): s blocks of the panel stand in its band row either way.
template <int NF, class S, bool FWD>
__global__ __launch_bounds__(NF * kWave) void k_band_tri(const BandView<S> lu, typename S::Store* __restrict__ y_all, const typename S::Store* __restrict__ part_all,
                                                          typename S::Store* __restrict__ x_all, const int K0, const int K1) {
  using T = typename S::Store;
  using V = typename S::Val;
  constexpr int P = kBandPanel, BB = NF * NF, UM = ((P - 1) * NF + kWave - 1) / kWave;
  constexpr bool WHOLE = S::kTriangleInRegisters;
  __shared__ T yp[P * NF];   // the panel's solution blocks
  __shared__ T dl[P * BB];   // D_k^-1
  __shared__ T rh[P * NF];   // forward: rhs_k - outside sum; backward: outside sum
  __shared__ T yk[P * NF];   // backward: y_k
  __shared__ T st[NF];
  const int f = S::kBatched ? blockIdx.x : 0;
  if (!band_live(lu, f)) return;
  const int t = threadIdx.x, wv = t / kWave, lane = t - wv * kWave;
  const int np = K1 - K0;
  T* y = y_all + (size_t)f * lu.vec_stride;
  const T* part = part_all + (size_t)f * lu.part_stride;
  // the s in-panel blocks of the row solved at step s (s >= 1): clamped indices, no address outside the band is formed
  auto load_row = [&](int s, V (&w)[UM]) {
    const int sc = min(s, np - 1), k = FWD ? K0 + sc : K1 - 1 - sc;
    const T* row = (FWD ? band_at<NF>(lu, f, k, K0) : band_at<NF>(lu, f, k, min(k + 1, lu.n - 1))) + wv * NF;
    const int last = max(sc * NF - 1, 0);
#pragma unroll
    for (int u = 0; u < UM; ++u) {
      const int idx = min(u * kWave + lane, last), qo = idx / NF, jj = idx - qo * NF;
      w[u] = (np > 1) ? S::ld(row + (size_t)qo * BB + jj) : S::real(0.0);
    }
  };
  // one step of the chain with its row's in-panel entries in w
  auto solve_row = [&](int s, const V (&w)[UM]) {
    const int kk = FWD ? s : np - 1 - s;
    const T* ys = yp + (FWD ? 0 : (kk + 1) * NF);   // entry (qo, j) of the in-panel row meets ys[qo * NF + j]
    V acc = S::real(0.0);
    if (s > 0) {
#pragma unroll
      for (int u = 0; u < UM; ++u)
        if (u * kWave < s * NF) {   // (compile time where the triangle is in registers)
          const int raw = u * kWave + lane;
          acc = S::dot(acc, raw < s * NF, w[u], S::ld(ys + min(raw, s * NF - 1)));
        }
      acc = S::wsum(acc);
    }
    if (lane == kWave - 1) { const V h = S::ld(rh + kk * NF + wv); S::st(st + wv, FWD ? S::sub(h, acc) : S::add(h, acc)); }
    __syncthreads();
    if (t < NF) {
      V r = S::real(0.0);
#pragma unroll
      for (int m = 0; m < NF; ++m) r = S::mac(r, S::ld(dl + kk * BB + t * NF + m), S::ld(st + m));
      if (!FWD) r = S::sub(S::ld(yk + kk * NF + t), r);
      S::st(yp + kk * NF + t, r);
    }
    __syncthreads();
  };
  // every global operand first: the triangle (registers) or its first row, then D^-1, the outside sums and the panel's y
  V v[WHOLE ? P : 2][UM];   // WHOLE: row s in v[s]; otherwise v[0] the row being solved, v[1] the next
  if constexpr (WHOLE) {
#pragma unroll
    for (int s = 1; s < P; ++s) load_row(s, v[s]);
  } else {
#pragma unroll
    for (int u = 0; u < UM; ++u) v[1][u] = S::real(0.0);
  }
  for (int idx = t; idx < np * BB; idx += NF * kWave) dl[idx] = lu.dinv[(size_t)f * lu.dinv_stride + (size_t)K0 * BB + idx];
  if (t < np * NF) {
    const int kk = t / NF;
    V sacc = S::real(0.0);
#pragma unroll
    for (int c = 0; c < kBandChunks; ++c) sacc = S::add(sacc, S::ld(part + ((size_t)kk * kBandChunks + c) * NF + (t - kk * NF)));
    const V yv = S::ld(y + (size_t)K0 * NF + t);
    S::st(rh + t, FWD ? S::sub(yv, sacc) : sacc);
    if (!FWD) S::st(yk + t, yv);
  }
  __syncthreads();
  if constexpr (WHOLE) {
#pragma unroll
    for (int s = 0; s < P; ++s)
      if (s < np) solve_row(s, v[s]);   // uniform
  } else {
    for (int s = 0; s < np; ++s) {
#pragma unroll
      for (int u = 0; u < UM; ++u) v[0][u] = v[1][u];
      if (s + 1 < np) load_row(s + 1, v[1]);
      solve_row(s, v[0]);
    }
  }
  // results leave in one piece (a global store inside the chain would be drained at every barrier)
  if (t < np * NF) {
    const int kk = t / NF;
    const T r = yp[t];
    y[(size_t)K0 * NF + t] = r;
    if (!FWD) x_all[(size_t)f * lu.vec_stride + (size_t)lu.lu_node[K0 + kk] * NF + (t - kk * NF)] = r;
  }
}

}  // namespace gmpnp
