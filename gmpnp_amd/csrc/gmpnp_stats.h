// Exact order statistics of vertex columns of the state on the device: gmpnp_column_select / gmpnp_group_column_select
// (include/gmpnp.h).  The reference's time loop takes np.median of four ion-concentration columns and min() of the CO2 column
// every step (3D/MPNP_CO2ER_pore.py:817-838); on a partitioned state these are order statistics over every rank's owned rows.
//
// Radix select on the order-preserving 64-bit key of each double (sign bit set: all bits flipped; else the sign bit set; -0.0 keys
// as +0.0): 8 passes of 8 bits, most significant byte first.  A pass is
//     ONE histogram launch over the owned rows of all local handles and all selections (LDS-private 256-bin counters per workgroup,
//     written out as per-workgroup rows)  ->  one launch that sums the rows into a 256 x n count buffer (doubles: exact integers)
//     ->  one all-reduce of the counts over the group's transport (group_allreduce)  ->  one small launch that picks, per selection,
//     the bucket holding the remaining rank and appends it to the key prefix.
// Counts are integers, so the result does not depend on the rank count, the transport or the order of anything.  Everything is
// stream-ordered behind the solve; the host waits once, for the values.  Included at the end of gmpnp_api.hip (after
// gmpnp_group.h, whose group_allreduce it uses).
#pragma once

namespace gmpnp {

constexpr int kSelBins = 256;
constexpr int kSelLds = 16;              // selections one histogram launch counts (kSelLds x 256 LDS counters: 16 KiB)
constexpr int kSelNodesPerBlock = 1024;  // owned rows per histogram workgroup
constexpr int kSelMax = 64;              // selections per call

// the local handles of one histogram launch (blockIdx.y): owned rows of u (internal order)
struct SelDoms { const double* u[8]; int32_t own0[8]; int32_t nown[8]; };

// per-call state, device and pinned host image alike
struct SelIo {
  int32_t field[kSelMax];
  int32_t flags[kSelMax];              // bit 0: the column holds a NaN, bit 1: rank >= the global row count
  long long krem[kSelMax];             // rank still to find inside the current prefix's bucket
  unsigned long long prefix[kSelMax];  // key bits found so far
  double out[kSelMax];
};

__device__ inline unsigned long long sel_key(double v) {
  unsigned long long b = (unsigned long long)__double_as_longlong(v);
  if (b == 0x8000000000000000ull) b = 0ull;   // -0.0 -> +0.0: a column with both zeros gives NumPy's value
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ inline double sel_value(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// counts of the byte at `shift` among the keys that match the prefix above it, selections [sel0, sel0 + nsel); part rows
// [(d * gridDim.x + block) * n + j][256]; with part_nan (first pass) also the NaNs of each column
__global__ __launch_bounds__(256) void k_sel_hist(const SelDoms doms, int nf, const SelIo* __restrict__ io, int sel0, int nsel, int n, int shift,
                                                  uint32_t* __restrict__ part, uint32_t* __restrict__ part_nan) {
  __shared__ uint32_t h[kSelLds * kSelBins];
  __shared__ uint32_t hn[kSelLds];
  const int d = blockIdx.y, tid = threadIdx.x;
  for (int i = tid; i < nsel * kSelBins; i += 256) h[i] = 0u;
  if (tid < kSelLds) hn[tid] = 0u;
  __syncthreads();
  const unsigned long long himask = shift >= 56 ? 0ull : (~0ull << (shift + 8));
  const int nown = doms.nown[d], i0 = blockIdx.x * kSelNodesPerBlock, i1 = min(nown, i0 + kSelNodesPerBlock);
  const double* u = doms.u[d] + (size_t)doms.own0[d] * nf;
  for (int j = 0; j < nsel; ++j) {
    const int f = io->field[sel0 + j];
    const unsigned long long pre = io->prefix[sel0 + j];
    for (int i = i0 + tid; i < i1; i += 256) {
      const double v = u[(size_t)i * nf + f];
      const unsigned long long k = sel_key(v);
      if (((k ^ pre) & himask) == 0ull) atomicAdd(&h[j * kSelBins + (int)((k >> shift) & 255ull)], 1u);
      if (part_nan && v != v) atomicAdd(&hn[j], 1u);
    }
  }
  __syncthreads();
  const size_t row = (size_t)(d * gridDim.x + blockIdx.x) * n + sel0;
  for (int i = tid; i < nsel * kSelBins; i += 256) part[row * kSelBins + i] = h[i];
  if (part_nan && tid < nsel) part_nan[row + tid] = hn[tid];
}

// cnt[d][j * 256 + b] = sum over the workgroups of handle d; with part_nan also cnt[d][n * 256 + j] = its NaNs
__global__ __launch_bounds__(256) void k_sel_sum(const uint32_t* __restrict__ part, const uint32_t* __restrict__ part_nan, int nblk, int n,
                                                 const PtrList cnt) {
  const int j = blockIdx.x, d = blockIdx.y, b = threadIdx.x;
  unsigned long long s = 0;
  for (int k = 0; k < nblk; ++k) s += part[((size_t)(d * nblk + k) * n + j) * kSelBins + b];
  cnt.p[d][j * kSelBins + b] = (double)s;
  if (part_nan && b == 0) {
    unsigned long long q = 0;
    for (int k = 0; k < nblk; ++k) q += part_nan[(size_t)(d * nblk + k) * n + j];
    cnt.p[d][n * kSelBins + j] = (double)q;
  }
}

// one workgroup per selection: the bucket b with  excl(b) <= krem < incl(b)  over the all-reduced counts; the last pass leaves the value
__global__ __launch_bounds__(256) void k_sel_pick(const double* __restrict__ cnt, int n, int shift, int with_nan, SelIo* __restrict__ io) {
  __shared__ long long sc[kSelBins];
  const int j = blockIdx.x, b = threadIdx.x;
  const long long c = (long long)cnt[j * kSelBins + b];
  const long long k = io->krem[j];
  sc[b] = c;
  __syncthreads();
  for (int o = 1; o < kSelBins; o <<= 1) {   // inclusive scan
    const long long t = b >= o ? sc[b - o] : 0;
    __syncthreads();
    sc[b] += t;
    __syncthreads();
  }
  const long long incl = sc[b], excl = incl - c;
  if (excl <= k && k < incl) {
    const unsigned long long pre = io->prefix[j] | ((unsigned long long)b << shift);
    io->prefix[j] = pre;
    io->krem[j] = k - excl;
    if (shift == 0) io->out[j] = sel_value(pre);
  }
  if (b == kSelBins - 1) {
    int f = io->flags[j];
    if (with_nan && cnt[n * kSelBins + j] > 0.0) f |= 1;
    if (k >= incl) f |= 2;
    io->flags[j] = f;
  }
}

}  // namespace gmpnp

namespace {

// The selections over the owned rows of `dom` (one process's handles; g = their group, nullptr for one handle on its own)
int column_select(const std::vector<gmpnp_solver*>& dom, gmpnp_group* g, int32_t n, const int32_t* field, const int64_t* rank, double* out,
                  int32_t* flags) {
  if (n < 1 || n > kSelMax || !field || !rank || !out || !flags) return fail(GMPNP_ERR_INVALID, "column select: bad arguments (1 ... 64 selections)");
  gmpnp_solver* s0 = dom[0];
  const int nf = s0->nf;
  for (int j = 0; j < n; ++j) {
    if (field[j] < 0 || field[j] >= nf) return fail(GMPNP_ERR_INVALID, "column select: field out of range");
    if (rank[j] < 0) return fail(GMPNP_ERR_INVALID, "column select: negative rank");
  }
  HIP_TRY(hipSetDevice(s0->opts.device_id));
  hipStream_t st = s0->stream;   // (an in-process group runs all its handles on dom[0]'s stream)
  int max_own = 0;
  for (gmpnp_solver* s : dom) max_own = std::max(max_own, s->t.own_node1 - s->t.own_node0);
  const int nblk = std::max(1, grid_for(max_own, kSelNodesPerBlock));
  const int ndom = (int)dom.size();
  for (gmpnp_solver* s : dom) {
    if (!s->selector) s->selector.reset(new gmpnp_selector);
    gmpnp_selector* q = s->selector.get();
    if (q->cnt.n < (size_t)kSelMax * (kSelBins + 1)) HIP_TRY(q->cnt.alloc((size_t)kSelMax * (kSelBins + 1)));
  }
  gmpnp_selector* q0 = s0->selector.get();
  const size_t npart = (size_t)ndom * nblk * n;
  if (q0->part.n < npart * kSelBins) HIP_TRY(q0->part.alloc(npart * kSelBins, false));
  if (q0->part_nan.n < npart) HIP_TRY(q0->part_nan.alloc(npart, false));
  if (!q0->h_io) {
    HIP_TRY(hipHostMalloc(&q0->h_io, sizeof(SelIo)));
    HIP_TRY(q0->io.alloc(sizeof(SelIo)));
  }
  SelIo* hio = static_cast<SelIo*>(q0->h_io);
  SelIo* dio = reinterpret_cast<SelIo*>(q0->io.p);
  std::memset(hio, 0, sizeof(SelIo));   // (free: the previous call waited for its read-back)
  for (int j = 0; j < n; ++j) { hio->field[j] = field[j]; hio->krem[j] = (long long)rank[j]; }
  HIP_TRY(hipMemcpyAsync(dio, hio, sizeof(SelIo), hipMemcpyHostToDevice, st));
  SelDoms sd{};
  PtrList cnt{};
  for (int d = 0; d < ndom; ++d) {
    gmpnp_solver* s = dom[d];
    sd.u[d] = s->u.p; sd.own0[d] = s->t.own_node0; sd.nown[d] = s->t.own_node1 - s->t.own_node0;
    cnt.p[d] = s->selector->cnt.p;
  }
  // all-reduce in pieces the transport's staging holds (peer mailbox slot, host-staged buffer)
  const size_t cap = !g ? 0 : g->peer ? (size_t)g->pa.red_cap : g->hosted ? g->h_stage_n : ~(size_t)0;
  for (int pass = 0; pass < 8; ++pass) {
    const int shift = 56 - 8 * pass;
    uint32_t* pn = pass == 0 ? q0->part_nan.p : nullptr;
    for (int j0 = 0; j0 < n; j0 += kSelLds)
      hipLaunchKernelGGL(k_sel_hist, dim3(nblk, ndom), dim3(256), 0, st, sd, nf, (const SelIo*)dio, j0, std::min(kSelLds, n - j0), (int)n, shift,
                         q0->part.p, pn);
    hipLaunchKernelGGL(k_sel_sum, dim3(n, ndom), dim3(256), 0, st, (const uint32_t*)q0->part.p, (const uint32_t*)pn, nblk, (int)n, cnt);
    HIP_TRY(hipGetLastError());
    if (g) {
      const size_t len = (size_t)n * kSelBins + (pass == 0 ? n : 0);
      for (size_t off = 0; off < len; off += cap) {
        const int m = (int)std::min(cap, len - off);
        int rc = group_allreduce(g, [off](gmpnp_solver* s) { return s->selector->cnt.p + off; }, m); if (rc) return rc;
      }
    }
    hipLaunchKernelGGL(k_sel_pick, dim3(n), dim3(256), 0, st, (const double*)q0->cnt.p, (int)n, shift, pass == 0 ? 1 : 0, dio);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipMemcpyAsync(hio, dio, sizeof(SelIo), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (g) { int rc = peer_check(g); if (rc) return rc; }
  int f = 0;
  for (int j = 0; j < n; ++j) { out[j] = hio->out[j]; f |= hio->flags[j]; }
  if (f & 2) return fail(GMPNP_ERR_INVALID, "column select: a rank is not below the number of owned rows");
  *flags = f & 1;
  return GMPNP_OK;
}

}  // namespace

extern "C" {

int gmpnp_column_select(gmpnp_solver* s, int32_t n, const int32_t* field, const int64_t* rank, double* out, int32_t* flags) {
  if (!s) return fail(GMPNP_ERR_INVALID, "NULL handle");
  return column_select({s}, nullptr, n, field, rank, out, flags);
}

int gmpnp_group_column_select(gmpnp_group* g, int32_t n, const int32_t* field, const int64_t* rank, double* out, int32_t* flags) {
  if (!g) return fail(GMPNP_ERR_INVALID, "NULL group");
  if (g->ml_level) return fail(GMPNP_ERR_INVALID, "this group is a coarse level of a multilevel term");
  return column_select(g->dom, g, n, field, rank, out, flags);
}

}  // extern "C"
