// Body of k_time_error2 (gmpnp_time_order.h), kept as text so that an ensemble kernel can share it later, as k_time_error_ens shares
// gmpnp_time_error_body.inc.  Expects `io` (a TimeError2Io) and NF in scope; the workgroup's node block is blockIdx.x.  The body of
// the order-1 estimator with the predictor formed while the rows stream in: LDS holds u, u_n and p, the order-1 footprint.
  constexpr int K = kTimeCols * NF;
  __shared__ double su[kVecBlock * NF], sn[kVecBlock * NF], sp[kVecBlock * NF];
  __shared__ uint8_t sb[kVecBlock * NF];
  __shared__ double red[4 * K];
  __shared__ double wl[kVecBlock / kWave];
  __shared__ int wd[kVecBlock / kWave];
  const int t = threadIdx.x, n0 = blockIdx.x * kVecBlock;
  const int cnt = min(kVecBlock, io.nv - n0) * NF;   // doubles of this workgroup's node blocks (gridDim.x = ceil(nv / 256): cnt > 0)
  const size_t base = (size_t)n0 * NF;
  int bad = 0;
  for (int k = t; k < cnt; k += kVecBlock) {
    const double x = io.u[base + k], xn = io.un[base + k];
    su[k] = x; sn[k] = xn; sb[k] = io.bcflag[base + k];
    sp[k] = io.wn * xn + io.wm1 * io.unm1[base + k] + io.wm2 * io.unm2[base + k];
    bad |= ((__double2hiint(x) & 0x7ff00000) == 0x7ff00000) ? 1 : 0;   // NaN or Inf
  }
  const int any_bad = __syncthreads_or(bad);
  double v[K];
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = 0.0;
  double worst = -1.0; int dof = -1;
  if (n0 + t < io.nv) {
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const int k = t * NF + f;
      if (sb[k]) continue;
      const double x = su[k], xn = sn[k];
      const double d = (x - sp[k]) * io.kappa;
      const double w = io.atol[f] + io.rtol * fmax(fabs(x), fabs(xn));
      const double q = d / w, r = (x - xn) * io.inv_h;
      v[f] = q * q; v[NF + f] = r * r; v[2 * NF + f] = 1.0;
      if (fabs(q) > worst) { worst = fabs(q); dof = (n0 + t) * NF + f; }   // fields ascend: a tie keeps the smaller dof
    }
  }
  block_sum<K>(v, red);
  wave_max_index(worst, dof);
  if ((t & (kWave - 1)) == 0) { wl[t >> 6] = worst; wd[t >> 6] = dof; }
  __syncthreads();
  if (t == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) io.part[(size_t)k * io.nblk + blockIdx.x] = v[k];
#pragma unroll
    for (int w = 1; w < kVecBlock / kWave; ++w)
      if (wl[w] > worst) { worst = wl[w]; dof = wd[w]; }   // the waves' dofs ascend: a tie keeps the smaller
    io.part_max[blockIdx.x] = worst;
    io.part_dof[blockIdx.x] = dof;
    io.part_bad[blockIdx.x] = any_bad;
  }
