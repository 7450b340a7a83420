  using L = Lay<DIM, NF>;
  constexpr int NS = L::NS, NN = L::NN, G = 2, MB = GMPNP_MAX_BILINEAR;
  const int wave = xcd_run_wave(c), lane = threadIdx.x & 63;
  if (wave >= c.n_work) return;
  const int s = c.wl_slice[wave], kpos = c.wl_kpos[wave];
  if (s < 0) return;   // padding of a run
  const int Iloc = lane / NF, i = lane - Iloc * NF;
  if (Iloc >= c.slice_nn[s]) return;
  const int I = c.slice_node0[s] + Iloc;
  const int k = c.sell_blk[(size_t)(c.slice_colbase[s] + kpos) * kSlicePad + Iloc];
  if (k < 0) return;  // padding stays zero (set at create)
  const int J = c.cols[k];
  const int qb = c.cptr[k], qend = c.cptr[k + 1];
  int rob = -1;
  if constexpr (ROBIN) rob = c.rob_blk[k];   // requested with the block's other table entries, used behind the element sum
  const int bc = c.bcflag[I * NF + i];
  double* out = c.vals + c.slice_off[s] + (size_t)kpos * NF * kWave + lane;
  const gmpnp_model_t& m = *c.model;
  const bool isp = (i == NS);
  const int is = isp ? 0 : i;
  const double zi = m.z[is], inv_dt = m.inv_dt;
  double rc1i[NS], c2t[MB];
#pragma unroll
  for (int j = 0; j < NS; ++j) rc1i[j] = m.rc1[is][j];
#pragma unroll
  for (int t = 0; t < MB; ++t) { const double v = m.rc2[is][t]; c2t[t] = (t < m.n_bilinear && !isp) ? v : 0.0; }
  const int tmax = max(m.n_bilinear, 1) - 1;
  const int qe = bc ? qb : qend;  // Dirichlet rows take no contributions
  double acc[NF];
#pragma unroll
  for (int j = 0; j < NF; ++j) acc[j] = 0.0;

  // G contributions per trip; every value of a trip is requested before the first one is used (unconditional loads on
  // clamped indices, masked by w = 0/1), and the contribution codes of the NEXT trip are requested with them: one
  // memory round trip per trip instead of one per table.
  int pk[G];
#pragma unroll
  for (int u = 0; u < G; ++u) pk[u] = c.contrib[max(min(qb + u, qe - 1), 0)];
  for (int q0 = qb; q0 < qe; q0 += G) {
    double vol[G], ggab[G], gpa[G], gga[G], cq[G], ij[G], bq[G], ub[G], ep[G], dj[G][MB], dk[G][MB];
    int pa[G], pb[G];
#pragma unroll
    for (int u = 0; u < G; ++u) {
      const int e = pk[u] >> 4, a = (pk[u] >> 2) & 3, b = pk[u] & 3;
      const double* ej = c.EJ + (size_t)e * L::EJ_STRIDE;
      pa[u] = a; pb[u] = b;
      vol[u] = ej[L::O_VOL]; ggab[u] = ej[L::O_GG + a * NN + b]; gpa[u] = ej[L::O_GP + a]; gga[u] = ej[L::O_GG_A + a];
      cq[u] = ej[L::O_C + is * NN + b]; ij[u] = ej[L::O_IJ + is]; bq[u] = ej[L::O_B + b]; ub[u] = ej[L::O_UBAR + is];
      ep[u] = ej[L::O_EPS];
#pragma unroll
      for (int t = 0; t < MB; ++t) {
        const double* dt = ej + L::O_D + min(t, tmax) * 2 * NN * NN + a * NN + b;
        dj[u][t] = dt[0]; dk[u][t] = dt[NN * NN];
      }
    }
    int pkn[G];
#pragma unroll
    for (int u = 0; u < G; ++u) pkn[u] = c.contrib[max(min(q0 + G + u, qe - 1), 0)];
#pragma unroll
    for (int u = 0; u < G; ++u) {
      const double w = (q0 + u < qe) ? 1.0 : 0.0;
      const double Mab = vol[u] * L::MDEN * (pa[u] == pb[u] ? 2.0 : 1.0), Kab = vol[u] * ggab[u];
      if (!isp) {
        const double ster = gga[u] * cq[u] + ij[u] * ggab[u];
        const double dg = inv_dt * Mab + Kab + zi * vol[u] * (1.0 / NN) * gpa[u] + gga[u] * bq[u];
#pragma unroll
        for (int j = 0; j < NS; ++j) {
          double term = m.a[j] * ster + rc1i[j] * Mab + (j == is ? dg : 0.0);
#pragma unroll
          for (int t = 0; t < MB; ++t)  // c2t = 0 beyond n_bilinear
            term += (j == m.bil_j[t] ? c2t[t] * dj[u][t] : 0.0) + (j == m.bil_k[t] ? c2t[t] * dk[u][t] : 0.0);
          acc[j] += w * term;
        }
        acc[NS] += w * (zi * ub[u] * Kab);
      } else {
        const double kpa = vol[u] * gpa[u] * (1.0 / NN);
#pragma unroll
        for (int j = 0; j < NS; ++j) acc[j] += w * (-m.epsc[j] * kpa + m.qzb[j] * Mab);
        acc[NS] += w * (-ep[u] * Kab);
      }
    }
#pragma unroll
    for (int u = 0; u < G; ++u) pk[u] = pkn[u];
  }
  if constexpr (DIM == 1) {
    if (c.supg_rho) {  // dense SUPG element matrices (PNP + stabilisation), added after the regular terms in element order
      for (int q = qb; q < qe; ++q) {
        const int pk = c.contrib[q];
        const int e = pk >> 4, a = (pk >> 2) & 3, b = pk & 3;
        const double* row = c.EJ + (size_t)e * L::EJ_STRIDE + L::O_S + ((size_t)(a * NF + i) * NN + b) * NF;
#pragma unroll
        for (int j = 0; j < NF; ++j) acc[j] += row[j];
      }
    }
  }
  if constexpr (ROBIN) {
    // the block's Robin entries (species rows, diagonal of the block): the one addition k_robin_add makes, on the same operands
    if (rob >= 0 && !isp) {
      const double rv = c.rob_blk_val[(size_t)rob * NS + is];
      const bool has = (c.rob_blk_mask[rob] >> is) & 1;
#pragma unroll
      for (int j = 0; j < NS; ++j) if (j == is && has) acc[j] += rv;
    }
  }
  if (bc) {  // [3P] DirichletBC.apply(A): identity row
#pragma unroll
    for (int j = 0; j < NF; ++j) acc[j] = (J == I && j == i) ? 1.0 : 0.0;
  }
#pragma unroll
  for (int j = 0; j < NF; ++j) out[j * kWave] = acc[j];
