  using L = Lay<DIM, NF>;
  constexpr int NS = L::NS, NN = L::NN;
  static_assert(!STAGED || DIM == 3, "staged record stores: 3D meshes");
  __shared__ double stage[STAGED ? 64 * kStagePitch : 1];
  // Coefficient and quadrature tables go to LDS first: read through the global pointers they would be re-fetched with
  // a vector load (and a full wait) at every use, because the element stores below may alias them.
  __shared__ gmpnp_model_t m;
  __shared__ gmpnp_quadrature_t qd;
  {
    static_assert(sizeof(gmpnp_model_t) % 4 == 0 && sizeof(gmpnp_quadrature_t) % 4 == 0, "word-wise staging");
    const uint32_t* gm = reinterpret_cast<const uint32_t*>(c.model);
    const uint32_t* gq = reinterpret_cast<const uint32_t*>(c.quad);
    uint32_t* lm = reinterpret_cast<uint32_t*>(&m);
    uint32_t* lq = reinterpret_cast<uint32_t*>(&qd);
    for (int w = threadIdx.x; w < (int)(sizeof(gmpnp_model_t) / 4); w += blockDim.x) lm[w] = gm[w];
    for (int w = threadIdx.x; w < (int)(sizeof(gmpnp_quadrature_t) / 4); w += blockDim.x) lq[w] = gq[w];
  }
  __syncthreads();
  const int e0 = blockIdx.x * blockDim.x;
  if (!STAGED && e0 + (int)threadIdx.x >= c.nc) return;
  const int e = min(e0 + (int)threadIdx.x, c.nc - 1);   // STAGED: every lane stays for the copy-out (surplus lanes redo the last cell; never stored)

  int nd[NN];
  double X[NN][DIM], U[NN][NF];
#pragma unroll
  for (int a = 0; a < NN; ++a) {
    nd[a] = c.cells[e * NN + a];
#pragma unroll
    for (int d = 0; d < DIM; ++d) X[a][d] = c.coords[(size_t)nd[a] * DIM + d];
#pragma unroll
    for (int f = 0; f < NF; ++f) U[a][f] = c.u[(size_t)nd[a] * NF + f];
  }
  // geometry: |K| and the constant gradients of the P1 basis
  double g[NN][DIM], vol;
  if constexpr (DIM == 1) {
    const double h = X[1][0] - X[0][0];
    g[0][0] = -1.0 / h; g[1][0] = 1.0 / h; vol = fabs(h);
  } else {
    double T[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int d = 0; d < 3; ++d) T[r][d] = X[r + 1][d] - X[0][d];
    const double c00 = T[1][1] * T[2][2] - T[1][2] * T[2][1];
    const double c01 = T[1][2] * T[2][0] - T[1][0] * T[2][2];
    const double c02 = T[1][0] * T[2][1] - T[1][1] * T[2][0];
    const double det = T[0][0] * c00 + T[0][1] * c01 + T[0][2] * c02;
    const double id = 1.0 / det;
    // columns of T^{-1} are grad phi_1..3
    g[1][0] = c00 * id; g[1][1] = c01 * id; g[1][2] = c02 * id;
    g[2][0] = (T[0][2] * T[2][1] - T[0][1] * T[2][2]) * id;
    g[2][1] = (T[0][0] * T[2][2] - T[0][2] * T[2][0]) * id;
    g[2][2] = (T[0][1] * T[2][0] - T[0][0] * T[2][1]) * id;
    g[3][0] = (T[0][1] * T[1][2] - T[0][2] * T[1][1]) * id;
    g[3][1] = (T[0][2] * T[1][0] - T[0][0] * T[1][2]) * id;
    g[3][2] = (T[0][0] * T[1][1] - T[0][1] * T[1][0]) * id;
#pragma unroll
    for (int d = 0; d < 3; ++d) g[0][d] = -(g[1][d] + g[2][d] + g[3][d]);
    vol = fabs(det) * (1.0 / 6.0);
  }
  double gg[NN][NN];
#pragma unroll
  for (int a = 0; a < NN; ++a)
#pragma unroll
    for (int b = 0; b < NN; ++b) {
      double s = 0.0;
#pragma unroll
      for (int d = 0; d < DIM; ++d) s += g[a][d] * g[b][d];
      gg[a][b] = s;
    }
  double gradp[DIM], G[DIM];
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    double sp = 0.0, sg = 0.0;
#pragma unroll
    for (int a = 0; a < NN; ++a) {
      sp += U[a][NS] * g[a][d];
      double au = 0.0;
#pragma unroll
      for (int j = 0; j < NS; ++j) au += m.a[j] * U[a][j];
      sg += au * g[a][d];
    }
    gradp[d] = sp; G[d] = sg;
  }
  double gp[NN], Gg[NN];
#pragma unroll
  for (int a = 0; a < NN; ++a) {
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int d = 0; d < DIM; ++d) { s1 += gradp[d] * g[a][d]; s2 += G[d] * g[a][d]; }
    gp[a] = s1; Gg[a] = s2;
  }
  double usum[NS], ubar[NS], epsbar = m.eps0;
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    double s = 0.0;
#pragma unroll
    for (int a = 0; a < NN; ++a) s += U[a][j];
    usum[j] = s; ubar[j] = s * (1.0 / NN); epsbar += m.epsc[j] * ubar[j];
  }
  // steric moments
  double If[NS], Ij[NS], Bq[NN], Cq[NS][NN];
#pragma unroll
  for (int j = 0; j < NS; ++j) { If[j] = 0.0; Ij[j] = 0.0;
#pragma unroll
    for (int b = 0; b < NN; ++b) Cq[j][b] = 0.0; }
#pragma unroll
  for (int b = 0; b < NN; ++b) Bq[b] = 0.0;
  bool bad = false;
  if (m.steric) {
    for (int q = 0; q < qd.nq_f; ++q) {
      double uq[NS], S = 0.0;
#pragma unroll
      for (int j = 0; j < NS; ++j) {
        double s = 0.0;
#pragma unroll
        for (int b = 0; b < NN; ++b) s += qd.lam_f[q][b] * U[b][j];
        uq[j] = s; S += m.a[j] * s;
      }
      bad |= !(1.0 - S > 0.0);
      const double wb = qd.w_f[q] * vol / (1.0 - S);
#pragma unroll
      for (int j = 0; j < NS; ++j) If[j] += wb * uq[j];
    }
    if constexpr (WANT_J) {
      for (int q = 0; q < qd.nq_j; ++q) {
        double uq[NS], S = 0.0;
#pragma unroll
        for (int j = 0; j < NS; ++j) {
          double s = 0.0;
#pragma unroll
          for (int b = 0; b < NN; ++b) s += qd.lam_j[q][b] * U[b][j];
          uq[j] = s; S += m.a[j] * s;
        }
        bad |= !(1.0 - S > 0.0);
        const double beta = 1.0 / (1.0 - S);
        const double wb = qd.w_j[q] * vol * beta;
#pragma unroll
        for (int b = 0; b < NN; ++b) Bq[b] += wb * qd.lam_j[q][b];
#pragma unroll
        for (int j = 0; j < NS; ++j) {
          Ij[j] += wb * uq[j];
          const double wbb = wb * beta * uq[j];
#pragma unroll
          for (int b = 0; b < NN; ++b) Cq[j][b] += wbb * qd.lam_j[q][b];
        }
      }
    }
  }
  if (bad) atomicOr(c.status, 1);

  // ---- element residual ------------------------------------------------------------------------
  double* ef = c.EF + (size_t)e * L::EF_STRIDE;
  // bilinear monomials int u_x u_y phi_a = |K| kappa (XY + x_a Y + X y_a + D + 2 x_a y_a)
  double mono[GMPNP_MAX_BILINEAR][NN];
  for (int t = 0; t < m.n_bilinear; ++t) {
    const int bj = m.bil_j[t], bk = m.bil_k[t];
    double xs[NN], ys[NN], Xs = 0.0, Ys = 0.0, D = 0.0;
#pragma unroll
    for (int a = 0; a < NN; ++a) {
      double xv = 0.0, yv = 0.0;
#pragma unroll
      for (int j = 0; j < NS; ++j) { xv = (j == bj) ? U[a][j] : xv; yv = (j == bk) ? U[a][j] : yv; }
      xs[a] = xv; ys[a] = yv; Xs += xv; Ys += yv; D += xv * yv;
    }
#pragma unroll
    for (int a = 0; a < NN; ++a)
      mono[t][a] = vol * L::KAPPA * (Xs * Ys + xs[a] * Ys + Xs * ys[a] + D + 2.0 * xs[a] * ys[a]);
    if constexpr (WANT_J) {  // derivative tables of the monomial: the Jacobian gather reads two numbers per term
      double* dt = c.EJ + (size_t)e * L::EJ_STRIDE + L::O_D + t * 2 * NN * NN;
      const int sp = (t & 1) * 2 * NN * NN;   // STAGED: two terms (2 x 32 words) share a piece
#pragma unroll
      for (int a = 0; a < NN; ++a)
#pragma unroll
        for (int b = 0; b < NN; ++b) {
          elem_put<STAGED>(dt, stage, sp + a * NN + b, a * NN + b, vol * L::KAPPA * (Ys + ys[a] + ys[b] + (a == b ? Ys + 2.0 * ys[a] : 0.0)));            // d/d u_{bj,b}
          elem_put<STAGED>(dt, stage, sp + NN * NN + a * NN + b, NN * NN + a * NN + b, vol * L::KAPPA * (Xs + xs[a] + xs[b] + (a == b ? Xs + 2.0 * xs[a] : 0.0)));  // d/d u_{bk,b}
        }
      if constexpr (STAGED) {
        static_assert(!STAGED || 4 * NN * NN <= kStageWords, "two terms per piece");
        if ((t & 1) || t + 1 == m.n_bilinear)
          elem_flush(c.EJ, L::EJ_STRIDE, L::O_D + (t & ~1) * 2 * NN * NN, ((t & 1) ? 4 : 2) * NN * NN, stage, e0, c.nc);
      }
    }
  }
#pragma unroll
  for (int a = 0; a < NN; ++a) {
    double fp = -epsbar * vol * gp[a];
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      // M-weighted nodal sums: sum_b M_ab w_b = |K| MDEN (sum_b w_b + w_a)
      double du_sum = 0.0;
#pragma unroll
      for (int b = 0; b < NN; ++b) du_sum += U[b][i] - c.un[(size_t)nd[b] * NF + i];
      const double du_a = U[a][i] - c.un[(size_t)nd[a] * NF + i];
      double f = m.inv_dt * vol * L::MDEN * (du_sum + du_a);
      double ku = 0.0;
#pragma unroll
      for (int b = 0; b < NN; ++b) ku += gg[a][b] * U[b][i];
      f += vol * ku;
      f += m.z[i] * vol * ubar[i] * gp[a];
      f += m.rc0[i] * vol * (1.0 / NN);
#pragma unroll
      for (int j = 0; j < NS; ++j) f += m.rc1[i][j] * (vol * L::MDEN * (usum[j] + U[a][j]));
      for (int t = 0; t < m.n_bilinear; ++t) f += m.rc2[i][t] * mono[t][a];
      f += If[i] * Gg[a];
      elem_put<STAGED>(ef, stage, a * NF + i, a * NF + i, f);
      fp += m.qzb[i] * (vol * L::MDEN * (usum[i] + U[a][i]));
    }
    elem_put<STAGED>(ef, stage, a * NF + NS, a * NF + NS, fp);
  }
  if constexpr (STAGED) {
    static_assert(!STAGED || L::EF_STRIDE <= kStageWords, "the residual rows are one piece");
    elem_flush(c.EF, L::EF_STRIDE, 0, L::EF_STRIDE, stage, e0, c.nc);
  }
  // ---- SUPG stabilisation of the PNP model (reference 1D:687-714; 1D meshes only) -----------------------------------
  //   F_stab = - sum_i rho_i z_i [ (u_i - u_i^n)/(dt L_D) + z_i grad(w_i).grad(p) + R_i ] grad(p).grad(v_i) dx
  // rho_i: nodal (P1), w_i = u_i except the reference's OH term, which takes grad(u_H) (SURVEY Q7; c.supg_w); R_i the
  // production rate (the tables hold -R_i).  Degree <= 3 on a P1 element: closed form.  The element matrix of these
  // terms is dense in (species, potential) and is stored whole (196 doubles) for the Jacobian gather.
  if constexpr (DIM == 1) {
    if (c.supg_rho) {
      double* js = nullptr;
      if constexpr (WANT_J) {
        js = c.EJ + (size_t)e * L::EJ_STRIDE + L::O_S;
        for (int q = 0; q < NN * NF * NN * NF; ++q) js[q] = 0.0;
      }
      for (int i = 0; i < NS; ++i) {
        const double zi = m.z[i];
        if (zi == 0.0) continue;
        const int wi = c.supg_w[i];
        double rho[NN], du[NN], uw[NN];
#pragma unroll
        for (int a = 0; a < NN; ++a) {
          rho[a] = c.supg_rho[(size_t)nd[a] * NS + i];
          du[a] = U[a][i] - c.un[(size_t)nd[a] * NF + i];
          double v = 0.0;
#pragma unroll
          for (int j = 0; j < NS; ++j) v = (j == wi) ? U[a][j] : v;
          uw[a] = v;
        }
        double rsum = 0.0, gradw = 0.0;
#pragma unroll
        for (int a = 0; a < NN; ++a) { rsum += rho[a]; gradw += uw[a] * g[a][0]; }
        const double rbar = rsum * (1.0 / NN);
        double rM[NN];
#pragma unroll
        for (int b = 0; b < NN; ++b) rM[b] = vol * L::MDEN * (rsum + rho[b]);
        double S = zi * (gradw * gradp[0]) * vol * rbar - m.rc0[i] * vol * rbar;
#pragma unroll
        for (int b = 0; b < NN; ++b) S += m.inv_dt * rM[b] * du[b];
        for (int j = 0; j < NS; ++j) {
          const double c1 = m.rc1[i][j];
          if (c1 != 0.0)
#pragma unroll
            for (int b = 0; b < NN; ++b) S -= c1 * rM[b] * U[b][j];
        }
        // bilinear terms: sum_abc rho_a x_b y_c T_abc |K|, T_abc = kappa (6 | 2 | 1 for three | two | no equal indices)
        double dSx[GMPNP_MAX_BILINEAR][NN], dSy[GMPNP_MAX_BILINEAR][NN];
        for (int t = 0; t < m.n_bilinear; ++t) {
          const double c2 = m.rc2[i][t];
          const int bj = m.bil_j[t], bk = m.bil_k[t];
          double xs[NN], ys[NN];
#pragma unroll
          for (int a = 0; a < NN; ++a) {
            double xv = 0.0, yv = 0.0;
#pragma unroll
            for (int j = 0; j < NS; ++j) { xv = (j == bj) ? U[a][j] : xv; yv = (j == bk) ? U[a][j] : yv; }
            xs[a] = xv; ys[a] = yv;
          }
          double tot = 0.0;
#pragma unroll
          for (int b = 0; b < NN; ++b) { dSx[t][b] = 0.0; dSy[t][b] = 0.0; }
#pragma unroll
          for (int a = 0; a < NN; ++a)
#pragma unroll
            for (int b = 0; b < NN; ++b)
#pragma unroll
              for (int cc = 0; cc < NN; ++cc) {
                const double T = vol * L::KAPPA * ((a == b && b == cc) ? 6.0 : ((a == b || b == cc || a == cc) ? 2.0 : 1.0));
                tot += rho[a] * xs[b] * ys[cc] * T;
                dSx[t][b] += rho[a] * ys[cc] * T;   // d/d x_b
                dSy[t][cc] += rho[a] * xs[b] * T;   // d/d y_c
              }
          S -= c2 * tot;
        }
#pragma unroll
        for (int a = 0; a < NN; ++a) ef[a * NF + i] += -zi * gp[a] * S;
        if constexpr (WANT_J) {
#pragma unroll
          for (int b = 0; b < NN; ++b) {
            double dS[NF];
#pragma unroll
            for (int j = 0; j < NF; ++j) dS[j] = 0.0;
            for (int j = 0; j < NS; ++j) {
              double v = -m.rc1[i][j] * rM[b];
              if (j == i) v += m.inv_dt * rM[b];
              if (j == wi) v += zi * gp[b] * vol * rbar;
              for (int t = 0; t < m.n_bilinear; ++t) {
                const double c2 = m.rc2[i][t];
                if (j == m.bil_j[t]) v -= c2 * dSx[t][b];
                if (j == m.bil_k[t]) v -= c2 * dSy[t][b];
              }
              dS[j] = v;
            }
            const double dSp = zi * (gradw * g[b][0]) * vol * rbar;
#pragma unroll
            for (int a = 0; a < NN; ++a) {
              double* row = js + ((size_t)(a * NF + i) * NN + b) * NF;
              for (int j = 0; j < NS; ++j) row[j] = -zi * gp[a] * dS[j];
              row[NS] = -zi * (gg[a][b] * S + gp[a] * dSp);
            }
          }
        }
      }
    }
  }
  if constexpr (WANT_J) {
    double* ej = c.EJ + (size_t)e * L::EJ_STRIDE;
    // two pieces: [0, O_B) = volume, gradients, means, eps, int u beta; [O_B, O_D) = int beta phi, int u beta^2 phi
    elem_put<STAGED>(ej, stage, L::O_VOL, L::O_VOL, vol);
#pragma unroll
    for (int a = 0; a < NN; ++a) {
#pragma unroll
      for (int b = 0; b < NN; ++b) elem_put<STAGED>(ej, stage, L::O_GG + a * NN + b, L::O_GG + a * NN + b, gg[a][b]);
      elem_put<STAGED>(ej, stage, L::O_GP + a, L::O_GP + a, gp[a]);
      elem_put<STAGED>(ej, stage, L::O_GG_A + a, L::O_GG_A + a, Gg[a]);
    }
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      elem_put<STAGED>(ej, stage, L::O_UBAR + j, L::O_UBAR + j, ubar[j]);
      elem_put<STAGED>(ej, stage, L::O_IJ + j, L::O_IJ + j, Ij[j]);
    }
    elem_put<STAGED>(ej, stage, L::O_EPS, L::O_EPS, epsbar);
    if constexpr (STAGED) {
      static_assert(!STAGED || (L::O_B <= kStageWords && L::O_D - L::O_B <= kStageWords), "the record head is two pieces");
      elem_flush(c.EJ, L::EJ_STRIDE, 0, L::O_B, stage, e0, c.nc);
    }
#pragma unroll
    for (int a = 0; a < NN; ++a) elem_put<STAGED>(ej, stage, a, L::O_B + a, Bq[a]);
#pragma unroll
    for (int j = 0; j < NS; ++j)
#pragma unroll
      for (int b = 0; b < NN; ++b) elem_put<STAGED>(ej, stage, (L::O_C - L::O_B) + j * NN + b, L::O_C + j * NN + b, Cq[j][b]);
    if constexpr (STAGED) elem_flush(c.EJ, L::EJ_STRIDE, L::O_B, L::O_D - L::O_B, stage, e0, c.nc);
  }
