// Host-side decisions that have no device in them: what a Newton residual means (one verdict for newton(), group_newton()
// and the ensemble driver), the predicted start of a linear solve, the policies of the linear solves inside Newton (coarse reuse,
// direct fallback, burst sizing), the options' resolution, and the tables of the geometric multilevel term.
// Includes gmpnp.h and the C++ standard library only, so it compiles (and is tested) with the host compiler alone.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "gmpnp.h"

namespace gmpnp {

// device status word: bit 1 = steric excursion (information, unless strict_steric), bits 2 / 4 / 8 = the linear solve failed,
// bit 16 = the step limiter met a NaN / Inf in the correction (the update was not applied), bit 32 = eps(u) <= 0 on the Stern boundary,
// bit 64 = a surface reaction rate that is not finite (kinetics on the Stern boundary), bit 128 = the galvanostat's constraint has no
// step (total current <= 0, a term that is not finite, or a zero denominator).  Bits 256 / 512 belong to the per-frequency status of
// gmpnp_frequency_response (gmpnp_response_t.status), not to the handle's word: a pivot of the complex block elimination that is (all
// but) zero, a value of the response that is not finite
inline std::string status_message(int flags) {
  std::string m;
  if (flags & 1) m += "1 - sum_j a_j u_j <= 0 at a quadrature point; ";
  if (flags & 2) m += "singular diagonal node block; ";
  if (flags & 4) m += "singular coarse operator; ";
  if (flags & 8) m += "in-launch hand-over timed out; ";
  if (flags & 16) m += "NaN / Inf in the Newton correction (step limiter); ";
  if (flags & 32) m += "eps(u) <= 0 on the Stern boundary (BDM model); ";
  if (flags & 64) m += "surface kinetics: a reaction rate on the Stern boundary is not finite; ";
  if (flags & 128) m += "galvanostat: the total current is <= 0, a term of the constraint is not finite or d - c.z == 0; ";
  if (flags & 256) m += "frequency response: a pivot of the complex block elimination is (all but) zero at this frequency; ";
  if (flags & 512) m += "frequency response: a value of the response at this frequency is not finite; ";
  return m;
}

// ---- Stern-layer boundary condition (include/gmpnp.h "Stern-layer boundary condition"; kernels: gmpnp_stern.h) ----------------------
// The Stern term of the potential row is g(eps) (p_M - p) / lam with eps = eps(u) at the outer Helmholtz plane:
//     linear (model 1)   g = eps                                   the layer has the OHP permittivity (stern.py: Stern_linear)
//     BDM    (model 2)   g = (eps - eps_s) / ln(eps / eps_s)       eps falls linearly to eps_s at the surface (stern.py: bdm_closed_form)
// BDM is evaluated as eps_s (r - 1) / log(r), r = eps / eps_s; for |r - 1| < 1e-4 the series 1 + d/2 - d^2/12 (d = r - 1) takes over
// (next term d^3/24 < 5e-14) and g' = 1/2 - d/6 + d^2/8.  eps <= 0 has no BDM layer: ok = 0, g = g' = 0, and the caller raises
// status bit 32.  One function for the host and the device; gmpnp_amd/stern.py's coupled_g is its Python statement, operation for
// operation (tests/test_stern_bc_reference.py compares the bits).
#if defined(__HIPCC__)
#define GMPNP_RULE_HD __host__ __device__
#else
#define GMPNP_RULE_HD
#endif
constexpr double kSternSeriesSwitch = 1.0e-4;
struct SternG { double g, dg; int ok; };   // g(eps), dg / d eps
GMPNP_RULE_HD inline SternG stern_g(int model, double eps, double eps_s) {
  if (model != 2) return SternG{eps, 1.0, 1};
  if (!(eps > 0.0)) return SternG{0.0, 0.0, 0};
  const double r = eps / eps_s, d = r - 1.0;
  if ((d < 0.0 ? -d : d) < kSternSeriesSwitch)
    return SternG{eps_s * (1.0 + d / 2.0 - d * d / 12.0), 0.5 - d / 6.0 + d * d / 8.0, 1};
  const double L = log(r);
  return SternG{eps_s * (d / L), 1.0 / L - d / (r * L * L), 1};
}
inline bool stern_options_valid(const gmpnp_stern_t& o) {
  if (o.model == 0) return true;
  return (o.model == 1 || o.model == 2) && o.p_electrode == o.p_electrode && !std::isinf(o.p_electrode) && o.lam > 0.0 && !std::isinf(o.lam) &&
         (o.model == 1 || (o.eps_surface > 0.0 && !std::isinf(o.eps_surface)));
}

// ---- surface kinetics (include/gmpnp.h "potential-dependent surface kinetics"; kernels: gmpnp_kinetics.h) --------------------------
// Reaction r on the Stern boundary runs at  rate = k (u_reactant or 1) E,  E = exp(-alpha (p_M - p - p_eq)),  with p and u at the
// boundary node.  d_u = d rate / d u_reactant = k E and d_p = d rate / d p = alpha rate are what the Jacobian takes.  The reactant
// is not clamped (a negative u gives a negative rate: the derivative stays exact).  ok = 0 where rate or k E is not finite (the
// exponent overflowed at a wild iterate): the caller raises status bit 64.  One function for the host and the device;
// gmpnp_amd/kinetics.py's surface_rate is its Python statement, operation for operation.
struct KinRate { double rate, d_u, d_p; int ok; };
GMPNP_RULE_HD inline KinRate surface_rate(double k, double alpha, double p_eq, double p_M, double p, int has_reactant, double u_reactant) {
  const double E = exp(-alpha * (p_M - p - p_eq));
  const double kE = k * E;
  const double rate = has_reactant ? kE * u_reactant : kE;
  const double d_p = alpha * rate;
  // finite: |x| <= DBL_MAX is false for Inf and NaN (x - x == 0 would not do: under FMA contraction the compiler may turn the
  // difference of a product and its rounded value into the rounding error)
  const double big = 1.7976931348623157e308;
  const int ok = ((rate < 0.0 ? -rate : rate) <= big) && ((kE < 0.0 ? -kE : kE) <= big) && ((d_p < 0.0 ? -d_p : d_p) <= big);
  return KinRate{rate, kE, d_p, ok};
}
inline bool kinetics_options_valid(const gmpnp_kinetics_t& o, int n_species) {
  auto fin = [](double v) { return v == v && !std::isinf(v); };
  if (o.n_reactions < 0 || o.n_reactions > GMPNP_MAX_SURFACE_REACTIONS) return false;
  if (!fin(o.p_electrode)) return false;
  for (int r = 0; r < o.n_reactions; ++r) {
    if (!fin(o.k[r]) || !fin(o.alpha[r]) || !fin(o.p_eq[r])) return false;
    if (o.reactant[r] < -1 || o.reactant[r] >= n_species) return false;
    for (int i = 0; i < GMPNP_MAX_SPECIES; ++i) if (!fin(o.nu[r][i])) return false;
  }
  return true;
}

// ---- galvanostatic mode (include/gmpnp.h "galvanostatic mode"; kernels: gmpnp_galvanostat.h) ---------------------------------------
// The extra equation of the bordered Newton solve is G = ln(I / I_target) with I = sum_r weight_r I_r the total kinetic current, and
// block elimination gives the potential's correction dp = (G - c.y) / (d - c.z) from y = J^-1 F, z = J^-1 b.  ok = 0 (status bit 128)
// where I <= 0, where I, G, c.y, c.z or dp is not finite, or where d - c.z == 0; G and dp are then whatever the arithmetic gave and
// the caller applies no update.  One function for the host and the device; gmpnp_amd/kinetics.py's galvanostat_step is its Python
// statement, operation for operation.
struct GalvStep { double G, dp; int ok; };
GMPNP_RULE_HD inline bool rule_finite(double v) { return (v < 0.0 ? -v : v) <= 1.7976931348623157e308; }   // false for Inf and NaN (see surface_rate)
GMPNP_RULE_HD inline GalvStep galvanostat_step(double I, double I_target, double cy, double cz, double d) {
  const double G = I > 0.0 ? log(I / I_target) : 0.0;
  const double den = d - cz;
  const double dp = den != 0.0 ? (G - cy) / den : 0.0;
  const int ok = (I > 0.0) && rule_finite(I) && rule_finite(G) && rule_finite(cy) && rule_finite(cz) && (den != 0.0) && rule_finite(den) && rule_finite(dp);
  return GalvStep{G, dp, ok};
}
// G alone (the convergence test at a new state): ok = 0 where I <= 0 or I or G is not finite
GMPNP_RULE_HD inline GalvStep galvanostat_constraint(double I, double I_target) {
  const double G = I > 0.0 ? log(I / I_target) : 0.0;
  const int ok = (I > 0.0) && rule_finite(I) && rule_finite(G);
  return GalvStep{G, 0.0, ok};
}
inline bool galvanostat_options_valid(const gmpnp_galvanostat_t& o) {
  if (!o.on) return true;
  auto fin = [](double v) { return v == v && !std::isinf(v); };
  if (!(o.target > 0.0) || !fin(o.target)) return false;
  bool any = false;
  for (int r = 0; r < GMPNP_MAX_SURFACE_REACTIONS; ++r) { if (!fin(o.weight[r])) return false; any = any || o.weight[r] != 0.0; }
  return any;
}

// ---- frequency response (include/gmpnp.h "small-signal frequency response"; kernels: gmpnp_response.h) ---------------------------------
// The response of the 1D handle per unit of p_M at time-term multiplier sigma solves (K + i sigma M) x = -b with K = J at inv_dt = 0,
// M the consistent P1 mass on the species rows that carry no Dirichlet value, b = dF/dp_M.  Its functionals at a Stern node (g, g' at
// the node's permittivity, p the node's potential, x_p and x_j the node's entries of x) and at a kinetic node of weight w:
//     C    += g / lam (1 - x_p) + g' (p_M - p) / lam  sum_j epsc_j x_j          (dD/dp_M + the Stern row of J applied to x, g' included)
//     dI_r += w (d_u x_reactant + d_p (x_p - 1))                                (d_p = alpha rate: dI_r/dp_M = -alpha_r I_r)
// The complex numbers are pairs (re, im); the operations below are written out so that the host, the device and the Python statement
// (gmpnp_amd/impedance.py) perform the same roundings.  The pivot search of the complex block elimination compares |re| + |im|.
// Every product and sum below is rounded on its own (no fused multiply-add: GMPNP_RULE_NO_CONTRACT), so the device's elimination and
// tests/response_reference.py's model of it perform the same operations on the same numbers.
#if defined(__clang__)
#define GMPNP_RULE_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define GMPNP_RULE_NO_CONTRACT
#endif
struct Cx { double re, im; };
GMPNP_RULE_HD inline Cx cx_mul(Cx a, Cx b) { GMPNP_RULE_NO_CONTRACT return Cx{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
GMPNP_RULE_HD inline Cx cx_sub(Cx a, Cx b) { return Cx{a.re - b.re, a.im - b.im}; }
GMPNP_RULE_HD inline Cx cx_add(Cx a, Cx b) { return Cx{a.re + b.re, a.im + b.im}; }
GMPNP_RULE_HD inline Cx cx_inv(Cx a) { GMPNP_RULE_NO_CONTRACT const double n = a.re * a.re + a.im * a.im; return Cx{a.re / n, -a.im / n}; }
GMPNP_RULE_HD inline double response_pivot_key(Cx a) { return (a.re < 0.0 ? -a.re : a.re) + (a.im < 0.0 ? -a.im : a.im); }
// the Stern node's share of C; s = sum_j epsc_j x_j
GMPNP_RULE_HD inline Cx response_capacitance_term(double g, double dg, double lam, double p_M, double p, Cx x_p, Cx s) {
  GMPNP_RULE_NO_CONTRACT
  const double a = g / lam, c = dg * (p_M - p) / lam;
  return Cx{a * (1.0 - x_p.re) + c * s.re, c * s.im - a * x_p.im};
}
// reaction r's share of dI_r at a kinetic node of weight w (x_u = 0 for a reaction without a reactant)
GMPNP_RULE_HD inline Cx response_current_term(double w, double d_u, double d_p, Cx x_u, Cx x_p) {
  GMPNP_RULE_NO_CONTRACT
  return Cx{w * (d_u * x_u.re + d_p * (x_p.re - 1.0)), w * (d_u * x_u.im + d_p * x_p.im)};
}
constexpr int kResponseMaxFrequencies = 4096;
constexpr int kResponseSingular = 256, kResponseNonFinite = 512;   // gmpnp_response_t.status
inline bool response_sigma_valid(double sigma) { return sigma >= 0.0 && !std::isinf(sigma); }
inline bool response_count_valid(int n) { return n >= 1 && n <= kResponseMaxFrequencies; }
// bytes of workspace one frequency takes on nv vertices: the eliminated blocks [nv][8 columns][8 lanes] complex and x [nv][8] complex
inline double response_bytes_per_frequency(int nv) { return (double)nv * (8.0 * 8.0 + 8.0) * 16.0; }
// frequencies per chunk under a memory cap: at least one, at most n, a whole number of 8-frequency waves where that fits
inline int response_chunk(int n, int nv, double cap_bytes) {
  const double per = response_bytes_per_frequency(nv);
  double k = std::floor(cap_bytes / per);
  if (!(k >= 1.0)) k = 1.0;
  int c = k >= (double)n ? n : (int)k;
  if (c < n && c >= 8) c -= c % 8;
  return c;
}

// ---- frequency response of the 3D pore (include/gmpnp.h "frequency response, 3D"; kernels: gmpnp_response_band.h) -------------------
// The same system on the block band of the 3D handle: (K + i sigma M) x = -b by a complex block-banded LU.  C and dI_r are the tangent's
// facet-wise functionals (tangent_current_term above all) applied to Re x and Im x separately; the explicit d/dp_M part (the slope of
// the Stern term, -d_p of a rate) goes to the real part alone.  One facet's share of (Stern row of J).x towards its node a from its
// node b: se_fn = sum_j epsc_j x_{b,j} / FN, m_ab the facet's P1 mass entry, w_a = int (p_M - p) phi_a ds:
GMPNP_RULE_HD inline double response_facet_term(double g, double dg, double lam, double w_a, double m_ab, double se_fn, double x_p) {
  GMPNP_RULE_NO_CONTRACT
  return dg * se_fn * w_a / lam - g * m_ab / lam * x_p;
}
// bytes of complex band one frequency takes: n (2 b + 1) blocks of nf x nf (re, im) pairs
inline double response_band_bytes_per_frequency(int n, int b, int nf) { return (double)n * (2.0 * b + 1.0) * nf * nf * 16.0; }
// frequencies per chunk under the band LU's memory cap: at least one, at most n (a band above the cap for ONE frequency is refused by
// the caller before this rule is asked)
inline int response_band_chunk(int n, int n_blocks, int b, int nf, double cap_bytes) {
  double k = std::floor(cap_bytes / response_band_bytes_per_frequency(n_blocks, b, nf));
  if (!(k >= 1.0)) k = 1.0;
  return k >= (double)n ? n : (int)k;
}
// Gauss-Jordan inverse of one complex NF x NF block with partial pivoting inside the block: the statement of what the device's 16-lane
// group does (group16_inverse_cx).  Column k's pivot is the row r >= k with the largest |re| + |im| (ties: the lower row), which changes
// places with row k.  pivot_row[k] = that row; returns true where a pivot column was all zero or not a number.  A and inv: row major.
template <int NF>
inline bool response_block_inverse(const Cx* A, Cx* inv, int* pivot_row) {
  Cx row[NF][2 * NF];
  for (int r = 0; r < NF; ++r)
    for (int j = 0; j < NF; ++j) { row[r][j] = A[r * NF + j]; row[r][NF + j] = Cx{j == r ? 1.0 : 0.0, 0.0}; }
  bool bad = false;
  for (int k = 0; k < NF; ++k) {
    int idx = k; double v = response_pivot_key(row[k][k]);
    for (int r = k + 1; r < NF; ++r) { const double o = response_pivot_key(row[r][k]); if (o > v) { v = o; idx = r; } }
    if (!(v > 0.0)) bad = true;   // (the block's status says so; what the inverse then holds is not used)
    pivot_row[k] = idx;
    const Cx ip = cx_inv(row[idx][k]);
    Cx piv[2 * NF], oldk[2 * NF];
    for (int j = 0; j < 2 * NF; ++j) { piv[j] = row[idx][j]; oldk[j] = row[k][j]; }
    for (int r = 0; r < NF; ++r) {
      const Cx* mine = (r == idx) ? oldk : row[r];
      const Cx f = cx_mul(mine[k], ip);
      Cx out[2 * NF];
      for (int j = k + 1; j < 2 * NF; ++j) out[j] = (r == k) ? cx_mul(piv[j], ip) : cx_sub(mine[j], cx_mul(f, piv[j]));
      for (int j = k + 1; j < 2 * NF; ++j) row[r][j] = out[j];
      row[r][k] = Cx{r == k ? 1.0 : 0.0, 0.0};
    }
  }
  for (int r = 0; r < NF; ++r)
    for (int j = 0; j < NF; ++j) inv[r * NF + j] = row[r][NF + j];
  return bad;
}

// ---- refinement of a block-banded LU solve (gmpnp_api.hip: band_refined_substitute; gmpnp_response_band.h: k_cband_judge) --------------
// The pivoting of the band LU is restricted to the node blocks, so every answer is checked with the true residual and refined.  `round`
// counts the refinements already made (0: the plain solve), rn is the residual of the present answer, best the one of the answer before
// (round > 0).  Another round is made while the residual is finite, above the tolerance and, after a refinement, at least halved
// (otherwise the attainable accuracy is reached); three rounds at the most.
GMPNP_RULE_HD inline bool band_refine_again(int round, bool finite, double rn, double best, double tol) {
  if (!finite || round >= 3 || !(rn > tol)) return false;
  return round == 0 || rn < 0.5 * best;
}

// ---- electrode tangent and polarisation curves (include/gmpnp.h "electrode tangent"; kernels: gmpnp_tangent.h) ----------------------
// The tangent z = du/dtheta of F(u; theta) = 0 solves J z = -dF/dtheta.  Parameter codes: 0 = p_M, 16 + r = ln k_r, 32 + r = alpha_r,
// 48 = ln lam; kinds 0 ... 3 in that order, -1 = unknown.  The explicit derivatives at a boundary node, per unit weight:
//     rate_r     p_M: -alpha_r rate_r (= -d_p)    ln k_s: delta_rs rate_r    alpha_s: -delta_rs rate_r (p_M - p - p_eq_r)    ln lam: 0
//     Stern term p_M: g M / lam (`slope`)         ln lam: -term              otherwise 0
// and the functionals take  dI_r += w (d_u z_reactant + d_p z_p + explicit),  dD += explicit + (Stern row of J).z.  Every product and sum
// is rounded on its own (GMPNP_RULE_NO_CONTRACT); gmpnp_amd/polarisation.py states the same operations in Python.
constexpr int kTangentMaxColumns = 10;
constexpr int kTangentNonFinite = 1;   // gmpnp_tangent_t.status
GMPNP_RULE_HD inline int tangent_param_kind(int param) {
  if (param == 0) return 0;
  if (param >= 16 && param < 16 + GMPNP_MAX_SURFACE_REACTIONS) return 1;
  if (param >= 32 && param < 32 + GMPNP_MAX_SURFACE_REACTIONS) return 2;
  if (param == 48) return 3;
  return -1;
}
GMPNP_RULE_HD inline int tangent_param_reaction(int param) { const int k = tangent_param_kind(param); return k == 1 ? param - 16 : k == 2 ? param - 32 : -1; }
// valid for a handle with n_reactions reactions (0: the kinetics are off)
GMPNP_RULE_HD inline bool tangent_param_valid(int param, int n_reactions) {
  const int k = tangent_param_kind(param);
  if (k < 0) return false;
  return (k == 0 || k == 3) ? true : tangent_param_reaction(param) < n_reactions;
}
inline bool tangent_count_valid(int n) { return n >= 1 && n <= kTangentMaxColumns; }
// d rate_r / d theta at fixed u; eta = p_M - p - p_eq_r
GMPNP_RULE_HD inline double tangent_rate_explicit(int param, int r, double rate, double d_p, double eta) {
  GMPNP_RULE_NO_CONTRACT
  const int k = tangent_param_kind(param);
  if (k == 0) return -d_p;
  if (k == 1) return tangent_param_reaction(param) == r ? rate : 0.0;
  if (k == 2) return tangent_param_reaction(param) == r ? -(rate * eta) : 0.0;
  return 0.0;
}
// d (Stern term) / d theta at fixed u; slope = d term / d p_M
GMPNP_RULE_HD inline double tangent_stern_explicit(int param, double slope, double term) {
  const int k = tangent_param_kind(param);
  return k == 0 ? slope : k == 3 ? -term : 0.0;
}
// reaction r's share of dI_r at a kinetic node of weight w (z_u = 0 for a reaction without a reactant)
GMPNP_RULE_HD inline double tangent_current_term(double w, double d_u, double d_p, double z_u, double z_p, double explicit_part) {
  GMPNP_RULE_NO_CONTRACT
  return w * ((d_u * z_u + d_p * z_p) + explicit_part);
}
// gmpnp_parameter_advance: how the options move along a step dtheta in the parameters of `param` (the state takes alpha of the step,
// the parameters the whole of it).  p_M: p_electrode += dtheta in both options; ln k_r: k_r *= exp(dtheta); alpha_r += dtheta; ln lam:
// lam *= exp(dtheta).  The moved options are validated by the setters' own rules BEFORE anything is changed: `stern` and `kinetics` are
// the caller's copies, and false leaves the handle as it was.  n_reactions = 0: the kinetics are off (a kinetic parameter is then
// refused by parameter_advance_refusal).  gmpnp_amd/fit.py's moved_options is its Python statement.
inline bool parameter_move(gmpnp_stern_t& stern, gmpnp_kinetics_t& kinetics, int n_species, int n, const int32_t* param, const double* dtheta) {
  for (int k = 0; k < n; ++k) {
    const int kind = tangent_param_kind(param[k]), r = tangent_param_reaction(param[k]);
    if (kind == 0) stern.p_electrode += dtheta[k];
    else if (kind == 1) kinetics.k[r] *= std::exp(dtheta[k]);
    else if (kind == 2) kinetics.alpha[r] += dtheta[k];
    else if (kind == 3) stern.lam *= std::exp(dtheta[k]);
    else return false;
  }
  if (kinetics.n_reactions != 0) kinetics.p_electrode = stern.p_electrode;
  return stern_options_valid(stern) && (kinetics.n_reactions == 0 || kinetics_options_valid(kinetics, n_species));
}
// the arguments of gmpnp_parameter_advance against the parameters of the last tangent call (last[n_last], status 0 = computed):
// nullptr = fine, otherwise what is wrong
inline const char* parameter_advance_refusal(int n, const int32_t* param, const double* dtheta, double tau, int n_last, const int32_t* last,
                                             const int32_t* last_status) {
  if (!tangent_count_valid(n)) return "n must lie in 1 ... 10";
  for (int k = 0; k < n; ++k) {
    for (int q = 0; q < k; ++q)
      if (param[q] == param[k]) return "a parameter is repeated";
    int at = -1;
    for (int q = 0; q < n_last; ++q) at = (last[q] == param[k]) ? q : at;
    if (at < 0) return "a parameter is not among those of the last gmpnp_electrode_tangent call";
    if (last_status[at] != 0) return "a requested column of the last gmpnp_electrode_tangent call is not finite";
    if (!rule_finite(dtheta[k])) return "every dtheta must be finite";
  }
  if (!(tau == 0.0 || (tau > 0.0 && tau < 1.0))) return "tau must be 0 (no damping) or lie in (0, 1)";
  return nullptr;
}
// The continuation rule of a polarisation curve.  Targets are the grid v_start + k v_step up to v_end, which is landed on exactly; an
// attempt goes from the last converged point `at` towards the next target with step `dp`; a failed attempt halves the step, a success
// tries the whole remainder to the target again; a step below |v_step| / 1024 ends the curve (stop = 1, "dp_min").
struct Continuation {
  double v_start, v_end, v_step;
  double at;        // the last converged potential
  int k;            // grid points reached so far (the start is point 0)
  double dp;        // the step of the next attempt
  int stop;         // 0 running, 1 dp_min, 2 the end was reached
};
inline bool continuation_valid(double v_start, double v_end, double v_step) {
  return rule_finite(v_start) && rule_finite(v_end) && rule_finite(v_step) && v_step != 0.0 && (v_end - v_start) * v_step >= 0.0;
}
inline double continuation_target(const Continuation& c) {
  const double t = c.v_start + (c.k + 1) * c.v_step;
  return (c.v_step > 0.0 ? t >= c.v_end : t <= c.v_end) ? c.v_end : t;
}
inline Continuation continuation_begin(double v_start, double v_end, double v_step) {
  Continuation c{v_start, v_end, v_step, v_start, 0, 0.0, 0};
  if (v_start == v_end) c.stop = 2;
  else c.dp = continuation_target(c) - c.at;
  return c;
}
// the potential of the next attempt: the target itself where the attempt lands on it
inline double continuation_attempt(const Continuation& c) {
  const double next = c.at + c.dp, t = continuation_target(c);
  return (c.v_step > 0.0 ? next >= t : next <= t) ? t : next;
}
// after an attempt of step c.dp: returns 1 where a grid point was reached (c.k counts it), else 0
inline int continuation_advance(Continuation& c, bool success) {
  const double target = continuation_target(c);
  const double dp_min = (c.v_step < 0.0 ? -c.v_step : c.v_step) / 1024.0;
  if (!success) {
    c.dp = c.dp / 2.0;
    if ((c.dp < 0.0 ? -c.dp : c.dp) < dp_min) c.stop = 1;
    return 0;
  }
  const double next = c.at + c.dp;
  const bool landed = c.v_step > 0.0 ? next >= target : next <= target;
  if (landed) {
    c.at = target; c.k += 1;
    if (target == c.v_end) { c.stop = 2; c.dp = 0.0; }
    else c.dp = continuation_target(c) - c.at;
    return 1;
  }
  c.at = next;
  c.dp = target - c.at;
  return 0;
}

// ---- potential programmes (include/gmpnp.h "potential programmes"; kernels: gmpnp_trace.h; gmpnp_amd/programme.py states the same in
// Python, operation for operation) ------------------------------------------------------------------------------------------------------
// A programme is a list of segments (t0, t1, p0, p1), t1 > t0, contiguous in time, p linear inside a segment.  A breakpoint where
// p1 of a segment equals p0 of the next is a corner, otherwise a jump.  Times are the driver's scaled time, potentials thermal voltages.
struct ProgrammeSegment { double t0, t1, p0, p1; };
using Programme = std::vector<ProgrammeSegment>;
inline bool programme_valid(const Programme& s) {
  if (s.empty()) return false;
  for (size_t k = 0; k < s.size(); ++k) {
    if (!(rule_finite(s[k].t0) && rule_finite(s[k].t1) && rule_finite(s[k].p0) && rule_finite(s[k].p1))) return false;
    if (!(s[k].t1 > s[k].t0)) return false;
    if (k > 0 && s[k].t0 != s[k - 1].t1) return false;
  }
  return true;
}
// the breakpoint behind segment k is a jump (the end of the programme is neither)
inline bool programme_jump(const Programme& s, int k) { return k + 1 < (int)s.size() && s[k].p1 != s[k + 1].p0; }
// The potential of an implicit step that ENDS at t_end inside the segment: p1 itself at t_end == t1 (landed values are exact, as
// Continuation lands on its targets), else the interpolated sum.  A step never straddles a breakpoint.
inline double programme_value(const ProgrammeSegment& s, double t_end) {
  GMPNP_RULE_NO_CONTRACT
  if (t_end >= s.t1) return s.p1;
  return s.p0 + (s.p1 - s.p0) * ((t_end - s.t0) / (s.t1 - s.t0));
}
// pulse: `cycles` times the holds levels[k] for durations[k], from t = 0.  rise_time > 0 replaces each jump by a ramp of that length
// taken from the following hold (which must be longer).  Empty where the arguments are not valid.
inline Programme programme_pulse(const std::vector<double>& levels, const std::vector<double>& durations, int cycles, double rise_time) {
  Programme out;
  const size_t n = levels.size();
  if (n == 0 || durations.size() != n || cycles < 1 || !(rise_time >= 0.0) || !rule_finite(rise_time)) return out;
  for (size_t k = 0; k < n; ++k)
    if (!rule_finite(levels[k]) || !rule_finite(durations[k]) || !(durations[k] > rise_time)) return Programme();
  double t = 0.0, last = levels[0];
  for (int c = 0; c < cycles; ++c)
    for (size_t k = 0; k < n; ++k) {
      const double end = t + durations[k];
      double t_hold = t;
      if (rise_time > 0.0 && levels[k] != last) { t_hold = t + rise_time; out.push_back({t, t_hold, last, levels[k]}); }
      out.push_back({t_hold, end, levels[k], levels[k]});
      t = end; last = levels[k];
    }
  return out;
}
// triangle: `cycles` times v_start -> v_vertex -> v_start at scan_rate > 0 (potential per time), from t = 0; every breakpoint a corner
inline Programme programme_triangle(double v_start, double v_vertex, double scan_rate, int cycles) {
  Programme out;
  if (!rule_finite(v_start) || !rule_finite(v_vertex) || !rule_finite(scan_rate) || !(scan_rate > 0.0) || cycles < 1 || v_start == v_vertex)
    return out;
  const double span = v_vertex - v_start, leg = (span < 0.0 ? -span : span) / scan_rate;
  if (!(leg > 0.0) || !rule_finite(leg)) return out;
  double t = 0.0;
  for (int c = 0; c < cycles; ++c) {
    const double mid = t + leg, end = mid + leg;
    out.push_back({t, mid, v_start, v_vertex});
    out.push_back({mid, end, v_vertex, v_start});
    t = end;
  }
  return out;
}
// table: straight lines through (times[k], potentials[k]); a time given twice in a row is a jump there (never three times)
inline Programme programme_table(const std::vector<double>& times, const std::vector<double>& potentials) {
  Programme out;
  const size_t n = times.size();
  if (n < 2 || potentials.size() != n) return out;
  for (size_t k = 0; k < n; ++k) if (!rule_finite(times[k]) || !rule_finite(potentials[k])) return out;
  for (size_t k = 0; k + 1 < n; ++k) {
    if (times[k + 1] == times[k]) {
      if (k == 0 || k + 2 >= n || times[k + 2] == times[k]) return Programme();
      continue;
    }
    if (!(times[k + 1] > times[k])) return Programme();
    out.push_back({times[k], times[k + 1], potentials[k], potentials[k + 1]});
  }
  return out;
}
// The walk.  Every attempt is judged by next_time_step with a copy of the policy whose t_end is programme_break: the smaller of the
// segment's end and the run's end.  programme_after moves the walk on from that decision: a stop_end at a breakpoint that is not the
// end moves to the next segment and does not stop; behind a jump the next attempt is a first step (h = dt_restart, h_prev = 0: the
// estimator reports no history, so the step is not judged against an extrapolation across the jump); behind a corner nothing is reset.
// A failed or rejected attempt stays in its segment with the controller's smaller step.  programme_clip is next_time_step's landing
// applied to a step that starts a segment: cut, or stretched by at most 1 %, to end on the breakpoint.
struct ProgrammeWalk {
  int seg = 0;
  double t = 0.0, h = 0.0, h_prev = 0.0;
  int steady_run = 0;
  int stop = 0;        // 0 running, 1 the end was reached, 2 h_min
};
inline double programme_break(const Programme& s, int seg, double run_end) { return s[seg].t1 < run_end ? s[seg].t1 : run_end; }
inline double programme_clip(double h, double t, double t_break) {
  const double left = t_break - t;
  return left <= 1.01 * h ? left : h;
}
// where the attempt (t, h) ends: the breakpoint itself where next_time_step will say the step landed on it.  The attempt's potential is
// programme_value there, so a landed step is solved at the segment's p1 exactly.
inline double programme_step_end(double t, double h, double t_break) {
  const double next = t + h, left = t_break - next;
  return left > 1e-12 * std::fabs(t_break) ? next : t_break;
}
inline ProgrammeWalk programme_begin(const Programme& s, double dt_init, double run_end) {
  ProgrammeWalk w;
  w.t = s[0].t0;
  w.h = programme_clip(dt_init, w.t, programme_break(s, 0, run_end));
  return w;
}
// (programme_after, which reads the decision of next_time_step, stands behind it below)
// fixed mode (steps_per_segment = n, no estimator): every step of a segment is (t1 - t0) / n long and the last one lands on t1
inline double programme_fixed_step(const ProgrammeSegment& s, int n) { return (s.t1 - s.t0) / n; }

// The combine step of one electrode record (gmpnp_electrode_trace_append): the host, the device and the Python statement perform the
// same operations, every product, quotient and sum rounded on its own.  The state keeps D_prev and the accumulated charges.
struct ElectrodeAccum { double D_prev, Q[GMPNP_MAX_SURFACE_REACTIONS], Q_D; };
GMPNP_RULE_HD inline double electrode_record_combine(ElectrodeAccum& a, double h, double D, const double (&I)[GMPNP_MAX_SURFACE_REACTIONS]) {
  GMPNP_RULE_NO_CONTRACT
  const double dD_dt = (D - a.D_prev) / h;
  a.Q[0] = a.Q[0] + h * I[0]; a.Q[1] = a.Q[1] + h * I[1]; a.Q[2] = a.Q[2] + h * I[2]; a.Q[3] = a.Q[3] + h * I[3];
  a.Q_D = a.Q_D + h * dD_dt;
  a.D_prev = D;
  return dD_dt;
}

// ---- record streams (RecordStream in gmpnp_api.hip: the electrode trace, the wall profile, the transient sensitivities) ------------------
// A buffer of `capacity` rows, one per accepted step, written without host synchronisation and read in chunks.  One more row stands
// behind the buffer for the timing hooks of gmpnp_time_kernel, which so never write a row that can be read.
inline size_t record_rows(int capacity) { return (size_t)capacity + 1; }
// rows first ... first + n - 1 have been written (the sum in 64 bits: first + n cannot wrap)
inline bool record_range_valid(int32_t first, int32_t n, int count) { return first >= 0 && n >= 1 && (int64_t)first + n <= count; }
inline bool record_can_append(int count, int capacity) { return count < capacity; }
// the step of length h that ends at t
inline bool record_step_valid(double t, double h) { return rule_finite(t) && rule_finite(h) && h > 0.0; }

// ---- wall profile (include/gmpnp.h "wall profile"; kernel: gmpnp_wall_profile.h; gmpnp_amd/programme.py states the same in Python) ------
// The wall of the 3D pore in n axial bins with the edges edges[0] < ... < edges[n] (z: the mesh's third coordinate, units of L).
// wall_bin uses comparisons only, so the two statements agree bit for bit by construction: the bin of z is the largest b with
// edges[b] <= z, z == edges[n] goes to bin n - 1, and z outside [edges[0], edges[n]] (or NaN) is bin -1 and belongs to no bin.
constexpr int kWallProfileMaxBins = 256;
inline int wall_bin(double z, const double* edges, int n) {
  if (!(z >= edges[0]) || !(z <= edges[n])) return -1;
  int b = 0;
  for (int k = 1; k < n; ++k) if (edges[k] <= z) b = k;
  return b;
}
inline bool wall_bins_valid(const double* edges, int n) {
  if (n < 1 || n > kWallProfileMaxBins || !edges) return false;
  for (int k = 0; k <= n; ++k) if (!rule_finite(edges[k])) return false;
  for (int k = 0; k < n; ++k) if (!(edges[k] < edges[k + 1])) return false;
  return true;
}
// n equal bins over [z_lo, z_hi]: every operation rounded on its own; the last edge is z_hi itself
inline std::vector<double> uniform_edges(double z_lo, double z_hi, int n) {
  GMPNP_RULE_NO_CONTRACT
  std::vector<double> e((size_t)(n > 0 ? n : 0) + 1, z_hi);
  for (int k = 0; k < n; ++k) e[k] = z_lo + (z_hi - z_lo) * ((double)k / (double)n);
  return e;
}
// the charge statement of electrode_record_combine for one bin: Q_b[r] += h I_b[r], product and sum rounded on their own
GMPNP_RULE_HD inline void wall_profile_charge(double (&Q)[GMPNP_MAX_SURFACE_REACTIONS], double h, const double (&I)[GMPNP_MAX_SURFACE_REACTIONS]) {
  GMPNP_RULE_NO_CONTRACT
  Q[0] = Q[0] + h * I[0]; Q[1] = Q[1] + h * I[1]; Q[2] = Q[2] + h * I[2]; Q[3] = Q[3] + h * I[3];
}

// [3P] dolfin::NewtonSolver, criterion "residual": r / r0 < rtol || r < atol, tested BEFORE the first iteration and after every
// update.  A driver hands every residual norm (with the device status word of its evaluation) to first() / next() and does what
// the verdict says; on `failed` and `limit` the error is (code, message).  Owns r0, steric_excursion, residuals[], n_residuals
// and converged of the statistics; reads st.iterations (the driver counts) against maximum_iterations.
struct NewtonJudge {
  enum Verdict { go_on, converged, limit, failed };
  const gmpnp_newton_options_t& o;
  gmpnp_newton_stats_t& st;
  const bool strict_steric;
  double r0 = 0.0;
  int code = GMPNP_OK;
  std::string message;

  NewtonJudge(const gmpnp_newton_options_t& o_, gmpnp_newton_stats_t& st_, bool strict) : o(o_), st(st_), strict_steric(strict) {}

  // residual at the state the solve starts from (the status bits of a linear solve mean nothing yet)
  Verdict first(double r, int flags) {
    if (steric(flags)) return fail(GMPNP_ERR_NUMERIC, status_message(flags));
    if (flags & (32 | 64 | 128)) return fail(GMPNP_ERR_NUMERIC, status_message(flags));
    r0 = r;
    st.residuals[0] = r; st.n_residuals = 1;
    if (!(r == r)) return fail(GMPNP_ERR_NUMERIC, "residual is NaN before the first Newton iteration");
    return test(r);
  }
  // residual after an update (st.iterations already counts it)
  Verdict next(double r, int flags) {
    if (steric(flags)) return fail(GMPNP_ERR_NUMERIC, status_message(flags));
    if (flags & (16 | 32 | 64 | 128)) return fail(GMPNP_ERR_NUMERIC, status_message(flags));
    if (flags & 14) return fail(GMPNP_ERR_LINEAR, status_message(flags));
    if (st.n_residuals < GMPNP_MAX_NEWTON_HISTORY) st.residuals[st.n_residuals++] = r;
    // NaN / Inf stay fatal (DOLFIN would iterate to its limit on a NaN residual and raise there)
    if (!(r == r) || std::isinf(r))
      return fail(GMPNP_ERR_NUMERIC, (flags & 1) ? "residual became NaN / Inf after an iterate left the admissible set (1 - sum_j a_j u_j <= 0)"
                                                 : "residual became NaN");
    return test(r);
  }

 private:
  Verdict fail(int c, const std::string& m) { code = c; message = m; return failed; }
  bool steric(int flags) {   // bit 1 is information; fatal only with strict_steric
    if (flags & 1) st.steric_excursion = 1;
    return (flags & 1) && strict_steric;
  }
  Verdict test(double res) {
    const double rel = res / r0;  // 0/0 = NaN compares false, as in DOLFIN
    if (res == res && (rel < o.relative_tolerance || res < o.absolute_tolerance)) { st.converged = 1; return converged; }
    if (st.iterations < o.maximum_iterations) return go_on;
    st.converged = 0; code = GMPNP_ERR_NOT_CONVERGED; message = "Newton solver did not converge because maximum number of iterations reached";
    return limit;
  }
};

// Fraction-to-boundary step limiter (gmpnp_newton_options_t.step_fraction = tau; kernels: gmpnp_step_limit.h).  For the correction
// dx of J dx = b at the state u, over the vertices I:
//     S_I = sum_j a_j u_{I,j}    dS_I = sum_j a_j dx_{I,j}    lambda = min_{dS_I < 0, S_I < 1} (1 - S_I) / (-dS_I)   (+inf: none)
//     alpha = tau lambda if lambda < 1, else 1                 u <- u - omega alpha dx      (omega alpha, not min(omega, tau lambda))
// The device forms lambda and alpha; the host checks the option and keeps the statistics.  A limited solve starts every linear
// solve from zero (predicted_start below assumes a constant step length: its callers pass warm_start = 0).
inline bool step_fraction_valid(double tau) { return tau == 0.0 || (tau > 0.0 && tau < 1.0); }
inline double step_factor(double lambda, double tau) { return lambda < 1.0 ? tau * lambda : 1.0; }
// alpha of Newton iteration `it` (0-based) into the statistics (min_step starts at 1.0)
inline void record_step(gmpnp_newton_stats_t& st, int it, double alpha) {
  if (it >= 0 && it < GMPNP_MAX_NEWTON_HISTORY) st.step_factor[it] = alpha;
  if (alpha < 1.0) { st.limited_steps++; st.min_step = std::min(st.min_step, alpha); }
}
inline gmpnp_newton_stats_t fresh_newton_stats() { gmpnp_newton_stats_t st{}; st.min_step = 1.0; return st; }

// ---- adaptive time stepping (include/gmpnp.h "adaptive time stepping"; kernels: gmpnp_time_step.h) ---------------------------------
// gmpnp_set_time_step's argument: finite and >= 0 (0 = the steady form, no time term)
inline bool time_step_valid(double inv_dt) { return inv_dt >= 0.0 && !std::isinf(inv_dt); }

// The accept / reject rule of one attempted step h at time t.  The exponent of the step factor is 1/2 because backward Euler's
// LOCAL error is O(h^2): err(h') = err(h) (h'/h)^2 = 1 at h' = h err^(-1/2), times the safety factor.
// At order 2 (variable-step BDF2, "second order" below) the local error is O(h^3): the factor is safety err^(-1/3), and an accepted
// step grows by min(max_factor, 2) at most, because variable-step BDF2 is zero-stable only for h / h_prev < 1 + sqrt(2).  Everything
// else is the same rule; order 1 (the default) performs the operations it always performed.
struct TimeStepPolicy {
  double safety = 0.9, min_factor = 0.2, max_factor = 4.0, fail_factor = 0.25;
  double h_min = 0.0, h_max = INFINITY, t_end = INFINITY;
  double steady_tol = 0.0;   // 0 = no steady stop
  int steady_steps = 2;      // consecutive accepted steps with rate < steady_tol
};
struct TimeStepDecision {
  enum Reason { accepted = 0, error_too_large = 1, newton_failed = 2, nonfinite = 3 };
  bool accept = false;
  int reason = accepted;
  double t_next = 0.0;       // t + h when accepted (t_end exactly when the step landed on it), else t
  double h_next = 0.0;       // the step to try next
  bool stop_end = false;     // accepted and t_next == t_end
  bool stop_steady = false;  // accepted and the steady counter reached steady_steps
  bool give_up = false;      // h_next < h_min (and not the last step, cut to land on t_end): the run ends
  int steady_run = 0;        // the counter after this attempt (the caller passes it back in)
};
// err / has_history / rate: gmpnp_time_error_t; newton_failed: the solve of the step did not converge or its state is not finite
// (a NaN err counts as such); steady_run: the counter the previous decision returned (0 at the start).
inline TimeStepDecision next_time_step(const TimeStepPolicy& p, double t, double h, double err, bool has_history, bool newton_failed,
                                       double rate, int steady_run, int order = 1) {
  TimeStepDecision d;
  const bool nan_err = !(err == err);
  auto clampd = [](double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); };
  auto factor = [&](double hi) {   // safety err^(-1/2) (order 2: err^(-1/3)) clamped; err = 0 gives the upper clamp
    if (!has_history) return 1.0;
    return err > 0.0 ? clampd(p.safety / (order == 2 ? std::cbrt(err) : std::sqrt(err)), p.min_factor, hi) : hi;
  };
  const double grow = order == 2 ? std::min(p.max_factor, 2.0) : p.max_factor;
  if (newton_failed || nan_err) {
    d.accept = false; d.reason = newton_failed ? TimeStepDecision::newton_failed : TimeStepDecision::nonfinite;
    d.t_next = t; d.h_next = p.fail_factor * h; d.steady_run = steady_run;
  } else if (has_history && err > 1.0) {
    d.accept = false; d.reason = TimeStepDecision::error_too_large;
    d.t_next = t; d.h_next = h * factor(1.0); d.steady_run = steady_run;
  } else {
    d.accept = true; d.reason = TimeStepDecision::accepted;
    d.t_next = t + h; d.h_next = h * factor(grow);
    d.steady_run = (p.steady_tol > 0.0 && rate < p.steady_tol) ? steady_run + 1 : 0;
    d.stop_steady = p.steady_tol > 0.0 && d.steady_run >= p.steady_steps;
  }
  if (d.h_next > p.h_max) d.h_next = p.h_max;
  // land on t_end exactly: shorten the step, or stretch it by at most 1 % instead of leaving a sliver behind it
  bool lands = false;   // the next step is the last one, cut (or stretched) to end on t_end: h_min does not judge it
  if (std::isfinite(p.t_end)) {
    const double left = p.t_end - d.t_next;
    if (d.accept && !(left > 1e-12 * std::fabs(p.t_end))) { d.t_next = p.t_end; d.stop_end = true; }
    else if (left <= 1.01 * d.h_next) { lands = d.h_next >= p.h_min; d.h_next = left; }
  }
  if (!d.stop_end && !d.stop_steady && !lands && d.h_next < p.h_min) d.give_up = true;
  return d;
}
// The walk of a potential programme after the decision of an attempt (its policy's t_end was programme_break; h_done: the step just
// judged).  Returns 1 where the accepted step landed on a breakpoint or on the end.
inline int programme_after(const Programme& s, ProgrammeWalk& w, const TimeStepDecision& d, double h_done, double dt_restart, double run_end) {
  w.steady_run = d.steady_run;
  w.t = d.t_next; w.h = d.h_next;
  if (!d.accept || !d.stop_end) {
    if (d.accept) w.h_prev = h_done;
    if (d.give_up) w.stop = 2;
    return 0;
  }
  w.h_prev = h_done;
  if (w.seg + 1 >= (int)s.size() || !(s[w.seg].t1 < run_end)) { w.stop = 1; return 1; }
  const bool jump = programme_jump(s, w.seg);
  w.seg += 1;
  if (jump) { w.h = dt_restart; w.h_prev = 0.0; }
  w.h = programme_clip(w.h, w.t, programme_break(s, w.seg, run_end));
  return 1;
}

// ---- second order: variable-step BDF2 (include/gmpnp.h "second-order adaptive time stepping"; kernels: gmpnp_time_order.h) ----------
// With omega = h / h_prev the time term of a BDF2 step is (alpha0 / h) M (u - u*): the element pass reads it as inv_dt M (u - un) with
// inv_dt = alpha0 inv_dt_of_h(h) and un = u* = a u_n - b u_nm1.
inline bool time_ratio_valid(double omega) { return omega > 0.0 && !std::isinf(omega); }
inline double bdf2_alpha0(double omega) { return (1.0 + 2.0 * omega) / (1.0 + omega); }
inline std::pair<double, double> bdf2_history_weights(double omega) {   // (a, b)
  const double q = 1.0 + 2.0 * omega;
  return {(1.0 + omega) * (1.0 + omega) / q, omega * omega / q};
}
// The estimator's predictor p = wn u_n + wm1 u_nm1 + wm2 u_nm2: the quadratic through (t - h1 - h2, u_nm2), (t - h1, u_nm1), (t, u_n)
// at t + h (Lagrange weights; h1 = the accepted step before h, h2 = the one before that).
struct TimePredictor { double wn, wm1, wm2; };
inline TimePredictor bdf2_predictor_weights(double h, double h1, double h2) {
  TimePredictor w;
  w.wn = (h + h1 + h2) * (h + h1) / ((h1 + h2) * h1);
  w.wm1 = -((h + h1 + h2) * h) / (h1 * h2);
  w.wm2 = (h + h1) * h / (h2 * (h1 + h2));
  return w;
}
// d = (u - p) kappa is BDF2's local error: u_exact - p = u'''/6 h (h + h1)(h + h1 + h2), the step's own error is
// u'''/6 h^2 (h + h1)(1 + omega)/(1 + 2 omega) with the same sign, so with c = h / alpha0 the share of the second in the sum u - p
// is kappa = c / (h + h1 + h2 + c).
inline double bdf2_error_share(double h, double h1, double h2) {
  const double c = h / bdf2_alpha0(h / h1);
  return c / (h + h1 + h2 + c);
}

// Predicted start x0 = a dx_k + b dx_{k-1} of the linear solve of Newton iteration `iteration` (0-based), q = 1 - omega: with the
// damped update consecutive corrections satisfy dx_{k+1} = q dx_k + O(|dx_k|^2), so x0 = q dx_k, plus the second-order term
// observed one iteration earlier, q^2 (dx_k - q dx_{k-1}), from the second iteration on (warm_start 1: first order only).
inline std::pair<double, double> predicted_start(int warm_start, double q, int iteration) {
  if (!warm_start || q == 0.0 || iteration < 1) return {0.0, 0.0};
  if (warm_start > 1 && iteration > 1) return {q + q * q, -q * q * q};
  return {q, 0.0};
}

// The predicted start is taken when it removes at least half of the residual: ||b - J x0||^2 = bb - 2 wb + ww from the three dot
// products wb = (w, b), ww = (w, w), bb = (b, b), w = J x0.  *rnorm = ||b - J x0|| when accepted.
inline bool accept_predicted_start(double wb, double ww, double bb, double* rnorm) {
  const double rn2 = bb - 2.0 * wb + ww;
  if (!(rn2 == rn2 && rn2 >= 0.0 && rn2 < 0.25 * bb)) return false;
  *rnorm = std::sqrt(rn2);
  return true;
}

// Whether the convergence test that follows the update of an iteration is expected to END the solve.  newton() starts the gather
// of the next Jacobian beside that test; one started for a solve that ends there is thrown away and holds up whatever the caller
// launches next, so it is not started where the end can be seen coming.  Newton's residual contracts by a near-constant factor from
// one iteration to the next ((1 - omega) under damping), so the factor observed last is applied once more: r_next = r_now^2 / r_prev,
// judged by NewtonJudge's own test (rel < rtol or res < atol; r0 = the solve's first residual).  `iterations` counts the update
// just made: at the limit the verdict cannot be go_on whatever the residual.  No contraction seen, a NaN, no history: no
// prediction (false).  A wrong answer costs time, never a result: the gather then runs behind the verdict, or is dropped.
inline bool last_test_expected(double r_prev, double r_now, double r0, double rtol, double atol, int iterations, int maximum_iterations) {
  if (iterations >= maximum_iterations) return true;
  if (!(r_prev > 0.0) || !(r_now >= 0.0) || !(r_now < r_prev)) return false;
  const double r_next = r_now * (r_now / r_prev);
  return r_next / r0 < rtol || r_next < atol;
}

// ---- policies of the linear solves inside Newton: each owns its state; newton() / group_newton() ask and report, nothing else --------

// kx holds the predicted start of the next linear solve (left by the previous Newton update).  (The previous time step's total
// update is useless as a start of a step's FIRST solve: optimal multiple ~1e-5, measured in round 1.)
struct PredictedX0 {
  bool held = false;
  void left(bool by_update) { held = by_update; }
  bool ready(int newton_it, double scale) const { return held && newton_it > 0 && scale != 0.0; }
};

// Coarse inverse of a single handle: reused for up to `lag` Newton iterations, unless the state was just set from outside (first
// solve of a run: the Jacobian changes a lot between iterations) or the last reuse cost iterations.  Asynchronous scheme (default):
// every iteration starts the coarse chain of its matrix on the side stream and solves with the inverse of the previous one; an
// inverse of THIS matrix is only built in-stream when it has to be.
struct CoarseReuse {
  bool refresh_due = false;  // a solve with a reused coarse inverse took clearly longer than the last fresh one
  int fresh_iters = 0;       // iterations of the last solve right after a coarse rebuild
  bool fresh(bool async, int lag, int newton_it, bool state_jumped) const {
    const bool must = state_jumped || refresh_due;
    return async ? must : (lag <= 1 || (newton_it % lag) == 0 || must);
  }
  // feedback: a reused coarse inverse that doubles the iteration count of the last fresh solve is dropped
  void solved(bool was_fresh, int iters) {
    if (was_fresh) { fresh_iters = iters; refresh_due = false; }
    else if (iters > 2 * fresh_iters + 10) refresh_due = true;
  }
  void fell_back() { refresh_due = true; }
};

// Coarse operator of the partitioned two-level preconditioner: rebuilt (Galerkin product, one all-reduce, 72 x 72 inverse: 180 us
// in the stream) for the first Newton iteration of a solve and every third one after it; in between the solves run with the
// inverse they have — any coarse operator gives a valid right preconditioner (the single-GPU solver does the same with a
// side stream).  A solve that needs 25 % more iterations than the last one with a fresh inverse forces a rebuild
// (from the zero state the Jacobian of the second Newton iteration is far from the first one's: 160 instead of 73 iterations).
// Every figure here is identical on all ranks, so all ranks decide alike.  Schedule and threshold differ from CoarseReuse's on
// purpose: either one's rule in the other's place changes iteration counts.
struct GroupCoarseReuse {
  int age = 1 << 20, fresh_iters = 0; bool slow = false;
  // (a solve that starts from a state set from outside — the zero state of time step 0 — rebuilds every time: its Jacobians differ
  // too much, 203 instead of 56 iterations with the first iteration's inverse in the second)
  bool rebuild(int newton_it, bool state_jumped) const { return newton_it == 0 || age >= 2 || slow || state_jumped; }
  void solved(bool rebuilt, int iters) {
    if (rebuilt) { age = 0; fresh_iters = iters; slow = false; }
    else { age++; slow = iters > fresh_iters + fresh_iters / 4 + 5; }
  }
};

// The reference's linear solver is direct (MUMPS, 3D:792): a Krylov solve that does not converge is not an error there.  The
// block-banded LU takes over for that system, the rest of that Newton solve and the next few solves.
struct DirectFallback {
  int sticky = 0;    // Newton solves that still go straight to the band LU after a Krylov failure
  int backoff = 0;   // length of the last such stretch (doubles with every new failure, resets on a converged Krylov solve)
  bool use_direct() const { return sticky > 0; }
  void krylov_converged(int newton_it) { if (newton_it == 0) backoff /= 2; }  // BiCGStab works again
  // back off: 8, 16, ... 256 Newton solves before BiCGStab is tried again (a failed try costs ~0.25 s)
  void fell_back() { backoff = std::min(256, std::max(8, 2 * backoff)); sticky = backoff; }
  void newton_done(bool band_lu_asked) { if (sticky > 0 && !band_lu_asked) sticky--; }
};

// First launch burst of a single handle's BiCGStab solve.  With the pinned progress mirror the host keeps up one iteration at a
// time, so the first burst is insurance against a slow host rather than a way to save polls: half the expected count (measured on
// the bench, sixteenths of the hint: 0..8 -> 529-533 its/s, 12 -> 525, 14 -> 522, 16 -> 516; more surplus early-exit launches the
// longer it is).
struct BurstHint {
  int hint = 0;  // expected iterations of the next solve (the same Newton iteration of the previous time step), 0 = none
  int by_newton_it[32] = {0};
  int last[2] = {0, 0};   // iterations of the last first-pass solve, [use_coarse]
  void expect(int newton_it) { hint = newton_it < 32 ? by_newton_it[newton_it] : 0; }
  void record(int newton_it, int iters) { if (newton_it < 32) by_newton_it[newton_it] = iters; hint = 0; }
  // krylov_batch: gmpnp_options_t; B: iterations per polling burst; the result is a multiple of B
  int first(int use_coarse, int krylov_batch, int B, bool restart) const {
    const int expect = hint > 0 ? hint / 2 : last[use_coarse] / 2;
    int n = krylov_batch > 0 ? krylov_batch : std::max(B, expect);
    if (restart) n = B;  // a restart pass only has to remove the drift
    return ((n + B - 1) / B) * B;
  }
  void solve_done(int use_coarse, int iters, bool restart) { if (!restart) last[use_coarse] = iters; }
};

// ... and of a partitioned solve: every rank launches the SAME number of iterations (the schedule depends only on earlier
// solves' counts, identical on all ranks).
struct GroupBurstHint {
  int last = 0;   // BiCGStab iterations of the previous solve (identical on every rank)
  // ... and those of the previous Newton solve BY NEWTON ITERATION (the k-th linear solve of a time step takes within an iteration
  // or two of what the k-th of the step before took — 85 / 65 / 53 / 44 ... — while consecutive solves differ by tens): the first
  // burst of a solve is sized by it, so that most solves end inside their first burst (a burst boundary is a device-to-host copy
  // and a stream synchronisation: 30 us of idle GPU; an iteration launched behind the end of a solve costs 14 us)
  int by_newton_it[16] = {0};
  int predicted(int attempt, bool state_jumped, int newton_it) const {
    return (attempt == 0 && !state_jumped && newton_it < 16) ? by_newton_it[newton_it] : 0;
  }
  void record(int attempt, bool solved, int newton_it, int iters) { if (attempt == 0 && solved && newton_it < 16) by_newton_it[newton_it] = iters; }
  int first(int predicted, bool sized_by_previous) const { return predicted > 0 ? predicted + 1 : (sized_by_previous ? std::max(2, (7 * last) / 8) : 4); }
  void solve_done(int iters) { last = iters; }
};

// gmpnp_options_t resolved into what the solver reads (every option's 0 is its default)
struct Settings {
  int coarse_async = 1;       // opts.coarse_refresh = N: rebuild in the main stream every Nth iteration (the older scheme)
  int coarse_lag = 3;   // rebuild the coarse inverse alone every coarse_lag-th Newton iteration of a solve (measured best: 1 -> 3 costs 0.7 % more Krylov iterations and saves 155 us per skipped rebuild)
  int warm_async = 1;         // opts.warm_in_stream: test of the predicted start in the main stream, behind the set-up
  int warm_start = 2;  // start Newton iteration k+1's linear solve from (1 - omega) dx_k (+ second-order term); opts.warm_start
  int host_poll = 1;            // opts.progress_by_copy: poll with a device-to-host copy + event per burst instead
  int burst_iters = 1;  // iterations per polling burst (opts.burst_iterations); with copy + event polling: 1 -> 453, 2 -> 463,
                        // 4 -> 456, 8 -> 436 Newton its/s; with the pinned progress mirror a poll costs nothing on the
                        // device: 1 -> 496, 2 -> 492
  bool phase_timing = false;  // opts.phase_timing fills ms_assemble / ms_setup / ms_krylov of the Newton statistics
  int direct_fallback = 1;      // opts.no_direct_fallback: a failed Krylov solve is an error again
  int strict_steric = 0;        // opts.strict_steric: 1 - S <= 0 at a quadrature point is fatal (the reference has no such test)
  double lu_max_gb = 48.0;      // opts.band_lu_max_gb: largest band storage the fallback may allocate
};

// The options' range checks and their mapping; returns the error text, empty when *out is set.  (launch_form 2, vector_form and
// the residency of a launch need the device and the topology: gmpnp_create decides those.)
inline std::string resolve_options(const gmpnp_options_t& po, int dim, Settings* out) {
  if (po.krylov_batch < 0 || po.profile_every < 0) return "negative option";
  if (po.launch_form != 0 && po.launch_form != 2 && po.launch_form != 4) return "launch_form must be 0, 2 or 4";
  if (po.coarse_refresh < 0 || po.burst_iterations < 0 || po.warm_start < -1 || po.warm_start > 1 || !(po.band_lu_max_gb >= 0.0) ||
      po.vector_form < 0 || po.vector_form > 2)
    return "option out of range";
  if (po.element_stores < 0 || po.element_stores > 2 || (po.element_stores == 2 && dim != 3))
    return "element_stores: 0 (automatic), 1 (direct), 2 (staged, 3D meshes)";
  Settings s;
  s.coarse_async = (po.coarse_refresh == 0 && !po.shared_device) ? 1 : 0;
  s.coarse_lag = po.coarse_refresh > 0 ? po.coarse_refresh : 3;
  s.warm_async = (po.warm_in_stream || po.shared_device) ? 0 : 1;
  s.warm_start = po.warm_start == 0 ? 2 : (po.warm_start == 1 ? 1 : 0);
  s.host_poll = po.progress_by_copy ? 0 : 1;
  s.burst_iters = std::max(1, po.burst_iterations);
  s.phase_timing = po.phase_timing != 0;
  s.direct_fallback = po.no_direct_fallback ? 0 : 1;
  s.strict_steric = po.strict_steric ? 1 : 0;
  if (po.band_lu_max_gb > 0.0) s.lu_max_gb = po.band_lu_max_gb;
  *out = s;
  return std::string();
}

// Tables of the multilevel term between a fine and a coarse handle, in the INTERNAL orders of both (perm[internal] = file,
// iperm[file] = internal).  parents[2 v + {0, 1}]: the two coarse vertices (coarse file order) fine vertex v lies between, equal
// for the copy of a coarse vertex; partition handles say -1 where a parent is not local (ghost rows only).  The tables serve the
// OWNED rows [f0, f1) / [c0, c1) — all rows of an unpartitioned handle: par = the prolongation of an owned fine vertex, child =
// the restriction onto an owned coarse vertex (every local fine vertex naming it, ascending internal index: a fixed summation
// order, and on partitions the global slab order restricted), copy = the injection of an owned coarse vertex.
struct LevelTables { std::vector<int32_t> par, copy, child_ptr, child; };

inline std::string build_level_tables(const std::vector<int32_t>& fine_perm, const std::vector<int32_t>& coarse_iperm, int f0, int f1, int c0,
                                      int c1, const int32_t* parents, bool partitions, LevelTables* out) {
  const int nvf = (int)fine_perm.size(), nvc = (int)coarse_iperm.size(), lowest = partitions ? -1 : 0;
  std::vector<int32_t> par((size_t)2 * nvf, -1), copy(nvc, -1);
  std::vector<std::vector<int32_t>> kids(nvc);
  for (int I = 0; I < nvf; ++I) {
    const int v = fine_perm[I];
    const int a = parents[2 * v], b = parents[2 * v + 1];
    const bool owned = I >= f0 && I < f1;
    if (a < lowest || a >= nvc || b < lowest || b >= nvc) return "parent vertex out of range";
    if (owned && (a < 0 || b < 0)) return "multilevel term: both parents of an owned fine vertex must be local on the coarse level";
    const int Ia = a >= 0 ? coarse_iperm[a] : -1, Ib = b >= 0 ? coarse_iperm[b] : -1;
    if (owned) { par[2 * I] = Ia; par[2 * I + 1] = (a == b) ? -1 : Ib; }
    else { par[2 * I] = 0; par[2 * I + 1] = -1; }   // never read (ghost rows are masked); kept in range all the same
    if (a >= 0 && a == b) {
      if (copy[Ia] >= 0) return "two fine vertices claim to be the copy of one coarse vertex";
      copy[Ia] = I; kids[Ia].push_back(I << 1);
    } else {
      if (Ia >= 0) kids[Ia].push_back((I << 1) | 1);
      if (Ib >= 0) kids[Ib].push_back((I << 1) | 1);
    }
  }
  std::vector<int32_t> cptr(nvc + 1, 0), clist;
  for (int Ic = 0; Ic < nvc; ++Ic) {
    const bool owned = Ic >= c0 && Ic < c1;
    if (owned && (copy[Ic] < f0 || copy[Ic] >= f1))
      return partitions ? "multilevel term: an owned coarse vertex must have its copy among the owned fine vertices (the meshes are not nested, or the plans do not match)"
                        : "a coarse vertex has no copy on the fine level (the meshes are not nested)";
    if (!owned) copy[Ic] = -1;
    else clist.insert(clist.end(), kids[Ic].begin(), kids[Ic].end());
    cptr[Ic + 1] = (int32_t)clist.size();
  }
  out->par.swap(par); out->copy.swap(copy); out->child_ptr.swap(cptr); out->child.swap(clist);
  return std::string();
}

// ---- periodic steady state (include/gmpnp.h "periodic steady state"; kernels: gmpnp_cycle.h; gmpnp_amd/periodic.py states both rules
// in Python, operation for operation) ---------------------------------------------------------------------------------------------------
// anderson_weights: the mixing weights of a window of m + 1 pairs from its normal system A theta = b (A[i * lda + j] = <d_i, d_j>_W,
// b_i = <d_i, r_k>_W, i, j < m; column 0 is the oldest difference).  Cholesky A = L L^T of the columns lo ... m - 1, lo = 0 first; where
// a squared pivot is below 1e-12 x the largest diagonal entry of those columns or is not finite, a theta is not finite, or the weights
// do not sum to 1 within 1e-12 (what gmpnp_cycle_mix asks), the oldest column is dropped (lo + 1) and the elimination starts again;
// m - lo = 0 columns give gamma = (0, ..., 0, 1), the plain iteration.  With x_{k+1} = g_k - sum_j theta_j (g_{j+1} - g_j):
//     gamma_lo = theta_lo      gamma_i = theta_i - theta_{i-1} (lo < i < m)      gamma_m = 1 - theta_{m-1}      gamma_i = 0 (i < lo)
// Every product, quotient and sum is rounded on its own.  Returns the number of dropped columns; gamma has m + 1 entries.
constexpr int kCycleRuleDepth = GMPNP_CYCLE_MAX_DEPTH;
constexpr double kCyclePivotFloor = 1.0e-12, kCycleSumSlack = 1.0e-12;

inline bool cycle_gamma_valid(int n, const double* gamma) {
  GMPNP_RULE_NO_CONTRACT
  if (n < 1 || n > kCycleRuleDepth + 1 || !gamma) return false;
  double sum = 0.0;
  for (int j = 0; j < n; ++j) {
    if (!rule_finite(gamma[j])) return false;
    sum = sum + gamma[j];
  }
  const double off = sum - 1.0;
  return (off < 0.0 ? -off : off) <= kCycleSumSlack;
}

inline int anderson_weights(int m, const double* A, int lda, const double* b, double* gamma) {
  GMPNP_RULE_NO_CONTRACT
  if (m < 0) m = 0;
  if (m > kCycleRuleDepth) m = kCycleRuleDepth;
  for (int lo = 0; lo < m; ++lo) {
    const int n = m - lo;
    double L[kCycleRuleDepth][kCycleRuleDepth] = {}, y[kCycleRuleDepth] = {}, th[kCycleRuleDepth] = {};
    double top = 0.0;
    bool ok = true;
    for (int i = 0; i < n; ++i) {
      const double d = A[(lo + i) * lda + (lo + i)];
      if (!rule_finite(d)) ok = false;
      else if (d > top) top = d;
    }
    for (int j = 0; j < n && ok; ++j) {
      double piv = A[(lo + j) * lda + (lo + j)];
      for (int k = 0; k < j; ++k) piv = piv - L[j][k] * L[j][k];
      if (!rule_finite(piv) || !(piv >= kCyclePivotFloor * top) || !(piv > 0.0)) { ok = false; break; }
      L[j][j] = std::sqrt(piv);
      for (int i = j + 1; i < n; ++i) {
        double v = A[(lo + j) * lda + (lo + i)];   // the upper triangle
        for (int k = 0; k < j; ++k) v = v - L[i][k] * L[j][k];
        L[i][j] = v / L[j][j];
      }
    }
    if (!ok) continue;
    for (int i = 0; i < n; ++i) {
      double v = b[lo + i];
      for (int k = 0; k < i; ++k) v = v - L[i][k] * y[k];
      y[i] = v / L[i][i];
    }
    for (int i = n - 1; i >= 0; --i) {
      double v = y[i];
      for (int k = i + 1; k < n; ++k) v = v - L[k][i] * th[k];
      th[i] = v / L[i][i];
      if (!rule_finite(th[i])) ok = false;
    }
    if (!ok) continue;
    for (int i = 0; i < lo; ++i) gamma[i] = 0.0;
    gamma[lo] = th[0];
    for (int i = 1; i < n; ++i) gamma[lo + i] = th[i] - th[i - 1];
    gamma[m] = 1.0 - th[n - 1];
    if (cycle_gamma_valid(m + 1, gamma)) return lo;
  }
  for (int i = 0; i < m; ++i) gamma[i] = 0.0;
  gamma[m] = 1.0;
  return m;
}

// cycle_verdict: what the residual history err[0 .. n - 1] of n marched cycles means.  Converged at err <= tol_cycle; give_up once
// max_cycles cycles are marched; restart (empty the window and go on from g_k) where the residual grew by more than `growth` over the
// cycle before, is not finite, or the report / the mix met a non-finite value (`nonfinite`); growth is a safeguard, not a tuned constant.
enum CycleVerdict : int32_t { cycle_continue = 0, cycle_converged = 1, cycle_restart = 2, cycle_give_up = 3 };
struct CyclePolicy { double tol_cycle = 1.0; int max_cycles = 50; double growth = 10.0; };

inline CycleVerdict cycle_verdict(const double* err, int n, bool nonfinite, const CyclePolicy& p) {
  GMPNP_RULE_NO_CONTRACT
  if (n < 1) return cycle_continue;
  const double e = err[n - 1];
  const bool bad = nonfinite || !rule_finite(e);
  if (!bad && e <= p.tol_cycle) return cycle_converged;
  if (n >= p.max_cycles) return cycle_give_up;
  if (bad) return cycle_restart;
  if (n >= 2 && rule_finite(err[n - 2]) && e > p.growth * err[n - 2]) return cycle_restart;
  return cycle_continue;
}

// ---- value layout of the column-scaled matrix (vals_s; kernels: TileRows, scale_columns_body, coarse_rows_body) ----------------------
// One block position of a slice holds nf x 64 doubles: entry (j, lane) is column j of the block row that lane `lane` of the slice's
// wave owns.  vals keeps them [j][lane] (value_plain_offset).  vals_s keeps the columns in PAIRS: [j / 2][lane][j & 1] for the nf / 2
// pairs, then [lane] for the last column of an odd nf, so that a lane moves two neighbouring columns with one 16-byte request
// (nf = 9: four of 16 bytes and one of 8 instead of nine of 8).  A position is nf x 64 doubles either way; position stride, slice
// offsets and padding are those of vals, and both are even, so every pair is 16-byte aligned (asserted at create).  The writer
// (scale_columns_body) and every reader of vals_s take their offsets from here and nowhere else.
constexpr int kValueLanes = 64;
GMPNP_RULE_HD constexpr int value_plain_offset(int /*nf*/, int j, int lane) { return j * kValueLanes + lane; }
GMPNP_RULE_HD constexpr int value_pair_offset(int nf, int j, int lane) {
  return (j | 1) < nf ? (j >> 1) * 2 * kValueLanes + 2 * lane + (j & 1)   // member j & 1 of pair j / 2
                      : (nf - 1) * kValueLanes + lane;                    // the single last column of an odd nf
}

}  // namespace gmpnp
