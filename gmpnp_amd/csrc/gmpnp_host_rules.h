// Host-side decisions that have no device in them: what a Newton residual means (one verdict for newton(), group_newton()
// and the ensemble driver), the predicted start of a linear solve, and the tables of the geometric multilevel term.
// Includes gmpnp.h and the C++ standard library only, so it compiles (and is tested) with the host compiler alone.
#pragma once

#include <cmath>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "gmpnp.h"

namespace gmpnp {

// device status word: bit 1 = steric excursion (information, unless strict_steric), bits 2 / 4 / 8 = the linear solve failed
inline std::string status_message(int flags) {
  std::string m;
  if (flags & 1) m += "1 - sum_j a_j u_j <= 0 at a quadrature point; ";
  if (flags & 2) m += "singular diagonal node block; ";
  if (flags & 4) m += "singular coarse operator; ";
  if (flags & 8) m += "in-launch hand-over timed out; ";
  return m;
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
    r0 = r;
    st.residuals[0] = r; st.n_residuals = 1;
    if (!(r == r)) return fail(GMPNP_ERR_NUMERIC, "residual is NaN before the first Newton iteration");
    return test(r);
  }
  // residual after an update (st.iterations already counts it)
  Verdict next(double r, int flags) {
    if (steric(flags)) return fail(GMPNP_ERR_NUMERIC, status_message(flags));
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

}  // namespace gmpnp
