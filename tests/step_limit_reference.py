"""The fraction-to-boundary step limiter of the Newton update (include/gmpnp.h, gmpnp_newton_options_t.step_fraction) restated in
NumPy, and a Newton loop over the oracle's assembly that applies it (imported like precond_reference.py; not a conftest).

    S_I = sum_j a_j u_{I,j}      dS_I = sum_j a_j dx_{I,j}          (j ascending, plain fp64 sums)
    lambda = min over the vertices with dS_I < 0 and S_I < 1 of (1 - S_I) / (-dS_I)       (+inf: none)
    alpha  = tau lambda if lambda < 1, else 1                       u <- u - omega alpha dx

Test infrastructure only.  ``tau = 0`` is the plain loop of ``gmpnp_oracle.newton_solve`` (same statements, same bits)."""
from dataclasses import dataclass, field

import numpy as np
import scipy.sparse.linalg as spla

import gmpnp_oracle as O


def steric_sum(a, x2d):
    """sum_j a_j x[:, j] over the species columns, j ascending, one rounded product and one rounded sum per term."""
    s = np.zeros(x2d.shape[0])
    for j in range(len(a)):
        s = s + a[j] * x2d[:, j]
    return s


def step_limit(a, u2d, dx2d, tau):
    """(alpha, lambda, limiting vertex or -1) of the rule for the (nv, nf) arrays u and dx; `a` = model.a[:n_species].
    Equal ratios: the first vertex in the order of the arrays.  ValueError on a NaN / Inf in dx."""
    if not np.all(np.isfinite(dx2d)):
        raise ValueError("NaN / Inf in the Newton correction")
    S, dS = steric_sum(a, u2d), steric_sum(a, dx2d)
    ratio = np.full(S.shape, np.inf)
    cand = (dS < 0.0) & (S < 1.0)
    ratio[cand] = (1.0 - S[cand]) / (-dS[cand])
    lam = float(ratio.min()) if ratio.size else np.inf
    node = int(np.argmin(ratio)) if lam < np.inf else -1
    alpha = tau * lam if lam < 1.0 else 1.0
    return alpha, lam, node


@dataclass
class LimitedStats:
    iterations: int = 0
    converged: bool = False
    residuals: list = field(default_factory=list)      # ||b||_2 before iteration 0 and after every update
    step_factor: list = field(default_factory=list)    # alpha of every iteration
    max_S: list = field(default_factory=list)          # max_I S_I after every update
    iterates: list = field(default_factory=list)       # u after every update (keep_iterates)
    same_as_plain: list = field(default_factory=list)  # beside_plain: the update equals the plain one, u - omega dx, bit for bit

    @property
    def limited_steps(self):
        return sum(1 for f in self.step_factor if f < 1.0)

    @property
    def min_step(self):
        return min([1.0] + [f for f in self.step_factor if f < 1.0])


def newton_loop(prob, u, un, tau=0.0, omega=1.0, maximum_iterations=50, relative_tolerance=1e-9, absolute_tolerance=1e-10,
                keep_iterates=False, beside_plain=False):
    """``gmpnp_oracle.newton_solve`` (residual criterion, tested before the first iteration and after every update, SuperLU for
    J dx = b) with the limited update; never raises on non-convergence.  Returns (u, LimitedStats).
    ``beside_plain``: every iteration also forms the plain update from the same u and dx and records whether the two are equal.
    Assembly and LU are deterministic, so by induction "equal at every iteration" is "the plain loop, run on its own, produces
    the same iterates" at half the cost (the 3D case spends its time in the sparse LU)."""
    u = np.array(u, dtype=np.float64, copy=True)
    nv, nf = prob.coords.shape[0], prob.nf
    a = np.asarray(prob.model.a, dtype=np.float64)[:nf - 1]
    st = LimitedStats()
    b, _ = O.assemble(prob, u, un, want_jacobian=False)
    r = float(np.linalg.norm(b))
    r0 = r
    st.residuals.append(r)

    def conv(res):
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.float64(res) / np.float64(r0)
        return bool(rel < relative_tolerance or res < absolute_tolerance)

    done = conv(r)
    while not done and st.iterations < maximum_iterations:
        b, A = O.assemble(prob, u, un, want_jacobian=True)
        dx = spla.splu(A.tocsc()).solve(b)
        if beside_plain:
            plain = u - omega * dx
        if tau:
            alpha = step_limit(a, u.reshape(nv, nf), dx.reshape(nv, nf), tau)[0]
            u -= (omega * alpha) * dx
        else:
            alpha = 1.0
            u -= omega * dx
        st.step_factor.append(alpha)
        st.iterations += 1
        st.max_S.append(float(steric_sum(a, u.reshape(nv, nf)).max()))
        if beside_plain:
            st.same_as_plain.append(bool(np.array_equal(u, plain)))
        if keep_iterates:
            st.iterates.append(u.copy())
        b, _ = O.assemble(prob, u, un, want_jacobian=False)
        r = float(np.linalg.norm(b))
        st.residuals.append(r)
        done = conv(r)
    st.converged = done
    return u, st


def first_step_state(prob):
    """(u, u_n) the 1D and 3D drivers start their first Newton solve from: u = 0, u_n = bulk (ones, potential 0)."""
    nv, nf = prob.coords.shape[0], prob.nf
    return np.zeros(prob.ndof), np.tile(np.r_[np.ones(nf - 1), 0.0], nv)
