"""The accelerated cycle map restated in NumPy (include/gmpnp.h "periodic steady state"): the report of
``gmpnp_cycle_end`` (residual norm, maximum, normal system of the window), the mix of ``gmpnp_cycle_mix`` in its stated order, and the
``ops`` of ``gmpnp_amd.periodic.run_periodic`` over ``NumpyProgrammeSystem`` (imported like programme_reference.py; not a conftest).
Test infrastructure only."""
import math

import numpy as np

import programme_reference as PR
from gmpnp_amd import periodic as PD
from step_limit_reference import step_limit

MAX_DEPTH = PD.MAX_DEPTH


def cycle_weights(un, nf, rtol, atol):
    """w = atol_f + rtol |u_n| per dof, (ndof,); ``atol`` a scalar or (nf,)."""
    un = np.asarray(un, dtype=np.float64).reshape(-1, nf)
    atol = np.broadcast_to(np.asarray(atol, dtype=np.float64), (nf,))
    return (atol[None, :] + rtol * np.abs(un)).ravel()


def cycle_report(X, G, w, free):
    """The report of a window of pairs (``X[j]``, ``G[j]``), oldest first, (ndof,) each, with the weights ``w`` over the dofs where
    ``free`` (ndof,) is true: r_j = g_j - x_j, d_j = r_{j+1} - r_j; r_k / w and the d_j / w are formed first, then the products.
    Returns the dict of ``DeviceSolver.cycle_end``: worst_dof is the first dof of the largest |r_k / w|; a NaN / Inf anywhere in a
    vector of the window or in the weights sets nonfinite (err and err_max NaN, worst_dof -1)."""
    X, G = [np.asarray(x, dtype=np.float64).ravel() for x in X], [np.asarray(g, dtype=np.float64).ravel() for g in G]
    free = np.asarray(free, dtype=bool).ravel()
    m1 = len(X)
    assert 1 <= m1 == len(G) <= MAX_DEPTH + 1
    nonfinite = not all(np.all(np.isfinite(v)) for v in X + G + [np.asarray(w)])
    with np.errstate(invalid="ignore", over="ignore"):
        R = [g - x for x, g in zip(X, G)]
        qk = (R[-1] / w)[free]
        Q = [((R[j + 1] - R[j]) / w)[free] for j in range(m1 - 1)]
        n_free = int(free.sum())
        err = math.sqrt(float((qk * qk).sum()) / n_free) if n_free else 0.0
        err_max, worst = (float(np.abs(qk).max()), int(np.nonzero(free)[0][int(np.argmax(np.abs(qk)))])) if n_free else (0.0, -1)
        m = m1 - 1
        A, b = np.zeros((m, m)), np.zeros(m)
        for i in range(m):
            b[i] = float((Q[i] * qk).sum())
            for j in range(i, m):
                A[i, j] = A[j, i] = float((Q[i] * Q[j]).sum())
    if nonfinite:
        err, err_max, worst = math.nan, math.nan, -1
    return {"err": err, "err_max": err_max, "worst_dof": worst, "n_free": n_free, "nonfinite": nonfinite, "window": m1, "A": A, "b": b}


def mix_direction(G, gamma):
    """sum_j gamma_j g_j - g_k, the sum from gamma_0 g_0 in window order, every product and sum rounded on its own."""
    G = [np.asarray(g, dtype=np.float64).ravel() for g in G]
    acc = float(gamma[0]) * G[0]
    for j in range(1, len(G)):
        acc = acc + float(gamma[j]) * G[j]
    return acc - G[-1]


def cycle_mix(G, gamma, free, alpha=1.0):
    """g_k + alpha (sum_j gamma_j g_j - g_k) on the free dofs, g_k on the others."""
    gk = np.asarray(G[-1], dtype=np.float64).ravel()
    return np.where(np.asarray(free, dtype=bool).ravel(), gk + alpha * mix_direction(G, gamma), gk)


def mix_alpha(prob, G, gamma, free, tau):
    """The step limiter's factor for the correction dx = -(sum_j gamma_j g_j - g_k) (0 on Dirichlet rows) at the state g_k."""
    if tau == 0.0:
        return 1.0
    nf = prob.nf
    dx = np.where(np.asarray(free, dtype=bool).ravel(), -mix_direction(G, gamma), 0.0)
    a = np.asarray(prob.model.a, dtype=np.float64)[:nf - 1]
    return step_limit(a, np.asarray(G[-1], dtype=np.float64).reshape(-1, nf), dx.reshape(-1, nf), tau)[0]


class NumpyPeriodicSystem(PR.NumpyProgrammeSystem):
    """``ops`` of ``run_periodic`` over the NumPy programme system: the window on the host, the report and the mix by the functions
    above.  ``cycle_tol`` = (rtol, atol) of the weights, frozen at ``cycle_open`` from u_n.  A mix leaves u = u_n, no history, fresh
    accumulators and no records, as the device ops do."""

    def __init__(self, prob, u, inv_dt_of_h, cycle_tol=(1e-2, 1e-4), **kw):
        super().__init__(prob, u, inv_dt_of_h, **kw)
        self.cycle_tol, self.depth, self.X, self.G, self.w, self.x_open = cycle_tol, 0, [], [], None, None
        self.newton_iterations = 0

    def solve(self):
        ok, its = super().solve()
        self.newton_iterations += its
        return ok, its

    def state(self):
        return self.un.copy()

    def cycle_open(self, depth):
        self.depth, self.X, self.G = int(depth), [], []
        self.w = cycle_weights(self.un, self.prob.nf, *self.cycle_tol)

    def cycle_close(self):
        self.x_open = None

    def cycle_begin(self):
        self.x_open = self.un.copy()

    def cycle_end(self):
        if len(self.X) == self.depth + 1:
            self.X.pop(0); self.G.pop(0)
        self.X.append(self.x_open); self.G.append(self.un.copy())
        self.x_open = None
        return cycle_report(self.X, self.G, self.w, self.free.ravel())

    def _fresh(self, u, keep_history=False):
        import stern_bc_reference as SR
        from gmpnp_amd import programme as P
        self.u, self.un = np.array(u), np.array(u)
        if not keep_history:      # a mix leaves the handle as set_state(u, u) does; a restart leaves the state and its history alone
            self.unm1 = None
        self.acc = P.fresh_accumulators(SR.stern_displacement(self.prob, self.u))
        self.D_first = self.acc["D_prev"]
        self.records, self.states = [], []

    def cycle_mix(self, gamma, tau):
        free = self.free.ravel()
        d = mix_direction(self.G, gamma)
        if not np.all(np.isfinite(d)):
            self._fresh(self.un, keep_history=True)      # nothing was applied
            return math.nan
        alpha = mix_alpha(self.prob, self.G, gamma, free, tau)
        self._fresh(cycle_mix(self.G, gamma, free, alpha))
        return alpha

    def cycle_restart(self):
        self.X, self.G = [], []
        self._fresh(self.un, keep_history=True)


def plain_march(system, segs, steps_per_segment, tol, max_cycles):
    """Plain iteration of the cycle map: marches period after period until the weighted residual of ``cycle_report`` is <= ``tol`` or
    ``max_cycles`` are marched.  Returns (residuals, converged)."""
    from gmpnp_amd import programme as P
    system.cycle_open(1)
    errs = []
    for _ in range(max_cycles):
        x = system.un.copy()
        P.run_programme(system, segs, steps_per_segment=steps_per_segment)
        errs.append(cycle_report([x], [system.un], system.w, system.free.ravel())["err"])
        if errs[-1] <= tol:
            return errs, True
    return errs, False
