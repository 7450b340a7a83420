"""A NumPy system for ``gmpnp_amd.programme.run_programme``: the operations the loop asks of a handle, over
the kinetics and Stern restatements (kinetics_reference.py: assemble, newton_loop, currents; stern_bc_reference.py: stern_displacement)
and the estimator of time_step_reference.py, with the electrode record formed by the Python statement of the combine step (imported
like tangent_reference.py; not a conftest).  Test infrastructure only."""
import numpy as np

import budget_reference as B
import kinetics_reference as K
import response_reference as R
import stern_bc_reference as SR
import time_step_reference as TS
from gmpnp_amd import programme as P

RECORD_KEYS = ("t", "h", "p_M", "p_boundary", "D", "dD_dt", "I", "Q", "Q_D", "u_boundary", "segment")


def boundary_means(prob, u):
    """(p_boundary, u_boundary (ns,)): sum_I w_I u_{I,f} / sum_I w_I over the Stern boundary with the kinetics' weights."""
    nf = prob.nf
    nodes, w = K.boundary_weights(prob)
    u2d = np.asarray(u, dtype=np.float64).reshape(-1, nf)
    m = (w[:, None] * u2d[nodes]).sum(axis=0) / w.sum()
    return float(m[nf - 1]), m[:nf - 1]


def currents4(prob, u):
    I = np.zeros(P.MAX_SURFACE_REACTIONS)
    if getattr(prob, "kinetics", None) is not None:
        c = K.currents(prob, u)
        I[:len(c)] = c
    return I


def budget_row(prob, u, un):
    """(table, scale, raw) of one step with the Stern and the kinetic term in it, as gmpnp_species_budget reports them: the table of
    ``budget_reference.budget`` (which knows neither) with the integrated kinetic fluxes added to the species' point entries, the
    Stern displacement to the potential's, ``closure`` the sum over the free rows of the residual that holds both terms, and
    ``dirichlet`` the remainder of the identity.  raw: that residual before the Dirichlet rows are overwritten, (nv, nf)."""
    nf, ns = prob.nf, prob.nf - 1
    table, scale = B.budget(prob, u, un)
    if getattr(prob, "kinetics", None) is not None:
        fl = K.species_fluxes(prob, u)
        table[:ns, B.POINT] += fl
        scale[:ns, B.POINT] += np.abs(fl)
    D = SR.stern_displacement(prob, u)
    table[ns, B.POINT] += D
    scale[ns, B.POINT] += abs(D)
    raw = K.assemble(prob, u, un, want_jacobian=False, apply_bc=False)[0].reshape(-1, nf)
    free = TS.free_mask(prob)
    lhs = (B.STO, B.REA, B.WALL, B.EXIT, B.POINT)
    for f in range(nf):
        table[f, B.CLO], scale[f, B.CLO] = raw[free[:, f], f].sum(), np.abs(raw[free[:, f], f]).sum()
    table[:, B.DIR] = table[:, lhs].sum(axis=1) - table[:, B.CLO]
    scale[:, B.DIR] = scale[:, lhs].sum(axis=1) + scale[:, B.CLO]
    return table, scale, raw


class NumpyProgrammeSystem:
    """``ops`` of ``run_programme`` over a problem with a Stern layer (kinetics on or off) from the state ``u`` (u_n = u, no history).
    ``inv_dt_of_h``: the model's inv_dt for a step h; ``newton``: keywords of ``kinetics_reference.newton_loop``; ``tol`` = (rtol,
    atol) of the estimator; ``fail_solves``: indices (0-based, counted over all solves) of Newton solves that are made to fail;
    ``budget``: every accepted step takes its ``budget_row`` while u_n is the previous state and inv_dt the step's (``budgets``, with
    the step's last Newton residual in ``residuals``)."""

    def __init__(self, prob, u, inv_dt_of_h, newton=None, tol=(1e-2, 1e-4), fail_solves=(), budget=False):
        self.prob, self.inv_dt_of_h = prob, inv_dt_of_h
        self.newton = dict(maximum_iterations=25, relative_tolerance=1e-13, absolute_tolerance=1e-7) if newton is None else dict(newton)
        self.tol = tol
        self.u, self.un, self.unm1 = np.array(u, dtype=np.float64), np.array(u, dtype=np.float64), None
        self.acc = P.fresh_accumulators(SR.stern_displacement(prob, self.u))
        self.D_first = self.acc["D_prev"]
        self.records, self.states, self.solves, self.steps = [], [], 0, []
        self.fail_solves = set(fail_solves)
        self.free = TS.free_mask(prob)
        self.budget, self.budgets, self.residuals, self.last_residual = bool(budget), [], [], None

    def set_potential(self, p):
        self.prob = R.with_potential(self.prob, p)

    def set_step(self, h):
        self.prob = R.with_inv_dt(self.prob, self.inv_dt_of_h(h))
        self.steps.append((float(self.prob.stern.p_electrode), float(h)))

    def solve(self):
        k, self.solves = self.solves, self.solves + 1
        if k in self.fail_solves:
            return False, 0
        u, st = K.newton_loop(self.prob, self.u, self.un, **self.newton)
        ok = bool(st.converged and np.all(np.isfinite(u)))
        if ok:
            self.u, self.last_residual = u, float(st.residuals[-1])
        return ok, st.iterations

    def estimate(self, h, h_prev):
        nf = self.prob.nf
        m1 = None if self.unm1 is None else self.unm1.reshape(-1, nf)
        return TS.time_error(self.u.reshape(-1, nf), self.un.reshape(-1, nf), m1, h, h_prev, self.tol[0], self.tol[1], self.free)

    def record(self, t, h, seg, p):
        if self.budget:
            self.budgets.append(budget_row(self.prob, self.u, self.un))
            self.residuals.append(self.last_residual)
        D, I = SR.stern_displacement(self.prob, self.u), currents4(self.prob, self.u)
        dD_dt = P.electrode_record_combine(self.acc, h, D, I)
        pb, ub = boundary_means(self.prob, self.u)
        self.records.append({"t": t, "h": h, "p_M": p, "p_boundary": pb, "D": D, "dD_dt": dD_dt, "I": I.copy(), "Q": np.array(self.acc["Q"]),
                             "Q_D": self.acc["Q_D"], "u_boundary": ub, "segment": seg})

    def accept(self):
        self.unm1, self.un = self.un, self.u.copy()

    def reject(self):
        self.u = self.un.copy()

    def breakpoint(self, seg, t):
        self.states.append((seg, t, self.u.copy()))

    def arrays(self):
        return {k: np.array([r[k] for r in self.records]) for k in RECORD_KEYS}
