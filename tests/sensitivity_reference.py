"""The transient sensitivities (include/gmpnp.h ``gmpnp_sensitivity_step``) restated in NumPy: a
``NumpyProgrammeSystem`` that carries S = du/dtheta through ``run_programme`` by the recursion
    J(u^{n+1}) s_k^{n+1} = -c_k(u^{n+1}) + inv_dt M s_k^n
with J and inv_dt M = J(inv_dt) - J(0) from ``kinetics_reference.assemble`` at two inv_dt, the columns c_k and the functionals dD, dI_r,
dp_boundary from tangent_reference.py and the combine step of the electrode record applied to the derivatives; and the maps the tests
difference it against (the whole march re-run at theta +- eps).  Imported like programme_reference.py; not a conftest.  Test
infrastructure only (1D)."""
import numpy as np
import scipy.sparse.linalg as spla

import programme_reference as PR
import response_reference as R
import tangent_reference as T
from gmpnp_amd import programme as P

SENS_KEYS = ("t", "h", "dD", "d_dD_dt", "dI", "dQ", "dQ_D", "dp_boundary")


def step_mass(prob, u, inv_dt):
    """inv_dt M as the difference of two assembled Jacobians (CSR)."""
    return (R.jacobian(prob, u, inv_dt) - R.jacobian(prob, u, 0.0)).tocsr()


def right_hand_sides(prob, u, params, S, inv_dt):
    """-c_k + inv_dt M s_k for every column, (n, ndof)."""
    Mi = step_mass(prob, u, inv_dt)
    return np.array([-T.column(prob, u, q) + Mi @ S[k] for k, q in enumerate(params)])


def functionals4(prob, u, s, param):
    """(dD, dI padded to four reactions, dp_boundary) of the column s."""
    dD, dI, dp = T.functionals(prob, u, s, param)
    dI4 = np.zeros(P.MAX_SURFACE_REACTIONS)
    dI4[:len(dI)] = dI
    return float(dD), dI4, float(dp)


class NumpySensitivitySystem(PR.NumpyProgrammeSystem):
    """``NumpyProgrammeSystem`` with the sensitivities of the parameter codes ``params``.  ``start`` = "zero": S = 0 (the start state is
    frozen); "steady": S = the tangent of the steady state at inv_dt = 0 (``u`` is the steady state of ``prob``).  ``record`` (accepted
    steps only) advances S; a rejected attempt never touches it."""

    def __init__(self, prob, u, inv_dt_of_h, params, start="zero", **kw):
        super().__init__(prob, u, inv_dt_of_h, **kw)
        self.params = [int(q) for q in params]
        n = len(self.params)
        self.S = T.tangent(prob, self.u, self.params, inv_dt=0.0)[0] if start == "steady" else np.zeros((n, prob.ndof))
        self.sacc = [P.fresh_accumulators(functionals4(prob, self.u, self.S[k], q)[0]) for k, q in enumerate(self.params)]
        self.srecords, self.rhs = [], None

    def record(self, t, h, seg, p):
        super().record(t, h, seg, p)
        self.sensitivity_step(t, h)

    def sensitivity_step(self, t, h):
        prob, u = self.prob, self.u
        inv_dt = float(prob.model.inv_dt)
        lu = spla.splu(R.jacobian(prob, u, inv_dt).tocsc())
        self.rhs = right_hand_sides(prob, u, self.params, self.S, inv_dt)
        self.S = np.array([lu.solve(b) for b in self.rhs])
        row = []
        for k, q in enumerate(self.params):
            dD, dI, dp = functionals4(prob, u, self.S[k], q)
            d_dD_dt = P.electrode_record_combine(self.sacc[k], h, dD, dI)
            row.append({"t": t, "h": h, "dD": dD, "d_dD_dt": d_dD_dt, "dI": dI, "dQ": np.array(self.sacc[k]["Q"]), "dQ_D": self.sacc[k]["Q_D"],
                        "dp_boundary": dp})
        self.srecords.append(row)

    def sensitivity_arrays(self):
        """Every field as an array (steps, columns, ...)."""
        return {key: np.array([[r[key] for r in row] for row in self.srecords]) for key in SENS_KEYS}


class NumpyTransient:
    """``fit.TransientCurve``'s system over the NumPy restatement: the kept problem and its steady start state; a trial moves the
    parameters (``fit_reference.moved``), predicts the start with the kept tangent, re-converges it and marches a
    ``NumpySensitivitySystem`` from the steady tangent in fixed mode.  Times in seconds by ``time_constant``."""

    def __init__(self, prob, u, inv_dt_of_h, segs, steps_per_segment, codes, time_constant=1.0, sigma_unit=1.0, newton=None):
        self.inv, self.segs, self.steps, self.codes = inv_dt_of_h, segs, int(steps_per_segment), tuple(int(c) for c in codes)
        self.tc, self.sigma_unit, self.newton_kw = float(time_constant), float(sigma_unit), newton
        self.kept = dict(prob=prob, u=np.array(u, dtype=np.float64))
        self.pending, self.newton, self.marches = None, 0, 0

    def start(self, delta):
        import fit_reference as FR
        k = self.kept
        prob = FR.moved(k["prob"], self.codes, delta)
        u0 = k["u"]
        if np.any(delta):
            u0 = u0 + np.asarray(delta) @ T.tangent(k["prob"], k["u"], self.codes, inv_dt=0.0)[0]
        self.pending = dict(prob=prob, u=reconverged(prob, u0))
        self.newton = 8
        return True

    def march(self):
        p = self.pending
        s = NumpySensitivitySystem(p["prob"], p["u"], self.inv, self.codes, start="steady", newton=self.newton_kw)
        try:
            P.run_programme(s, self.segs, steps_per_segment=self.steps)
        except RuntimeError:
            return None
        self.marches += 1
        rec, A = s.arrays(), s.sensitivity_arrays()
        q = self.sigma_unit
        return {"t": rec["t"] * self.tc, "i_CO": rec["I"][:, 0], "i_H2": rec["I"][:, 1], "surface_charge": q * rec["D"], "newton": self.newton,
                "slopes": {"i_CO": A["dI"][:, :, 0], "i_H2": A["dI"][:, :, 1], "surface_charge": q * A["dD"]}}

    def keep(self):
        self.kept = self.pending


def shifted_segments(segs, delta):
    """The programme with every potential moved by ``delta``: the offset parameter."""
    return [(t0, t1, p0 + delta, p1 + delta) for t0, t1, p0, p1 in segs]


def reconverged(prob, u, iterations=8):
    """The steady state of ``prob`` (inv_dt = 0) from the nearby state ``u``: a fixed number of full Newton steps with sparse LU, which by
    the quadratic convergence leaves the state at its rounding floor whatever norm the residual has there."""
    import kinetics_reference as K
    q = R.with_inv_dt(prob, 0.0)
    u = np.array(u, dtype=np.float64)
    for _ in range(iterations):
        F, A = K.assemble(q, u, u, want_jacobian=True)
        u = u - spla.splu(A.tocsc()).solve(F)
    assert np.isfinite(u).all()
    return u


def marched(prob, u, inv_dt_of_h, segs, param, delta, start, steps_per_segment=4, newton=None):
    """The fixed-mode march re-run with parameter ``param`` moved by ``delta``: the arrays of the electrode records and the final state.
    "steady": the start is the steady state of the moved problem, re-converged from ``u``; "zero": the start state stays ``u``.  The
    offset moves the potential of the start with the waveform."""
    q = T.with_parameter(prob, param, delta)
    u0 = np.array(u, dtype=np.float64)
    if start == "steady":
        u0 = reconverged(q, u0)
    sys_ = PR.NumpyProgrammeSystem(q, u0, inv_dt_of_h, newton=newton)
    P.run_programme(sys_, shifted_segments(segs, delta) if param == 0 else segs, steps_per_segment=steps_per_segment)
    return sys_.arrays(), sys_.u


def central_difference(prob, u, inv_dt_of_h, segs, param, eps, start, **kw):
    """(d records / d theta as a dict of arrays over D, dD_dt, I, Q, Q_D, p_boundary; d u_end / d theta) by central differences."""
    (a, ua), (b, ub) = (marched(prob, u, inv_dt_of_h, segs, param, d, start, **kw) for d in (eps, -eps))
    return {k: (a[k] - b[k]) / (2.0 * eps) for k in ("D", "dD_dt", "I", "Q", "Q_D", "p_boundary")}, (ua - ub) / (2.0 * eps)
