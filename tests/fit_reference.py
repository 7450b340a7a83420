"""The fit of the electrode kinetics (gmpnp_amd/fit.py) over the NumPy restatement of the tangent
(tangent_reference.py): the evaluator ``fit.LevenbergMarquardt`` is handed, planted data, and scripted evaluators for the rule's own
tests (imported like tangent_reference.py; not a conftest).  Test infrastructure only (1D)."""
import math

import numpy as np

import response_reference as R
import tangent_reference as T
from gmpnp_amd import fit as ft
from gmpnp_amd import polarisation as pol

POTENTIALS = (-5.0, -6.0, -7.0, -8.0, -9.0, -10.0)
FOUR = ("i0_CO", "i0_H2", "alpha_CO", "alpha_H2")
FIVE = FOUR + ("stern_length",)
DISPLACEMENT = {"i0_CO": 0.7, "i0_H2": -0.5, "alpha_CO": 0.08, "alpha_H2": -0.06, "stern_length": 0.2}   # of ln i0, alpha, ln lam


def moved(prob, codes, delta):
    for c, d in zip(codes, delta):
        prob = T.with_parameter(prob, c, float(d))
    return prob


def theta_of(prob, codes):
    out = []
    for c in codes:
        kind, r = pol.param_kind(c), pol.param_reaction(c)
        out.append(math.log(prob.kinetics.reactions[r].k) if kind == 1 else prob.kinetics.reactions[r].alpha if kind == 2 else math.log(prob.stern.lam))
    return np.array(out)


def steady_curve(prob, u, potentials):
    """The steady states of ``prob`` at ``potentials`` by the continuation rule from the state ``u`` (near the steady state at the
    first of them): [(u_m, currents, displacement)], Newton iterations."""
    out, newton, at = [], 0, float(prob.stern.p_electrode)
    sys_ = T.NumpySystem(R.with_potential(prob, at), u)
    for v in potentials:
        if v == at:
            ok, its, _ = sys_.solve()
            assert ok
            newton += its
        else:
            _, _, its, stop = pol.run_continuation(sys_, at, v, v - at)
            assert stop == "v_end"
            newton += sum(its)
        out.append((sys_.u.copy(), T.currents(sys_.prob, sys_.u), T.displacement(sys_.prob, sys_.u)))
        at = v
    return out, newton


def planted_data(prob, u, potentials=POTENTIALS, surface_charge=False, sigma_unit=1.0):
    pts, _ = steady_curve(prob, u, potentials)
    data = {"electrode_voltage": np.array(potentials), "i_CO": np.array([p[1][0] for p in pts]), "i_H2": np.array([p[1][1] for p in pts])}
    if surface_charge:
        data["surface_charge"] = sigma_unit * np.array([p[2] for p in pts])
    return data


class NumpyCurve:
    """``fit.DeviceCurve``'s operations over the NumPy restatement: the kept problem and per-point states, a trial by the predictor
    u_m + sum_k delta_k z_k (``predictor`` True) and Newton at inv_dt = 0, the Jacobian from ``tangent_reference.tangent``."""

    def __init__(self, prob, u, data, codes, predictor=True, sigma_unit=1.0):
        self.data, self.codes, self.predictor, self.sigma_unit = data, tuple(codes), predictor, sigma_unit
        self.V = [float(v) for v in data["electrode_voltage"]]
        pts, newton = steady_curve(prob, u, self.V)
        self.kept = self.assembled(prob, [p[0] for p in pts], newton)
        self.last = self.kept

    def assembled(self, prob, states, newton):
        r, J, z = [], [], []
        for m, (v, u) in enumerate(zip(self.V, states)):
            q = R.with_potential(prob, v)
            I, D = T.currents(q, u), T.displacement(q, u)
            if not np.all(I > 0.0):
                return None
            zz, dD, dI, _ = T.tangent(q, u, self.codes)
            values = {"i_CO": float(I[0]), "i_H2": float(I[1]), "surface_charge": self.sigma_unit * D}
            slopes = {"i_CO": dI[:, 0], "i_H2": dI[:, 1], "surface_charge": self.sigma_unit * dD}
            rr, JJ = ft.residual_rows(self.data, m, values, slopes)
            r += rr; J += JJ; z.append(zz)
        return dict(prob=prob, states=states, z=z, r=np.array(r), J=np.array(J).reshape(len(r), len(self.codes)), newton=newton)

    def trial(self, theta, delta):
        if not np.any(delta):
            self.last = self.kept
            return self.kept
        k = self.kept
        prob = moved(k["prob"], self.codes, delta)
        states, newton = [], 0
        for m, v in enumerate(self.V):
            u0 = k["states"][m] + (np.asarray(delta) @ k["z"][m] if self.predictor else 0.0)
            u, its, ok = T.steady_state(R.with_potential(prob, v), u0)
            newton += its
            if not ok:
                self.failed_newton = newton
                return None
            states.append(u)
        self.last = self.assembled(prob, states, newton)
        if self.last is None:
            self.failed_newton = newton
        return self.last

    def accept(self):
        self.kept = self.last


class Scripted:
    """An evaluator over a closed-form model ``model(theta) -> (r, J)``; ``fail(theta)`` True makes the trial a failed one."""

    def __init__(self, model, fail=None):
        self.model, self.fail, self.trials, self.kept_theta, self.last_theta = model, fail, [], None, None

    def trial(self, theta, delta):
        t = np.asarray(theta, dtype=np.float64) + np.asarray(delta, dtype=np.float64)
        self.trials.append((np.array(theta, dtype=np.float64), np.array(delta, dtype=np.float64)))
        if self.fail is not None and self.fail(t):
            return None
        r, J = self.model(t)
        self.last_theta = t
        return dict(r=r, J=J, newton=1)

    def accept(self):
        self.kept_theta = self.last_theta


def tafel_law(potentials, data_theta):
    """Two reactions I_r = exp(ln k_r - alpha_r V): theta = (ln k_0, ln k_1, alpha_0, alpha_1); residuals ln I - ln I_data."""
    V = np.asarray(potentials, dtype=np.float64)

    def ln_I(theta):
        return np.concatenate([theta[0] - theta[2] * V, theta[1] - theta[3] * V])

    target = ln_I(np.asarray(data_theta, dtype=np.float64))

    def model(theta):
        J = np.zeros((2 * V.size, 4))
        J[:V.size, 0], J[V.size:, 1], J[:V.size, 2], J[V.size:, 3] = 1.0, 1.0, -V, -V
        return ln_I(theta) - target, J
    return model
