"""Electrode kinetics fitted to polarisation data (``--fit_data`` of the 1D MPNP driver,
``gmpnp_electrode_tangent`` / ``gmpnp_parameter_advance``): the parameters by name, the data format, the Levenberg-Marquardt rule over
an evaluator it is handed, the evaluator over a driver run's own handle, and the physical tables of ``fit.npz``.

The residuals of a curve with data at the potentials V_m are, per reaction r with data and (where given) for the surface charge,

    w (ln I_r,model(V_m) - ln I_r,data)          row  w dI_r/dtheta_k / I_r
    w (sigma_model(V_m) - sigma_data) / max |sigma_data|          row  w dD/dtheta_k in the same units

with the rows from the steady tangent (inv_dt = 0) at every point: exact sensitivities out of one cyclic reduction per point.  The
parameters are ln i0 (= ln k_r), alpha_r and ln stern_length.  No reference counterpart.
"""
from __future__ import annotations

import math

import numpy as np

from . import polarisation as pol

PARAMETERS = {"i0_CO": 16, "i0_H2": 17, "alpha_CO": 32, "alpha_H2": 33, "stern_length": 48}   # the tangent's codes: no new ones
DEFAULT_PARAMS = ("i0_CO", "i0_H2", "alpha_CO", "alpha_H2")
CURRENT_KEYS = ("i_CO", "i_H2")               # reaction 0 and 1 of kinetics.edl_tafel
DATA_KEYS = ("electrode_voltage",) + CURRENT_KEYS + ("surface_charge",) + tuple("weight_" + k for k in CURRENT_KEYS + ("surface_charge",))
FIT_KEYWORDS = ("fit",)
LAMBDA_START, LAMBDA_FLOOR, LAMBDA_STALL = 1.0e-3, 1.0e-12, 1.0e8
STEP_TOL, MAX_TRIALS, RANK_TOL = 1.0e-8, 50, 1.0e-8
LOG_CAP, ALPHA_CAP = 2.0, 0.25                # the largest move of a log parameter / of an alpha in one trial
METADATA_KEYS = ("fit_parameters", "fit_values", "fit_standard_errors", "fit_stop_reason", "fit_trials", "fit_rejected_trials",
                 "fit_newton_iterations", "fit_final_cost", "fit_condition_number")


def is_log(code):
    """ln k_r and ln lam move as logarithms, alpha_r as it is."""
    return pol.param_kind(code) in (1, 3)


def param_codes(names):
    """The tangent's codes of the parameter names ``names``; ValueError for an unknown or repeated name or none at all."""
    names = tuple(names)
    if not names or any(n not in PARAMETERS for n in names) or len(set(names)) != len(names):
        raise ValueError("fit: params are distinct names out of %s" % ", ".join(PARAMETERS))
    return tuple(PARAMETERS[n] for n in names)


# ---- the options under a step (gmpnp_host_rules.h: parameter_move), operation for operation -------------------------------------------
def moved_options(stern, kinetics, n_species, params, dtheta):
    """(stern, kinetics, valid) after the step ``dtheta`` in the parameters ``params``: dicts as ``DeviceSolver.electrode_options``
    returns them (``kinetics`` None: off).  p_M: p_electrode += d in both; ln k_r: k_r *= exp(d); alpha_r += d; ln lam: lam *= exp(d);
    then the setters' validity rules."""
    stern = dict(stern)
    kinetics = None if kinetics is None else {"reactions": [dict(r) for r in kinetics["reactions"]], "p_electrode": kinetics["p_electrode"]}
    for p, d in zip(params, dtheta):
        kind, r = pol.param_kind(p), pol.param_reaction(p)
        d = float(d)
        if kind == 0:
            stern["p_electrode"] = stern["p_electrode"] + d
        elif kind == 3:
            stern["lam"] = stern["lam"] * _exp(d)
        elif kind in (1, 2) and kinetics is not None and r < len(kinetics["reactions"]):
            rx = kinetics["reactions"][r]
            if kind == 1:
                rx["k"] = rx["k"] * _exp(d)
            else:
                rx["alpha"] = rx["alpha"] + d
        else:
            return stern, kinetics, False
    if kinetics is not None:
        kinetics["p_electrode"] = stern["p_electrode"]
    fin = math.isfinite
    ok = fin(stern["p_electrode"]) and stern["lam"] > 0.0 and fin(stern["lam"]) and \
        (stern["model"] == "linear" or (stern["eps_surface"] > 0.0 and fin(stern["eps_surface"])))
    if kinetics is not None:
        ok = ok and fin(kinetics["p_electrode"]) and all(fin(rx["k"]) and fin(rx["alpha"]) and fin(rx["p_eq"]) and all(fin(v) for v in rx["nu"].values())
                                                         for rx in kinetics["reactions"])
    return stern, kinetics, bool(ok)


def _exp(d):
    try:
        return math.exp(d)
    except OverflowError:
        return math.inf


# ---- data ----------------------------------------------------------------------------------------------------------------------------
def load_data(path):
    """The columns of a data file: an ``.npz`` with the keys ``DATA_KEYS`` (what ``polarisation.npz`` holds is accepted as it is; its
    other keys are not read) or a CSV with those names in a header row."""
    path = str(path)
    if path.lower().endswith(".npz"):
        with np.load(path) as z:
            return {k: np.asarray(z[k], dtype=np.float64).ravel() for k in DATA_KEYS if k in z.files}
    with open(path) as fh:
        header = [h.strip() for h in fh.readline().lstrip("#").split(",")]
        rows = [line.split(",") for line in fh if line.strip()]
    if "electrode_voltage" not in header or any(len(r) != len(header) for r in rows):
        raise ValueError("fit: a CSV needs a header row with electrode_voltage and as many values per row")
    try:
        table = np.array([[float(x) for x in r] for r in rows], dtype=np.float64).reshape(len(rows), len(header))
    except ValueError:
        raise ValueError("fit: a CSV holds numbers below its header row") from None
    return {h: table[:, j].copy() for j, h in enumerate(header) if h in DATA_KEYS}


def check_data(data, electrode_voltage, n_params):
    """The refusals of the data and its points ordered by their distance from ``electrode_voltage``.  Returns a dict: ``electrode_voltage``
    (n,), per quantity with data (``i_CO``, ``i_H2``, ``surface_charge``) its values and ``weight_<quantity>`` (n,), ``quantities``."""
    if "electrode_voltage" not in data or not any(k in data for k in CURRENT_KEYS):
        raise ValueError("fit: the data hold electrode_voltage and i_CO and / or i_H2 (optional: surface_charge, weight_*)")
    V = np.asarray(data["electrode_voltage"], dtype=np.float64).ravel()
    out = {"quantities": tuple(k for k in CURRENT_KEYS + ("surface_charge",) if k in data)}
    for k in out["quantities"]:
        v = np.asarray(data[k], dtype=np.float64).ravel()
        w = np.asarray(data.get("weight_" + k, np.ones(V.size)), dtype=np.float64).ravel()
        if w.size == 1:
            w = np.full(V.size, w[0])
        if v.size != V.size or w.size != V.size:
            raise ValueError("fit: %s has %d values and %d weights for %d potentials" % (k, v.size, w.size, V.size))
        if not (np.isfinite(v).all() and np.isfinite(w).all() and np.all(w >= 0.0)):
            raise ValueError("fit: %s and its weights must be finite, the weights >= 0" % k)
        if k in CURRENT_KEYS and np.any(v <= 0.0):
            raise ValueError("fit: %s must be > 0 (the residual is that of ln I)" % k)
        out[k], out["weight_" + k] = v, w
    if V.size < 1 or not np.isfinite(V).all():
        raise ValueError("fit: the potentials must be finite")
    if len(set(V.tolist())) != V.size:
        raise ValueError("fit: a potential is repeated")
    d = V - float(electrode_voltage)
    if np.any(d > 0.0) and np.any(d < 0.0):
        raise ValueError("fit: the potentials must all lie at or on one side of electrode_voltage (%g)" % electrode_voltage)
    if "surface_charge" in out["quantities"] and not np.abs(out["surface_charge"]).max() > 0.0:
        raise ValueError("fit: surface_charge is zero everywhere")
    n_res = V.size * len(out["quantities"])
    if n_res < int(n_params):
        raise ValueError("fit: %d residuals are fewer than the %d parameters" % (n_res, n_params))
    order = np.argsort(np.abs(d), kind="stable")
    out["electrode_voltage"] = V[order]
    for k in out["quantities"]:
        out[k], out["weight_" + k] = out[k][order], out["weight_" + k][order]
    return out


def residual_rows(data, m, values, slopes):
    """The residuals of point ``m`` and their Jacobian rows from the model's ``values`` {quantity: value} and ``slopes`` {quantity:
    (n_params,) d value / d theta}: ln I for the currents, sigma / max |sigma_data| for the surface charge."""
    r, J = [], []
    for k in data["quantities"]:
        w = float(data["weight_" + k][m])
        if k in CURRENT_KEYS:
            r.append(w * (math.log(values[k]) - math.log(float(data[k][m]))))
            J.append(w * np.asarray(slopes[k], dtype=np.float64) / values[k])
        else:
            s = float(np.abs(data[k]).max())
            r.append(w * (values[k] - float(data[k][m])) / s)
            J.append(w * np.asarray(slopes[k], dtype=np.float64) / s)
    return r, J


# ---- the rule ------------------------------------------------------------------------------------------------------------------------
class LevenbergMarquardt:
    """Levenberg-Marquardt over an evaluator:

        evaluator.trial(theta, delta) -> None | dict(r=(N,), J=(N, n), newton=int)   the residuals and their Jacobian at theta + delta
                                                    (``theta``: the last accepted parameters; the first call has delta = 0); None: the
                                                    trial failed (a Newton failure, a numeric error, an integrated rate <= 0)
        evaluator.accept()                          the last trial becomes what the next one starts from; a trial that is not accepted
                                                    changes nothing that is kept

    The step solves (J^T J + lambda diag(J^T J)) delta = -J^T r and is scaled down as a whole so that no log parameter moves by more
    than 2 and no alpha by more than 0.25.  A trial of lower cost |r|^2 / 2 is accepted and lambda becomes max(lambda / 10, 1e-12);
    any other is rejected and lambda grows tenfold.  Stops: "converged" (max |delta| < 1e-8 after an accepted trial), "stalled"
    (lambda > 1e8), "max_iterations" (50 trials), "rank_deficient" (before the first step: the smallest over the largest singular
    value of the column-normalised Jacobian < 1e-8; nothing is moved, the covariance is NaN)."""

    def __init__(self, evaluator, log_parameter, max_trials=MAX_TRIALS):
        self.evaluator, self.log = evaluator, np.asarray(log_parameter, dtype=bool)
        self.max_trials = int(max_trials)

    def capped(self, delta):
        big_log = float(np.abs(delta[self.log]).max()) if self.log.any() else 0.0
        big_alpha = float(np.abs(delta[~self.log]).max()) if (~self.log).any() else 0.0
        s = 1.0
        if big_log > LOG_CAP:
            s = min(s, LOG_CAP / big_log)
        if big_alpha > ALPHA_CAP:
            s = min(s, ALPHA_CAP / big_alpha)
        return delta * s

    def run(self, theta0):
        theta = np.array(theta0, dtype=np.float64)
        n = theta.size
        first = self.evaluator.trial(theta, np.zeros(n))
        if first is None:
            raise RuntimeError("fit: the model could not be evaluated at the starting parameters")
        self.evaluator.accept()
        r, J = np.asarray(first["r"], dtype=np.float64), np.asarray(first["J"], dtype=np.float64).reshape(-1, n)
        cost, lam = 0.5 * float(r @ r), LAMBDA_START
        history = [dict(cost=cost, lam=lam, accepted=True, newton=int(first.get("newton", 0)), step=0.0)]
        sv = column_scaled_singular_values(J)
        stop = None
        if not (np.isfinite(sv).all() and sv[0] > 0.0 and sv[-1] / sv[0] >= RANK_TOL):
            stop = "rank_deficient"
        trials = 0
        while stop is None:
            if trials >= self.max_trials:
                stop = "max_iterations"
                break
            A, g = J.T @ J, J.T @ r
            try:
                delta = self.capped(np.linalg.solve(A + lam * np.diag(np.diag(A)), -g))
            except np.linalg.LinAlgError:
                delta = np.full(n, np.nan)
            t = self.evaluator.trial(theta, delta) if np.isfinite(delta).all() else None
            trials += 1
            step = float(np.abs(delta).max())
            t_cost = None if t is None else 0.5 * float(np.asarray(t["r"], dtype=np.float64) @ np.asarray(t["r"], dtype=np.float64))
            good = t_cost is not None and t_cost < cost
            history.append(dict(cost=t_cost if t_cost is not None else float("nan"), lam=lam, accepted=bool(good),
                                newton=int(t.get("newton", 0)) if t is not None else int(getattr(self.evaluator, "failed_newton", 0)), step=step))
            if good:
                self.evaluator.accept()
                theta = theta + delta
                r, J, cost = np.asarray(t["r"], dtype=np.float64), np.asarray(t["J"], dtype=np.float64).reshape(-1, n), t_cost
                lam = max(lam / 10.0, LAMBDA_FLOOR)
                if step < STEP_TOL:
                    stop = "converged"
            else:
                lam = lam * 10.0
                if lam > LAMBDA_STALL:
                    stop = "stalled"
        return finish(theta, r, J, stop, history, rank_deficient=(stop == "rank_deficient"))


def column_scaled_singular_values(J):
    """The singular values (descending) of J with every column scaled to unit length (a zero column stays zero)."""
    J = np.asarray(J, dtype=np.float64)
    norms = np.sqrt((J * J).sum(axis=0))
    sv = np.linalg.svd(J / np.where(norms > 0.0, norms, 1.0), compute_uv=False)
    return np.concatenate([sv, np.zeros(max(J.shape[1] - sv.size, 0))])   # (fewer rows than columns: the missing ones are zero)


def finish(theta, r, J, stop, history, rank_deficient=False):
    """The result of a fit: covariance s^2 (J^T J)^-1 with s^2 = |r|^2 / (N - n) (1 where N = n), standard errors, correlation, the
    singular values of the column-scaled Jacobian and the counts of the history."""
    N, n = J.shape
    s2 = float(r @ r) / (N - n) if N > n else 1.0
    cov = np.full((n, n), np.nan)
    if not rank_deficient:
        try:
            cov = s2 * np.linalg.inv(J.T @ J)
        except np.linalg.LinAlgError:
            pass
    with np.errstate(invalid="ignore", divide="ignore"):
        se = np.sqrt(np.diag(cov))
        corr = cov / np.outer(se, se)
    sv = column_scaled_singular_values(J)
    trials = history[1:]
    return {"theta": theta, "residuals": r, "jacobian": J, "stop_reason": stop, "covariance": cov, "standard_errors": se, "correlation": corr,
            "singular_values": sv, "condition_number": float(sv[0] / sv[-1]) if sv[-1] > 0.0 else float("inf"),
            "cost": 0.5 * float(r @ r), "history": history, "trials": len(trials), "rejected_trials": sum(1 for h in trials if not h["accepted"]),
            "newton_iterations": int(sum(h["newton"] for h in history))}


# ---- the evaluator over a driver run's handle ----------------------------------------------------------------------------------------
def records_of(stern, kinetics, p):
    """(SternLayer, SurfaceKinetics or None) at the potential ``p`` from option dicts (``DeviceSolver.electrode_options``)."""
    from .problem import SternLayer, SurfaceKinetics, SurfaceReaction
    s = SternLayer(stern["model"], float(p), stern["lam"], stern["eps_surface"])
    k = None
    if kinetics is not None:
        k = SurfaceKinetics([SurfaceReaction(k=r["k"], alpha=r["alpha"], p_eq=r["p_eq"], reactant=r["reactant"], nu=dict(r["nu"]))
                             for r in kinetics["reactions"]], float(p))
    return s, k


def theta_of(stern, kinetics, codes):
    """ln k_r, alpha_r and ln lam of the option dicts, for the parameter codes ``codes``."""
    out = []
    for c in codes:
        kind, r = pol.param_kind(c), pol.param_reaction(c)
        out.append(math.log(kinetics["reactions"][r]["k"]) if kind == 1 else kinetics["reactions"][r]["alpha"] if kind == 2 else math.log(stern["lam"]))
    return np.array(out, dtype=np.float64)


class DeviceCurve:
    """The evaluator of ``LevenbergMarquardt`` over a driver run (``EDLRun``) and its own handle; it owns no second handle.

    ``prepare()``: ``set_time_step(0)``, one Newton solve at the run's potential, then ``polarisation.run_continuation`` segment by
    segment (a one-target grid each: uneven spacings work and the halving rule stays) to every data potential; every converged state
    is kept on the host.  A trial theta + delta, per point: ``set_state(u_m)``, the options at (theta, V_m), ``electrode_tangent`` of
    the fit's parameters, ``parameter_advance(delta)`` with the run's ``step_fraction``, ``newton_solve`` (``polarisation.NEWTON``),
    the currents and the displacement, and the tangent again for the Jacobian (speculatively: an accepted trial needs no second
    visit).  A point that fails is tried once more from the converged trial state of its neighbour by one continuation segment in p_M
    at the trial parameters; if that fails too the trial fails.  ``predictor`` = False sets the trial's parameters with ``set_stern`` /
    ``set_kinetics`` and starts Newton from u_m."""

    def __init__(self, run, data, codes, sigma_unit, predictor=True, solver_parameters=None):
        from . import backend
        self.run, self.dev, self.data, self.codes = run, run.sys.dev, data, tuple(int(c) for c in codes)
        self.sigma_unit, self.predictor = float(sigma_unit), bool(predictor)
        self.V = [float(v) for v in data["electrode_voltage"]]
        self.options = backend.newton_options(backend.with_step_fraction(solver_parameters or pol.NEWTON, run.step_fraction), dim=1)
        self.n_species = run.problem.nf - 1
        self.kept, self.last = None, None
        self.failed_newton, self.retried_points = 0, 0

    # -- the handle at a point ---------------------------------------------------------------------------------------------------------
    def set_options(self, stern, kinetics, p):
        s, k = records_of(stern, kinetics, p)
        self.run.stern, self.run.kinetics = s, k
        self.dev.set_stern(s)
        self.dev.set_kinetics(k)

    def ops(self):
        return pol.DeviceOps(self.run, self.options, (pol.PARAM_P_M,), lambda u: float(u[self.run.problem.nf - 1]))

    def segment(self, v_from, v_to):
        """One continuation segment in p_M from the handle's converged state at ``v_from``; (reached, Newton iterations)."""
        if v_from == v_to:
            ok, its, rates = self.ops().solve()
            return bool(ok) and not np.any(np.asarray(rates) <= 0.0), int(its)
        try:
            _, _, newton, stop = pol.run_continuation(self.ops(), v_from, v_to, v_to - v_from)
        except RuntimeError:
            return False, 0
        return stop == "v_end", int(sum(newton))

    def measure(self):
        """(values, slopes, state) at the handle's converged state: the currents [A/m2], the surface charge [C/m2] and their
        derivatives for the fit's parameters; None where a rate is <= 0 or a column is not finite."""
        I = self.dev.kinetics_currents()
        if not (np.all(I > 0.0) and np.isfinite(I).all()):
            return None
        D = self.dev.stern_displacement()
        tan = self.dev.electrode_tangent(self.codes)
        if tan["status"].any():
            return None
        values = {"i_CO": float(I[0]), "i_H2": float(I[1]), "surface_charge": self.sigma_unit * D}
        slopes = {"i_CO": tan["dI"][:, 0].copy(), "i_H2": tan["dI"][:, 1].copy(), "surface_charge": self.sigma_unit * tan["dD"]}
        return values, slopes, self.dev.get_state()

    def prepare(self):
        """The curve at the starting parameters; returns its Newton iterations.  RuntimeError where a data potential is not reached."""
        run = self.run
        run.sys.set_time_step(0.0)
        stern, kinetics = self.dev.electrode_options()
        at, newton, points = float(run.stern.p_electrode), 0, []
        for m, v in enumerate(self.V):
            ok, its = self.segment(at, v)
            newton += its
            got = self.measure() if ok else None
            if got is None:
                raise RuntimeError("fit: the steady curve at the starting parameters did not reach the data potential %g; run to the steady stop first "
                                   "(--adaptive_dt --steady_tol)" % v)
            points.append(got)
            at = v
        self.kept = self.assembled(stern, kinetics, points, newton)
        self.last = self.kept
        return newton

    def assembled(self, stern, kinetics, points, newton):
        r, J = [], []
        for m, (values, slopes, _) in enumerate(points):
            rr, JJ = residual_rows(self.data, m, values, slopes)
            r += rr
            J += JJ
        return dict(stern=stern, kinetics=kinetics, points=points, r=np.array(r), J=np.array(J).reshape(len(r), len(self.codes)), newton=newton)

    # -- what LevenbergMarquardt asks ---------------------------------------------------------------------------------------------------
    def trial(self, theta, delta):
        from . import backend
        if self.kept is None:
            self.prepare()
        if not np.any(delta):
            self.last = self.kept
            return self.kept
        k = self.kept
        stern, kinetics, ok = moved_options(k["stern"], k["kinetics"], self.n_species, self.codes, delta)
        self.failed_newton = 0
        if not ok:
            return None
        soft = (backend.ERR_NOT_CONVERGED, backend.ERR_NUMERIC)
        points, newton = [], 0
        try:
            for m, v in enumerate(self.V):
                got = None
                try:
                    self.dev.set_state(k["points"][m][2], k["points"][m][2])
                    if self.predictor:
                        self.set_options(k["stern"], k["kinetics"], v)
                        self.dev.electrode_tangent(self.codes)
                        self.dev.parameter_advance(self.codes, delta, self.run.step_fraction)
                        if m == 0:   # the numbers the library's own exp produced: every other point gets the same ones
                            stern, kinetics = self.dev.electrode_options()
                        self.run.stern, self.run.kinetics = records_of(stern, kinetics, v)
                    else:
                        self.set_options(stern, kinetics, v)
                    st = self.dev.newton_solve(self.options)
                    self.run.sys.record(st)
                    newton += st["iterations"]
                    got = self.measure()
                except backend.GmpnpError as e:
                    if e.code not in soft:
                        raise
                    newton += (e.stats or {}).get("iterations", 0)
                if got is None and m > 0:   # once more, from the neighbour's converged trial state
                    self.retried_points += 1
                    self.dev.set_state(points[m - 1][2], points[m - 1][2])
                    self.set_options(stern, kinetics, self.V[m - 1])
                    reached, its = self.segment(self.V[m - 1], v)
                    newton += its
                    got = self.measure() if reached else None
                if got is None:
                    self.failed_newton = newton
                    return None
                points.append(got)
        finally:
            self.run.stern, self.run.kinetics = records_of(k["stern"], k["kinetics"], self.run.stern.p_electrode)
        self.last = self.assembled(stern, kinetics, points, newton)
        return self.last

    def accept(self):
        self.kept = self.last

    def finish(self, electrode_voltage, inv_dt):
        """The handle and the run at ``electrode_voltage`` with the kept parameters, at the steady state there, ``inv_dt`` put back."""
        k = self.kept
        self.dev.set_state(k["points"][0][2], k["points"][0][2])
        self.set_options(k["stern"], k["kinetics"], self.V[0])
        ok, _ = self.segment(self.V[0], float(electrode_voltage))
        if not ok:
            raise RuntimeError("fit: the steady state at electrode_voltage was not reached with the fitted parameters")
        self.dev.assign_previous()
        self.run.sys.set_time_step(inv_dt)


# ---- fits to transients: the same rule over a marched programme ---------------------------------------------------
TIME_TOL = 1.0e-9                             # a data time coincides with a step end to this relative difference
PROGRAMME_DATA_KEYS = ("time_s",) + DATA_KEYS[1:]


def load_programme_data(path):
    """``load_data`` for transient data: ``time_s`` in the place of ``electrode_voltage`` (what ``programme.npz`` holds is accepted as
    it is; its other keys are not read)."""
    path = str(path)
    if path.lower().endswith(".npz"):
        with np.load(path) as z:
            return {k: np.asarray(z[k], dtype=np.float64).ravel() for k in PROGRAMME_DATA_KEYS if k in z.files}
    table = np.genfromtxt(path, delimiter=",", names=True, dtype=np.float64)
    names = table.dtype.names or ()
    if "time_s" not in names:
        raise ValueError("fit_programme: a CSV needs a header row with time_s")
    return {k: np.atleast_1d(table[k]).astype(np.float64) for k in names if k in PROGRAMME_DATA_KEYS}


def check_programme_data(data, n_params):
    """The refusals of transient data; returns a dict as ``check_data`` does, with ``time_s`` (n,) in the order given."""
    if "time_s" not in data or not any(k in data for k in CURRENT_KEYS):
        raise ValueError("fit_programme: the data hold time_s and i_CO and / or i_H2 (optional: surface_charge, weight_*)")
    t = np.asarray(data["time_s"], dtype=np.float64).ravel()
    out = {"quantities": tuple(k for k in CURRENT_KEYS + ("surface_charge",) if k in data), "time_s": t}
    if t.size < 1 or not np.isfinite(t).all() or len(set(t.tolist())) != t.size:
        raise ValueError("fit_programme: the times must be finite and distinct")
    for k in out["quantities"]:
        v = np.asarray(data[k], dtype=np.float64).ravel()
        w = np.asarray(data.get("weight_" + k, np.ones(t.size)), dtype=np.float64).ravel()
        if w.size == 1:
            w = np.full(t.size, w[0])
        if v.size != t.size or w.size != t.size:
            raise ValueError("fit_programme: %s has %d values and %d weights for %d times" % (k, v.size, w.size, t.size))
        if not (np.isfinite(v).all() and np.isfinite(w).all() and np.all(w >= 0.0)):
            raise ValueError("fit_programme: %s and its weights must be finite, the weights >= 0" % k)
        if k in CURRENT_KEYS and np.any(v <= 0.0):
            raise ValueError("fit_programme: %s must be > 0 (the residual is that of ln I)" % k)
        out[k], out["weight_" + k] = v, w
    if "surface_charge" in out["quantities"] and not np.abs(out["surface_charge"]).max() > 0.0:
        raise ValueError("fit_programme: surface_charge is zero everywhere")
    if t.size * len(out["quantities"]) < int(n_params):
        raise ValueError("fit_programme: %d residuals are fewer than the %d parameters" % (t.size * len(out["quantities"]), n_params))
    return out


def match_times(data_times, step_times):
    """The index of the step that ends at every data time (both in seconds); ValueError names the first data time that coincides with
    no step end to a relative ``TIME_TOL``."""
    steps = np.asarray(step_times, dtype=np.float64)
    idx = []
    for t in np.asarray(data_times, dtype=np.float64):
        j = int(np.argmin(np.abs(steps - t)))
        if not abs(steps[j] - t) <= TIME_TOL * max(abs(t), abs(steps[j])):
            raise ValueError("fit_programme: the data time %.17g s is not the end of a step of the programme (the nearest ends at %.17g s)" % (t, steps[j]))
        idx.append(j)
    return np.array(idx, dtype=np.int64)


class TransientCurve:
    """The evaluator of ``LevenbergMarquardt`` over a marched programme in fixed mode.  ``system`` supplies

        start(delta) -> bool      from the kept start: the parameters moved by ``delta`` (the predictor of the state with them), the
                                  steady state at the start potential re-converged, the tangent taken there; False: it failed
        march() -> None | dict    the programme marched with sensitivities from that start: ``t`` (steps,) [s], the values ``i_CO``,
                                  ``i_H2``, ``surface_charge`` (steps,) and ``slopes`` {quantity: (steps, n_params)}, ``newton``
        keep()                    the last trial's start (parameters and state) becomes the kept one
        newton                    the Newton iterations of the last start() and march(), also of a failed one

    Residuals and rows come from ``residual_rows`` at the steps the data times coincide with (``match_times``).  A trial that is not
    accepted leaves nothing behind: every trial begins at the kept start."""

    def __init__(self, system, data, n_params):
        self.system, self.data, self.n = system, data, int(n_params)
        self.kept, self.last, self.failed_newton, self.index = None, None, 0, None

    def evaluate(self, delta):
        s = self.system
        out = s.march() if s.start(delta) else None
        if out is None:
            self.failed_newton = int(s.newton)
            return None
        if self.index is None:
            self.index = match_times(self.data["time_s"], out["t"])
        r, J, values = [], [], []
        for m, j in enumerate(self.index):
            v = {k: float(out[k][j]) for k in CURRENT_KEYS + ("surface_charge",)}
            if not (v["i_CO"] > 0.0 and v["i_H2"] > 0.0 and all(math.isfinite(x) for x in v.values())):
                self.failed_newton = int(out["newton"])
                return None
            rr, JJ = residual_rows(self.data, m, v, {k: out["slopes"][k][j] for k in v})
            r += rr
            J += JJ
            values.append(v)
        return dict(r=np.array(r), J=np.array(J).reshape(len(r), self.n), newton=int(out["newton"]), values=values)

    def trial(self, theta, delta):
        if self.kept is not None and not np.any(delta):
            self.last = self.kept
            return self.kept
        self.last = self.evaluate(np.asarray(delta, dtype=np.float64))
        return self.last

    def accept(self):
        self.kept = self.last
        self.system.keep()


class DeviceTransient:
    """``TransientCurve``'s system over a driver run (``EDLRun``) at the steady state of its start potential, and its own handle.
    start(): ``set_state`` of the kept start, the kept options, ``electrode_tangent`` and ``parameter_advance(delta)`` at inv_dt = 0
    (the predictor, with the run's ``step_fraction``), a Newton solve (``polarisation.NEWTON``) to the steady state of the moved
    parameters, and the tangent there, which the sensitivities start from.  march(): ``run_programme`` in fixed mode over
    ``DeviceProgrammeOps`` with the sensitivities of the fit's parameters."""

    def __init__(self, run, segs, steps_per_segment, codes, sigma_unit, inv_dt_of_h, time_constant, capacity=4096):
        from . import backend
        self.run, self.dev, self.segs, self.steps, self.codes = run, run.sys.dev, segs, int(steps_per_segment), tuple(int(c) for c in codes)
        self.sigma_unit, self.capacity, self.inv_dt_of_h, self.time_constant = float(sigma_unit), int(capacity), inv_dt_of_h, float(time_constant)
        self.options = backend.newton_options(backend.with_step_fraction(pol.NEWTON, run.step_fraction), dim=1)
        self.V0 = float(run.stern.p_electrode)
        stern, kinetics = self.dev.electrode_options()
        u = self.dev.get_state()
        self.kept = dict(stern=stern, kinetics=kinetics, u=u)
        self.pending, self.newton = None, 0

    def set_options(self, stern, kinetics):
        s, k = records_of(stern, kinetics, self.V0)
        self.run.stern, self.run.kinetics = s, k
        self.run.problem.stern, self.run.problem.kinetics = s, k
        self.dev.set_stern(s)
        self.dev.set_kinetics(k)

    def start(self, delta):
        from . import backend
        k, run = self.kept, self.run
        self.newton, self.pending = 0, None
        stern, kinetics, ok = moved_options(k["stern"], k["kinetics"], run.problem.nf - 1, self.codes, delta)
        if not ok:
            return False
        try:
            run.sys.set_time_step(0.0)
            self.dev.set_state(k["u"], k["u"])
            self.set_options(k["stern"], k["kinetics"])
            if np.any(delta):
                self.dev.electrode_tangent(self.codes)
                self.dev.parameter_advance(self.codes, delta, run.step_fraction)
                stern, kinetics = self.dev.electrode_options()   # the numbers the library's own exp produced
                s, kk = records_of(stern, kinetics, self.V0)
                run.stern, run.kinetics, run.problem.stern, run.problem.kinetics = s, kk, s, kk
            st = self.dev.newton_solve(self.options)
            self.newton += st["iterations"]
            u = self.dev.get_state()
            self.dev.set_state(u, u)
            if self.dev.electrode_tangent(self.codes)["status"].any():
                return False
        except backend.GmpnpError as e:
            if e.code not in (backend.ERR_NOT_CONVERGED, backend.ERR_NUMERIC, backend.ERR_LINEAR):
                raise
            self.newton += (e.stats or {}).get("iterations", 0)
            return False
        self.pending = dict(stern=stern, kinetics=kinetics, u=u)
        return True

    def march(self):
        from . import backend
        from . import programme as prg
        run, tc = self.run, self.time_constant
        ops = prg.DeviceProgrammeOps(run, pol.NEWTON, self.inv_dt_of_h, capacity=self.capacity, sensitivities=self.codes, sensitivity_start="steady")
        budget, run.budget = run.budget, None   # (a trial's steps are no rows of the run's budget log)
        try:
            prg.run_programme(ops, self.segs, steps_per_segment=self.steps)
            srec = ops.sensitivity_records()
            self.dev.sensitivity_close()
            rec = ops.records()
        except (RuntimeError, backend.GmpnpError) as e:
            ops.abort()
            self.newton += ops.newton_iterations
            if isinstance(e, backend.GmpnpError) and e.code == backend.ERR_HIP:
                raise
            return None
        finally:
            run.budget = budget
        self.newton += ops.newton_iterations
        if rec["status"].any() or srec["status"].any():
            return None
        q = self.sigma_unit
        return {"t": rec["t"] * tc, "i_CO": rec["I"][:, 0], "i_H2": rec["I"][:, 1], "surface_charge": q * rec["D"], "newton": self.newton,
                "slopes": {"i_CO": srec["dI"][:, :, 0], "i_H2": srec["dI"][:, :, 1], "surface_charge": q * srec["dD"]}}

    def keep(self):
        self.kept = self.pending

    def finish(self, inv_dt):
        """The handle and the run at the start potential with the kept parameters, at the steady state there, ``inv_dt`` put back."""
        k = self.kept
        self.dev.set_state(k["u"], k["u"])
        self.set_options(k["stern"], k["kinetics"])
        self.run.sys.set_time_step(inv_dt)


def programme_fit_keywords(a):
    """The fit_programme keyword of a parsed command line; empty without --fit_programme_data."""
    if getattr(a, "fit_programme_data", None) is None:
        return {}
    par = dict(data=a.fit_programme_data)
    if a.fit_params is not None:
        par["params"] = tuple(a.fit_params)
    return {"fit_programme": par}


def check_fit_programme(par, kwargs, dt_order=1):
    """The refusals of a driver's ``fit_programme`` keyword, before anything touches the device; returns the checked dict."""
    par = dict(par)
    if set(par) - {"data", "params"} or "data" not in par:
        raise ValueError("fit_programme: the keyword is dict(data=[, params=])")
    if kwargs.get("fit") or kwargs.get("polarisation"):
        raise ValueError("fit_programme: not in one run with fit or polarisation (each leaves the run at a potential of its own)")
    prog = kwargs.get("programme")
    if not prog:
        raise ValueError("fit_programme: the fit to transients needs the programme the data were taken with (programme)")
    if prog.get("steps_per_segment") is None:
        raise ValueError("fit_programme: the programme runs in fixed mode (steps_per_segment)")
    if prog.get("sensitivities"):
        raise ValueError("fit_programme: the fit carries the sensitivities of its own parameters (leave the programme's sensitivities out)")
    if prog.get("periodic") is not None and prog.get("periodic") is not False:
        raise ValueError("fit_programme: not with a periodic programme (the data are the transient of a march, not the limit cycle)")
    if kwargs.get("kinetics") is None:
        raise ValueError("fit_programme: the fit needs the surface kinetics (kinetics='tafel')")
    par["params"] = tuple(par.get("params") or DEFAULT_PARAMS)
    try:
        param_codes(par["params"])
    except ValueError as e:
        raise ValueError("fit_programme: %s" % e) from None
    return par


# ---- units and tables ------------------------------------------------------------------------------------------------------------------
def physical_values(codes, theta, L_n):
    """i0 [A/m2], alpha and stern_length [m] from ln k_r, alpha_r and ln lam."""
    return np.array([math.exp(t) * (L_n if pol.param_kind(c) == 3 else 1.0) if is_log(c) else t for c, t in zip(codes, theta)], dtype=np.float64)


def fit_arrays(names, codes, data, theta0, res, model_values, L_n, abscissa="electrode_voltage"):
    """The arrays of ``fit.npz`` (``abscissa`` = "time_s": of ``fit_programme.npz``, the same tables over the data times)."""
    h = res["history"]
    out = {"names": np.array(names), "codes": np.asarray(codes, dtype=np.int32),
           "initial_values": physical_values(codes, theta0, L_n), "fitted_values": physical_values(codes, res["theta"], L_n),
           "initial_theta": np.asarray(theta0, dtype=np.float64), "fitted_theta": res["theta"],
           "standard_errors": res["standard_errors"], "covariance": res["covariance"], "correlation": res["correlation"],
           "singular_values": res["singular_values"], "residuals": res["residuals"], "quantities": np.array(data["quantities"]),
           "history_cost": np.array([x["cost"] for x in h]), "history_lambda": np.array([x["lam"] for x in h]),
           "history_accepted": np.array([x["accepted"] for x in h]), "history_newton_iterations": np.array([x["newton"] for x in h], dtype=np.int64),
           "history_step": np.array([x["step"] for x in h]), abscissa: data[abscissa]}
    for k in data["quantities"]:
        out["data_" + k], out["weight_" + k], out["model_" + k] = data[k], data["weight_" + k], np.array([v[k] for v in model_values])
    return out


def fit_metadata(names, arrays, res):
    return {"fit_parameters": list(names), "fit_values": [float(v) for v in arrays["fitted_values"]],
            "fit_standard_errors": [float(v) for v in res["standard_errors"]], "fit_stop_reason": res["stop_reason"], "fit_trials": int(res["trials"]),
            "fit_rejected_trials": int(res["rejected_trials"]), "fit_newton_iterations": int(res["newton_iterations"]),
            "fit_final_cost": float(res["cost"]), "fit_condition_number": float(res["condition_number"])}


# ---- keywords of the drivers ---------------------------------------------------------------------------------------------------------
def add_fit_arguments(p):
    p.add_argument("--fit_data", required=False, default=None, type=str,
                   help="(addition) fit the electrode kinetics to the polarisation data of this .npz / .csv (electrode_voltage, i_CO, i_H2[, surface_charge]): fit.npz")
    p.add_argument("--fit_programme_data", required=False, default=None, type=str, metavar="FILE",
                   help="(addition) fit the electrode parameters (--fit_params) to the transient data of this .npz / .csv (time_s, i_CO, i_H2[, surface_charge]; "
                        "what programme.npz holds) over --programme in fixed mode (--programme_steps_per_segment): fit_programme.npz")
    p.add_argument("--fit_params", required=False, default=None, nargs="+", type=str, help="(addition) the fitted parameters out of %s (default: %s)"
                   % (" ".join(PARAMETERS), " ".join(DEFAULT_PARAMS)))


def fit_keywords(a):
    """The fit keyword of a parsed command line (``add_fit_arguments``); empty without --fit_data."""
    if a.fit_data is None:
        if a.fit_params is not None and getattr(a, "fit_programme_data", None) is None:
            raise ValueError("fit: --fit_params needs --fit_data")
        return {}
    par = dict(data=a.fit_data)
    if a.fit_params is not None:
        par["params"] = tuple(a.fit_params)
    return {"fit": par}


def refuse_fit(kwargs, what):
    """ValueError where ``kwargs`` asks for a fit (``fit``) in a driver that has none."""
    if kwargs.get("fit"):
        raise ValueError("fit: the fit of the electrode kinetics is not available in %s" % what)


def check_fit(par, kwargs, dt_order=1):
    """The refusals of a driver's ``fit`` keyword, before anything touches the device; returns the checked dict (``params``: names)."""
    par = dict(par)
    if set(par) - {"data", "params", "predictor"} or "data" not in par:
        raise ValueError("fit: the keyword is dict(data=[, params=])")
    try:   # the fit walks steady curves: whatever refuses a polarisation curve of this run refuses the fit (any valid grid will do)
        v = kwargs.get("electrode_voltage")
        pol.check_polarisation(dict(v_end=0.0, v_step=1.0), dict(kwargs, electrode_voltage=None if v is None else -1.0), dt_order)
    except ValueError as e:
        raise ValueError("fit: not available where the steady polarisation curve is not (%s)" % e) from None
    if kwargs.get("kinetics") is None:
        raise ValueError("fit: the fit needs the surface kinetics (kinetics='tafel')")
    par["params"] = tuple(par.get("params") or DEFAULT_PARAMS)
    param_codes(par["params"])
    return par
