"""Steady-state polarisation curves by continuation in the electrode potential (``--polarisation`` of the 1D MPNP
driver, ``gmpnp_electrode_tangent`` / ``gmpnp_electrode_advance``): the Python statement of the tangent's rule (parameter codes, the
explicit derivatives, the node terms of the functionals), the continuation rule, and the physical curve built from the library's
scaled numbers.

With the electrode potential p_M and the other electrode parameters theta as parameters of the steady state F(u; theta) = 0, the tangent
z = du/dtheta solves J z = -dF/dtheta, and along a curve

    u(p_M + dp) = u + dp z + O(dp^2)          (the predictor; a few Newton iterations at inv_dt = 0 follow)
    dD   = dD/dtheta + (dD/du).z              D the integrated Stern term (``stern_displacement``): the differential capacitance
    dI_r = dI_r/dtheta + (dI_r/du).z          I_r the integrated rates (``kinetics_currents``): the Tafel slopes

come out of the same solve at every point.  No reference counterpart.
"""
from __future__ import annotations

import math

import numpy as np

MAX_COLUMNS = 10                              # GMPNP_TANGENT_MAX_COLUMNS
MAX_SURFACE_REACTIONS = 4                     # GMPNP_MAX_SURFACE_REACTIONS
PARAM_P_M, PARAM_LN_K, PARAM_ALPHA, PARAM_LN_LAM = 0, 16, 32, 48   # ln k_r = 16 + r, alpha_r = 32 + r
STATUS_NONFINITE = 1                          # bit of gmpnp_tangent_t.status
DP_MIN_DIVISOR = 1024.0                       # a step below |v_step| / 1024 ends the curve
POLARISATION_KEYWORDS = ("polarisation",)


# ---- the rule (gmpnp_host_rules.h), operation for operation -------------------------------------------------------------------------
def param_kind(param):
    """0 p_M, 1 ln k_r, 2 alpha_r, 3 ln lam, -1 unknown (``tangent_param_kind``)."""
    param = int(param)
    if param == 0:
        return 0
    if 16 <= param < 16 + MAX_SURFACE_REACTIONS:
        return 1
    if 32 <= param < 32 + MAX_SURFACE_REACTIONS:
        return 2
    if param == 48:
        return 3
    return -1


def param_reaction(param):
    k = param_kind(param)
    return int(param) - 16 if k == 1 else int(param) - 32 if k == 2 else -1


def param_valid(param, n_reactions):
    """Valid on a handle with ``n_reactions`` reactions (0: the kinetics are off) (``tangent_param_valid``)."""
    k = param_kind(param)
    if k < 0:
        return False
    return True if k in (0, 3) else param_reaction(param) < int(n_reactions)


def count_valid(n):
    return 1 <= int(n) <= MAX_COLUMNS


def param_name(param):
    k, r = param_kind(param), param_reaction(param)
    return {0: "p_M", 1: "ln_k_%d" % r, 2: "alpha_%d" % r, 3: "ln_lam"}.get(k, "unknown")


def rate_explicit(param, r, rate, d_p, eta):
    """d rate_r / d theta at fixed u, eta = p_M - p - p_eq_r (``tangent_rate_explicit``)."""
    k = param_kind(param)
    rate, d_p, eta = np.float64(rate), np.float64(d_p), np.float64(eta)
    if k == 0:
        return float(-d_p)
    if k == 1:
        return float(rate) if param_reaction(param) == r else 0.0
    if k == 2:
        return float(-(rate * eta)) if param_reaction(param) == r else 0.0
    return 0.0


def stern_explicit(param, slope, term):
    """d (Stern term) / d theta at fixed u, slope = d term / d p_M (``tangent_stern_explicit``)."""
    k = param_kind(param)
    return float(slope) if k == 0 else float(-np.float64(term)) if k == 3 else 0.0


def current_term(w, d_u, d_p, z_u, z_p, explicit_part):
    """Reaction r's share of dI_r at a kinetic node of weight w (``tangent_current_term``)."""
    w, d_u, d_p, z_u, z_p, e = (np.float64(v) for v in (w, d_u, d_p, z_u, z_p, explicit_part))
    return float(w * ((d_u * z_u + d_p * z_p) + e))


class Continuation:
    """The continuation rule of a curve (``Continuation`` of gmpnp_host_rules.h): targets are the grid v_start + k v_step up to v_end,
    which is landed on exactly; an attempt goes from the last converged point ``at`` towards the next target with step ``dp``; a
    failed attempt halves the step, a success tries the whole remainder to the target again; a step below |v_step| / 1024 ends the
    curve (``stop`` = 1, "dp_min"; 2 = the end was reached)."""

    STOP_REASONS = {0: "running", 1: "dp_min", 2: "v_end"}

    def __init__(self, v_start, v_end, v_step):
        if not continuation_valid(v_start, v_end, v_step):
            raise ValueError("polarisation: finite v_start, v_end and v_step, v_step != 0 and pointing from v_start to v_end")
        self.v_start, self.v_end, self.v_step = float(v_start), float(v_end), float(v_step)
        self.at, self.k, self.dp, self.stop = self.v_start, 0, 0.0, 0
        if self.v_start == self.v_end:
            self.stop = 2
        else:
            self.dp = self.target() - self.at

    def target(self):
        t = self.v_start + (self.k + 1) * self.v_step
        return self.v_end if (t >= self.v_end if self.v_step > 0.0 else t <= self.v_end) else t

    def attempt_potential(self):
        """The potential of the next attempt: the target itself where the attempt lands on it."""
        nxt = self.at + self.dp
        t = self.target()
        return t if (nxt >= t if self.v_step > 0.0 else nxt <= t) else nxt

    def advance(self, success):
        """After an attempt of step ``dp``: True where a grid point was reached (``k`` counts it)."""
        target = self.target()
        dp_min = abs(self.v_step) / DP_MIN_DIVISOR
        if not success:
            self.dp = self.dp / 2.0
            if abs(self.dp) < dp_min:
                self.stop = 1
            return False
        nxt = self.at + self.dp
        if (nxt >= target) if self.v_step > 0.0 else (nxt <= target):
            self.at, self.k = target, self.k + 1
            if target == self.v_end:
                self.stop, self.dp = 2, 0.0
            else:
                self.dp = self.target() - self.at
            return True
        self.at = nxt
        self.dp = target - self.at
        return False

    @property
    def stop_reason(self):
        return self.STOP_REASONS[self.stop]


def continuation_valid(v_start, v_end, v_step):
    vals = (float(v_start), float(v_end), float(v_step))
    return all(math.isfinite(v) for v in vals) and vals[2] != 0.0 and (vals[1] - vals[0]) * vals[2] >= 0.0


def run_continuation(system, v_start, v_end, v_step, predictor=True):
    """Walks a curve by the rule above over ``system``, which supplies the operations of a handle:

        solve() -> (converged, iterations, rates or None)    Newton at the present potential; a GMPNP_ERR_NUMERIC end is ``converged``
                                                             False
        point(p) -> record                                   the converged point's record (tangent included), kept by the caller
        predict(dp)                                          p_M += dp, u += alpha dp z (``predictor`` off: p_M += dp alone)
        set_potential(p)                                     p_M = p exactly
        keep() / back(p)                                     the converged state is kept / the handle returns to it at potential p

    An attempt fails when the solve does not converge or any integrated rate is negative (the unphysical branch on which the
    reactant is consumed below zero).  Returns (records, attempts per grid point, Newton iterations per grid point, stop_reason);
    the first record is the start."""
    c = Continuation(v_start, v_end, v_step)
    ok, its, rates = system.solve()
    if not ok or (rates is not None and np.any(np.asarray(rates) < 0.0)):
        raise RuntimeError("polarisation: the Newton solve at the first potential did not converge; run to the steady stop first "
                           "(--adaptive_dt --steady_tol)")
    system.keep()
    records, substeps, newton = [system.point(c.at)], [0], [int(its)]
    n_sub, n_its = 0, 0
    while c.stop == 0:
        p_try = c.attempt_potential()
        system.predict(p_try - c.at, predictor)
        system.set_potential(p_try)
        ok, its, rates = system.solve()
        good = bool(ok) and not (rates is not None and np.any(np.asarray(rates) < 0.0))
        n_sub, n_its = n_sub + 1, n_its + int(its)
        reached = c.advance(good)
        if not good:
            system.back(c.at)
            continue
        system.keep()
        rec = system.point(c.at)
        if reached:
            records.append(rec); substeps.append(n_sub); newton.append(n_its)
            n_sub, n_its = 0, 0
    return records, substeps, newton, c.stop_reason


# ---- the operations of a device handle ------------------------------------------------------------------------------------------------
# the Newton solves of a curve (inv_dt = 0): every point is a steady state in its own right, so the residual goes to its rounding
# floor; a solve that needs more than 25 iterations counts as failed and the step is halved
NEWTON = {"newton_solver": {"maximum_iterations": 25, "relative_tolerance": 1.0e-13, "absolute_tolerance": 1.0e-7}}


class DeviceOps:
    """What ``run_continuation`` asks of a system, over a driver run (``EDLRun`` / ``PoreRun``: its ``sys``, ``stern``, ``kinetics``
    and ``step_fraction``) and its device handle.  ``boundary_potential(u)``: the potential the records report beside p_M.
    ``after_solve()`` (3D: the Sechenov update of the CO2 Dirichlet value) returns True where the point has to be solved again with
    new Dirichlet values; at most ``max_rounds`` solves per attempt, their number is recorded.  A predictor that ends in a numeric
    error (a direction that is not finite) makes the attempt a failed one, as a Newton solve with that end does."""

    def __init__(self, run, options, params, boundary_potential, after_solve=None, max_rounds=10):
        self.run, self.dev, self.options, self.params = run, run.sys.dev, options, tuple(params)
        self.boundary_potential, self.after_solve, self.max_rounds = boundary_potential, after_solve, int(max_rounds)
        self.fresh, self.failed_predictor, self.rounds = False, False, 0
        self.p_dev = float(run.stern.p_electrode)

    def solve(self):
        from . import backend
        self.fresh = False
        if self.failed_predictor:
            self.failed_predictor = False
            return False, 0, None
        its, self.rounds = 0, 0
        for _ in range(self.max_rounds):
            try:
                st = self.dev.newton_solve(self.options)
            except backend.GmpnpError as e:
                if e.code not in (backend.ERR_NOT_CONVERGED, backend.ERR_NUMERIC):
                    raise
                return False, its + (e.stats or {}).get("iterations", 0), None
            self.run.sys.record(st)
            its, self.rounds = its + st["iterations"], self.rounds + 1
            if self.after_solve is None or not self.after_solve():
                break
        return True, its, (self.dev.kinetics_currents() if self.run.kinetics is not None else None)

    def point(self, p):
        tan = self.dev.electrode_tangent(self.params)
        self.fresh = True
        return {"p_M": p, "potential_OHP": self.boundary_potential(self.dev.get_state()), "tangent": tan, "displacement": self.dev.stern_displacement(),
                "currents": self.dev.kinetics_currents() if self.run.kinetics is not None else None, "sechenov_rounds": self.rounds if self.after_solve else 0}

    def predict(self, dp, predictor):
        from . import backend
        if predictor:
            try:
                if not self.fresh:
                    self.dev.electrode_tangent([PARAM_P_M])
                self.dev.electrode_advance(dp, self.run.step_fraction)
                self.p_dev = self.p_dev + dp   # (the library's own addition)
            except backend.GmpnpError as e:
                if e.code != backend.ERR_NUMERIC:
                    raise
                self.failed_predictor = True   # nothing was applied: the attempt fails and the rule returns to the last point
        self.fresh = False

    def set_potential(self, p):
        import dataclasses
        run = self.run
        run.stern = dataclasses.replace(run.stern, p_electrode=float(p))
        if run.kinetics is not None:
            run.kinetics = dataclasses.replace(run.kinetics, p_electrode=float(p))
        if self.p_dev != p:   # (the predictor's sum missed the grid value by a rounding, or there was no predictor)
            self.dev.set_stern(run.stern)
            if run.kinetics is not None:
                self.dev.set_kinetics(run.kinetics)
            self.p_dev = float(p)

    def keep(self):
        self.dev.assign_previous()

    def back(self, p):
        self.dev.time_reject()
        self.set_potential(p)
        self.fresh = False


# ---- units ---------------------------------------------------------------------------------------------------------------------------
def tafel_slope(thermal_voltage, I, dI):
    """[V/decade] = ln 10 V_T / (dI_r / I_r) of one reaction (NaN where the current or its slope is zero)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return math.log(10.0) * thermal_voltage / (np.asarray(dI, dtype=np.float64) / np.asarray(I, dtype=np.float64))


def curve_arrays(ep, eps_0, area, records, params, substeps, newton):
    """The arrays of ``polarisation.npz`` from the per-point records of ``run_continuation`` (``record``: p_M, potential_OHP [thermal
    voltages], currents (integrated rates), displacement, tangent (``DeviceSolver.electrode_tangent``), sechenov_rounds)."""
    from .kinetics import current_summary
    n = len(records)
    V_T = ep.thermal_voltage
    p = np.array([r["p_M"] for r in records])
    cur = [current_summary(r["currents"], area) if r["currents"] is not None and len(r["currents"]) >= 2 else
           {"i_CO": float("nan"), "i_H2": float("nan"), "FE_H2": float("nan")} for r in records]
    k0 = list(params).index(PARAM_P_M)
    nr = max((len(r["currents"]) for r in records if r["currents"] is not None), default=0)
    I = np.array([np.asarray(r["currents"], dtype=np.float64)[:nr] if nr else np.zeros(0) for r in records]).reshape(n, nr)
    dI0 = np.array([r["tangent"]["dI"][k0][:nr] for r in records]).reshape(n, nr)
    dD0 = np.array([r["tangent"]["dD"][k0] for r in records])
    table = np.array([np.concatenate([r["tangent"]["dD"][:, None], r["tangent"]["dI"][:, :nr], r["tangent"]["dp_boundary"][:, None]], axis=1)
                      for r in records])
    return {"electrode_voltage": p, "electrode_voltage_V": p * V_T,
            "potential_OHP": np.array([r["potential_OHP"] for r in records]) * V_T,
            "i_CO": np.array([c["i_CO"] for c in cur]), "i_H2": np.array([c["i_H2"] for c in cur]), "FE_H2": np.array([c["FE_H2"] for c in cur]),
            "surface_charge": eps_0 * V_T / ep.L_n * np.array([r["displacement"] for r in records]) / area,
            "capacitance": eps_0 / ep.L_n * dD0 / area,
            "dI_dV": dI0 / V_T / area,
            "tafel_slope": tafel_slope(V_T, I, dI0),
            "sensitivity": table, "sensitivity_params": np.asarray(params, dtype=np.int32),
            "newton_iterations": np.asarray(newton, dtype=np.int64), "substeps": np.asarray(substeps, dtype=np.int64),
            "tangent_residual": np.array([float(np.max(r["tangent"]["residual"])) for r in records]),
            "sechenov_rounds": np.array([int(r.get("sechenov_rounds", 0)) for r in records], dtype=np.int64)}


# ---- keywords of the drivers ---------------------------------------------------------------------------------------------------------
def add_polarisation_arguments(p):
    p.add_argument("--polarisation", action="store_true",
                   help="(addition) steady-state polarisation curve from the last state and --electrode_voltage to --v_end (polarisation.npz)")
    p.add_argument("--v_end", required=False, default=None, type=float, help="(addition) last electrode potential of --polarisation [thermal voltages]")
    p.add_argument("--v_step", required=False, default=None, type=float, help="(addition) grid step of --polarisation [thermal voltages], signed")


def polarisation_keywords(a):
    """The polarisation keyword of a parsed command line (``add_polarisation_arguments``); empty without --polarisation."""
    if not a.polarisation:
        return {}
    if a.v_end is None or a.v_step is None:
        raise ValueError("polarisation: --polarisation needs --v_end and --v_step")
    return {"polarisation": dict(v_end=a.v_end, v_step=a.v_step)}


def refuse_polarisation(kwargs, what):
    """ValueError where ``kwargs`` asks for a polarisation curve (``polarisation``) in a driver that has none."""
    if kwargs.get("polarisation"):
        raise ValueError("polarisation: the polarisation curve is not available in %s" % what)


def check_polarisation(par, kwargs, dt_order=1):
    """The refusals of a driver's ``polarisation`` keyword, before anything touches the device; returns the checked dict."""
    par = dict(par)
    if set(par) - {"v_end", "v_step", "params"} or "v_end" not in par or "v_step" not in par:
        raise ValueError("polarisation: the keyword is dict(v_end=, v_step=[, params=])")
    if kwargs.get("electrode_voltage") is None:
        raise ValueError("polarisation: the curve needs an electrode potential (electrode_voltage)")
    if kwargs.get("target_current") is not None:
        raise ValueError("polarisation: the curve is not available with target_current (the galvanostat)")
    if kwargs.get("stabilization", "N") == "Y":
        raise ValueError("polarisation: the curve is not available with stabilization Y")
    if kwargs.get("H_OHP") is not None:
        raise ValueError("polarisation: the curve is not available with the H_OHP flux controller")
    if int(dt_order) == 2:
        raise ValueError("polarisation: the curve is not available with dt_order 2")
    if not continuation_valid(float(kwargs["electrode_voltage"]), par["v_end"], par["v_step"]):
        raise ValueError("polarisation: finite v_end and v_step, v_step != 0 and pointing from electrode_voltage to v_end")
    params = tuple(int(q) for q in par.get("params", (PARAM_P_M,)))
    nr = 2 if kwargs.get("kinetics") is not None else 0
    if not count_valid(len(params)) or len(set(params)) != len(params) or PARAM_P_M not in params or not all(param_valid(q, nr) for q in params):
        raise ValueError("polarisation: params are 1 ... %d distinct parameter codes valid for the run, p_M (0) among them" % MAX_COLUMNS)
    par["params"] = params
    return par
