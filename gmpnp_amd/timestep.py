"""Adaptive time stepping with error control and a steady-state stop (not a reference feature: the reference marches with the
step of its YAML file).  Backward Euler, or with ``order`` = 2 variable-step BDF2 after a backward Euler start-up (DESIGN.md section
5g; kernels: csrc/gmpnp_time_order.h); the step is chosen from the device's estimate of its local error (include/gmpnp.h,
gmpnp_time_error; kernels: csrc/gmpnp_time_step.h).  ``next_time_step`` is the Python statement of the rule that
csrc/gmpnp_host_rules.h states in C++ (``next_time_step`` there; tests/test_time_step_reference.py compiles that one with the host
compiler and holds both against a NumPy restatement of its own).  ``AdaptiveStepper`` owns the loop body of one attempted step,
``EnsembleStepper`` the round of a device ensemble whose members each follow their own clock."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from . import backend

REASONS = ("accepted", "error_too_large", "newton_failed", "nonfinite")


def _c_cbrt():
    """The C library's cbrt, the function std::cbrt of csrc/gmpnp_host_rules.h calls (``math.cbrt`` where Python has it; NumPy's
    cube root is another implementation and differs from it in the last bit, e.g. at 0.125)."""
    if hasattr(math, "cbrt"):
        return math.cbrt
    import ctypes
    import ctypes.util
    fn = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6").cbrt
    fn.restype, fn.argtypes = ctypes.c_double, [ctypes.c_double]
    return fn


cbrt = _c_cbrt()


@dataclass
class TimeStepPolicy:
    safety: float = 0.9
    min_factor: float = 0.2
    max_factor: float = 4.0
    fail_factor: float = 0.25
    h_min: float = 0.0
    h_max: float = math.inf
    t_end: float = math.inf
    steady_tol: float = 0.0    # 0 = no steady stop
    steady_steps: int = 2      # consecutive accepted steps with rate < steady_tol


@dataclass
class TimeStepDecision:
    accept: bool
    reason: int          # index into REASONS
    t_next: float        # t + h when accepted (t_end exactly when the step landed on it), else t
    h_next: float        # the step to try next
    stop_end: bool
    stop_steady: bool
    give_up: bool        # h_next < h_min: the run ends
    steady_run: int      # the steady counter after this attempt (handed back in at the next one)


def next_time_step(p: TimeStepPolicy, t, h, err, has_history, newton_failed, rate, steady_run, order=1) -> TimeStepDecision:
    """The accept / reject rule of one attempted step h at time t.  The exponent of the step factor is 1/2 because backward
    Euler's LOCAL error is O(h^2): err(h') = err(h) (h'/h)^2 = 1 at h' = h err^(-1/2), times the safety factor.  ``order`` = 2
    (a BDF2 step, local error O(h^3)): the factor is safety err^(-1/3) and an accepted step grows by min(max_factor, 2) at most
    (variable-step BDF2 is zero-stable only for h / h_prev < 1 + sqrt(2)); everything else is the same rule."""
    nan_err = err != err

    def factor(hi):
        if not has_history:
            return 1.0
        if err > 0.0:
            return min(max(p.safety / (cbrt(err) if order == 2 else math.sqrt(err)), p.min_factor), hi)
        return hi
    grow = min(p.max_factor, 2.0) if order == 2 else p.max_factor

    stop_steady = False
    if newton_failed or nan_err:
        accept, reason, t_next, h_next, run = False, (2 if newton_failed else 3), t, p.fail_factor * h, steady_run
    elif has_history and err > 1.0:
        accept, reason, t_next, h_next, run = False, 1, t, h * factor(1.0), steady_run
    else:
        accept, reason, t_next, h_next = True, 0, t + h, h * factor(grow)
        run = steady_run + 1 if (p.steady_tol > 0.0 and rate < p.steady_tol) else 0
        stop_steady = p.steady_tol > 0.0 and run >= p.steady_steps
    if h_next > p.h_max:
        h_next = p.h_max
    stop_end = lands = False     # lands: the next step is the last one, cut (or stretched) to end on t_end: h_min does not judge it
    if math.isfinite(p.t_end):   # land on t_end exactly: shorten the step, or stretch it by at most 1 % instead of leaving a sliver
        left = p.t_end - t_next
        if accept and not left > 1e-12 * abs(p.t_end):
            t_next, stop_end = p.t_end, True
        elif left <= 1.01 * h_next:
            lands, h_next = h_next >= p.h_min, left
    give_up = (not stop_end) and (not stop_steady) and (not lands) and h_next < p.h_min
    return TimeStepDecision(accept, reason, t_next, h_next, stop_end, stop_steady, give_up, run)


# ---- the coefficients of variable-step BDF2 (csrc/gmpnp_host_rules.h states them in C++, statement for statement) ---------------
def bdf2_alpha0(omega):
    return (1.0 + 2.0 * omega) / (1.0 + omega)


def bdf2_history_weights(omega):
    """(a, b) of u* = a u_n - b u_nm1."""
    q = 1.0 + 2.0 * omega
    return (1.0 + omega) * (1.0 + omega) / q, omega * omega / q


def bdf2_predictor_weights(h, h1, h2):
    """Lagrange weights (u_n, u_nm1, u_nm2) at t + h of the quadratic through (t - h1 - h2, u_nm2), (t - h1, u_nm1), (t, u_n)."""
    wn = (h + h1 + h2) * (h + h1) / ((h1 + h2) * h1)
    wm1 = -((h + h1 + h2) * h) / (h1 * h2)
    wm2 = (h + h1) * h / (h2 * (h1 + h2))
    return wn, wm1, wm2


def bdf2_error_share(h, h1, h2):
    """kappa: BDF2's local error as a share of u - p."""
    c = h / bdf2_alpha0(h / h1)
    return c / (h + h1 + h2 + c)


class AdaptiveStepper:
    """The loop body of an adaptive run on a ``GMPNPSystem``: set the step, solve, estimate, decide, accept or reject.
    ``tol`` = (rtol, atol) with atol a scalar or one value per field; ``inv_dt_of_h(h)`` = the model's inv_dt for a step h in the
    driver's time units (3D: 1/h, 1D: 1/(h L_D), L_D the scaled Debye length).  ``log`` holds one row per attempt.
    ``order`` = 2: variable-step BDF2.  The order of each attempt follows the handle's history: backward Euler without an estimate,
    backward Euler with its estimate, then BDF2 for as long as the handle holds three accepted states (``order`` in the row)."""

    COLUMNS = ("t", "h", "accepted", "reason", "err", "rate", "newton", "krylov", "worst_dof", "steric_excursion")

    def __init__(self, system, policy: TimeStepPolicy, tol, inv_dt_of_h, h_init, t0=0.0, solver_parameters=None, order=1):
        from .solver import PartitionedSystem
        if isinstance(system, PartitionedSystem):
            raise ValueError("adaptive time stepping is not available on a partitioned system")
        if order not in (1, 2):
            raise ValueError("order is 1 (backward Euler) or 2 (variable-step BDF2)")
        self.order = int(order)
        self.h_prev2 = 0.0
        self.columns = self.COLUMNS + (("order",) if self.order == 2 else ())
        if self.order == 2:
            system.set_time_order(2)
        self.sys, self.policy, self.inv_dt_of_h = system, policy, inv_dt_of_h
        self.rtol, self.atol = float(tol[0]), tol[1]
        self.solver_parameters = solver_parameters
        self.t, self.h, self.h_prev = float(t0), float(h_init), 0.0
        self.steady_run = 0
        self.stop_reason = None   # "t_end", "steady", "h_min"; the drivers add "max_steps"
        self.log = []
        self.last_decision = None

    @property
    def accepted(self):
        return sum(1 for r in self.log if r["accepted"])

    @property
    def rejected(self):
        return sum(1 for r in self.log if not r["accepted"])

    @property
    def newton_failures(self):
        return sum(1 for r in self.log if r["reason"] == 2)

    def start(self):
        """(t, h) of the step to attempt next; RuntimeError once the run has ended."""
        if self.stop_reason is not None:
            raise RuntimeError("the adaptive run has ended (%s)" % self.stop_reason)
        return self.t, self.h

    def decide(self, t, h, st, failed, est, order=1):
        """The decision and the log row of the attempt (t, h): ``st`` = the Newton statistics (None: none came back), ``failed`` =
        Newton gave up (``RETRY_CODES``), ``est`` = the estimator's report of a converged solve, else None."""
        err = est["err"] if est else 0.0
        rate = est["rate"] if est else math.inf
        d = next_time_step(self.policy, t, h, err, bool(est and est["has_history"]), failed, rate, self.steady_run, order)
        row = {"t": t, "h": h, "accepted": bool(d.accept), "reason": d.reason, "err": err if est else math.nan,
               "rate": rate if est else math.nan, "newton": st["iterations"] if st else -1,
               "krylov": st["krylov_iterations"] if st else -1, "worst_dof": est["worst_dof"] if est else -1,
               "steric_excursion": st["steric_excursion"] if st else -1}
        if self.order == 2:
            row["order"] = order
        return d, row

    def finish(self, d, row):
        """The clock, the controller's memory, the log and the stop reason after the attempt's accept / reject went to the device."""
        if d.accept:
            self.h_prev2, self.h_prev = self.h_prev, row["h"]
        self.t, self.h, self.steady_run = d.t_next, d.h_next, d.steady_run
        self.log.append(row)
        self.last_decision = d
        if d.stop_end:
            self.stop_reason = "t_end"
        elif d.stop_steady:
            self.stop_reason = "steady"
        elif d.give_up:
            self.stop_reason = "h_min"

    def attempt(self, before_solve=None, before_accept=None):
        """One attempted step.  ``before_solve(t, h)``: the driver's glue in front of the Newton solve (its clock is the
        stepper's); ``before_accept(stats)``: the driver's glue of an accepted step, called while u_n is still the previous state
        (budgets, history row, new Dirichlet values) — a rejected step calls neither it nor anything else of the driver.
        Returns the log row.  (``EnsembleStepper.round`` runs the same phases for many members at once.)"""
        t, h = self.start()
        order = 2 if (self.order == 2 and self.sys.time_history_levels() >= 2) else 1
        if order == 2:
            self.sys.set_time_step_bdf2(self.inv_dt_of_h(h), h / self.h_prev)
        else:
            self.sys.set_time_step(self.inv_dt_of_h(h))
        if before_solve is not None:
            before_solve(t, h)
        st, failed = None, False
        try:
            st = self.sys.solve(self.solver_parameters)
        except backend.GmpnpError as e:
            if e.code not in (backend.ERR_NUMERIC, backend.ERR_LINEAR):   # (a linear solve that breaks down on an iterate outside
                raise                                                     # the admissible set is the same failure, found earlier)
            st, failed = e.stats, True
        except RuntimeError as e:   # DOLFIN's "Newton solver did not converge"
            cause = e.__cause__
            if not (isinstance(cause, backend.GmpnpError) and cause.code == backend.ERR_NOT_CONVERGED):
                raise
            st, failed = cause.stats, True
        if failed and st is not None:   # solve() accounts converged solves only
            self.sys.record(st)
        est = None
        if not failed and order == 2:
            est = self.sys.time_error_bdf2(h, self.h_prev, self.h_prev2, self.rtol, self.atol)
        elif not failed:
            est = self.sys.time_error(h, self.h_prev, self.rtol, self.atol)
        d, row = self.decide(t, h, st, failed, est, order)
        if d.accept:
            if before_accept is not None:
                before_accept(st)
            self.sys.time_accept()
        else:
            self.sys.time_reject()
        self.finish(d, row)
        return row

    def log_arrays(self):
        """The log as arrays by column (what ``timestep_log.npz`` holds)."""
        out = {}
        for c in self.columns:
            kind = np.float64 if c in ("t", "h", "err", "rate") else (np.bool_ if c == "accepted" else np.int64)
            out[c] = np.array([r[c] for r in self.log], dtype=kind)
        return out

    def summary(self):
        """The keys an adaptive run adds to metadata.json."""
        out = {"adaptive_dt": True, "dt_rtol": self.rtol, "dt_atol": np.asarray(self.atol, dtype=float).tolist(),
               "steps_accepted": self.accepted, "steps_rejected": self.rejected, "newton_failures": self.newton_failures,
               "t_reached": self.t, "stop_reason": self.stop_reason}
        if self.order == 2:
            out["dt_order"] = 2
        return out


# a Newton solve that ends with one of these is a failed ATTEMPT (rejected and tried again with a smaller step), as in ``attempt``
RETRY_CODES = (backend.ERR_NOT_CONVERGED, backend.ERR_NUMERIC, backend.ERR_LINEAR)


class EnsembleStepper:
    """Adaptive runs of the members of a device ensemble, every member on its own clock.  Holds the members' ``AdaptiveStepper``s
    and owns one *round*: one attempted step of every member that has not stopped, with ONE ensemble Newton solve, ONE batched
    estimate and ONE batched accept / reject (``backend.DeviceEnsemble``).  The decision and the log row are the members' own
    (``AdaptiveStepper.decide`` / ``finish``).

    ``ensemble_of(live)``: the ensemble of the members ``live`` (indices, ascending), rebuilt by the caller when the list changes;
    ``options``: what its ``newton_solve`` takes; ``max_steps``: None, or per member None or the largest number of attempted steps.
    Hooks, all optional, ``k`` the member: ``before_solve(k, t, h)`` and ``before_accept(k, stats, u_row)`` as in
    ``AdaptiveStepper.attempt`` (``u_row`` = the member's row of the round's one ``get_state``), ``after_attempt(k, row)``,
    ``on_error(k, code, message)`` for a member whose solve ends with another status than ``RETRY_CODES``: it stops
    (``errors[k]`` keeps the message, ``status[k]`` the code) and its neighbours go on."""

    def __init__(self, steppers, ensemble_of, options, max_steps=None, before_solve=None, before_accept=None, after_attempt=None,
                 on_error=None):
        self.steppers = list(steppers)
        n = len(self.steppers)
        self.ensemble_of, self.options = ensemble_of, options
        self.max_steps = [None] * n if max_steps is None else [None if m is None else int(m) for m in max_steps]
        if len(self.max_steps) != n:
            raise ValueError("max_steps holds one entry per member")
        self.before_solve, self.before_accept, self.after_attempt, self.on_error = before_solve, before_accept, after_attempt, on_error
        self.errors, self.status = [None] * n, [0] * n
        self.rounds = 0

    def live(self):
        """The members that go into the next round (``max_steps`` ends a member here, as ``DriverStepping.run`` does)."""
        out = []
        for k, s in enumerate(self.steppers):
            if self.errors[k] is not None or s.stop_reason is not None:
                continue
            if self.max_steps[k] is not None and len(s.log) >= self.max_steps[k]:
                s.stop_reason = "max_steps"
                continue
            out.append(k)
        return out

    def round(self):
        """One attempted step of every live member.  Returns {member: log row} (a member that ended with an error has none)."""
        live = self.live()
        if not live:
            return {}
        ens = self.ensemble_of(live)
        S = [self.steppers[k] for k in live]
        th = [s.start() for s in S]
        ens.set_time_step([s.inv_dt_of_h(h) for s, (_, h) in zip(S, th)])
        if self.before_solve is not None:
            for k, (t, h) in zip(live, th):
                self.before_solve(k, t, h)
        stats, codes, msgs = ens.newton_solve(self.options)
        failed, fatal = [], []
        for i, k in enumerate(live):
            failed.append(codes[i] in RETRY_CODES)
            fatal.append(codes[i] != backend.OK and not failed[i])
            if fatal[i]:
                self.errors[k], self.status[k] = msgs[i] or "status %d" % codes[i], codes[i]
                if self.on_error is not None:
                    self.on_error(k, codes[i], msgs[i])
            else:
                S[i].sys.record(stats[i])
        mask = [not (failed[i] or fatal[i]) for i in range(len(live))]
        ests = [None] * len(live)
        if any(mask):
            ests = ens.time_error([h for _, h in th], [s.h_prev for s in S], [s.rtol for s in S], [s.atol for s in S], mask)
        plan, actions = [None] * len(live), [0] * len(live)
        for i, s in enumerate(S):
            if fatal[i]:
                continue
            plan[i] = s.decide(th[i][0], th[i][1], stats[i], failed[i], ests[i] if mask[i] else None)
            actions[i] = 1 if plan[i][0].accept else 2
        if self.before_accept is not None and 1 in actions:   # while u_n is still the previous state
            U = ens.get_state()
            for i, k in enumerate(live):
                if actions[i] == 1:
                    self.before_accept(k, stats[i], U[i])
        ens.time_advance(actions)
        rows = {}
        for i, k in enumerate(live):
            if plan[i] is None:
                continue
            S[i].finish(*plan[i])
            rows[k] = plan[i][1]
            if self.after_attempt is not None:
                self.after_attempt(k, rows[k])
        self.rounds += 1
        return rows

    def run(self):
        """Rounds until every member has stopped."""
        while self.live():
            self.round()
        return self


# ---- what the four drivers share ----------------------------------------------------------------------------------------------------
ADAPTIVE_KEYWORDS = dict(adaptive_dt=False, dt_rtol=1e-2, dt_atol=1e-4, dt_init=None, dt_min=0.0, dt_max=None, t_end=None, steady_tol=0.0,
                         max_steps=None, dt_order=1)
ORDER2_ENSEMBLE_REFUSAL = ("dt_order=2: the device ensembles have no order 2 (variable-step BDF2) yet; an order-2 adaptive run is a "
                           "single run (EDLRun / PoreRun / RxnDiffRun / RxnPoreRun with adaptive_dt=True, dt_order=2)")


def refuse_ensemble_order2(members, adaptive):
    """ValueError when a member dict or an adaptive-stepping keyword of an ensemble asks for order 2 (before anything touches the
    device)."""
    asked = [adaptive.get("dt_order", 1)] + [m.get("dt_order", 1) for m in members]
    for v in asked:
        if any(int(x) != 1 for x in (v if isinstance(v, (list, tuple, np.ndarray)) else [v])):
            raise ValueError(ORDER2_ENSEMBLE_REFUSAL)


def pop_adaptive(kwargs):
    """The adaptive-stepping keywords of a run class taken out of its ``**kwargs`` (defaults: ``ADAPTIVE_KEYWORDS``)."""
    return {k: kwargs.pop(k, d) for k, d in ADAPTIVE_KEYWORDS.items()}


def member_adaptive_keywords(n, adaptive):
    """The adaptive-stepping keywords of an ensemble of ``n`` members as one dict per member.  Each value of ``adaptive`` is a
    scalar (all members) or a sequence with one value per member; a wrong length is a ValueError naming the keyword."""
    out = [dict() for _ in range(n)]
    for key, v in adaptive.items():
        if key not in ADAPTIVE_KEYWORDS:
            raise TypeError("unknown adaptive-stepping keyword %r" % key)
        if isinstance(v, (list, tuple, np.ndarray)):
            if len(v) != n:
                raise ValueError("%s: %d values for %d ensemble members (a scalar, or one value per member)" % (key, len(v), n))
            vals = list(v)
        else:
            vals = [v] * n
        for d, x in zip(out, vals):
            d[key] = x
    return out


def add_adaptive_arguments(p):
    """The adaptive-stepping flags every driver shares; times in the driver's scaled units."""
    p.add_argument("--adaptive_dt", action="store_true", help="(addition) adaptive time stepping with error control: the step size is the controller's")
    p.add_argument("--dt_rtol", required=False, default=1e-2, type=float, help="(addition) relative weight of the controller's error norm")
    p.add_argument("--dt_atol", required=False, default=1e-4, type=float, help="(addition) absolute weight of the controller's error norm")
    p.add_argument("--dt_init", required=False, default=None, type=float, help="(addition) first step (default: the reference step)")
    p.add_argument("--dt_min", required=False, default=0.0, type=float, help="(addition) a smaller step ends the run")
    p.add_argument("--dt_max", required=False, default=None, type=float, help="(addition) largest step")
    p.add_argument("--t_end", required=False, default=None, type=float, help="(addition) end time (default: the driver's own T)")
    p.add_argument("--steady_tol", required=False, default=0.0, type=float, help="(addition) stop when the rate of change stays below it; 0 = off")
    p.add_argument("--max_steps", required=False, default=None, type=int, help="(addition) largest number of attempted steps")
    p.add_argument("--dt_order", required=False, default=1, type=int, choices=(1, 2),
                   help="(addition) 1 = backward Euler, 2 = variable-step BDF2 after a backward Euler start-up")


def adaptive_keywords(a):
    """The parsed adaptive-stepping flags as the keywords of the run classes."""
    return {k: getattr(a, k) for k in ADAPTIVE_KEYWORDS}


class DriverStepping:
    """The adaptive mode of a driver's run class: the stepper built from the driver's keywords (``h_ref`` = the reference step,
    ``T`` = the driver's own end time), the actual times of the history rows, the attempt loop and the outputs."""

    def __init__(self, system, solver_parameters, inv_dt_of_h, h_ref, T, dt_rtol=1e-2, dt_atol=1e-4, dt_init=None, dt_min=0.0, dt_max=None,
                 t_end=None, steady_tol=0.0, max_steps=None, adaptive_dt=True, dt_order=1):
        policy = TimeStepPolicy(h_min=float(dt_min), h_max=math.inf if dt_max is None else float(dt_max),
                                t_end=float(T) if t_end is None else float(t_end), steady_tol=float(steady_tol))
        self.stepper = AdaptiveStepper(system, policy, (dt_rtol, dt_atol), inv_dt_of_h, h_ref if dt_init is None else float(dt_init),
                                       solver_parameters=solver_parameters, order=dt_order)
        self.max_steps = None if max_steps is None else int(max_steps)
        self.times = [0.0]

    def attempt(self, before_solve, before_accept, verbose=False):
        """One attempted step; an accepted one adds its time (t_end exactly when the step landed on it).  Returns the log row."""
        return self.attempted(self.stepper.attempt(before_solve, before_accept), verbose)

    def attempted(self, row, verbose=False):
        """What follows an attempt whoever ran it (``attempt``, or an ensemble's round): the time of an accepted step."""
        if row["accepted"]:
            self.times.append(self.stepper.t)
        if verbose:
            print("t = %.6g  h = %.6g  %s  err = %.3g  newton = %d" % (row["t"], row["h"], "accepted" if row["accepted"] else "rejected",
                                                                     row["err"], row["newton"]))
        return row

    def run(self, attempt):
        """``attempt()`` until the run ends: t_end, the steady stop, h_min, or ``max_steps`` attempted steps."""
        while self.stepper.stop_reason is None:
            if self.max_steps is not None and len(self.stepper.log) >= self.max_steps:
                self.stepper.stop_reason = "max_steps"
                break
            attempt()

    def save(self, newpath, meta):
        """timestep_log.npz beside the arrays and the new metadata.json keys."""
        import os
        np.savez(os.path.join(newpath, "timestep_log.npz"), **self.stepper.log_arrays())
        meta.update(self.stepper.summary(), timestep_log="timestep_log.npz")
