"""Periodic steady state of a potential programme: the limit cycle of a pulse train or a voltammogram by Anderson acceleration of the
cycle map (not a reference feature).  The cycle map Phi takes the state at the start of one period of the
waveform, marched in fixed mode, to the state at its end; its fixed point is the cycle that repeats.  The two host rules are stated in
C++ in csrc/gmpnp_host_rules.h (``anderson_weights``, ``cycle_verdict``) and here in Python, operation for operation
(tests/test_periodic_reference.py compiles that one with the host compiler alone and compares); ``run_periodic`` is the loop over an
``ops`` object, as ``programme.run_programme`` is: the same loop runs over a NumPy system on the CPU (tests/periodic_reference.py) and
over a device handle (``programme.DeviceProgrammeOps``)."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from .programme import run_programme

MAX_DEPTH = 8               # GMPNP_CYCLE_MAX_DEPTH
PIVOT_FLOOR = 1.0e-12       # kCyclePivotFloor
SUM_SLACK = 1.0e-12         # kCycleSumSlack
CONTINUE, CONVERGED, RESTART, GIVE_UP = 0, 1, 2, 3
VERDICTS = {CONTINUE: "continue", CONVERGED: "converged", RESTART: "restart", GIVE_UP: "give_up"}


@dataclass
class PeriodicPolicy:
    tol: float = 1.0            # converged at err <= tol (the weighted RMS of Phi(x) - x, in units of the weights)
    depth: int = 4              # differences of a full window, 1 ... 8
    max_cycles: int = 50
    tau: float = 0.9            # the step limiter's fraction of the mix (0: none)
    growth: float = 10.0        # restart where the residual grew by more than this over the cycle before: a safeguard, not a tuned constant


def check_policy(policy):
    """ValueError (``periodic``) where a field of the policy is out of range."""
    if not (math.isfinite(float(policy.tol)) and float(policy.tol) > 0.0):
        raise ValueError("periodic: tol must be finite and > 0")
    if not (float(policy.depth).is_integer() and 1 <= int(policy.depth) <= MAX_DEPTH):
        raise ValueError("periodic: depth is 1 ... %d" % MAX_DEPTH)
    if not (float(policy.max_cycles).is_integer() and int(policy.max_cycles) >= 1):
        raise ValueError("periodic: max_cycles must be at least 1")
    if not (float(policy.tau) == 0.0 or 0.0 < float(policy.tau) < 1.0):
        raise ValueError("periodic: tau must be 0 (no limiter) or lie in (0, 1)")
    if not (math.isfinite(float(policy.growth)) and float(policy.growth) > 1.0):
        raise ValueError("periodic: growth must be finite and > 1")
    return policy


# ---- the rules (csrc/gmpnp_host_rules.h states them in C++, statement for statement) ------------------------------------------------------
def gamma_valid(gamma):
    """What ``gmpnp_cycle_mix`` asks of its weights: finite, and summing (left to right) to 1 within 1e-12."""
    if not 1 <= len(gamma) <= MAX_DEPTH + 1:
        return False
    total = 0.0
    for g in gamma:
        g = float(g)
        if not math.isfinite(g):
            return False
        total = total + g
    return abs(total - 1.0) <= SUM_SLACK


def anderson_weights(m, A, b):
    """(gamma (m + 1,), dropped): the mixing weights of a window of m + 1 pairs from its normal system A theta = b (A (m, m) symmetric,
    the upper triangle is read; column 0 is the oldest difference).  Cholesky of the columns lo ... m - 1; where a squared pivot is below
    1e-12 x the largest diagonal entry of those columns or not finite, a theta is not finite or the weights do not sum to 1 within
    1e-12, the oldest column is dropped and the elimination starts again; no column left: gamma = (0, ..., 0, 1)."""
    m = min(max(int(m), 0), MAX_DEPTH)
    A = [[float(A[i][j]) for j in range(m)] for i in range(m)]
    b = [float(b[i]) for i in range(m)]
    for lo in range(m):
        n = m - lo
        L = [[0.0] * n for _ in range(n)]
        top, ok = 0.0, True
        for i in range(n):
            d = A[lo + i][lo + i]
            if not math.isfinite(d):
                ok = False
            elif d > top:
                top = d
        for j in range(n):
            if not ok:
                break
            piv = A[lo + j][lo + j]
            for k in range(j):
                piv = piv - L[j][k] * L[j][k]
            if not math.isfinite(piv) or not piv >= PIVOT_FLOOR * top or not piv > 0.0:
                ok = False
                break
            L[j][j] = math.sqrt(piv)
            for i in range(j + 1, n):
                v = A[lo + j][lo + i]
                for k in range(j):
                    v = v - L[i][k] * L[j][k]
                L[i][j] = v / L[j][j]
        if not ok:
            continue
        y, th = [0.0] * n, [0.0] * n
        for i in range(n):
            v = b[lo + i]
            for k in range(i):
                v = v - L[i][k] * y[k]
            y[i] = v / L[i][i]
        for i in range(n - 1, -1, -1):
            v = y[i]
            for k in range(i + 1, n):
                v = v - L[k][i] * th[k]
            th[i] = v / L[i][i]
            if not math.isfinite(th[i]):
                ok = False
        if not ok:
            continue
        gamma = [0.0] * (m + 1)
        gamma[lo] = th[0]
        for i in range(1, n):
            gamma[lo + i] = th[i] - th[i - 1]
        gamma[m] = 1.0 - th[n - 1]
        if gamma_valid(gamma):
            return gamma, lo
    return [0.0] * m + [1.0], m


def cycle_verdict(errs, policy, nonfinite=False):
    """CONTINUE, CONVERGED, RESTART or GIVE_UP from the residuals ``errs`` of the cycles marched so far (the last one is judged)."""
    n = len(errs)
    if n < 1:
        return CONTINUE
    e = float(errs[-1])
    bad = bool(nonfinite) or not math.isfinite(e)
    if not bad and e <= float(policy.tol):
        return CONVERGED
    if n >= int(policy.max_cycles):
        return GIVE_UP
    if bad:
        return RESTART
    if n >= 2 and math.isfinite(float(errs[-2])) and e > float(policy.growth) * float(errs[-2]):
        return RESTART
    return CONTINUE


# ---- the loop --------------------------------------------------------------------------------------------------------------------------
HISTORY_COLUMNS = ("err", "err_max", "window", "gamma", "alpha", "dropped", "restart", "newton", "verdict")


def run_periodic(ops, period_segs, policy=None, steps_per_segment=None):
    """Looks for the limit cycle of the waveform ``period_segs`` (ONE period as ``programme`` segments; it repeats from its first
    potential, with a jump where the last one differs) from the current state of ``ops`` and returns dict(history, converged, cycles, restarts, residual, record, state).  ``ops`` supplies
    ``run_programme``'s operations and

        cycle_open(depth) / cycle_close()
        cycle_begin()                       x_k <- the state
        cycle_end() -> dict                 g_k <- the state; err, err_max, window, nonfinite, A, b
        cycle_mix(gamma, tau) -> alpha      the state <- g_k + alpha (sum_j gamma_j g_j - g_k), records dropped, accumulators fresh;
                                            NaN where the mix met a value that is not finite (nothing applied)
        cycle_restart()                     empties the window
        state()                             a copy of the state (``state`` of the result: where the recorded period starts)
        newton_iterations                   a running count (optional)

    Every cycle marches one period with the unchanged ``run_programme`` in fixed mode (``steps_per_segment``: the map is then a
    deterministic, smooth function of the state) between ``cycle_begin`` and ``cycle_end``, and ``cycle_verdict`` decides: converged;
    give up at ``max_cycles``; restart (the window is emptied and the next cycle starts from g_k); or mix with ``anderson_weights``.
    On convergence the state is put to g_k by a mix with gamma = (0, ..., 0, 1) — the handle is then where a state set from outside
    leaves it, with fresh accumulators — and ONE more period is marched: ``record`` is ``run_programme``'s result of that period, and
    the records ``ops`` holds are that period's alone.  Where the search gives up, ``record`` is the last marched period (``converged``
    False)."""
    policy = check_policy(PeriodicPolicy() if policy is None else policy)
    if steps_per_segment is None or int(steps_per_segment) < 1:
        raise ValueError("periodic: the cycle map is marched in fixed mode (steps_per_segment)")
    segs = [tuple(float(v) for v in s) for s in period_segs]
    if not segs:
        raise ValueError("periodic: the waveform of one period has no segment")
    history, errs, restarts, converged, record, state = [], [], 0, False, None, None
    ops.cycle_open(int(policy.depth))
    try:
        while True:
            n0 = int(getattr(ops, "newton_iterations", 0))
            ops.cycle_begin()
            last = run_programme(ops, segs, steps_per_segment=int(steps_per_segment))
            rep = ops.cycle_end()
            errs.append(float(rep["err"]))
            verdict = cycle_verdict(errs, policy, rep["nonfinite"])
            row = {"err": float(rep["err"]), "err_max": float(rep["err_max"]), "window": int(rep["window"]), "gamma": [], "alpha": math.nan,
                   "dropped": 0, "restart": False, "newton": int(getattr(ops, "newton_iterations", 0)) - n0, "verdict": verdict}
            history.append(row)
            if verdict == CONVERGED:
                converged = True
                ops.cycle_mix([0.0] * (int(rep["window"]) - 1) + [1.0], 0.0)
                state = ops.state()
                record = run_programme(ops, segs, steps_per_segment=int(steps_per_segment))
                break
            if verdict == GIVE_UP:   # the last marched period stands in for the record (its records are what ``ops`` holds)
                record, state = last, ops.state()
                break
            if verdict == CONTINUE:
                gamma, dropped = anderson_weights(int(rep["window"]) - 1, rep["A"], rep["b"])
                alpha = ops.cycle_mix(gamma, float(policy.tau))
                row.update(gamma=[float(g) for g in gamma], alpha=float(alpha), dropped=int(dropped))
                if math.isfinite(alpha):
                    continue
            ops.cycle_restart()   # from g_k, which is the state the period left
            row["restart"] = True
            restarts += 1
    finally:
        ops.cycle_close()
    return {"history": history, "converged": converged, "cycles": len(history), "restarts": restarts,
            "residual": errs[-1] if errs else math.nan, "record": record, "state": state}


def history_arrays(history):
    """The history as arrays by column (``programme_periodic.npz``): err, err_max [units of the weights], window, gamma (cycles,
    MAX_DEPTH + 1; NaN behind the window and where no mix was made), alpha, dropped, restart, newton, verdict."""
    n = len(history)
    gamma = np.full((n, MAX_DEPTH + 1), np.nan)
    for k, r in enumerate(history):
        gamma[k, :len(r["gamma"])] = r["gamma"]
    out = {"err": np.array([r["err"] for r in history], dtype=np.float64), "err_max": np.array([r["err_max"] for r in history], dtype=np.float64),
           "window": np.array([r["window"] for r in history], dtype=np.int64), "gamma": gamma,
           "alpha": np.array([r["alpha"] for r in history], dtype=np.float64), "dropped": np.array([r["dropped"] for r in history], dtype=np.int64),
           "restart": np.array([r["restart"] for r in history], dtype=np.bool_), "newton": np.array([r["newton"] for r in history], dtype=np.int64),
           "verdict": np.array([r["verdict"] for r in history], dtype=np.int64)}
    assert set(out) == set(HISTORY_COLUMNS)
    return out


# ---- the keyword of the 1D driver ---------------------------------------------------------------------------------------------------------
PERIODIC_FIELDS = {"tol", "depth", "max_cycles", "tau", "growth", "rtol", "atol"}
METADATA_KEYS = ("programme_periodic_cycles", "programme_periodic_converged", "programme_periodic_residual", "programme_periodic_restarts")


def check_periodic(periodic, par):
    """The refusals of the ``periodic`` key of a driver's ``programme`` dict ``par``, before anything touches the device; returns
    (policy, rtol, atol)."""
    if not isinstance(periodic, dict) or set(periodic) - PERIODIC_FIELDS:
        raise ValueError("programme: periodic takes dict(%s)" % ", ".join(sorted(PERIODIC_FIELDS)))
    if par.get("steps_per_segment") is None:
        raise ValueError("programme: periodic needs the fixed mode (steps_per_segment): the cycle map must be a smooth function of the state")
    if par.get("sensitivities"):
        raise ValueError("programme: periodic is not available with sensitivities (the sensitivities of the limit cycle are not computed)")
    if int(par.get("cycles", 1) or 1) != 1:
        raise ValueError("programme: with periodic the waveform is one period: cycles must be 1 or absent (max_cycles bounds the search)")
    if par.get("kind") == "table" and float(par["electrode_voltage"][-1]) != float(par["electrode_voltage"][0]):
        raise ValueError("programme: periodic needs a table whose last potential equals its first")
    rtol, atol = float(periodic.get("rtol", 1e-2)), float(periodic.get("atol", 1e-4))
    if not (math.isfinite(rtol) and rtol >= 0.0 and math.isfinite(atol) and atol > 0.0):
        raise ValueError("programme: periodic needs a finite rtol >= 0 and a finite atol > 0")
    try:
        policy = check_policy(PeriodicPolicy(**{k: periodic[k] for k in ("tol", "depth", "max_cycles", "tau", "growth") if k in periodic}))
    except ValueError as e:
        raise ValueError("programme: " + str(e)) from None
    return policy, rtol, atol


def metadata(res):
    out = {"programme_periodic_cycles": int(res["cycles"]), "programme_periodic_converged": bool(res["converged"]),
           "programme_periodic_residual": float(res["residual"]), "programme_periodic_restarts": int(res["restarts"])}
    assert set(out) == set(METADATA_KEYS)
    return out
