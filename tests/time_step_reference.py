"""Adaptive time stepping (include/gmpnp.h "adaptive time stepping", csrc/gmpnp_host_rules.h next_time_step) restated in NumPy: the
error estimator, the accept / reject rule, and the adaptive loop over the oracle's assembly with SuperLU for J dx = b (imported
like step_limit_reference.py; not a conftest).  Test infrastructure only.

    p = u_n + (h / h_prev)(u_n - u_nm1)        d = (u - p) h / (2h + h_prev)        w = atol_f + rtol max(|u|, |u_n|)
    err_f = sqrt(sum_I (d/w)^2 / n_free_f)     rate_f = sqrt(sum_I ((u - u_n)/h)^2 / n_free_f)          over the free dofs"""
import dataclasses
import math
from dataclasses import dataclass, field

import numpy as np
import scipy.sparse.linalg as spla

import gmpnp_oracle as O
from step_limit_reference import step_limit, steric_sum


def free_mask(prob):
    """(nv, nf) True where the dof carries no Dirichlet condition."""
    m = np.ones(prob.ndof, dtype=bool)
    if len(prob.bc_dofs):
        m[np.asarray(prob.bc_dofs, dtype=np.int64)] = False
    return m.reshape(-1, prob.nf)


def time_error(u, un, unm1, h, h_prev, rtol, atol, free):
    """The estimator for (nv, nf) arrays; ``unm1`` None or h_prev <= 0: no history (err 0, rates all the same).  ``atol``: scalar or
    (nf,).  Returns a dict shaped like ``DeviceSolver.time_error``'s; worst_dof = vertex * nf + field of the largest |d/w| (first
    in the order of the arrays), -1 without history or free dofs."""
    u, un = np.asarray(u, dtype=np.float64), np.asarray(un, dtype=np.float64)
    nv, nf = u.shape
    atol = np.broadcast_to(np.asarray(atol, dtype=np.float64), (nf,))
    history = unm1 is not None and h_prev > 0.0
    nonfinite = not np.all(np.isfinite(u))
    n_free = free.sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        rate2 = np.where(free, ((u - un) / h) ** 2, 0.0).sum(axis=0)
        rate_field = np.where(n_free > 0, np.sqrt(rate2 / np.maximum(n_free, 1)), 0.0)
        err_field, worst = np.zeros(nf), -1
        if history:
            p = un + (h / h_prev) * (un - np.asarray(unm1, dtype=np.float64))
            d = (u - p) * (h / (2.0 * h + h_prev))
            w = atol[None, :] + rtol * np.maximum(np.abs(u), np.abs(un))
            q = np.where(free, d / w, 0.0)
            err_field = np.where(n_free > 0, np.sqrt((q ** 2).sum(axis=0) / np.maximum(n_free, 1)), 0.0)
            if free.any() and not nonfinite:
                a = np.where(free, np.abs(q), -1.0).ravel()
                worst = int(np.argmax(a))
    if nonfinite:
        err_field = np.full(nf, np.nan)
        rate_field = np.full(nf, np.nan)
    nanmax = lambda x: float(np.nan) if np.isnan(x).any() else float(x.max(initial=0.0))
    return {"err": nanmax(err_field), "err_field": err_field, "rate": nanmax(rate_field), "rate_field": rate_field,
            "worst_dof": worst, "has_history": bool(history), "nonfinite": bool(nonfinite)}


@dataclass
class Policy:
    safety: float = 0.9
    min_factor: float = 0.2
    max_factor: float = 4.0
    fail_factor: float = 0.25
    h_min: float = 0.0
    h_max: float = np.inf
    t_end: float = np.inf
    steady_tol: float = 0.0
    steady_steps: int = 2


def next_time_step(p, t, h, err, has_history, newton_failed, rate, steady_run):
    """NumPy mirror of the rule.  Returns the tuple (accept, reason, t_next, h_next, stop_end, stop_steady, give_up, steady_run);
    reason: 0 accepted, 1 error too large, 2 Newton failed, 3 NaN error."""
    err, rate = np.float64(err), np.float64(rate)
    if has_history and err > 0.0:
        raw = np.float64(p.safety) / np.sqrt(err)
    else:
        raw = None   # no history: factor 1; err = 0 with history: the upper clamp

    def factor(hi):
        if not has_history:
            return np.float64(1.0)
        if raw is None:
            return np.float64(hi)
        return np.clip(raw, p.min_factor, hi)

    stop_steady = False
    if newton_failed or np.isnan(err):
        accept, reason, t_next, h_next, run = False, 2 if newton_failed else 3, t, np.float64(p.fail_factor) * h, steady_run
    elif has_history and err > 1.0:
        accept, reason, t_next, h_next, run = False, 1, t, h * factor(1.0), steady_run
    else:
        accept, reason, t_next, h_next = True, 0, t + h, h * factor(p.max_factor)
        run = steady_run + 1 if (p.steady_tol > 0.0 and rate < p.steady_tol) else 0
        stop_steady = bool(p.steady_tol > 0.0 and run >= p.steady_steps)
    h_next = min(h_next, p.h_max)
    stop_end = lands = False
    if np.isfinite(p.t_end):
        left = p.t_end - t_next
        if accept and not left > 1e-12 * abs(p.t_end):
            t_next, stop_end = p.t_end, True
        elif left <= 1.01 * h_next:
            lands, h_next = bool(h_next >= p.h_min), left   # the last step, cut to land on t_end, is exempt from h_min
    give_up = bool(not stop_end and not stop_steady and not lands and h_next < p.h_min)
    return bool(accept), int(reason), float(t_next), float(h_next), bool(stop_end), stop_steady, give_up, int(run)


def newton(prob, u, un, tau=0.0, omega=1.0, maximum_iterations=25, relative_tolerance=1e-9, absolute_tolerance=1e-10):
    """The Newton loop of step_limit_reference.newton_loop with the device's verdict on a residual that is not finite (csrc/
    gmpnp_host_rules.h NewtonJudge: NaN / Inf ends the solve as failed at once).  Returns (u, iterations, converged)."""
    u = np.array(u, dtype=np.float64, copy=True)
    nv, nf = prob.coords.shape[0], prob.nf
    a = np.asarray(prob.model.a, dtype=np.float64)[:nf - 1]
    with np.errstate(all="ignore"):
        b, _ = O.assemble(prob, u, un, want_jacobian=False)
        r = float(np.linalg.norm(b))
        r0, its = r, 0
        if not np.isfinite(r):
            return u, its, False
        conv = lambda res: bool(np.float64(res) / np.float64(r0) < relative_tolerance or res < absolute_tolerance)
        done = conv(r)
        while not done and its < maximum_iterations:
            b, A = O.assemble(prob, u, un, want_jacobian=True)
            try:
                dx = spla.splu(A.tocsc()).solve(b)
            except RuntimeError:   # exactly singular
                return u, its, False
            if not np.all(np.isfinite(dx)):
                return u, its, False
            alpha = step_limit(a, u.reshape(nv, nf), dx.reshape(nv, nf), tau)[0] if tau else 1.0
            u -= (omega * alpha) * dx
            its += 1
            b, _ = O.assemble(prob, u, un, want_jacobian=False)
            r = float(np.linalg.norm(b))
            if not np.isfinite(r):
                return u, its, False
            done = conv(r)
    return u, its, done


@dataclass
class LoopResult:
    log: list = field(default_factory=list)       # one dict per attempt: t, h, accepted, reason, err, rate, newton, max_S
    states: list = field(default_factory=list)    # accepted states (as the loop carried them on: perturbed ones when asked)
    times: list = field(default_factory=list)     # their times
    u: np.ndarray = None                          # the last accepted state (unperturbed)
    stop_reason: str = None

    def sequence(self):
        return [r["accepted"] for r in self.log]

    def failures(self):
        return [r["reason"] == 2 for r in self.log]


def adaptive_loop(prob, policy, rtol, atol, h_init, inv_dt_of_h, max_attempts, tau=0.0, omega=1.0, maximum_iterations=25,
                  relative_tolerance=1e-9, absolute_tolerance=1e-10, perturb=0.0, on_accept=None, seed=1234):
    """The drivers' adaptive loop on the oracle: u = 0, u_n = bulk at the start (as ``GMPNPSystem.initialise``); every attempt
    solves from the u it holds (the last accepted state; u_n after a rejection), estimates, decides, accepts (u_nm1 <- u_n,
    u_n <- u) or rejects (u <- u_n).  ``perturb`` = eps: every accepted state is multiplied by (1 + eps xi), xi = +-1 per dof
    from a fixed seed, before the loop goes on from it — the loop's own sensitivity to a change of that size in its iterates.
    ``on_accept(prob, u2d)``: the driver's glue of an accepted step (new Dirichlet values: it may set prob.bc_dofs / bc_vals).
    ``prob.model`` is replaced, never mutated."""
    nv, nf = prob.coords.shape[0], prob.nf
    rng = np.random.default_rng(seed)
    a = np.asarray(prob.model.a, dtype=np.float64)[:nf - 1]
    u = np.zeros(prob.ndof)
    un = np.tile(np.r_[np.ones(nf - 1), 0.0], nv)
    unm1 = None
    t, h, h_prev, run = 0.0, float(h_init), 0.0, 0
    out = LoopResult(u=un.copy())
    for _ in range(max_attempts):
        prob.model = dataclasses.replace(prob.model, inv_dt=float(inv_dt_of_h(h)))
        u_new, its, ok = newton(prob, u, un, tau, omega, maximum_iterations, relative_tolerance, absolute_tolerance)
        est = None
        if ok:
            est = time_error(u_new.reshape(nv, nf), un.reshape(nv, nf), None if unm1 is None else unm1.reshape(nv, nf), h, h_prev,
                             rtol, atol, free_mask(prob))
        err = est["err"] if est else 0.0
        rate = est["rate"] if est else math.inf
        d = next_time_step(policy, t, h, err, bool(est and est["has_history"]), not ok, rate, run)
        row = {"t": t, "h": h, "accepted": d[0], "reason": d[1], "err": err if est else math.nan, "rate": rate if est else math.nan,
               "newton": its, "max_S": math.nan}
        if d[0]:
            row["max_S"] = float(steric_sum(a, u_new.reshape(nv, nf)).max())
            out.u = u_new.copy()
            if perturb:
                u_new = u_new * (1.0 + perturb * rng.choice([-1.0, 1.0], size=u_new.size))
            if on_accept is not None:
                on_accept(prob, u_new.reshape(nv, nf))
            unm1, un, u = un, u_new.copy(), u_new
            h_prev = h
            out.states.append(u_new.copy()); out.times.append(d[2])
        else:
            u = un.copy()
        t, h, run = d[2], d[3], d[7]
        out.log.append(row)
        if d[4] or d[5] or d[6]:
            out.stop_reason = "t_end" if d[4] else ("steady" if d[5] else "h_min")
            break
    return out


def sensitivity(base, other):
    """(s_err, s_u) of two runs of one loop that took the same decisions: the largest change of err at any attempt both estimated,
    and of the final state (max norm).  AssertionError if the decisions differ."""
    assert base.sequence() == other.sequence() and base.failures() == other.failures(), "the perturbed loop decided differently"
    s_err = 0.0
    for r0, r1 in zip(base.log, other.log):
        if not (math.isnan(r0["err"]) or math.isnan(r1["err"])):
            s_err = max(s_err, abs(r0["err"] - r1["err"]))
    return s_err, float(np.abs(base.u - other.u).max())


def decision_margin(log):
    """min |err - 1| over the attempts whose decision read err (history and a converged solve)."""
    m = [abs(r["err"] - 1.0) for r in log if not math.isnan(r["err"]) and (r["err"] > 0.0 or not r["accepted"])]
    return min(m) if m else math.inf
