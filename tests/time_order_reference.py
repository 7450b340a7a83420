"""Second-order adaptive time stepping (include/gmpnp.h "second-order adaptive time stepping", csrc/gmpnp_host_rules.h) restated in
NumPy over the oracle's assembly: the coefficients of variable-step BDF2, its error estimator, the accept / reject rule with an
order, fixed-step marches of either order and the adaptive loop that starts with backward Euler and goes on with BDF2 (imported
like time_step_reference.py; not a conftest).  Test infrastructure only.

    omega = h / h1      alpha0 = (1 + 2 omega)/(1 + omega)      u* = ((1 + omega)^2 u_n - omega^2 u_nm1)/(1 + 2 omega)
    time term: (alpha0 / h) M (u - u*)  =  the oracle's inv_dt M (u - un) with inv_dt = alpha0 inv_dt_of_h(h), un = u*
    p = quadratic through (t - h1 - h2, u_nm2), (t - h1, u_nm1), (t, u_n) at t + h
    d = (u - p) kappa,  kappa = c/(h + h1 + h2 + c),  c = h / alpha0          w = atol_f + rtol max(|u|, |u_n|)"""
import dataclasses
import math

import numpy as np

import time_step_reference as T
from step_limit_reference import steric_sum


def alpha0(omega):
    omega = np.float64(omega)
    return (1.0 + 2.0 * omega) / (1.0 + omega)


def history_weights(omega):
    omega = np.float64(omega)
    q = 1.0 + 2.0 * omega
    return (1.0 + omega) * (1.0 + omega) / q, omega * omega / q


def predictor_weights(h, h1, h2):
    h, h1, h2 = np.float64(h), np.float64(h1), np.float64(h2)
    return (h + h1 + h2) * (h + h1) / ((h1 + h2) * h1), -((h + h1 + h2) * h) / (h1 * h2), (h + h1) * h / (h2 * (h1 + h2))


def error_share(h, h1, h2):
    h, h1, h2 = np.float64(h), np.float64(h1), np.float64(h2)
    c = h / alpha0(h / h1)
    return c / (h + h1 + h2 + c)


def history_vector(un, unm1, omega):
    a, b = history_weights(omega)
    return a * np.asarray(un, dtype=np.float64) - b * np.asarray(unm1, dtype=np.float64)


def time_error2(u, un, unm1, unm2, h, h1, h2, rtol, atol, free):
    """The order-2 estimator for (nv, nf) arrays, shaped like ``time_step_reference.time_error``; ``unm1`` or ``unm2`` None, or
    h1 <= 0 or h2 <= 0: no history (err 0, the rates all the same)."""
    u, un = np.asarray(u, dtype=np.float64), np.asarray(un, dtype=np.float64)
    nv, nf = u.shape
    atol = np.broadcast_to(np.asarray(atol, dtype=np.float64), (nf,))
    history = unm1 is not None and unm2 is not None and h1 > 0.0 and h2 > 0.0
    nonfinite = not np.all(np.isfinite(u))
    n_free = free.sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        rate2 = np.where(free, ((u - un) / h) ** 2, 0.0).sum(axis=0)
        rate_field = np.where(n_free > 0, np.sqrt(rate2 / np.maximum(n_free, 1)), 0.0)
        err_field, worst = np.zeros(nf), -1
        if history:
            wn, wm1, wm2 = predictor_weights(h, h1, h2)
            p = wn * un + wm1 * np.asarray(unm1, dtype=np.float64) + wm2 * np.asarray(unm2, dtype=np.float64)
            d = (u - p) * error_share(h, h1, h2)
            w = atol[None, :] + rtol * np.maximum(np.abs(u), np.abs(un))
            q = np.where(free, d / w, 0.0)
            err_field = np.where(n_free > 0, np.sqrt((q ** 2).sum(axis=0) / np.maximum(n_free, 1)), 0.0)
            if free.any() and not nonfinite:
                worst = int(np.argmax(np.where(free, np.abs(q), -1.0).ravel()))
    if nonfinite:
        err_field = np.full(nf, np.nan)
        rate_field = np.full(nf, np.nan)
    nanmax = lambda x: float(np.nan) if np.isnan(x).any() else float(x.max(initial=0.0))
    return {"err": nanmax(err_field), "err_field": err_field, "rate": nanmax(rate_field), "rate_field": rate_field,
            "worst_dof": worst, "has_history": bool(history), "nonfinite": bool(nonfinite)}


def next_time_step(p, t, h, err, has_history, newton_failed, rate, steady_run, order=1):
    """NumPy mirror of the rule with an order; order 1 IS ``time_step_reference.next_time_step``.  The tuple of that function."""
    if order == 1:
        return T.next_time_step(p, t, h, err, has_history, newton_failed, rate, steady_run)
    err, rate = np.float64(err), np.float64(rate)
    raw = np.float64(p.safety) / np.cbrt(err) if (has_history and err > 0.0) else None

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
        accept, reason, t_next, h_next = True, 0, t + h, h * factor(min(p.max_factor, 2.0))
        run = steady_run + 1 if (p.steady_tol > 0.0 and rate < p.steady_tol) else 0
        stop_steady = bool(p.steady_tol > 0.0 and run >= p.steady_steps)
    h_next = min(h_next, p.h_max)
    stop_end = lands = False
    if np.isfinite(p.t_end):
        left = p.t_end - t_next
        if accept and not left > 1e-12 * abs(p.t_end):
            t_next, stop_end = p.t_end, True
        elif left <= 1.01 * h_next:
            lands, h_next = bool(h_next >= p.h_min), left
    give_up = bool(not stop_end and not stop_steady and not lands and h_next < p.h_min)
    return bool(accept), int(reason), float(t_next), float(h_next), bool(stop_end), stop_steady, give_up, int(run)


def solve_step(prob, u, un, unm1, h, h1, inv_dt_of_h, order2, **newton):
    """One step of length h from the start u: backward Euler against un, or (``order2``) BDF2 against u* with alpha0 inv_dt.
    ``prob.model`` is replaced, never mutated.  Returns ``time_step_reference.newton``'s (u, iterations, converged)."""
    if order2:
        omega = h / h1
        prob.model = dataclasses.replace(prob.model, inv_dt=float(alpha0(omega) * inv_dt_of_h(h)))
        return T.newton(prob, u, history_vector(un, unm1, omega), **newton)
    prob.model = dataclasses.replace(prob.model, inv_dt=float(inv_dt_of_h(h)))
    return T.newton(prob, u, un, **newton)


def fixed_step_march(prob, u0, h, n, inv_dt_of_h, order, startup=1, **newton):
    """n steps of length h from the state u0 (u = u_n = u0, no history).  Order 2: ``startup`` backward Euler steps, then BDF2 with
    omega = 1 (one first-order step costs O(h^2), as the scheme's global error; the adaptive stepper takes two, the second for its
    estimate).  Returns the list of the n + 1 states."""
    states = [np.array(u0, dtype=np.float64, copy=True)]
    for k in range(n):
        order2 = order == 2 and k >= startup
        u, _, ok = solve_step(prob, states[-1], states[-1], states[-2] if order2 else None, h, h, inv_dt_of_h, order2, **newton)
        assert ok, "Newton did not converge in step %d of the fixed-step march" % k
        states.append(u)
    return states


def adaptive_loop(prob, policy, rtol, atol, h_init, inv_dt_of_h, max_attempts, order=2, tau=0.0, omega=1.0, maximum_iterations=25,
                  relative_tolerance=1e-9, absolute_tolerance=1e-10, perturb=0.0, on_accept=None, seed=1234):
    """``time_step_reference.adaptive_loop`` with an order: the order of an attempt is 2 when ``order`` is 2 and the loop holds three
    accepted states (levels = 2), else 1 — one backward Euler step without an estimate, one with the order-1 estimator, BDF2 from
    then on; a rejection keeps the history.  The rows of the log also hold ``order``.  Same arguments and result otherwise."""
    nv, nf = prob.coords.shape[0], prob.nf
    rng = np.random.default_rng(seed)
    a = np.asarray(prob.model.a, dtype=np.float64)[:nf - 1]
    newton = dict(tau=tau, omega=omega, maximum_iterations=maximum_iterations, relative_tolerance=relative_tolerance,
                  absolute_tolerance=absolute_tolerance)
    u = np.zeros(prob.ndof)
    un = np.tile(np.r_[np.ones(nf - 1), 0.0], nv)
    unm1 = unm2 = None
    levels = 0
    t, h, h1, h2, run = 0.0, float(h_init), 0.0, 0.0, 0
    out = T.LoopResult(u=un.copy())
    shape = lambda x: None if x is None else x.reshape(nv, nf)
    for _ in range(max_attempts):
        o = 2 if (order == 2 and levels >= 2) else 1
        u_new, its, ok = solve_step(prob, u, un, unm1, h, h1, inv_dt_of_h, o == 2, **newton)
        est = None
        if ok and o == 2:
            est = time_error2(shape(u_new), shape(un), shape(unm1), shape(unm2), h, h1, h2, rtol, atol, T.free_mask(prob))
        elif ok:
            est = T.time_error(shape(u_new), shape(un), shape(unm1), h, h1, rtol, atol, T.free_mask(prob))
        err = est["err"] if est else 0.0
        rate = est["rate"] if est else math.inf
        d = next_time_step(policy, t, h, err, bool(est and est["has_history"]), not ok, rate, run, o)
        row = {"t": t, "h": h, "accepted": d[0], "reason": d[1], "err": err if est else math.nan, "rate": rate if est else math.nan,
               "newton": its, "max_S": math.nan, "order": o}
        if d[0]:
            row["max_S"] = float(steric_sum(a, shape(u_new)).max())
            out.u = u_new.copy()
            if perturb:
                u_new = u_new * (1.0 + perturb * rng.choice([-1.0, 1.0], size=u_new.size))
            if on_accept is not None:
                on_accept(prob, shape(u_new))
            unm2, unm1, un, u = unm1, un, u_new.copy(), u_new
            levels = min(levels + 1, 2 if order == 2 else 1)
            h2, h1 = h1, h
            out.states.append(u_new.copy()); out.times.append(d[2])
        else:
            u = un.copy()
        t, h, run = d[2], d[3], d[7]
        out.log.append(row)
        if d[4] or d[5] or d[6]:
            out.stop_reason = "t_end" if d[4] else ("steady" if d[5] else "h_min")
            break
    return out
