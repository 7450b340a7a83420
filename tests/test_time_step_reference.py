"""Adaptive time stepping on the CPU: the NumPy estimator (tests/time_step_reference.py) against closed forms, the accept / reject
rule of the library (gmpnp_host_rules.h next_time_step, compiled with the host compiler alone) against its NumPy mirror and the
Python statement the drivers run (gmpnp_amd/timestep.py), and the reference adaptive loop over the oracle's assembly on the 1 um
mesh with its attempt log pinned.

Newton tolerances of the reference loop: relative 1e-9 as everywhere; absolute 1e-6, NOT the 1e-10 of the first-solve tests.  From
the second step on a solve starts at u = u_n, where the residual is small already (0.34 for K+ at -2.5, 4.7 for Cs+ at -10), and the
assembled residual cannot fall below its rounding floor: measured 6.7e-10 ... 1.5e-9 (K+, -2.5) and 2.1e-8 ... 2.9e-8 (Cs+, -10) on
this oracle, both above 1e-10 and above 1e-9 times the start, so with 1e-10 every solve after the first ends at the iteration cap.
1e-6 is 40 times the larger floor and is passed by the quadratic phase in one iteration (4.9e-1 -> 3.0e-7 -> 2.4e-8): the stopping
iteration does not depend on the rounding, which is what comparing iterates instead of stopping points needs."""
import math
import os
import subprocess
import warnings

import numpy as np
import pytest

import time_step_reference as T
from conftest import ROOT, _edl

NEWTON = dict(maximum_iterations=25, relative_tolerance=1e-9, absolute_tolerance=1e-6)
DT_ATOL = 1e-4
# (cation, voltage) -> dt_rtol, steady_tol, attempts.  K+ runs with dt_rtol 5e-2: at 1e-2 the loop's own sensitivity (s_err 2.5e-3 from
# a 1e-8 perturbation of the accepted states, 58 attempts) is more than 1/100 of the controller's distance from err = 1 (0.11; the
# controller steers err to safety^2 = 0.81), 3e-2 and 5e-2 pass (s_err 7.8e-4 / 6.3e-4, margins 0.110 / 0.116)
CASES = {("K", -2.5): dict(dt_rtol=5e-2, steady_tol=1e-5, attempts=400), ("Cs", -10.0): dict(dt_rtol=1e-2, steady_tol=0.0, attempts=12)}
# the pinned attempt logs: A accepted, R rejected by the error test, F Newton failure; Newton iterations of every attempt that was
# not a failure (a failed solve's iterates are outside the admissible set, where nothing pins them; its count is the cap)
PINNED = {
    ("K", -2.5): dict(sequence="ARRRARA" + "A" * 31, stop="steady", attempts=38,
                      newton=[6, 4] + [3] * 10 + [2] * 25 + [1]),
    ("Cs", -10.0): dict(sequence="FFARRRAAAAAA", stop=None, attempts=12, newton=[25, 25, 6, 4, 4, 3, 3, 3, 3, 3, 4, 4]),
}


def run_case(cation, voltage, perturb=0.0):
    c = CASES[(cation, voltage)]
    ep, _, prob = _edl(L_n=1e-6, cation=cation, voltage_multiplier=voltage)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = T.adaptive_loop(prob, T.Policy(steady_tol=c["steady_tol"]), c["dt_rtol"], DT_ATOL, ep.dts[0], lambda h: 1.0 / (h * ep.L_D),
                              c["attempts"], perturb=perturb, **NEWTON)
    return ep, res


_runs = {}


def reference_runs(cation, voltage):
    """(ep, plain run, run with every accepted state perturbed by 1e-8 relative), computed once and shared (tests/test_gpu_time_step.py
    imports this)."""
    key = (cation, voltage)
    if key not in _runs:
        ep, base = run_case(cation, voltage)
        _, pert = run_case(cation, voltage, perturb=1e-8)
        _runs[key] = (ep, base, pert)
    return _runs[key]


def letters(res):
    return "".join("A" if r["accepted"] else ("F" if r["reason"] == 2 else "R") for r in res.log)


# ---- estimator model against closed forms ------------------------------------------------------------------------------------------
def quadratic_states(nv=37, nf=7, seed=3):
    rng = np.random.default_rng(seed)
    a, b, c = rng.uniform(0.5, 1.5, (nv, nf)), rng.standard_normal((nv, nf)), rng.standard_normal((nv, nf))
    t0, t1, t2 = 0.3, 0.3 + 0.07, 0.3 + 0.07 + 0.11   # three unequal times: h_prev = 0.07, h = 0.11
    f = lambda t: a + b * t + 0.5 * c * t * t
    # u_nm1, u_n: the quadratic itself; u: the backward Euler step of u' = b + c t from u_n, which is what the estimator is fed
    # in a run (u_BE - u(t2) = 1/2 c h^2, and u(t2) - p = 1/2 c h (h + h_prev): together the 1/2 c h (2h + h_prev) of the rule)
    h = t2 - t1
    return f(t0), f(t1), f(t1) + h * (b + c * t2), c, t1 - t0, h


def test_quadratic_in_time_gives_half_u_tt_h_squared():
    """u'' constant: d = 1/2 u'' h^2 exactly, for the backward Euler step u of the quadratic's ODE.  (The exact sample u(t2) in u's
    place gives 1/2 u'' h^2 (h + h_prev) / (2h + h_prev): the second case.)"""
    unm1, un, u, c, h_prev, h = quadratic_states()
    free = np.ones(u.shape, dtype=bool)
    rtol, atol = 1e-2, np.linspace(1e-4, 7e-4, 7)
    w = atol[None, :] + rtol * np.maximum(np.abs(u), np.abs(un))
    d = 0.5 * c * h * h
    e = T.time_error(u, un, unm1, h, h_prev, rtol, atol, free)
    want = np.sqrt(((d / w) ** 2).mean(axis=0))
    assert e["has_history"] and not e["nonfinite"]
    assert np.abs(e["err_field"] - want).max() <= 1e-14 * want.max() + 1e-14
    assert e["err"] == e["err_field"].max()
    assert e["worst_dof"] == int(np.argmax(np.abs(d / w)))
    rate = np.sqrt((((u - un) / h) ** 2).mean(axis=0))
    assert np.abs(e["rate_field"] - rate).max() <= 1e-14 * rate.max()
    e2 = T.time_error(u - d, un, unm1, h, h_prev, rtol, atol, free)   # u - 1/2 c h^2 = the quadratic at t2
    w2 = atol[None, :] + rtol * np.maximum(np.abs(u - d), np.abs(un))
    want2 = np.sqrt(((d * (h + h_prev) / (2 * h + h_prev) / w2) ** 2).mean(axis=0))
    assert np.abs(e2["err_field"] - want2).max() <= 1e-13 * want2.max()


def test_linear_in_time_gives_zero():
    unm1, un, u, c, h_prev, h = quadratic_states()
    u = un + (h / h_prev) * (un - unm1)
    e = T.time_error(u, un, unm1, h, h_prev, 1e-2, 1e-4, np.ones(u.shape, dtype=bool))
    assert e["err"] <= 1e-12   # (rounding of the extrapolation over w >= 1e-4)


def test_dirichlet_dofs_are_ignored_and_a_field_without_free_dofs_reports_zero():
    unm1, un, u, c, h_prev, h = quadratic_states()
    free = np.ones(u.shape, dtype=bool)
    free[[0, 5, 36], 6] = False
    free[:, 2] = False
    base = T.time_error(u, un, unm1, h, h_prev, 1e-2, 1e-4, free)
    u2 = u.copy()
    u2[[0, 5, 36], 6] += 1e6
    u2[:, 2] -= 1e6
    e = T.time_error(u2, un, unm1, h, h_prev, 1e-2, 1e-4, free)
    assert np.array_equal(e["err_field"], base["err_field"]) and np.array_equal(e["rate_field"], base["rate_field"])
    assert e["worst_dof"] == base["worst_dof"] and e["err_field"][2] == 0.0 and e["rate_field"][2] == 0.0


def test_no_history_and_nonfinite():
    unm1, un, u, c, h_prev, h = quadratic_states()
    free = np.ones(u.shape, dtype=bool)
    for e in (T.time_error(u, un, None, h, h_prev, 1e-2, 1e-4, free), T.time_error(u, un, unm1, h, 0.0, 1e-2, 1e-4, free)):
        assert not e["has_history"] and e["err"] == 0.0 and e["rate"] > 0.0 and e["worst_dof"] == -1
    u[3, 1] = np.nan
    e = T.time_error(u, un, unm1, h, h_prev, 1e-2, 1e-4, free)
    assert e["nonfinite"] and math.isnan(e["err"]) and np.all(np.isnan(e["err_field"]))


# ---- the host rule: C++ (g++ alone), the NumPy mirror, the drivers' Python statement ------------------------------------------------
DRIVER = r"""
#include <cstdio>
#include <iostream>
#include <sstream>
#include "gmpnp_host_rules.h"
using namespace gmpnp;
int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string tok;
    auto num = [&]() { in >> tok; return std::stod(tok); };   // (reads "nan" and "inf" too)
    TimeStepPolicy p;
    p.safety = num(); p.min_factor = num(); p.max_factor = num(); p.fail_factor = num(); p.h_min = num(); p.h_max = num();
    p.t_end = num(); p.steady_tol = num(); p.steady_steps = (int)num();
    const double t = num(), h = num(), err = num(); const bool hist = num() != 0.0, failed = num() != 0.0;
    const double rate = num(); const int run = (int)num();
    const TimeStepDecision d = next_time_step(p, t, h, err, hist, failed, rate, run);
    printf("%d %d %.17g %.17g %d %d %d %d\n", (int)d.accept, d.reason, d.t_next, d.h_next, (int)d.stop_end, (int)d.stop_steady, (int)d.give_up, d.steady_run);
  }
  printf("%d %d\n", (int)time_step_valid(0.0), (int)(time_step_valid(-1.0) || time_step_valid(NAN) || time_step_valid(INFINITY)));
  return 0;
}
"""

DEFAULT = dict(safety=0.9, min_factor=0.2, max_factor=4.0, fail_factor=0.25, h_min=0.0, h_max=math.inf, t_end=math.inf, steady_tol=0.0,
               steady_steps=2)
# (policy overrides, t, h, err, has_history, newton_failed, rate, steady_run)
RULE_CASES = [
    ({}, 0.0, 1.0, 0.0, False, False, 3.0, 0),                     # no history: accept, factor 1
    ({}, 1.0, 1.0, 0.0, True, False, 3.0, 0),                      # err = 0 with history: max_factor
    ({}, 1.0, 0.5, 0.25, True, False, 3.0, 0),                     # accept, factor 0.9 * 2
    ({}, 1.0, 0.5, 1e-6, True, False, 3.0, 0),                     # accept, clamped to max_factor
    ({}, 1.0, 0.5, 1.0, True, False, 3.0, 0),                      # err = 1 exactly: accepted
    ({}, 1.0, 0.5, 1.0000001, True, False, 3.0, 0),                # just above: rejected, factor 0.9
    ({}, 1.0, 0.5, 4.0, True, False, 3.0, 0),                      # rejected, factor 0.45
    ({}, 1.0, 0.5, 62.8, True, False, 3.0, 0),                     # rejected, clamped to min_factor
    ({}, 1.0, 0.5, 0.95, True, False, 3.0, 0),                     # accepted with a factor below 1 (0.9 / sqrt(0.95))
    ({}, 1.0, 0.5, 0.3, True, True, 3.0, 1),                       # Newton failed: fail_factor, the steady counter stays
    ({}, 1.0, 0.5, math.nan, True, False, 3.0, 1),                 # NaN err: reject, fail_factor
    ({}, 1.0, 0.5, math.nan, False, False, math.nan, 0),           # NaN err without history
    (dict(h_max=0.7), 1.0, 0.5, 0.01, True, False, 3.0, 0),        # h_max clamp
    (dict(h_max=0.1), 1.0, 0.5, 9.0, True, False, 3.0, 0),         # h_max clamp after a rejection
    (dict(t_end=2.0), 1.0, 0.5, 0.81, True, False, 3.0, 0),        # next step shortened to land on t_end (left 0.5 = h_next)
    (dict(t_end=2.0), 1.0, 0.5, 0.05, True, False, 3.0, 0),        # ... (left 0.5 < h_next 2.0)
    (dict(t_end=2.0), 1.0, 0.5, 0.83, True, False, 3.0, 0),        # sliver rule: h_next 0.4939, left 0.5 <= 1.01 h_next is false -> kept
    (dict(t_end=2.0), 1.0, 0.5, 0.8262, True, False, 3.0, 0),      # ... stretched by less than 1 %: h_next = left
    (dict(t_end=2.0), 1.5, 0.5, 0.5, True, False, 3.0, 0),         # lands on t_end: stop_end, t_next = t_end exactly
    (dict(t_end=2.0), 1.7, 0.3, 0.5, True, False, 3.0, 0),         # ... through rounding (1.7 + 0.3)
    (dict(t_end=2.0), 1.5, 0.5, 9.0, True, False, 3.0, 0),         # rejected in front of t_end: no stop
    (dict(t_end=2.0, h_min=0.2), 1.5, 0.5, 90.0, True, False, 3.0, 0),   # h_min give-up after an error rejection
    (dict(h_min=0.2), 1.0, 0.5, 0.1, True, True, 3.0, 0),          # h_min give-up after a Newton failure
    (dict(h_min=0.1), 1.0, 0.5, 0.1, True, True, 3.0, 0),          # 0.125 >= h_min: goes on
    (dict(steady_tol=1e-5), 1.0, 0.5, 0.1, True, False, 1e-6, 0),  # steady counter 0 -> 1
    (dict(steady_tol=1e-5), 1.0, 0.5, 0.1, True, False, 1e-6, 1),  # 1 -> 2: stop_steady
    (dict(steady_tol=1e-5), 1.0, 0.5, 0.1, True, False, 1e-4, 1),  # a non-steady accept resets the counter
    (dict(steady_tol=1e-5), 1.0, 0.5, 9.0, True, False, 1e-6, 1),  # a rejection leaves it
    (dict(steady_tol=1e-5, steady_steps=3), 1.0, 0.5, 0.1, True, False, 1e-6, 1),
    (dict(steady_tol=1e-5, h_min=10.0), 1.0, 0.5, 0.1, True, False, 1e-6, 1),   # the steady stop wins over give-up
    (dict(steady_tol=0.0), 1.0, 0.5, 0.1, True, False, 0.0, 5),    # steady stop off
    (dict(t_end=2.0, h_min=0.2), 1.4, 0.5, 0.5, True, False, 3.0, 0),    # a last sliver below h_min lands on t_end: no give-up
    (dict(t_end=2.0, h_min=0.2), 1.9, 0.5, 30.0, True, False, 3.0, 0),   # ... but a step that h_min refuses anyway gives up
]


@pytest.fixture(scope="module")
def rule_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("time_rule")
    src = d / "rule.cpp"
    src.write_text(DRIVER)
    exe = d / "rule"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "gmpnp_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True)
    return str(exe)


def test_host_rule_against_its_mirrors(rule_exe):
    from gmpnp_amd import timestep
    lines, want, py = [], [], []
    for over, t, h, err, hist, failed, rate, run in RULE_CASES:
        p = dict(DEFAULT, **over)
        lines.append(" ".join(repr(float(p[k])) for k in ("safety", "min_factor", "max_factor", "fail_factor", "h_min", "h_max", "t_end", "steady_tol"))
                     + " %d %r %r %r %d %d %r %d" % (p["steady_steps"], t, h, err, hist, failed, rate, run))
        want.append(T.next_time_step(T.Policy(**p), t, h, err, hist, failed, rate, run))
        d = timestep.next_time_step(timestep.TimeStepPolicy(**p), t, h, err, hist, failed, rate, run)
        py.append((d.accept, d.reason, d.t_next, d.h_next, d.stop_end, d.stop_steady, d.give_up, d.steady_run))
    out = subprocess.run([rule_exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert out[-1] == "1 0"   # time_step_valid
    for k, (line, w, q) in enumerate(zip(out, want, py)):
        g = line.split()
        got = (bool(int(g[0])), int(g[1]), float(g[2]), float(g[3]), bool(int(g[4])), bool(int(g[5])), bool(int(g[6])), int(g[7]))
        assert got == w, (k, RULE_CASES[k], got, w)          # bit for bit: the same IEEE operations in the same order
        assert tuple(q) == w, (k, RULE_CASES[k], q, w)
    # what the table is meant to hit
    acc = [w[0] for w in want]
    assert acc[:9] == [True, True, True, True, True, False, False, False, True]
    assert want[1][3] == 4.0 and want[3][3] == 2.0 and want[7][3] == 0.1 and want[9][3] == 0.125 and want[9][1] == 2 and want[10][1] == 3
    assert want[12][3] == 0.7 and want[13][3] == 0.1
    assert want[14][3] == 0.5 and want[15][3] == 0.5 and want[16][3] < 0.5 and want[17][3] == 0.5
    assert want[18][4] and want[18][2] == 2.0 and want[19][4] and want[19][2] == 2.0 and not want[20][4]
    assert want[21][6] and want[22][6] and not want[23][6]
    assert [w[7] for w in want[24:29]] == [1, 2, 0, 1, 2] and [w[5] for w in want[24:31]] == [False, True, False, False, False, True, False]
    assert not want[29][6]
    assert want[31][0] and abs(want[31][3] - 0.1) < 1e-12 and not want[31][6] and not want[31][4]
    assert not want[32][0] and want[32][6]


# ---- the reference loop on the 1 um mesh --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cation,voltage", sorted(CASES))
def test_reference_loop_attempt_log(cation, voltage):
    ep, base, _ = reference_runs(cation, voltage)
    pin = PINNED[(cation, voltage)]
    dt = ep.dts[0]
    for r in base.log:
        print("t/dt %.5g h/dt %.5g %s err %.6g rate %.3g newton %d max S %.3f" % (r["t"] / dt, r["h"] / dt, "AFR"[0 if r["accepted"] else (1 if r["reason"] == 2 else 2)],
                                                                           r["err"], r["rate"], r["newton"], r["max_S"]))
    assert len(base.log) == pin["attempts"] and letters(base) == pin["sequence"] and base.stop_reason == pin["stop"]
    assert all(r["max_S"] < 1.0 for r in base.log if r["accepted"])   # every accepted state is admissible
    assert all(r["newton"] == 25 for r in base.log if r["reason"] == 2)
    if "newton" in pin:
        assert [r["newton"] for r in base.log] == pin["newton"]
    if cation == "K":
        rej = [r["err"] for r in base.log if not r["accepted"]]
        assert len(rej) == 4 and rej[0] > rej[1] > rej[2] > 1.0 and rej[3] > 1.0   # 17.8, 2.29, 1.13 at t = dt, 1.68 one step later
        acc = [r for r in base.log if r["accepted"]]
        assert acc[-1]["rate"] < 1e-5 and acc[-2]["rate"] < 1e-5 and acc[-3]["rate"] >= 1e-5
        assert acc[-1]["h"] > 100 * dt > acc[1]["h"]          # the step grows from a fraction of the reference step to hundreds
        assert base.times[-1] > 100 * dt                      # ... and the run covers more than the 100-step dry run
    else:
        f = [r["h"] / dt for r in base.log if r["reason"] == 2]
        assert f == [1.0, 0.25] and base.log[2]["h"] / dt == 0.0625 and 0.27 < base.log[2]["max_S"] < 0.29


@pytest.mark.parametrize("cation,voltage", sorted(CASES))
def test_decision_margins(cation, voltage):
    """Input condition of the GPU comparison: a 1e-8 relative perturbation of every accepted state (the tolerance the project states
    for Newton iterates) changes err by s_err at most, and every decision keeps 100 s_err between err and 1."""
    _, base, pert = reference_runs(cation, voltage)
    s_err, s_u = T.sensitivity(base, pert)
    margin = T.decision_margin(base.log)
    print("%s %g: s_err %.3e  s_u %.3e  min |err - 1| %.3e" % (cation, voltage, s_err, s_u, margin))
    assert s_err > 0.0 and s_u > 0.0
    assert margin > 100.0 * s_err


def test_the_residual_floor_lies_above_1e_minus_10():
    """Why NEWTON's absolute tolerance is 1e-6: with relative 1e-9 / absolute 1e-10 the first solve of K+ at -2.5 (from u = 0, a large
    first residual) converges, and the second one, started at u = u_n, runs to the iteration cap on a residual that has stopped at
    its rounding floor, below 1e-8 and above both 1e-10 and 1e-9 of its start; with 1e-6 it converges in 4 iterations."""
    import step_limit_reference as R
    _, _, prob = _edl(L_n=1e-6, cation="K", voltage_multiplier=-2.5)
    u0, un = R.first_step_state(prob)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        u1, st1 = R.newton_loop(prob, u0, un, maximum_iterations=25, relative_tolerance=1e-9, absolute_tolerance=1e-10)
        _, st2 = R.newton_loop(prob, u1, u1, maximum_iterations=25, relative_tolerance=1e-9, absolute_tolerance=1e-10)
        _, its, ok = T.newton(prob, u1, u1, **NEWTON)
    assert st1.converged and st1.iterations == 6
    floor = st2.residuals[5:]
    print("second solve: start %.3g, floor %.3g ... %.3g" % (st2.residuals[0], min(floor), max(floor)))
    assert not st2.converged and st2.iterations == 25
    assert 1e-10 < min(floor) and max(floor) < 1e-8 and min(floor) > 1e-9 * st2.residuals[0]
    assert ok and its == 4


def test_ensembles_refuse_adaptive_members():
    """Before anything touches the device (no GPU here)."""
    from gmpnp_amd.edl_ensemble import EDLEnsemble
    from gmpnp_amd.pore_ensemble import PoreEnsemble
    with pytest.raises(ValueError, match="adaptive_dt"):
        EDLEnsemble([dict(voltage_multiplier=-1.0), dict(voltage_multiplier=-2.0, adaptive_dt=True)])
    with pytest.raises(ValueError, match="adaptive_dt"):
        PoreEnsemble([dict(concentration_elec=0.5, L=10e-9, R=5e-9, adaptive_dt=True)])
