"""Second-order adaptive time stepping on the CPU: the NumPy estimator of variable-step BDF2
(tests/time_order_reference.py) against closed forms, the host rule and the coefficient functions of the library
(gmpnp_host_rules.h, compiled with the host compiler alone) against the NumPy mirror and the Python statements the drivers run
(gmpnp_amd/timestep.py), the observed order of the fixed-step marches, work against accuracy of the adaptive loops, and the
reference loops whose attempt logs the GPU tests compare with (tests/test_gpu_time_order.py), pinned with their decision margins.

Newton tolerances of the adaptive loops: tests/test_time_step_reference.py (relative 1e-9, absolute 1e-6, and why not 1e-10)."""
import math
import os
import subprocess
import warnings

import numpy as np
import pytest

import time_order_reference as R
import time_step_reference as T
from conftest import ROOT, _edl

NEWTON = dict(maximum_iterations=25, relative_tolerance=1e-9, absolute_tolerance=1e-6)
TIGHT = dict(maximum_iterations=25, relative_tolerance=1e-11, absolute_tolerance=1e-7)   # the observed-order marches
DT_ATOL = 1e-4
# (cation, voltage) -> the adaptive loop's arguments.  Cs+ at -10: the case of 5e, twice its attempts.  K+ at -2.5 with dt_rtol 1e-2
# to the steady stop takes 43 attempts and does NOT meet the margin condition of test_decision_margins (its near-steady tail
# amplifies the 1e-8 perturbation: s_err 3.1e-3 against a margin of 0.069); pinned is its longest prefix that does, 17 attempts
# (s_err 6.2e-4; with an 18th attempt 1.1e-3).
CASES = {("Cs", -10.0): dict(dt_rtol=1e-2, steady_tol=0.0, attempts=24), ("K", -2.5): dict(dt_rtol=1e-2, steady_tol=1e-5, attempts=17)}
PINNED = {
    ("Cs", -10.0): dict(sequence="FFARRRAAAAAAAAAAAARARAAA", orders=[1] * 7 + [2] * 17,
                        newton=[25, 25, 6, 4, 4, 3, 3, 3, 3, 3, 4, 4, 4, 5, 5, 6, 6, 5, 5, 5, 4, 4, 4, 4]),
    ("K", -2.5): dict(sequence="ARRRAAARRAAAAAAAA", orders=[1] * 5 + [2] * 12, newton=[6, 4] + [3] * 12 + [2] * 3),
}
PORE_ATTEMPTS = 8   # the 259-vertex cylinder: 5 attempts at order 1 (A R R R A), then three at order 2 (A R R)
PORE_PINNED = dict(sequence="ARRRAARR", orders=[1] * 5 + [2] * 3, newton=[14, 9, 9, 8, 7, 7, 7, 6])


def letters(res):
    return "".join("A" if r["accepted"] else ("F" if r["reason"] == 2 else "R") for r in res.log)


def run_case(cation, voltage, perturb=0.0):
    c = CASES[(cation, voltage)]
    ep, _, prob = _edl(L_n=1e-6, cation=cation, voltage_multiplier=voltage)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = R.adaptive_loop(prob, T.Policy(steady_tol=c["steady_tol"]), c["dt_rtol"], DT_ATOL, ep.dts[0], lambda h: 1.0 / (h * ep.L_D),
                              c["attempts"], order=2, perturb=perturb, **NEWTON)
    return ep, res


_runs = {}


def reference_runs(cation, voltage):
    """(ep, plain run, run with every accepted state perturbed by 1e-8 relative), computed once and shared (tests/
    test_gpu_time_order.py imports this)."""
    key = (cation, voltage)
    if key not in _runs:
        ep, base = run_case(cation, voltage)
        _, pert = run_case(cation, voltage, perturb=1e-8)
        _runs[key] = (ep, base, pert)
    return _runs[key]


def pore_reference(perturb):
    """The order-2 reference loop with the Sechenov glue on 5e's generated 259-vertex cylinder (tests/test_gpu_time_step.py
    small_pore): PORE_ATTEMPTS attempts from 10 reference steps, omega 0.9."""
    import test_gpu_time_step as G
    from gmpnp_amd.problem import pore_dirichlet
    key = ("pore", perturb)
    if key not in _runs:
        pp, bnd, prob = G.small_pore()

        def glue(p, u2d):
            p.bc_dofs, p.bc_vals = pore_dirichlet(pp, bnd, G.sechenov(pp, u2d))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _runs[key] = R.adaptive_loop(prob, T.Policy(), 1e-2, DT_ATOL, 10.0 * pp.dt, lambda h: 1.0 / h, PORE_ATTEMPTS, order=2, omega=0.9,
                                         maximum_iterations=50, relative_tolerance=1e-9, absolute_tolerance=1e-6, perturb=perturb, on_accept=glue)
    return _runs[key]


_order = {}


def order_start_state():
    """(ep, problem, the state after 64 backward Euler reference steps) of K+ at -2.5 on the 1 um mesh: where the fixed-step marches
    of the observed-order tests start (shared with tests/test_gpu_time_order.py)."""
    if "start" not in _order:
        import dataclasses
        ep, _, prob = _edl(L_n=1e-6, cation="K", voltage_multiplier=-2.5)
        nv, nf = prob.coords.shape[0], prob.nf
        u, un = np.zeros(prob.ndof), np.tile(np.r_[np.ones(nf - 1), 0.0], nv)
        prob.model = dataclasses.replace(prob.model, inv_dt=1.0 / (ep.dts[0] * ep.L_D))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for _ in range(64):
                u, _, ok = T.newton(prob, u, un, **TIGHT)
                assert ok
                un = u.copy()
        _order["start"] = (ep, prob, u)
    return _order["start"]


def refinement_ratios(march):
    """``march(m)`` = the end state of 64 / m steps of m reference steps: the two ratios of the successive max-norm differences."""
    ends = [march(m) for m in (8, 4, 2, 1)]
    d = [float(np.abs(ends[i] - ends[i + 1]).max()) for i in range(3)]
    return d[0] / d[1], d[1] / d[2], d


# ---- the estimator against closed forms ----------------------------------------------------------------------------------------------
def cubic_states(steps, nv=23, nf=7, seed=7, g=1.0):
    """(u, u_n, u_nm1, u_nm2) for u(t) = a + b t + c t^2 + g t^3 per dof at four times with the steps (h, h1, h2): the history exact,
    u the BDF2 step of u' = b + 2 c t + 3 g t^2 from it."""
    h, h1, h2 = steps
    rng = np.random.default_rng(seed)
    a, b, c = rng.uniform(0.5, 1.5, (nv, nf)), rng.standard_normal((nv, nf)), rng.standard_normal((nv, nf))
    f = lambda t: a + b * t + c * t * t + g * t ** 3
    t2 = 0.4
    t1, t0, t3 = t2 - h1, t2 - h1 - h2, t2 + h
    om = h / h1
    u = R.history_vector(f(t2), f(t1), om) + (h / R.alpha0(om)) * (b + 2.0 * c * t3 + 3.0 * g * t3 * t3)
    return u, f(t2), f(t1), f(t0)


@pytest.mark.parametrize("steps,value", [((1.0, 1.0, 1.0), 4.0 / 3.0), ((0.7, 1.3, 0.4), 0.7259259259259259)])
def test_cubic_in_time_gives_the_local_error_of_bdf2(steps, value):
    """u''' / 6 = 1: d = h^2 (h + h1)(1 + omega)/(1 + 2 omega) at every dof, to 1e-13 (weights 1: rtol 0, atol 1)."""
    h, h1, h2 = steps
    om = h / h1
    want = h * h * (h + h1) * (1.0 + om) / (1.0 + 2.0 * om)
    assert abs(want - value) <= 1e-13
    u, un, unm1, unm2 = cubic_states(steps)
    e = R.time_error2(u, un, unm1, unm2, h, h1, h2, 0.0, 1.0, np.ones(u.shape, dtype=bool))
    assert e["has_history"] and not e["nonfinite"]
    print(steps, e["err_field"] - want)
    assert np.abs(e["err_field"] - want).max() <= 1e-13 and abs(e["err"] - want) <= 1e-13
    rate = np.sqrt((((u - un) / h) ** 2).mean(axis=0))
    assert np.abs(e["rate_field"] - rate).max() <= 1e-14 * rate.max()


def test_quadratic_in_time_gives_zero():
    steps = (0.7, 1.3, 0.4)
    u, un, unm1, unm2 = cubic_states(steps, g=0.0)
    e = R.time_error2(u, un, unm1, unm2, *steps, 1e-2, 1e-4, np.ones(u.shape, dtype=bool))
    assert e["has_history"] and e["err"] <= 1e-11   # (rounding of the predictor over w >= 1e-4)


def test_dirichlet_dofs_are_ignored_and_a_field_without_free_dofs_reports_zero():
    steps = (0.7, 1.3, 0.4)
    u, un, unm1, unm2 = cubic_states(steps)
    free = np.ones(u.shape, dtype=bool)
    free[[0, 5, 22], 6] = False
    free[:, 2] = False
    base = R.time_error2(u, un, unm1, unm2, *steps, 1e-2, 1e-4, free)
    u2 = u.copy()
    u2[[0, 5, 22], 6] += 1e6
    u2[:, 2] -= 1e6
    e = R.time_error2(u2, un, unm1, unm2, *steps, 1e-2, 1e-4, free)
    assert np.array_equal(e["err_field"], base["err_field"]) and np.array_equal(e["rate_field"], base["rate_field"])
    assert e["worst_dof"] == base["worst_dof"] and e["err_field"][2] == 0.0 and e["rate_field"][2] == 0.0 and e["err"] > 0.0


def test_no_history_and_nonfinite():
    steps = (0.7, 1.3, 0.4)
    u, un, unm1, unm2 = cubic_states(steps)
    free = np.ones(u.shape, dtype=bool)
    for e in (R.time_error2(u, un, unm1, None, *steps, 1e-2, 1e-4, free), R.time_error2(u, un, None, None, *steps, 1e-2, 1e-4, free),
              R.time_error2(u, un, unm1, unm2, 0.7, 1.3, 0.0, 1e-2, 1e-4, free), R.time_error2(u, un, unm1, unm2, 0.7, 0.0, 0.4, 1e-2, 1e-4, free)):
        assert not e["has_history"] and e["err"] == 0.0 and e["rate"] > 0.0 and e["worst_dof"] == -1
    u[3, 1] = np.nan
    e = R.time_error2(u, un, unm1, unm2, *steps, 1e-2, 1e-4, free)
    assert e["nonfinite"] and math.isnan(e["err"]) and np.all(np.isnan(e["err_field"]))


# ---- the host rule and the coefficient functions: C++ (g++ alone), the NumPy mirror, the drivers' Python statements ----------------
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
    in >> tok;
    if (tok == "coef") {
      const double h = num(), h1 = num(), h2 = num(), om = h / h1;
      const std::pair<double, double> ab = bdf2_history_weights(om);
      const TimePredictor w = bdf2_predictor_weights(h, h1, h2);
      printf("%.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", bdf2_alpha0(om), ab.first, ab.second, w.wn, w.wm1, w.wm2, bdf2_error_share(h, h1, h2));
      continue;
    }
    TimeStepPolicy p;
    p.safety = num(); p.min_factor = num(); p.max_factor = num(); p.fail_factor = num(); p.h_min = num(); p.h_max = num();
    p.t_end = num(); p.steady_tol = num(); p.steady_steps = (int)num();
    const double t = num(), h = num(), err = num(); const bool hist = num() != 0.0, failed = num() != 0.0;
    const double rate = num(); const int run = (int)num(); const int order = (int)num();
    const TimeStepDecision d = next_time_step(p, t, h, err, hist, failed, rate, run, order);
    printf("%d %d %.17g %.17g %d %d %d %d\n", (int)d.accept, d.reason, d.t_next, d.h_next, (int)d.stop_end, (int)d.stop_steady, (int)d.give_up, d.steady_run);
  }
  printf("%d %d\n", (int)(time_ratio_valid(0.3) && time_ratio_valid(2.0)),
         (int)(time_ratio_valid(0.0) || time_ratio_valid(-1.0) || time_ratio_valid(NAN) || time_ratio_valid(INFINITY)));
  return 0;
}
"""

DEFAULT = dict(safety=0.9, min_factor=0.2, max_factor=4.0, fail_factor=0.25, h_min=0.0, h_max=math.inf, t_end=math.inf, steady_tol=0.0,
               steady_steps=2)
# (policy overrides, t, h, err, has_history, newton_failed, rate, steady_run), each run at order 1 and at order 2
RULE_CASES = [
    ({}, 0.0, 1.0, 0.0, False, False, 3.0, 0),                     # no history: accept, factor 1
    ({}, 1.0, 1.0, 0.0, True, False, 3.0, 0),                      # err = 0 with history: the growth clamp (4; order 2: 2)
    ({}, 1.0, 0.5, 0.125, True, False, 3.0, 0),                    # accept; order 2: factor 0.9 * 2 = 1.8
    ({}, 1.0, 0.5, 1e-6, True, False, 3.0, 0),                     # accept, clamped (order 2: 0.9 * 100 -> 2)
    (dict(max_factor=1.5), 1.0, 0.5, 1e-6, True, False, 3.0, 0),   # a max_factor below 2 stays the clamp at order 2
    ({}, 1.0, 0.5, 1.0, True, False, 3.0, 0),                      # err = 1 exactly: accepted
    ({}, 1.0, 0.5, 1.0000001, True, False, 3.0, 0),                # just above: rejected
    ({}, 1.0, 0.5, 8.0, True, False, 3.0, 0),                      # rejected; order 2: factor 0.45
    ({}, 1.0, 0.5, 1000.0, True, False, 3.0, 0),                   # rejected, clamped to min_factor at both orders
    ({}, 1.0, 0.5, 0.95, True, False, 3.0, 0),                     # accepted with a factor below 1
    ({}, 1.0, 0.5, 0.3, True, True, 3.0, 1),                       # Newton failed: fail_factor, the steady counter stays
    ({}, 1.0, 0.5, math.nan, True, False, 3.0, 1),                 # NaN err: reject, fail_factor
    ({}, 1.0, 0.5, math.nan, False, False, math.nan, 0),           # NaN err without history
    (dict(h_max=0.7), 1.0, 0.5, 0.01, True, False, 3.0, 0),        # h_max clamp
    (dict(t_end=2.0), 1.0, 0.5, 0.729, True, False, 3.0, 0),       # order 2: factor 1 exactly, next step lands on t_end (left = h_next)
    (dict(t_end=2.0), 1.0, 0.5, 0.05, True, False, 3.0, 0),        # left 0.5 < h_next
    (dict(t_end=2.0), 1.5, 0.5, 0.5, True, False, 3.0, 0),         # lands on t_end: stop_end, t_next = t_end exactly
    (dict(t_end=2.0), 1.7, 0.3, 0.5, True, False, 3.0, 0),         # ... through rounding (1.7 + 0.3)
    (dict(t_end=2.0, h_min=0.2), 1.5, 0.5, 900.0, True, False, 3.0, 0),   # h_min give-up after an error rejection
    (dict(h_min=0.2), 1.0, 0.5, 0.1, True, True, 3.0, 0),          # h_min give-up after a Newton failure
    (dict(t_end=2.0, h_min=0.2), 1.4, 0.5, 0.5, True, False, 3.0, 0),    # a last sliver below h_min lands on t_end: no give-up
    (dict(t_end=2.0, h_min=0.2), 1.9, 0.5, 300.0, True, False, 3.0, 0),  # ... but a step that h_min refuses anyway gives up
    (dict(steady_tol=1e-5), 1.0, 0.5, 0.1, True, False, 1e-6, 1),  # 1 -> 2: stop_steady
    (dict(steady_tol=1e-5, h_min=10.0), 1.0, 0.5, 0.1, True, False, 1e-6, 1),   # the steady stop wins over give-up
] + [({}, 1.0, 0.5, e, True, False, 3.0, 0) for e in (3e-4, 0.0123, 0.2, 0.4567, 0.81, 1.7, 2.9, 33.0)]   # cube roots that do not come out even
COEF_CASES = [(1.0, 1.0, 1.0), (0.7, 1.3, 0.4), (0.11, 0.07, 0.05), (3.0e-3, 1.7e-3, 2.9e-3)]


@pytest.fixture(scope="module")
def rule_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("time_order_rule")
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
        for order in (1, 2):
            p = dict(DEFAULT, **over)
            lines.append("rule " + " ".join(repr(float(p[k])) for k in ("safety", "min_factor", "max_factor", "fail_factor", "h_min", "h_max", "t_end", "steady_tol"))
                         + " %d %r %r %r %d %d %r %d %d" % (p["steady_steps"], t, h, err, hist, failed, rate, run, order))
            want.append(R.next_time_step(T.Policy(**p), t, h, err, hist, failed, rate, run, order))
            d = timestep.next_time_step(timestep.TimeStepPolicy(**p), t, h, err, hist, failed, rate, run, order=order)
            py.append((d.accept, d.reason, d.t_next, d.h_next, d.stop_end, d.stop_steady, d.give_up, d.steady_run))
            if order == 1:   # order 1 IS the rule of 5e, in all three statements
                d1 = timestep.next_time_step(timestep.TimeStepPolicy(**p), t, h, err, hist, failed, rate, run)
                assert (d1.accept, d1.reason, d1.t_next, d1.h_next, d1.stop_end, d1.stop_steady, d1.give_up, d1.steady_run) == py[-1]
                assert want[-1] == T.next_time_step(T.Policy(**p), t, h, err, hist, failed, rate, run)
    out = subprocess.run([rule_exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert out[-1] == "1 0"   # time_ratio_valid
    assert len(out) == len(lines) + 1
    for k, (line, w, q) in enumerate(zip(out, want, py)):
        g = line.split()
        got = (bool(int(g[0])), int(g[1]), float(g[2]), float(g[3]), bool(int(g[4])), bool(int(g[5])), bool(int(g[6])), int(g[7]))
        assert got == tuple(q), (k, RULE_CASES[k // 2], got, q)   # bit for bit: the same IEEE operations in the same order, one cbrt
        if k % 2 == 0:
            assert got == w, (k, RULE_CASES[k // 2], got, w)      # order 1: the NumPy mirror too
        else:   # order 2: NumPy's cube root is not the C library's (0.125: 0.5 against 0.49999999999999994); each is within an ulp
            # of the root and h_next = h * safety / root carries that: 2 ulp.  Every other entry is exact.
            assert got[:3] + got[4:] == w[:3] + w[4:] and abs(got[3] - w[3]) <= 2.0 * np.spacing(abs(w[3])), (k, RULE_CASES[k // 2], got, w)
    # what the table is meant to hit, at order 2 (odd rows)
    w2 = want[1::2]
    assert w2[1][3] == 2.0 and abs(w2[2][3] - 0.9) < 1e-15 and w2[3][3] == 1.0 and w2[4][3] == 0.75
    assert w2[5][0] and not w2[6][0] and abs(w2[7][3] - 0.225) < 1e-15 and w2[8][3] == 0.1
    assert w2[10][1] == 2 and w2[10][3] == 0.125 and w2[11][1] == 3 and w2[13][3] == 0.7
    assert w2[14][3] == 0.5 and w2[15][3] == 0.5 and w2[16][4] and w2[16][2] == 2.0 and w2[17][4] and w2[17][2] == 2.0
    assert w2[18][6] and w2[19][6] and not w2[20][6] and abs(w2[20][3] - 0.1) < 1e-12 and w2[21][6]
    assert w2[22][5] and w2[23][5] and not w2[23][6]
    assert want[2][3] == 4.0 and want[3][3] == 2.0   # err = 0 with history: max_factor at order 1, the growth clamp 2 at order 2


def test_coefficient_functions(rule_exe):
    """alpha0, the weights of u*, the predictor's weights and kappa: pinned at omega = 1 (3/2, 4/3, 1/3, (3, -3, 1), 2/11) and at
    unequal triples, the C++ functions against the Python statements and the NumPy mirror bit for bit."""
    from gmpnp_amd import timestep
    lines = ["coef %r %r %r" % c for c in COEF_CASES]
    out = subprocess.run([rule_exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    for (h, h1, h2), line in zip(COEF_CASES, out):
        got = tuple(float(x) for x in line.split())
        om = h / h1
        py = (timestep.bdf2_alpha0(om),) + timestep.bdf2_history_weights(om) + timestep.bdf2_predictor_weights(h, h1, h2) + (timestep.bdf2_error_share(h, h1, h2),)
        ref = (R.alpha0(om),) + R.history_weights(om) + R.predictor_weights(h, h1, h2) + (R.error_share(h, h1, h2),)
        assert got == py == tuple(float(x) for x in ref), ((h, h1, h2), got, py, ref)
    one = tuple(float(x) for x in out[0].split())
    assert one[0] == 1.5 and one[1] == 4.0 / 3.0 and one[2] == 1.0 / 3.0 and one[3:6] == (3.0, -3.0, 1.0) and abs(one[6] - 2.0 / 11.0) <= 1e-16
    # the unequal triple (0.7, 1.3, 0.4) in exact rational arithmetic
    from fractions import Fraction as F
    h, h1, h2 = F(7, 10), F(13, 10), F(4, 10)
    om = h / h1
    a0 = (1 + 2 * om) / (1 + om)
    exact = (a0, (1 + om) ** 2 / (1 + 2 * om), om ** 2 / (1 + 2 * om), (h + h1 + h2) * (h + h1) / ((h1 + h2) * h1), -(h + h1 + h2) * h / (h1 * h2),
             (h + h1) * h / (h2 * (h1 + h2)), (h / a0) / (h + h1 + h2 + h / a0))
    two = tuple(float(x) for x in out[1].split())
    for g, e in zip(two, exact):
        assert abs(g - float(e)) <= 8e-16 * abs(float(e)), (g, float(e))
    assert abs(sum(two[3:6]) - 1.0) <= 1e-14   # the predictor reproduces constants


# ---- observed order -----------------------------------------------------------------------------------------------------------------
def test_observed_order_of_the_fixed_step_marches():
    """K+ at -2.5 on the 1 um mesh, from the state at t = 64 reference steps: 64 reference steps in steps of 8, 4, 2 and 1.  The
    successive max-norm differences fall by 2^order: above 3 at order 2, below 2.5 at order 1 (theory 4 and 2; 3 lies between).
    Measured: 4.69 and 4.21 against 1.92 and 1.96."""
    ep, prob, u0 = order_start_state()
    dt = ep.dts[0]
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for order in (2, 1):
            out[order] = refinement_ratios(lambda m: R.fixed_step_march(prob, u0, m * dt, 64 // m, lambda h: 1.0 / (h * ep.L_D), order, **TIGHT)[-1])
            print("order %d: differences %s ratios %.3f %.3f" % (order, out[order][2], out[order][0], out[order][1]))
    assert out[2][0] > 3.0 and out[2][1] > 3.0
    assert out[1][0] < 2.5 and out[1][1] < 2.5


# ---- work against accuracy ------------------------------------------------------------------------------------------------------------
def test_order_2_takes_fewer_attempts_for_a_smaller_error():
    """K+ at -2.5 to t_end = 200 reference steps with dt_rtol 2e-3: against the order-2 run with dt_rtol 1e-4 / dt_atol 1e-6 (136
    attempts), order 2 takes fewer attempts than order 1 and ends closer.  Measured: 51 attempts (122 Newton iterations, error
    0.0064) against 85 (193, 0.0150)."""
    res = {}
    for key, (order, rtol, atol) in {"tight": (2, 1e-4, 1e-6), 1: (1, 2e-3, DT_ATOL), 2: (2, 2e-3, DT_ATOL)}.items():
        ep, _, prob = _edl(L_n=1e-6, cation="K", voltage_multiplier=-2.5)
        dt = ep.dts[0]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res[key] = R.adaptive_loop(prob, T.Policy(t_end=200 * dt), rtol, atol, dt, lambda h: 1.0 / (h * ep.L_D), 2000, order=order, **NEWTON)
        assert res[key].stop_reason == "t_end" and abs(res[key].times[-1] - 200 * dt) <= 1e-12 * 200 * dt
    err = {k: float(np.abs(res[k].u - res["tight"].u).max()) for k in (1, 2)}
    for k in (1, 2):
        print("order %d: %d attempts, %d Newton iterations, max error %.4f" % (k, len(res[k].log), sum(r["newton"] for r in res[k].log), err[k]))
    assert len(res[2].log) < len(res[1].log)
    assert err[2] < err[1]
    assert all(r["order"] == 1 for r in res[1].log) and sum(r["order"] == 2 for r in res[2].log) >= len(res[2].log) - 8


# ---- the pinned reference loops -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cation,voltage", sorted(CASES))
def test_reference_loop_attempt_log(cation, voltage):
    ep, base, _ = reference_runs(cation, voltage)
    pin = PINNED[(cation, voltage)]
    dt = ep.dts[0]
    for r in base.log:
        print("t/dt %.5g h/dt %.5g %s order %d err %.6g rate %.3g newton %d max S %.3f" % (
            r["t"] / dt, r["h"] / dt, "AFR"[0 if r["accepted"] else (1 if r["reason"] == 2 else 2)], r["order"], r["err"], r["rate"], r["newton"], r["max_S"]))
    assert letters(base) == pin["sequence"] and base.stop_reason is None
    assert [r["order"] for r in base.log] == pin["orders"]
    assert [r["newton"] for r in base.log] == pin["newton"]
    assert all(r["max_S"] < 1.0 for r in base.log if r["accepted"])   # every accepted state is admissible
    # the start-up: the first accepted step has no estimate, the second one backward Euler's, BDF2 from the third on
    acc = [r for r in base.log if r["accepted"]]
    assert acc[0]["err"] == 0.0 and acc[1]["order"] == 1 and acc[1]["err"] > 0.0 and all(r["order"] == 2 for r in acc[2:])
    # a rejection keeps the history: the attempt behind a rejected order-2 attempt is an order-2 attempt again
    rej2 = [k for k, r in enumerate(base.log[:-1]) if r["order"] == 2 and not r["accepted"]]
    assert rej2 and all(base.log[k + 1]["order"] == 2 for k in rej2)
    # zero stability: an accepted order-2 step is followed by a step of at most twice its length
    for k, r in enumerate(base.log[:-1]):
        if r["accepted"] and r["order"] == 2:
            assert base.log[k + 1]["h"] <= 2.0 * r["h"]


@pytest.mark.parametrize("cation,voltage", sorted(CASES))
def test_decision_margins(cation, voltage):
    """Input condition of the GPU comparison, as in 5e: a 1e-8 relative perturbation of every accepted state changes err by s_err at
    most, and every decision keeps 100 s_err between err and 1.  Measured: Cs+ s_err 4.1e-5, s_u 3.1e-6, margin 0.0215; the K+
    prefix s_err 6.2e-4, margin 0.0686."""
    _, base, pert = reference_runs(cation, voltage)
    s_err, s_u = T.sensitivity(base, pert)
    margin = T.decision_margin(base.log)
    print("%s %g: s_err %.3e  s_u %.3e  min |err - 1| %.3e" % (cation, voltage, s_err, s_u, margin))
    assert s_err > 0.0 and s_u > 0.0
    assert margin >= 100.0 * s_err


def test_pore_reference_loop():
    """3D, the generated 259-vertex cylinder: three order-2 attempts behind the start-up, under the same margin condition.
    Measured over 12 attempts: s_err 1.8e-7, s_u 7.7e-7."""
    base, pert = pore_reference(0.0), pore_reference(1e-8)
    print(letters(base), [r["newton"] for r in base.log], ["%.4g" % r["err"] for r in base.log])
    assert letters(base) == PORE_PINNED["sequence"] and [r["order"] for r in base.log] == PORE_PINNED["orders"]
    assert [r["newton"] for r in base.log] == PORE_PINNED["newton"]
    assert sum(r["order"] == 2 for r in base.log) >= 3
    s_err, s_u = T.sensitivity(base, pert)
    margin = T.decision_margin(base.log)
    print("pore (259 vertices): s_err %.3e  s_u %.3e  min |err - 1| %.3e" % (s_err, s_u, margin))
    assert s_err > 0.0 and s_u > 0.0 and margin >= 100.0 * s_err


# ---- ensembles ----------------------------------------------------------------------------------------------------------------------
def test_ensembles_refuse_order_2():
    """Before anything touches the device (no GPU here); the keyword itself is one of the adaptive-stepping keywords."""
    from gmpnp_amd import edl_sweep, sweep, timestep
    from gmpnp_amd.edl_ensemble import EDLEnsemble
    from gmpnp_amd.pore_ensemble import PoreEnsemble
    assert timestep.ADAPTIVE_KEYWORDS["dt_order"] == 1
    assert timestep.member_adaptive_keywords(2, dict(dt_order=1)) == [dict(dt_order=1), dict(dt_order=1)]
    assert timestep.member_adaptive_keywords(2, dict(dt_order=[1, 2])) == [dict(dt_order=1), dict(dt_order=2)]
    edl = [dict(voltage_multiplier=-1.0), dict(voltage_multiplier=-2.0)]
    pore = [dict(concentration_elec=0.5, L=10e-9, R=5e-9)]
    for make in (lambda: EDLEnsemble(edl, adaptive_dt=True, dt_order=2), lambda: EDLEnsemble(edl, adaptive_dt=True, dt_order=[1, 2]),
                 lambda: EDLEnsemble([dict(edl[0], dt_order=2)]), lambda: PoreEnsemble(pore, adaptive_dt=True, dt_order=2),
                 lambda: edl_sweep.run_sweep(edl, adaptive_dt=True, dt_order=2),
                 lambda: sweep.run_group(5, [-1.0], 3, adaptive_dt=True, dt_order=2),
                 lambda: sweep.main(["--ensemble", "--adaptive_dt", "--dt_order", "2"]),
                 lambda: edl_sweep.main(["--voltage_multiplier", "-1.0", "--adaptive_dt", "--dt_order", "2"])):
        with pytest.raises(ValueError, match="order 2"):
            make()
    with pytest.raises(ValueError, match="order"):
        timestep.AdaptiveStepper(None, timestep.TimeStepPolicy(), (1e-2, 1e-4), lambda h: 1.0 / h, 1.0, order=3)
    for mod in ("edl1d", "pore3d", "rxndiff1d", "rxnpore3d"):
        import importlib
        m = importlib.import_module("gmpnp_amd." + mod)
        assert m.build_parser().parse_args(["--adaptive_dt", "--dt_order", "2"]).dt_order == 2
        assert m.build_parser().parse_args([]).dt_order == 1
