"""The electrode tangent and the polarisation curve on the CPU: the closed forms of tests/tangent_reference.py
against differences of the reference's F, D and I_r and of steady states, the predictor's order, the continuation rule over scripted
systems, the host rule (g++ alone) against its Python statement (gmpnp_amd/polarisation.py), the ctypes image against the header, the
Python refusals and the command lines.  The case is K+ on the 1 um mesh, Stern BDM, the TAFEL parameters, the steady state at p_M = -5."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import kinetics_reference as K
import response_reference as R
import tangent_reference as T
from gmpnp_amd import polarisation as pol
from step_limit_reference import first_step_state
from test_kinetics_reference import TAFEL, _edl_k, first_step_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_M = -5.0
PARAMS = (0, 16, 17, 32, 33, 48)


@pytest.fixture(scope="module")
def steady():
    """(problem, steady state at p_M = -5), computed once and left unchanged."""
    ep, mesh = _edl_k()
    prob = first_step_problem(ep, mesh, P_M)
    u1, st = K.newton_loop(prob, *first_step_state(prob))
    assert st.converged
    u, _, ok = T.steady_state(prob, u1)
    assert ok
    u.setflags(write=False)
    return prob, u


@pytest.fixture(scope="module")
def tangents(steady):
    prob, u = steady
    return T.tangent(prob, u, PARAMS)


def rel(a, b):
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    scale = np.abs(b).max()
    return float(np.abs(a - b).max() / scale) if scale > 0.0 else float(np.abs(a).max())


@pytest.mark.parametrize("param", PARAMS)
def test_columns_and_explicit_derivatives_against_central_differences(steady, param):
    """c = dF/dtheta, dD/dtheta and dI_r/dtheta at fixed u against central differences of the reference's F, D and I_r in that
    parameter (step 1e-5: truncation ~1e-10 relative, rounding ~1e-11), below 1e-7 relative; an explicit part that is identically
    zero is compared absolutely."""
    prob, u = steady
    d = 1e-5
    fp, fm = T.with_parameter(prob, param, d), T.with_parameter(prob, param, -d)
    c = T.column(prob, u, param)
    eD, eI = T.explicit(prob, u, param)
    got = (rel((T.residual(fp, u) - T.residual(fm, u)) / (2 * d), c), rel((T.displacement(fp, u) - T.displacement(fm, u)) / (2 * d), eD),
           rel((T.currents(fp, u) - T.currents(fm, u)) / (2 * d), eI))
    print("param %d: c %.2e dD %.2e dI %.2e" % ((param,) + got))
    assert max(got) < 1e-7
    assert not c[np.asarray(prob.bc_dofs, dtype=np.int64)].any()
    # the same column at the first step's inv_dt: the parameters do not enter the time term
    inv_dt = float(prob.model.inv_dt)
    assert rel((T.residual(fp, u, u, inv_dt) - T.residual(fm, u, u, inv_dt)) / (2 * d), c) < 1e-7


def test_p_M_tangent_against_differences_of_two_steady_states(steady, tangents):
    """dD and dI_r of the p_M column against central differences of stern_displacement and the currents of two steady states at
    p_M -+ 1e-3, below 1e-6 relative (truncation O(delta^2); measured at most 2.6e-8)."""
    prob, u = steady
    _, dD, dI, _ = tangents
    d = 1e-3
    D, I = {}, {}
    for s in (+1, -1):
        q = R.with_potential(prob, P_M + s * d)
        us, _, ok = T.steady_state(q, u)
        assert ok
        D[s], I[s] = T.displacement(q, us), T.currents(q, us)
    eD, eI = rel((D[1] - D[-1]) / (2 * d), dD[0]), rel((I[1] - I[-1]) / (2 * d), dI[0])
    print("p_M against steady differences: dD %.2e dI %.2e" % (eD, eI))
    assert eD < 1e-6 and eI < 1e-6


def test_p_M_column_is_the_zero_frequency_response(steady):
    """At inv_dt = 0 the p_M tangent is response_reference.response(S, 0): x, C and dI_r (both refined in extended precision)."""
    prob, u = steady
    z, dD, dI, _ = T.tangent(prob, u, [0], how="refined")
    x, C, dIr = R.response(R.system(prob, u), 0.0)
    assert rel(z[0], np.asarray(x.real, dtype=np.float64)) < 1e-12 and abs(float(C.real) - dD[0]) < 1e-12 * abs(dD[0])
    assert rel(dI[0], np.asarray(dIr.real, dtype=np.float64)) < 1e-12 and float(np.abs(np.asarray(x.imag, dtype=np.float64)).max()) == 0.0


@pytest.mark.parametrize("param", (16, 48))
def test_a_further_parameter_against_differences_of_two_steady_states(steady, tangents, param):
    """ln k_0 and ln lam: dD and dI_r against differences of two steady states at theta -+ 3e-4, below 1e-6 relative (the truncation
    of the difference quotient is delta^2 / 6 times a ratio of derivatives of order one: ~2e-8) plus the quotient's own rounding, 16
    ulp of the differenced quantity over 2 delta.  That term matters for one entry only: D = -2.0e5 hardly depends on k_0 (dD/dln k_0
    = -1.1e-6), the two D differ by less than one ulp of D and their quotient carries no information, which the bound states; that
    entry rests on the explicit derivatives and the closed-form rows checked above."""
    prob, u = steady
    _, dD, dI, _ = tangents
    k, d = PARAMS.index(param), 3e-4
    D, I = {}, {}
    for s in (+1, -1):
        q = T.with_parameter(prob, param, s * d)
        us, _, ok = T.steady_state(q, u)
        assert ok
        D[s], I[s] = T.displacement(q, us), T.currents(q, us)
    fD, fI = (D[1] - D[-1]) / (2 * d), (I[1] - I[-1]) / (2 * d)
    ulp16 = 16 * np.finfo(float).eps / (2 * d)
    print("param %d against steady differences: dD %.3e (differences %.3e), dI %s (%s)" % (param, dD[k], fD, dI[k], fI))
    assert abs(fD - dD[k]) <= 1e-6 * abs(dD[k]) + ulp16 * abs(D[1])
    assert np.all(np.abs(fI - dI[k]) <= 1e-6 * np.abs(dI[k]).max() + ulp16 * np.abs(I[1]))


@pytest.mark.parametrize("p_M", (-5.0, -10.0))
def test_predictor_is_second_order(steady, p_M):
    """max |u(p + h) - (u + h z)| at h = -1 against h = -0.5: the ratio lies in 3.5 ... 4.6 (second order gives 4; measured 3.91
    and 4.21)."""
    prob, u = steady
    q = R.with_potential(prob, p_M)
    u0, _, ok = T.steady_state(q, u)
    assert ok
    z = T.tangent(q, u0, [0])[0][0]
    e = []
    for h in (-1.0, -0.5):
        uh, _, ok = T.steady_state(R.with_potential(q, p_M + h), u0 + h * z)
        assert ok
        e.append(float(np.abs(uh - (u0 + h * z)).max()))
    print("predictor error ratio at %g: %.3f" % (p_M, e[0] / e[1]))
    assert 3.5 < e[0] / e[1] < 4.6


def test_functionals_by_the_rule_are_the_closed_form_rows(steady, tangents):
    """``tangent_reference.functionals`` (the node terms the device forms) against the rows of response_reference applied to z."""
    prob, u = steady
    z, dD, dI, dp = tangents
    for k, param in enumerate(PARAMS):
        fD, fI, fp = T.functionals(prob, u, z[k], param)
        assert rel(fD, dD[k]) < 1e-12 and rel(fI, dI[k]) < 1e-12 and abs(fp - dp[k]) <= 1e-15 * max(abs(dp[k]), 1.0)


def test_reference_continuation_takes_no_halving(steady):
    """-5 to -10 in steps of -1 over the NumPy restatement: six points, one attempt each, no failed solve, every rate positive, and
    every point the steady state an independent solve finds at that potential."""
    prob, u = steady
    S = T.NumpySystem(prob, u)
    rec, sub, newt, stop = pol.run_continuation(S, P_M, -10.0, -1.0)
    assert stop == "v_end" and [r["p_M"] for r in rec] == [-5.0, -6.0, -7.0, -8.0, -9.0, -10.0]
    assert sub == [0, 1, 1, 1, 1, 1] and S.failed == 0 and all((r["currents"] > 0.0).all() for r in rec)
    print("reference continuation: Newton iterations per point", newt)
    q = R.with_potential(prob, -10.0)
    ui, _, ok = T.steady_state(q, rec[-2]["u"])
    assert ok and rel(rec[-1]["u"], ui) < 1e-9


# ---- the continuation rule over scripted systems ---------------------------------------------------------------------------------------
class Scripted:
    """A system whose solves succeed or fail by a script: entries True, False or "negative" (a converged solve with a negative rate)."""

    def __init__(self, script):
        self.script, self.log, self.p, self.kept_p = list(script), [], None, None

    def solve(self):
        what = self.script.pop(0) if self.script else True
        self.log.append(("solve", self.p, what))
        if what == "negative":
            return True, 3, np.array([1.0, -1e-3])
        return bool(what), 2 if what else 25, (np.array([1.0, 2.0]) if what else None)

    def point(self, p):
        return {"p_M": p}

    def predict(self, dp, predictor):
        self.log.append(("predict", dp, predictor))

    def set_potential(self, p):
        self.p = p

    def keep(self):
        self.kept_p = self.p
        self.log.append(("keep", self.p))

    def back(self, p):
        self.p = p
        self.log.append(("back", p))


def test_continuation_lands_on_the_grid_and_on_v_end():
    s = Scripted([])
    rec, sub, newt, stop = pol.run_continuation(s, -5.0, -7.5, -1.0)
    assert [r["p_M"] for r in rec] == [-5.0, -6.0, -7.0, -7.5] and sub == [0, 1, 1, 1] and newt == [2, 2, 2, 2] and stop == "v_end"
    assert [e[1] for e in s.log if e[0] == "predict"] == [-1.0, -1.0, -0.5]
    # a grid the floating-point sum misses: the points are the grid's own values, v_end exactly
    rec = pol.run_continuation(Scripted([]), 0.0, 0.35, 0.1)[0]
    assert [r["p_M"] for r in rec] == [0.0, 0.0 + 1 * 0.1, 0.0 + 2 * 0.1, 0.0 + 3 * 0.1, 0.35]
    # no curve at all
    rec, sub, newt, stop = pol.run_continuation(Scripted([]), -5.0, -5.0, -1.0)
    assert len(rec) == 1 and stop == "v_end"
    with pytest.raises(ValueError, match="polarisation"):
        pol.run_continuation(Scripted([]), -5.0, -10.0, 1.0)
    with pytest.raises(ValueError, match="polarisation"):
        pol.run_continuation(Scripted([]), -5.0, -10.0, 0.0)
    with pytest.raises(RuntimeError, match="steady stop"):
        pol.run_continuation(Scripted([False]), -5.0, -10.0, -1.0)


def test_continuation_halves_returns_and_tries_the_remainder():
    """First point, then: fail at -7 (from -5, step -2), succeed at -6 (half), succeed with the remainder -1 to -7."""
    s = Scripted([True, False, True, True])
    rec, sub, newt, stop = pol.run_continuation(s, -5.0, -7.0, -2.0)
    assert [r["p_M"] for r in rec] == [-5.0, -7.0] and sub == [0, 3] and newt == [2, 25 + 2 + 2] and stop == "v_end"
    assert [e for e in s.log if e[0] in ("back", "predict")] == [("predict", -2.0, True), ("back", -5.0), ("predict", -1.0, True), ("predict", -1.0, True)]
    assert [e[1] for e in s.log if e[0] == "solve"] == [None, -7.0, -6.0, -7.0]


def test_a_negative_rate_counts_as_a_failure():
    s = Scripted([True, "negative", True, True])
    rec, sub, newt, stop = pol.run_continuation(s, -5.0, -6.0, -1.0)
    assert [r["p_M"] for r in rec] == [-5.0, -6.0] and sub == [0, 3] and ("back", -5.0) in s.log and stop == "v_end"
    with pytest.raises(RuntimeError, match="steady stop"):
        pol.run_continuation(Scripted(["negative"]), -5.0, -6.0, -1.0)


def test_dp_min_ends_the_curve():
    s = Scripted([True, True] + [False] * 40)
    rec, sub, newt, stop = pol.run_continuation(s, -5.0, -8.0, -1.0)
    assert stop == "dp_min" and [r["p_M"] for r in rec] == [-5.0, -6.0]
    steps = [e[1] for e in s.log if e[0] == "predict"][1:]
    assert steps == [-1.0 / 2 ** k for k in range(11)]            # 2^-10 = |v_step| / 1024 is still tried; 2^-11 is not
    assert s.p == -6.0                                            # the handle is back at the last converged point


# ---- the host rule against its Python statement -------------------------------------------------------------------------------------
DRIVER = r"""
#include <cstdio>
#include <cstring>
#include "gmpnp_host_rules.h"
using namespace gmpnp;
int main() {
  char cmd[32];
  while (std::scanf("%31s", cmd) == 1) {
    if (!std::strcmp(cmd, "param")) {
      int p, nr; if (std::scanf("%d %d", &p, &nr) != 2) return 1;
      std::printf("%d %d %d %d\n", tangent_param_kind(p), tangent_param_reaction(p), (int)tangent_param_valid(p, nr), (int)tangent_count_valid(p));
    } else if (!std::strcmp(cmd, "terms")) {
      int p, r; double rate, d_p, eta, slope, term, w, d_u, z_u, z_p;
      if (std::scanf("%d %d %lf %lf %lf %lf %lf %lf %lf %lf %lf", &p, &r, &rate, &d_p, &eta, &slope, &term, &w, &d_u, &z_u, &z_p) != 11) return 1;
      const double e = tangent_rate_explicit(p, r, rate, d_p, eta);
      std::printf("%a %a %a\n", e, tangent_stern_explicit(p, slope, term), tangent_current_term(w, d_u, d_p, z_u, z_p, e));
    } else if (!std::strcmp(cmd, "curve")) {
      double a, b, h; int n; if (std::scanf("%lf %lf %lf %d", &a, &b, &h, &n) != 4) return 1;
      if (!continuation_valid(a, b, h)) { for (int i = 0; i < n; ++i) { int ok; if (std::scanf("%d", &ok) != 1) return 1; } std::printf("invalid\n"); continue; }
      Continuation c = continuation_begin(a, b, h);
      for (int i = 0; i < n; ++i) {
        int ok; if (std::scanf("%d", &ok) != 1) return 1;
        if (c.stop) continue;
        const double at = continuation_attempt(c);
        const int reached = continuation_advance(c, ok != 0);
        std::printf("%a %d %a %a %d %d;", at, reached, c.at, c.dp, c.k, c.stop);
      }
      std::printf("\n");
    }
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    d = tmp_path_factory.mktemp("tangent_rule")
    src, exe = d / "rule.cpp", d / "rule"
    src.write_text(DRIVER)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "gmpnp_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True)

    def ask(lines):
        return subprocess.run([str(exe)], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
    return ask


def test_host_rule_against_its_python_statement(rules):
    codes = list(range(-2, 60))
    out = rules(["param %d %d" % (p, nr) for p in codes for nr in (0, 2, 4)])
    k = 0
    for p in codes:
        for nr in (0, 2, 4):
            want = [pol.param_kind(p), pol.param_reaction(p), int(pol.param_valid(p, nr)), int(pol.count_valid(p))]
            assert [int(x) for x in out[k].split()] == want, (p, nr)
            k += 1
    assert [p for p in codes if pol.param_kind(p) >= 0] == [0, 16, 17, 18, 19, 32, 33, 34, 35, 48]
    rng = np.random.default_rng(7)
    cases = [(p, r) + tuple(float(x) for x in rng.standard_normal(9) * 3.0) for p in (0, 16, 17, 32, 33, 48, 5) for r in (0, 1)]
    out = rules(["terms %d %d " % c[:2] + " ".join(repr(x) for x in c[2:]) for c in cases])
    for c, line in zip(cases, out):
        p, r, rate, d_p, eta, slope, term, w, d_u, z_u, z_p = c
        e = pol.rate_explicit(p, r, rate, d_p, eta)
        want = (e, pol.stern_explicit(p, slope, term), pol.current_term(w, d_u, d_p, z_u, z_p, e))
        assert tuple(float.fromhex(x) for x in line.split()) == want, c       # the same operations: equal bits
    scripts = [(-5.0, -10.0, -1.0, [1] * 8), (-5.0, -7.5, -1.0, [1, 0, 1, 1, 1, 1, 1]), (0.0, 0.35, 0.1, [1, 0, 0, 1, 1, 1, 1, 1, 1, 1]),
               (-5.0, -8.0, -1.0, [1] + [0] * 14), (-5.0, -5.0, -1.0, [1]), (-5.0, -10.0, 1.0, [1]), (2.0, 9.0, 2.5, [0, 1, 1, 0, 1, 1, 1, 1])]
    out = rules(["curve %r %r %r %d " % (a, b, h, len(sc)) + " ".join(str(x) for x in sc) for a, b, h, sc in scripts])
    for (a, b, h, sc), line in zip(scripts, out):
        if not pol.continuation_valid(a, b, h):
            assert line == "invalid"
            continue
        c = pol.Continuation(a, b, h)
        want = []
        for ok in sc:
            if c.stop:
                continue
            at = c.attempt_potential()
            reached = c.advance(bool(ok))
            want.append((at, int(reached), c.at, c.dp, c.k, c.stop))
        got = [tuple(x.split()) for x in line.split(";") if x.strip()]
        got = [(float.fromhex(g[0]), int(g[1]), float.fromhex(g[2]), float.fromhex(g[3]), int(g[4]), int(g[5])) for g in got]
        assert got == want, (a, b, h)


def test_ctypes_image_has_the_layout_of_the_header(tmp_path):
    from gmpnp_amd import backend
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gmpnp.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %d\\n",sizeof(gmpnp_tangent_t),'
                   'offsetof(gmpnp_tangent_t,dD),offsetof(gmpnp_tangent_t,dI),offsetof(gmpnp_tangent_t,dp_boundary),offsetof(gmpnp_tangent_t,residual),'
                   'offsetof(gmpnp_tangent_t,status),GMPNP_TANGENT_MAX_COLUMNS);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    C = backend.CTangent
    assert got == [ctypes.sizeof(C), C.dD.offset, C.dI.offset, C.dp_boundary.offset, C.residual.offset, C.status.offset, backend.TANGENT_MAX_COLUMNS]
    assert pol.MAX_COLUMNS == backend.TANGENT_MAX_COLUMNS and pol.MAX_SURFACE_REACTIONS == backend.MAX_SURFACE_REACTIONS
    for name in ("gmpnp_electrode_tangent", "gmpnp_tangent_columns", "gmpnp_electrode_advance"):
        assert name in backend.EXPORTS


def test_python_refusals():
    """Every refusal is a ValueError that names the polarisation, raised before anything touches the device (no GPU here)."""
    from gmpnp_amd import edl1d, edl_ensemble, edl_sweep, pore3d, pore_ensemble, rxndiff1d, rxnpore3d, sweep
    t = dict(kinetics="tafel", i0_CO=TAFEL["i0_CO"], i0_H2=TAFEL["i0_H2"])
    c = dict(polarisation=dict(v_end=-10.0, v_step=-1.0))
    calls = {
        "no electrode voltage": lambda: edl1d.EDLRun(**c),
        "target_current": lambda: edl1d.EDLRun(electrode_voltage=-5.0, target_current=10.0, **t, **c),
        "stabilization": lambda: edl1d.EDLRun(electrode_voltage=-5.0, stabilization="Y", model="PNP", **c),
        "H_OHP": lambda: edl1d.EDLRun(electrode_voltage=-5.0, H_OHP=0.5, **c),
        "dt_order": lambda: edl1d.EDLRun(electrode_voltage=-5.0, adaptive_dt=True, dt_order=2, **c),
        "wrong direction": lambda: edl1d.EDLRun(electrode_voltage=-5.0, polarisation=dict(v_end=-10.0, v_step=1.0)),
        "zero step": lambda: edl1d.EDLRun(electrode_voltage=-5.0, polarisation=dict(v_end=-10.0, v_step=0.0)),
        "no v_step": lambda: edl1d.EDLRun(electrode_voltage=-5.0, polarisation=dict(v_end=-10.0)),
        "kinetic column without kinetics": lambda: edl1d.EDLRun(electrode_voltage=-5.0, polarisation=dict(v_end=-10.0, v_step=-1.0, params=(0, 16))),
        "no p_M column": lambda: edl1d.EDLRun(electrode_voltage=-5.0, polarisation=dict(v_end=-10.0, v_step=-1.0, params=(48,))),
        "repeated column": lambda: edl1d.EDLRun(electrode_voltage=-5.0, polarisation=dict(v_end=-10.0, v_step=-1.0, params=(0, 48, 48))),
        "3D no electrode voltage": lambda: pore3d.PoreRun(**c),
        "3D target_current": lambda: pore3d.PoreRun(electrode_voltage=-5.0, target_current=10.0, **t, **c),
        "3D dt_order": lambda: pore3d.PoreRun(electrode_voltage=-5.0, adaptive_dt=True, dt_order=2, **c),
        "partition": lambda: pore3d.PoreRun(electrode_voltage=-5.0, partition=(2, None), **c),
        "multilevel": lambda: pore3d.PoreRun(electrode_voltage=-5.0, multilevel=True, refine=1, **c),
        "rxn 1D": lambda: rxndiff1d.RxnDiffRun(**c),
        "rxn 3D": lambda: rxnpore3d.RxnPoreRun(**c),
        "EDLEnsemble": lambda: edl_ensemble.EDLEnsemble([dict(voltage_multiplier=-1.0), dict(voltage_multiplier=-1.0, **c)]),
        "PoreEnsemble": lambda: pore_ensemble.PoreEnsemble([dict(**c)]),
        "edl sweep": lambda: edl_sweep.run_sweep([dict(**c)]),
        "edl sweep keywords": lambda: edl_sweep.run_sweep([dict(voltage_multiplier=-1.0)], **c),
        "pore sweep group": lambda: sweep.run_group(5, [-1.0], 1, **c),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError, match="polarisation"):
            call()
    with pytest.raises(ValueError, match="polarisation"):
        edl1d.main(["--polarisation", "--v_end", "-10", "--v_step", "-1"])                       # no --electrode_voltage
    with pytest.raises(ValueError, match="polarisation"):
        edl1d.main(["--polarisation", "--electrode_voltage", "-5"])                               # no grid
    with pytest.raises(ValueError, match="polarisation"):
        pol.refuse_polarisation(c, "a test")
    pol.refuse_polarisation({}, "a test")


def test_command_lines():
    from gmpnp_amd import edl1d, pore3d, rxnpore3d
    for mod in (edl1d, pore3d):
        a = mod.build_parser().parse_args([])
        assert a.polarisation is False and a.v_end is None and a.v_step is None and pol.polarisation_keywords(a) == {}
        a = mod.build_parser().parse_args(["--polarisation", "--v_end", "-30", "--v_step", "-2.5"])
        assert pol.polarisation_keywords(a) == {"polarisation": dict(v_end=-30.0, v_step=-2.5)}
    with pytest.raises(ValueError, match="polarisation"):
        pore3d.main(["--polarisation", "--v_end", "-2", "--v_step", "-0.5"])                      # no --electrode_voltage
    with pytest.raises(SystemExit):
        rxnpore3d.build_parser().parse_args(["--polarisation"])
    par = pol.check_polarisation(dict(v_end=-10.0, v_step=-1.0), dict(electrode_voltage=-5.0))
    assert par["params"] == (0,)
    par = pol.check_polarisation(dict(v_end=-10.0, v_step=-1.0, params=[0, 17, 48]), dict(electrode_voltage=-5.0, kinetics="tafel"))
    assert par["params"] == (0, 17, 48)
    assert [pol.param_name(p) for p in (0, 16, 33, 48, 7)] == ["p_M", "ln_k_0", "alpha_1", "ln_lam", "unknown"]


def test_curve_arrays_units():
    """The physical arrays from scaled records: volts, A/m2 per area, F/m2 = eps_0 / L_n dD, S/m2 = dI / V_T, Tafel slopes."""
    class Ep:
        thermal_voltage, L_n = 0.025, 1e-6
    tan = {"dD": np.array([2.0, 5.0]), "dI": np.array([[-3.0, -8.0], [1.0, 0.0]]), "dp_boundary": np.array([0.4, 0.1]), "residual": np.array([1e-13, 3e-13])}
    rec = [{"p_M": -5.0, "potential_OHP": -2.0, "currents": np.array([6.0, 2.0]), "displacement": -4.0, "tangent": tan, "sechenov_rounds": 0}]
    out = pol.curve_arrays(Ep, 8.0e-12, 2.0, rec, (0, 16), [0], [3])
    assert out["electrode_voltage_V"][0] == -5.0 * 0.025 and out["potential_OHP"][0] == -2.0 * 0.025
    assert (out["i_CO"][0], out["i_H2"][0], out["FE_H2"][0]) == (3.0, 1.0, 0.25)
    assert out["capacitance"][0] == 8.0e-12 / 1e-6 * 2.0 / 2.0 and out["surface_charge"][0] == 8.0e-12 * 0.025 / 1e-6 * -4.0 / 2.0
    assert np.array_equal(out["dI_dV"], np.array([[-3.0, -8.0]]) / 0.025 / 2.0)
    assert np.allclose(out["tafel_slope"], np.log(10.0) * 0.025 / np.array([[-3.0 / 6.0, -8.0 / 2.0]]), rtol=1e-15)
    assert out["sensitivity"].shape == (1, 2, 4) and np.array_equal(out["sensitivity"][0, 1], [5.0, 1.0, 0.0, 0.1])
    assert out["tangent_residual"][0] == 3e-13 and out["newton_iterations"][0] == 3 and out["substeps"][0] == 0
