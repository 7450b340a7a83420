"""The periodic steady state on the CPU: the two host rules (g++ alone) against their Python statements
(gmpnp_amd/periodic.py), Anderson acceleration of a linear map with three eigenvalues (the Krylov property), case A of the section —
K+ at L_n = 1 um on 33 uniform vertices, BDM Stern layer, two Tafel reactions, the pulse -5.5 / -4.5 for 30 / 20 in 4 fixed steps per
segment, from the steady state at p_M = -5 — over the NumPy system of tests/periodic_reference.py against plain marching, the Python
refusals, the command lines, the ctypes image against the header and the arrays of the history."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import periodic_reference as QR
from gmpnp_amd import periodic as PD
from gmpnp_amd import programme as P
from test_kinetics_reference import TAFEL
from test_programme_reference import steady_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the rules: C++ (g++ alone) against the Python statements -------------------------------------------------------------------------------
DRIVER = r"""
#include <cstdio>
#include <cstring>
#include "gmpnp_host_rules.h"
using namespace gmpnp;
int main() {
  char cmd[32];
  while (std::scanf("%31s", cmd) == 1) {
    if (!std::strcmp(cmd, "weights")) {
      int m; if (std::scanf("%d", &m) != 1 || m < 0 || m > 8) return 1;
      double A[64] = {}, b[8] = {}, gamma[9] = {};
      for (int i = 0; i < m; ++i) for (int j = 0; j < m; ++j) if (std::scanf("%la", &A[i * 8 + j]) != 1) return 1;
      for (int i = 0; i < m; ++i) if (std::scanf("%la", &b[i]) != 1) return 1;
      const int dropped = anderson_weights(m, A, 8, b, gamma);
      std::printf("%d %d", dropped, (int)cycle_gamma_valid(m + 1, gamma));
      for (int i = 0; i <= m; ++i) std::printf(" %a", gamma[i]);
      std::printf("\n");
    } else if (!std::strcmp(cmd, "verdict")) {
      CyclePolicy p; int n, bad; if (std::scanf("%la %d %la %d %d", &p.tol_cycle, &p.max_cycles, &p.growth, &bad, &n) != 5) return 1;
      std::vector<double> e(n);
      for (int i = 0; i < n; ++i) if (std::scanf("%la", &e[i]) != 1) return 1;
      for (int k = 1; k <= n; ++k) std::printf("%d ", (int)cycle_verdict(e.data(), k, bad != 0 && k == n, p));
      std::printf("\n");
    }
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    d = tmp_path_factory.mktemp("periodic_rule")
    src, exe = d / "rule.cpp", d / "rule"
    src.write_text(DRIVER)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "gmpnp_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True)

    def ask(lines):
        return subprocess.run([str(exe)], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
    return ask


def _hex(v):
    v = float(v)
    return "nan" if math.isnan(v) else ("inf" if v == math.inf else ("-inf" if v == -math.inf else v.hex()))


def _weights_line(A, b):
    m = len(b)
    return "weights %d " % m + " ".join(_hex(A[i][j]) for i in range(m) for j in range(m)) + " " + " ".join(_hex(x) for x in b)


def _gram(m, n, seed, scale=None):
    """A normal system of m differences of length n: (A, b, the columns, the residual)."""
    rng = np.random.default_rng(seed)
    D = rng.normal(size=(m, n)) * (np.ones(m) if scale is None else np.asarray(scale))[:, None]
    r = rng.normal(size=n)
    return D @ D.T, D @ r, D, r


def test_anderson_weights_against_the_host_rule_and_least_squares(rules):
    cases = [_gram(m, 40, seed=m) for m in range(1, 9)] + [_gram(4, 30, seed=20, scale=[1e-3, 1.0, 10.0, 1e2]), _gram(8, 200, seed=21)]
    out = rules([_weights_line(A, b) for A, b, _, _ in cases])
    for (A, b, D, r), line in zip(cases, out):
        m = len(b)
        gamma, dropped = PD.anderson_weights(m, A, b)
        tok = line.split()
        got = np.array([float.fromhex(x) for x in tok[2:]])
        assert int(tok[0]) == dropped == 0 and int(tok[1]) == 1 and PD.gamma_valid(gamma)
        assert np.all(np.abs(got - np.array(gamma)) <= 2.0 * np.spacing(np.abs(gamma))), (m, got, gamma)     # within 2 ulp
        # the weights are those of the least-squares problem min |r - sum theta_j d_j| (SVD), to the conditioning of the normal system
        theta = np.linalg.lstsq(D.T, r, rcond=None)[0]
        want = np.r_[theta, 1.0] - np.r_[0.0, theta]
        assert np.allclose(gamma, want, rtol=0.0, atol=100.0 * np.finfo(float).eps * np.linalg.cond(A) * np.abs(want).max())
        assert abs(sum(gamma) - 1.0) <= 1e-12
    assert PD.anderson_weights(0, [], []) == ([1.0], 0)
    tok = rules(["weights 0"])[0].split()
    assert tok[:2] == ["0", "1"] and float.fromhex(tok[2]) == 1.0


def test_singular_systems_drop_the_oldest_columns(rules):
    A, b, D, r = _gram(4, 30, seed=5)
    rep = np.vstack([D[1], D[1], D[2], D[3]])               # a repeated column: columns 0 and 1 are equal
    A_rep, b_rep = rep @ rep.T, rep @ r
    A_nan = A.copy(); A_nan[0, 0] = math.nan                  # a NaN in the oldest column
    A_nan2 = A.copy(); A_nan2[1, 2] = A_nan2[2, 1] = math.nan
    b_nan = b.copy(); b_nan[3] = math.nan                     # nothing is left: the plain iteration
    zero = np.zeros((3, 3))
    cases = [(A_rep, b_rep, 1), (A_nan, b, 1), (A_nan2, b, 2), (A, b_nan, 4), (zero, np.zeros(3), 3), (A * math.inf, b, 4)]
    with np.errstate(invalid="ignore"):
        out = rules([_weights_line(a, c) for a, c, _ in cases])
        for (a, c, want_dropped), line in zip(cases, out):
            gamma, dropped = PD.anderson_weights(len(c), a, c)
            tok = line.split()
            assert int(tok[0]) == dropped == want_dropped, (tok, dropped, want_dropped)
            got = [float.fromhex(x) for x in tok[2:]]
            assert int(tok[1]) == 1 and PD.gamma_valid(gamma) and gamma[:dropped] == [0.0] * dropped == got[:dropped]
            assert np.all(np.abs(np.array(got) - np.array(gamma)) <= 2.0 * np.spacing(np.abs(gamma)))
    gamma, dropped = PD.anderson_weights(4, A_rep, b_rep)     # with the repeated column gone the weights are the 3-column problem's
    g3, d3 = PD.anderson_weights(3, A_rep[1:, 1:], b_rep[1:])
    assert d3 == 0 and gamma[1:] == g3
    assert PD.anderson_weights(4, A, b_nan)[0] == [0.0, 0.0, 0.0, 0.0, 1.0]


def test_cycle_verdict_against_the_host_rule(rules):
    scripts = [(1e-3, 12, 10.0, 0, [1.56, 4.4e-2, 3.7e-2, 6.1e-3, 6.2e-4]),              # converged at the fifth
               (1e-3, 12, 10.0, 0, [1.0, 0.5, 6.0, 0.4, 0.39, 4.0, 1e-3]),               # restarts on growth: 6.0 > 10 x 0.5 and 4.0 > 10 x 0.39
               (1e-3, 4, 10.0, 0, [1.0, 0.9, 0.8, 0.7, 0.6]),                            # max_cycles
               (1e-3, 12, 10.0, 1, [1.0, 0.5, 0.25]),                                    # a non-finite value met by the report / the mix
               (1.0, 50, 10.0, 0, [math.nan, 2.0, math.inf, 0.5]),
               (1e-3, 3, 10.0, 0, [1.0, 0.5, 5e-4])]                                     # converged at the cap is converged
    lines = ["verdict %s %d %s %d %d " % (_hex(t), mc, _hex(g), bad, len(e)) + " ".join(_hex(x) for x in e) for t, mc, g, bad, e in scripts]
    out = rules(lines)
    for (t, mc, g, bad, e), line in zip(scripts, out):
        pol = PD.PeriodicPolicy(tol=t, max_cycles=mc, growth=g)
        want = [PD.cycle_verdict(e[:k], pol, bool(bad) and k == len(e)) for k in range(1, len(e) + 1)]
        assert [int(x) for x in line.split()] == want, (e, want)
    C, K, R, G = PD.CONTINUE, PD.CONVERGED, PD.RESTART, PD.GIVE_UP
    pol = PD.PeriodicPolicy(tol=1e-3, max_cycles=12)
    assert [PD.cycle_verdict(scripts[0][4][:k], pol) for k in range(1, 6)] == [C, C, C, C, K]
    assert [PD.cycle_verdict(scripts[1][4][:k], pol) for k in range(1, 8)] == [C, C, R, C, C, R, K]
    assert [PD.cycle_verdict(scripts[2][4][:k], PD.PeriodicPolicy(tol=1e-3, max_cycles=4)) for k in range(1, 6)] == [C, C, C, G, G]
    assert PD.cycle_verdict([1.0, 0.5, 0.25], pol, nonfinite=True) == R and PD.cycle_verdict([1.0, 5e-4], pol, nonfinite=True) == R
    assert PD.cycle_verdict([math.nan], pol) == R and PD.cycle_verdict([], pol) == C
    assert PD.cycle_verdict([1.0, 0.5, 5e-4], PD.PeriodicPolicy(tol=1e-3, max_cycles=3)) == K


# ---- a linear map: the Krylov property -----------------------------------------------------------------------------------------------------
class LinearMapSystem(QR.NumpyPeriodicSystem):
    """x -> M x + c with M diagonal as the cycle map: one segment, one step; unit weights, every dof free."""

    def __init__(self, Md, c, x0):
        self.Md, self.c = np.asarray(Md, dtype=np.float64), np.asarray(c, dtype=np.float64)
        self.u, self.un = np.array(x0, dtype=np.float64), np.array(x0, dtype=np.float64)
        self.free, self.prob, self.X, self.G, self.newton_iterations = np.ones(len(self.c), dtype=bool), None, [], [], 0

    def set_potential(self, p):
        pass

    def set_step(self, h):
        pass

    def solve(self):
        self.u = self.Md * self.un + self.c
        return True, 1

    def record(self, t, h, seg, p):
        pass

    def accept(self):
        self.un = self.u.copy()

    def breakpoint(self, seg, t):
        pass

    def cycle_open(self, depth):
        self.depth, self.X, self.G, self.w = int(depth), [], [], np.ones(len(self.c))

    def _fresh(self, u, keep_history=False):
        self.u, self.un = np.array(u), np.array(u)


def test_three_eigenvalues_are_solved_by_depth_three():
    """M has the eigenvalues 0.99, 0.9 and 0.5 on three blocks of dofs, so the residuals of the iteration span a Krylov space of
    dimension 3: Anderson acceleration with a window of 3 differences is GMRES on (I - M) x = c and the iterate behind the fourth
    evaluation is the fixed point (a property, not a measurement).  Plain iteration contracts by 0.99 per cycle."""
    rng = np.random.default_rng(7)
    Md = np.repeat([0.99, 0.9, 0.5], [5, 4, 6])
    c = rng.uniform(0.5, 1.5, size=len(Md))
    fixed = c / (1.0 - Md)
    seg = [(0.0, 1.0, 0.0, 0.0)]
    s = LinearMapSystem(Md, c, np.zeros(len(Md)))
    res = PD.run_periodic(s, seg, PD.PeriodicPolicy(tol=1e-13, depth=3, max_cycles=5, tau=0.0), steps_per_segment=1)
    print("linear map, depth 3: residuals %s, dropped %s" % ([r["err"] for r in res["history"]], [r["dropped"] for r in res["history"]]))
    assert res["cycles"] <= 5
    assert np.abs(s.un - fixed).max() <= 1e-10 * np.abs(fixed).max()
    plain = LinearMapSystem(Md, c, np.zeros(len(Md)))
    for _ in range(100):
        P.run_programme(plain, seg, steps_per_segment=1)
    assert np.abs(plain.un - fixed).max() > 1e-3 * np.abs(fixed).max()


class ScriptedSystem(LinearMapSystem):
    """The linear map with one period whose result is thrown far off (the residual grows by more than ``growth``) and one mix that
    meets a value that is not finite (nothing applied, NaN returned)."""

    def __init__(self, Md, c, x0, kick_cycle, nan_mix):
        super().__init__(Md, c, x0)
        self.kick_cycle, self.nan_mix, self.solves, self.mixes, self.restarts_seen = kick_cycle, nan_mix, 0, 0, 0

    def solve(self):
        self.solves += 1
        ok, its = super().solve()
        if self.solves == self.kick_cycle:
            self.u = self.u + 1e3
        return ok, its

    def cycle_mix(self, gamma, tau):
        self.mixes += 1
        if self.mixes == self.nan_mix:
            return math.nan
        return super().cycle_mix(gamma, tau)

    def cycle_restart(self):
        self.restarts_seen += 1
        super().cycle_restart()


def test_the_loop_restarts_on_growth_and_on_a_mix_that_is_not_finite():
    """Both restart branches of ``run_periodic``: the RESTART verdict (cycle 3's residual is more than 10 times cycle 2's) and a mix
    that returns NaN (the third mix asked for).  Each empties the window, the next cycle starts from g_k with a window of one pair,
    and the search still converges to the fixed point."""
    rng = np.random.default_rng(3)
    Md = np.repeat([0.9, 0.5], [5, 6])
    c = rng.uniform(0.5, 1.5, size=len(Md))
    fixed = c / (1.0 - Md)
    s = ScriptedSystem(Md, c, np.zeros(len(Md)), kick_cycle=3, nan_mix=3)
    res = PD.run_periodic(s, [(0.0, 1.0, 0.0, 0.0)], PD.PeriodicPolicy(tol=1e-11, depth=3, max_cycles=40, tau=0.0), steps_per_segment=1)
    h = res["history"]
    print("scripted restarts: verdicts %s, windows %s, restart %s" % ([r["verdict"] for r in h], [r["window"] for r in h], [r["restart"] for r in h]))
    assert res["converged"] and res["restarts"] == 2 == s.restarts_seen == sum(r["restart"] for r in h)
    k = 2                                                   # the kicked cycle: judged RESTART, no mix asked for
    assert h[k]["verdict"] == PD.RESTART and h[k]["restart"] and h[k]["gamma"] == [] and h[k]["err"] > 10.0 * h[k - 1]["err"]
    assert h[k + 1]["window"] == 1 and h[k]["window"] == 3
    j = next(i for i, r in enumerate(h) if r["restart"] and r["verdict"] == PD.CONTINUE)      # the mix that returned NaN
    assert j > k and math.isnan(h[j]["alpha"]) and len(h[j]["gamma"]) == h[j]["window"] and h[j + 1]["window"] == 1
    assert s.mixes >= 3 and np.abs(res["state"] - fixed).max() <= 1e-9 * np.abs(fixed).max()


# ---- case A ----------------------------------------------------------------------------------------------------------------------------------
CASE_A = dict(nv=33, levels=[-5.5, -4.5], durations=[30.0, 20.0], steps=4, tol=1e-3, depth=4, max_cycles=12, tau=0.9, cycle_tol=(1e-2, 1e-4))


def case_a_segments():
    return P.pulse(CASE_A["levels"], CASE_A["durations"], 1)


def period_figures(s):
    """(FE_H2 of the period, its charges Q_CO, Q_H2, Q_D) from the records of ONE recorded period."""
    a = s.arrays()
    qc, qh = float((a["h"] * a["I"][:, 0]).sum()), float((a["h"] * a["I"][:, 1]).sum())
    return np.array([qh / (qc + qh), a["Q"][-1][0], a["Q"][-1][1]]), float(a["Q_D"][-1]), float(np.abs(a["D"] - s.D_first).max())


@pytest.fixture(scope="module")
def case_a():
    """The accelerated run, plain marching under the same cap, and plain marching taken to 1e-3 x tol with one recorded period."""
    ep, prob, u, inv = steady_case(CASE_A["nv"])
    segs, n = case_a_segments(), CASE_A["steps"]
    acc = QR.NumpyPeriodicSystem(prob, u, inv, cycle_tol=CASE_A["cycle_tol"])
    res = PD.run_periodic(acc, segs, PD.PeriodicPolicy(tol=CASE_A["tol"], depth=CASE_A["depth"], max_cycles=CASE_A["max_cycles"], tau=CASE_A["tau"]), n)
    capped = QR.NumpyPeriodicSystem(prob, u, inv, cycle_tol=CASE_A["cycle_tol"])
    capped_errs, capped_ok = QR.plain_march(capped, segs, n, CASE_A["tol"], CASE_A["max_cycles"])
    long_ = QR.NumpyPeriodicSystem(prob, u, inv, cycle_tol=CASE_A["cycle_tol"])
    long_errs, long_ok = QR.plain_march(long_, segs, n, 1e-3 * CASE_A["tol"], 400)
    x_long = long_.un.copy()
    long_._fresh(x_long)
    P.run_programme(long_, segs, steps_per_segment=n)
    return dict(prob=prob, u=u, inv=inv, segs=segs, acc=acc, res=res, capped=(capped_errs, capped_ok), long=long_, long_errs=long_errs,
                long_ok=long_ok, x_long=x_long)


def test_case_a_converges_where_plain_marching_does_not(case_a):
    res = case_a["res"]
    errs = [r["err"] for r in res["history"]]
    print("case A, Anderson depth 4: %d cycles, residuals %s, windows %s, alpha %s, dropped %s, restarts %d" %
          (res["cycles"], errs, [r["window"] for r in res["history"]], [r["alpha"] for r in res["history"]],
           [r["dropped"] for r in res["history"]], res["restarts"]))
    assert res["converged"] and res["cycles"] <= CASE_A["max_cycles"] and errs[-1] <= CASE_A["tol"]
    assert [r["window"] for r in res["history"]] == [min(k + 1, CASE_A["depth"] + 1) for k in range(res["cycles"])] and res["restarts"] == 0
    capped_errs, capped_ok = case_a["capped"]
    print("case A, plain marching under the same cap: residuals %s" % capped_errs)
    assert not capped_ok and len(capped_errs) == CASE_A["max_cycles"] and capped_errs[-1] > CASE_A["tol"]
    assert abs(capped_errs[0] - errs[0]) <= 1e-12 * errs[0]                      # the first cycle is the same march
    n_plain = next(k + 1 for k, e in enumerate(case_a["long_errs"]) if e <= CASE_A["tol"])
    print("case A, plain marching to the same tolerance: %d cycles; to 1e-3 x tol: %d cycles" % (n_plain, len(case_a["long_errs"])))
    assert case_a["long_ok"] and n_plain > 2 * res["cycles"]
    # the recorded period: one period of records from the converged state, which is where ``state`` says it starts
    assert len(case_a["acc"].records) == CASE_A["steps"] * len(case_a["segs"]) and res["record"]["stop_reason"] == "end"
    assert res["record"]["breakpoints"] == [g[1] for g in case_a["segs"]] and res["state"].shape == case_a["u"].shape


def test_case_a_agrees_with_the_long_march(case_a):
    """With rho the contraction of the cycle map in the weighted norm (estimated from the long march's last two residuals), a state
    whose residual is e lies within e / (1 - rho) of the limit cycle: the accelerated state (e <= tol) and the long march's
    (e <= 1e-3 tol) differ by less than 2 tol / (1 - rho) in that norm.  FE_H2 and the charges of the recorded period agree with those of
    the long march's within the same figure as a relative bound."""
    errs = case_a["long_errs"]
    rho = errs[-1] / errs[-2]
    bound = 2.0 * CASE_A["tol"] / (1.0 - rho)
    acc, long_ = case_a["acc"], case_a["long"]
    free = acc.free.ravel()
    q = ((case_a["res"]["state"] - case_a["x_long"]) / acc.w)[free]
    dist = math.sqrt(float((q * q).sum()) / free.sum())
    fig_a, qd_a, swing = period_figures(acc)
    fig_l, qd_l, _ = period_figures(long_)
    rel = np.abs(fig_a - fig_l) / np.abs(fig_l)
    print("case A: rho %.4f, bound %.3e, distance of the states %.3e, relative differences (FE_H2, Q_CO, Q_H2) %s, |Q_D| %.3e and %.3e of a swing of %.3e"
          % (rho, bound, dist, rel.tolist(), abs(qd_a), abs(qd_l), swing))
    assert 0.5 < rho < 0.95
    assert dist <= bound
    assert np.all(rel <= bound)
    assert abs(qd_a - qd_l) <= bound * swing        # the displacement charge of a period of the limit cycle is zero: compared on the swing of D


def test_case_b_short_pulses_on_65_vertices():
    """Case B of the section: 65 vertices, holds of 3 / 2, tolerance 1e-4, where the cycle map contracts by 0.985 per cycle and plain
    marching needs 251 cycles (one run; it is not repeated here).  Depth 4 converges under a cap of 30 cycles
    (16 in that run) and plain marching under the same cap stays more than a decade above the tolerance."""
    ep, prob, u, inv = steady_case(65)
    segs = P.pulse(CASE_A["levels"], [3.0, 2.0], 1)
    s = QR.NumpyPeriodicSystem(prob, u, inv)
    res = PD.run_periodic(s, segs, PD.PeriodicPolicy(tol=1e-4, depth=4, max_cycles=30, tau=0.9), CASE_A["steps"])
    print("case B, depth 4: %d cycles, residuals %s" % (res["cycles"], [r["err"] for r in res["history"]]))
    assert res["converged"] and res["restarts"] == 0 and res["residual"] <= 1e-4
    plain = QR.NumpyPeriodicSystem(prob, u, inv)
    errs, ok = QR.plain_march(plain, segs, CASE_A["steps"], 1e-4, 30)
    print("case B, plain marching: residual %.3e after 30 cycles, contraction %.4f" % (errs[-1], errs[-1] / errs[-2]))
    assert not ok and errs[-1] > 10.0 * 1e-4 and errs[-1] / errs[-2] > 0.9


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------
PULSE_KW = dict(kind="pulse", v_levels=[-5.5, -4.5], durations=[3e-5, 2e-5])


def test_python_refusals():
    """Every refusal is a ValueError that names the programme, raised before anything touches the device (no GPU here)."""
    from gmpnp_amd import edl1d, pore3d
    t = dict(kinetics="tafel", i0_CO=TAFEL["i0_CO"], i0_H2=TAFEL["i0_H2"])
    fixed = dict(PULSE_KW, steps_per_segment=4)
    calls = {
        "no steps_per_segment": (dict(PULSE_KW, periodic={}), "steps_per_segment"),
        "sensitivities": (dict(fixed, periodic={}, sensitivities=["i0_CO"]), "sensitivities"),
        "cycles": (dict(fixed, periodic={}, cycles=3), "cycles"),
        "table that does not close": (dict(kind="table", time_s=[0.0, 1e-5, 3e-5], electrode_voltage=[-5.0, -5.5, -5.25], steps_per_segment=2, periodic={}), "table"),
        "unknown key": (dict(fixed, periodic=dict(beta=0.5)), "periodic"),
        "depth": (dict(fixed, periodic=dict(depth=9)), "depth"),
        "depth 0": (dict(fixed, periodic=dict(depth=0)), "depth"),
        "tol": (dict(fixed, periodic=dict(tol=0.0)), "tol"),
        "max_cycles": (dict(fixed, periodic=dict(max_cycles=0)), "max_cycles"),
        "tau": (dict(fixed, periodic=dict(tau=1.0)), "tau"),
        "growth": (dict(fixed, periodic=dict(growth=1.0)), "growth"),
        "rtol": (dict(fixed, periodic=dict(rtol=-1.0)), "rtol"),
        "atol": (dict(fixed, periodic=dict(atol=0.0)), "atol"),
        "not a dict": (dict(fixed, periodic=3), "periodic"),
    }
    for name, (par, word) in calls.items():
        with pytest.raises(ValueError, match="programme.*" + word):
            edl1d.EDLRun(electrode_voltage=-5.0, programme=par, **t)
    P.check_programme(dict(fixed, periodic={}), dict(electrode_voltage=-5.0))                       # the defaults are fine,
    P.check_programme(dict(fixed, periodic=dict(tol=1e-3, depth=8, max_cycles=12, tau=0.0, growth=5.0, rtol=1e-3, atol=1e-6), cycles=1),
                      dict(electrode_voltage=-5.0))
    P.check_programme(dict(kind="table", time_s=[0.0, 1e-5, 3e-5], electrode_voltage=[-5.0, -5.5, -5.0], steps_per_segment=2, periodic={}),
                      dict(electrode_voltage=-5.0))                                                 # a table that closes,
    P.check_programme(dict(kind="triangle", v_vertex=-6.0, scan_rate=1.0, steps_per_segment=2, periodic={}), dict(electrode_voltage=-5.0))
    assert P.check_programme(dict(fixed, periodic=None), dict(electrode_voltage=-5.0))["periodic"] is None       # and None is the option off
    with pytest.raises(ValueError, match="pore_programme.*periodic"):
        pore3d.PoreRun(electrode_voltage=-1.0, pore_programme=dict(fixed, periodic={}))
    with pytest.raises(ValueError, match="fit_programme.*periodic"):
        edl1d.EDLRun(electrode_voltage=-5.0, programme=dict(fixed, periodic={}), fit_programme=dict(data="no_such_file.npz"), **t)
    with pytest.raises(ValueError, match="periodic"):
        PD.run_periodic(None, [(0.0, 1.0, -5.0, -5.0)], PD.PeriodicPolicy(), None)                  # the loop itself asks for the fixed mode


def test_command_lines():
    from gmpnp_amd import edl1d, pore3d
    base = ["--programme", "pulse", "--v_levels", "-5.5", "-4.5", "--durations", "3e-5", "2e-5", "--programme_steps_per_segment", "4"]
    a = edl1d.build_parser().parse_args(base)
    assert "periodic" not in P.programme_keywords(a)["programme"]                                   # without the flag nothing changes
    a = edl1d.build_parser().parse_args(base + ["--programme_periodic"])
    assert P.programme_keywords(a)["programme"]["periodic"] == {}
    a = edl1d.build_parser().parse_args(base + ["--programme_periodic", "--periodic_tol", "1e-3", "--periodic_depth", "2", "--periodic_max_cycles", "12"])
    par = P.programme_keywords(a)["programme"]
    assert par["periodic"] == dict(tol=1e-3, depth=2, max_cycles=12) and par["steps_per_segment"] == 4
    policy, rtol, atol = PD.check_periodic(par["periodic"], par)
    assert policy == PD.PeriodicPolicy(tol=1e-3, depth=2, max_cycles=12) and (rtol, atol) == (1e-2, 1e-4)
    with pytest.raises(ValueError, match="programme"):
        P.programme_keywords(edl1d.build_parser().parse_args(["--programme_periodic"]))             # no --programme
    with pytest.raises(ValueError, match="programme"):
        P.programme_keywords(edl1d.build_parser().parse_args(base + ["--periodic_depth", "2"]))     # no --programme_periodic
    with pytest.raises(ValueError, match="programme.*steps_per_segment"):
        edl1d.main(["--electrode_voltage", "-5", "--programme", "pulse", "--v_levels", "-5.5", "-4.5", "--durations", "3e-5", "2e-5", "--programme_periodic"])
    with pytest.raises(SystemExit):
        pore3d.build_parser().parse_args(["--programme_periodic"])


def test_ctypes_image_has_the_layout_of_the_header(tmp_path):
    from gmpnp_amd import backend
    fields = ("err", "err_max", "worst_dof", "n_free", "nonfinite", "window", "A", "b")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gmpnp.h"\nint main(void){printf("%zu %d", sizeof(gmpnp_cycle_report_t), GMPNP_CYCLE_MAX_DEPTH);\n'
                   + "".join('printf(" %%zu", offsetof(gmpnp_cycle_report_t,%s));\n' % f for f in fields) + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    C = backend.CCycleReport
    assert got == [ctypes.sizeof(C), backend.CYCLE_MAX_DEPTH] + [getattr(C, f).offset for f in fields]
    assert backend.CYCLE_MAX_DEPTH == PD.MAX_DEPTH == QR.MAX_DEPTH
    for name in ("gmpnp_cycle_open", "gmpnp_cycle_begin", "gmpnp_cycle_end", "gmpnp_cycle_mix", "gmpnp_cycle_restart", "gmpnp_cycle_vectors",
                 "gmpnp_cycle_close"):
        assert name in backend.EXPORTS
    header = open(os.path.join(ROOT, "include", "gmpnp.h")).read()
    for name in backend.EXPORTS:
        if name.startswith("gmpnp_cycle_"):
            assert "int %s(gmpnp_solver* s" % name in header


def test_history_arrays_and_metadata():
    """programme_periodic.npz from a hand-made history: residuals in units of the weights (no conversion), gamma padded with NaN."""
    hist = [dict(err=1.5, err_max=9.0, window=1, gamma=[1.0], alpha=1.0, dropped=0, restart=False, newton=24, verdict=PD.CONTINUE),
            dict(err=0.04, err_max=0.3, window=2, gamma=[-0.25, 1.25], alpha=0.9, dropped=0, restart=False, newton=17, verdict=PD.CONTINUE),
            dict(err=0.9, err_max=4.0, window=3, gamma=[], alpha=math.nan, dropped=0, restart=True, newton=16, verdict=PD.RESTART),
            dict(err=5e-4, err_max=2e-3, window=1, gamma=[], alpha=math.nan, dropped=0, restart=False, newton=9, verdict=PD.CONVERGED)]
    out = PD.history_arrays(hist)
    assert sorted(out) == sorted(PD.HISTORY_COLUMNS) and all(len(v) == 4 for v in out.values())
    assert out["err"].tolist() == [1.5, 0.04, 0.9, 5e-4] and out["window"].tolist() == [1, 2, 3, 1] and out["newton"].sum() == 66
    assert out["gamma"].shape == (4, PD.MAX_DEPTH + 1) and out["gamma"][1, :2].tolist() == [-0.25, 1.25] and np.isnan(out["gamma"][1, 2:]).all()
    assert np.isnan(out["gamma"][2]).all() and out["restart"].tolist() == [False, False, True, False] and out["verdict"][-1] == PD.CONVERGED
    meta = PD.metadata(dict(cycles=4, converged=True, residual=5e-4, restarts=1))
    assert meta == {"programme_periodic_cycles": 4, "programme_periodic_converged": True, "programme_periodic_residual": 5e-4,
                    "programme_periodic_restarts": 1} and sorted(meta) == sorted(PD.METADATA_KEYS)
    assert PD.VERDICTS[PD.GIVE_UP] == "give_up"
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for key in PD.METADATA_KEYS + ("programme_periodic.npz",):
        assert "`%s`" % key in text, key
