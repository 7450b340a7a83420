"""The fraction-to-boundary step limiter on the CPU: the NumPy restatement of the rule (tests/step_limit_reference.py) in a Newton
loop over the oracle's assembly, the host rules of the library (gmpnp_host_rules.h, compiled with the host compiler alone), and the
argument checks that need no GPU.  The figures pinned here are this oracle's (SuperLU, zero start, omega = 1, rtol 1e-9 /
atol 1e-10)."""
import os
import subprocess
import warnings

import numpy as np
import pytest

import step_limit_reference as R
from conftest import ROOT, _edl

TAU = 0.9
# first Newton solve of the 1 um mesh from the zero state: (cation, voltage_multiplier) -> (iterations, smallest step factor)
HARD_CASES = {("Cs", -10.0): (10, 0.205), ("Cs", -12.5): (11, 0.128), ("K", -10.0): (11, 0.213), ("Li", -10.0): (10, 0.157)}


@pytest.mark.parametrize("cation,voltage", sorted(HARD_CASES))
def test_first_solve_of_the_hard_cases_converges_with_the_limiter(cation, voltage):
    iterations, min_factor = HARD_CASES[(cation, voltage)]
    _, _, prob = _edl(L_n=1e-6, cation=cation, voltage_multiplier=voltage)
    u0, un = R.first_step_state(prob)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, st = R.newton_loop(prob, u0, un, tau=TAU)
    print(cation, voltage, st.iterations, st.min_step, st.step_factor, max(st.max_S))
    assert st.converged and st.iterations == iterations
    assert abs(st.min_step - min_factor) <= 0.02 * min_factor
    assert st.limited_steps >= 1 and all(0.0 < f <= 1.0 for f in st.step_factor)
    assert max(st.max_S) < 1.0   # admissible after every update


def test_without_the_limiter_the_same_loop_diverges():
    """tau = 0 is the plain loop: the divergence tests/test_oracle.py::test_config0_first_newton_solve_diverges_in_the_oracle asserts."""
    _, _, prob = _edl(L_n=1e-6, cation="Cs", voltage_multiplier=-10.0)
    u0, un = R.first_step_state(prob)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, st = R.newton_loop(prob, u0, un, tau=0.0)
    r = np.array(st.residuals)
    assert not st.converged and st.iterations == 50
    assert not np.all(np.isfinite(r)) or r[-1] > 1e-2 * r[0]
    assert max(st.max_S) >= 1.0   # the iterate left the admissible set


def never_engages(prob, omega, plain_loop=True):
    u0, un = R.first_step_state(prob)
    _, lim = R.newton_loop(prob, u0, un, tau=TAU, omega=omega, keep_iterates=True, beside_plain=True)
    assert lim.converged and lim.iterations >= 5
    assert lim.step_factor == [1.0] * lim.iterations and lim.limited_steps == 0 and lim.min_step == 1.0
    assert lim.same_as_plain == [True] * lim.iterations
    if plain_loop:   # the plain loop on its own (what same_as_plain says by induction)
        _, plain = R.newton_loop(prob, u0, un, tau=0.0, omega=omega, keep_iterates=True)
        assert plain.converged and lim.iterations == plain.iterations
        for a, b in zip(plain.iterates, lim.iterates):
            assert np.array_equal(a, b)
        assert lim.residuals == plain.residuals


def test_the_limiter_never_engages_on_edl1(edl1):
    never_engages(edl1[2], 1.0)


def test_the_limiter_never_engages_on_edl50(edl50):
    never_engages(edl50[2], 1.0)


def test_the_limiter_never_engages_on_the_small_pore(pore10):
    """L_10_R_5 at 0.5 M with the 3D driver's omega = 0.9.  The plain update is formed beside the limited one in ONE loop
    (step_limit_reference.newton_loop, beside_plain): a sparse LU of the 3D Jacobian per iteration is what this test costs, and a
    second loop would double it.  (The suite has no marker for slow oracle tests; this is the slowest test of this file.)"""
    never_engages(pore10[2], 0.9, plain_loop=False)


# ---- the rule itself ---------------------------------------------------------------------------------------------------------------
A = np.array([0.5, 0.25, 0.125])


def state(S):
    """(n, 4) vertex rows (three species + potential) with the given steric sums: all of S in species 0."""
    S = np.asarray(S, dtype=float)
    return np.stack([S / A[0], np.zeros_like(S), np.zeros_like(S), np.full_like(S, -3.0)], axis=1)


def test_rule_without_a_decreasing_node():
    u, dx = state([0.2, 0.9, 0.5]), state([0.1, 0.5, 0.0])    # dS >= 0 everywhere: S does not grow along -dx
    assert R.step_limit(A, u, dx, TAU) == (1.0, np.inf, -1)


def test_rule_skips_an_inadmissible_node():
    u, dx = state([1.5, 0.5, 1.0]), state([-10.0, -0.25, -10.0])   # nodes 0 and 2 have S >= 1: only node 1 counts
    alpha, lam, node = R.step_limit(A, u, dx, TAU)
    assert (lam, node) == (2.0, 1) and alpha == 1.0


def test_rule_at_and_just_below_one():
    u = state([0.5, 0.25])
    alpha, lam, node = R.step_limit(A, u, state([-0.5, -0.5]), TAU)    # lambda exactly 1: not limited
    assert (alpha, lam, node) == (1.0, 1.0, 0)
    d = np.nextafter(0.5, 1.0)
    alpha, lam, node = R.step_limit(A, u, state([-d, -0.5]), TAU)      # just below 1: limited
    assert lam == 0.5 / d < 1.0 and node == 0 and alpha == TAU * lam


def test_rule_takes_the_minimum_and_the_first_of_equal_ratios():
    u = state([0.5, 0.75, 0.5, 0.0])
    alpha, lam, node = R.step_limit(A, u, state([-1.0, -1.0, -1.0, 0.5]), TAU)   # ratios 0.5, 0.25, 0.5, -
    assert (lam, node) == (0.25, 1) and alpha == TAU * 0.25
    alpha, lam, node = R.step_limit(A, u, state([-1.0, 0.5, -1.0, 0.5]), TAU)    # ratios 0.5, -, 0.5, -
    assert (lam, node) == (0.5, 0)


def test_rule_refuses_a_nan_or_inf_correction():
    u = state([0.5, 0.25])
    for bad in (np.nan, np.inf, -np.inf):
        dx = state([-0.1, -0.1])
        dx[1, 3] = bad    # the potential's entry counts too
        with pytest.raises(ValueError):
            R.step_limit(A, u, dx, TAU)


def test_update_uses_omega_times_alpha():
    """One iteration of the loop: u_1 = u_0 - (omega alpha) dx with alpha of the rule at (u_0, dx) — not min(omega, tau lambda)."""
    import gmpnp_oracle as O
    import scipy.sparse.linalg as spla
    _, _, prob = _edl(L_n=1e-6, cation="Cs", voltage_multiplier=-10.0)
    u0, un = R.first_step_state(prob)
    _, st = R.newton_loop(prob, u0, un, tau=TAU, omega=0.5, maximum_iterations=3, keep_iterates=True)
    u2 = st.iterates[1]
    b, J = O.assemble(prob, u2, un, want_jacobian=True)
    dx = spla.splu(J.tocsc()).solve(b)
    nv, nf = prob.coords.shape[0], prob.nf
    alpha, lam, _ = R.step_limit(np.asarray(prob.model.a)[:nf - 1], u2.reshape(nv, nf), dx.reshape(nv, nf), TAU)
    assert lam < 1.0 and alpha == TAU * lam == st.step_factor[2]
    assert np.array_equal(st.iterates[2], u2 - (0.5 * alpha) * dx)


# ---- host rules of the library (no device in them) -------------------------------------------------------------------------------
HOST_DRIVER = r"""
#include <cstdio>
#include <cmath>
#include "gmpnp_host_rules.h"
using namespace gmpnp;
int main() {
  const double taus[] = {0.0, 0.9, 1e-300, 1.0, -0.5, 1.5, NAN, INFINITY};
  for (double t : taus) printf("%d ", step_fraction_valid(t) ? 1 : 0);
  printf("\n%.17g %.17g %.17g %.17g\n", step_factor(1.0, 0.9), step_factor(0.5, 0.9), step_factor(INFINITY, 0.9), step_factor(std::nextafter(1.0, 0.0), 0.9));
  gmpnp_newton_stats_t st = fresh_newton_stats();
  printf("%d %.17g\n", st.limited_steps, st.min_step);
  record_step(st, 0, 1.0); record_step(st, 1, 0.25); record_step(st, 2, 0.5); record_step(st, 200, 0.125);
  printf("%d %.17g %.17g %.17g %.17g\n", st.limited_steps, st.min_step, st.step_factor[0], st.step_factor[1], st.step_factor[2]);
  gmpnp_newton_options_t o{}; o.relative_tolerance = 1e-4; o.absolute_tolerance = 1e-4; o.maximum_iterations = 50;
  NewtonJudge j(o, st, false);
  j.first(1.0, 0); st.iterations++;
  const NewtonJudge::Verdict v = j.next(0.5, 16);
  printf("%d %d %s\n", (int)(v == NewtonJudge::failed), j.code, j.message.c_str());
  return 0;
}
"""


def test_host_rules_of_the_limiter(tmp_path):
    src, exe = tmp_path / "sl.cpp", tmp_path / "sl"
    src.write_text(HOST_DRIVER)
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "gmpnp_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert out[0].split() == ["1", "1", "1", "0", "0", "0", "0", "0"]
    below = float(np.nextafter(1.0, 0.0))
    assert [float(x) for x in out[1].split()] == [1.0, 0.9 * 0.5, 1.0, 0.9 * below]
    assert out[2].split() == ["0", "1"]
    assert [float(x) for x in out[3].split()] == [3.0, 0.125, 1.0, 0.25, 0.5]   # an iteration past the history still counts
    assert out[4].startswith("1 -5 ") and "NaN / Inf in the Newton correction" in out[4]


# ---- argument checks that need no GPU -----------------------------------------------------------------------------------------------
def test_newton_options_carry_the_step_fraction():
    from gmpnp_amd import backend
    base = {"nonlinear_solver": "newton", "newton_solver": {"maximum_iterations": 50, "relative_tolerance": 1e-4, "absolute_tolerance": 1e-4}}
    assert backend.newton_options(base, dim=1).step_fraction == 0.0   # absent = off
    sp = backend.with_step_fraction(base, 0.9)
    assert "step_fraction" not in base["newton_solver"] and sp["newton_solver"]["step_fraction"] == 0.9
    assert backend.with_step_fraction(base, 0.0) is base
    o = backend.newton_options(sp, dim=1)
    assert o.step_fraction == 0.9 and o.linear_solver == backend.LINEAR_BLOCK_TRIDIAGONAL and o.relaxation_parameter == 1.0
    for bad in (1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="step_fraction"):
            backend.newton_options(backend.with_step_fraction(base, bad), dim=1)
    with pytest.raises(RuntimeError):   # 'snes' stays refused, with or without the key
        backend.newton_options({"nonlinear_solver": "snes", "newton_solver": {"step_fraction": 0.9}})
    st = backend.CNewtonStats()
    st.iterations, st.min_step, st.limited_steps = 2, 0.25, 1
    st.step_factor[0], st.step_factor[1] = 1.0, 0.25
    d = backend.DeviceSolver.stats_dict(st)
    assert (d["limited_steps"], d["min_step"], d["step_factor"]) == (1, 0.25, [1.0, 0.25])


def test_drivers_take_the_flag():
    from gmpnp_amd import edl1d, edl_sweep, pore3d, rxndiff1d, rxnpore3d
    for mod, extra in ((edl1d, []), (rxndiff1d, []), (pore3d, []), (rxnpore3d, []), (edl_sweep, ["--voltage_multiplier", "-10"])):
        assert mod.build_parser().parse_args(extra).step_fraction == 0.0
        assert mod.build_parser().parse_args(extra + ["--step_fraction", "0.9"]).step_fraction == 0.9


def test_3d_ensembles_and_partitioned_runs_refuse_the_limiter_before_the_device():
    from gmpnp_amd.pore3d import PoreRun
    from gmpnp_amd.pore_ensemble import PoreEnsemble
    members = [dict(concentration_elec=0.5, L=10e-9, R=5e-9), dict(concentration_elec=1.0, L=10e-9, R=5e-9)]
    with pytest.raises(ValueError, match="step_fraction"):
        PoreEnsemble(members, num_steps=1, step_fraction=0.9)
    with pytest.raises(ValueError, match="step_fraction"):
        PoreRun(num_steps=1, partition=(2, None), step_fraction=0.9, concentration_elec=0.5, L=10e-9, R=5e-9)
