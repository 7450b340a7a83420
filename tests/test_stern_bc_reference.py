"""The Stern-layer boundary condition on the CPU: the rule g(eps) of the library (gmpnp_host_rules.h, compiled
with the host compiler alone) against its Python statement (gmpnp_amd/stern.py: coupled_g), the NumPy restatement of the boundary term
(tests/stern_bc_reference.py) against finite differences and a closed form, the first-step figures the GPU tests compare with
(tests/test_gpu_stern_bc.py), and every refusal of the Python layer."""
import copy
import math
import os
import subprocess

import numpy as np
import pytest

import stern_bc_reference as R
from conftest import random_state
from step_limit_reference import first_step_state
from gmpnp_amd.problem import SternLayer, edl_problem
from gmpnp_amd.stern import COUPLED_SERIES_SWITCH, EPS_REL_SURFACE, L_STERN, coupled_g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the rule: C++ (g++ alone) against the Python statement ------------------------------------------------------------------------------
DRIVER = r"""
#include <cstdio>
#include "gmpnp_host_rules.h"
using namespace gmpnp;
int main() {
  int model; double eps, eps_s;
  while (std::scanf("%d %lf %lf", &model, &eps, &eps_s) == 3) {
    const SternG G = stern_g(model, eps, eps_s);
    std::printf("%a %a %d\n", G.g, G.dg, G.ok);
  }
  gmpnp_stern_t o{2, -5.0, 4e-4, 6.0};
  std::printf("%d", (int)stern_options_valid(o));
  o.lam = 0.0; std::printf("%d", (int)stern_options_valid(o));
  o.lam = 1.0; o.model = 3; std::printf("%d", (int)stern_options_valid(o));
  o.model = 2; o.eps_surface = 0.0; std::printf("%d", (int)stern_options_valid(o));
  o.model = 1; std::printf("%d", (int)stern_options_valid(o));
  o.model = 0; o.lam = -1.0; std::printf("%d\n", (int)stern_options_valid(o));
  return 0;
}
"""
EPS_VALUES = (6.0, 6.0 * (1.0 + 1e-5), 6.0 * (1.0 - 1e-5), 49.3, 80.1)


@pytest.fixture(scope="module")
def rule_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("stern_rule")
    src = d / "rule.cpp"
    src.write_text(DRIVER)
    exe = d / "rule"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "gmpnp_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True)
    return str(exe)


def test_host_rule_and_python_statement_give_equal_bits(rule_exe):
    """g and g' of both models at eps = 6, 6 (1 +- 1e-5) (the series branch), 49.3 and 80.1 (the closed form): the library's host function
    and coupled_g agree bit for bit; eps <= 0 under BDM is ok = 0 there and a ValueError here; the option check of gmpnp_set_stern."""
    cases = [(m, e) for m in (1, 2) for e in EPS_VALUES] + [(2, 0.0), (2, -3.0), (1, -3.0)]
    text = "".join("%d %r %r\n" % (m, e, EPS_REL_SURFACE) for m, e in cases)
    out = subprocess.run([rule_exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    for (m, e), line in zip(cases, out):
        g_hex, dg_hex, ok = line.split()
        name = {1: "linear", 2: "BDM"}[m]
        if m == 2 and e <= 0.0:
            assert ok == "0" and float.fromhex(g_hex) == 0.0 and float.fromhex(dg_hex) == 0.0
            with pytest.raises(ValueError, match="eps <= 0"):
                coupled_g(name, e)
            continue
        g, dg = coupled_g(name, e)
        assert ok == "1" and float.fromhex(g_hex) == g and float.fromhex(dg_hex) == dg, (m, e, line, g.hex(), dg.hex())
    assert out[len(cases)] == "100011"
    assert coupled_g("linear", 49.3) == (49.3, 1.0)
    assert coupled_g("BDM", 6.0) == (6.0, 0.5)
    with pytest.raises(ValueError):
        coupled_g("quadratic", 49.3)


def test_g_is_continuous_and_smooth_across_the_series_switch():
    """Both branches against eps_s d / log1p(d) (accurate for every d) on either side of |d| = 1e-4, to 1e-12 relative; g' against a
    central difference of g away from the switch and against the accurate derivative next to it."""
    es = EPS_REL_SURFACE
    for sign in (1.0, -1.0):
        for f in (1.0 - 1e-6, 1.0 + 1e-6, 0.5, 1e-3):
            eps = es * (1.0 + sign * COUPLED_SERIES_SWITCH * f)
            d = eps / es - 1.0
            g, dg = coupled_g("BDM", eps)
            assert abs(g / (es * d / math.log1p(d)) - 1.0) < 1e-12, (sign, f)
            lp = math.log1p(d)
            assert abs(dg / (1.0 / lp - d / ((1.0 + d) * lp * lp)) - 1.0) < 1e-6 if abs(d) > 1e-5 else abs(dg - 0.5) < 1e-5
        below, above = (es * (1.0 + sign * COUPLED_SERIES_SWITCH * f) for f in (1.0 - 1e-9, 1.0 + 1e-9))
        gb, ga = coupled_g("BDM", below)[0], coupled_g("BDM", above)[0]
        assert abs(ga - gb) / gb < 1e-12 + 2e-13 * 0.5    # the jump; the function itself moves by 0.5 x 2e-13 over the gap
    for eps in (20.0, 49.3, 80.1):
        h = 1e-5 * eps
        fd = (coupled_g("BDM", eps + h)[0] - coupled_g("BDM", eps - h)[0]) / (2 * h)
        assert abs(coupled_g("BDM", eps)[1] / fd - 1.0) < 1e-8


# ---- the boundary term: finite differences ------------------------------------------------------------------------------------------------
def _edl_k(L_n=1e-6):
    from gmpnp_amd.mesh import read_dolfin_xml, resolve_mesh_path
    from gmpnp_amd.params import edl_parameters, utilities_dir
    ep = edl_parameters(L_n=L_n, cation="K")
    return ep, read_dolfin_xml(resolve_mesh_path(utilities_dir(), ep.mesh_name))


@pytest.fixture(scope="module")
def edl_k():
    return _edl_k()


@pytest.fixture(scope="module")
def cylinder():
    """The (4, 24) generated cylinder of closed_forms.bessel_case with the pore's own model and the Stern Dirichlet set."""
    prob, state, check = R.bessel_stern_case(0, coarse=(4, 24))
    return prob


def stern_free_rows(prob):
    """The potential dofs of the Stern boundary that are not Dirichlet."""
    nf = prob.nf
    nodes = np.unique(prob.wall_facets) if prob.coords.shape[1] == 3 else np.asarray(prob.point_vertices)
    rows = nodes.astype(np.int64) * nf + (nf - 1)
    return np.setdiff1d(rows, prob.bc_dofs)


@pytest.mark.parametrize("model", ["linear", "BDM"])
@pytest.mark.parametrize("dim", [1, 3])
def test_jacobian_of_the_stern_rows_is_the_derivative_of_the_residual(edl_k, cylinder, model, dim):
    """Directional central differences of the Stern rows against J dv at a random admissible state, p_M = -20: within 1e-7 of
    max |J dv| over those rows (the rows are O(1e6): an entry-wise relative test would measure rounding)."""
    if dim == 1:
        ep, mesh = edl_k
        prob = edl_problem(ep, mesh, stern=SternLayer(model, -20.0, L_STERN / ep.L_n))
    else:
        prob = copy.copy(cylinder)
        prob.stern = SternLayer(model, -20.0, L_STERN / 50e-9)
    nv, ns = prob.coords.shape[0], prob.nf - 1
    u, un = random_state(nv, ns, seed=3)
    rows = stern_free_rows(prob)
    assert len(rows) == (1 if dim == 1 else len(np.unique(prob.wall_facets)) - 2 * 24)   # 3D: the rim vertices of both ends keep p = 0
    _, A = R.assemble(prob, u, un)
    rng = np.random.default_rng(7)
    worst = 0.0
    for _ in range(3):
        dv = rng.standard_normal(prob.ndof)
        dv[prob.bc_dofs] = 0.0
        h = 1e-6
        Fp, _ = R.assemble(prob, u + h * dv, un, want_jacobian=False)
        Fm, _ = R.assemble(prob, u - h * dv, un, want_jacobian=False)
        fd, jdv = ((Fp - Fm) / (2 * h))[rows], (A @ dv)[rows]
        worst = max(worst, np.abs(fd - jdv).max() / np.abs(jdv).max())
    print("stern rows, %dD %s: |FD - J dv| / max |J dv| = %.2e" % (dim, model, worst))
    assert worst < 1e-7
    # the term is really there: without it the same rows have another derivative
    off = copy.copy(prob)
    off.stern = None
    _, A0 = R.assemble(off, u, un)
    assert abs((A - A0)[rows]).max() > 1.0


def test_bessel_stern_profile_on_the_generated_cylinder():
    """Poisson coupling with the wall potential applied through a linear Stern layer of lam = 1 / kappa:
    p / p_M = I0(kappa r) / (I0(kappa R) + lam kappa I1(kappa R)) at mid-pore.  rms < 5e-2 (the Dirichlet case's bound in
    test_oracle_pins.py); axis value < 0.6 (Dirichlet: 0.726, Stern closed form: 0.482 — a lost factor or sign fails)."""
    prob, state, check = R.bessel_stern_case(0, coarse=(4, 24))
    u, st = R.newton_loop(prob, state.copy(), state.copy(), relative_tolerance=1e-12, absolute_tolerance=1e-12)
    assert st.converged
    emax, erms, axis, expect = check(u)
    print("bessel-stern: max %.4f rms %.4f axis %.4f expected %.4f" % (emax, erms, axis, expect))
    assert erms < 5e-2 and axis < 0.6, (emax, erms, axis, expect)
    assert abs(expect - 0.482) < 2e-3


# ---- first-step figures of the 1D driver (K+, 1 um mesh, u = 0, u_n = bulk, reference dt; Newton rtol 1e-9 / atol 1e-6) --------------------
# (model, p_M, tau) -> (Newton iterations, smallest step factor, p_OHP, max S over the iterations): measured with the loop below
FIRST_STEP = {
    ("linear", -5.0, 0.0): (6, 1.0, -3.3100173958584014, None),
    ("BDM", -5.0, 0.0): (6, 1.0, -2.2621744442101446, None),
    ("linear", -20.0, 0.9): (9, 0.3237687620554807, -10.631917923758223, 0.9943147443360445),
    ("BDM", -20.0, 0.9): (7, 0.64752450434372, -6.607787654309093, None),
}


def first_step_problem(ep, mesh, model, p_M):
    return edl_problem(ep, mesh, stern=SternLayer(model, p_M, L_STERN / ep.L_n))


@pytest.mark.parametrize("case", sorted(FIRST_STEP))
def test_first_step_figures(edl_k, case):
    ep, mesh = edl_k
    model, p_M, tau = case
    its, min_step, p_ohp, max_S = FIRST_STEP[case]
    prob = first_step_problem(ep, mesh, model, p_M)
    assert not np.isin(prob.point_vertices * prob.nf + prob.nf - 1, prob.bc_dofs).any()   # the OHP potential is free
    u0, un = first_step_state(prob)
    u, st = R.newton_loop(prob, u0, un, tau=tau)
    got = u.reshape(-1, prob.nf)[prob.point_vertices[0], prob.nf - 1]
    print(case, st.iterations, st.min_step, got, max(st.max_S))
    assert st.converged and st.iterations == its
    assert abs(st.min_step - min_step) < 1e-6 and abs(got - p_ohp) < 1e-6
    assert p_M < got < 0.0                                     # part of the voltage drops across the Stern layer
    if max_S is not None:
        assert abs(max(st.max_S) - max_S) < 1e-6
    assert abs(R.stern_displacement(prob, u) - coupled_g(model, prob.model.eps0 + float(np.asarray(prob.model.epsc)[:6] @ u.reshape(-1, 7)[0, :6]))[0]
               * (p_M - got) / prob.stern.lam) < 1e-6 * abs(R.stern_displacement(prob, u))


def test_first_step_at_minus_20_diverges_without_the_limiter(edl_k):
    ep, mesh = edl_k
    prob = first_step_problem(ep, mesh, "linear", -20.0)
    u0, un = first_step_state(prob)
    with np.errstate(all="ignore"):
        u, st = R.newton_loop(prob, u0, un, tau=0.0)
    assert not st.converged and not (st.residuals[-1] < 1e50)


# ---- refusals of the Python layer: ValueError before anything touches the device (there is none here) --------------------------------------
def test_python_refusals():
    from gmpnp_amd import edl1d, edl_ensemble, edl_sweep, pore3d, pore_ensemble, rxndiff1d, rxnpore3d, sweep
    calls = {
        "both voltages": lambda: edl1d.EDLRun(electrode_voltage=-5.0, voltage_multiplier=-1.0),
        "both voltages 3D": lambda: pore3d.PoreRun(electrode_voltage=-5.0, voltage_multiplier=-1.0),
        "stabilization": lambda: edl1d.EDLRun(electrode_voltage=-5.0, stabilization="Y"),
        "H_OHP": lambda: edl1d.EDLRun(electrode_voltage=-5.0, H_OHP=0.5),
        "partition": lambda: pore3d.PoreRun(electrode_voltage=-5.0, partition=(2, None)),
        "multilevel": lambda: pore3d.PoreRun(electrode_voltage=-5.0, multilevel=True, refine=1),
        "rxn 1D": lambda: rxndiff1d.RxnDiffRun(electrode_voltage=-5.0),
        "rxn 3D": lambda: rxnpore3d.RxnPoreRun(electrode_voltage=-5.0),
        "EDLEnsemble": lambda: edl_ensemble.EDLEnsemble([dict(voltage_multiplier=-1.0), dict(electrode_voltage=-5.0)]),
        "PoreEnsemble": lambda: pore_ensemble.PoreEnsemble([dict(electrode_voltage=-5.0)]),
        "edl sweep": lambda: edl_sweep.run_sweep([dict(electrode_voltage=-5.0)]),
        "pore sweep job": lambda: sweep.run_job(5, -1.0, 1, electrode_voltage=-5.0),
        "pore sweep group": lambda: sweep.run_group(5, [-1.0], 1, electrode_voltage=-5.0),
        "bad model": lambda: edl1d.EDLRun(electrode_voltage=-5.0, stern_model="cubic"),
        "bad length": lambda: edl1d.EDLRun(electrode_voltage=-5.0, stern_length=0.0),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError, match="electrode_voltage|Stern"):
            call()
    with pytest.raises(ValueError, match="electrode_voltage"):
        pore3d.main(["--electrode_voltage", "-5", "--partitions", "2"])
    with pytest.raises(ValueError, match="electrode_voltage"):
        pore3d.main(["--electrode_voltage", "-5", "--voltage_multiplier", "-1"])
    with pytest.raises(ValueError, match="electrode_voltage"):
        edl1d.main(["--electrode_voltage", "-5", "--voltage_multiplier", "-1"])
    # the system surfaces refuse the record too (a Problem built by hand)
    from gmpnp_amd.dist import PartitionedSolver
    from gmpnp_amd.solver import GMPNPSystem
    ep, mesh = _edl_k()
    prob = edl_problem(ep, mesh, stern=SternLayer("BDM", -5.0, 4e-4))
    with pytest.raises(ValueError, match="Stern"):
        PartitionedSolver(prob, 2)
    with pytest.raises(ValueError, match="Stern"):
        GMPNPSystem(prob, levels=[(prob, None, None), (prob, None, None)])


def test_command_lines_and_problem_records(edl_k):
    from gmpnp_amd import edl1d, pore3d, rxnpore3d
    from gmpnp_amd.problem import edl_problem as ep_, pop_stern
    for mod in (edl1d, pore3d):
        a = mod.build_parser().parse_args([])
        assert a.electrode_voltage is None and a.voltage_multiplier is None and a.stern_model == "BDM" and a.stern_length == 4e-10 and a.stern_eps_surface == 6.0
        a = mod.build_parser().parse_args(["--electrode_voltage", "-7.5", "--stern_model", "linear", "--stern_length", "5e-10", "--stern_eps_surface", "8"])
        assert (a.electrode_voltage, a.stern_model, a.stern_length, a.stern_eps_surface) == (-7.5, "linear", 5e-10, 8.0)
    with pytest.raises(SystemExit):
        rxnpore3d.build_parser().parse_args(["--electrode_voltage", "-5"])
    kw = dict(electrode_voltage=-5.0, stern_model="linear", L_n=1e-6, voltage_multiplier=None)
    st = pop_stern(kw, kw["L_n"])
    assert kw == {"L_n": 1e-6} and st == SternLayer("linear", -5.0, 4e-4, 6.0)
    kw = dict(voltage_multiplier=-2.0, stern_model="linear")
    assert pop_stern(kw, 1.0) is None and kw == {"voltage_multiplier": -2.0}
    # the Dirichlet sets: only the OHP / wall potential entry goes
    ep, mesh = edl_k
    plain, stern = ep_(ep, mesh), ep_(ep, mesh, stern=st)
    gone = np.setdiff1d(plain.bc_dofs, stern.bc_dofs)
    assert list(gone) == [plain.point_vertices[0] * 7 + 6] and np.isin(stern.bc_dofs, plain.bc_dofs).all() and plain.stern is None
    from gmpnp_amd.mesh import mark_pore_boundaries, pore_wall_tolerance, read_dolfin_xml, resolve_mesh_path
    from gmpnp_amd.params import pore_parameters, utilities_dir
    from gmpnp_amd.problem import pore_dirichlet
    pp = pore_parameters(concentration_elec=0.5, L=10e-9, R=5e-9)
    m3 = read_dolfin_xml(resolve_mesh_path(utilities_dir(), pp.mesh_name))
    bnd = mark_pore_boundaries(m3, pp.aspect_pore, pore_wall_tolerance(pp.L, pp.R))
    d0, v0 = pore_dirichlet(pp, bnd)
    d1, v1 = pore_dirichlet(pp, bnd, stern=True)
    d0b, v0b = pore_dirichlet(pp, bnd)                        # (the cache is keyed by the flag)
    assert np.array_equal(d0, d0b) and np.array_equal(v0, v0b)
    gone = np.setdiff1d(d0, d1)
    s13 = np.union1d(bnd.dirichlet_vertices[1], bnd.dirichlet_vertices[3])
    assert np.array_equal(gone, np.setdiff1d(bnd.dirichlet_vertices[2], s13) * 9 + 8) and len(gone) > 0
    shared = np.intersect1d(bnd.dirichlet_vertices[2], s13) * 9 + 8
    assert len(shared) > 0 and np.all(v1[np.searchsorted(d1, shared)] == 0.0) and np.all(v0[np.searchsorted(d0, shared)] == pp.voltage_scaled)
