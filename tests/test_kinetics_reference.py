"""The potential-dependent surface kinetics on the CPU: the rate rule of the library (gmpnp_host_rules.h, compiled
with the host compiler alone) against its Python statement (gmpnp_amd/kinetics.py: surface_rate), the NumPy restatement of the boundary
term (tests/kinetics_reference.py) against finite differences and against the constant flux it generalises, the first-step figures the
GPU tests compare with (tests/test_gpu_kinetics.py), the option records and every refusal of the Python layer."""
import copy
import dataclasses
import math
import os
import subprocess

import numpy as np
import pytest

import kinetics_reference as K
import stern_bc_reference as SR
from conftest import random_state
from step_limit_reference import first_step_state
from gmpnp_amd.kinetics import edl_tafel, pore_tafel, surface_rate
from gmpnp_amd.problem import SternLayer, SurfaceKinetics, SurfaceReaction, edl_problem
from gmpnp_amd.stern import L_STERN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the rule: C++ (g++ alone) against the Python statement ------------------------------------------------------------------------------
DRIVER = r"""
#include <cstdio>
#include "gmpnp_host_rules.h"
using namespace gmpnp;
int main() {
  double k, alpha, p_eq, p_M, p, u; int has;
  while (std::scanf("%lf %lf %lf %lf %lf %d %lf", &k, &alpha, &p_eq, &p_M, &p, &has, &u) == 7) {
    const KinRate R = surface_rate(k, alpha, p_eq, p_M, p, has, u);
    std::printf("%a %a %a %d\n", R.rate, R.d_u, R.d_p, R.ok);
  }
  gmpnp_kinetics_t o{};
  o.n_reactions = 2; o.reactant[0] = 4; o.reactant[1] = -1; o.k[0] = 1.0; o.k[1] = 0.2; o.alpha[0] = o.alpha[1] = 0.5; o.p_electrode = -5.0;
  std::printf("%d", (int)kinetics_options_valid(o, 6));
  o.n_reactions = 5; std::printf("%d", (int)kinetics_options_valid(o, 6));
  o.n_reactions = -1; std::printf("%d", (int)kinetics_options_valid(o, 6));
  o.n_reactions = 2; o.reactant[0] = 6; std::printf("%d", (int)kinetics_options_valid(o, 6));
  o.reactant[0] = -2; std::printf("%d", (int)kinetics_options_valid(o, 6));
  o.reactant[0] = 5; std::printf("%d", (int)kinetics_options_valid(o, 6));
  o.k[1] = 1.0 / 0.0; std::printf("%d", (int)kinetics_options_valid(o, 6));
  o.k[1] = 0.2; o.nu[1][7] = 0.0 / 0.0; std::printf("%d", (int)kinetics_options_valid(o, 6));
  o.nu[1][7] = 0.0; o.p_electrode = 0.0 / 0.0; std::printf("%d", (int)kinetics_options_valid(o, 6));
  o.n_reactions = 0; o.p_electrode = 0.0; o.k[3] = 0.0 / 0.0; std::printf("%d\n", (int)kinetics_options_valid(o, 6));   // unused slots are not read
  return 0;
}
"""
# (k, alpha, p_eq, p_M, p, has_reactant, u_reactant)
RATE_CASES = [(1.0, 0.5, 0.0, -20.0, -6.6, 1, 0.178), (0.2, 0.5, 0.0, -20.0, -6.6, 0, 0.0), (3.7, 0.31, -1.25, -5.0, -2.26, 1, 0.92),
              (1.0, 0.0, 0.0, -5.0, -2.0, 0, 0.0), (1.0, 0.5, 0.0, -40.0, -9.0, 1, -0.05), (2.0, 1.0, 2.0, 3.0, 0.5, 1, 1.5),
              (1.0, 0.5, 0.0, -3000.0, 0.0, 1, 0.5), (1.0, 0.5, 0.0, -3000.0, 0.0, 1, 0.0), (1e300, 0.5, 0.0, -1400.0, 0.0, 0, 0.0)]


def ulps(a, b):
    if a == b:
        return 0.0
    return abs(a - b) / math.ulp(max(abs(a), abs(b)))


@pytest.fixture(scope="module")
def rule_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("kinetics_rule")
    src = d / "rule.cpp"
    src.write_text(DRIVER)
    exe = d / "rule"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "gmpnp_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True)
    return str(exe)


def test_host_rule_against_its_python_statement(rule_exe):
    """rate, d rate / d u and d rate / d p of the library's host function and of surface_rate agree within 2 ulp (exp comes from two
    libms), the verdict is equal — the overflowing cases are not finite on both sides —, and the option check of gmpnp_set_kinetics."""
    text = "".join("%r %r %r %r %r %d %r\n" % c for c in RATE_CASES)
    out = subprocess.run([rule_exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    verdicts = []
    for c, line in zip(RATE_CASES, out):
        h = line.split()
        got = [float.fromhex(x) if "0x" in x else float(x) for x in h[:3]]
        rate, d_u, d_p, ok = surface_rate(*c)
        assert int(h[3]) == int(ok), (c, line)
        verdicts.append(ok)
        if ok:
            worst = max(ulps(a, b) for a, b in zip(got, (rate, d_u, d_p)))
            assert worst <= 2.0, (c, line, worst)
    assert verdicts == [True] * 6 + [False] * 3
    assert out[len(RATE_CASES)] == "1000010001"
    assert surface_rate(1.0, 0.0, 0.0, -5.0, -2.0, False, 0.0) == (1.0, 1.0, 0.0, True)       # the constant flux
    r = surface_rate(1.0, 0.5, 0.0, -40.0, -9.0, True, -0.05)
    assert r[0] < 0.0 and r[1] > 0.0 and r[3]                                                  # the reactant is not clamped


# ---- the boundary term ---------------------------------------------------------------------------------------------------------------------
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
    """The (4, 24) generated cylinder of closed_forms.bessel_case with the pore's full model and the Stern Dirichlet set."""
    import closed_forms as cf
    prob = SR.bessel_stern_case(0, coarse=(4, 24))[0]
    prob.model = cf._base(10e-9, 5e-9, 0, reactions=True, wall_flux=True, steady=False, q_scale=1.0, coarse=(4, 24))[1]
    return prob


def two_reactions(species, p_M, k=(5e-2, 1e-2)):
    """Two reactions, one with a reactant (CO2), alpha = 0.5, O(1) flux weights on three species."""
    assert "CO2" in species and "OH" in species
    other = "CO" if "CO" in species else "H"
    return SurfaceKinetics([SurfaceReaction(k=k[0], alpha=0.5, p_eq=0.25, reactant="CO2", nu={"CO2": 0.7, "OH": -1.3, other: -0.4}),
                            SurfaceReaction(k=k[1], alpha=0.5, p_eq=-0.5, reactant=None, nu={"OH": -2.1, other: 0.0})], p_M)


def kinetic_case(dim, edl_k, cylinder, stern="BDM", p_M=-20.0):
    if dim == 1:
        ep, mesh = edl_k
        st = SternLayer(stern, p_M, L_STERN / ep.L_n) if stern else None
        return edl_problem(ep, mesh, stern=st, kinetics=two_reactions(ep.species, p_M))
    prob = copy.copy(cylinder)
    prob.stern = SternLayer(stern, p_M, L_STERN / 50e-9) if stern else None
    prob.kinetics = two_reactions(list(prob.model.species), p_M)
    return prob


@pytest.mark.parametrize("dim", [1, 3])
def test_jacobian_of_the_kinetic_rows_is_the_derivative_of_the_residual(edl_k, cylinder, dim):
    """Directional central differences of the kinetic rows against J dv at a random state, p_M = -20, two reactions, one with a
    reactant, alpha = 0.5: within 1e-7 of max |J dv| over those rows (the bound of section 5h for the same procedure)."""
    prob = kinetic_case(dim, edl_k, cylinder)
    nv, ns = prob.coords.shape[0], prob.nf - 1
    u, un = random_state(nv, ns, seed=3)
    rows = K.kinetic_free_rows(prob)
    n_nodes = 1 if dim == 1 else len(np.unique(prob.wall_facets))
    assert len(rows) == 3 * n_nodes                     # CO2, OH and the third species; no species row of the wall is Dirichlet here
    _, A = K.assemble(prob, u, un)
    rng = np.random.default_rng(7)
    worst = 0.0
    for _ in range(3):
        dv = rng.standard_normal(prob.ndof)
        dv[prob.bc_dofs] = 0.0
        h = 1e-6
        Fp, _ = K.assemble(prob, u + h * dv, un, want_jacobian=False)
        Fm, _ = K.assemble(prob, u - h * dv, un, want_jacobian=False)
        fd, jdv = ((Fp - Fm) / (2 * h))[rows], (A @ dv)[rows]
        worst = max(worst, np.abs(fd - jdv).max() / np.abs(jdv).max())
    print("kinetic rows, %dD: |FD - J dv| / max |J dv| = %.2e" % (dim, worst))
    assert worst < 1e-7
    # the term is really there, and it is the whole difference to the problem without the option
    off = copy.copy(prob)
    off.kinetics = None
    F0, A0 = K.assemble(off, u, un)
    F1, _ = K.assemble(prob, u, un)
    D = (A - A0).tocsr()
    assert (abs(D[rows]).max(axis=1).toarray().ravel() > 0.0).all()
    other = np.setdiff1d(np.arange(prob.ndof), rows)
    assert abs(D[other]).max() == 0.0 and np.array_equal(F0[other], F1[other]) and not np.array_equal(F0[rows], F1[rows])


@pytest.mark.parametrize("dim", [1, 3])
def test_one_reaction_without_potential_or_reactant_is_the_constant_flux(edl_k, cylinder, dim):
    """alpha = 0, reactant none, k = 1, nu = J: the kinetic F equals the constant-flux F to 1e-14 of the largest term (not bitwise:
    sum_f (J |f| / 3) and J sum_f |f| / 3 round differently), and the Jacobian gains nothing."""
    prob = kinetic_case(dim, edl_k, cylinder, stern=None)
    prob.kinetics = None
    m = prob.model
    J = np.asarray(m.point_flux if dim == 1 else m.wall_flux, dtype=np.float64)
    assert np.count_nonzero(J) >= 2
    zero = {("point_flux" if dim == 1 else "wall_flux"): np.zeros_like(J)}
    kin = copy.copy(prob)
    kin.model = dataclasses.replace(m, **zero)
    kin.kinetics = SurfaceKinetics([SurfaceReaction(k=1.0, alpha=0.0, reactant=None, nu={s: J[i] for i, s in enumerate(m.species) if J[i] != 0.0})], -7.0)
    u, un = random_state(prob.coords.shape[0], prob.nf - 1, seed=3)
    F0, A0 = K.assemble(prob, u, un, apply_bc=False)
    F1, A1 = K.assemble(kin, u, un, apply_bc=False)
    bare = copy.copy(kin)
    bare.kinetics = None
    Fz, _ = K.assemble(bare, u, un, want_jacobian=False, apply_bc=False)
    largest = np.abs(F0 - Fz).max()                      # the flux term itself
    assert largest > 0.0
    print("constant-flux identity, %dD: %.2e of the largest flux term" % (dim, np.abs(F1 - F0).max() / largest))
    assert np.abs(F1 - F0).max() <= 1e-14 * max(largest, np.abs(F0).max())
    assert abs(A1 - A0).max() == 0.0


# ---- first-step figures of the 1D driver (K+, 1 um mesh, Stern BDM, u = 0, u_n = bulk, reference dt; Newton rtol 1e-9 / atol 1e-6) ----------
TAFEL = dict(i0_CO=0.1, i0_H2=0.02, alpha_CO=0.5, alpha_H2=0.5, p_eq_CO=0.0, p_eq_H2=0.0)   # illustrative, not fitted to anything
# (p_M, tau) -> (Newton iterations, smallest step factor, p_OHP, i_CO, i_H2): measured with the loop below
FIRST_STEP = {
    (-5.0, 0.0): (6, 1.0, -2.26181984, 0.36189237, 0.07863543),
    (-5.0, 0.9): (6, 1.0, -2.26181984, 0.36189237, 0.07863543),
    (-20.0, 0.9): (8, 0.6646639643, -6.60870096, 14.40704133, 16.17758291),
}


def first_step_problem(ep, mesh, p_M, par=TAFEL):
    ep = copy.copy(ep)
    kin, ep.model = edl_tafel(ep, par, p_M)
    return edl_problem(ep, mesh, stern=SternLayer("BDM", p_M, L_STERN / ep.L_n), kinetics=kin)


@pytest.mark.parametrize("case", sorted(FIRST_STEP))
def test_first_step_figures(edl_k, case):
    ep, mesh = edl_k
    p_M, tau = case
    its, min_step, p_ohp, i_CO, i_H2 = FIRST_STEP[case]
    prob = first_step_problem(ep, mesh, p_M)
    assert not prob.model.point_flux.any() and ep.model.point_flux.any()        # the driven constant fluxes are zeroed, on a copy
    u, st = K.newton_loop(prob, *first_step_state(prob), tau=tau)
    got = u.reshape(-1, prob.nf)[prob.point_vertices[0], prob.nf - 1]
    cur = K.currents(prob, u)
    print(case, st.iterations, st.min_step, got, cur)
    assert st.converged and st.iterations == its
    assert abs(st.min_step - min_step) < 1e-6 and abs(got - p_ohp) < 1e-6
    assert np.allclose(cur, (i_CO, i_H2), rtol=1e-6, atol=0.0)
    # the rates are what the rule gives at the OHP state, and the fluxes are the prefactors times the rates
    u0 = u.reshape(-1, 7)[0]
    E = math.exp(-0.5 * (p_M - u0[6]))
    assert np.allclose(cur, (0.1 * u0[4] * E, 0.02 * E), rtol=1e-12)
    fl = K.species_fluxes(prob, u)
    assert abs(fl[4] - ep.J_CO2_prefactor * 0.5 * cur[0]) <= 1e-12 * abs(fl[4]) and abs(fl[1] + ep.J_OH_prefactor * cur.sum()) <= 1e-12 * abs(fl[1])


# ---- records, options and refusals of the Python layer: ValueError before anything touches the device (there is none here) -------------------
def test_option_records_and_the_two_tafel_reactions(edl_k):
    from gmpnp_amd import backend
    from gmpnp_amd.params import pore_parameters
    from gmpnp_amd.problem import pop_kinetics
    ep, mesh = edl_k
    kin, model = edl_tafel(ep, TAFEL, -5.0)
    assert [r.reactant for r in kin.reactions] == ["CO2", None] and kin.p_electrode == -5.0
    assert kin.reactions[0].nu["CO2"] == ep.J_CO2_prefactor * 0.5 and kin.reactions[1].nu["OH"] == -ep.J_OH_prefactor and "CO2" not in kin.reactions[1].nu
    assert not model.point_flux.any() and ep.model.point_flux.any()
    c = backend.to_ckinetics(kin, list(ep.species))
    assert c.n_reactions == 2 and list(c.reactant)[:2] == [4, -1] and list(c.k)[:2] == [0.1, 0.02] and c.p_electrode == -5.0
    assert c.nu[0][4] == ep.J_CO2_prefactor * 0.5 and c.nu[1][1] == -ep.J_OH_prefactor and c.nu[1][4] == 0.0
    pp = pore_parameters(concentration_elec=0.5, L=10e-9, R=5e-9)
    kin3, model3 = pore_tafel(pp, TAFEL, -1.0, _farad())
    assert not model3.wall_flux.any() and np.count_nonzero(pp.model.wall_flux) == 4
    # with the rates equal to the prescribed partial currents the weights give back J_wall (the default H2_FE = 0.05 of pore_parameters)
    i_tot = pp.current_planar
    for name, J in pp.scalars["J_wall"].items():
        got = sum(r.nu.get(name, 0.0) * i for r, i in zip(kin3.reactions, (i_tot * 0.95, i_tot * 0.05)))
        assert abs(got - J) <= 1e-12 * abs(J), name
    kw = dict(kinetics="tafel", i0_CO=1.0, i0_H2=0.5, alpha_H2=0.4, L_n=1e-6)
    assert pop_kinetics(kw) == dict(i0_CO=1.0, i0_H2=0.5, alpha_CO=0.5, alpha_H2=0.4, p_eq_CO=0.0, p_eq_H2=0.0) and kw == {"L_n": 1e-6}
    assert pop_kinetics(dict(i0_CO=1.0)) is None
    for bad in (dict(kinetics="butler"), dict(kinetics="tafel", i0_CO=1.0), dict(kinetics="tafel", i0_CO=1.0, i0_H2=float("nan"))):
        with pytest.raises(ValueError, match="kinetics"):
            pop_kinetics(bad)
    with pytest.raises(ValueError, match="kinetics"):
        SurfaceKinetics([], -5.0)
    with pytest.raises(ValueError, match="kinetics"):
        SurfaceKinetics([SurfaceReaction(k=1.0)] * 5, -5.0)
    with pytest.raises(ValueError, match="kinetics"):
        SurfaceKinetics([SurfaceReaction(k=float("inf"))], -5.0)
    with pytest.raises(ValueError, match="kinetics"):
        SurfaceKinetics([SurfaceReaction(k=1.0, nu={"CO2": float("nan")})], -5.0)
    with pytest.raises(ValueError, match="no species"):
        SurfaceKinetics([SurfaceReaction(k=1.0, reactant="Xe")], -5.0).check_species(ep.species)


def _farad():
    from gmpnp_amd.params import _load_yaml, utilities_dir
    return _load_yaml(os.path.join(utilities_dir(), "parameters_pore.yaml"))["nat_const"]["F"]


def test_python_refusals():
    from gmpnp_amd import edl1d, edl_ensemble, edl_sweep, pore3d, pore_ensemble, rxndiff1d, rxnpore3d, sweep
    t = dict(kinetics="tafel", i0_CO=1.0, i0_H2=0.2)
    calls = {
        "no electrode voltage": lambda: edl1d.EDLRun(**t),
        "no electrode voltage 3D": lambda: pore3d.PoreRun(**t),
        "no i0": lambda: edl1d.EDLRun(electrode_voltage=-5.0, kinetics="tafel", i0_CO=1.0),
        "unknown kind": lambda: edl1d.EDLRun(electrode_voltage=-5.0, kinetics="marcus", i0_CO=1.0, i0_H2=1.0),
        "stabilization": lambda: edl1d.EDLRun(electrode_voltage=-5.0, stabilization="Y", model="PNP", **t),
        "H_OHP": lambda: edl1d.EDLRun(electrode_voltage=-5.0, H_OHP=0.5, **t),
        "partition": lambda: pore3d.PoreRun(electrode_voltage=-5.0, partition=(2, None), **t),
        "multilevel": lambda: pore3d.PoreRun(electrode_voltage=-5.0, multilevel=True, refine=1, **t),
        "rxn 1D": lambda: rxndiff1d.RxnDiffRun(**t),
        "rxn 3D": lambda: rxnpore3d.RxnPoreRun(**t),
        "EDLEnsemble": lambda: edl_ensemble.EDLEnsemble([dict(voltage_multiplier=-1.0), dict(voltage_multiplier=-1.0, **t)]),
        "PoreEnsemble": lambda: pore_ensemble.PoreEnsemble([dict(**t)]),
        "edl sweep": lambda: edl_sweep.run_sweep([dict(**t)]),
        "edl sweep keywords": lambda: edl_sweep.run_sweep([dict(voltage_multiplier=-1.0)], **t),
        "pore sweep job": lambda: sweep.run_job(5, -1.0, 1, kinetics="tafel"),
        "pore sweep group": lambda: sweep.run_group(5, [-1.0], 1, **t),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError, match="kinetics|electrode_voltage|Stern"):
            call()
    # the kinetics' own message wherever the Stern check does not come first
    for name in ("no electrode voltage", "no electrode voltage 3D", "no i0", "unknown kind", "rxn 1D", "rxn 3D", "EDLEnsemble", "PoreEnsemble", "edl sweep",
                 "edl sweep keywords", "pore sweep job", "pore sweep group"):
        with pytest.raises(ValueError, match="kinetics"):
            calls[name]()
    with pytest.raises(ValueError, match="kinetics|electrode_voltage"):
        pore3d.main(["--electrode_voltage", "-5", "--partitions", "2", "--kinetics", "tafel", "--i0_CO", "1", "--i0_H2", "1"])
    with pytest.raises(ValueError, match="kinetics"):
        edl1d.main(["--kinetics", "tafel", "--i0_CO", "1", "--i0_H2", "1"])
    with pytest.raises(ValueError, match="kinetics"):
        pore3d.main(["--kinetics", "tafel", "--i0_CO", "1", "--i0_H2", "1"])
    # the system surfaces refuse the record too (a Problem built by hand)
    from gmpnp_amd.dist import PartitionedSolver
    from gmpnp_amd.solver import GMPNPSystem
    ep, mesh = _edl_k()
    prob = edl_problem(ep, mesh, kinetics=edl_tafel(ep, TAFEL, -5.0)[0])
    with pytest.raises(ValueError, match="kinetics"):
        PartitionedSolver(prob, 2)
    with pytest.raises(ValueError, match="kinetics"):
        GMPNPSystem(prob, levels=[(prob, None, None), (prob, None, None)])


def test_command_lines():
    from gmpnp_amd import edl1d, pore3d, rxnpore3d
    from gmpnp_amd.problem import kinetics_keywords
    for mod in (edl1d, pore3d):
        a = mod.build_parser().parse_args([])
        assert a.kinetics is None and a.i0_CO is None and a.i0_H2 is None and (a.alpha_CO, a.alpha_H2, a.p_eq_CO, a.p_eq_H2) == (0.5, 0.5, 0.0, 0.0)
        assert kinetics_keywords(a) == {}
        a = mod.build_parser().parse_args(["--kinetics", "tafel", "--i0_CO", "2.5", "--i0_H2", "0.5", "--alpha_CO", "0.4", "--p_eq_H2", "-1.5"])
        assert kinetics_keywords(a) == dict(kinetics="tafel", i0_CO=2.5, i0_H2=0.5, alpha_CO=0.4, alpha_H2=0.5, p_eq_CO=0.0, p_eq_H2=-1.5)
        with pytest.raises(SystemExit):
            mod.build_parser().parse_args(["--kinetics", "marcus"])
    with pytest.raises(SystemExit):
        rxnpore3d.build_parser().parse_args(["--kinetics", "tafel"])


def test_ctypes_image_has_the_layout_of_the_header(tmp_path):
    import ctypes
    from gmpnp_amd import backend
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gmpnp.h"\nint main(void){printf("%zu %zu %zu %zu %d\\n",sizeof(gmpnp_kinetics_t),'
                   'offsetof(gmpnp_kinetics_t,k),offsetof(gmpnp_kinetics_t,nu),offsetof(gmpnp_kinetics_t,p_electrode),GMPNP_MAX_SURFACE_REACTIONS);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    C = backend.CKinetics
    assert got == [ctypes.sizeof(C), C.k.offset, C.nu.offset, C.p_electrode.offset, backend.MAX_SURFACE_REACTIONS]
    from gmpnp_amd.problem import MAX_SURFACE_REACTIONS
    assert MAX_SURFACE_REACTIONS == backend.MAX_SURFACE_REACTIONS
