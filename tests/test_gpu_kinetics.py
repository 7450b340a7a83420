"""The potential-dependent surface kinetics on the GPU (gmpnp_set_kinetics, csrc/gmpnp_kinetics.h) against the
NumPy restatement of tests/kinetics_reference.py: assembly on the mesh shapes where the addressing changes form, alone and together
with the Stern boundary condition, the option switched off again, a Dirichlet species row, the calibration identity with the constant
fluxes, the first-step figures of the 1D driver, two steps of the 3D driver under two linear solvers, the budgets, the status of a
rate that is not finite, every refusal of the library, hook 25 and the two command lines.  Every handle is closed by `with` / `finally`."""
import copy
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import budget_reference as B
import hp_reference as H
import kinetics_reference as K
from conftest import random_state
from precond_reference import relerr
from step_limit_reference import first_step_state
from test_gpu_stern_bc import SP_FIRST, _closes, _metadata_of, frob_rel, stern_problem
from test_kinetics_reference import FIRST_STEP, TAFEL, first_step_problem, two_reactions
from gmpnp_amd.kinetics import edl_tafel
from gmpnp_amd.problem import SternLayer, edl_problem
from gmpnp_amd.stern import L_STERN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _edl_k():
    from gmpnp_amd.mesh import read_dolfin_xml, resolve_mesh_path
    from gmpnp_amd.params import edl_parameters, utilities_dir
    ep = edl_parameters(L_n=1e-6, cation="K")
    return ep, read_dolfin_xml(resolve_mesh_path(utilities_dir(), ep.mesh_name))


@pytest.fixture(scope="module")
def edl_k():
    return _edl_k()


def kinetic_problem(case, config, pore10, edl_k, p_M=-20.0):
    """(problem with the option, the same problem without it) of an assembly case.  config "kin": the potential of the Stern boundary
    is Dirichlet as the drivers prescribe it without --electrode_voltage (the generated cylinder: free, no term); "kin+linear" /
    "kin+BDM": the Stern boundary condition is on as well."""
    if config == "kin":
        if case.startswith("int"):
            from gmpnp_amd.params import edl_parameters
            prob = edl_problem(edl_parameters(cation="K"), H.uniform_mesh_1d(int(case[3:])))
        elif case == "edl1um":
            prob = edl_problem(edl_k[0], edl_k[1])
        elif case == "cyl259":
            prob = stern_problem(case, None, pore10, edl_k)
        else:
            prob = copy.copy(pore10[2])
    else:
        lam = L_STERN / (1e-6 if case == "edl1um" else 50e-6 if case.startswith("int") else 10e-9)
        prob = stern_problem(case, SternLayer(config[4:], p_M, lam), pore10, edl_k)
    off = copy.copy(prob)
    off.kinetics = None
    on = copy.copy(prob)
    on.kinetics = two_reactions(list(prob.model.species), p_M)
    return on, off


ASSEMBLY_CASES = ["int2", "int255", "int256", "int257", "edl1um", "cyl259", "pore10"]


@pytest.mark.parametrize("config", ["kin", "kin+linear", "kin+BDM"])
@pytest.mark.parametrize("case", ASSEMBLY_CASES)
def test_assembly_matches_the_numpy_restatement(case, config, pore10, edl_k, gpu_lib):
    """F and the CSR Jacobian at a random state to 1e-12 relative (the bound of the Stern tests), the kinetic rows alone under the
    same bound; two calls give equal bits; every row outside the free kinetic species rows is bitwise what a handle without the
    option computes (with Stern on: a Stern-only handle); after set_kinetics(None) so is everything."""
    on, off = kinetic_problem(case, config, pore10, edl_k)
    nv, ns = on.coords.shape[0], on.nf - 1
    u, un = random_state(nv, ns, seed=3)
    rows = K.kinetic_free_rows(on)
    nodes, w = K.boundary_weights(on)
    assert len(rows) >= 3
    if case == "pore10":
        assert len(nodes) > 256                                     # more boundary nodes than one workgroup has lanes
        assert len(rows) < 3 * len(nodes)                           # wall vertices on S1 carry Dirichlet species rows: skipped at run time
    with gpu_lib.DeviceSolver(off) as dev0:
        dev0.set_state(u, un)
        F0, _ = dev0.assemble(True)
        A0 = dev0.jacobian_csr()
    with gpu_lib.DeviceSolver(on) as dev:
        dev.set_state(u, un)
        F, nrm = dev.assemble(True)
        A = dev.jacobian_csr()
        F2, _ = dev.assemble(True)
        assert np.array_equal(F, F2) and np.array_equal(A.data, dev.jacobian_csr().data)
        cur = dev.kinetics_currents()
        assert np.array_equal(cur, dev.kinetics_currents())
        dev.set_kinetics(None)
        with pytest.raises(gpu_lib.GmpnpError, match="no Jacobian"):      # setting the option invalidates the Jacobian
            dev.jacobian_csr()
        F3, _ = dev.assemble(True)
        A3 = dev.jacobian_csr()
    Fo, Ao = K.assemble(on, u, un)
    print("%s %s: F %.2e  J %.2e  rows F %.2e  J %.2e" % (case, config, relerr(F, Fo), frob_rel(A, Ao), relerr(F[rows], Fo[rows]), frob_rel(A[rows], Ao[rows])))
    assert relerr(F, Fo) < 1e-12 and abs(nrm - np.linalg.norm(Fo)) / np.linalg.norm(Fo) < 1e-12
    assert np.array_equal(A.indptr, Ao.indptr) and np.array_equal(A.indices, Ao.indices)
    assert frob_rel(A, Ao) < 1e-12
    assert relerr(F[rows], Fo[rows]) < 1e-12 and frob_rel(A[rows], Ao[rows]) < 1e-12
    ref = K.currents(on, u)
    assert np.all(np.abs(cur - ref) <= 1e-12 * np.abs(ref))
    other = np.setdiff1d(np.arange(on.ndof), rows)
    assert np.array_equal(F[other], F0[other]) and np.array_equal(A[other].data, A0[other].data)
    assert not np.array_equal(F[rows], F0[rows]) and (abs(A[rows] - A0[rows]).max(axis=1).toarray().ravel() > 0).all()
    d = on.bc_dofs
    assert np.array_equal(F[d], u[d] - on.bc_vals) and np.all(A.diagonal()[d] == 1.0) and abs(A[d]).sum() == len(d)
    assert np.array_equal(F3, F0) and np.array_equal(A3.data, A0.data)


def test_a_dirichlet_species_row_receives_nothing(edl_k, gpu_lib):
    """A Dirichlet value planted on the CO2 row of the OHP vertex: that row is the identity row of a handle without the option, in F
    and in J, while the OH row still carries the term; the flag is read at run time (set_dirichlet after set_kinetics)."""
    ep, mesh = edl_k
    base = edl_problem(ep, mesh, stern=SternLayer("BDM", -20.0, L_STERN / ep.L_n), kinetics=two_reactions(ep.species, -20.0))
    v = int(base.point_vertices[0])
    planted = copy.copy(base)
    planted.bc_dofs, planted.bc_vals = np.r_[base.bc_dofs, v * 7 + 4], np.r_[base.bc_vals, 0.75]
    order = np.argsort(planted.bc_dofs)
    planted.bc_dofs, planted.bc_vals = planted.bc_dofs[order], planted.bc_vals[order]
    off = copy.copy(planted)
    off.kinetics = None
    u, un = random_state(base.coords.shape[0], 6, seed=3)
    with gpu_lib.DeviceSolver(off) as dev0:
        dev0.set_state(u, un)
        F0, _ = dev0.assemble(True)
        A0 = dev0.jacobian_csr()
    with gpu_lib.DeviceSolver(base) as dev:                              # created without the planted value: it arrives afterwards
        dev.set_dirichlet(planted.bc_dofs, planted.bc_vals)
        dev.set_state(u, un)
        F, _ = dev.assemble(True)
        A = dev.jacobian_csr()
    Fo, Ao = K.assemble(planted, u, un)
    r_co2, r_oh = v * 7 + 4, v * 7 + 1
    assert F[r_co2] == F0[r_co2] == u[r_co2] - 0.75 and np.array_equal(A[r_co2].toarray(), A0[r_co2].toarray()) and A[r_co2, r_co2] == 1.0
    assert F[r_oh] != F0[r_oh] and A[r_oh, v * 7 + 6] != A0[r_oh, v * 7 + 6]
    assert list(K.kinetic_free_rows(planted)) == [v * 7, v * 7 + 1]
    assert relerr(F, Fo) < 1e-12 and frob_rel(A, Ao) < 1e-12


def test_calibration_identity_with_the_constant_fluxes(edl_k, gpu_lib):
    """1D, 1 um mesh, Stern BDM, p_M = -5.  One reference step with the constant fluxes is converged; at that state
    i0_r = i_prescribed_r / (reactant x E_r) makes the kinetic residual the constant-flux residual to 1e-12 of its largest term (the
    largest flux entering the OHP rows, |J_OH|: the two differ by the rounding of i0 x reactant x E), kinetics_currents returns the
    prescribed partial currents to 1e-12, and gmpnp_newton_solve reports convergence at the first residual with 0 iterations."""
    ep, mesh = edl_k
    p_M = -5.0
    stern = SternLayer("BDM", p_M, L_STERN / ep.L_n)
    const = edl_problem(ep, mesh, stern=stern)
    tight = {"nonlinear_solver": "newton", "newton_solver": {"maximum_iterations": 50, "relative_tolerance": 1.0e-14, "absolute_tolerance": 1.0e-7}}
    u0, un = first_step_state(const)
    with gpu_lib.DeviceSolver(const) as dev:
        dev.set_state(u0, un)
        st = dev.newton_solve(gpu_lib.newton_options(tight, dim=1))
        assert st["converged"] and st["iterations"] > 0
        u = dev.get_state()
        Fc, rc = dev.assemble(False)
    ohp = u.reshape(-1, 7)[int(const.point_vertices[0])]
    i_presc = np.array([ep.current_OHP_ss * 0.8, ep.current_OHP_ss * 0.2])          # H2_FE = 0.2, the default of edl_parameters
    E = math.exp(-0.5 * (p_M - ohp[6]))
    par = dict(TAFEL, i0_CO=i_presc[0] / (ohp[4] * E), i0_H2=i_presc[1] / E)
    kin, model = edl_tafel(ep, par, p_M)
    epk = copy.copy(ep)
    epk.model = model
    prob = edl_problem(epk, mesh, stern=stern, kinetics=kin)
    with gpu_lib.DeviceSolver(prob) as dev:
        dev.set_state(u, un)
        Fk, rk = dev.assemble(False)
        cur = dev.kinetics_currents()
        st = dev.newton_solve(gpu_lib.newton_options(SP_FIRST, dim=1))
    largest = np.abs(ep.model.point_flux).max()
    print("calibration: |F_kin - F_const| / largest = %.2e, currents %s, residual %.2e -> %.2e" % (np.abs(Fk - Fc).max() / largest, cur, rc, rk))
    assert np.abs(Fk - Fc).max() <= 1e-12 * largest
    assert np.all(np.abs(cur - i_presc) <= 1e-12 * i_presc)
    assert st["converged"] and st["iterations"] == 0 and len(st["residuals"]) == 1


@pytest.mark.parametrize("case", sorted(FIRST_STEP))
def test_first_step_through_the_driver(case, edl_k, gpu_lib):
    """EDLRun's first step with the kinetics on (K+, 1 um mesh, Stern BDM) against the NumPy loop: the same Newton count and limiter
    factors, the state within 1e-8, the currents of the table."""
    from gmpnp_amd.edl1d import EDLRun
    p_M, tau = case
    its, min_step, p_ohp, i_CO, i_H2 = FIRST_STEP[case]
    ep, mesh = edl_k
    prob = first_step_problem(ep, mesh, p_M)
    u_ref, st_ref = K.newton_loop(prob, *first_step_state(prob), tau=tau)
    run = EDLRun(num_steps=1, solver_parameters=SP_FIRST, step_fraction=tau, electrode_voltage=p_M, stern_model="BDM", L_n=1e-6, cation="K", kinetics="tafel",
                 **{k: TAFEL[k] for k in ("i0_CO", "i0_H2")})
    try:
        assert run.problem.kinetics == prob.kinetics and run.problem.stern == prob.stern and np.array_equal(run.problem.bc_dofs, prob.bc_dofs)
        assert not run.problem.model.point_flux.any()
        st = run.step(verbose=False)
        u = run.sys.dev.get_state()
        summary = run.kinetics_summary()
    finally:
        run.sys.close()
    print(case, st["iterations"], st["min_step"], np.abs(u - u_ref).max(), summary)
    assert st["converged"] and st["iterations"] == st_ref.iterations == its
    if tau:
        assert np.allclose(st["step_factor"], st_ref.step_factor, rtol=1e-8, atol=0.0) and abs(st["min_step"] - min_step) < 1e-6
    assert np.abs(u - u_ref).max() <= 1e-8 * max(1.0, np.abs(u_ref).max())
    assert abs(u.reshape(-1, 7)[0, 6] - p_ohp) < 1e-6
    assert np.allclose([summary["i_CO"][0], summary["i_H2"][0]], (i_CO, i_H2), rtol=1e-6, atol=0.0)
    assert abs(summary["FE_H2"][0] - i_H2 / (i_CO + i_H2)) < 1e-6


PORE_TAFEL = dict(kinetics="tafel", i0_CO=10.0, i0_H2=1.0)   # illustrative: partial currents of the order of the prescribed 20 A/m2 at p_M = -1


def test_two_pore_steps_under_two_linear_solvers(gpu_lib):
    """Two PoreRun steps on L_10_R_5 with the kinetics on, once with the band LU and once with two-level BiCGStab: the states agree
    within 5e-2 (the bound test_gpu_stern_bc.py puts on the two solvers' profiles of the 3D Stern case), i_CO and i_H2 are finite and
    positive."""
    from gmpnp_amd.pore3d import SOLVER_PARAMETERS, PoreRun
    got = {}
    for linear in ("band_lu", "bicgstab"):
        sp = {"nonlinear_solver": "newton", "newton_solver": dict(SOLVER_PARAMETERS["newton_solver"], linear_solver=linear)}
        run = PoreRun(num_steps=2, solver_parameters=sp, electrode_voltage=-1.0, L=10e-9, R=5e-9, concentration_elec=0.5, **PORE_TAFEL)
        try:
            sts = [run.step(verbose=False) for _ in range(2)]
            got[linear] = (run.sys.dev.get_state(), run.kinetics_summary(), sts)
        finally:
            run.sys.close()
    (u_lu, k_lu, st_lu), (u_kr, k_kr, st_kr) = got["band_lu"], got["bicgstab"]
    assert all(s["converged"] for s in st_lu + st_kr) and st_lu[0]["direct_solves"] > 0 and st_kr[0]["krylov_iterations"] > 0
    diff = np.abs(u_lu - u_kr).max() / max(1.0, np.abs(u_lu).max())
    print("band LU against BiCGStab after two steps: %.2e; currents %s" % (diff, k_lu))
    assert diff < 5e-2
    for k in (k_lu, k_kr):
        for name in ("i_CO", "i_H2"):
            assert len(k[name]) == 2 and np.isfinite(k[name]).all() and (k[name] > 0.0).all()
        assert ((k["FE_H2"] > 0.0) & (k["FE_H2"] < 1.0)).all()
    assert np.allclose(k_lu["i_CO"], k_kr["i_CO"], rtol=5e-2) and np.allclose(k_lu["i_H2"], k_kr["i_H2"], rtol=5e-2)


def _species_rows_close(t, col, prob, u):
    """Every row of a budget table keeps its identity to rounding, and the species rows' point / wall entries are the constant
    flux plus the NumPy integral of the kinetic flux, to 1e-10."""
    sto = [B.COLUMNS.index(c) for c in ("storage", "reaction", "wall", "exit", "point")]
    for f in range(t.shape[0]):
        lhs, rhs = t[f, sto].sum(), t[f, B.COLUMNS.index("dirichlet")] + t[f, B.COLUMNS.index("closure")]
        assert abs(lhs - rhs) <= 1e-10 * np.abs(t[f, 1:]).max(), (f, lhs, rhs)
    fl = K.species_fluxes(prob, u)
    m = prob.model
    if prob.coords.shape[1] == 1:
        const = np.asarray(m.point_flux) * len(prob.point_vertices)
    else:
        const = np.asarray(m.wall_flux) * K.SR.facet_areas(prob).sum()
    ns = prob.nf - 1
    assert np.count_nonzero(fl) >= 2                       # 1D: CO2 and OH (the proton fraction of the current is 0 without H_OHP)
    assert np.all(np.abs(t[:ns, col] - (const[:ns] + fl)) <= 1e-10 * np.abs(fl).max())


def test_budget_1d(edl_k, gpu_lib):
    """--budget with the option on, 1D: every row closes under the normalisation and bound of test_gpu_stern_bc._closes, and the
    species rows' point entries carry the kinetic flux."""
    from gmpnp_amd.edl1d import EDLRun
    run = EDLRun(num_steps=2, budget=True, electrode_voltage=-5.0, stern_model="BDM", L_n=1e-6, cation="K", kinetics="tafel", i0_CO=1.0, i0_H2=0.2)
    try:
        st = [run.step(verbose=False) for _ in range(2)]
        t = run.budget.array()
        u = run.sys.dev.get_state()
        table_now = run.sys.species_budget()
    finally:
        run.sys.close()
    assert t.shape == (2, 7, 8) and np.isfinite(t).all()
    for k in range(2):
        _closes(t[k], run.problem, st[k]["residuals"][-1])
    _species_rows_close(table_now, B.COLUMNS.index("point"), run.problem, u)
    assert not table_now[:6, B.COLUMNS.index("wall")].any()


def test_budget_3d(gpu_lib):
    """The same on L_10_R_5 through PoreRun: the kinetic fluxes sit in the species rows' wall column."""
    from gmpnp_amd.pore3d import PoreRun
    run = PoreRun(num_steps=1, budget=True, electrode_voltage=-1.0, stern_model="linear", L=10e-9, R=5e-9, concentration_elec=0.5, **PORE_TAFEL)
    try:
        st = run.step(verbose=False)
        t = run.budget.array()
        u = run.sys.dev.get_state()
        table_now = run.sys.species_budget()
    finally:
        run.sys.close()
    _closes(t[0], run.problem, st["residuals"][-1])
    _species_rows_close(table_now, B.COLUMNS.index("wall"), run.problem, u)
    assert not table_now[:8, B.COLUMNS.index("point")].any()


def test_a_rate_that_is_not_finite_is_a_numeric_status(edl_k, gpu_lib):
    """A potential planted at the OHP vertex makes E_r overflow: the residual evaluation and the Newton solve report
    GMPNP_ERR_NUMERIC and name the kinetics (a status, not a fault); a good state afterwards assembles again."""
    ep, mesh = edl_k
    prob = first_step_problem(ep, mesh, -5.0)
    nv = prob.coords.shape[0]
    u, un = random_state(nv, 6, seed=5)
    bad = u.copy().reshape(nv, 7)
    v = int(prob.point_vertices[0])
    bad[v, 6] = 3000.0                                                   # exp(-0.5 (-5 - 3000)) = exp(1502.5) = inf
    assert not K.kinetic_terms(prob, bad.ravel())[2] and K.kinetic_terms(prob, u)[2]
    with gpu_lib.DeviceSolver(prob) as dev:
        dev.set_state(bad.ravel(), un)
        for call in (lambda: dev.assemble(False), lambda: dev.assemble(True), lambda: dev.newton_solve(gpu_lib.newton_options(SP_FIRST, dim=1))):
            with pytest.raises(gpu_lib.GmpnpError, match="kinetics") as ei:
                call()
            assert ei.value.code == gpu_lib.ERR_NUMERIC
        assert not np.isfinite(dev.kinetics_currents()).all()
        dev.set_state(u, un)
        F, _ = dev.assemble(False)
        assert relerr(F, K.assemble(prob, u, un, want_jacobian=False)[0]) < 1e-12


def test_library_refusals_and_hook_25(pore10, edl_k, gpu_lib):
    """gmpnp_set_kinetics on a partition handle, on either side of a multilevel link, attaching a coarse level to a handle with the
    option on, an ensemble with such a member (at create and at a later call), SUPG terms, a mesh without a Stern boundary, bad
    options, the calls that need the option on, and hook 25."""
    from ctypes import byref
    from gmpnp_amd import dist
    from gmpnp_amd.problem import pore_hierarchy
    from gmpnp_amd.solver import GMPNPSystem
    pp, mesh, prob3, _ = pore10
    ep, m1 = edl_k
    kin3, kin1 = two_reactions(list(prob3.model.species), -1.0), two_reactions(ep.species, -5.0)
    prob1 = edl_problem(ep, m1)

    def refused(call, what="kinetics"):
        with pytest.raises(gpu_lib.GmpnpError, match=what) as ei:
            call()
        assert ei.value.code == gpu_lib.ERR_INVALID

    dom, perm, part = dist.partition_plan(prob3, 2, 0)
    with gpu_lib.DeviceSolver(dom.problem, perm=perm, partition=part) as partitioned:
        refused(lambda: partitioned.set_kinetics(kin3))
        partitioned.set_kinetics(None)                                 # off is always accepted
    levels = pore_hierarchy(pp, mesh, 1)
    ml = GMPNPSystem(levels[0][0], levels=levels)
    try:
        refused(lambda: ml.dev.set_kinetics(kin3))
        refused(lambda: ml._coarse[0].set_kinetics(kin3))
    finally:
        ml.close()
    with gpu_lib.DeviceSolver(levels[0][0]) as fine, gpu_lib.DeviceSolver(levels[1][0], shared_device=1) as coarse:
        fine.set_kinetics(kin3)
        refused(lambda: fine.attach_coarse_level(coarse, levels[0][2]))
    bare = copy.copy(prob1)
    bare.point_vertices = np.zeros(0, dtype=np.int32)
    with gpu_lib.DeviceSolver(bare) as nob:
        refused(lambda: nob.set_kinetics(kin1))
    with gpu_lib.DeviceSolver(prob1) as a, gpu_lib.DeviceSolver(prob1) as b:
        u0, un = first_step_state(prob1)
        for d in (a, b):
            d.set_state(u0, un)
        refused(lambda: a.time_kernel(25, 1))
        refused(lambda: a.kinetics_currents())
        with gpu_lib.DeviceEnsemble([a, b]) as ens:
            b.set_kinetics(kin1)
            refused(lambda: ens.newton_solve(gpu_lib.newton_options(SP_FIRST, dim=1)))
            refused(lambda: ens.set_time_step([1.0, 1.0]))
            refused(lambda: ens.assign_previous())
            refused(lambda: ens.get_state())
            b.set_kinetics(None)
        b.set_kinetics(kin1)
        refused(lambda: gpu_lib.DeviceEnsemble([a, b]))
        rho = np.full((prob1.coords.shape[0], 6), 0.1)
        a.set_supg(rho)
        refused(lambda: a.set_kinetics(kin1))
        a.set_supg(None)
        refused(lambda: b.set_supg(rho))
        good = gpu_lib.to_ckinetics(kin1, list(ep.species))
        for field, r, value in (("n_reactions", None, 5), ("n_reactions", None, -1), ("reactant", 0, 6), ("reactant", 1, -2), ("k", 0, float("inf")),
                                ("alpha", 1, float("nan")), ("p_eq", 0, float("inf")), ("p_electrode", None, float("nan"))):
            bad = gpu_lib.CKinetics.from_buffer_copy(good)
            if r is None:
                setattr(bad, field, value)
            else:
                getattr(bad, field)[r] = value
            code = a.lib.gmpnp_set_kinetics(a._h, byref(bad))
            assert code == gpu_lib.ERR_INVALID and "kinetics" in a.lib.gmpnp_last_error().decode(), (field, r)
        bad = gpu_lib.CKinetics.from_buffer_copy(good)
        bad.nu[1][3] = float("nan")
        assert a.lib.gmpnp_set_kinetics(a._h, byref(bad)) == gpu_lib.ERR_INVALID
        b.assemble(True)
        assert b.time_kernel(25, 2) > 0.0
        refused(lambda: b.jacobian_csr(), "no Jacobian")                # the timed launches added their entries again: not a Jacobian


def test_command_line_1d(gpu_lib, tmp_path):
    """1D/MPNP_CO2ER_EDL.py --electrode_voltage ... --kinetics tafel ...: the new metadata keys and arrays, and the budget closing."""
    env = dict(os.environ, GMPNP_OUT=str(tmp_path))
    cmd = [sys.executable, os.path.join(ROOT, "1D", "MPNP_CO2ER_EDL.py"), "--L_n=1e-6", "--electrode_voltage=-5", "--num_steps=2", "--budget",
           "--kinetics=tafel", "--i0_CO=1.0", "--i0_H2=0.2", "--alpha_H2=0.4"]
    out = subprocess.run(cmd, check=True, env=env, cwd=str(tmp_path), capture_output=True, text=True).stdout
    assert out.count("kinetics tafel: current_OHP_ss and H2_FE are not used") == 1
    path, meta = _metadata_of(tmp_path)
    assert meta["kinetics"] == "tafel" and (meta["i0_CO"], meta["i0_H2"], meta["alpha_CO"], meta["alpha_H2"], meta["p_eq_CO"], meta["p_eq_H2"]) == (1.0, 0.2, 0.5, 0.4, 0.0, 0.0)
    assert meta["i_CO"] > 0.0 and meta["i_H2"] > 0.0 and abs(meta["FE_H2"] - meta["i_H2"] / (meta["i_CO"] + meta["i_H2"])) < 1e-12
    z = np.load(os.path.join(os.path.dirname(path), "arrays_unscaled.npz"))
    assert z["i_CO"].shape == z["i_H2"].shape == z["FE_H2"].shape == (2,) and z["i_CO"][-1] == meta["i_CO"]
    none = subprocess.run(cmd[:2] + ["--L_n=1e-6", "--kinetics=tafel", "--i0_CO=1", "--i0_H2=1"], env=env, cwd=str(tmp_path), capture_output=True, text=True)
    assert none.returncode != 0 and "electrode_voltage" in none.stderr


def test_command_line_3d(gpu_lib, tmp_path):
    env = dict(os.environ, GMPNP_OUT=str(tmp_path))
    cmd = [sys.executable, os.path.join(ROOT, "3D", "MPNP_CO2ER_pore.py"), "--L=10e-9", "--R=5e-9", "--concentration_elec=0.5", "--num_steps=2",
           "--electrode_voltage=-1", "--step_fraction=0.9", "--kinetics=tafel", "--i0_CO=10", "--i0_H2=1"]
    subprocess.run(cmd, check=True, env=env, cwd=str(tmp_path), stdout=subprocess.DEVNULL)
    path, meta = _metadata_of(tmp_path)
    assert meta["kinetics"] == "tafel" and (meta["i0_CO"], meta["i0_H2"], meta["alpha_CO"], meta["alpha_H2"]) == (10.0, 1.0, 0.5, 0.5)
    assert meta["i_CO"] > 0.0 and meta["i_H2"] > 0.0 and 0.0 < meta["FE_H2"] < 1.0 and meta["num_steps_run"] == 2
    z = np.load(os.path.join(os.path.dirname(path), "arrays_unscaled.npz"))
    assert z["i_CO"].shape == (2,) and z["FE_H2"][-1] == meta["FE_H2"]
