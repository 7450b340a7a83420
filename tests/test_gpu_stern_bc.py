"""The Stern-layer boundary condition on the GPU (gmpnp_set_stern, csrc/gmpnp_stern.h) against the NumPy
restatement of tests/stern_bc_reference.py: assembly on the mesh shapes where the gather lists change form, the option switched off
again, the first-step figures of the 1D driver, the Bessel-Stern closed form, the budget's potential row, the metadata, the eps <= 0
status, every refusal of the library and the two command lines.  Every handle is closed by `with` / `finally`."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import budget_reference as B
import hp_reference as H
import stern_bc_reference as R
from conftest import random_state
from precond_reference import relerr
from step_limit_reference import first_step_state
from test_stern_bc_reference import FIRST_STEP, first_step_problem, stern_free_rows
from gmpnp_amd.problem import SternLayer, edl_problem, pore_problem
from gmpnp_amd.stern import L_STERN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def frob_rel(A, Bm):
    D = (A - Bm).tocsr()
    return np.sqrt((D.data ** 2).sum()) / np.sqrt((Bm.data ** 2).sum())


def _edl_k():
    from gmpnp_amd.mesh import read_dolfin_xml, resolve_mesh_path
    from gmpnp_amd.params import edl_parameters, utilities_dir
    ep = edl_parameters(L_n=1e-6, cation="K")
    return ep, read_dolfin_xml(resolve_mesh_path(utilities_dir(), ep.mesh_name))


@pytest.fixture(scope="module")
def edl_k():
    return _edl_k()


def stern_problem(case, stern, pore10=None, edl_k=None):
    """The problem of an assembly case with the record `stern` (None: the same Dirichlet set without the term, the parent path)."""
    if case.startswith("int"):
        from gmpnp_amd.params import edl_parameters
        ep = edl_parameters(cation="K")
        prob = edl_problem(ep, H.uniform_mesh_1d(int(case[3:])), stern=SternLayer("BDM", 0.0, 1.0))
    elif case == "edl1um":
        prob = edl_problem(edl_k[0], edl_k[1], stern=SternLayer("BDM", 0.0, 1.0))
    elif case == "cyl259":
        import closed_forms as cf
        prob = R.bessel_stern_case(0, coarse=(3, 6))[0]      # (its Dirichlet set: the wall potential free, p = 0 on both rims)
        assert prob.coords.shape[0] == 259
        prob.model = cf._base(10e-9, 5e-9, 0, reactions=True, wall_flux=True, steady=False, q_scale=1.0, coarse=(3, 6))[1]   # the pore's full model
    else:
        pp, mesh = pore10[0], pore10[1]
        prob, _ = pore_problem(pp, mesh, stern=SternLayer("BDM", 0.0, 1.0))
    prob = copy.copy(prob)
    prob.stern = stern
    return prob


ASSEMBLY_CASES = ["int2", "int255", "int256", "int257", "edl1um", "cyl259", "pore10"]


@pytest.mark.parametrize("model", ["linear", "BDM"])
@pytest.mark.parametrize("case", ASSEMBLY_CASES)
def test_assembly_matches_the_numpy_restatement(case, model, pore10, edl_k, gpu_lib):
    """F and the CSR Jacobian at a random state to 1e-12 relative (the bound of test_assembly_matches_oracle); two calls give equal
    bits; every row outside the free Stern rows — the wall vertices whose potential row is Dirichlet among them — is bitwise what a
    handle without the option computes; after set_stern(None) so is everything, as on a handle that never had the option."""
    lam = L_STERN / (1e-6 if case == "edl1um" else 50e-6 if case.startswith("int") else 10e-9)
    on = stern_problem(case, SternLayer(model, -20.0, lam), pore10, edl_k)
    off = stern_problem(case, None, pore10, edl_k)
    nv, ns = on.coords.shape[0], on.nf - 1
    u, un = random_state(nv, ns, seed=3)
    rows = stern_free_rows(on)
    assert len(rows) >= 1
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
        d_gpu = dev.stern_displacement()
        assert d_gpu == dev.stern_displacement()
        dev.set_stern(None)
        with pytest.raises(gpu_lib.GmpnpError, match="no Jacobian"):      # setting the option invalidates the Jacobian
            dev.jacobian_csr()
        F3, _ = dev.assemble(True)
        A3 = dev.jacobian_csr()
    Fo, Ao = R.assemble(on, u, un)
    print("%s %s: F %.2e  J %.2e" % (case, model, relerr(F, Fo), frob_rel(A, Ao)))
    assert relerr(F, Fo) < 1e-12 and abs(nrm - np.linalg.norm(Fo)) / np.linalg.norm(Fo) < 1e-12
    assert np.array_equal(A.indptr, Ao.indptr) and np.array_equal(A.indices, Ao.indices)
    assert frob_rel(A, Ao) < 1e-12
    # the Stern rows alone, against their own size (they are a small part of the Frobenius norm on the 3D meshes)
    assert relerr(F[rows], Fo[rows]) < 1e-12 and frob_rel(A[rows], Ao[rows]) < 1e-12
    assert abs(d_gpu - R.stern_displacement(on, u)) <= 1e-10 * abs(d_gpu)
    other = np.setdiff1d(np.arange(on.ndof), rows)
    assert np.array_equal(F[other], F0[other]) and np.array_equal(A[other].data, A0[other].data)
    assert not np.array_equal(F[rows], F0[rows]) and (abs(A[rows] - A0[rows]).max(axis=1).toarray().ravel() > 0).all()
    d = on.bc_dofs
    assert np.array_equal(F[d], u[d] - on.bc_vals) and np.all(A.diagonal()[d] == 1.0) and abs(A[d]).sum() == len(d)
    assert np.array_equal(F3, F0) and np.array_equal(A3.data, A0.data)


SP_FIRST = {"nonlinear_solver": "newton", "newton_solver": {"maximum_iterations": 50, "relative_tolerance": 1.0e-9, "absolute_tolerance": 1.0e-6}}


@pytest.mark.parametrize("case", sorted(FIRST_STEP))
def test_first_step_through_the_driver(case, edl_k, gpu_lib):
    """EDLRun's first step (K+, 1 um mesh) against the NumPy loop: the same Newton count and limiter factors, the state within 1e-8."""
    from gmpnp_amd.edl1d import EDLRun
    model, p_M, tau = case
    its, min_step, p_ohp, _ = FIRST_STEP[case]
    ep, mesh = edl_k
    prob = first_step_problem(ep, mesh, model, p_M)
    u_ref, st_ref = R.newton_loop(prob, *first_step_state(prob), tau=tau)
    run = EDLRun(num_steps=1, solver_parameters=SP_FIRST, step_fraction=tau, electrode_voltage=p_M, stern_model=model, L_n=1e-6, cation="K")
    try:
        assert run.problem.stern == prob.stern and np.array_equal(run.problem.bc_dofs, prob.bc_dofs)
        st = run.step(verbose=False)
        u = run.sys.dev.get_state()
        ohp = run.ohp_summary()
    finally:
        run.sys.close()
    print(case, st["iterations"], st["min_step"], np.abs(u - u_ref).max())
    assert st["converged"] and st["iterations"] == st_ref.iterations == its
    if tau:
        assert np.allclose(st["step_factor"], st_ref.step_factor, rtol=1e-8, atol=0.0) and abs(st["min_step"] - min_step) < 1e-6
    assert np.abs(u - u_ref).max() <= 1e-8 * max(1.0, np.abs(u_ref).max())
    assert abs(u.reshape(-1, 7)[0, 6] - p_ohp) < 1e-6 and abs(ohp["potential_OHP"] / ep.thermal_voltage - p_ohp) < 1e-6


@pytest.mark.parametrize("linear", ["band_lu", "bicgstab"])
def test_bessel_stern_profile_on_the_reference_mesh(linear, gpu_lib):
    """stern_bc_reference.bessel_stern_case on L_50_R_5, once with the band LU and once with two-level BiCGStab: rms < 5e-2 (the bound
    of the Dirichlet case on this mesh in test_gpu_parity.py), the axis value within 0.05 of the closed form."""
    prob, state, check = R.bessel_stern_case(0)
    ns = {"linear_solver": linear, "maximum_iterations": 50, "relative_tolerance": 1e-12, "absolute_tolerance": 1e-12, "relaxation_parameter": 1.0}
    if linear == "bicgstab":
        ns["krylov_solver"] = {"relative_tolerance": 1e-10}
    with gpu_lib.DeviceSolver(prob) as dev:
        dev.set_state(state, state)
        st = dev.newton_solve(gpu_lib.newton_options({"nonlinear_solver": "newton", "newton_solver": ns}))
        u = dev.get_state()
    emax, erms, axis, expect = check(u)
    print("bessel-stern (%s): max %.4f rms %.4f axis %.4f expected %.4f, Newton %d, Krylov %d" % (linear, emax, erms, axis, expect, st["iterations"],
                                                                                                 st["krylov_iterations"]))
    assert st["converged"] and (st["direct_solves"] > 0 if linear == "band_lu" else st["krylov_iterations"] > 0)
    assert erms < 5e-2 and abs(axis - expect) < 0.05, (emax, erms, axis, expect)


def _closes(t, prob, residual):
    """The potential row of a budget table: the identity to rounding, and the closure under 5g's bound."""
    p = t[-1]
    lhs = p[[B.COLUMNS.index(c) for c in ("storage", "reaction", "wall", "exit", "point")]].sum()
    rhs = p[B.COLUMNS.index("dirichlet")] + p[B.COLUMNS.index("closure")]
    assert abs(lhs - rhs) <= 1e-10 * np.abs(p[1:]).max(), (lhs, rhs, p)
    ratio = np.abs(t[:, B.COLUMNS.index("closure")]) / (np.sqrt(B.n_free(prob)) * residual)
    print("max |closure| / (sqrt(n_free) x residual) =", ratio.max(), "potential row:", ratio[-1])
    assert ratio.max() < 1.0


def test_budget_and_metadata_1d(edl_k, gpu_lib):
    """--budget with the option on, 1D: the potential row closes (the Stern term sits in its point column), stern_displacement is the
    NumPy integral of the term on the downloaded state, surface_charge its physical value."""
    from gmpnp_amd.edl1d import EDLRun
    run = EDLRun(num_steps=2, budget=True, electrode_voltage=-5.0, stern_model="BDM", L_n=1e-6, cation="K")
    try:
        st = [run.step(verbose=False) for _ in range(2)]
        t = run.budget.array()
        meta = run.stern_summary()
        u = run.sys.dev.get_state()
        table_now = run.sys.species_budget()
    finally:
        run.sys.close()
    assert t.shape == (2, 7, 8) and np.isfinite(t).all()
    for k in range(2):
        _closes(t[k], run.problem, st[k]["residuals"][-1])
    point, wall = B.COLUMNS.index("point"), B.COLUMNS.index("wall")
    ref = R.stern_displacement(run.problem, u)
    assert meta["stern_displacement"] < 0.0 and abs(meta["stern_displacement"] - ref) <= 1e-10 * abs(ref)
    assert table_now[-1, point] == meta["stern_displacement"] and table_now[-1, wall] == 0.0
    assert meta["electrode_voltage"] == -5.0 and meta["stern_model"] == "BDM" and abs(meta["stern_length"] - 4e-10) < 1e-24
    from gmpnp_amd.params import _load_yaml, utilities_dir
    ep, eps_0 = run.ep, _load_yaml(os.path.join(utilities_dir(), "parameters.yaml"))["nat_const"]["eps_0"]
    assert abs(meta["surface_charge"] - eps_0 * ep.thermal_voltage / ep.L_n * ref) < 1e-9 * abs(meta["surface_charge"])
    assert -1.0 < meta["surface_charge"] < 0.0            # a cathode: negative charge, well under 1 C/m2


def test_budget_and_metadata_3d(gpu_lib):
    """The same on L_10_R_5 through PoreRun: the Stern term sits in the potential row's wall column."""
    from gmpnp_amd.pore3d import PoreRun
    run = PoreRun(num_steps=1, budget=True, electrode_voltage=-1.0, stern_model="linear", L=10e-9, R=5e-9, concentration_elec=0.5)
    try:
        st = run.step(verbose=False)
        t = run.budget.array()
        meta = run.stern_summary()
        u = run.sys.dev.get_state()
    finally:
        run.sys.close()
    free = stern_free_rows(run.problem)
    p_wall = u[free]
    assert -1.0 < p_wall.min() and p_wall.max() < 0.0        # the wall potential is a result, between the electrode's and the bulk's
    _closes(t[0], run.problem, st["residuals"][-1])
    ref = R.stern_displacement(run.problem, u)
    assert abs(meta["stern_displacement"] - ref) <= 1e-10 * abs(ref)
    assert abs(t[0, -1, B.COLUMNS.index("wall")] - ref) <= 1e-10 * abs(ref) and t[0, -1, B.COLUMNS.index("point")] == 0.0
    assert meta["stern_model"] == "linear" and abs(meta["stern_length"] - 4e-10) < 1e-24 and meta["surface_charge"] < 0.0


def test_eps_not_positive_is_a_numeric_status(edl_k, gpu_lib):
    """BDM with eps <= 0 planted at the OHP vertex: the residual evaluation and the Newton solve report GMPNP_ERR_NUMERIC (a status,
    not a fault); the linear model evaluates the same state; a good state afterwards assembles again."""
    ep, mesh = edl_k
    prob = edl_problem(ep, mesh, stern=SternLayer("BDM", -5.0, L_STERN / ep.L_n))
    nv = prob.coords.shape[0]
    u, un = random_state(nv, 6, seed=5)
    epsc = np.asarray(prob.model.epsc)[:6]
    j = int(np.argmin(epsc))
    assert epsc[j] < 0.0
    bad = u.copy().reshape(nv, 7)
    v = int(prob.point_vertices[0])
    bad[v, j] = (prob.model.eps0 + float(epsc @ bad[v, :6]) - epsc[j] * bad[v, j] + 1.0) / -epsc[j]   # eps = -1 at the vertex
    assert prob.model.eps0 + float(epsc @ bad[v, :6]) < 0.0
    with pytest.raises(ValueError):
        R.stern_terms(prob, bad.ravel())
    with gpu_lib.DeviceSolver(prob) as dev:
        dev.set_state(bad.ravel(), un)
        for call in (lambda: dev.assemble(False), lambda: dev.assemble(True), lambda: dev.newton_solve(gpu_lib.newton_options(SP_FIRST, dim=1))):
            with pytest.raises(gpu_lib.GmpnpError, match="Stern") as ei:
                call()
            assert ei.value.code == gpu_lib.ERR_NUMERIC
        dev.set_stern(SternLayer("linear", -5.0, L_STERN / ep.L_n))
        F, _ = dev.assemble(False)
        assert np.isfinite(F).all()
        dev.set_stern(prob.stern)
        dev.set_state(u, un)
        F, _ = dev.assemble(False)
        assert relerr(F, R.assemble(prob, u, un, want_jacobian=False)[0]) < 1e-12


def test_library_refusals(pore10, edl_k, gpu_lib):
    """gmpnp_set_stern on a partition handle, on either side of a multilevel link, attaching a coarse level to a handle with the option
    on, an ensemble with such a member (at create and at a later call), bad options, and the calls that need the option on."""
    from ctypes import byref
    from gmpnp_amd import dist
    from gmpnp_amd.problem import pore_hierarchy
    from gmpnp_amd.solver import GMPNPSystem
    pp, mesh, prob3, _ = pore10
    ep, m1 = edl_k
    stern3, stern1 = SternLayer("BDM", -1.0, L_STERN / 10e-9), SternLayer("BDM", -5.0, L_STERN / ep.L_n)
    prob1 = edl_problem(ep, m1)

    def refused(call, what="Stern"):
        with pytest.raises(gpu_lib.GmpnpError, match=what) as ei:
            call()
        assert ei.value.code == gpu_lib.ERR_INVALID

    dom, perm, part = dist.partition_plan(prob3, 2, 0)
    with gpu_lib.DeviceSolver(dom.problem, perm=perm, partition=part) as partitioned:
        refused(lambda: partitioned.set_stern(stern3))
        partitioned.set_stern(None)                                    # off is always accepted
    levels = pore_hierarchy(pp, mesh, 1)
    ml = GMPNPSystem(levels[0][0], levels=levels)
    try:
        refused(lambda: ml.dev.set_stern(stern3))
        refused(lambda: ml._coarse[0].set_stern(stern3))
    finally:
        ml.close()
    with gpu_lib.DeviceSolver(levels[0][0]) as fine, gpu_lib.DeviceSolver(levels[1][0], shared_device=1) as coarse:
        fine.set_stern(stern3)
        refused(lambda: fine.attach_coarse_level(coarse, levels[0][2]))
    with gpu_lib.DeviceSolver(prob1) as a, gpu_lib.DeviceSolver(prob1) as b:
        u0, un = first_step_state(prob1)
        for d in (a, b):
            d.set_state(u0, un)
        refused(lambda: a.time_kernel(24, 1))
        refused(lambda: a.stern_displacement())
        with gpu_lib.DeviceEnsemble([a, b]) as ens:
            b.set_stern(stern1)
            refused(lambda: ens.newton_solve(gpu_lib.newton_options(SP_FIRST, dim=1)))
            refused(lambda: ens.set_time_step([1.0, 1.0]))
            refused(lambda: ens.assign_previous())
            refused(lambda: ens.get_state())
            b.set_stern(None)
        b.set_stern(stern1)
        refused(lambda: gpu_lib.DeviceEnsemble([a, b]))
        for bad in (gpu_lib.CStern(3, -5.0, 1e-3, 6.0), gpu_lib.CStern(2, -5.0, 0.0, 6.0), gpu_lib.CStern(2, -5.0, 1e-3, 0.0),
                    gpu_lib.CStern(1, float("nan"), 1e-3, 6.0)):
            code = a.lib.gmpnp_set_stern(a._h, byref(bad))
            assert code == gpu_lib.ERR_INVALID and "Stern" in a.lib.gmpnp_last_error().decode()
        b.assemble(True)
        assert b.time_kernel(24, 2) > 0.0
        refused(lambda: b.jacobian_csr(), "no Jacobian")                # the timed launches added their entries again: not a Jacobian


def _metadata_of(tmp_path):
    found = [os.path.join(d, "metadata.json") for d, _, files in os.walk(str(tmp_path)) if "metadata.json" in files]
    assert len(found) == 1, found
    return found[0], json.load(open(found[0]))


def test_command_line_1d(gpu_lib, tmp_path):
    """1D/MPNP_CO2ER_EDL.py --electrode_voltage ...: the metadata keys, potential_OHP as a result, the directory named by the electrode."""
    env = dict(os.environ, GMPNP_OUT=str(tmp_path))
    cmd = [sys.executable, os.path.join(ROOT, "1D", "MPNP_CO2ER_EDL.py"), "--L_n=1e-6", "--electrode_voltage=-5", "--stern_model=linear", "--num_steps=2",
           "--budget"]
    subprocess.run(cmd, check=True, env=env, cwd=str(tmp_path), stdout=subprocess.DEVNULL)
    path, meta = _metadata_of(tmp_path)
    assert "electrode_-5.0_linear" in path
    assert meta["electrode_voltage"] == -5.0 and meta["stern_model"] == "linear" and abs(meta["stern_length"] - 4e-10) < 1e-24
    assert meta["stern_displacement"] < 0.0 and meta["surface_charge"] < 0.0
    assert -5.0 * 0.0257 < meta["potential_OHP"] < 0.0                 # [V]: between the electrode's potential and the bulk's
    both = subprocess.run(cmd + ["--voltage_multiplier=-2"], env=env, cwd=str(tmp_path), capture_output=True, text=True)
    assert both.returncode != 0 and "electrode_voltage takes the place of voltage_multiplier" in both.stderr


def test_command_line_3d(gpu_lib, tmp_path):
    env = dict(os.environ, GMPNP_OUT=str(tmp_path))
    cmd = [sys.executable, os.path.join(ROOT, "3D", "MPNP_CO2ER_pore.py"), "--L=10e-9", "--R=5e-9", "--concentration_elec=0.5", "--num_steps=2",
           "--electrode_voltage=-1", "--step_fraction=0.9"]
    subprocess.run(cmd, check=True, env=env, cwd=str(tmp_path), stdout=subprocess.DEVNULL)
    path, meta = _metadata_of(tmp_path)
    assert "electrode_-1.0_BDM" in path
    assert meta["electrode_voltage"] == -1.0 and meta["stern_model"] == "BDM" and abs(meta["stern_length"] - 4e-10) < 1e-24
    assert meta["stern_displacement"] < 0.0 and meta["surface_charge"] < 0.0 and meta["num_steps_run"] == 2
    z = np.load(os.path.join(os.path.dirname(path), "arrays_unscaled.npz"))
    assert -1.0 < z["p"][-1].min() < 0.0
