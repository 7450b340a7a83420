"""GPU parity tests: every call goes through the C-ABI of libgmpnp.so (gmpnp_amd.backend) and is compared with the
CPU oracle on the same seeded inputs, or with the committed golden vectors (tests/golden) at full size.

Stated tolerances (fp64 everywhere):
  assembly / SpMV vs oracle ................ 1e-12 relative (different summation order only)
  linear solve vs sparse LU ................ 1e-8  relative (BiCGStab at 1e-10 relative residual)
  Newton iterates / time steps vs oracle ... 1e-8  relative, identical Newton iteration counts
"""
import copy
import os

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import gmpnp_oracle as O
from conftest import GOLDEN, random_state
from golden_cases import EXTRA_EDL, EXTRA_PORE, EXTRA_RXN1D, EXTRA_RXN3D

pytestmark = pytest.mark.gpu

MUMPS_09 = {"nonlinear_solver": "newton", "newton_solver": {
    "linear_solver": "mumps", "maximum_iterations": 50, "relative_tolerance": 1e-4, "absolute_tolerance": 1e-4,
    "relaxation_parameter": 0.9}}
DEFAULT_1D = {"nonlinear_solver": "newton", "newton_solver": {
    "maximum_iterations": 50, "relative_tolerance": 1e-4, "absolute_tolerance": 1e-4}}


def relerr(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def frob_rel(A, B):
    D = (A - B).tocsr()
    return np.sqrt((D.data ** 2).sum()) / np.sqrt((B.data ** 2).sum())


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["pore10", "pore50", "edl1", "edl50"])
def test_assembly_matches_oracle(case, request, gpu_lib):
    fx = request.getfixturevalue(case)
    prob = fx[2]
    nv, ns = prob.coords.shape[0], prob.nf - 1
    u, un = random_state(nv, ns, seed=3)
    with gpu_lib.DeviceSolver(prob) as dev:
        dev.set_state(u, un)
        F, nrm = dev.assemble(True)
        A = dev.jacobian_csr()
        # a second assembly is bitwise reproducible (gather assembly, no atomics)
        F2, _ = dev.assemble(True)
        assert np.array_equal(F, F2) and np.array_equal(A.data, dev.jacobian_csr().data)
    Fo, Ao = O.assemble(prob, u, un)
    assert relerr(F, Fo) < 1e-12
    assert abs(nrm - np.linalg.norm(Fo)) / np.linalg.norm(Fo) < 1e-12
    assert A.nnz == Ao.nnz and np.array_equal(A.indptr, Ao.indptr) and np.array_equal(A.indices, Ao.indices)
    assert frob_rel(A, Ao) < 1e-12
    d = prob.bc_dofs
    assert np.array_equal(F[d], u[d] - prob.bc_vals)  # b = x - g exactly
    assert np.all(A.diagonal()[d] == 1.0) and abs(A[d]).sum() == len(d)  # identity rows exactly


def test_assembly_as_published_variant(pore10, gpu_lib):
    """without the ds(2)/ds(3) terms (what the published script assembles)."""
    from gmpnp_amd.params import pore_parameters
    from gmpnp_amd.problem import pore_problem
    pp = pore_parameters(concentration_elec=0.5, L=10e-9, R=5e-9, as_published=True)
    prob, _ = pore_problem(pp, pore10[1])
    u, un = random_state(prob.coords.shape[0], 8, seed=4)
    with gpu_lib.DeviceSolver(prob) as dev:
        dev.set_state(u, un)
        F, _ = dev.assemble(True)
        A = dev.jacobian_csr()
    Fo, Ao = O.assemble(prob, u, un)
    assert relerr(F, Fo) < 1e-12 and frob_rel(A, Ao) < 1e-12
    Fi, _ = O.assemble(pore10[2], u, un)
    assert relerr(Fo, Fi) > 1e-6  # the flux terms do matter


def test_staged_element_stores_give_the_same_bits(pore10, gpu_lib):
    """The element kernel's two ways of writing its per-cell records (direct stores of one lane per cell; staged through LDS and
    written record by record, the form large meshes take) leave bit-identical residuals and Jacobians — on a mesh whose cell count
    is not a multiple of 64 (the last wave is ragged)."""
    prob = pore10[2]
    assert prob.cells.shape[0] % 64 != 0
    u, un = random_state(prob.coords.shape[0], 8, seed=5)
    out = []
    for mode in (1, 2):
        with gpu_lib.DeviceSolver(prob, element_stores=mode) as dev:
            dev.set_state(u, un)
            F, _ = dev.assemble(True)
            out.append((F, dev.jacobian_csr()))
    assert np.array_equal(out[0][0], out[1][0])
    assert np.array_equal(out[0][1].data, out[1][1].data) and np.array_equal(out[0][1].indices, out[1][1].indices)
    Fo, Ao = O.assemble(prob, u, un)
    assert relerr(out[1][0], Fo) < 1e-12 and frob_rel(out[1][1], Ao) < 1e-12


def test_steric_excursion_is_information_by_default_and_fatal_on_request(pore10, gpu_lib):
    """UFL/FFC evaluate u_i / (1 - S) as it stands (3D:534-750): a state with 1 - S <= 0 at quadrature points assembles like any
    other (negative quotients) — and so it does here, matching the oracle; `strict_steric` brings back the rounds-1-2 error."""
    prob = pore10[2]
    u, un = random_state(prob.coords.shape[0], 8)
    u = u.reshape(-1, 9)
    u[:, 7] = 40.0  # sum_j a_j u_j > 1 everywhere
    with gpu_lib.DeviceSolver(prob) as dev:
        dev.set_state(u.ravel(), un)
        F, _ = dev.assemble(True)
        A = dev.jacobian_csr()
    Fo, Ao = O.assemble(prob, u.ravel(), un)
    assert relerr(F, Fo) < 1e-12 and frob_rel(A, Ao) < 1e-12
    with gpu_lib.DeviceSolver(prob, strict_steric=1) as dev:
        dev.set_state(u.ravel(), un)
        with pytest.raises(gpu_lib.GmpnpError) as ei:
            dev.assemble(True)
        assert ei.value.code == gpu_lib.ERR_NUMERIC


def test_newton_through_a_steric_excursion_follows_the_unguarded_oracle(gpu_lib):
    """1 um mesh, K+, V = -6.25, first solve from the zero state: Newton's third iterate has S = 1.25 at a quadrature point and the
    iteration then CONVERGES (8 iterations) to a root with S = 1.52 — outside the admissible set, but that is what the published
    forms and DOLFIN's Newton do: neither has a test for it (the oracle has none either).  The product follows the oracle iterate by
    iterate and reports the excursion in the statistics; with `strict_steric` it raises instead."""
    from conftest import _edl
    ep, mesh, prob = _edl(L_n=1e-6, voltage_multiplier=-6.25)
    nv = mesh.num_vertices
    u0, un = np.zeros(nv * 7), np.tile(np.r_[np.ones(6), 0.0], nv)
    u_ref, st_ref = O.newton_solve(prob, u0, un, relaxation_parameter=1.0)
    a = np.asarray(prob.model.a)
    assert st_ref.converged and (u_ref.reshape(nv, 7)[:, :6] @ a).max() > 1.2
    opts = gpu_lib.newton_options({"newton_solver": {"maximum_iterations": 50, "relative_tolerance": 1e-4, "absolute_tolerance": 1e-4}}, dim=1)
    with gpu_lib.DeviceSolver(prob) as dev:
        dev.set_state(u0, un)
        st = dev.newton_solve(opts)
        u = dev.get_state()
    assert st["converged"] and st["iterations"] == st_ref.iterations and st["steric_excursion"] == 1
    assert np.allclose(st["residuals"], st_ref.residuals, rtol=1e-5)
    assert relerr(u, u_ref) < 1e-8
    with gpu_lib.DeviceSolver(prob, strict_steric=1) as dev:
        dev.set_state(u0, un)
        with pytest.raises(gpu_lib.GmpnpError) as ei:
            dev.newton_solve(opts)
        assert ei.value.code == gpu_lib.ERR_NUMERIC


def test_spmv_and_linear_solve_3d(pore10, gpu_lib):
    prob = pore10[2]
    nv, ns = prob.coords.shape[0], prob.nf - 1
    u, un = random_state(nv, ns, seed=5)
    rng = np.random.default_rng(6)
    x = rng.standard_normal(prob.ndof)
    Fo, Ao = O.assemble(prob, u, un)
    xo = spla.splu(Ao.tocsc()).solve(Fo)
    with gpu_lib.DeviceSolver(prob) as dev:
        dev.set_state(u, un)
        dev.assemble(True)
        assert relerr(dev.spmv(x), Ao @ x) < 1e-13
        # linearity of the device operator
        y1, y2 = dev.spmv(x), dev.spmv(2.5 * x)
        assert relerr(y2, 2.5 * y1) < 1e-15
        xs, st = dev.linear_solve(Fo, gpu_lib.LINEAR_TWOLEVEL, 1e-10, 0.0, 5000)
        assert st["converged"] and relerr(Ao @ xs, Fo) < 2e-10 and relerr(xs, xo) < 1e-6
        xj, stj = dev.linear_solve(Fo, gpu_lib.LINEAR_JACOBI, 1e-10, 0.0, 20000)
        # ||x - x*|| <= cond(J) * residual: on this random (unphysical) state only the residual is tight
        assert stj["converged"] and relerr(Ao @ xj, Fo) < 2e-10 and relerr(xj, xo) < 1e-3
        assert stj["iterations"] > 3 * st["iterations"]  # the coarse correction pays
        # zero right-hand side
        xz, stz = dev.linear_solve(np.zeros(prob.ndof), gpu_lib.LINEAR_TWOLEVEL, 1e-10, 0.0, 100)
        assert not xz.any() and stz["iterations"] == 0
        # iteration limit reached -> status, not garbage
        with pytest.raises(gpu_lib.GmpnpError) as ei:
            dev.linear_solve(Fo, gpu_lib.LINEAR_JACOBI, 1e-14, 0.0, 3)
        assert ei.value.code == gpu_lib.ERR_LINEAR
        with pytest.raises(gpu_lib.GmpnpError) as ei:
            dev.linear_solve(Fo, gpu_lib.LINEAR_BLOCK_TRIDIAGONAL)
        assert ei.value.code == gpu_lib.ERR_INVALID


@pytest.mark.parametrize("case", ["edl1", "edl50"])
def test_spmv_and_direct_solve_1d(case, request, gpu_lib):
    """Block cyclic reduction against SciPy's sparse LU on the 1D Jacobian (q ~ 4e5 ... 1e9)."""
    prob = request.getfixturevalue(case)[2]
    nv = prob.coords.shape[0]
    g = np.load(os.path.join(GOLDEN, case + "_steps.npz"))
    u, un = g["states"][1], g["states"][0]  # a physical state: second dry-run step
    rng = np.random.default_rng(6)
    x = rng.standard_normal(prob.ndof)
    Fo, Ao = O.assemble(prob, u, un)
    b = rng.standard_normal(prob.ndof)
    lu = spla.splu(Ao.tocsc())
    with gpu_lib.DeviceSolver(prob) as dev:
        dev.set_state(u, un)
        dev.assemble(True)
        assert relerr(dev.spmv(x), Ao @ x) < 1e-13
        for rhs in (Fo, b):
            xs, st = dev.linear_solve(rhs, gpu_lib.LINEAR_BLOCK_TRIDIAGONAL)
            xo = lu.solve(rhs)
            assert st["converged"] and relerr(xs, xo) < 1e-8


def test_newton_first_step_matches_oracle(pore10, gpu_lib):
    pp, mesh, prob, bnd = pore10
    g = np.load(os.path.join(GOLDEN, "pore10_steps.npz"))
    nv = mesh.num_vertices
    u0, un = np.zeros(prob.ndof), np.tile(np.r_[np.ones(8), 0.0], nv)
    with gpu_lib.DeviceSolver(prob) as dev:
        dev.set_state(u0, un)
        st = dev.newton_solve(gpu_lib.newton_options(MUMPS_09))
        u = dev.get_state()
        # the relative test is relative to the entry residual of EACH solve, so a second solve iterates until the
        # absolute test passes; a third one then performs 0 iterations (the test runs before the first iteration)
        st1 = dev.newton_solve(gpu_lib.newton_options(MUMPS_09))
        assert st1["residuals"][0] == pytest.approx(st["residuals"][-1], rel=1e-12) and st1["residuals"][-1] < 1e-4
        u1 = dev.get_state()
        st0 = dev.newton_solve(gpu_lib.newton_options(MUMPS_09))
        assert st0["iterations"] == 0 and st0["converged"] and np.array_equal(dev.get_state(), u1)
    assert st["iterations"] == int(g["newton_its"][0]) == 7
    ref = g["residuals"][0][:8]
    # (the early iterates sit on the ill-conditioned Jacobian of the zero state: BiCGStab at 1e-10 against the oracle's sparse LU
    # leaves their residuals 1e-7 apart; the converged state is what is pinned tightly)
    assert np.allclose(st["residuals"], ref, rtol=1e-6)
    assert relerr(u, g["states"][0]) < 1e-8
    assert abs(st["residuals"][0] - ref[0]) / ref[0] < 1e-13  # ||b0|| is dominated by the bc rows (~1.2e3)


def test_newton_nonconvergence_is_an_error(pore10, gpu_lib):
    prob = pore10[2]
    nv = prob.coords.shape[0]
    sp = copy.deepcopy(MUMPS_09)
    sp["newton_solver"]["maximum_iterations"] = 2
    from gmpnp_amd.solver import GMPNPSystem
    s = GMPNPSystem(prob)
    try:
        s.initialise([1.0] * 8 + [0.0])
        with pytest.raises(RuntimeError, match="did not converge"):
            s.solve(sp)
        st = s.dev.newton_solve(gpu_lib.newton_options(sp), error_on_nonconvergence=False)
        assert st["iterations"] == 2 and not st["converged"]
    finally:
        s.close()


BAND_09 = {"nonlinear_solver": "newton", "newton_solver": dict(MUMPS_09["newton_solver"], linear_solver="band_lu")}


def test_band_lu_matches_sparse_lu(pore10, gpu_lib):
    """The 3D direct solver (block-banded LU in slab order) against SciPy's sparse LU on the oracle's Jacobian."""
    prob = pore10[2]
    u, un = random_state(prob.coords.shape[0], prob.nf - 1, seed=5)
    Fo, Ao = O.assemble(prob, u, un)
    lu = spla.splu(Ao.tocsc())
    rng = np.random.default_rng(8)
    with gpu_lib.DeviceSolver(prob) as dev:
        dev.set_state(u, un)
        dev.assemble(True)
        for rhs in (Fo, rng.standard_normal(prob.ndof)):
            x, st = dev.linear_solve(rhs, gpu_lib.LINEAR_BAND_LU)
            # refinement stops at the requested 1e-10 relative residual; on this random (unphysical) state
            # ||x|| ~ 3e4 ||b||, so the solution error is looser than the residual
            assert st["converged"] and relerr(Ao @ x, rhs) < 2e-10 and relerr(x, lu.solve(rhs)) < 1e-6
            x2, _ = dev.linear_solve(rhs, gpu_lib.LINEAR_BAND_LU)
            assert np.array_equal(x, x2)  # no atomics, fixed elimination order
        xz, _ = dev.linear_solve(np.zeros(prob.ndof), gpu_lib.LINEAR_BAND_LU)
        assert not xz.any()


@pytest.mark.parametrize("rings,layers", [(1, 1), (1, 4), (2, 5)])
def test_band_lu_on_meshes_smaller_than_a_substitution_panel(rings, layers, gpu_lib):
    """Generated cylinders of 14 / 35 / 114 vertices: fewer block rows than one 16-row panel of the substitution, a band narrower
    than a panel (the library widens the stored band to 15 blocks), a last panel of 3 rows — against SciPy's sparse LU."""
    import closed_forms as cf
    prob = cf._base(10e-9, 5e-9, 0, reactions=True, wall_flux=True, steady=False, q_scale=1.0, coarse=(rings, layers))[0]
    nv = prob.coords.shape[0]
    assert nv == (1 + 3 * rings * (rings + 1)) * (layers + 1)
    u, un = random_state(nv, prob.nf - 1, seed=11)
    Fo, Ao = O.assemble(prob, u, un)
    lu = spla.splu(Ao.tocsc())
    with gpu_lib.DeviceSolver(prob) as dev:
        dev.set_state(u, un)
        dev.assemble(True)
        for rhs in (Fo, np.random.default_rng(3).standard_normal(prob.ndof)):
            x, st = dev.linear_solve(rhs, gpu_lib.LINEAR_BAND_LU)
            # the library stops at 1e-10 against ITS matrix; ||x|| ~ 1e4 ||b|| on these random states, so the oracle's matrix
            # (equal to 1e-13) sees a residual of up to 1e-9
            assert st["converged"] and relerr(Ao @ x, rhs) < 5e-9 and relerr(x, lu.solve(rhs)) < 1e-6
            x2, _ = dev.linear_solve(rhs, gpu_lib.LINEAR_BAND_LU)
            assert np.array_equal(x, x2)


def test_band_lu_is_3d_only(edl1, gpu_lib):
    prob = edl1[2]
    with gpu_lib.DeviceSolver(prob) as dev:
        dev.set_state(np.zeros(prob.ndof), np.zeros(prob.ndof))
        dev.assemble(True)
        with pytest.raises(gpu_lib.GmpnpError) as ei:
            dev.linear_solve(np.ones(prob.ndof), gpu_lib.LINEAR_BAND_LU)
        assert ei.value.code == gpu_lib.ERR_INVALID
    # ... and the name maps to the 1D direct solver there
    assert gpu_lib.newton_options(BAND_09, dim=1).linear_solver == gpu_lib.LINEAR_BLOCK_TRIDIAGONAL


@pytest.mark.parametrize("case,L,nsteps", [("pore10", 10e-9, 2), ("pore50", 50e-9, 1)])
def test_newton_with_band_lu_matches_golden(case, L, nsteps, gpu_lib, monkeypatch):
    """'mumps' read literally: every Newton system solved by the direct solver; same iterates as the golden steps
    (pore50 = the north-star mesh, selected there through GMPNP_3D_DIRECT=1 and the reference's own parameter dict)."""
    from gmpnp_amd.pore3d import PoreRun
    g = np.load(os.path.join(GOLDEN, case + "_steps.npz"))
    if case == "pore50":
        monkeypatch.setenv("GMPNP_3D_DIRECT", "1")   # read by the Python option translation (backend.newton_options)
    run = PoreRun(num_steps=nsteps, concentration_elec=0.5, L=L, R=5e-9, solver_parameters=BAND_09 if case == "pore10" else None)
    try:
        for k in range(nsteps):
            st = run.step(verbose=False)
            assert st["direct_solves"] == st["iterations"] == int(g["newton_its"][k]) and st["krylov_iterations"] == 0
            assert relerr(run.history[k + 1].ravel(), g["states"][k]) < 1e-8
    finally:
        run.sys.close()


def test_krylov_failure_falls_back_to_band_lu(pore10, gpu_lib, monkeypatch):
    """The reference's linear solver is direct and cannot fail to converge; a BiCGStab solve that does (here: an
    iteration cap of 3) hands the system to the block-banded LU, and the Newton iterates stay those of the golden
    steps.  gmpnp_options_t.no_direct_fallback turns the failure back into the error it used to be."""
    from gmpnp_amd.solver import GMPNPSystem
    prob = pore10[2]
    g = np.load(os.path.join(GOLDEN, "pore10_steps.npz"))
    sp = copy.deepcopy(MUMPS_09)
    sp["newton_solver"]["krylov_solver"] = {"maximum_iterations": 3}
    s = GMPNPSystem(prob)
    try:
        s.initialise([1.0] * 8 + [0.0])
        st = s.solve(sp)
        assert st["iterations"] == int(g["newton_its"][0]) and st["direct_solves"] == st["iterations"]
        assert relerr(s.dev.get_state(), g["states"][0]) < 1e-8
    finally:
        s.close()
    s = GMPNPSystem(prob, no_direct_fallback=1)
    try:
        s.initialise([1.0] * 8 + [0.0])
        with pytest.raises(RuntimeError, match="BiCGStab stopped without convergence"):
            s.solve(sp)
    finally:
        s.close()


@pytest.mark.parametrize("case,nsteps", [("pore10", 3), ("pore50", 2)])
def test_pore_time_loop_matches_golden(case, nsteps, gpu_lib):
    """The driver's loop (Newton, median -> Sechenov -> new bc4, u_n.assign(u)) against the oracle's golden steps."""
    from gmpnp_amd.pore3d import PoreRun
    g = np.load(os.path.join(GOLDEN, case + "_steps.npz"))
    _, L, R = g["args"]
    run = PoreRun(num_steps=nsteps, concentration_elec=0.5, L=float(L), R=float(R))
    try:
        run.run(verbose=False)
        assert run.newton_its == list(g["newton_its"][:nsteps])
        for k in range(nsteps):
            assert relerr(run.history[k + 1].ravel(), g["states"][k]) < 1e-8
        co2 = run.problem.bc_vals[np.searchsorted(run.problem.bc_dofs, run.bnd.dirichlet_vertices[1][0] * 9 + 4)]
        assert abs(co2 - g["co2_bc"][nsteps - 1]) / co2 < 1e-9
        assert run.history[0][:, :8].min() == 1.0 and not run.history[0][:, 8].any()
    finally:
        run.sys.close()


@pytest.mark.parametrize("case", sorted(EXTRA_PORE))
def test_pore_flag_surface_matches_golden(case, gpu_lib):
    """Other corners of the 3D CLI (bulk file, published form at a higher voltage, pore length, H2_FE / current)."""
    from gmpnp_amd.pore3d import PoreRun
    kw, nsteps = EXTRA_PORE[case]
    g = np.load(os.path.join(GOLDEN, case + "_steps.npz"))
    run = PoreRun(num_steps=nsteps, **kw)
    try:
        run.run(verbose=False)
        assert run.newton_its == list(g["newton_its"][:nsteps])
        for k in range(nsteps):
            assert relerr(run.history[k + 1].ravel(), g["states"][k]) < 1e-8
        assert abs(run.co2_bc - g["co2_bc"][nsteps - 1]) / run.co2_bc < 1e-9
    finally:
        run.sys.close()


@pytest.mark.parametrize("case", sorted(EXTRA_EDL))
def test_edl_flag_surface_matches_golden(case, gpu_lib):
    """Other corners of the 1D CLI (PNP model, Li / Na hydration numbers, mesh length, the H_OHP flux controller)."""
    from gmpnp_amd.edl1d import EDLRun
    kw, nsteps = EXTRA_EDL[case]
    g = np.load(os.path.join(GOLDEN, case + "_steps.npz"))
    run = EDLRun(num_steps=nsteps, **kw)
    try:
        run.run(verbose=False)
        assert run.newton_its == list(g["newton_its"][:nsteps])
        for k in range(nsteps):
            assert relerr(run.history[k + 1].ravel(), g["states"][k]) < 1e-8
    finally:
        run.sys.close()


@pytest.mark.parametrize("case,kw,nsteps", [("edl1", dict(L_n=1e-6, cation="Cs", voltage_multiplier=-5.0), 5),
                                             ("edl50", dict(cation="Cs", voltage_multiplier=-10.0), 3)])
def test_edl_time_loop_matches_golden(case, kw, nsteps, gpu_lib):
    from gmpnp_amd.edl1d import EDLRun
    g = np.load(os.path.join(GOLDEN, case + "_steps.npz"))
    run = EDLRun(num_steps=nsteps, **kw)
    try:
        run.run(verbose=False)
        assert run.newton_its == list(g["newton_its"][:nsteps])
        for k in range(nsteps):
            assert relerr(run.history[k + 1].ravel(), g["states"][k]) < 1e-8
    finally:
        run.sys.close()


@pytest.mark.parametrize("which", ["pore50", "edl50", "pore10"])
def test_device_projection_matches_the_oracle(which, pore50, pore10, edl50, gpu_lib):
    """gmpnp_project_gradient / gmpnp_project_cellwise (mass-matrix CG on the device; reference 1D:802-805, 3D:884-909,
    1D:599,651-653) against the oracle's sparse-LU projection: `field_values` and every `<X>_grad` the 3D driver writes,
    to 1e-10 of the field's magnitude, on a converged state of the north-star mesh and on the graded 1D mesh."""
    if which == "edl50":
        ep, mesh, prob = edl50
        g = np.load(os.path.join(GOLDEN, "edl50_steps.npz"))
    else:
        pp, mesh, prob, _ = pore50 if which == "pore50" else pore10
        g = np.load(os.path.join(GOLDEN, which + "_steps.npz"))
    nv, nf = mesh.num_vertices, prob.nf
    state = g["states"][-1].reshape(nv, nf)
    rng = np.random.default_rng(4)
    with gpu_lib.DeviceSolver(prob) as dev:
        for i in range(nf):
            for sign in ((-1.0,) if i == nf - 1 else (1.0,)):
                got = dev.project_gradient(state[:, i], sign=sign)
                ref = O.project_gradient(mesh.coords, mesh.cells, state[:, i], sign=sign)
                assert got.shape == ref.shape
                assert np.abs(got - ref).max() <= 1e-10 * max(np.abs(ref).max(), 1e-30), (which, i)
        assert dev.last_projection_iterations < 80
        vals = rng.uniform(0.5, 2.0, len(mesh.cells))
        assert np.abs(dev.project_cellwise(vals) - O.project_cellwise(mesh.coords, mesh.cells, vals)).max() < 1e-12
        assert np.allclose(dev.project_cellwise(np.full(len(mesh.cells), 3.0)), 3.0, rtol=1e-13)   # constants are reproduced
        d = mesh.coords.shape[1]
        slope = np.array([2.0, 0.0, -0.5])[:d] if d == 3 else np.array([1.5])
        gl = dev.project_gradient(mesh.coords @ slope + 1.0)       # a P1 function: its projected gradient is the constant slope
        assert np.allclose(gl, slope[None, :], atol=1e-8)


def test_bench_window_matches_golden(gpu_lib):
    """bench.py's metric is a COUNT of Newton iterations over time steps 0..49 of BASELINE configs[2]: the GPU's
    BiCGStab@1e-10 solves must give the direct-solve oracle's count at EVERY step of that window, its residual history,
    its Sechenov feedback and its states (tests/golden/pore50_window.npz, tools/make_golden_window.py)."""
    from gmpnp_amd.pore3d import PoreRun
    g = np.load(os.path.join(GOLDEN, "pore50_window.npz"))
    nsteps = len(g["newton_its"])
    assert nsteps == 50
    run = PoreRun(num_steps=nsteps, concentration_elec=0.5, L=50e-9, R=5e-9)
    try:
        co2, res = [], []
        for k in range(nsteps):
            st = run.step(verbose=False)
            co2.append(run.co2_bc)
            res.append(st["residuals"])
        assert run.newton_its == [int(v) for v in g["newton_its"]]
        assert int(np.sum(run.newton_its)) == int(g["newton_its"].sum())
        H = np.array(run.history[1:])                      # (steps, nv, 9)
        assert np.allclose(np.array(co2), g["co2_bc"], rtol=1e-9, atol=0)
        for k in range(nsteps):
            gr = g["residuals"][k][: len(res[k])]
            # residual norms: the entries that decide the stopping test sit at 1e-4 relative, where the 1e-10 linear
            # solves leave ~1e-6 relative differences
            assert len(res[k]) == int(np.sum(np.isfinite(g["residuals"][k]))) and np.allclose(res[k], gr, rtol=1e-4), k
        assert relerr(H[:, g["probes"], :].ravel(), g["probe_values"].ravel()) < 1e-8
        assert np.allclose(np.sqrt((H ** 2).sum(axis=1)), g["field_norms"], rtol=1e-8)
        for k, full in zip(g["full_steps"], g["full_states"]):
            assert relerr(H[int(k)].ravel(), full) < 1e-8
    finally:
        run.sys.close()


def test_config0_diverges_on_the_gpu_as_in_the_oracle(gpu_lib):
    """BASELINE configs[0] (1 um mesh, Cs, V = -10): the undamped Newton of the first time step fails on the GPU as it
    does in the oracle (tests/test_oracle.py::test_config0_first_newton_solve_diverges_in_the_oracle); the driver raises
    the RuntimeError DOLFIN raises.  V = -5 on the same mesh converges (golden edl1)."""
    from gmpnp_amd.edl1d import EDLRun
    run = EDLRun(num_steps=1, L_n=1e-6, cation="Cs", voltage_multiplier=-10.0)
    try:
        with pytest.raises(RuntimeError):
            run.step(verbose=False)
    finally:
        run.sys.close()


def test_sweep_radius_7p5_inherits_the_mesh_name_bug(gpu_lib):
    """configs[4] lists R = 7.5 nm; the reference builds 'L_50_R_7.xml' with int() (3D:330-331), a file that
    does not exist: same failure here, before anything touches the GPU."""
    from gmpnp_amd.pore3d import PoreRun
    with pytest.raises((FileNotFoundError, OSError, RuntimeError), match="L_50_R_7"):
        PoreRun(num_steps=1, concentration_elec=0.5, L=50e-9, R=7.5e-9)


def test_full_size_properties(pore50, gpu_lib):
    """Size-independent properties on the north-star mesh: Newton reduces the residual monotonically once the bc rows
    are absorbed, the update direction satisfies J dx = b, two handles give bitwise-identical results, and the driver
    state round-trips through the file-order permutation."""
    pp, mesh, prob, _ = pore50
    nv = mesh.num_vertices
    u, un = random_state(nv, 8, seed=7)
    with gpu_lib.DeviceSolver(prob) as a, gpu_lib.DeviceSolver(prob) as b:
        for d in (a, b):
            d.set_state(u, un)
        assert np.array_equal(a.get_state(), u) and np.array_equal(a.get_state(previous=True), un)
        Fa, na = a.assemble(True)
        Fb, nb = b.assemble(True)
        assert np.array_equal(Fa, Fb) and na == nb
        xa, sta = a.linear_solve(Fa)
        xb, stb = b.linear_solve(Fb)
        assert np.array_equal(xa, xb) and sta == stb  # deterministic reductions, no atomics
        assert relerr(a.spmv(xa), Fa) < 2e-10
        a.set_state(np.zeros(prob.ndof), np.tile(np.r_[np.ones(8), 0.0], nv))
        st = a.newton_solve(gpu_lib.newton_options(MUMPS_09))
        r = np.array(st["residuals"])
        assert st["converged"] and np.all(r[2:] < r[1:-1])
        assert np.allclose(r[3:] / r[2:-1], 0.1, rtol=0.25)  # omega = 0.9: error x0.1 per iteration near the solution
        assert a.n_aggregates == 8 and a.jacobian_nnz == 3931821


def test_dirichlet_and_model_updates(pore10, gpu_lib):
    pp, mesh, prob, bnd = pore10
    from gmpnp_amd.problem import pore_dirichlet
    u, un = random_state(mesh.num_vertices, 8, seed=8)
    p2 = copy.copy(prob)
    p2.bc_dofs, p2.bc_vals = pore_dirichlet(pp, bnd, 3.21)
    m2 = copy.deepcopy(prob.model)
    m2.inv_dt *= 7.0
    m2.exit_kappa = m2.exit_kappa * 2.0
    p3 = copy.copy(p2)
    p3.model = m2
    with gpu_lib.DeviceSolver(prob) as dev:
        dev.set_state(u, un)
        dev.set_dirichlet(p2.bc_dofs, p2.bc_vals)
        F, _ = dev.assemble(True)
        Fo, Ao = O.assemble(p2, u, un)
        assert relerr(F, Fo) < 1e-12
        dev.set_model(m2)
        F, _ = dev.assemble(True)
        Fo, Ao = O.assemble(p3, u, un)
        assert relerr(F, Fo) < 1e-12 and frob_rel(dev.jacobian_csr(), Ao) < 1e-12


def test_invalid_arguments(pore10, gpu_lib):
    prob = pore10[2]
    with gpu_lib.DeviceSolver(prob) as dev:
        with pytest.raises(gpu_lib.GmpnpError) as ei:
            dev.set_dirichlet([prob.ndof + 5], [0.0])
        assert ei.value.code == gpu_lib.ERR_INVALID
        with pytest.raises(gpu_lib.GmpnpError):
            dev.jacobian_csr()  # nothing assembled yet
        bad = copy.deepcopy(prob.model)
        bad.species = bad.species[:-1]
        with pytest.raises((gpu_lib.GmpnpError, ValueError, IndexError)):
            dev.set_model(bad)
    p = copy.copy(prob)
    p.cells = prob.cells.copy()
    p.cells[0, 0] = prob.coords.shape[0] + 3
    with pytest.raises(gpu_lib.GmpnpError) as ei:
        gpu_lib.DeviceSolver(p, perm=np.arange(prob.coords.shape[0], dtype=np.int32))
    assert ei.value.code == gpu_lib.ERR_INVALID


def test_driver_outputs(tmp_path, monkeypatch, gpu_lib):
    """Output layout of the 3D and 1D drivers: file names, npz keys, shapes, metadata keys."""
    import json
    monkeypatch.setenv("GMPNP_OUT", str(tmp_path))
    from gmpnp_amd import edl1d, pore3d
    out = pore3d.main(["--L=10e-9", "--R=5e-9", "--concentration_elec=0.5", "--num_steps=2"])
    files = set(os.listdir(out))
    assert {"arrays_unscaled.npz", "arrays_scaled.npz", "metadata.json", "solution_K.pvd", "solution_p.pvd",
            "solution_CO2.pvd"} <= files
    a = np.load(os.path.join(out, "arrays_unscaled.npz"))
    nv = 1767
    assert a["H"].shape == (3, nv) and a["p"].shape == (3, nv) and a["coor"].shape == (nv, 3)
    assert a["field_values"].shape == (3 * nv,) and a["cat_grad"].shape == (3 * nv,) and a["tau"].shape == (2,)
    s = np.load(os.path.join(out, "arrays_scaled.npz"))
    assert {"coor_scaled", "psi", "t_H", "c_cat", "eps_rel", "charge_density", "CO_grad"} <= set(s.files)
    meta = json.load(open(os.path.join(out, "metadata.json")))
    assert {"concentration_elec", "cation", "voltage_multiplier", "H2_FE", "L", "R", "time_step", "total_sim_time",
            "porosity", "tortuosity", "constrictivity", "y_CO2", "press_gas", "pore_geom_multiplier",
            "electrolyte_flow_geom_multiplier", "end_time", "eq_conc_CO", "eq_conc_H2", "current_planar",
            "CO2_min"} <= set(meta)
    assert "v_-1.0_L_10_R_5_P_g_1.0_D_eff_1.0_Re_1.0_rough_150.0" in out
    out1 = edl1d.main(["--L_n=1e-6", "--num_steps=3"])
    a1 = np.load(os.path.join(out1, "arrays_unscaled.npz"))
    assert a1["cat"].shape == (4, 1091) and a1["field_values"].shape == (1091,) and a1["coor"].shape == (1091, 1)
    m1 = json.load(open(os.path.join(out1, "metadata.json")))
    assert {"eps_rel_OHP", "field_OHP", "pH_OHP", "CO2_OHP_frac", "mesh_number", "mesh_structure"} <= set(m1)
    assert "/MPNP/" in out1 and out1.endswith("voltage_-1.0_H2_FE_0.2_current_10.0_H_OHP_None_cation_K")
    # the same 3D run on two mesh partitions writes the same files: the projections of the output stage take global vertex
    # arrays and run on an unpartitioned post-processing handle (PartitionedSystem.project_gradient), not on rank 0's local one
    prun = pore3d.PoreRun(num_steps=2, partition=(2, None), concentration_elec=0.5, L=10e-9, R=5e-9)
    try:
        prun.run(verbose=False)
        outp = prun.write_outputs(stamp="partitioned")
    finally:
        prun.sys.close()
    ap = np.load(os.path.join(outp, "arrays_unscaled.npz"))
    assert set(ap.files) == set(a.files)
    for key in ("p", "cat", "field_values", "cat_grad", "CO2_grad"):
        assert ap[key].shape == a[key].shape
        assert np.abs(ap[key] - a[key]).max() <= 1e-7 * max(1.0, np.abs(a[key]).max()), key


def test_supg_assembly_matches_oracle(edl1, gpu_lib):
    """PNP + SUPG (reference 1D:687-714) with random nodal rho: residual and Jacobian against the oracle; switching the
    terms off restores the plain PNP assembly; 3D handles refuse them."""
    from gmpnp_amd.params import edl_parameters
    from gmpnp_amd.problem import edl_problem
    _, mesh, _ = edl1
    ep = edl_parameters(L_n=1e-6, model="PNP", voltage_multiplier=-2.5)
    prob = edl_problem(ep, mesh)
    nv = mesh.num_vertices
    u, un = random_state(nv, 6, seed=21)
    rng = np.random.default_rng(22)
    rho = rng.uniform(1e-9, 1e-4, (nv, 6)) * (np.asarray(prob.model.z) != 0)[None, :]
    w = np.arange(6, dtype=np.int32)
    w[1] = 0  # OH takes grad(u_H), SURVEY Q7
    F0, A0 = O.assemble(prob, u, un)
    p2 = copy.copy(prob)
    p2.supg_rho, p2.supg_w = rho, w
    Fs, As = O.assemble(p2, u, un)
    assert relerr(Fs, F0) > 1e-6  # the terms are there
    with gpu_lib.DeviceSolver(prob) as dev:
        dev.set_state(u, un)
        dev.set_supg(rho, w)
        F, _ = dev.assemble(True)
        assert relerr(F, Fs) < 1e-12
        J = dev.jacobian_csr()
        assert abs(J - As).max() / abs(As).max() < 1e-12
        x = rng.standard_normal(prob.ndof)
        assert relerr(dev.spmv(x), As @ x) < 1e-12
        dev.set_supg(None)
        F, _ = dev.assemble(True)
        assert relerr(F, F0) < 1e-12 and abs(dev.jacobian_csr() - A0).max() / abs(A0).max() < 1e-12
        with pytest.raises(gpu_lib.GmpnpError):
            dev.set_supg(-rho, w)


@pytest.mark.parametrize("case", sorted(EXTRA_RXN1D))
def test_rxn_diff_1d_matches_golden(case, tmp_path, monkeypatch, gpu_lib):
    """Reference 1D/rxn_diff_planar.py on the same kernels (valences 0, steric off, potential pinned by its Dirichlet
    ends): Newton counts and states against the oracle's golden steps, then the driver's output files."""
    import json
    from gmpnp_amd.rxndiff1d import RxnDiffRun
    kw, nsteps = EXTRA_RXN1D[case]
    g = np.load(os.path.join(GOLDEN, case + "_steps.npz"))
    run = RxnDiffRun(num_steps=nsteps, **kw)
    try:
        run.run(verbose=False)
        assert run.newton_its == list(g["newton_its"][:nsteps])
        nv = run.mesh.num_vertices
        for k in range(nsteps):
            ref = g["states"][k].reshape(nv, 7)
            assert relerr(run.history[k + 1].ravel(), ref[:, :5].ravel()) < 1e-8
        full = run.sys.vertex_values()
        assert np.allclose(full[:, 5], 1.0, rtol=0, atol=1e-12) and np.abs(full[:, 6]).max() < 1e-12  # cation placeholder, potential
        monkeypatch.setenv("GMPNP_OUT", str(tmp_path))
        out = run.write_outputs()
    finally:
        run.sys.close()
    a = np.load(os.path.join(out, "arrays_unscaled.npz"))
    assert a["OH"].shape == (nsteps + 1, nv) and a["coor_array"].shape == (nv, 1) and a["tau_array"].shape == (nsteps,)
    s = np.load(os.path.join(out, "arrays_scaled.npz"))
    assert {"x", "t_H", "c_H", "t_CO2", "c_CO2", "c_cat"} <= set(s.files)
    assert np.allclose(s["c_cat"], s["c_HCO3"] + 2 * s["c_CO32"] + s["c_OH"] - s["c_H"])
    meta = json.load(open(os.path.join(out, "metadata.json")))
    assert {"concentration_KHCO3", "L_n", "bulk_pH", "time_constant", "total_sim_time", "time_step", "mesh_structure", "H2_FE",
            "CO_FE", "current_OHP_ss", "pH_OHP", "pH_overpotential", "CO2_overpotential", "CO2_OHP_frac"} <= set(meta)


@pytest.mark.parametrize("case", sorted(EXTRA_RXN3D))
def test_rxn_diff_3d_matches_golden(case, tmp_path, monkeypatch, gpu_lib):
    """Reference 3D/rxn_diff_CO2ER_pore.py on the same kernels: Newton counts, states and the Sechenov CO2 value (cation
    from electroneutrality) against the oracle's golden steps, then the driver's output files."""
    import json
    from gmpnp_amd.rxnpore3d import RxnPoreRun
    kw, nsteps = EXTRA_RXN3D[case]
    g = np.load(os.path.join(GOLDEN, case + "_steps.npz"))
    run = RxnPoreRun(num_steps=nsteps, **kw)
    try:
        run.run(verbose=False)
        assert run.newton_its == list(g["newton_its"][:nsteps])
        nv = run.mesh.num_vertices
        for k in range(nsteps):
            ref = g["states"][k].reshape(nv, 9)
            assert relerr(run.history[k + 1].ravel(), ref[:, :7].ravel()) < 1e-8
        assert abs(run.co2_bc - g["co2_bc"][nsteps - 1]) / run.co2_bc < 1e-9
        full = run.sys.vertex_values()
        # cation placeholder: 1 up to what the damped Newton (x0.1 per iteration from u = 0) leaves; potential: pinned
        assert np.allclose(full[:, 7], 1.0, rtol=0, atol=1e-5) and np.abs(full[:, 8]).max() < 1e-10
        monkeypatch.setenv("GMPNP_OUT", str(tmp_path))
        out = run.write_outputs()
    finally:
        run.sys.close()
    files = set(os.listdir(out))
    assert {"arrays_unscaled.npz", "arrays_scaled.npz", "metadata.json", "solution_CO.pvd", "solution_H2.pvd", "solution_CO2.pvd",
            "solution_OH.pvd", "solution_H.pvd", "solution_HCO3.pvd", "solution_CO32.pvd"} <= files
    assert "solution_K.pvd" not in files and "solution_p.pvd" not in files
    a = np.load(os.path.join(out, "arrays_unscaled.npz"))
    assert a["H2"].shape == (nsteps + 1, nv) and a["coor"].shape == (nv, 3) and a["CO_grad"].shape == (3 * nv,)
    assert "cat" not in a.files and "p" not in a.files
    s = np.load(os.path.join(out, "arrays_scaled.npz"))
    assert np.allclose(s["c_cat"], s["c_HCO3"] + 2 * s["c_CO32"] + s["c_OH"] - s["c_H"])
    meta = json.load(open(os.path.join(out, "metadata.json")))
    assert "voltage_multiplier" not in meta and {"eq_conc_CO", "eq_conc_H2", "current_planar", "CO2_min"} <= set(meta)
    assert out.rstrip("/").endswith("L_10_R_5_P_g_1.0_D_eff_1.0_Re_1.0_rough_150.0")


def test_refined_mesh_uses_the_large_mesh_paths(gpu_lib):
    """One uniform refinement of L_10_R_5 (12.9k vertices, 116k dofs): more tiles than resident workgroup slots (four-launch
    iteration) and more tiles per aggregate than the prologues preload (tail loops of the partial sums).  Assembly and
    SpMV against the oracle, the Krylov solve against the oracle matrix, Newton by its contraction property."""
    from gmpnp_amd.mesh import read_dolfin_xml, resolve_mesh_path
    from gmpnp_amd.params import pore_parameters, utilities_dir
    from gmpnp_amd.problem import pore_problem
    pp = pore_parameters(concentration_elec=0.5, L=10e-9, R=5e-9)
    mesh = read_dolfin_xml(resolve_mesh_path(utilities_dir(), pp.mesh_name))
    prob, _ = pore_problem(pp, mesh, refine=1)
    nv = prob.coords.shape[0]
    assert nv > 12000
    u, un = random_state(nv, 8, seed=11)
    Fo, Ao = O.assemble(prob, u, un)
    with gpu_lib.DeviceSolver(prob) as dev:
        assert dev.krylov_launches_per_iteration == 4
        dev.set_state(u, un)
        F, _ = dev.assemble(True)
        assert relerr(F, Fo) < 1e-12
        x = np.random.default_rng(12).standard_normal(prob.ndof)
        assert relerr(dev.spmv(x), Ao @ x) < 1e-13
        xs, st = dev.linear_solve(Fo, gpu_lib.LINEAR_TWOLEVEL, 1e-10, 0.0, 20000)
        assert st["converged"] and relerr(Ao @ xs, Fo) < 1e-8
        dev.set_state(np.zeros(prob.ndof), np.tile(np.r_[np.ones(8), 0.0], nv))
        stn = dev.newton_solve(gpu_lib.newton_options(MUMPS_09))
        r = np.array(stn["residuals"])
        assert stn["converged"] and 5 <= stn["iterations"] <= 9
        assert np.allclose(r[3:] / r[2:-1], 0.1, rtol=0.3)


def _run_pore10(nsteps=3, **options):
    """`options`: fields of gmpnp_options_t (include/gmpnp.h)."""
    from gmpnp_amd.pore3d import PoreRun
    run = PoreRun(num_steps=nsteps, concentration_elec=0.5, L=10e-9, R=5e-9, device_kwargs=options)
    try:
        run.run(verbose=False)
        return np.array(run.history[1:]), list(run.newton_its), run.sys.dev.krylov_launches_per_iteration
    finally:
        run.sys.close()


def test_solver_variants_agree(gpu_lib):
    """The launch form must not change a single bit (same arithmetic, different hand-over); warm starts and coarse reuse
    change the Krylov path only: Newton counts identical, states equal to the linear-solve tolerance."""
    ref, its, launches = _run_pore10()
    assert launches == 2  # L_10_R_5: every workgroup of a launch is resident (occupancy query at create)
    unfused, its_u, launches_u = _run_pore10(launch_form=4)
    assert launches_u == 4 and its_u == its and np.array_equal(unfused, ref)
    shared, its_sh, launches_sh = _run_pore10(shared_device=1)   # no in-launch hand-over, no side stream
    assert launches_sh == 4 and its_sh == its and relerr(shared.ravel(), ref.ravel()) < 1e-8
    cold, its_c, _ = _run_pore10(warm_start=-1, coarse_refresh=1)
    assert its_c == its and relerr(cold.ravel(), ref.ravel()) < 1e-8
    first_order, its_f, _ = _run_pore10(warm_start=1)
    assert its_f == its and relerr(first_order.ravel(), ref.ravel()) < 1e-8
    # materialised vector form (automatic on meshes above 768 MB of matrix): p / s written for all rows by streaming
    # kernels, the tile kernels stage one vector instead of four / two — the same recurrences in other launches
    mat, its_m, launches_m = _run_pore10(vector_form=1)
    assert launches_m == 4 and its_m == its and relerr(mat.ravel(), ref.ravel()) < 1e-8
    with pytest.raises(gpu_lib.GmpnpError, match="vector_form 1"):
        _run_pore10(vector_form=1, launch_form=2)
    # coarse operator rebuilt in the main stream every third iteration instead of on the side stream: another valid
    # preconditioner, same Newton path; and the side-stream scheme is deterministic (events order the two streams)
    sync3, its_s, _ = _run_pore10(coarse_refresh=3)
    assert its_s == its and relerr(sync3.ravel(), ref.ravel()) < 1e-8
    again, its_a, _ = _run_pore10()
    assert its_a == its and np.array_equal(again, ref)
    # how the host learns about progress (pinned mirror or copy + event), how many iterations it queues per poll and
    # whether the phases are timed changes no arithmetic at all
    for opt in (dict(progress_by_copy=1), dict(burst_iterations=3), dict(phase_timing=1), dict(warm_in_stream=1),
                dict(progress_by_copy=1, launch_form=4)):
        other, its_o, _ = _run_pore10(**opt)
        assert its_o == its and np.array_equal(other, ref), opt


def test_in_launch_handover_needs_proven_residency(pore50, gpu_lib):
    """The two-launch form (tile workgroups wait inside the launch for flags raised by the coarse workgroups of the same
    launch) is only enabled when hipOccupancyMaxActiveBlocksPerMultiprocessor x CUs covers the whole grid.  Asking for
    it on the once-refined L_50_R_5 mesh (about 3,700 tiles against at most 3 x 256 resident workgroups) is refused at
    create instead of left to the kernels' time-out; the default falls back to four launches there, and a device
    declared shared never gets the hand-over."""
    pp, mesh, prob, bnd = pore50
    with gpu_lib.DeviceSolver(prob) as dev:
        assert dev.krylov_launches_per_iteration == 2
    with gpu_lib.DeviceSolver(prob, shared_device=1) as dev:
        assert dev.krylov_launches_per_iteration == 4
    with pytest.raises(gpu_lib.GmpnpError, match="launch_form 2 refused"):
        gpu_lib.DeviceSolver(prob, shared_device=1, launch_form=2)
    from gmpnp_amd.problem import pore_problem
    fprob, _ = pore_problem(pp, mesh, refine=1)
    with pytest.raises(gpu_lib.GmpnpError, match="launch_form 2 refused"):
        gpu_lib.DeviceSolver(fprob, launch_form=2)
    with gpu_lib.DeviceSolver(fprob) as dev:
        assert dev.krylov_launches_per_iteration == 4


def test_two_handles_on_one_device_run_concurrently_without_handover_timeouts(pore10, gpu_lib):
    """Two handles driven from two host threads on the same GPU (what `sweep --jobs_per_gpu 2` does): both reach the golden
    steps; a hand-over time-out (status bit 8) would end a BiCGStab solve with an error or send it to the direct fallback."""
    import threading
    from gmpnp_amd.pore3d import PoreRun
    g = np.load(os.path.join(GOLDEN, "pore10_steps.npz"))
    out = {}

    def work(tag):
        run = PoreRun(num_steps=3, concentration_elec=0.5, L=10e-9, R=5e-9, device_kwargs={"shared_device": 1})
        try:
            direct = 0
            for _ in range(3):
                direct += run.step(verbose=False)["direct_solves"]
            out[tag] = (list(run.newton_its), np.array(run.history[1:]), direct)
        except Exception as e:  # noqa: BLE001
            out[tag] = e
        finally:
            run.sys.close()

    th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    [t.start() for t in th]
    [t.join() for t in th]
    for k in range(2):
        assert not isinstance(out[k], Exception), out[k]
        its, hist, direct = out[k]
        assert its == [int(v) for v in g["newton_its"][:3]] and direct == 0
        assert relerr(hist.reshape(3, -1), g["states"][:3]) < 1e-8


def test_non_finite_linear_systems_are_errors_not_answers(pore10, gpu_lib):
    """A NaN right-hand side or matrix must end in GMPNP_ERR_LINEAR / GMPNP_ERR_NUMERIC, never in `converged` with a
    NaN update (the true residual of a 'converged' recurrence used to be accepted when it was NaN)."""
    pp, mesh, prob, _ = pore10
    u, un = random_state(mesh.num_vertices, 8, seed=5)
    with gpu_lib.DeviceSolver(prob, no_direct_fallback=1) as dev:
        dev.set_state(u, un)
        dev.assemble(True)
        b = np.ones(prob.ndof)
        b[17] = np.nan
        with pytest.raises(gpu_lib.GmpnpError) as ei:
            dev.linear_solve(b)
        assert ei.value.code in (gpu_lib.ERR_LINEAR, gpu_lib.ERR_NUMERIC)
        b[17] = np.inf
        with pytest.raises(gpu_lib.GmpnpError):
            dev.linear_solve(b)
        ubad = u.copy()
        ubad[9 * 40 + 2] = np.nan   # NaN state -> NaN residual: Newton must stop with a numeric error
        dev.set_state(ubad, un)
        with pytest.raises(gpu_lib.GmpnpError) as ei:
            dev.newton_solve(gpu_lib.newton_options(MUMPS_09))
        assert ei.value.code in (gpu_lib.ERR_LINEAR, gpu_lib.ERR_NUMERIC)


# field_OHP [V/nm] and eps_rel_OHP "obtained from solving the MPNP code", reference 1D/Stern_CO2ER.py:66-68 — the only
# outputs of the hot path the reference holds.  Configuration (not stated there, verified in SURVEY §8c): the 1D
# defaults, K+, 0.1 M KHCO3, MPNP, 50 um mesh.
STERN_OHP = {-2.5: (-0.08032108300135771, 74.56149297894756), -5.0: (-0.2524415478848975, 57.64572780716129),
             -7.5: (-0.4612956299192668, 50.16243860179017), -10.0: (-0.6149631587776277, 49.311548142969336),
             -12.5: (-0.7310301485096051, 49.2556833480052)}


@pytest.mark.parametrize("voltage", sorted(STERN_OHP))
def test_reference_recorded_ohp_field_and_permittivity(voltage, tmp_path, monkeypatch, gpu_lib):
    """End-to-end pin of the product path on reference-held data: the 1D driver (GPU Newton/time loop, then the
    consistent-mass projection of -grad(p) and the rescaling of 1D:802-805,893-954) run through its CLI reproduces
    the recorded OHP field to 1 % and the recorded OHP permittivity to 0.3 % after 300 steps.  The remaining gap is RUN
    LENGTH only: the recorded numbers belong to the 20,000-solve staged schedule, which reproduces them to 1e-10
    (test_staged_schedule_reproduces_the_recorded_digits)."""
    import json
    monkeypatch.setenv("GMPNP_OUT", str(tmp_path))
    from gmpnp_amd import edl1d
    out = edl1d.main(["--voltage_multiplier=%s" % voltage, "--num_steps=300"])
    meta = json.load(open(os.path.join(out, "metadata.json")))
    field, eps = STERN_OHP[voltage]
    assert abs(meta["field_OHP"] / field - 1.0) < 0.01
    assert abs(meta["eps_rel_OHP"] / eps - 1.0) < 0.003


@pytest.mark.parametrize("voltage", sorted(STERN_OHP))
def test_staged_schedule_reproduces_the_recorded_digits(voltage, gpu_lib):
    """The reference's FULL 1D schedule (1D:273-290: 10,000 steps of 1e-5 s, then 10,000 steps whose clock advances by
    1e-3 s while the form keeps dt = 1e-5 s) on the GPU, post-processed as the reference does (1D:802-805,
    893-954), lands on ALL FIVE vectors 1D/Stern_CO2ER.py:66-68 records: measured 1.9e-13 / 3e-14 (V = -2.5), 8e-11 / 2.5e-11
    (-5), 4e-11 / 5e-12 (-7.5), 1.9e-11 / 3e-13 (-10), 2.6e-11 / 3e-14 (-12.5) relative for field_OHP / eps_rel_OHP
    (profiles/r03/stern_schedule.json, tools/stern_schedule.py) — with exactly the Newton iterations the C oracle takes over
    the same 20,000 solves (tests/golden/stern_oracle.json: 40,024 ... 40,075; 2 per solve once the layer has formed).
    Newton stops at 1e-4, so agreement at 1e-10 after 20,000 solves means the iterates themselves follow FEniCS's: forms,
    scaling, the 2-point Gauss-Legendre rule of the steric term in F AND in J, DOLFIN's Newton/BC semantics, the direct solve
    and the projection are pinned for the 1D MPNP path.  (Rounds 1-2 gave J the 3-point rule of the UFL-estimate reading:
    Newton then degenerates near steric saturation and V = -12.5 stopped at solve 6,000 — tests/test_edl1d_oracle.py.)"""
    import json
    from gmpnp_amd.edl1d import EDLRun
    field, eps = STERN_OHP[voltage]
    with open(os.path.join(GOLDEN, "stern_oracle.json")) as fh:
        oracle_row = {r["voltage_multiplier"]: r for r in json.load(fh)["rows"]}[voltage]["rows"][-1]
    run = EDLRun(voltage_multiplier=voltage, dry_run=False)
    try:
        assert run.tot_num_steps == 20000
        for _ in range(run.tot_num_steps):
            run.step(verbose=False)
            run.history = run.history[-1:]
        s = run.ohp_summary()
    finally:
        run.sys.close()
    assert abs(s["field_OHP"] / field - 1.0) < 5e-10, s
    assert abs(s["eps_rel_OHP"] / eps - 1.0) < 2e-10, s
    assert int(sum(run.newton_its)) == oracle_row["newton_total"] and max(run.newton_its[-1000:]) == 2
    assert abs(s["field_OHP"] / oracle_row["field_OHP"] - 1.0) < 5e-10 and abs(s["eps_rel_OHP"] / oracle_row["eps_rel_OHP"] - 1.0) < 2e-10


@pytest.mark.parametrize("case,nparts", [("pore10", 2), ("pore10", 4), ("pore10", 8), ("pore50", 4)])
def test_partitioned_solve_in_library_matches_serial(case, nparts, pore10, pore50, gpu_lib):
    """ONE problem cut into mesh partitions and solved inside libgmpnp.so (gmpnp_group_newton_solve): global coarse
    space, one fused all-reduce and one ghost-row exchange per BiCGStab half-iteration.  All ranks live in this process
    (the test box has one GPU; RCCL refuses two ranks on one device), the exchanges are device copies — every other line
    of the algorithm is the multi-GPU one.  The serial golden step is reproduced with the same Newton count, and BiCGStab
    needs about what the single-GPU solver needs (the partitioned preconditioner is the same operator)."""
    from gmpnp_amd import dist
    pp, mesh, prob, _ = pore10 if case == "pore10" else pore50
    g = np.load(os.path.join(GOLDEN, case + "_steps.npz"))
    nv = mesh.num_vertices
    un = np.tile(np.r_[np.ones(8), 0.0], nv)
    opts = gpu_lib.newton_options(MUMPS_09)
    with gpu_lib.DeviceSolver(prob, warm_start=-1, coarse_refresh=1) as dev:   # cold starts, fresh coarse operator: like the group
        dev.set_state(np.zeros(nv * 9), un)
        serial = dev.newton_solve(opts)
    with dist.PartitionedSolver(prob, nparts) as ps:
        assert ps.selftest() == 0.0   # in-process transport: device copies between the handles
        ps.set_state(np.zeros(nv * 9), un)
        st = ps.newton_solve(opts)
        u = ps.get_state()
    assert st["converged"] and st["iterations"] == int(g["newton_its"][0]) == serial["iterations"]
    assert relerr(u, g["states"][0]) < 1e-8
    assert np.allclose(st["residuals"], serial["residuals"], rtol=1e-5)
    assert st["krylov_iterations"] < 1.3 * serial["krylov_iterations"] + 10, (st["krylov_per_iteration"], serial["krylov_per_iteration"])


def test_partitioned_time_loop_matches_golden(gpu_lib):
    """The 3D driver on two partitions (PoreRun(partition=...)): Newton, global medians -> Sechenov -> new bc4 on every
    rank's handle, u_n.assign(u) — the golden steps of the serial oracle."""
    from gmpnp_amd.pore3d import PoreRun
    g = np.load(os.path.join(GOLDEN, "pore10_steps.npz"))
    run = PoreRun(num_steps=3, concentration_elec=0.5, L=10e-9, R=5e-9, partition=(2, None))
    try:
        run.run(verbose=False)
        assert run.newton_its == list(g["newton_its"][:3])
        for k in range(3):
            assert relerr(run.history[k + 1].ravel(), g["states"][k]) < 1e-8
        assert abs(run.co2_bc - g["co2_bc"][2]) / run.co2_bc < 1e-9
    finally:
        run.sys.close()


def test_config3_geometry_on_four_partitions(gpu_lib):
    """BASELINE configs[3]: L_100_R_50 (mesh generated by gmpnp_amd.meshgen — the reference's file was never published),
    4 mesh partitions.  With the stated 1.0 M bulk Newton leaves the admissible set (1 - sum a_j u_j <= 0) in the first
    solve from the zero state, serial and partitioned alike (the oracle diverges on this geometry too);
    with the 0.5 M bulk of the north-star case the partitioned run reproduces the single-GPU run: same Newton counts,
    states to round-off of the linear solves."""
    from gmpnp_amd.pore3d import PoreRun
    for part in (None, (4, None)):
        run = PoreRun(num_steps=1, concentration_elec=1.0, L=100e-9, R=50e-9, partition=part)
        try:
            with pytest.raises(RuntimeError):   # the iterates leave the admissible set and never come back: NaN / Inf, or 50 iterations
                run.step(verbose=False)
        finally:
            run.sys.close()
    out = []
    for part in (None, (4, None)):
        run = PoreRun(num_steps=3, concentration_elec=0.5, L=100e-9, R=50e-9, partition=part)
        try:
            run.run(verbose=False)
            out.append((list(run.newton_its), np.array(run.history[1:])))
            assert run.mesh.num_vertices == 11725
        finally:
            run.sys.close()
    assert out[0][0] == out[1][0] and len(out[0][0]) == 3
    assert relerr(out[1][1].ravel(), out[0][1].ravel()) < 1e-8


def test_bench_partitioned_code_path_at_world_size_one(gpu_lib):
    """Everything `bench.py --gpus N` does for N > 1 — torch.distributed process group, the RCCL id made by rank 0 and
    broadcast through it, the communicator inside the library, PoreRun(partition=(N, rank)) with its per-step gather and
    Dirichlet update, warm-up / reset / timed steps, the output line — run with ONE rank (`--force-partitioned`), which is
    all a single-GPU box can host.  The one-partition run must count the Newton iterations of the single-GPU solver."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    env = dict(os.environ, MASTER_PORT="29631")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "4", "--warmup", "1", "--no-cpu-baseline",
                        "--force-partitioned"], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    reh = out["partitioned_rehearsal"]
    assert "error" not in reh, reh
    assert reh["newton_iterations"] == out["config"]["newton_iterations"] and reh["value"] > 0
    assert out["n_gpus"] == 1 and out["scaling"] == "weak"


def test_bench_dumps_what_its_last_timed_step_computed(gpu_lib, tmp_path):
    """`bench.py --steps K --dump-outputs DIR`, both cases: exactly K timed steps (after warm-up and reset to t = 0), and the state
    after the last one is the oracle's state after step K (tests/golden/pore50_window.npz, edl50_default_steps.npz)."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    lines = {}
    for case, steps in (("pore50", 3), ("edl50", 3)):
        d = str(tmp_path / case)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--case", case, "--steps", str(steps), "--warmup", "1",
                            "--no-cpu-baseline", "--no-edl50", "--dump-outputs", d], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert p.returncode == 0, p.stderr[-2000:]
        line = json.loads(p.stdout.strip().splitlines()[-1])
        its = np.load(os.path.join(d, "newton_iterations.npy"))
        assert line["steps"] == steps and len(its) == steps and its.sum() == line["config"]["newton_iterations"]
        assert line["ms_per_step"] > 0 and np.isclose(line["value"], its.sum() / (line["ms_per_step"] * 1e-3 * steps), rtol=1e-9)
        lines[case] = (np.load(os.path.join(d, "vertex_values.npy")), its)
    u, its = lines["pore50"]
    g = np.load(os.path.join(GOLDEN, "pore50_window.npz"))
    assert u.dtype == np.float64 and u.shape == (g["full_states"].shape[1] // 9, 9)
    assert list(its) == list(g["newton_its"][:3])
    assert relerr(u[g["probes"]].ravel(), g["probe_values"][2].ravel()) < 1e-8
    assert np.allclose(np.sqrt((u ** 2).sum(axis=0)), g["field_norms"][2], rtol=1e-8)
    u, its = lines["edl50"]
    g = np.load(os.path.join(GOLDEN, "edl50_default_steps.npz"))
    assert u.shape == (5991, 7) and list(its) == list(g["newton_its"][:3])
    assert relerr(u.ravel(), g["states"][2]) < 1e-8


def test_plain_bench_run_dumps_the_1d_arrays_and_measures_nothing_more(gpu_lib, tmp_path):
    """A plain `bench.py --steps K --dump-outputs DIR` (no --full) writes what the parent layout has — the 3D arrays and those of
    the secondary 1D case, whose 100 steps start with the oracle's Newton counts — while its line carries the headline and the
    live roofline only: no CPU baseline, no 1D rate, no launches timed by themselves."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    d = str(tmp_path / "plain")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--dump-outputs", d],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert "cpu_baseline" not in line and "edl50" not in line, sorted(line)
    assert line["roofline"]["empty_event_pair_us"] is None and line["roofline"]["mean_launch_us"] > 0
    assert sorted(os.listdir(d)) == ["edl50_newton_iterations.npy", "edl50_vertex_values.npy", "newton_iterations.npy", "vertex_values.npy"]
    its = np.load(os.path.join(d, "edl50_newton_iterations.npy"))
    g = np.load(os.path.join(GOLDEN, "edl50_default_steps.npz"))
    assert len(its) == 100 and list(its[:3]) == list(g["newton_its"])
    assert np.load(os.path.join(d, "edl50_vertex_values.npy")).shape == (5991, 7)


@pytest.mark.parametrize("nparts", [4, 8])
def test_partitioned_time_loop_survives_krylov_breakdowns(gpu_lib, nparts):
    """Twelve time steps of the bench problem on 4 / 8 partitions (all ranks in one process): 88 linear solves, some of which
    break down in their first pass on these partitions (BiCGStab spikes past 1e5 times its starting residual after a warm
    start) and are repeated with a pseudo-random shadow vector.  Newton counts equal the single-GPU run's at every step."""
    from gmpnp_amd.pore3d import PoreRun
    common = dict(num_steps=12, concentration_elec=0.5, L=50e-9, R=5e-9)
    ref = PoreRun(**common)
    run = PoreRun(partition=(nparts, None), **common)
    try:
        for _ in range(12):
            ref.step(verbose=False)
            run.step(verbose=False)
        assert run.newton_its == ref.newton_its
        assert relerr(np.asarray(run.history[-1]), np.asarray(ref.history[-1])) < 1e-9
        assert run.sys.krylov_iterations < 1.3 * ref.sys.krylov_iterations
    finally:
        run.sys.close()
        ref.sys.close()


def test_bench_two_ranks_share_the_card_over_peer_mailboxes():
    """The driver's N = 2 invocation of bench.py (torch.distributed.run, one process per rank), rehearsed with both ranks on the
    test box's one GPU (GMPNP_BENCH_BACKEND=gloo: RCCL refuses two ranks on one device): the replica phase, then ONE problem on
    two mesh partitions over the peer-mailbox transport, Newton counts equal to the single-GPU run's."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    env = dict(os.environ, GMPNP_BENCH_BACKEND="gloo")
    port = 29500 + (os.getpid() % 400) + 63
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1"],
                       capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads([ln for ln in p.stdout.strip().splitlines() if ln.startswith("{")][-1])
    assert out["n_gpus"] == 2 and out["scaling"] == "strong", out
    assert out["partitioned"]["transport"] == "peer" and "earlier_errors" not in out["partitioned"], out["partitioned"]
    assert out["config"]["newton_iterations"] * 2 == out["replicas"]["newton_iterations"]
    assert out["value"] > 0 and out["replicas"]["value"] > 0


def _library_partition_worker(rank, world, port, out_dir, transport="host", exchange_form=0, refine=0):
    import sys
    from conftest import ROOT
    sys.path.insert(0, ROOT)
    import torch.distributed as tdist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    tdist.init_process_group("gloo", rank=rank, world_size=world)   # both ranks share the one GPU of the test box
    try:
        from gmpnp_amd import backend, dist
        from gmpnp_amd.mesh import read_dolfin_xml, resolve_mesh_path
        from gmpnp_amd.params import pore_parameters, utilities_dir
        from gmpnp_amd.problem import pore_problem
        pp = pore_parameters(concentration_elec=0.5, L=10e-9, R=5e-9)
        mesh = read_dolfin_xml(resolve_mesh_path(utilities_dir(), pp.mesh_name))
        prob, _ = pore_problem(pp, mesh, refine=refine)
        nv = prob.coords.shape[0]
        kw = {"exchange_form": exchange_form} if transport == "peer" else {}
        with dist.PartitionedSolver(prob, world, rank=rank, transport=transport, **kw) as ps:
            form = ps.exchange_form()
            assert ps.selftest() == 0.0     # gmpnp_group_selftest: self-checking all-reduce + ghost-row messages over THIS transport
            ps.set_state(np.zeros(nv * 9), np.tile(np.r_[np.ones(8), 0.0], nv))
            import time
            t0 = time.perf_counter()
            st = ps.newton_solve(backend.newton_options(MUMPS_09))
            wall = time.perf_counter() - t0
            ug = ps.get_state()
        if rank == 0:
            np.savez(os.path.join(out_dir, "libdist.npz"), u=ug, its=st["iterations"], res=np.array(st["residuals"]),
                     kits=np.array(st["krylov_per_iteration"]), wall=wall, form=form)
    finally:
        tdist.destroy_process_group()


def test_library_partitioned_solve_two_processes_on_one_card(gpu_lib, tmp_path):
    """Two PROCESSES, each driving its own partition handle through gmpnp_group_newton_solve, sharing the test box's one GPU:
    the library's lock-step (burst schedule, device-side verdict, warm-start decision) under real inter-process asynchrony.
    RCCL refuses two ranks on one device, so the collectives travel through the library's host-staged transport
    (gmpnp_group_create_hosted) and torch.distributed/gloo; every other line is the production path."""
    import torch.multiprocessing as mp
    port = 29500 + (os.getpid() % 400) + 31
    mp.spawn(_library_partition_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    g = np.load(os.path.join(GOLDEN, "pore10_steps.npz"))
    d = np.load(os.path.join(str(tmp_path), "libdist.npz"))
    assert int(d["its"]) == int(g["newton_its"][0])
    assert relerr(d["u"], g["states"][0]) < 1e-8
    assert np.allclose(d["res"], g["residuals"][0][: len(d["res"])], rtol=1e-4)
    assert d["kits"].sum() < 700     # the single-GPU solver needs about 450 BiCGStab iterations for this solve


@pytest.mark.parametrize("world,exchange_form", [(2, 0), (4, 0), (2, 1), (4, 1)])
def test_peer_mailbox_transport_between_processes_on_one_card(gpu_lib, tmp_path, world, exchange_form):
    """The peer-mailbox transport between real PROCESSES: every rank maps the others' mailboxes through IPC handles, every
    collective of the partitioned Newton solve is one k_peer_exchange launch that stores into the peers' mailboxes and waits on
    its own flags (no RCCL, no host step).  The ranks share the test box's one GPU, so the stores do not cross xGMI here; the
    protocol (handles, mapping, sequence numbers, parity slots, flag waits between kernels of different processes) is the
    multi-GPU one.  Against the serial golden step.  exchange_form 0: the exchange of a half-iteration rides in front of the NEXT
    launch's coarse workgroups (k_half_a_x / k_half_b_x: two launches per BiCGStab iteration; the boundary tiles re-read their ghost
    rows behind the hand-over, on whatever XCD they run); 1: its own launch (k_dist_reduce_exchange)."""
    import torch.multiprocessing as mp
    port = 29500 + (os.getpid() % 400) + 47 + world + 10 * exchange_form
    mp.spawn(_library_partition_worker, args=(world, port, str(tmp_path), "peer", exchange_form), nprocs=world, join=True)
    g = np.load(os.path.join(GOLDEN, "pore10_steps.npz"))
    d = np.load(os.path.join(str(tmp_path), "libdist.npz"))
    assert int(d["form"]) == (2 if exchange_form == 0 else 1)   # the launches of these partitions are resident with the exchange in front
    assert int(d["its"]) == int(g["newton_its"][0])
    assert relerr(d["u"], g["states"][0]) < 1e-8
    assert np.allclose(d["res"], g["residuals"][0][: len(d["res"])], rtol=1e-4)
    assert d["kits"].sum() < 700
    print("peer transport (exchange form %d), %d ranks on one card: %d BiCGStab iterations in %.1f ms" % (int(d["form"]), world, int(d["kits"].sum()), 1e3 * float(d["wall"])))


def test_rccl_transport_at_world_size_one(pore10, gpu_lib):
    """The RCCL transport itself (librccl.so loaded by the library, communicator from gmpnp_comm_unique_id /
    gmpnp_comm_create, ncclAllReduce on the solver's stream) on the one rank a single-GPU box allows."""
    from gmpnp_amd import dist
    pp, mesh, prob, _ = pore10
    g = np.load(os.path.join(GOLDEN, "pore10_steps.npz"))
    nv = mesh.num_vertices
    with dist.PartitionedSolver(prob, 1, rank=0, use_torch_dist=False) as ps:
        assert ps.comm_selftest(5000) == 0.0          # grouped ncclSend/ncclRecv (to self) + ncclAllReduce: exact copies
        assert ps.selftest() == 0.0
        ps.set_state(np.zeros(nv * 9), np.tile(np.r_[np.ones(8), 0.0], nv))
        st = ps.newton_solve(gpu_lib.newton_options(MUMPS_09))
        u = ps.get_state()
    assert st["iterations"] == int(g["newton_its"][0]) and relerr(u, g["states"][0]) < 1e-8


def test_peer_exchange_form_follows_the_residency_of_the_launch(gpu_lib, tmp_path):
    """The exchange rides inside the next half-iteration's launch only where that launch — tiles, coarse workgroups AND exchange
    workgroups — is resident at once (gmpnp_group_exchange_form = 2); a partition too large for that (here: the once-refined mesh,
    1.8k tiles on 768 slots) runs the separate exchange launches (1), and so does everybody when asked to (exchange_form=1).  One rank
    (the whole mesh as one partition), in a process of its own like the multi-rank tests: a process that loads this library BEFORE
    PyTorch and initialises PyTorch's HIP runtime afterwards gets the four-launch form from the occupancy query (two HIP runtimes in
    one process), which is the safe answer but not the one under test."""
    import torch.multiprocessing as mp
    g = np.load(os.path.join(GOLDEN, "pore10_steps.npz"))
    states = {}
    for k, (asked, runs, refine) in enumerate(((0, 2, 0), (1, 1, 0), (0, 1, 1))):
        port = 29500 + (os.getpid() % 400) + 83 + k
        mp.spawn(_library_partition_worker, args=(1, port, str(tmp_path), "peer", asked, refine), nprocs=1, join=True)
        d = np.load(os.path.join(str(tmp_path), "libdist.npz"))
        assert int(d["form"]) == runs
        if refine == 0:
            assert int(d["its"]) == int(g["newton_its"][0]) and relerr(d["u"], g["states"][0]) < 1e-8
            states[runs] = d["u"]
        else:
            assert int(d["its"]) >= 5 and np.isfinite(d["u"]).all()
    assert relerr(states[2], states[1]) < 1e-9


def test_partition_plans_are_refused_when_inconsistent(pore10, gpu_lib):
    from gmpnp_amd import dist
    pp, mesh, prob, _ = pore10
    dom, perm, part = dist.partition_plan(prob, 2, 0)
    bad = dict(part)
    bad["vertex_owned"] = np.ones_like(part["vertex_owned"])      # ghosts declared owned: slabs would mix, lists are wrong
    with pytest.raises(gpu_lib.GmpnpError):
        gpu_lib.DeviceSolver(dom.problem, perm=perm, partition=bad)
    with pytest.raises(gpu_lib.GmpnpError, match="ascending"):
        gpu_lib.DeviceSolver(dom.problem, perm=perm[::-1].copy(), partition=part)


def test_multilevel_term_changes_iteration_counts_not_results(gpu_lib):
    """The geometric multilevel term of the preconditioner (gmpnp_attach_coarse_level; once-refined L_10_R_5, two nested meshes):
    identical Newton counts, states to solver accuracy, less than half the BiCGStab iterations of the two-level scheme; the coarse
    level is assembled by this library's own kernels at the injected state.  (L_50_R_5 refined twice / three times, 1.77 M / 13.7 M dofs:
    206 -> 25 / 494 -> 29 iterations per solve, Newton iterations 3.8 x / 8.6 x faster, profiles/r03/multilevel_refine{2,3}.json.)"""
    from gmpnp_amd.pore3d import PoreRun
    out = {}
    for name, kw in (("two-level", {}), ("multilevel", {"multilevel": True})):
        run = PoreRun(num_steps=2, concentration_elec=0.5, L=10e-9, R=5e-9, refine=1, **kw)
        try:
            run.run(verbose=False)
            out[name] = (list(run.newton_its), int(run.sys.krylov_iterations), np.array(run.history[1:]))
            if kw:
                assert run.sys.dev.krylov_launches_per_iteration == 4   # materialised vector form
        finally:
            run.sys.close()
    assert out["two-level"][0] == out["multilevel"][0]
    assert relerr(out["multilevel"][2].ravel(), out["two-level"][2].ravel()) < 1e-8
    assert out["multilevel"][1] < 0.5 * out["two-level"][1], (out["multilevel"][1], out["two-level"][1])
    # refused: levels that are not nested, partitioned handles
    pp, mesh, prob, _ = _pore_case(10e-9)
    with gpu_lib.DeviceSolver(prob) as a, gpu_lib.DeviceSolver(prob) as b:
        with pytest.raises(gpu_lib.GmpnpError):
            a.attach_coarse_level(b, np.zeros((mesh.num_vertices, 2), dtype=np.int32))


def _pore_case(L):
    from conftest import _pore
    return _pore(L, 5e-9)


def test_refined_multilevel_run_through_the_driver_and_the_bench(tmp_path, monkeypatch, gpu_lib):
    """`--refine 1 --multilevel` through the 3D driver's CLI (outputs on the refined mesh: 12,109 vertices) and through bench.py
    --full (the line names the preconditioner and times the tile kernels by themselves for the roofline object)."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    monkeypatch.setenv("GMPNP_OUT", str(tmp_path))
    from gmpnp_amd import pore3d
    out = pore3d.main(["--L=10e-9", "--R=5e-9", "--concentration_elec=0.5", "--num_steps=1", "--refine=1", "--multilevel"])
    a = np.load(os.path.join(out, "arrays_unscaled.npz"))
    assert a["p"].shape == (2, 12109) and a["field_values"].shape == (3 * 12109,) and np.isfinite(a["cat_grad"]).all()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--mesh", "L_10_R_5", "--refine", "1", "--multilevel", "--steps", "2", "--warmup", "1",
                        "--full", "--no-cpu-baseline", "--no-edl50"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert "multilevel" in line["config"]["preconditioner"] and line["config"]["n_vertices"] == 12109
    assert line["roofline"]["multilevel_note"] and "k_bicg_a_mat" in line["roofline"]["kernel"] and 0.0 < line["roofline"]["frac"] < 1.0
    assert line["roofline"]["launches_per_krylov_iteration"] == 4


# ---- closed-form pins of the 3D forms (tests/closed_forms.py): the same four cases run with the oracle in tests/test_oracle_pins.py ----
TIGHT = {"nonlinear_solver": "newton", "newton_solver": {"linear_solver": "mumps", "maximum_iterations": 50, "relative_tolerance": 1e-12,
                                                         "absolute_tolerance": 1e-10, "relaxation_parameter": 1.0}}


def _gpu_steady(gpu_lib, prob, state, sp=TIGHT):
    with gpu_lib.DeviceSolver(prob) as dev:
        dev.set_state(state, state)
        assert dev.newton_solve(gpu_lib.newton_options(sp))["converged"]
        return dev.get_state()


def test_pore_equilibrium_is_the_steric_boltzmann_distribution(gpu_lib):
    """closed_forms.boltzmann_case on the GPU, reference mesh and one uniform refinement: the zero-flux steady state of the pore
    satisfies u_i = (1 - S) / (1 - S_b) exp(-z_i p) at every vertex up to the discretisation error (largest on the wall, where the
    concentrations are steepest), whose rms falls by 2.9 under refinement; the uncharged species satisfy it to solver accuracy."""
    import closed_forms as cf
    errs = []
    for refine in (0, 1):
        prob, state, check = cf.boltzmann_case(refine)
        emax, erms, neutral = check(_gpu_steady(gpu_lib, prob, state))
        assert neutral < 1e-6
        errs.append((emax, erms))
    print("|u - closed form| (max, rms) on the mesh and on its refinement:", errs)   # 1.8e-2, 2.2e-3 -> 1.2e-2, 7.4e-4
    assert errs[0][0] < 2e-2 and errs[1][0] < 0.8 * errs[0][0] and errs[1][1] < 0.4 * errs[0][1], errs


def test_pore_potential_is_the_debye_hueckel_bessel_profile(gpu_lib):
    """closed_forms.bessel_case on the GPU: p(r) = V I0(kappa r) / I0(kappa R) at the mid-pore vertices of L_50_R_5."""
    import closed_forms as cf
    errs = []
    for refine in (0, 1):
        prob, state, check = cf.bessel_case(refine)
        errs.append(check(_gpu_steady(gpu_lib, prob, state, cf.sp_tight(1e-12, 1e-12))))
    print("p / V - I0(kappa r) / I0(kappa R) (max, rms), smallest p / V:", errs)
    # 6.5e-2 / 4.1e-2 on the reference mesh, 3.5e-2 / 2.0e-2 after one refinement, p / V = 0.76 on the axis.  (The cross-section of the
    # mesh is a polygon and stays that polygon under red refinement, so the error does not keep falling at second order.)  A factor
    # 2 in q, a valence entering linearly instead of squared or a missing bulk concentration moves the axis value by 0.1-0.2.
    assert errs[0][2] < 0.9                                        # the profile really sags towards the axis
    assert errs[0][1] < 5e-2 and errs[1][1] < 2.5e-2 and errs[1][1] < 0.6 * errs[0][1], errs


def test_uniform_state_follows_the_published_rate_equations(gpu_lib):
    """closed_forms.rates_case on the GPU: one backward-Euler step of a uniform electroneutral state against the literal
    8-unknown solve.  H moves by 16 %, OH by 0.24 % in the step; the GPU agrees to 3e-7 (charged species) / 2e-8 (neutral ones):
    the bulk composition of the YAML file is electroneutral to its printed digits only, and the 3e-7 potential that leaves
    shifts the ions by exp(-z p)."""
    import closed_forms as cf
    prob, state, check = cf.rates_case()
    dev_rel, neutral_rel, pmax = check(_gpu_steady(gpu_lib, prob, state, cf.sp_tight(1e-13, 1e-11)))
    assert pmax < 1e-6 and dev_rel < 2e-6 and neutral_rel < 1e-7


def test_wall_and_exit_fluxes_balance_with_the_published_coefficients(gpu_lib):
    """closed_forms.flux_case on the GPU: J_X_wall |S2| + kappa_X int_S3 (u_X - 1) ds + (time term) = 0 for CO and H2, closed to
    1e-11 of 18."""
    import closed_forms as cf
    prob, state, check = cf.flux_case()
    for X, (balance, scale, excess) in check(_gpu_steady(gpu_lib, prob, state, cf.sp_tight(1e-9, 1e-9))).items():
        assert excess > 1e3 and abs(balance) < 1e-7 * scale, (X, balance, scale)
