"""The linear-algebra kernels on the mesh shapes the reference meshes do not reach, against the high-precision references of
tests/hp_reference.py (all on the GPU, every handle closed by `with`).

(a) The 1D direct solve (block cyclic reduction: k_bcr_forward / k_bcr_tail / k_bcr_backward) on uniform and graded meshes of
    2 ... 4097 vertices — every shape of the one-wave tail, solves that run entirely inside it — and on the five reference
    meshes: backward error within 10x that of SciPy's splu (floor 1e-14), forward error against the refined solution within
    10x that of splu (floor 1e-13), bitwise repeatable.
(b) The NF = 7 Krylov kernels (two-level and Jacobi BiCGStab, 1D: SELL slices of 9 rows) with 1, the default and the most
    aggregates, and Newton with 'bicgstab' against the oracle.
(c) The two-level BiCGStab, Jacobi, band LU, Newton and the projections on small and odd 3D meshes (1, 2 and 8 aggregates,
    nv mod 7 != 0).
"""

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import gmpnp_oracle as O
import hp_reference as H
from conftest import GOLDEN, box_pore_problem, random_state
from precond_reference import assembly_matches as _assembly_matches, relerr

pytestmark = pytest.mark.gpu

MUMPS_09 = {"nonlinear_solver": "newton", "newton_solver": {
    "linear_solver": "mumps", "maximum_iterations": 50, "relative_tolerance": 1e-4, "absolute_tolerance": 1e-4,
    "relaxation_parameter": 0.9}}


# ---- (a) 1D block cyclic reduction -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep():
    return H.sweep_1d_inputs(GOLDEN)


N_SWEEP = len(H.SWEEP_NV) * 3 + len(H.NEEDS_PIVOTING) + len(H.REFERENCE_1D)


@pytest.mark.parametrize("k", range(N_SWEEP))
def test_direct_solve_1d_sweep(k, sweep, gpu_lib):
    """Right-hand sides: F, a random vector and A x_true.  The limits are measured per input on the device's own Jacobian
    (hp_reference.direct_solve_tolerances); where kappa_1 u > 1e-2 only the backward error is checked.  Where the NumPy model
    of the same reduction (hp_reference.bcr_model, partial pivoting) is itself further than 10x splu from the solution, the
    forward limit is 2x the model's error (hp_reference.forward_limit): on the golden state of the 10 um mesh with F the
    reduction is less forward-accurate than sparse LU — measured on the MI355X 2.67e-11 against splu's 8.7e-13 (the model on
    the CPU: 2.59e-11), backward error 1e-18.  The inputs that need pivoting are solved with F only."""
    assert len(sweep) == N_SWEEP
    name, prob, u, un, needs_pivoting = sweep[k]
    with gpu_lib.DeviceSolver(prob) as dev:
        dev.set_state(u, un)
        Fo, A = _assembly_matches(dev, prob, u, un)
        lu = spla.splu(A.tocsc())
        blocks = H.tri_blocks(A, prob.nf)
        rng = np.random.default_rng(6)
        xt = rng.uniform(1.0, 2.0, prob.ndof) * rng.choice([-1.0, 1.0], prob.ndof)
        rhss = (("F", Fo), ("random", rng.standard_normal(prob.ndof)), ("Ax", A @ xt))
        for rn, rhs in rhss[:1] if needs_pivoting else rhss:
            x, st = dev.linear_solve(rhs, gpu_lib.LINEAR_BLOCK_TRIDIAGONAL)
            x2, _ = dev.linear_solve(rhs, gpu_lib.LINEAR_BLOCK_TRIDIAGONAL)
            assert st["converged"] and np.array_equal(x, x2), (name, rn)
            xr, tb, tf = H.direct_solve_tolerances(A, rhs, lu)
            be = H.dd_backward_error(A, x, rhs)
            assert be <= tb, (name, rn, be, tb)
            if xr is not None:
                fe = H.max_rel(x, xr)
                tf = H.forward_limit(tf, H.max_rel(H.bcr_model(blocks, rhs, pivot=True), xr))
                assert fe <= tf, (name, rn, fe, tf)


# ---- (b) NF = 7 Krylov kernels ---------------------------------------------------------------------------------------
KRYLOV_NV = (9, 10, 64, 65, 577, 1091)


def _krylov_problem(nv):
    return H.edl_generated(H.uniform_mesh_1d(nv), q_scale=H.KRYLOV_Q_SCALE)


@pytest.mark.parametrize("nv", KRYLOV_NV)
@pytest.mark.parametrize("nagg", [0, 1, 16])
def test_krylov_nf7_linear_solves(nv, nagg, gpu_lib):
    """Two-level and Jacobi BiCGStab at 1e-10 on the 1D Jacobian (q / 1e4, SciPy's node-block Jacobi BiCGStab converges on
    it: test_hp_reference.py): double-double residual < 2e-10, forward error within kappa_1 x 2e-10, the four-launch form
    bitwise equal to the default, a shared device to 1e-8."""
    prob = _krylov_problem(nv)
    u, un = random_state(nv, 6, seed=nv)
    Fo, Ao = O.assemble(prob, u, un)
    xr, kappa = H.reference_solve(Ao, Fo)
    out = {}
    for opts in (dict(), dict(launch_form=4), dict(shared_device=1)):
        with gpu_lib.DeviceSolver(prob, n_aggregates=nagg, **opts) as dev:
            assert dev.krylov_launches_per_iteration == 4     # 1D: no in-launch hand-over
            if nagg == 0:
                assert dev.n_aggregates == max(1, min(8, nv // 8))
            elif nagg == 1:
                assert dev.n_aggregates == 1
            else:
                assert dev.n_aggregates == max(1, min(16, nv // 8))
            dev.set_state(u, un)
            if opts:
                dev.assemble(True)
            else:
                _assembly_matches(dev, prob, u, un)
            for solver in (gpu_lib.LINEAR_TWOLEVEL, gpu_lib.LINEAR_JACOBI):
                x, st = dev.linear_solve(Fo, solver, 1e-10, 0.0, 20000)
                assert st["converged"], (solver, st)
                out[(tuple(opts.items()), solver)] = x
                r = H.dd_residual(Ao, x, Fo)
                assert np.linalg.norm(r) / np.linalg.norm(Fo) < 2e-10, solver
                assert H.max_rel(x, xr) <= kappa * 2e-10, solver
    for solver in (gpu_lib.LINEAR_TWOLEVEL, gpu_lib.LINEAR_JACOBI):
        ref = out[((), solver)]
        assert np.array_equal(out[((("launch_form", 4),), solver)], ref)
        assert relerr(out[((("shared_device", 1),), solver)], ref) < 1e-8


@pytest.mark.parametrize("nv", KRYLOV_NV)
@pytest.mark.parametrize("pc", ["default", "jacobi"])
def test_krylov_nf7_newton_matches_oracle(nv, pc, gpu_lib):
    """Newton from the zero state with 'bicgstab' at an explicit 1e-10 (the 'bicgstab' default is 1e-6): the oracle's iteration
    count and its iterate to 1e-8 — or to 10x the distance the oracle's own Newton with SciPy's node-block Jacobi BiCGStab at
    1e-10 keeps from it, where that is larger.  On the 9- and 10-vertex meshes Newton stops after three iterations at a
    residual of 1.4 (r0 = 2.2e5): the last correction is large and carries the Krylov solve's forward error (kappa_1 ~ 2e8
    times 1e-10) into the result.  SciPy's Krylov Newton ends 9.4e-8 / 3.8e-8 from the direct one there (MI355X: 2.4e-8 ...
    1.0e-7); from 64 vertices on a fourth iteration brings both to 1e-11."""
    prob = _krylov_problem(nv)
    u0, un = np.zeros(prob.ndof), np.tile(np.r_[np.ones(6), 0.0], nv)
    sp_ = {"nonlinear_solver": "newton", "newton_solver": {
        "linear_solver": "bicgstab", "preconditioner": pc, "maximum_iterations": 50, "relative_tolerance": 1e-4,
        "absolute_tolerance": 1e-4, "krylov_solver": {"relative_tolerance": 1e-10}}}
    opts = gpu_lib.newton_options(sp_, dim=1)
    assert opts.linear_solver == (gpu_lib.LINEAR_JACOBI if pc == "jacobi" else gpu_lib.LINEAR_TWOLEVEL)
    assert opts.krylov_relative_tolerance == 1e-10
    u_ref, st_ref = O.newton_solve(prob, u0, un)
    with gpu_lib.DeviceSolver(prob) as dev:
        dev.set_state(u0, un)
        st = dev.newton_solve(opts)
        u = dev.get_state()
    assert st["converged"] and st["iterations"] == st_ref.iterations
    assert st["krylov_iterations"] > 0 and st["direct_solves"] == 0
    u_kry, st_kry = O.newton_solve(prob, u0, un, linear_solve=H.jacobi_bicgstab)
    assert st_kry.iterations == st_ref.iterations
    assert relerr(u, u_ref) < max(1e-8, 10.0 * relerr(u_kry, u_ref))


# ---- (c) small and odd 3D meshes -------------------------------------------------------------------------------------
CYLINDERS = ((1, 1), (1, 2), (1, 4), (2, 5), (2, 12), (3, 9), (4, 16))
BOXES = ((2, 3), (4, 12), (5, 17))
SHAPES_3D = ["cyl%d_%d" % c for c in CYLINDERS] + ["box%d_%d" % b for b in BOXES]


def _problem_3d(name):
    if name.startswith("cyl"):
        import closed_forms as cf
        rings, layers = (int(v) for v in name[3:].split("_"))
        prob = cf._base(10e-9, 5e-9, 0, reactions=True, wall_flux=True, steady=False, q_scale=1.0, coarse=(rings, layers))[0]
        assert prob.coords.shape[0] == (1 + 3 * rings * (rings + 1)) * (layers + 1)
        return prob
    nx, nz = (int(v) for v in name[3:].split("_"))
    return box_pore_problem(nx, nz)[2]


def test_3d_shapes_reach_the_aggregate_counts(gpu_lib):
    """The sweep reaches 1, 2 and 8 aggregates (nagg = min(8, nv / 8)) and partial SELL slices (nv mod 7 != 0)."""
    naggs, nvs = set(), set()
    for name in SHAPES_3D:
        prob = _problem_3d(name)
        with gpu_lib.DeviceSolver(prob) as dev:
            naggs.add(dev.n_aggregates)
        nvs.add(prob.coords.shape[0])
    assert {1, 2, 8} <= naggs
    assert any(nv % 7 for nv in nvs)


@pytest.mark.parametrize("name", SHAPES_3D)
def test_3d_small_shapes(name, gpu_lib):
    """Assembly / J / SpMV as in (a); two-level, Jacobi and band LU at 1e-10 against the refined solution (double-double
    residual < 2e-10 on the device's matrix, forward error within kappa_1 x 2e-10 where kappa_1 u <= 1e-2); the two-launch form
    bitwise equal to the four-launch one wherever it is granted."""
    prob = _problem_3d(name)
    nv = prob.coords.shape[0]
    u, un = random_state(nv, prob.nf - 1, seed=11)
    xs = {}
    for form in (0, 4):
        with gpu_lib.DeviceSolver(prob, launch_form=form) as dev:
            dev.set_state(u, un)
            Fo, A = _assembly_matches(dev, prob, u, un)
            launches = dev.krylov_launches_per_iteration
            try:
                xr, kappa = H.reference_solve(A, Fo)
            except H.IllConditioned:
                xr, kappa = None, None
            for solver in (gpu_lib.LINEAR_TWOLEVEL, gpu_lib.LINEAR_JACOBI, gpu_lib.LINEAR_BAND_LU):
                if form == 4 and solver == gpu_lib.LINEAR_BAND_LU:
                    continue
                x, st = dev.linear_solve(Fo, solver, 1e-10, 0.0, 20000)
                assert st["converged"], (name, solver)
                xs[(form, solver)] = (x, launches)
                res = np.linalg.norm(H.dd_residual(A, x, Fo)) / np.linalg.norm(Fo)
                assert res < 2e-10, (name, solver, res)
                if xr is not None:
                    assert H.max_rel(x, xr) <= kappa * 2e-10, (name, solver)
    assert xs[(4, gpu_lib.LINEAR_TWOLEVEL)][1] == 4
    if xs[(0, gpu_lib.LINEAR_TWOLEVEL)][1] == 2:
        for solver in (gpu_lib.LINEAR_TWOLEVEL, gpu_lib.LINEAR_JACOBI):
            assert np.array_equal(xs[(0, solver)][0], xs[(4, solver)][0]), (name, solver)


@pytest.mark.parametrize("name", SHAPES_3D)
def test_3d_small_shapes_newton_and_projections(name, gpu_lib):
    """The first Newton solve from the zero state with MUMPS_09 (two-level BiCGStab at 1e-10): the oracle's iteration count and
    its iterate to 1e-8; project_gradient to 1e-10 of the field's magnitude and project_cellwise to 1e-12 against the oracle."""
    prob = _problem_3d(name)
    nv, nf = prob.coords.shape[0], prob.nf
    u0, un = np.zeros(prob.ndof), np.tile(np.r_[np.ones(nf - 1), 0.0], nv)
    u_ref, st_ref = O.newton_solve(prob, u0, un, relaxation_parameter=0.9)
    with gpu_lib.DeviceSolver(prob) as dev:
        dev.set_state(u0, un)
        st = dev.newton_solve(gpu_lib.newton_options(MUMPS_09), error_on_nonconvergence=False)
        u = dev.get_state()
        assert st_ref.converged and st["converged"] and st["iterations"] == st_ref.iterations
        assert relerr(u, u_ref) < 1e-8
        state = u_ref.reshape(nv, nf)
        for i in range(nf):
            sign = -1.0 if i == nf - 1 else 1.0
            got = dev.project_gradient(state[:, i], sign=sign)
            ref = O.project_gradient(prob.coords, prob.cells, state[:, i], sign=sign)
            assert np.abs(got - ref).max() <= 1e-10 * max(np.abs(ref).max(), 1e-30), (name, i)
        vals = np.random.default_rng(4).uniform(0.5, 2.0, len(prob.cells))
        assert np.abs(dev.project_cellwise(vals) - O.project_cellwise(prob.coords, prob.cells, vals)).max() < 1e-12
