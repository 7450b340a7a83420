"""The high-precision references of tests/hp_reference.py and the sharpness of the 1D inputs test_gpu_shapes.py feeds the GPU
(CPU only): the reference solve recovers a known solution to a few units of roundoff, the model of the block cyclic reduction
meets the GPU test's tolerance on every 1D input, and the sweep reaches every shape of the one-wave tail of the reduction."""
import os

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import gmpnp_oracle as O
import hp_reference as H
from conftest import GOLDEN, _edl, random_state


def _x_true(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(1.0, 2.0, n) * rng.choice([-1.0, 1.0], n)


@pytest.mark.parametrize("case", ["edl1", "edl50", "uniform9", "graded17"])
def test_reference_solve_recovers_a_known_solution(case):
    """b = A x_true held in double-double, so x_true is the exact solution: refinement must return it to 4u (max-relative),
    where SciPy's splu alone is off by kappa u (1e-9 ... 1e-7 on these Jacobians)."""
    if case in ("edl1", "edl50"):
        kw = dict(H.REFERENCE_1D)[case]
        prob = _edl(**kw)[2]
        g = np.load(os.path.join(GOLDEN, case + "_steps.npz"))
        u, un = g["states"][1], g["states"][0]
    else:
        nv = int(case.lstrip("uniformgraded"))
        prob = H.edl_generated(H.uniform_mesh_1d(nv) if case.startswith("uniform") else H.graded_mesh_1d(nv))
        u, un = random_state(nv, 6, seed=nv)
    _, A = O.assemble(prob, u, un)
    xt = _x_true(prob.ndof, 1)
    b = H.dd_matvec(A, xt)
    x, kappa = H.reference_solve(A, b)
    assert kappa > 1e7                                  # ill-conditioned enough that plain LU is visibly worse
    assert H.max_rel(x, xt) <= 4 * H.U
    assert np.abs(x - xt).max() / np.abs(xt).min() <= 4 * H.U * np.abs(xt).max() / np.abs(xt).min()
    assert H.max_rel(spla.splu(A.tocsc()).solve(b[0]), xt) > 100 * H.U
    # the double-double residual of the exact solution is at the u^2 level; the fp64 one is not
    assert np.abs(H.dd_residual(A, xt, b)).max() <= 1e-28 * np.abs(b[0]).max()
    assert H.dd_backward_error(A, xt, b) < 1e-30


def test_double_double_kernels_are_exact_on_a_known_cancellation():
    """(1 + 2^-30)(1 - 2^-30) - 1 = -2^-60: lost in fp64, exact in double-double."""
    import scipy.sparse as sp
    A = sp.csr_matrix(np.array([[1.0 + 2.0 ** -30]]))
    r = H.dd_residual(A, np.array([1.0 - 2.0 ** -30]), np.array([1.0]))
    assert r[0] == 2.0 ** -60
    assert (np.array([1.0]) - A @ np.array([1.0 - 2.0 ** -30]))[0] == 0.0


def test_reference_solve_refuses_hopeless_conditioning():
    import scipy.sparse as sp
    A = sp.csr_matrix(np.array([[1.0, 1.0], [1.0, 1.0 + 1e-15]]))
    with pytest.raises(H.IllConditioned):
        H.reference_solve(A, np.array([1.0, 2.0]))


def test_generated_meshes_are_what_edl_problem_expects():
    for nv in (2, 3, 64, 4097):
        for mesh in (H.uniform_mesh_1d(nv), H.graded_mesh_1d(nv, 1e3)):
            x = mesh.coords[:, 0]
            assert mesh.dim == 1 and mesh.num_vertices == nv and x[0] == 0.0 and x[-1] == 1.0 and np.all(np.diff(x) > 0)
            prob = H.edl_generated(mesh)
            assert prob.ndof == 7 * nv and list(prob.point_vertices) == [0]
    h = np.diff(H.graded_mesh_1d(129, 1e3).coords[:, 0])
    assert h.argmin() == 0 and h.max() / h.min() == pytest.approx(1e3, rel=1e-9)


def test_sweep_covers_every_tail_shape():
    """bcr_tail_levels mirrors tri_solve in gmpnp_api.hip (kBcrTailRows = 4, kBcrTailLevels = 8) and must change with it.
    The sweep must reach every lowest tail level from 2 to 8 rows and solves that run entirely inside k_bcr_tail."""
    assert H.bcr_tail_levels(1091) == ([5, 3, 2, 1], 8) and H.bcr_tail_levels(5991) == ([6, 3, 2, 1], 10)
    tails = {nv: H.bcr_tail_levels(nv) for nv in H.SWEEP_NV}
    assert {t[0][0] for t in tails.values()} >= set(range(2, 9))
    assert {t[0][0] for t in tails.values() if t[1] == 0} >= set(range(2, 9))        # whole solve in the one wave
    assert any(t[1] > 0 and t[0][0] in (7, 8) for t in tails.values())                 # [7|8,4,2,1] below forward levels
    for nv, (lv, l0) in tails.items():
        assert lv[-1] == 1 and all(n <= 4 for n in lv[1:]) and (l0 == 0 or lv[0] > 4)


@pytest.fixture(scope="module")
def sweep():
    return H.sweep_1d_inputs(GOLDEN)


def test_sweep_inputs(sweep):
    """Every 1D input of the GPU sweep (test_gpu_shapes.py): the model of the reduction WITH partial pivoting meets the GPU
    test's tolerance for the right-hand sides F, a random vector and A x_true; the model WITHOUT pivoting misses it on the
    inputs marked as needing pivoting (solved with F only), one of them below forward levels of the reduction."""
    names = [s[0] for s in sweep]
    assert len(names) == len(set(names))
    assert any(s[4] and H.bcr_tail_levels(s[1].coords.shape[0])[1] == 0 for s in sweep)
    assert any(s[4] and H.bcr_tail_levels(s[1].coords.shape[0])[1] > 0 for s in sweep)
    for name, prob, u, un, needs_pivoting in sweep:
        F, A = O.assemble(prob, u, un)
        blocks = H.tri_blocks(A, prob.nf)
        lu = spla.splu(A.tocsc())
        rng = np.random.default_rng(6)
        rhss = (("F", F),) if needs_pivoting else (("F", F), ("random", rng.standard_normal(prob.ndof)), ("Ax", A @ _x_true(prob.ndof, 2)))
        for rn, rhs in rhss:
            lim = H.direct_solve_tolerances(A, rhs, lu)
            assert H.meets_direct_tolerance(A, H.bcr_model(blocks, rhs, pivot=True), rhs, lim), (name, rn)
            if needs_pivoting:
                assert not H.meets_direct_tolerance(A, H.bcr_model(blocks, rhs, pivot=False), rhs, lim), (name, rn)


@pytest.mark.parametrize("case,expect", [("edl1", 93), ("edl50", 4990)])
def test_physical_blocks_have_nontrivial_pivots(case, expect):
    """LAPACK's partial pivoting swaps rows in most level-0 diagonal blocks of the physical Jacobians (the Poisson row holds
    q z_i M, far larger than a species row's diagonal): the kernel's pivot search is exercised on every such block."""
    prob = _edl(**dict(H.REFERENCE_1D)[case])[2]
    g = np.load(os.path.join(GOLDEN, case + "_steps.npz"))
    _, A = O.assemble(prob, g["states"][1], g["states"][0])
    assert H.level0_pivoted_blocks(H.tri_blocks(A, prob.nf)) == expect


def test_steep_inputs_need_pivoting_in_their_level0_blocks():
    for kind, nv, P in H.NEEDS_PIVOTING:
        mesh = H.uniform_mesh_1d(nv) if kind == "uniform" else H.graded_mesh_1d(nv)
        u, un = H.steep_state(nv, P, nv)
        _, A = O.assemble(H.edl_generated(mesh), u, un)
        assert H.level0_pivoted_blocks(H.tri_blocks(A, 7)) > 0


@pytest.mark.parametrize("nv", [9, 10, 64, 65, 577, 1091])
def test_krylov_problems_converge_with_node_block_jacobi(nv):
    """The NF = 7 Krylov problems of test_gpu_shapes.py (uniform mesh, q scaled by KRYLOV_Q_SCALE, random state): SciPy's
    BiCGStab with node-block Jacobi reaches 1e-10 on them, so a device solve that does not is the device's fault."""
    prob = H.edl_generated(H.uniform_mesh_1d(nv), q_scale=H.KRYLOV_Q_SCALE)
    u, un = random_state(nv, 6, seed=nv)
    F, A = O.assemble(prob, u, un)
    x = H.jacobi_bicgstab(A, F)
    assert np.linalg.norm(H.dd_residual(A, x, F)) / np.linalg.norm(F) < 2e-10
