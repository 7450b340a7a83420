"""The pair layout of vals_s (value_pair_offset, gmpnp_host_rules.h) seen through gmpnp_spmv_scaled: y = As x with As = J Dinv as
k_scale_columns wrote it and as TileRows reads it in the Krylov kernels, against NumPy's J @ blockdiag(inv(J_II)) @ x built from
get_jacobian_csr — without forty BiCGStab iterations in between.

Cases (tests/precond_reference.py): box4_12 and box5_17 (NF = 9, partial slices, nv mod 7 != 0, rows with more than 8 blocks: the
tail loop of TileRows::dot and the clamped preload both run), cyl1_1 (one aggregate), the 1D problems with 9 and 577 vertices
(NF = 7: three pairs and a single column).  x: a random vector, and each of the NF unit vectors of one interior node (the node with
the most neighbours) and of one boundary-adjacent node (a neighbour of a Dirichlet node, or that node where it has none) — a swapped
or shifted pair member shows as a wrong column of As.

Tolerance: 1e-13, the figure at which tests/test_gpu_parity.py compares the plain SpMV with the oracle's, here relative to
||As||_F ||x||_2 (the rounding bound of a matrix-vector product is gamma || |As| |x| || <= gamma ||As||_F ||x||; unit vectors pick
single columns, whose own norm may be far below the matrix's)."""
import numpy as np
import pytest
import scipy.sparse as sp

import precond_reference as R

pytestmark = pytest.mark.gpu

TOL = 1e-13                 # tests/test_gpu_parity.py: relerr(dev.spmv(x), Ao @ x) < 1e-13
CASES = ("box4_12", "box5_17", "cyl1_1", "1d9", "1d577")


def _problem(case):
    return R.problem_1d(int(case[2:])) if case.startswith("1d") else R.problem_3d(case)


def _probe_nodes(A, nf, bc_dofs):
    """(interior, boundary-adjacent): the node with the most neighbours; a neighbour of a Dirichlet node."""
    nv = A.shape[0] // nf
    B = sp.bsr_matrix(A, blocksize=(nf, nf))
    G = sp.csr_matrix((np.ones(len(B.indices)), B.indices, B.indptr), shape=(nv, nv))
    degree = np.diff(G.indptr)
    bc_nodes = np.unique(np.asarray(bc_dofs, dtype=np.int64) // nf)
    interior = int(np.argmax(np.where(np.isin(np.arange(nv), bc_nodes), -1, degree)))
    is_bc = np.isin(np.arange(nv), bc_nodes)
    for b in bc_nodes:
        for n in G.indices[G.indptr[b]:G.indptr[b + 1]]:
            if not is_bc[n] and n != interior:
                return interior, int(n)
    return interior, int(bc_nodes[0])


@pytest.mark.parametrize("case", CASES)
def test_scaled_spmv_matches_numpy(case, gpu_lib):
    prob = _problem(case)
    nf, n = prob.nf, prob.ndof
    u, un = R.case_state(case, prob)
    with gpu_lib.DeviceSolver(prob) as dev:
        dev.set_state(u, un)
        F, _ = dev.assemble(True)
        A = dev.jacobian_csr()
        with pytest.raises(gpu_lib.GmpnpError):
            dev.spmv_scaled(np.ones(n))                  # no set-up yet
        dev.linear_solve(R.case_rhs(case, F, A), gpu_lib.LINEAR_TWOLEVEL, 1e-10, 0.0, 20000)   # the set-up: Dinv, As
        As = (A @ R.block_inverse(A, nf)).tocsr()
        norm = np.sqrt((As.data ** 2).sum())
        interior, boundary = _probe_nodes(A, nf, prob.bc_dofs)
        xs = [("random", np.random.default_rng(12).standard_normal(n))]
        for what, node in (("interior", interior), ("boundary", boundary)):
            for j in range(nf):
                e = np.zeros(n)
                e[node * nf + j] = 1.0
                xs.append(("%s node %d column %d" % (what, node, j), e))
        worst = 0.0
        for what, x in xs:
            y = dev.spmv_scaled(x)
            assert np.array_equal(y, dev.spmv_scaled(x)), (case, what)      # bit-reproducible
            err = np.linalg.norm(y - As @ x) / (norm * np.linalg.norm(x))
            worst = max(worst, err)
            print("%s %s: |y - As x| / (|As|_F |x|) = %.3g" % (case, what, err))
            assert err < TOL, (case, what, err)
        # the unscaled operator still reads vals in its own layout
        x = xs[0][1]
        assert np.linalg.norm(dev.spmv(x) - A @ x) / np.linalg.norm(A @ x) < TOL
        print("%s: worst %.3g" % (case, worst))


def test_four_launch_form_gives_the_same_bits_on_box4_12(gpu_lib):
    """The invariant of tests/test_gpu_shapes.py on the smallest mesh that has a tail position: the four-launch form and the
    default form give array_equal solutions (both read vals_s through the same TileRows)."""
    case = "box4_12"
    prob = _problem(case)
    u, un = R.case_state(case, prob)
    out = {}
    for form in (0, 4):
        with gpu_lib.DeviceSolver(prob, launch_form=form) as dev:
            dev.set_state(u, un)
            F, _ = dev.assemble(True)
            if form == 4:
                assert dev.krylov_launches_per_iteration == 4
            for solver in (gpu_lib.LINEAR_TWOLEVEL, gpu_lib.LINEAR_JACOBI):
                x, st = dev.linear_solve(F, solver, 1e-10, 0.0, 20000)
                assert st["converged"], (form, solver, st)
                out[(form, solver)] = x
    for solver in (gpu_lib.LINEAR_TWOLEVEL, gpu_lib.LINEAR_JACOBI):
        assert np.array_equal(out[(0, solver)], out[(4, solver)]), solver
