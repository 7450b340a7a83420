"""High-precision references for the linear-algebra tests (imported like golden_cases.py; not a conftest).

* ``dd_residual`` / ``dd_backward_error``: b - A x of a SciPy CSR matrix in double-double (Dekker's split for every product,
  Knuth's TwoSum for every addition; the error terms are summed in a second double: Ogita, Rump and Oishi's Dot2).
* ``reference_solve``: sparse LU + iterative refinement on the double-double residual, with a 1-norm condition estimate.
* ``uniform_mesh_1d`` / ``graded_mesh_1d``: interval meshes of any nv >= 2 that ``edl_problem`` accepts as they are.
* ``bcr_model``: a NumPy model of the structure of the 1D direct solve (block cyclic reduction, gmpnp_kernels.h k_bcr_*):
  which rows survive a level, how the last odd row is eliminated, Gauss-Jordan with or without partial pivoting inside a
  block.  Test infrastructure only — it shows that the tests' inputs tell a correct kernel from a subtly wrong one.
* ``bcr_tail_levels``: the row counts of the levels ``tri_solve`` (gmpnp_api.hip) hands to the one-wave k_bcr_tail.
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

U = np.finfo(np.float64).eps / 2          # unit roundoff, 2^-53
_SPLIT = 134217729.0                      # 2^27 + 1


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = _SPLIT * a
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _as_dd(b):
    if isinstance(b, tuple):
        return np.asarray(b[0], dtype=np.float64), np.asarray(b[1], dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return b, np.zeros_like(b)


def dd_matvec(A, x):
    """A x in double-double: (hi, lo) with hi + lo accurate to about u^2 |A| |x| per row."""
    return dd_residual(A, -np.asarray(x, dtype=np.float64), 0.0 * np.asarray(x, dtype=np.float64), split=True)


def dd_residual(A, x, b, split=False):
    """b - A x for a SciPy sparse matrix A, computed in double-double.  ``b`` may be an array or a (hi, lo) pair; returns
    the residual rounded to fp64 (or the (hi, lo) pair with ``split=True``)."""
    A = sp.csr_matrix(A)
    A.sort_indices()
    x = np.asarray(x, dtype=np.float64)
    bh, bl = _as_dd(b)
    n = A.shape[0]
    s, e = bh.copy(), bl.copy()
    cnt = np.diff(A.indptr)
    for k in range(int(cnt.max()) if n else 0):      # k-th stored entry of every row that has one
        rows = np.nonzero(cnt > k)[0]
        pos = A.indptr[rows] + k
        p, pe = _two_prod(-A.data[pos], x[A.indices[pos]])
        s[rows], se = _two_sum(s[rows], p)
        e[rows] += se + pe
    hi, lo = _two_sum(s, e)
    return (hi, lo) if split else hi + lo


def dd_backward_error(A, x, b):
    """Normwise backward error ||b - A x||_inf / (||A||_inf ||x||_inf + ||b||_inf), the residual in double-double."""
    r = dd_residual(A, x, b)
    bh, _ = _as_dd(b)
    nA = abs(sp.csr_matrix(A)).sum(axis=1).max()
    return float(np.abs(r).max() / (nA * np.abs(x).max() + np.abs(bh).max()))


def cond1_estimate(A, lu=None):
    """kappa_1(A) = ||A||_1 ||A^-1||_1 with Hager / Higham's estimator (scipy onenormest) on the LU factors."""
    A = sp.csc_matrix(A)
    lu = lu or spla.splu(A)
    n = A.shape[0]
    inv = spla.LinearOperator((n, n), matvec=lu.solve, rmatvec=lambda y: lu.solve(y, trans="T"), dtype=np.float64)
    return float(abs(A).sum(axis=0).max() * spla.onenormest(inv))


class IllConditioned(ValueError):
    """kappa_1 u > 1e-2: refinement is not guaranteed to converge; use backward-error criteria only."""


def reference_solve(A, b, max_refinements=40):
    """x = A^{-1} b to working accuracy: SciPy's sparse LU, then iterative refinement with the double-double residual until
    the correction is below 1e-17 of x (normwise).  The fp64 x cannot always get there: when a correction changes nothing, or
    stays at the last-bit level (< 4u ||x||) without shrinking (a component flips between two neighbouring doubles around a
    solution that lies half-way), x is as accurate as fp64 holds it and the loop stops too.  Returns (x, kappa_1 estimate).
    Raises IllConditioned when kappa_1 u > 1e-2."""
    A = sp.csr_matrix(A)
    lu = spla.splu(A.tocsc())
    kappa = cond1_estimate(A, lu)
    if kappa * U > 1e-2:
        raise IllConditioned("kappa_1 ~ %.2e: refinement is not reliable, use backward-error criteria" % kappa)
    bh, bl = _as_dd(b)
    x = lu.solve(bh)
    dprev = np.inf
    for _ in range(max_refinements):
        d = lu.solve(dd_residual(A, x, (bh, bl)))
        xn = x + d
        dn, xm = np.abs(d).max(), np.abs(xn).max()
        if dn <= 1e-17 * xm or np.array_equal(xn, x) or (dn <= 4 * U * xm and dn > 0.5 * dprev):
            return xn, kappa
        x, dprev = xn, dn
    raise RuntimeError("iterative refinement did not settle in %d steps (kappa_1 ~ %.2e)" % (max_refinements, kappa))


def max_rel(x, ref):
    """||x - ref||_inf / ||ref||_inf."""
    return float(np.abs(np.asarray(x) - ref).max() / max(np.abs(ref).max(), 1e-300))


# ---- 1D meshes ------------------------------------------------------------------------------------
def _interval_mesh(x):
    from gmpnp_amd.mesh import Mesh
    nv = len(x)
    cells = np.stack([np.arange(nv - 1), np.arange(1, nv)], axis=1).astype(np.int32)
    return Mesh(dim=1, coords=np.ascontiguousarray(x, dtype=np.float64)[:, None], cells=cells)


def uniform_mesh_1d(nv):
    """nv equidistant vertices on [0, 1] (nv >= 2)."""
    assert nv >= 2
    return _interval_mesh(np.linspace(0.0, 1.0, nv))


def graded_mesh_1d(nv, ratio=1e3):
    """nv vertices on [0, 1], the finest cell at x = 0 and geometric growth to h_max / h_min = ratio (<= 1e3) at x = 1,
    like the reference's variable meshes (0.1 nm cells at the electrode)."""
    assert nv >= 2 and 1.0 <= ratio <= 1e3
    nc = nv - 1
    g = ratio ** (1.0 / (nc - 1)) if nc > 1 else 1.0
    h = g ** np.arange(nc)
    x = np.concatenate([[0.0], np.cumsum(h)])
    x /= x[-1]
    x[-1] = 1.0
    return _interval_mesh(x)


# ---- the 1D direct solve --------------------------------------------------------------------------
def bcr_tail_levels(nv, tail_rows=4, tail_levels=8):
    """Row counts of the levels that run in the one-wave k_bcr_tail, lowest first.  Mirrors tri_solve (gmpnp_api.hip:
    kBcrTailRows = 4, kBcrTailLevels = 8 in gmpnp_kernels.h): it must change when that rule does."""
    ns = [nv]
    while ns[-1] > 1:
        ns.append((ns[-1] + 1) // 2)
    nl = len(ns)
    l0 = nl - 1
    while l0 > 0 and ns[l0] <= tail_rows and nl - l0 < tail_levels:
        l0 -= 1
    return ns[l0:], l0


def tri_blocks(A, nf):
    """Block-tridiagonal (L, D, U) of a 1D Jacobian in path order: (n, nf, nf) each, L[0] = U[n-1] = 0."""
    A = sp.csr_matrix(A)
    n = A.shape[0] // nf
    Ad = A.toarray() if n <= 64 else None

    def blk(i, j):
        if Ad is not None:
            return Ad[i * nf:(i + 1) * nf, j * nf:(j + 1) * nf]
        return A[i * nf:(i + 1) * nf, j * nf:(j + 1) * nf].toarray()
    if Ad is None:   # vectorised extraction: every entry of a 1D Jacobian lies in one of the three block diagonals
        C = A.tocoo()
        bi, bj = C.row // nf, C.col // nf
        assert np.all(np.abs(bi - bj) <= 1)
        out = np.zeros((3, n, nf, nf))
        out[bj - bi + 1, bi, C.row % nf, C.col % nf] = C.data
        return out[0], out[1], out[2]
    L, D, Uu = np.zeros((n, nf, nf)), np.zeros((n, nf, nf)), np.zeros((n, nf, nf))
    for i in range(n):
        D[i] = blk(i, i)
        if i > 0:
            L[i] = blk(i, i - 1)
        if i + 1 < n:
            Uu[i] = blk(i, i + 1)
    return L, D, Uu


def gauss_jordan(D, R, pivot=True):
    """Solve D_k X_k = R_k for a batch (m, nf, nf) / (m, nf, c) by Gauss-Jordan elimination, rows kept in place: in step k the
    pivot is the row with the largest |D[., k]| among the rows not used yet (the first of equal ones), or row k without
    pivoting."""
    W = np.concatenate([D, R], axis=2).astype(np.float64, copy=True)
    m, nf, _ = D.shape
    used = np.zeros((m, nf), dtype=bool)
    home = np.zeros((m, nf), dtype=np.int64)
    ar = np.arange(m)
    for k in range(nf):
        if pivot:
            mag = np.where(used, -1.0, np.abs(W[:, :, k]))
            p = np.argmax(mag, axis=1)
        else:
            p = np.full(m, k)
        used[ar, p] = True
        home[:, k] = p
        prow = W[ar, p] / W[ar, p, k][:, None]
        f = W[:, :, k].copy()
        f[ar, p] = 0.0
        W -= f[:, :, None] * prow[:, None, :]
        W[ar, p] = prow
    return W[ar[:, None], home, nf:]


def bcr_model(blocks, rhs, pivot=True):
    """Block cyclic reduction of the block-tridiagonal system (L, D, U) x = rhs ((n, nf) or (n*nf,)), with the kernels' rules:
    the even rows of a level survive to the next; every odd row is eliminated by its left (even) neighbour — the last row,
    when odd, has no right neighbour and is eliminated the same way with U = 0; each neighbour block is solved by
    Gauss-Jordan (``gauss_jordan``).  Returns x as (n*nf,)."""
    L, D, Uu = (np.asarray(a, dtype=np.float64) for a in blocks)
    n, nf, _ = D.shape
    b = np.asarray(rhs, dtype=np.float64).reshape(n, nf)
    levels = []
    while n > 1:
        odd = np.arange(1, n, 2)
        X = gauss_jordan(D[odd], np.concatenate([L[odd], Uu[odd], b[odd][:, :, None]], axis=2), pivot)
        Li, Ui, bi = X[:, :, :nf], X[:, :, nf:2 * nf], X[:, :, 2 * nf]
        ev = np.arange(0, n, 2)
        nh = len(ev)
        Lh, Dh, Uh, bh = np.zeros((nh, nf, nf)), D[ev].copy(), np.zeros((nh, nf, nf)), b[ev].copy()
        # left neighbour of even row 2i is odd row 2i-1 = odd[i-1]; right neighbour 2i+1 = odd[i]
        il = np.arange(1, nh)
        Lh[il] = -L[ev[il]] @ Li[il - 1]
        Dh[il] -= L[ev[il]] @ Ui[il - 1]
        bh[il] -= np.einsum("kij,kj->ki", L[ev[il]], bi[il - 1])
        ir = np.nonzero(ev + 1 < n)[0]
        Dh[ir] -= Uu[ev[ir]] @ Li[ir]
        Uh[ir] = -Uu[ev[ir]] @ Ui[ir]
        bh[ir] -= np.einsum("kij,kj->ki", Uu[ev[ir]], bi[ir])
        levels.append((n, Li, Ui, bi))
        L, D, Uu, b, n = Lh, Dh, Uh, bh, nh
    x = gauss_jordan(D, b[:, :, None], pivot)[:, :, 0]
    for n, Li, Ui, bi in reversed(levels):
        xl = np.zeros((n, nf))
        xl[0::2] = x
        odd = np.arange(1, n, 2)
        xr = np.zeros((len(odd), nf))
        has_r = odd + 1 < n
        xr[has_r] = x[(odd[has_r] + 1) // 2]
        xl[odd] = bi - np.einsum("kij,kj->ki", Li, x[(odd - 1) // 2]) - np.einsum("kij,kj->ki", Ui, xr)
        x = xl
    return x.ravel()


def level0_pivoted_blocks(blocks):
    """Number of level-0 diagonal blocks whose LAPACK LU (scipy.linalg.lu_factor, partial pivoting) swaps rows."""
    import scipy.linalg as sla
    D = blocks[1]
    cnt = 0
    for k in range(D.shape[0]):
        _, piv = sla.lu_factor(D[k], check_finite=False)
        cnt += int(np.any(piv != np.arange(D.shape[1])))
    return cnt


# ---- the inputs of the 1D sweep (shared by test_hp_reference.py and test_gpu_shapes.py) ------------------------------
SWEEP_NV = (2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 33, 64, 65, 129, 1025, 4097)
# (mesh, nv, potential range P): a state whose potential is drawn from U(-P, 0) at every vertex (steep, unphysical fields).
# On these the model WITHOUT pivoting misses the solve tolerance with the residual F as right-hand side while the pivoted one
# meets it (test_hp_reference.py); the physical and the U(0.5, 1.5) states are solved to tolerance without any pivoting.  They
# are solved with F only.  The 4-vertex one runs entirely in k_bcr_tail, the 129-vertex one has five forward levels below it.
NEEDS_PIVOTING = (("graded", 4, 3000.0), ("graded", 129, 1000.0))
# the five reference meshes of the 1D driver and the golden state that goes with each (None: a random state)
REFERENCE_1D = (("edl1", dict(L_n=1e-6, cation="Cs", voltage_multiplier=-5.0)),
                ("edl5_na", dict(L_n=5e-6, cation="Na", voltage_multiplier=-2.5)),
                ("edl10_hohp", dict(L_n=10e-6, voltage_multiplier=-2.5, H_OHP=0.5, H2_FE=0.4)),
                ("edl50", dict(cation="Cs", voltage_multiplier=-10.0)),
                (None, "1D_variable_200um_mesh_4998.xml.gz"))   # (no parameter set of the driver loads it: SURVEY Q8)
KRYLOV_Q_SCALE = 1e-4      # q / 1e4 (q ~ 1e5): node-block Jacobi BiCGStab converges on the uniform 1D meshes (as closed_forms._base)


def jacobi_bicgstab(A, b, rtol=1e-10, nf=7):
    """SciPy's BiCGStab with node-block Jacobi (the inverse of every nf x nf diagonal block) to ``rtol``: the CPU counterpart
    of the device's Jacobi BiCGStab, for Newton solves whose outcome depends on the Krylov error."""
    n = A.shape[0] // nf
    M = sp.block_diag([np.linalg.inv(A[i * nf:(i + 1) * nf, i * nf:(i + 1) * nf].toarray()) for i in range(n)]).tocsr()
    x, info = spla.bicgstab(A, b, rtol=rtol, atol=0.0, M=M, maxiter=20000)
    if info != 0:
        raise RuntimeError("node-block Jacobi BiCGStab did not converge (info %d)" % info)
    return x


def edl_generated(mesh, q_scale=1.0, **kw):
    """The 1D EDL problem (edl50 parameters unless overridden) on a generated interval mesh, q scaled by ``q_scale``."""
    import copy
    from gmpnp_amd.params import edl_parameters
    from gmpnp_amd.problem import edl_problem
    prob = edl_problem(edl_parameters(**(kw or dict(cation="Cs", voltage_multiplier=-10.0))), mesh)
    if q_scale != 1.0:
        m = copy.deepcopy(prob.model)
        m.q = m.q * q_scale
        prob = copy.copy(prob)
        prob.model = m
    return prob


def steep_state(nv, P, seed):
    from conftest import random_state
    u, un = random_state(nv, 6, seed=seed)
    u = u.reshape(nv, 7)
    u[:, 6] = np.random.default_rng(seed + 100).uniform(-P, 0.0, nv)
    return u.ravel(), un


def sweep_1d_inputs(golden_dir):
    """Every (id, problem, u, un, needs_pivoting) of the 1D sweep: generated uniform and graded meshes of SWEEP_NV vertices
    with a random state (a uniform state too on the uniform ones), the steep NEEDS_PIVOTING inputs, and the five reference
    meshes with their golden state (second dry-run step) where one exists."""
    import os
    from conftest import _edl, random_state
    out = []
    for nv in SWEEP_NV:
        for kind in ("uniform", "graded"):
            mesh = uniform_mesh_1d(nv) if kind == "uniform" else graded_mesh_1d(nv)
            prob = edl_generated(mesh)
            u, un = random_state(nv, 6, seed=nv)
            out.append(("%s%d-random" % (kind, nv), prob, u, un, False))
            if kind == "uniform":
                w = np.tile(np.r_[np.ones(6), 0.0], nv)
                out.append(("%s%d-uniform" % (kind, nv), prob, w, w.copy(), False))
    for kind, nv, P in NEEDS_PIVOTING:
        mesh = uniform_mesh_1d(nv) if kind == "uniform" else graded_mesh_1d(nv)
        u, un = steep_state(nv, P, nv)
        out.append(("%s%d-steep%g" % (kind, nv, P), edl_generated(mesh), u, un, True))
    for name, kw in REFERENCE_1D:
        if name is None:
            from gmpnp_amd.mesh import read_dolfin_xml, resolve_mesh_path
            from gmpnp_amd.params import utilities_dir
            mesh = read_dolfin_xml(resolve_mesh_path(utilities_dir(), kw))
            prob, nv = edl_generated(mesh), mesh.num_vertices
            u, un = random_state(nv, 6, seed=7)
            name = "edl200-random"
        else:
            _, mesh, prob = _edl(**kw)
            g = np.load(os.path.join(golden_dir, name + "_steps.npz"))
            u, un = g["states"][1], g["states"][0]
        out.append((name, prob, u, un, False))
    return out


def direct_solve_tolerances(A, rhs, lu):
    """The 1D direct solve's acceptance limits on (A, rhs): backward error <= max(10 x that of SciPy's splu, 1e-14) and forward
    error against reference_solve <= max(10 x that of splu, 1e-13).  Returns (x_ref or None when ill-conditioned, tol_be, tol_fe)."""
    xs = lu.solve(rhs)
    tb = max(10.0 * dd_backward_error(A, xs, rhs), 1e-14)
    try:
        xr, _ = reference_solve(A, rhs)
    except IllConditioned:
        return None, tb, None
    return xr, tb, max(10.0 * max_rel(xs, xr), 1e-13)


def forward_limit(tf, model_fe):
    """The forward limit of the 1D direct solve on one input: 10x splu's forward error (``tf``), or 2x that of the model of the
    reduction itself where the model needs more than that (the reduction, not the kernel, is less forward-accurate than sparse
    LU there: the golden state of the 10 um mesh, F, model 2.59e-11 against splu 2.66e-12)."""
    return 2.0 * model_fe if model_fe > tf else tf


def meets_direct_tolerance(A, x, rhs, limits):
    xr, tb, tf = limits
    if not np.all(np.isfinite(x)) or dd_backward_error(A, x, rhs) > tb:
        return False
    return xr is None or max_rel(x, xr) <= tf
