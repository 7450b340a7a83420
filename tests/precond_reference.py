"""A restatement of the BiCGStab preconditioners M^-1 of the library in NumPy / SciPy (imported like hp_reference.py; not a
conftest), and of the device's right-preconditioned BiCGStab, so that a test can say WHICH operator a kernel got wrong.

    As   = J Dinv                        Dinv = inverses of the NF x NF diagonal node blocks of J (Dirichlet rows: identity rows)
    Aci  = (P^T As P)^-1                 P = per field, piecewise constant on the slab aggregates, no Dirichlet mask
    M^-1 = Dinv (I + P Aci P^T)          Jacobi mode: M^-1 = Dinv                           (gmpnp_kernels.h)
    multilevel:  M^-1 += theta * mask P_1 S_1 P_1^T mask                                    (gmpnp_multilevel.h)
    S_L r:  x = w M_L^-1 r;  x += mask P S_{L+1} mask P^T (r - J_L x);  x += w M_L^-1 (r - J_L x)   (gmpnp_api.hip, ml_level_apply)

Sparse operators only (the coarse matrix, nagg * NF square, is the one dense object); LAPACK inverses for the node blocks and
for P^T As P, the latter refined to fp64 accuracy (refined_inverse).  Test infrastructure only.  The constants mirrored here must change when the library's rule does:

* ``ML_OMEGA = 0.7``       gmpnp_solver::ml_omega (gmpnp_api.hip): damping w of every smoothing step of the V-cycle.
* ``ML_MID_JACOBI = True`` gmpnp_solver::ml_mid_jacobi: an intermediate level smooths with Dinv_L alone, the coarsest level with
                           its own two-level M_L^-1; the coarsest has no coarse-grid correction and repeats the post-smoothing
                           step ``sweeps - 1`` times.
* ``ML_THETA = 2.0``, ``ML_SWEEPS = 4``   the defaults of DeviceSolver.attach_coarse_level / solver.py (ml_theta, ml_sweeps).
* ``aggregates`` / ``aggregate_count``    gmpnp_topology.cpp: aggregate g is the range [nv*g/nagg, nv*(g+1)/nagg) of the vertex
                           order ``DeviceSolver.perm`` (the degree re-sort stays inside an aggregate); nagg = the request capped by
                           min(kMaxCoarse / NF, 16) (kMaxCoarse = 140, gmpnp_internal.h) or 8 by default, at most nv / 8, at least 1,
                           and lowered until no block row touches more than kMaxRowAggs = 4 aggregates.
"""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

import hp_reference as H

ML_OMEGA = 0.7
ML_MID_JACOBI = True
ML_THETA = 2.0
ML_SWEEPS = 4
K_MAX_COARSE = 140
K_MAX_ROW_AGGS = 4
NOISE = 2.0 ** -52          # the relative perturbation of the rounding-sensitivity runs
TOL_FLOOR, TOL_FACTOR, TOL_CEILING = 1e-12, 100.0, 1e-6
K_COMPARED = 4              # iterations the tests look at (steps whose tolerance exceeds TOL_CEILING are not compared)
N_NOISE_RUNS = 3


# ---- aggregates ------------------------------------------------------------------------------------------------------
def aggregates(perm, nv, nagg):
    """agg[file vertex] = g for the vertices perm[nv*g/nagg : nv*(g+1)/nagg] (integer division, as the library's int64 one)."""
    perm = np.asarray(perm, dtype=np.int64)
    assert perm.shape == (nv,) and nagg >= 1
    agg = np.empty(nv, dtype=np.int64)
    for g in range(nagg):
        agg[perm[nv * g // nagg: nv * (g + 1) // nagg]] = g
    return agg


def aggregate_count(perm, cells, nv, nf, requested=0):
    """The number of aggregates gmpnp_create grants for ``n_aggregates = requested`` (0: the default)."""
    nagg_max = min(K_MAX_COARSE // nf, 16)
    while nagg_max > 1 and ((nagg_max * nf) ** 2 + nagg_max * nf * nf + 2 * nf * nf) * 8 > 160 * 1024:
        nagg_max -= 1
    nagg = min(requested, nagg_max) if requested > 0 else min(nagg_max, 8)
    nagg = max(1, min(nagg, nv // 8 if nv // 8 > 0 else 1))
    cells = np.asarray(cells, dtype=np.int64)
    k = cells.shape[1]
    rows, cols = np.repeat(cells, k, axis=1).ravel(), np.tile(cells, (1, k)).ravel()
    while nagg > 1:
        agg = aggregates(perm, nv, nagg)
        pairs = np.unique(rows * nagg + agg[cols])            # (vertex, aggregate of a neighbour)
        if np.bincount(pairs // nagg, minlength=nv).max() <= K_MAX_ROW_AGGS:
            break
        nagg -= 1
    return nagg


def aggregate_prolongation(agg, nf):
    """P (n x nagg*nf): dof (I, f) belongs to coarse dof (agg[I], f)."""
    agg = np.asarray(agg, dtype=np.int64)
    nv, nagg = len(agg), int(agg.max()) + 1
    rows = np.arange(nv * nf)
    cols = np.repeat(agg, nf) * nf + np.tile(np.arange(nf), nv)
    return sp.csr_matrix((np.ones(nv * nf), (rows, cols)), shape=(nv * nf, nagg * nf))


# ---- the operators ---------------------------------------------------------------------------------------------------
def block_inverse(A, nf):
    """Dinv as a sparse block-diagonal matrix: the LAPACK inverse of every nf x nf diagonal block of A."""
    A = sp.csr_matrix(A)
    n = A.shape[0]
    nv = n // nf
    C = A.tocoo()
    on = (C.row // nf) == (C.col // nf)
    D = np.zeros((nv, nf, nf))
    np.add.at(D, (C.row[on] // nf, C.row[on] % nf, C.col[on] % nf), C.data[on])
    Di = np.linalg.inv(D)                                     # LAPACK getrf / getri, block by block
    return sp.bsr_matrix((Di, np.arange(nv), np.arange(nv + 1)), shape=(n, n)).tocsr()


def jacobi_minv(A, nf):
    """y -> Dinv y."""
    Dinv = block_inverse(A, nf)
    return lambda y: Dinv @ y


def refined_inverse(M, steps=3):
    """inv(M) to fp64 accuracy: LAPACK's inverse, then Newton-Schulz steps X += X (I - M X) with the residual in double-double
    (hp_reference's TwoProd / TwoSum).  P^T As P has kappa_2 = 2e8 on the 3D cases and LAPACK's inverse alone is 6e-11 of |Aci| off
    (a block Gauss-Jordan like k_coarse_invert's: 1e-11) — enough to move ||b - A x_1|| of the model by 3e-9."""
    M = np.asarray(M, dtype=np.float64)
    n = M.shape[0]
    X = sla.inv(M, check_finite=False)
    for _ in range(steps):
        s, e = np.eye(n), np.zeros((n, n))
        for k in range(n):
            p, pe = H._two_prod(-M[:, k:k + 1], X[k:k + 1, :])
            s, se = H._two_sum(s, p)
            e += se + pe
        X = X + X @ (s + e)
    return X


def noisy_gauss_jordan(M, noise, rng):
    """inv(M) by Gauss-Jordan elimination with partial pivoting in which every product is multiplied by 1 + noise * N(0, 1)."""
    n = M.shape[0]
    W = np.concatenate([np.asarray(M, dtype=np.float64), np.eye(n)], axis=1)
    for k in range(n):
        p = k + int(np.argmax(np.abs(W[k:, k])))
        if p != k:
            W[[k, p]] = W[[p, k]]
        W[k] = W[k] * ((1.0 / W[k, k]) * (1.0 + noise * rng.standard_normal(2 * n)))
        f = W[:, k].copy()
        f[k] = 0.0
        W -= np.outer(f, W[k]) * (1.0 + noise * rng.standard_normal((n, 2 * n)))
        W[:, k] = 0.0
        W[k, k] = 1.0
    return W[:, n:]


def noisy_inverse(M, nf, noise, rng):
    """What rounding alone does to the coarse inverse AS THE LIBRARY FORMS IT (k_coarse_invert): an in-place
    BLOCK Gauss-Jordan elimination, block = one aggregate (nf x nf), pivoting inside the diagonal block only, every product
    multiplied by 1 + noise * N(0, 1).  The pivot rule is part of the sensitivity: with kappa_2(P^T As P) = 2e8 the error that
    block elimination leaves lies in the direction ||b - A x_k|| feels — on cyl3_9 an exact-arithmetic-order block Gauss-Jordan
    in fp64 moves ||b - A x_1|| by 3e-9 although its Aci is 1e-11 accurate, LAPACK's (6e-11) by 1e-10, noise on a partially
    pivoted elimination (4e-10) by 8e-12."""
    A = np.array(M, dtype=np.float64)
    n = A.shape[0]

    def jit(X):
        return X * (1.0 + noise * rng.standard_normal(X.shape))
    for K in range(n // nf):
        s = slice(K * nf, (K + 1) * nf)
        D = noisy_gauss_jordan(A[s, s], noise, rng)
        colK = A[:, s].copy()
        rowK = jit(D[:, :, None] * A[s, :][None, :, :]).sum(axis=1)
        rowK[:, s] = D
        upd = jit(colK[:, :, None] * rowK[None, :, :]).sum(axis=1)
        A[:, s] = 0.0
        A -= upd
        A[s, :] = rowK
    return A


def two_level_minv(A, nf, agg, P=None, R=None, coarse_from=None, noise=0.0, seed=0):
    """y -> Dinv (I + P Aci P^T) y with Aci = (P^T A Dinv P)^-1.  ``P``, ``R`` and ``coarse_from`` exist for the tests that show
    what a wrong operator looks like: ``P`` replaces the prolongation everywhere, ``R`` replaces P^T in the APPLICATION only (Aci
    stays that of P), ``coarse_from`` = another Jacobian whose (P^T A' Dinv' P)^-1 is used as Aci (a lagged coarse operator).
    ``noise`` > 0: the products of the SET-UP carry the rounding noise of right_bicgstab too — A (Dinv P) componentwise, and the
    inverse through noisy_inverse (the library's elimination order)."""
    A = sp.csr_matrix(A)
    Dinv = block_inverse(A, nf)
    P = aggregate_prolongation(agg, nf) if P is None else sp.csr_matrix(P)
    R = P.T.tocsr() if R is None else sp.csr_matrix(R)
    if coarse_from is None:
        AsP = A @ (Dinv @ P)
    else:
        Ao = sp.csr_matrix(coarse_from)
        AsP = Ao @ (block_inverse(Ao, nf) @ P)
    if noise > 0.0:
        rng = np.random.default_rng(1000 + seed)
        AsP = AsP.tocsr(copy=True)
        AsP.data *= 1.0 + noise * rng.standard_normal(AsP.data.shape)
        Aci = noisy_inverse((P.T @ AsP).toarray(), nf, noise, rng)
    else:
        Aci = refined_inverse((P.T @ AsP).toarray())
    return lambda y: Dinv @ (y + P @ (Aci @ (R @ y)))


def level_prolongation(parents, nv_coarse, nf):
    """P_l (level l <- level l+1) of a red-refined mesh: a vertex whose two parents are equal is a copy, else the mean."""
    par = np.asarray(parents, dtype=np.int64).reshape(-1, 2)
    nv = par.shape[0]
    copy = par[:, 0] == par[:, 1]
    rows = np.concatenate([np.arange(nv), np.arange(nv)[~copy]])
    cols = np.concatenate([par[:, 0], par[~copy, 1]])
    w = np.concatenate([np.where(copy, 1.0, 0.5), np.full((~copy).sum(), 0.5)])
    Pv = sp.csr_matrix((w, (rows, cols)), shape=(nv, nv_coarse))
    return sp.kron(Pv, sp.identity(nf), format="csr")


def inject_state(u_fine, parents, nv_coarse, nf):
    """The state one level down: a coarse vertex takes the value of the fine vertex that copies it."""
    par = np.asarray(parents, dtype=np.int64).reshape(-1, 2)
    copy = np.nonzero(par[:, 0] == par[:, 1])[0]
    out = np.full((nv_coarse, nf), np.nan)
    out[par[copy, 0]] = np.asarray(u_fine).reshape(-1, nf)[copy]
    assert np.isfinite(out).all()
    return out.ravel()


MASKS = ("restrict_fine", "restrict_coarse", "prolong")


def multilevel_minv(levels, parents, theta=ML_THETA, omega=ML_OMEGA, sweeps=ML_SWEEPS, mid_jacobi=ML_MID_JACOBI, restrictions=None,
                    masks=MASKS, jacobi_base=False, noise=0.0, seed=0):
    """y -> (Dinv (I + P Aci P^T) + theta mask P_1 S_1 P_1^T mask) y; with ``jacobi_base`` the term is added to Dinv alone (what
    the Jacobi mode of a handle with an attached level applies).

    ``levels``: finest first, one dict per level with "A" (the level's Jacobian, rediscretised at the injected state: CSR),
    "nf", "bc" (boolean Dirichlet mask of its dofs) and "agg" (its aggregates); ``parents[l]`` the (nv_l, 2) table of level l's
    vertices in level l + 1.  ``restrictions`` (a list of matrices in place of P_l^T) and ``masks`` (which of the three transfer
    masks are applied) exist for the tests that show what a wrong operator looks like; ``noise``: as in two_level_minv, for
    every two-level operator of the hierarchy."""
    nf = levels[0]["nf"]
    nl = len(levels)
    assert nl >= 2 and len(parents) == nl - 1
    A = [sp.csr_matrix(lv["A"]) for lv in levels]
    free = [(~np.asarray(lv["bc"], dtype=bool)).astype(np.float64) for lv in levels]
    Pl = [level_prolongation(parents[l], A[l + 1].shape[0] // nf, nf) for l in range(nl - 1)]
    Rl = [p.T.tocsr() for p in Pl] if restrictions is None else [sp.csr_matrix(r) for r in restrictions]
    base = jacobi_minv(A[0], nf) if jacobi_base else two_level_minv(A[0], nf, levels[0]["agg"], noise=noise, seed=seed)
    smooth = [None] + [jacobi_minv(A[l], nf) if (l < nl - 1 and mid_jacobi) else
                       two_level_minv(A[l], nf, levels[l]["agg"], noise=noise, seed=seed + 100 * l) for l in range(1, nl)]
    mf = lambda l, v: free[l] * v if "restrict_fine" in masks else v          # noqa: E731
    mc = lambda l, v: free[l] * v if "restrict_coarse" in masks else v        # noqa: E731
    mp = lambda l, v: free[l] * v if "prolong" in masks else v                # noqa: E731

    def restrict(l, v):       # level l -> l + 1
        return mc(l + 1, Rl[l] @ mf(l, v))

    def prolong(l, w):        # level l + 1 -> l
        return mp(l, Pl[l] @ w)

    def cycle(l, r):
        x = omega * smooth[l](r)
        if l < nl - 1:
            x = x + prolong(l, cycle(l + 1, restrict(l, r - A[l] @ x)))
            x = x + omega * smooth[l](r - A[l] @ x)
        else:
            for _ in range(1, sweeps):
                x = x + omega * smooth[l](r - A[l] @ x)
        return x

    return lambda y: base(y) + theta * prolong(0, cycle(1, restrict(0, y)))


# ---- the device's BiCGStab -------------------------------------------------------------------------------------------
def right_bicgstab(A, minv, b, K, noise=0.0, seed=0, true_residuals=True):
    """K iterations of the right-preconditioned BiCGStab of the library (gmpnp_kernels.h, coarse_a_body / coarse_b_body): shadow
    vector r_0, p = r + beta (p - omega v), v = A M^-1 p, s = r - alpha v, t = A M^-1 s, x += alpha M^-1 p + omega M^-1 s; the
    convergence test is made on r_k at the start of iteration k, so a solve that reports k iterations returns x_k.
    Returns (xs, rec, true): x_0 ... x_K, the recurrence residual norms ||r_k|| and the true residuals b - A x_k as vectors
    (hp_reference.dd_residual: double-double; None with ``true_residuals=False``).
    ``noise`` > 0 multiplies every product with M^-1 and with A componentwise by 1 + noise * N(0, 1)."""
    A = sp.csr_matrix(A)
    b = np.asarray(b, dtype=np.float64)
    rng = np.random.default_rng(seed)

    def jitter(v):
        return v * (1.0 + noise * rng.standard_normal(v.shape)) if noise > 0.0 else v

    def M(v):
        return jitter(minv(v))

    def Av(v):
        return jitter(A @ v)

    x, r = np.zeros_like(b), b.copy()
    rhat, p = r.copy(), r.copy()
    rho = float(rhat @ r)
    xs, rec = [x.copy()], [float(np.linalg.norm(r))]
    for _ in range(K):
        ph = M(p)
        v = Av(ph)
        alpha = rho / float(rhat @ v)
        s = r - alpha * v
        sh = M(s)
        t = Av(sh)
        omega = float(t @ s) / float(t @ t)
        x = x + alpha * ph + omega * sh
        r = s - omega * t
        rho_new = float(rhat @ r)
        beta = (rho_new / rho) * (alpha / omega)
        p = r + beta * (p - omega * v)
        rho = rho_new
        xs.append(x.copy())
        rec.append(float(np.linalg.norm(r)))
    true = [b.copy()] + [H.dd_residual(A, xk, b) for xk in xs[1:]] if true_residuals else None
    return xs, np.array(rec), true


def stopping_rungs(rel_history):
    """The iterations k at which a solve can be made to stop by its tolerance: [(k, rtol_k)] for every k >= 1 with
    min_{j<k} rho_j >= 1.5 rho_k (rho_k = ||r_k|| / ||b||), rtol_k = sqrt(min_{j<k} rho_j * rho_k)."""
    rho = np.asarray(rel_history, dtype=np.float64)
    out = []
    for k in range(1, len(rho)):
        lo = rho[:k].min()
        if lo >= 1.5 * rho[k]:
            out.append((k, float(np.sqrt(lo * rho[k]))))
    return out


class Observables:
    """What the tests compare of one (matrix, M^-1, right-hand side): the exact model's x_k and ||b - A x_k||, the rounding
    sensitivities d_k of both (the largest relative change over N_NOISE_RUNS seeded runs with noise 2^-52), the tolerances
    tol_k = max(1e-12, 100 d_k), the capped steps kept (tol_k <= 1e-6) and the rungs kept [(k, rtol_k)].
    ``make_minv(noise, seed)`` builds the operator: the noise runs perturb the products of its set-up as well as those of the
    iteration (the coarse inverse is the most rounding-sensitive part of M^-1)."""

    def __init__(self, A, make_minv, b, K=K_COMPARED, noise_runs=N_NOISE_RUNS):
        A = sp.csr_matrix(A)
        self.K = K
        self.xs, self.rec, rvec = right_bicgstab(A, make_minv(0.0, 0), b, K)
        self.true = np.array([float(np.linalg.norm(r)) for r in rvec])
        bn = float(np.linalg.norm(b))
        self.rel = self.rec / bn
        dx, dr = np.zeros(K + 1), np.zeros(K + 1)
        for seed in range(1, noise_runs + 1):
            xs, _, _ = right_bicgstab(A, make_minv(NOISE, seed), b, K, noise=NOISE, seed=seed, true_residuals=False)
            for k in range(1, K + 1):
                dx[k] = max(dx[k], H.max_rel(xs[k], self.xs[k]))
                # b - A x' = (b - A x_k) - A (x' - x_k): the first term in double-double, the second is 1e-10 of it at the most and
                # its fp64 rounding far below anything compared here
                tr = float(np.linalg.norm(rvec[k] - A @ (xs[k] - self.xs[k])))
                dr[k] = max(dr[k], abs(tr - self.true[k]) / self.true[k])
        self.d_x, self.d_res = dx, dr
        self.tol_x = np.maximum(TOL_FLOOR, TOL_FACTOR * dx)
        self.tol_res = np.maximum(TOL_FLOOR, TOL_FACTOR * dr)
        self.capped = [k for k in range(1, K + 1) if self.tol_res[k] <= TOL_CEILING]
        self.rungs = [(k, rt) for k, rt in stopping_rungs(self.rel) if self.tol_x[k] <= TOL_CEILING]

    def meets_conditions(self):
        """At least k = 1, 2, 3 of the capped history and the rung k = 1."""
        return {1, 2, 3} <= set(self.capped) and any(k == 1 for k, _ in self.rungs)


def two_level_factory(A, nf, agg):
    return lambda noise, seed: two_level_minv(A, nf, agg, noise=noise, seed=seed)


def jacobi_factory(A, nf):
    minv = jacobi_minv(A, nf)
    return lambda noise, seed: minv


def multilevel_factory(levels, parents, **kw):
    return lambda noise, seed: multilevel_minv(levels, parents, noise=noise, seed=seed, **kw)


def distance(model, other):
    """The largest |difference| / tol over the quantities both compare at k <= 3 (other: an Observables of a mutated operator, or
    any object with .xs and .true, the true residual NORMS): > 1 means a test with ``model``'s tolerances tells them apart."""
    worst = 0.0
    for k in range(1, 4):
        if k in model.capped:
            worst = max(worst, abs(other.true[k] - model.true[k]) / model.true[k] / model.tol_res[k])
        if any(k == kk for kk, _ in model.rungs):
            worst = max(worst, H.max_rel(other.xs[k], model.xs[k]) / model.tol_x[k])
    return worst


# ---- the cases (shared by test_precond_reference.py and test_gpu_precond.py) ------------------------------------------------
CASES_3D = (("cyl1_1", 0), ("cyl1_4", 0), ("box2_3", 0), ("cyl3_9", 0), ("box4_12", 0), ("box5_17", 0), ("box5_17", 16), ("pore10", 0))
CASES_1D = tuple((nv, nagg) for nv in (9, 10, 65, 577) for nagg in (0, 1, 16))
STATE_SEED = 11
CASE_SEED = {"cyl1_4": 21}  # at seed 11 (and most others) d_3 of the two-level mode is 1e-8 on this mesh: 100 d_3 straddles the 1e-6 ceiling


# The one (case, mode) that cannot meet the input conditions (k = 1, 2, 3 kept and a rung at k = 1), whatever the seed (11 ... 22
# tried) or the right-hand side: on cyl3_9 (370 vertices, 8 aggregates that straddle its 37-vertex layers) the block elimination
# of k_coarse_invert amplifies rounding by kappa_2(P^T As P) = 2e8 into the direction the first iterates feel: d_1 ... d_3 =
# 9e-9, 2e-8, 6e-8 of ||b - A x_k|| and 4e-7, 4e-8, 7e-8 of x_k (a partially pivoted elimination: 8e-12, 4e-11, 3e-10).  The
# inverse itself is as accurate as LAPACK's (1e-11 against 6e-11 of |Aci|), so this is the attainable accuracy of the operator on
# that mesh, not a defect; the steps whose tolerance stays below 1e-6 are still compared, and the Jacobi mode meets the conditions.
ROUNDING_LIMITED = {("cyl3_9", "two-level")}


def case_state(case, prob):
    """(u, un) of a case: random_state with seed 11 unless CASE_SEED names another."""
    from conftest import random_state
    return random_state(prob.coords.shape[0], prob.nf - 1, seed=CASE_SEED.get(case, STATE_SEED))


def x_true(n):
    rng = np.random.default_rng(6)
    return rng.uniform(1.0, 2.0, n) * rng.choice([-1.0, 1.0], n)


def case_rhs(case, F, A):
    """The right-hand side of a case: F, or A x_true on the generated cylinders ("cyl...", and the hierarchies "ml..."): with F
    the two-level residual of those grows over the first iterations and no solve can be stopped by its tolerance."""
    return A @ x_true(A.shape[0]) if case.startswith(("cyl", "ml")) else F
ML_CYLINDER = (2, 5)        # the generated cylinder the hierarchies are refined from (114 vertices)


def problem_3d(name):
    """The 3D problems of tests/test_gpu_shapes.py by name (cyl<rings>_<layers>, box<nx>_<nz>) and the reference mesh pore10."""
    if name == "pore10":
        from conftest import _pore
        return _pore(10e-9, 5e-9)[2]
    a, b = (int(v) for v in name[3:].split("_"))
    if name.startswith("cyl"):
        import closed_forms as cf
        return cf._base(10e-9, 5e-9, 0, reactions=True, wall_flux=True, steady=False, q_scale=1.0, coarse=(a, b))[0]
    from conftest import box_pore_problem
    return box_pore_problem(a, b)[2]


def problem_1d(nv):
    return H.edl_generated(H.uniform_mesh_1d(nv), q_scale=H.KRYLOV_Q_SCALE)


def cylinder_hierarchy(refine, coarse=ML_CYLINDER):
    """The nested problems of the generated cylinder refined ``refine`` times, FINEST first: [(problem, parents)] like
    gmpnp_amd.problem.pore_hierarchy (parents None on the coarsest), with the model and the potential-only Dirichlet
    conditions of closed_forms._base(..., coarse=coarse) as problem_3d uses it; the facets are marked once, on the generated
    mesh with its own wall tolerance, and inherited under refinement."""
    from gmpnp_amd.mesh import mark_pore_boundaries, refine_pore
    from gmpnp_amd.meshgen import cylinder_mesh
    from gmpnp_amd.params import pore_parameters
    from gmpnp_amd.problem import Problem, pore_dirichlet
    pp = pore_parameters(concentration_elec=0.5, L=10e-9, R=5e-9)
    mesh = cylinder_mesh(pp.aspect_pore, coarse[0], coarse[1])
    sag = pp.aspect_pore ** 2 * (1.0 - np.cos(np.pi / (6 * coarse[0])) ** 2)
    levels = [(mesh, mark_pore_boundaries(mesh, pp.aspect_pore, 1.5 * sag))]
    for _ in range(refine):
        levels.append(refine_pore(*levels[-1]))
    ns = len(pp.species)
    out = []
    for m, bnd in levels[::-1]:
        dofs, vals = pore_dirichlet(pp, bnd)
        keep = (dofs % (ns + 1)) == ns
        prob = Problem(coords=m.coords, cells=m.cells, model=pp.model, wall_facets=bnd.ds_facets[2], exit_facets=bnd.ds_facets[3],
                       bc_dofs=dofs[keep], bc_vals=vals[keep])
        out.append((prob, getattr(m, "parents", None)))
    return out


def problem_perm(prob):
    from gmpnp_amd.backend import slab_permutation
    return slab_permutation(np.ascontiguousarray(prob.coords, dtype=np.float64), np.ascontiguousarray(prob.cells, dtype=np.int32), window=0)


def problem_aggregates(prob, requested=0, perm=None):
    """(agg, nagg) of a problem as gmpnp_create forms them for ``n_aggregates = requested`` and the default vertex order."""
    perm = problem_perm(prob) if perm is None else perm
    nv = prob.coords.shape[0]
    nagg = aggregate_count(perm, prob.cells, nv, prob.nf, requested)
    return aggregates(perm, nv, nagg), nagg


def bc_mask(prob):
    m = np.zeros(prob.ndof, dtype=bool)
    m[np.asarray(prob.bc_dofs, dtype=np.int64)] = True
    return m


def hierarchy_levels(hier, u, un, A0=None):
    """The ``levels`` / ``parents`` arguments of multilevel_minv for a hierarchy [(problem, parents)] (finest first) at the fine
    state (u, un): every coarser level's Jacobian is gmpnp_oracle.assemble of its problem at the injected state; ``A0`` (the
    device's matrix) replaces the oracle's on the finest level."""
    import gmpnp_oracle as O
    levels, parents = [], []
    for l, (prob, par) in enumerate(hier):
        nv = prob.coords.shape[0]
        if l > 0:
            u, un = (inject_state(v, hier[l - 1][1], nv, prob.nf) for v in (u, un))
        A = A0 if (l == 0 and A0 is not None) else O.assemble(prob, u, un)[1]
        levels.append({"A": A, "nf": prob.nf, "bc": bc_mask(prob), "agg": problem_aggregates(prob)[0]})
        if par is not None:
            parents.append(par)
    return levels, parents


# ---- the device Jacobian against the oracle's (moved here from test_gpu_shapes.py) ----------------------------------------------
def relerr(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def frob_rel(A, B):
    D = (A - B).tocsr()
    return np.sqrt((D.data ** 2).sum()) / np.sqrt((B.data ** 2).sum())


def assembly_matches(dev, prob, u, un):
    """Assembly, CSR pattern and SpMV against the oracle (1e-12, identical pattern, 1e-13) on a random state of the mesh (on
    the uniform and the converged states F is a difference of nearly equal terms and 1e-12 of its norm is below their
    rounding), then the state (u, un) is assembled; returns (oracle F, device J) of that state."""
    import gmpnp_oracle as O
    from conftest import random_state
    nv = prob.coords.shape[0]
    ur, unr = random_state(nv, prob.nf - 1, seed=3)
    dev.set_state(ur, unr)
    F, _ = dev.assemble(True)
    A = dev.jacobian_csr()
    Fo, Ao = O.assemble(prob, ur, unr)
    assert relerr(F, Fo) < 1e-12
    assert A.nnz == Ao.nnz and np.array_equal(A.indptr, Ao.indptr) and np.array_equal(A.indices, Ao.indices)
    assert frob_rel(A, Ao) < 1e-12
    x = np.random.default_rng(12).standard_normal(prob.ndof)
    assert relerr(dev.spmv(x), Ao @ x) < 1e-13
    dev.set_state(u, un)
    dev.assemble(True)
    A = dev.jacobian_csr()
    Fo, Ao = O.assemble(prob, u, un)
    assert A.nnz == Ao.nnz and np.array_equal(A.indptr, Ao.indptr) and np.array_equal(A.indices, Ao.indices)
    assert frob_rel(A, Ao) < 1e-12
    return Fo, A
