"""The small-signal frequency response of the 3D pore (include/gmpnp.h ``gmpnp_frequency_response_3d``) restated
in NumPy over the existing restatements (imported like response_reference.py; not a conftest).

At a state u of a 3D ``prob`` with the Stern layer on (kinetics on or off), per unit of p_M and with i sigma in the place of inv_dt:
    (K + i sigma M) x = -b        K = J(u) at inv_dt = 0 (kinetics_reference.assemble: Stern rows facet by facet, kinetic rows, Dirichlet
                                  identity rows), M = the consistent P1 tetrahedron mass |K| (1 + delta_ab) / 20 on the species rows that
                                  carry no Dirichlet value, b = dF/dp_M (tangent_reference.column / galvanostat_reference.rhs_b)
    C = dD/dp_M + (dD/du).x       dI_r = dI_r/dp_M + (dI_r/du).x      tangent_reference.functionals on Re x and on Im x, the explicit
                                  d/dp_M part in the real part alone
The complex system is solved as the real 2N system [[K, -sigma M], [sigma M, K]] [Re x; Im x] = [-b; 0] with splu and with
galvanostat_reference.refined_solve (residuals in extended precision).  Test infrastructure only."""
import copy

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import galvanostat_reference as GR
import response_reference as R
import stern_bc_reference as SR
import tangent_reference as T
from gmpnp_amd import polarisation as pol
from gmpnp_amd.stern import L_STERN, coupled_g

# a parameter code whose explicit parts are all zero on the problems here (ln k of reaction 3; they have two reactions): what the
# imaginary part of x is given to tangent_reference.functionals with
PARAM_NO_EXPLICIT = 16 + 3
SIGMAS = (0.0, 1.0, 1e2, 1e4, 1e6, 1e14)


def cylinder_case(coarse, p_M=-1.0, stern_model="BDM", kinetics=True):
    """The generated cylinder ``coarse`` = (rings, layers) with the pore's full model, the Stern layer and two Tafel reactions (the
    'cyl259' problem of the Stern, kinetics and galvanostat tests at any size).  The mesh and the Dirichlet set are those of
    stern_bc_reference.bessel_stern_case(0, coarse=coarse): the potential free on the wall, p = 0 on both rims, no species condition.
    They are rebuilt here because that function asserts more than 50 interior vertices for its own closed form, which the smallest
    shapes ((1, 1): 14 vertices) do not have; (3, 6) gives the problem of the other tests, array for array."""
    import closed_forms as cf
    from test_kinetics_reference import two_reactions
    from gmpnp_amd.problem import SternLayer
    prob, m, ns, nv, wall = cf._base(50e-9, 5e-9, 0, coarse=coarse)
    prob = copy.copy(prob)
    zc = prob.coords[prob.bc_dofs // (ns + 1), 2]
    keep = ~wall | (np.abs(zc) < 1e-12) | (np.abs(zc - 1.0) < 1e-12)
    prob.bc_dofs, prob.bc_vals = prob.bc_dofs[keep], np.zeros(int(keep.sum()))
    prob.model = cf._base(10e-9, 5e-9, 0, reactions=True, wall_flux=True, steady=False, q_scale=1.0, coarse=coarse)[1]
    prob.stern = SternLayer(stern_model, p_M, L_STERN / 10e-9)
    prob.kinetics = two_reactions(list(prob.model.species), p_M) if kinetics else None
    return prob


def with_stern_and_kinetics(prob, p_M=-1.0, stern_model="BDM", lam=L_STERN / 10e-9):
    """``prob`` (a problem that prescribes the wall potential as a Dirichlet value, such as conftest.box_pore_problem's) with the Stern
    layer and two Tafel reactions in its place: the wall vertices lose the potential's Dirichlet value, except on the rims z = 0 and
    z = 1, where p = 0 stays (stern_bc_reference.bessel_stern_case's rule); the species conditions stay."""
    from test_kinetics_reference import two_reactions
    from gmpnp_amd.problem import SternLayer
    q = copy.copy(prob)
    nf = prob.nf
    dofs, vals = np.asarray(prob.bc_dofs), np.asarray(prob.bc_vals, dtype=np.float64).copy()
    pot = (dofs % nf) == nf - 1
    zc = np.asarray(prob.coords)[dofs // nf, 2]
    ends = (np.abs(zc) < 1e-12) | (np.abs(zc - 1.0) < 1e-12)
    keep = ~(pot & (vals != 0.0)) | ends
    vals[pot] = 0.0
    q.bc_dofs, q.bc_vals = dofs[keep], vals[keep]
    q.stern = SternLayer(stern_model, p_M, lam)
    q.kinetics = two_reactions(list(prob.model.species), p_M)
    return q


def cell_volumes(prob):
    X = np.asarray(prob.coords, dtype=np.float64)[np.asarray(prob.cells, dtype=np.int64)]
    return np.abs(np.linalg.det(X[:, 1:] - X[:, :1])) / 6.0


def mass(prob):
    """M from the mesh (CSR): |K| (1 + delta_ab) / 20 per tetrahedron on the species rows, zero on the potential and Dirichlet rows."""
    assert prob.coords.shape[1] == 3
    nf, ns = prob.nf, prob.nf - 1
    cells = np.asarray(prob.cells, dtype=np.int64)
    vol = cell_volumes(prob)
    rows, cols, vals = [], [], []
    for a in range(4):
        for b in range(4):
            w = vol * (1.0 / 20.0) * (2.0 if a == b else 1.0)
            for i in range(ns):
                rows.append(cells[:, a] * nf + i); cols.append(cells[:, b] * nf + i); vals.append(w)
    M = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(prob.ndof, prob.ndof)).tolil()
    for r in np.asarray(prob.bc_dofs, dtype=np.int64):
        M.rows[r], M.data[r] = [], []
    return M.tocsr()


def rhs_b(prob, u):
    """b = dF/dp_M: tangent_reference.column (galvanostat_reference.rhs_b) with the kinetics on, its Stern rows alone with them off."""
    if getattr(prob, "kinetics", None) is not None:
        return T.column(prob, u, pol.PARAM_P_M)
    nf, ns = prob.nf, prob.nf - 1
    u2d = np.asarray(u, dtype=np.float64).reshape(-1, nf)
    st = prob.stern
    eps0, epsc = float(prob.model.eps0), np.asarray(prob.model.epsc, dtype=np.float64)[:ns]
    b = np.zeros(prob.ndof)
    for f, ar in zip(np.asarray(prob.wall_facets, dtype=np.int64), SR.facet_areas(prob)):
        g, _ = coupled_g(st.model, eps0 + float(epsc @ u2d[f, :ns].mean(axis=0)), st.eps_surface)
        for a in range(3):
            b[f[a] * nf + ns] += g * (ar / 3.0) / st.lam
    b[prob.bc_dofs] = 0.0
    return b


def real_equivalent(K, M, sigma):
    """[[K, -sigma M], [sigma M, K]] (CSC)."""
    return sp.bmat([[K, -sigma * M], [sigma * M, K]], format="csc")


def solve(K, M, b, sigma, how="refined"):
    """x (complex; np.clongdouble for ``refined``) of (K + i sigma M) x = -b through the real 2N system; ``how`` = "splu" or
    "refined" (galvanostat_reference.refined_solve: three rounds of residuals in extended precision), or "both" from one factorisation."""
    n = K.shape[0]
    A = real_equivalent(K.tocsr(), M.tocsr(), float(sigma))
    rhs = np.r_[-np.asarray(b, dtype=np.float64), np.zeros(n)]
    lu = spla.splu(A)
    ys = lu.solve(rhs)
    if how == "splu":
        return ys[:n] + 1j * ys[n:]
    y = GR.refined_solve(A, lu, rhs)
    if how == "both":      # (refined as complex128, splu): one factorisation for the two
        return np.asarray(y[:n] + 1j * y[n:], dtype=np.complex128), ys[:n] + 1j * ys[n:]
    return y[:n] + 1j * y[n:]


def solve_complex(K, M, b, sigma, rounds=3):
    """(refined as complex128, splu) of (K + i sigma M) x = -b through ONE complex splu of the N system, refined with residuals
    formed in extended precision from the real K and M (refined_solve's scheme on complex vectors).  For meshes on which the real
    2N system fills in too far (L_10_R_5: minutes against about ten seconds; with the minimum-degree ordering of A^T A, 35e6 entries in
    the factors; the default column ordering takes about twice as long)."""
    Kc, Mc = K.tocoo(), M.tocoo()
    kd, md = Kc.data.astype(np.longdouble), Mc.data.astype(np.longdouble) * np.longdouble(sigma)
    lu = spla.splu((K + 1j * float(sigma) * M).tocsc(), permc_spec="MMD_ATA")
    xs = lu.solve(-np.asarray(b, dtype=np.complex128))
    xr, xi = xs.real.astype(np.longdouble), xs.imag.astype(np.longdouble)
    for _ in range(rounds):
        re, im = -np.asarray(b, dtype=np.longdouble), np.zeros(len(b), dtype=np.longdouble)
        np.subtract.at(re, Kc.row, kd * xr[Kc.col]); np.subtract.at(im, Kc.row, kd * xi[Kc.col])
        np.add.at(re, Mc.row, md * xi[Mc.col]); np.subtract.at(im, Mc.row, md * xr[Mc.col])
        d = lu.solve(np.asarray(re, dtype=np.float64) + 1j * np.asarray(im, dtype=np.float64))
        xr, xi = xr + d.real, xi + d.imag
    return np.asarray(xr, dtype=np.float64) + 1j * np.asarray(xi, dtype=np.float64), xs


def residual(K, M, b, sigma, x):
    """(max |(K + i sigma M) x + b| / max |b| evaluated in extended precision, the rounding of its fp64 evaluation over max |b|:
    a row is a sum of n terms (its entries of K and of sigma M and b), so n eps times the largest row sum of the absolute values of
    the terms bounds what any order of summation, and a mass entry that is itself a rounded sum, can move it by)."""
    xr, xi = np.asarray(x.real, dtype=np.longdouble), np.asarray(x.imag, dtype=np.longdouble)
    Kc, Mc = K.tocoo(), M.tocoo()
    kd, md = Kc.data.astype(np.longdouble), Mc.data.astype(np.longdouble) * np.longdouble(sigma)
    re, im = np.asarray(b, dtype=np.longdouble).copy(), np.zeros(len(b), dtype=np.longdouble)
    np.add.at(re, Kc.row, kd * xr[Kc.col]); np.add.at(im, Kc.row, kd * xi[Kc.col])
    np.subtract.at(re, Mc.row, md * xi[Mc.col]); np.add.at(im, Mc.row, md * xr[Mc.col])
    mod = np.sqrt(re * re + im * im)
    ax = np.abs(np.asarray(x, dtype=np.complex128))
    scale = abs(K) @ ax + float(sigma) * (abs(M) @ ax) + np.abs(b)
    bmax = float(np.abs(b).max())
    nterms = int(np.diff(K.tocsr().indptr).max() + np.diff(M.tocsr().indptr).max() + 1)
    return float(mod.max()) / bmax, float(nterms * np.finfo(float).eps * scale.max()) / bmax


def functionals(prob, u, x, want_scale=False):
    """(C, dI (nr,)) complex of a solution x (file order) by the rule's facet and node terms: tangent_reference.functionals with the
    p_M parameter on Re x and with a parameter without explicit parts on Im x.  ``want_scale``: also the sums of the absolute values of
    the terms, (aC_re, aI_re, aC_im, aI_im)."""
    assert len(prob.kinetics.reactions) <= 3 if getattr(prob, "kinetics", None) is not None else True
    xr, xi = np.asarray(x.real, dtype=np.float64), np.asarray(x.imag, dtype=np.float64)
    Dr, Ir, _, aDr, aIr = T.functionals(prob, u, xr, pol.PARAM_P_M, want_scale=True)
    Di, Ii, _, aDi, aIi = T.functionals(prob, u, xi, PARAM_NO_EXPLICIT, want_scale=True)
    C, dI = complex(Dr, Di), np.asarray(Ir, dtype=np.float64) + 1j * np.asarray(Ii, dtype=np.float64)
    return (C, dI, (aDr, aIr, aDi, aIi)) if want_scale else (C, dI)


def system(prob, u):
    """(K, M, b) of the NumPy restatement at the state u."""
    return R.jacobian(prob, u, 0.0), mass(prob), rhs_b(prob, u)


def potential_block_capacitance(prob, u, K, b):
    """C at sigma -> infinity (gmpnp_amd/impedance.py: potential_block_capacitance) and the x it belongs to."""
    from gmpnp_amd import impedance as imp
    nf = prob.nf
    rows = np.arange(nf - 1, prob.ndof, nf)
    return imp.potential_block_capacitance(K, b, rows, lambda x: T.functionals(prob, u, x, pol.PARAM_P_M)[0])
