"""NumPy restatement of the species-budget table (include/gmpnp.h, gmpnp_species_budget), independent of the device code.

Per field one row of ``COLUMNS``.  ``inventory`` ... ``point`` come from the mesh and the state with the closed-form P1 integrals
(int phi_a phi_b = |K| (1 + delta_ab) / ((d+1)(d+2)), int phi_a phi_b phi_c = |K| d! / (d+3)! (6 | 2 | 1 for three | two | no
equal indices), facet mass |f| (1 + delta_ab) / 12); ``closure`` is the sum of the oracle's assembled residual over the free dofs
(where the raw residual equals F); ``dirichlet`` is the remainder of the identity
    storage + reaction + wall + exit + point = dirichlet + closure.
``budget`` also returns, per entry, the sum of the absolute values of the shares it was added up from: the scale a comparison's
tolerance refers to (for ``dirichlet``: the sum of the scales of the entries it is the remainder of)."""
import math

import numpy as np

import gmpnp_oracle as O

COLUMNS = ("inventory", "storage", "reaction", "wall", "exit", "point", "dirichlet", "closure")
INV, STO, REA, WALL, EXIT, POINT, DIR, CLO = range(8)


def cell_volumes(coords, cells):
    X = coords[cells]
    if coords.shape[1] == 1:
        return np.abs(X[:, 1, 0] - X[:, 0, 0])
    return np.abs(np.linalg.det(X[:, 1:] - X[:, :1])) / 6.0


def facet_areas(coords, fv):
    X = coords[fv]
    return 0.5 * np.linalg.norm(np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]), axis=1)


def budget(prob, u, un, owned=None):
    """(table, scale), both (nf, 8).  ``owned`` (nv,) bool restricts every sum to the rows of those vertices (a partition's share);
    the closure then needs the residual of the whole problem all the same, which is what ``prob`` is."""
    m = prob.model
    nv, nf, ns = prob.coords.shape[0], prob.nf, prob.model.n_species
    d = prob.coords.shape[1]
    nn = d + 1
    own = np.ones(nv, dtype=bool) if owned is None else np.asarray(owned, dtype=bool)
    U, Un = np.asarray(u, dtype=float).reshape(nv, nf), np.asarray(un, dtype=float).reshape(nv, nf)
    cells = prob.cells
    vol = cell_volumes(prob.coords, cells)
    mden = 1.0 / ((d + 1) * (d + 2))
    kappa3 = math.factorial(d) / math.factorial(d + 3)
    Uc, dUc = U[cells], (U - Un)[cells]                                        # (nc, nn, nf)
    w = own[cells]                                                            # (nc, nn): is local node a's row counted
    M = mden * (np.ones((nn, nn)) + np.eye(nn))                               # int phi_a phi_b / |K|
    T = np.ones((nn, nn, nn))
    for a in range(nn):
        for b in range(nn):
            for c in range(nn):
                T[a, b, c] = 6.0 if a == b == c else (2.0 if (a == b or b == c or a == c) else 1.0)
    T *= kappa3                                                               # int phi_a phi_b phi_c / |K|

    table, scale = np.zeros((nf, 8)), np.zeros((nf, 8))

    def add(f, col, shares):
        """shares: per (cell or facet, local node) contributions already masked to the counted rows."""
        table[f, col] += shares.sum()
        scale[f, col] += np.abs(shares).sum()

    mass = vol[:, None, None] * np.einsum("ab,cbf->caf", M, Uc)               # int u_f phi_a over each cell
    dmass = vol[:, None, None] * np.einsum("ab,cbf->caf", M, dUc)
    for f in range(nf):
        add(f, INV, mass[:, :, f] * w)
    for i in range(ns):
        add(i, STO, m.inv_dt * dmass[:, :, i] * w)
        r = m.rc0[i] * vol[:, None] / nn * np.ones((1, nn))
        for j in range(ns):
            if m.rc1[i, j] != 0.0:
                r = r + m.rc1[i, j] * mass[:, :, j]
        for t, (bj, bk) in enumerate(m.bil):
            if m.rc2[i, t] != 0.0:
                r = r + m.rc2[i, t] * vol[:, None] * np.einsum("abc,nb,nc->na", T, Uc[:, :, bj], Uc[:, :, bk])
        add(i, REA, r * w)
    charge = np.zeros_like(mass[:, :, 0])
    for j in range(ns):
        charge = charge + m.q * m.z[j] * m.bulk[j] * mass[:, :, j]
    add(ns, REA, charge * w)

    if len(prob.wall_facets):
        fv = prob.wall_facets
        ar = facet_areas(prob.coords, fv)
        for i in range(ns):
            add(i, WALL, m.wall_flux[i] * (ar[:, None] / 3.0) * own[fv])
    if len(prob.exit_facets):
        fv = prob.exit_facets
        ar = facet_areas(prob.coords, fv)
        Mf = (np.ones((3, 3)) + np.eye(3)) / 12.0
        for i in range(ns):
            add(i, EXIT, m.exit_kappa[i] * ar[:, None] * (U[fv, i] @ Mf.T - 1.0 / 3.0) * own[fv])
    for v in prob.point_vertices:
        if own[int(v)]:
            for i in range(ns):
                add(i, POINT, np.array([m.point_flux[i]]))

    F, _ = O.assemble(prob, np.asarray(u, dtype=float).ravel(), np.asarray(un, dtype=float).ravel(), want_jacobian=False, apply_bc=True)
    free = np.ones(prob.ndof, dtype=bool)
    free[prob.bc_dofs] = False
    F2, free2 = F.reshape(nv, nf), free.reshape(nv, nf)
    for f in range(nf):
        sel = free2[:, f] & own
        add(f, CLO, F2[sel, f])
    lhs = (STO, REA, WALL, EXIT, POINT)
    table[:, DIR] = table[:, lhs].sum(axis=1) - table[:, CLO]
    scale[:, DIR] = scale[:, lhs].sum(axis=1) + scale[:, CLO]
    return table, scale


def n_free(prob, owned=None):
    """Free dofs per field (over the rows of ``owned``)."""
    nv, nf = prob.coords.shape[0], prob.nf
    free = np.ones(prob.ndof, dtype=bool)
    free[prob.bc_dofs] = False
    free = free.reshape(nv, nf)
    if owned is not None:
        free = free & np.asarray(owned, dtype=bool)[:, None]
    return free.sum(axis=0)
