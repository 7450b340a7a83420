"""The Stern-layer boundary condition of the potential (include/gmpnp.h ``gmpnp_set_stern``) restated in NumPy
over the oracle's assembly, and a Newton loop that applies it (imported like step_limit_reference.py; not a conftest).

    F_p += int_{Gamma_S} g(eps) (p_M - p) / lam v ds         eps = eps0 + sum_j epsc_j u_j,  g = gmpnp_amd.stern.coupled_g

    1D   eps at the OHP vertex v (Problem.point_vertices)
         F[p_v] += g (p_M - p_v) / lam      J[p_v, p_v] += -g / lam      J[p_v, u_{v,j}] += g' epsc_j (p_M - p_v) / lam
    3D   per wall facet f (Problem.wall_facets), eps at the facet mean of u, Mf = |f| (1 + delta_ab) / 12
         w_a = |f| (p_M / 3 - sum_b Mf_ab p_b / |f|)
         F[p_a] += g w_a / lam              J[p_a, p_b] += -g Mf_ab / lam      J[p_a, u_{b,j}] += g' (epsc_j / 3) w_a / lam

A potential row that is Dirichlet receives nothing (``assemble`` overwrites it like every Dirichlet row).  Test infrastructure only."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import gmpnp_oracle as O
from gmpnp_amd.stern import coupled_g
from step_limit_reference import LimitedStats, steric_sum, step_limit


def facet_areas(prob):
    X = prob.coords[prob.wall_facets]
    return 0.5 * np.linalg.norm(np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]), axis=1)


def stern_terms(prob, u, want_jacobian=True):
    """(Fs, (rows, cols, vals) or None): the Stern term of every potential row of the Stern boundary, Dirichlet rows included (the
    caller overwrites them), and its exact derivative as COO triplets.  ValueError where coupled_g refuses (eps <= 0, BDM)."""
    st = prob.stern
    nf, nv = prob.nf, prob.coords.shape[0]
    ns = nf - 1
    u2d = np.asarray(u, dtype=np.float64).reshape(nv, nf)
    eps0, epsc = float(prob.model.eps0), np.asarray(prob.model.epsc, dtype=np.float64)[:ns]
    Fs = np.zeros(prob.ndof)
    rows, cols, vals = [], [], []
    if prob.coords.shape[1] == 1:
        for v in np.asarray(prob.point_vertices, dtype=np.int64):
            eps = eps0 + float(epsc @ u2d[v, :ns])
            g, dg = coupled_g(st.model, eps, st.eps_surface)
            w = st.p_electrode - u2d[v, ns]
            r = v * nf + ns
            Fs[r] += g * w / st.lam
            if want_jacobian:
                rows.append(r); cols.append(r); vals.append(-g / st.lam)
                for j in range(ns):
                    rows.append(r); cols.append(v * nf + j); vals.append(dg * epsc[j] * w / st.lam)
    else:
        area = facet_areas(prob)
        for f, ar in zip(np.asarray(prob.wall_facets, dtype=np.int64), area):
            eps = eps0 + float(epsc @ u2d[f, :ns].mean(axis=0))
            g, dg = coupled_g(st.model, eps, st.eps_surface)
            p = u2d[f, ns]
            Mf = ar * (np.ones((3, 3)) + np.eye(3)) / 12.0
            w = ar * (st.p_electrode / 3.0 - (Mf @ p) / ar)
            for a in range(3):
                r = f[a] * nf + ns
                Fs[r] += g * w[a] / st.lam
                if want_jacobian:
                    for b in range(3):
                        rows.append(r); cols.append(f[b] * nf + ns); vals.append(-g * Mf[a, b] / st.lam)
                        for j in range(ns):
                            rows.append(r); cols.append(f[b] * nf + j); vals.append(dg * (epsc[j] / 3.0) * w[a] / st.lam)
    coo = (np.array(rows, dtype=np.int64), np.array(cols, dtype=np.int64), np.array(vals)) if want_jacobian else None
    return Fs, coo


def add_in_pattern(A, rows, cols, vals):
    """A copy of the CSR matrix A with the triplets added at their places in A's own pattern (explicit zeros stay; every Stern pair
    shares an element, so the place exists: asserted)."""
    A = A.tocsr(copy=True)
    A.sort_indices()
    S = sp.csr_matrix((vals, (rows, cols)), shape=A.shape)     # duplicates summed
    S.sort_indices()
    for r in np.unique(rows):
        a0, a1 = A.indptr[r], A.indptr[r + 1]
        sc, sv = S.indices[S.indptr[r]:S.indptr[r + 1]], S.data[S.indptr[r]:S.indptr[r + 1]]
        pos = np.searchsorted(A.indices[a0:a1], sc)
        assert (pos < a1 - a0).all() and np.array_equal(A.indices[a0:a1][pos], sc)
        A.data[a0 + pos] += sv
    return A


def assemble(prob, u, un, want_jacobian=True, apply_bc=True):
    """``gmpnp_oracle.assemble`` plus the Stern term of ``prob.stern`` (None: the oracle's own result)."""
    F, A = O.assemble(prob, u, un, want_jacobian=want_jacobian, apply_bc=False)
    if getattr(prob, "stern", None) is not None:
        Fs, coo = stern_terms(prob, u, want_jacobian)
        F = F + Fs
        if want_jacobian:
            A = add_in_pattern(A, *coo)
    if apply_bc and len(prob.bc_dofs):
        F[prob.bc_dofs] = u[prob.bc_dofs] - prob.bc_vals
        if A is not None:
            A = O.apply_identity_rows(A, prob.bc_dofs)
    return F, A


def stern_displacement(prob, u):
    """int_{Gamma_S} g (p_M - p) / lam ds over the potential rows that are NOT Dirichlet (what the potential row of the species budget
    reports in its wall / point column), scaled units."""
    Fs, _ = stern_terms(prob, u, want_jacobian=False)
    Fs[prob.bc_dofs] = 0.0
    return float(Fs.sum())


def newton_loop(prob, u, un, tau=0.0, omega=1.0, maximum_iterations=50, relative_tolerance=1e-9, absolute_tolerance=1e-6):
    """``step_limit_reference.newton_loop`` over ``assemble`` above (same statements otherwise); never raises on non-convergence, and
    stops where the residual is no longer finite.  Returns (u, LimitedStats)."""
    u = np.array(u, dtype=np.float64, copy=True)
    nv, nf = prob.coords.shape[0], prob.nf
    a = np.asarray(prob.model.a, dtype=np.float64)[:nf - 1]
    st = LimitedStats()
    b, _ = assemble(prob, u, un, want_jacobian=False)
    r = float(np.linalg.norm(b))
    r0 = r
    st.residuals.append(r)

    def conv(res):
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.float64(res) / np.float64(r0)
        return bool(rel < relative_tolerance or res < absolute_tolerance)

    done = conv(r)
    while not done and st.iterations < maximum_iterations and np.isfinite(r):
        b, A = assemble(prob, u, un, want_jacobian=True)
        dx = spla.splu(A.tocsc()).solve(b)
        if tau:
            alpha = step_limit(a, u.reshape(nv, nf), dx.reshape(nv, nf), tau)[0]
            u -= (omega * alpha) * dx
        else:
            alpha = 1.0
            u -= omega * dx
        st.step_factor.append(alpha)
        st.iterations += 1
        st.max_S.append(float(steric_sum(a, u.reshape(nv, nf)).max()))
        with np.errstate(all="ignore"):
            b, _ = assemble(prob, u, un, want_jacobian=False)
        r = float(np.linalg.norm(b))
        st.residuals.append(r)
        done = conv(r)
    st.converged = done
    return u, st


def bessel_stern_case(refine=0, V=-0.005, coarse=None, model="linear"):
    """``closed_forms.bessel_case`` with the wall potential applied through a Stern layer of lam = 1 / kappa instead of a Dirichlet
    value: eps_b dp/dr = eps_b (p_M - p) / lam at r = R gives  p / p_M = I0(kappa r) / (I0(kappa R) + lam kappa I1(kappa R)).
    Returns (problem, start state, check) with check(state) -> (max error, rms error, axis value of p / p_M, expected axis value)."""
    import copy
    from scipy.special import i0, i1
    import closed_forms as cf
    from gmpnp_amd.problem import SternLayer
    prob, state, _ = cf.bessel_case(refine, V=V, coarse=coarse)
    prob = copy.copy(prob)
    m = prob.model
    ns, nv = m.n_species, prob.coords.shape[0]
    z, bulk = np.asarray(m.z), np.asarray(m.bulk)
    eps_b = m.eps0 + float(np.sum(m.epsc))
    kappa = np.sqrt(m.q * float(np.sum(z * z * bulk)) / eps_b)
    # the wall vertices lose the potential's Dirichlet value, except those shared with S1 / S3 (z = 0, z = 1), where p = 0 stays
    zc = prob.coords[prob.bc_dofs // (ns + 1), 2]
    wall = prob.bc_vals != 0.0
    ends = (np.abs(zc) < 1e-12) | (np.abs(zc - 1.0) < 1e-12)
    keep = ~wall | ends
    prob.bc_dofs, prob.bc_vals = prob.bc_dofs[keep], np.zeros(int(keep.sum()))
    prob.stern = SternLayer(model=model, p_electrode=V, lam=1.0 / kappa)
    r = np.hypot(prob.coords[:, 0], prob.coords[:, 1])
    R = 0.1
    mid = (prob.coords[:, 2] > 0.3) & (prob.coords[:, 2] < 0.7) & (r < 0.999 * R)
    denom = i0(kappa * R) + prob.stern.lam * kappa * i1(kappa * R)

    def check(st):
        u = np.asarray(st).reshape(nv, ns + 1)
        d = u[mid, ns] / V - i0(kappa * r[mid]) / denom
        return np.abs(d).max(), np.sqrt((d ** 2).mean()), float((u[mid, ns] / V).min()), float(1.0 / denom)

    return prob, state, check
