"""The potential-dependent surface kinetics (include/gmpnp.h ``gmpnp_set_kinetics``) restated in NumPy over the
oracle's assembly (and over the Stern restatement of stern_bc_reference.py, which the option works together with), and a Newton loop
that applies it (imported like stern_bc_reference.py; not a conftest).

At every node I of the Stern boundary (1D: Problem.point_vertices, 3D: the vertices of Problem.wall_facets), p_M = kinetics.p_electrode:
    E_r = exp(-alpha_r (p_M - p_I - p_eq_r))        rate_r = k_r (u_{I,reactant_r} or 1) E_r
    F[(I,i)] += w_I sum_r nu[r][i] rate_r           J[(I,i),(I,reactant_r)] += w_I nu[r][i] k_r E_r
                                                    J[(I,i),(I,p)]          += w_I nu[r][i] alpha_r rate_r
w_I = 1 (1D) or the sum over the wall facets holding I of |f| / 3 in list order (3D).  A species row that is Dirichlet receives
nothing (``assemble`` overwrites it like every Dirichlet row).  Test infrastructure only."""
import numpy as np
import scipy.sparse.linalg as spla

import gmpnp_oracle as O
import stern_bc_reference as SR
from gmpnp_amd.kinetics import surface_rate
from step_limit_reference import LimitedStats, steric_sum, step_limit


def boundary_weights(prob):
    """(nodes ascending, w_I) of the Stern boundary."""
    nv = prob.coords.shape[0]
    w = np.zeros(nv)
    if prob.coords.shape[1] == 1:
        np.add.at(w, np.asarray(prob.point_vertices, dtype=np.int64), 1.0)
        nodes = np.unique(np.asarray(prob.point_vertices, dtype=np.int64))
    else:
        fv = np.asarray(prob.wall_facets, dtype=np.int64)
        np.add.at(w, fv.ravel(), np.repeat(SR.facet_areas(prob) / 3.0, 3))     # unbuffered: facet list order
        nodes = np.unique(fv)
    return nodes, w[nodes]


def resolved(prob):
    """[(k, alpha, p_eq, reactant index or -1, nu (ns,))] of prob.kinetics, species by index."""
    species = list(prob.model.species)
    ns = prob.nf - 1
    out = []
    for r in prob.kinetics.reactions:
        nu = np.zeros(ns)
        for name, v in r.nu.items():
            nu[species.index(name)] = v
        out.append((float(r.k), float(r.alpha), float(r.p_eq), -1 if r.reactant is None else species.index(r.reactant), nu))
    return out


def node_rates(prob, u2d, I):
    """[(rate, d_u, d_p, ok)] of the reactions at node I."""
    ns = prob.nf - 1
    p_M = float(prob.kinetics.p_electrode)
    return [surface_rate(k, al, pe, p_M, u2d[I, ns], re >= 0, u2d[I, re] if re >= 0 else 0.0) for k, al, pe, re, _ in resolved(prob)]


def kinetic_terms(prob, u, want_jacobian=True):
    """(Fk, (rows, cols, vals) or None, ok): the kinetic term of every species row of the Stern boundary, Dirichlet rows included (the
    caller overwrites them), its exact derivative as COO triplets (entries that are identically zero left out), and whether every
    rate was finite."""
    nf, nv = prob.nf, prob.coords.shape[0]
    ns = nf - 1
    u2d = np.asarray(u, dtype=np.float64).reshape(nv, nf)
    rx = resolved(prob)
    Fk = np.zeros(prob.ndof)
    rows, cols, vals = [], [], []
    ok = True
    nodes, w = boundary_weights(prob)
    for I, wI in zip(nodes, w):
        R = node_rates(prob, u2d, I)
        ok = ok and all(r[3] for r in R)
        for i in range(ns):
            term = 0.0
            with np.errstate(all="ignore"):
                for (k, al, pe, re, nu), (rate, d_u, d_p, _) in zip(rx, R):
                    if nu[i] == 0.0:
                        continue
                    term += nu[i] * rate
                    if want_jacobian:
                        if re >= 0:
                            rows.append(I * nf + i); cols.append(I * nf + re); vals.append(wI * (nu[i] * d_u))
                        if al != 0.0:
                            rows.append(I * nf + i); cols.append(I * nf + ns); vals.append(wI * (nu[i] * d_p))
                Fk[I * nf + i] += wI * term
    coo = (np.array(rows, dtype=np.int64), np.array(cols, dtype=np.int64), np.array(vals)) if want_jacobian else None
    return Fk, coo, ok


def kinetic_free_rows(prob):
    """The species dofs of the Stern boundary that a reaction drives and that are not Dirichlet."""
    nf = prob.nf
    nodes, _ = boundary_weights(prob)
    driven = np.nonzero(np.any([nu != 0.0 for *_, nu in resolved(prob)], axis=0))[0]
    rows = (nodes[:, None] * nf + driven[None, :]).ravel()
    return np.setdiff1d(rows, prob.bc_dofs)


def assemble(prob, u, un, want_jacobian=True, apply_bc=True):
    """``stern_bc_reference.assemble`` (the oracle plus the Stern term of ``prob.stern``) plus the kinetic term of ``prob.kinetics``."""
    F, A = SR.assemble(prob, u, un, want_jacobian=want_jacobian, apply_bc=False)
    if getattr(prob, "kinetics", None) is not None:
        Fk, coo, _ = kinetic_terms(prob, u, want_jacobian)
        F = F + Fk
        if want_jacobian and len(coo[0]):
            A = SR.add_in_pattern(A, *coo)
    if apply_bc and len(prob.bc_dofs):
        F[prob.bc_dofs] = u[prob.bc_dofs] - prob.bc_vals
        if A is not None:
            A = O.apply_identity_rows(A, prob.bc_dofs)
    return F, A


def currents(prob, u):
    """sum_I w_I rate_r per reaction (what gmpnp_kinetics_currents returns)."""
    nv = prob.coords.shape[0]
    u2d = np.asarray(u, dtype=np.float64).reshape(nv, prob.nf)
    nodes, w = boundary_weights(prob)
    out = np.zeros(len(prob.kinetics.reactions))
    for I, wI in zip(nodes, w):
        out += wI * np.array([r[0] for r in node_rates(prob, u2d, I)])
    return out


def species_fluxes(prob, u):
    """Per species: the integrated kinetic flux over the rows that are NOT Dirichlet (what the species rows of the budget gain in their
    wall / point column)."""
    Fk, _, _ = kinetic_terms(prob, u, want_jacobian=False)
    Fk[prob.bc_dofs] = 0.0
    return Fk.reshape(-1, prob.nf)[:, :prob.nf - 1].sum(axis=0)


def newton_loop(prob, u, un, tau=0.0, omega=1.0, maximum_iterations=50, relative_tolerance=1e-9, absolute_tolerance=1e-6):
    """``stern_bc_reference.newton_loop`` over ``assemble`` above (same statements otherwise); never raises on non-convergence, and
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
