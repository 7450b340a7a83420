"""The electrode tangent (include/gmpnp.h ``gmpnp_electrode_tangent``) restated in NumPy over the response,
kinetics and Stern restatements (response_reference.py, kinetics_reference.py, stern_bc_reference.py), with the parameter maps the
tests difference against (imported like response_reference.py; not a conftest).

At a state u of ``prob`` (1D, Stern layer on, kinetics on or off), for the parameters theta (0 = p_M, 16 + r = ln k_r, 32 + r = alpha_r,
48 = ln lam):
    J z = -c,  c = dF/dtheta          dD = dD/dtheta + (dD/du).z          dI_r = dI_r/dtheta + (dI_r/du).z
Test infrastructure only (1D)."""
import copy
import dataclasses
import math

import numpy as np
import scipy.sparse.linalg as spla

import galvanostat_reference as GR
import kinetics_reference as K
import response_reference as R
import stern_bc_reference as SR
from gmpnp_amd import polarisation as pol
from gmpnp_amd.stern import coupled_g


def with_parameter(prob, param, delta):
    """``prob`` with parameter ``param`` moved by ``delta`` (p_M, ln k_r, alpha_r or ln lam), everything else as it is."""
    kind, r = pol.param_kind(param), pol.param_reaction(param)
    if kind == 0:
        return R.with_potential(prob, prob.stern.p_electrode + delta)
    q = copy.copy(prob)
    if kind == 3:
        q.stern = dataclasses.replace(prob.stern, lam=prob.stern.lam * math.exp(delta))
        return q
    rx = list(prob.kinetics.reactions)
    rx[r] = dataclasses.replace(rx[r], k=rx[r].k * math.exp(delta)) if kind == 1 else dataclasses.replace(rx[r], alpha=rx[r].alpha + delta)
    q.kinetics = dataclasses.replace(prob.kinetics, reactions=rx)
    return q


def residual(prob, u, un=None, inv_dt=0.0):
    """F(u) at ``inv_dt`` with u_n = ``un`` (None: u)."""
    return K.assemble(R.with_inv_dt(prob, inv_dt), u, u if un is None else un, want_jacobian=False)[0]


def displacement(prob, u):
    return SR.stern_displacement(prob, u)


def currents(prob, u):
    return np.asarray(K.currents(prob, u), dtype=np.float64) if getattr(prob, "kinetics", None) is not None else np.zeros(0)


def column(prob, u, param):
    """c = dF/dtheta, closed form; every Dirichlet row 0."""
    kind, r = pol.param_kind(param), pol.param_reaction(param)
    if kind == 0:
        return R.rhs_b(prob, u)
    nf, ns = prob.nf, prob.nf - 1
    u2d = np.asarray(u, dtype=np.float64).reshape(-1, nf)
    c = np.zeros(prob.ndof)
    if kind == 3:
        st = prob.stern
        eps0, epsc = float(prob.model.eps0), np.asarray(prob.model.epsc, dtype=np.float64)[:ns]
        for v in np.asarray(prob.point_vertices, dtype=np.int64):
            g, _ = coupled_g(st.model, eps0 + float(epsc @ u2d[v, :ns]), st.eps_surface)
            c[v * nf + ns] += -(g * (st.p_electrode - u2d[v, ns]) / st.lam)
    else:
        rx = K.resolved(prob)
        nodes, w = K.boundary_weights(prob)
        for I, wI in zip(nodes, w):
            k, al, pe, re, nu = rx[r]
            rate, d_u, d_p, _ = K.node_rates(prob, u2d, I)[r]
            eta = prob.kinetics.p_electrode - u2d[I, ns] - pe
            e = pol.rate_explicit(param, r, rate, d_p, eta)
            for i in range(ns):
                c[I * nf + i] += wI * (float(nu[i]) * e)
    c[np.asarray(prob.bc_dofs, dtype=np.int64)] = 0.0
    return c


def explicit(prob, u, param):
    """(dD/dtheta, dI_r/dtheta (nr,)) at fixed u, closed form."""
    kind, r = pol.param_kind(param), pol.param_reaction(param)
    dD0, _ = R.displacement_row(prob, u)
    I = currents(prob, u)
    dI = np.zeros(len(I))
    dD = 0.0
    if kind == 0:
        dD = dD0
        dI0, _ = R.current_rows(prob, u)
        dI = np.asarray(dI0, dtype=np.float64)
    elif kind == 3:
        dD = -displacement(prob, u)
    elif kind == 1:
        dI[r] = I[r]
    elif kind == 2:
        nf, ns = prob.nf, prob.nf - 1
        u2d = np.asarray(u, dtype=np.float64).reshape(-1, nf)
        rx = K.resolved(prob)
        nodes, w = K.boundary_weights(prob)
        for J, wJ in zip(nodes, w):
            rate = K.node_rates(prob, u2d, J)[r][0]
            dI[r] += -wJ * rate * (prob.kinetics.p_electrode - u2d[J, ns] - rx[r][2])
    return dD, dI


def tangent(prob, u, params, inv_dt=0.0, how="splu"):
    """(z (n, ndof), dD (n,), dI (n, nr), dp_boundary (n,)) of the parameters ``params`` at the state u."""
    A = R.jacobian(prob, u, inv_dt).tocsc()
    lu = spla.splu(A)
    rowD = R.displacement_row(prob, u)[1]
    rowsI = R.current_rows(prob, u)[1]
    nf = prob.nf
    pv = np.asarray(prob.point_vertices, dtype=np.int64)
    z, dD, dI, dp = [], [], [], []
    for q in params:
        c = column(prob, u, q)
        x = np.asarray(GR.refined_solve(A, lu, -c), dtype=np.float64) if how == "refined" else lu.solve(-c)
        eD, eI = explicit(prob, u, q)
        z.append(x); dD.append(eD + rowD @ x); dI.append(eI + rowsI @ x); dp.append(float(np.mean(x[pv * nf + nf - 1])))
    return np.array(z), np.array(dD), np.array(dI).reshape(len(params), -1), np.array(dp)


def steady_state(prob, u0, iterations=40, tol=1e-9):
    """Newton at inv_dt = 0 from u0 with sparse LU: returns (u, iterations, converged).  Once ||F|| <= tol max(||F_0||, 1) one more
    step is taken, which by the quadratic convergence leaves the state at its rounding floor (the differences of steady states and
    the predictor errors below need that)."""
    u = np.array(u0, dtype=np.float64, copy=True)
    q = R.with_inv_dt(prob, 0.0)
    r0 = None
    for it in range(iterations):
        F, A = K.assemble(q, u, u, want_jacobian=True)
        r = float(np.linalg.norm(F))
        if not np.isfinite(r):
            return u, it, False
        r0 = r if r0 is None else r0
        u = u - spla.splu(A.tocsc()).solve(F)
        if r <= tol * max(r0, 1.0):
            return u, it, bool(np.isfinite(u).all())
    return u, iterations, False


class NumpySystem:
    """The operations ``polarisation.run_continuation`` asks of a handle, over the NumPy restatement."""

    def __init__(self, prob, u):
        self.prob, self.u, self.kept = prob, np.array(u, dtype=np.float64), np.array(u, dtype=np.float64)
        self.z = None
        self.failed = 0

    def solve(self):
        u, its, ok = steady_state(self.prob, self.u)
        if ok:
            self.u = u
        else:
            self.failed += 1
        return ok, its, (currents(self.prob, u) if ok else None)

    def point(self, p):
        z, dD, dI, dp = tangent(self.prob, self.u, [pol.PARAM_P_M])
        self.z = z[0]
        return {"p_M": p, "u": self.u.copy(), "potential_OHP": float(self.u[self.prob.nf - 1]), "displacement": displacement(self.prob, self.u),
                "currents": currents(self.prob, self.u), "tangent": {"dD": dD, "dI": dI, "dp_boundary": dp, "residual": np.zeros(1)}}

    def predict(self, dp, predictor):
        if predictor:
            self.u = self.u + dp * self.z

    def set_potential(self, p):
        self.prob = R.with_potential(self.prob, p)

    def keep(self):
        self.kept = self.u.copy()

    def back(self, p):
        self.u = self.kept.copy()
        self.set_potential(p)


def functionals(prob, u, z, param, want_scale=False):
    """(dD, dI (n_reactions,), dp_boundary) of the tangent ``z`` (file order) for parameter ``param`` at the state ``u`` (1D or 3D, Stern
    layer on, kinetics on or off) by the rule's node terms (gmpnp_amd/polarisation.py), facet by facet as the device forms them: 1D
    one facet per point vertex, 3D the wall facets with eps at the facet mean, w_a = |f| (p_M / 3 - (sum p + p_a) / 12) and the
    facet mass |f| (1 + delta_ab) / 12.  ``want_scale``: also the sums of the absolute values of the terms of dD and of dI_r (what
    the rounding of a sum taken in another order is measured against)."""
    from gmpnp_amd.kinetics import surface_rate
    nf, ns = prob.nf, prob.nf - 1
    dim = prob.coords.shape[1]
    u2d, z2d = np.asarray(u, dtype=np.float64).reshape(-1, nf), np.asarray(z, dtype=np.float64).reshape(-1, nf)
    st = prob.stern
    eps0, epsc = float(prob.model.eps0), np.asarray(prob.model.epsc, dtype=np.float64)[:ns]
    bc = set(int(r) for r in prob.bc_dofs)
    if dim == 1:
        facets, areas = np.asarray(prob.point_vertices, dtype=np.int64).reshape(-1, 1), np.ones(len(prob.point_vertices))
    else:
        facets, areas = np.asarray(prob.wall_facets, dtype=np.int64), SR.facet_areas(prob)
    FN = facets.shape[1]
    pM, lam = float(st.p_electrode), float(st.lam)
    dD, absD = 0.0, 0.0
    for nd, area in zip(facets, areas):
        g, dg = coupled_g(st.model, eps0 + float(epsc @ u2d[nd, :ns].mean(axis=0)), st.eps_surface)
        p = u2d[nd, ns]
        se = [float(epsc @ z2d[b, :ns]) for b in nd]
        for a in range(FN):
            if int(nd[a]) * nf + ns in bc:
                continue
            wa = area * (pM / 3.0 - (p.sum() + p[a]) / 12.0) if dim == 3 else pM - p[0]
            share = area / 3.0 if dim == 3 else 1.0
            terms = [pol.stern_explicit(param, g * share / lam, g * wa / lam)]
            for b in range(FN):
                mass = area * (2.0 if a == b else 1.0) / 12.0 if dim == 3 else 1.0
                terms += [dg * (se[b] / FN) * wa / lam, -g * mass / lam * z2d[nd[b], ns]]
            dD, absD = dD + sum(terms), absD + sum(abs(t) for t in terms)
    nodes, w = K.boundary_weights(prob)
    dp = float((w * z2d[nodes, ns]).sum() / w.sum())
    kin = getattr(prob, "kinetics", None)
    nr = len(kin.reactions) if kin is not None else 0
    dI, absI = np.zeros(nr), np.zeros(nr)
    if kin is not None:
        rx = K.resolved(prob)
        for I, wI in zip(nodes, w):
            for r, (k, al, pe, re, nu) in enumerate(rx):
                rate, d_u, d_p, _ = surface_rate(k, al, pe, kin.p_electrode, u2d[I, ns], re >= 0, u2d[I, re] if re >= 0 else 0.0)
                e = pol.rate_explicit(param, r, rate, d_p, kin.p_electrode - u2d[I, ns] - pe)
                zu = z2d[I, re] if re >= 0 else 0.0
                dI[r] += pol.current_term(wI, d_u if re >= 0 else 0.0, d_p, zu, z2d[I, ns], e)
                absI[r] += abs(wI) * (abs(d_u * zu) + abs(d_p * z2d[I, ns]) + abs(e))
    return (dD, dI, dp, absD, absI) if want_scale else (dD, dI, dp)
