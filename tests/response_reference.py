"""The small-signal frequency response (include/gmpnp.h ``gmpnp_frequency_response``) restated in NumPy over the
kinetics and galvanostat restatements (kinetics_reference.py, galvanostat_reference.py), with the solvers the tests compare
(imported like galvanostat_reference.py; not a conftest).

At a state u and the electrode potential p_M the records of ``prob`` hold, per unit of p_M, with i sigma in the place of inv_dt:
    (K + i sigma M) x = -b      K = J(u) at inv_dt = 0 (Stern and kinetic terms, identity Dirichlet rows)
                                M = the consistent P1 mass |K| (1 + delta_ab) / ((d + 1)(d + 2)) on the species rows that are not Dirichlet
                                b = dF/dp_M (galvanostat_reference.rhs_b)
    C    = dD/dp_M + (dD/du).x      1D: dD/dp_M = g / lam, dD/dp_v = -g / lam, dD/du_{v,j} = g' epsc_j (p_M - p_v) / lam
    dI_r = dI_r/dp_M + (dI_r/du).x  = -alpha_r I_r + sum_I w_I (k_r E_r x_reactant + alpha_r rate_r x_p)
Test infrastructure only (1D)."""
import copy
import dataclasses

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import galvanostat_reference as GR
import hp_reference as H
import kinetics_reference as K
import stern_bc_reference as SR
from gmpnp_amd import impedance as imp
from gmpnp_amd.stern import coupled_g


def with_inv_dt(prob, inv_dt):
    q = copy.copy(prob)
    q.model = dataclasses.replace(prob.model, inv_dt=float(inv_dt))
    return q


def with_potential(prob, p_M):
    """``galvanostat_reference.with_potential`` for problems with or without kinetics."""
    q = copy.copy(prob)
    q.stern = dataclasses.replace(prob.stern, p_electrode=float(p_M))
    if getattr(prob, "kinetics", None) is not None:
        q.kinetics = dataclasses.replace(prob.kinetics, p_electrode=float(p_M))
    return q


def jacobian(prob, u, inv_dt):
    """J(u) at ``inv_dt`` (CSR, identity Dirichlet rows); u_n does not enter J."""
    return K.assemble(with_inv_dt(prob, inv_dt), u, u, want_jacobian=True)[1].tocsr()


def residual(prob, u, inv_dt=0.0):
    return K.assemble(with_inv_dt(prob, inv_dt), u, u, want_jacobian=False)[0]


def mass(prob):
    """M from the mesh (CSR): |K| (1 + delta_ab) / 6 per 1D cell on the species rows, zero on the potential and the Dirichlet rows."""
    assert prob.coords.shape[1] == 1
    nf, ns = prob.nf, prob.nf - 1
    x = prob.coords[:, 0]
    rows, cols, vals = [], [], []
    for a, b in np.asarray(prob.cells, dtype=np.int64):
        vol = abs(x[b] - x[a])
        for i in range(ns):
            for (p, q, w) in ((a, a, 2.0), (a, b, 1.0), (b, a, 1.0), (b, b, 2.0)):
                rows.append(p * nf + i); cols.append(q * nf + i); vals.append(vol * (1.0 / 6.0) * w)
    M = sp.csr_matrix((vals, (rows, cols)), shape=(prob.ndof, prob.ndof)).tolil()
    for r in np.asarray(prob.bc_dofs, dtype=np.int64):
        M.rows[r], M.data[r] = [], []
    return M.tocsr()


def rhs_b(prob, u):
    """b = dF/dp_M; ``galvanostat_reference.rhs_b`` where the kinetics are on, its Stern rows alone where they are off."""
    if getattr(prob, "kinetics", None) is not None:
        return GR.rhs_b(prob, u)
    nf, ns = prob.nf, prob.nf - 1
    u2d = np.asarray(u, dtype=np.float64).reshape(-1, nf)
    st = prob.stern
    eps0, epsc = float(prob.model.eps0), np.asarray(prob.model.epsc, dtype=np.float64)[:ns]
    b = np.zeros(prob.ndof)
    for v in np.asarray(prob.point_vertices, dtype=np.int64):
        g, _ = coupled_g(st.model, eps0 + float(epsc @ u2d[v, :ns]), st.eps_surface)
        b[v * nf + ns] += g / st.lam
    b[prob.bc_dofs] = 0.0
    return b


def displacement_row(prob, u):
    """(dD/dp_M, dD/du (ndof,)) of D = stern_displacement, closed form, g' included; nothing from a Dirichlet potential row."""
    nf, ns = prob.nf, prob.nf - 1
    u2d = np.asarray(u, dtype=np.float64).reshape(-1, nf)
    st = prob.stern
    eps0, epsc = float(prob.model.eps0), np.asarray(prob.model.epsc, dtype=np.float64)[:ns]
    d_p, row = 0.0, np.zeros(prob.ndof)
    bc = set(int(r) for r in prob.bc_dofs)
    for v in np.asarray(prob.point_vertices, dtype=np.int64):
        if v * nf + ns in bc:
            continue
        g, dg = coupled_g(st.model, eps0 + float(epsc @ u2d[v, :ns]), st.eps_surface)
        d_p += g / st.lam
        row[v * nf + ns] += -g / st.lam
        row[v * nf:v * nf + ns] += dg * epsc * (st.p_electrode - u2d[v, ns]) / st.lam
    return d_p, row


def current_rows(prob, u):
    """(dI_r/dp_M (nr,), dI_r/du (nr, ndof)) of the integrated rates, closed form; empty without kinetics."""
    if getattr(prob, "kinetics", None) is None:
        return np.zeros(0), np.zeros((0, prob.ndof))
    nf, ns = prob.nf, prob.nf - 1
    u2d = np.asarray(u, dtype=np.float64).reshape(-1, nf)
    rx = K.resolved(prob)
    d_p, rows = np.zeros(len(rx)), np.zeros((len(rx), prob.ndof))
    nodes, w = K.boundary_weights(prob)
    for I, wI in zip(nodes, w):
        for r, ((k, al, pe, re, nu), (rate, d_u, dpr, _)) in enumerate(zip(rx, K.node_rates(prob, u2d, I))):
            d_p[r] += -wI * dpr                      # d rate / d p_M = -alpha rate
            rows[r, I * nf + ns] += wI * dpr
            if re >= 0:
                rows[r, I * nf + re] += wI * d_u
    return d_p, rows


def functionals(prob, u, x):
    """(C, dI (nr,)) of a solution x (complex, any precision)."""
    dD, rowD = displacement_row(prob, u)
    dI, rowsI = current_rows(prob, u)
    xt = np.asarray(x)
    return dD + rowD.astype(xt.dtype) @ xt, dI + rowsI.astype(xt.dtype) @ xt


def functionals_by_rule(prob, u, x):
    """The same through the rule's node terms (gmpnp_amd/impedance.py: capacitance_term, current_term), as the device forms them."""
    nf, ns = prob.nf, prob.nf - 1
    u2d = np.asarray(u, dtype=np.float64).reshape(-1, nf)
    x2d = np.asarray(x, dtype=np.complex128).reshape(-1, nf)
    st = prob.stern
    eps0, epsc = float(prob.model.eps0), np.asarray(prob.model.epsc, dtype=np.float64)[:ns]
    bc = set(int(r) for r in prob.bc_dofs)
    C = 0j
    for v in np.asarray(prob.point_vertices, dtype=np.int64):
        if v * nf + ns in bc:
            continue
        g, dg = coupled_g(st.model, eps0 + float(epsc @ u2d[v, :ns]), st.eps_surface)
        se_r = se_i = 0.0
        for j in range(ns):      # the kernel's order, one rounding per product and sum
            se_r, se_i = se_r + float(epsc[j]) * float(x2d[v, j].real), se_i + float(epsc[j]) * float(x2d[v, j].imag)
        C += imp.capacitance_term(g, dg, st.lam, st.p_electrode, u2d[v, ns], complex(x2d[v, ns]), complex(se_r, se_i))
    if getattr(prob, "kinetics", None) is None:
        return C, np.zeros(0, dtype=complex)
    rx = K.resolved(prob)
    dI = np.zeros(len(rx), dtype=complex)
    nodes, w = K.boundary_weights(prob)
    for I, wI in zip(nodes, w):
        for r, ((k, al, pe, re, nu), (rate, d_u, dpr, _)) in enumerate(zip(rx, K.node_rates(prob, u2d, I))):
            dI[r] += imp.current_term(wI, d_u if re >= 0 else 0.0, dpr, complex(x2d[I, re]) if re >= 0 else 0j, complex(x2d[I, ns]))
    return C, dI


@dataclasses.dataclass
class System:
    """K, M, b of one linearisation and the real block diagonals the block-Thomas model works on."""
    prob: object
    u: np.ndarray
    K: sp.csr_matrix
    M: sp.csr_matrix
    b: np.ndarray

    def matrix(self, sigma):
        return (self.K + 1j * float(sigma) * self.M).tocsc()


def system(prob, u):
    return System(prob, np.asarray(u, dtype=np.float64), jacobian(prob, u, 0.0), mass(prob), rhs_b(prob, u))


def refined_solve(A, lu, rhs, rounds=3):
    """``galvanostat_reference.refined_solve`` for a complex matrix: residuals formed in np.clongdouble."""
    C = A.tocoo()
    data = C.data.astype(np.clongdouble)
    x = lu.solve(rhs.astype(np.complex128)).astype(np.clongdouble)
    for _ in range(rounds):
        r = rhs.astype(np.clongdouble)
        np.subtract.at(r, C.row, data * x[C.col])
        x = x + lu.solve(np.asarray(r, dtype=np.complex128))
    return x


def block_gauss_jordan(Wr, Wi, nf):
    """The device's Gauss-Jordan on one block, rows kept in place, on separate real and imaginary parts so that every product and sum
    is rounded on its own (the kernel is compiled without fused multiply-add): W = [D' | right-hand sides] (nf, nc).  In step k the
    pivot is the unused row with the largest key, the bit pattern of |re| + |im| with its last three mantissa bits replaced by 7 - row
    (ties go to the lower row); the pivot row is scaled by the reciprocal conj(z) / |z|^2 and taken out of the others.  Returns the
    solution rows (nf, nc - nf) as (re, im)."""
    used = np.zeros(nf, dtype=bool)
    home = np.zeros(nf, dtype=np.int64)
    low = (7 - np.arange(nf)).astype(np.uint64)
    for k in range(nf):
        key = ((np.abs(Wr[:, k]) + np.abs(Wi[:, k])).view(np.uint64) & ~np.uint64(7)) | low
        key[used] = 0
        p = int(np.argmax(key))
        used[p] = True
        home[k] = p
        n2 = Wr[p, k] * Wr[p, k] + Wi[p, k] * Wi[p, k]
        ipr, ipi = Wr[p, k] / n2, -Wi[p, k] / n2
        fr = Wr[:, k] * ipr - Wi[:, k] * ipi
        fi = Wr[:, k] * ipi + Wi[:, k] * ipr
        fr[p] = fi[p] = 0.0
        rr, ri = Wr[p, k + 1:].copy(), Wi[p, k + 1:].copy()
        Wr[:, k + 1:], Wi[:, k + 1:] = (Wr[:, k + 1:] - (fr[:, None] * rr[None, :] - fi[:, None] * ri[None, :]),
                                        Wi[:, k + 1:] - (fr[:, None] * ri[None, :] + fi[:, None] * rr[None, :]))
        Wr[p, k + 1:], Wi[p, k + 1:] = rr * ipr - ri * ipi, rr * ipi + ri * ipr
    return Wr[home, nf:], Wi[home, nf:]


def thomas_model(S, sigma, order=None):
    """The device algorithm in NumPy, operation for operation (k_response_solve): the vertices in the handle's internal order
    (``order[internal] = file vertex``; None: file order), forward block elimination D' = D_j - L_j X_{j-1}[U],
    b' = -b_j - L_j X_{j-1}[b] with the products taken out one column of L_j after the other, X_j = D'^-1 [U_j | b'] by
    ``block_gauss_jordan``, then x_j = X_j[b] - X_j[U] x_{j+1}.  Returns x in file order (complex128)."""
    nf = S.prob.nf
    n = S.prob.coords.shape[0]
    order = np.arange(n) if order is None else np.asarray(order, dtype=np.int64)
    idx = (order[:, None] * nf + np.arange(nf)[None, :]).ravel()
    Kp, Mp = S.K.tocsr()[idx][:, idx], S.M.tocsr()[idx][:, idx]
    L, D, U = H.tri_blocks(Kp, nf)
    mL, mD, mU = (float(sigma) * a for a in H.tri_blocks(Mp, nf))
    b = S.b[idx].reshape(n, nf)
    Xr, Xi = np.zeros((n, nf, nf + 1)), np.zeros((n, nf, nf + 1))
    pr, pi = np.zeros((nf, nf + 1)), np.zeros((nf, nf + 1))
    cols = list(range(nf)) + [2 * nf]
    for j in range(n):
        Wr = np.concatenate([D[j], U[j], -b[j][:, None]], axis=1)
        Wi = np.concatenate([mD[j], mU[j], np.zeros((nf, 1))], axis=1)
        for m in range(nf):
            lr, li = L[j][:, m][:, None], mL[j][:, m][:, None]
            xr, xi = pr[m][None, :], pi[m][None, :]
            Wr[:, cols], Wi[:, cols] = Wr[:, cols] - (lr * xr - li * xi), Wi[:, cols] - (lr * xi + li * xr)
        pr, pi = block_gauss_jordan(Wr, Wi, nf)
        Xr[j], Xi[j] = pr, pi
    xr, xi = np.zeros((n, nf)), np.zeros((n, nf))
    xr[n - 1], xi[n - 1] = Xr[n - 1][:, nf], Xi[n - 1][:, nf]
    for j in range(n - 2, -1, -1):
        ar, ai = Xr[j][:, nf].copy(), Xi[j][:, nf].copy()
        for m in range(nf):
            ur, ui = Xr[j][:, m], Xi[j][:, m]
            ar, ai = ar - (ur * xr[j + 1, m] - ui * xi[j + 1, m]), ai - (ur * xi[j + 1, m] + ui * xr[j + 1, m])
        xr[j], xi[j] = ar, ai
    x = np.zeros(n * nf, dtype=np.complex128)
    x[idx] = (xr + 1j * xi).ravel()
    return x


def relative_residual(S, sigma, x):
    """max |(K + i sigma M) x + b| / max |b|, the terms formed in extended precision."""
    A = S.matrix(sigma).tocoo()
    r = S.b.astype(np.clongdouble)
    np.add.at(r, A.row, A.data.astype(np.clongdouble) * np.asarray(x).astype(np.clongdouble)[A.col])
    return float(np.abs(r).max() / np.abs(S.b).max())


def solve(S, sigma, how="refined", order=None):
    """x of one frequency: "refined" (splu + extended-precision refinement, np.clongdouble), "splu" (plain complex128) or "thomas"
    (the model of the device algorithm, its functionals by the rule's node terms; ``order``: the handle's vertex order)."""
    if how == "thomas":
        return thomas_model(S, float(sigma), order)
    A = S.matrix(sigma)
    lu = spla.splu(A)
    if how == "splu":
        return lu.solve(-S.b.astype(np.complex128))
    return refined_solve(A, lu, -S.b)


def response(S, sigma, how="refined", order=None):
    """(x, C, dI) of one frequency; the model's functionals are formed as the device forms them (``functionals_by_rule``)."""
    x = solve(S, sigma, how, order)
    C, dI = functionals_by_rule(S.prob, S.u, x) if how == "thomas" else functionals(S.prob, S.u, x)
    return x, C, dI


def steady_state(prob, u0, iterations=30, tol=1e-9):
    """Newton at inv_dt = 0 from u0 with sparse LU (the operating point of the zero-frequency tests); returns (u, iterations)."""
    u = np.array(u0, dtype=np.float64, copy=True)
    q = with_inv_dt(prob, 0.0)
    r0 = None
    for it in range(iterations):
        F, A = K.assemble(q, u, u, want_jacobian=True)
        r = float(np.linalg.norm(F))
        r0 = r if r0 is None else r0
        if r <= tol * max(r0, 1.0):
            return u, it
        u -= spla.splu(A.tocsc()).solve(F)
    raise RuntimeError("steady state: Newton did not converge")


def high_frequency_closed_form(prob, u):
    """1 / (lam / g + sum_e h_e / eps_e), scaled (gmpnp_amd/impedance.py)."""
    return imp.high_frequency_capacitance(prob.coords, np.asarray(u).reshape(-1, prob.nf), prob.model, prob.stern)
