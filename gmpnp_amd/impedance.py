"""Impedance spectroscopy of the 1D double layer (``--impedance`` of the 1D MPNP driver,
``gmpnp_frequency_response``): the Python statement of the small-signal rule, the frequency grid, the conversion between a
frequency in Hz and the library's time-term multiplier sigma, and the physical spectrum built from the library's scaled response.

At the state u and the electrode potential p_M of a handle, per unit of p_M (thermal voltages) and with i sigma in the place of
``model.inv_dt``:

    (K + i sigma M) x = -b          K = J(u) at inv_dt = 0,  M = the consistent P1 mass of the free species rows,  b = dF/dp_M
    C(sigma)    = dD/dp_M + (dD/du).x         D the integrated Stern term (``stern_displacement``)
    dI_r(sigma) = dI_r/dp_M + (dI_r/du).x     I_r the integrated rates (``kinetics_currents``)

The driver's ``model.inv_dt`` is ``1 / (h L_D)`` with the step h in units of ``time_constant``, so a harmonic perturbation of
frequency f [Hz] has sigma = 2 pi f time_constant / L_D.  With C_phys = eps_0 / L_n C [F/m2] and dI_r/dV = dI_r / thermal_voltage
[S/m2] (the OHP is one point: the area is 1) the admittance of the interface per area is

    Y = i omega C_phys - sum_r dI_r/dV          Z = 1 / Y

(cathodic currents are positive in this code, so the charge-transfer conductance -dI/dV comes out positive).  No reference counterpart.
"""
from __future__ import annotations

import math

import numpy as np

MAX_FREQUENCIES = 4096                       # gmpnp_frequency_response: n in 1 ... 4096
STATUS_SINGULAR, STATUS_NONFINITE = 256, 512  # bits of gmpnp_response_t.status
IMPEDANCE_KEYWORDS = ("impedance",)


# ---- the rule (gmpnp_host_rules.h), operation for operation ---------------------------------------------------------------------
def pivot_key(z):
    """|re| + |im|: what the pivot search of the complex block elimination compares (``response_pivot_key``)."""
    return abs(z.real) + abs(z.imag)


def capacitance_term(g, dg, lam, p_M, p, x_p, s):
    """A Stern node's share of C (``response_capacitance_term``): g / lam (1 - x_p) + g' (p_M - p) / lam s with s = sum_j epsc_j x_j."""
    a = np.float64(g) / np.float64(lam)
    c = np.float64(dg) * (np.float64(p_M) - np.float64(p)) / np.float64(lam)
    return complex(a * (1.0 - x_p.real) + c * s.real, c * s.imag - a * x_p.imag)


def current_term(w, d_u, d_p, x_u, x_p):
    """Reaction r's share of dI_r at a kinetic node of weight w (``response_current_term``): w (d_u x_u + d_p (x_p - 1))."""
    w, d_u, d_p = np.float64(w), np.float64(d_u), np.float64(d_p)
    return complex(w * (d_u * x_u.real + d_p * (x_p.real - 1.0)), w * (d_u * x_u.imag + d_p * x_p.imag))


def sigma_valid(sigma):
    return bool(sigma >= 0.0 and math.isfinite(sigma))


def count_valid(n):
    return 1 <= int(n) <= MAX_FREQUENCIES


def bytes_per_frequency(nv):
    """Workspace one frequency takes on nv vertices (``response_bytes_per_frequency``)."""
    return float(nv) * (8.0 * 8.0 + 8.0) * 16.0


def chunk(n, nv, cap_bytes):
    """Frequencies per chunk under a memory cap (``response_chunk``): at least one, at most n, whole 8-frequency waves where that fits."""
    k = math.floor(cap_bytes / bytes_per_frequency(nv)) if math.isfinite(cap_bytes) else float("inf")
    if not k >= 1.0:
        k = 1.0
    c = n if k >= n else int(k)
    if c < n and c >= 8:
        c -= c % 8
    return c


# ---- frequencies and units ---------------------------------------------------------------------------------------------------------
def frequency_grid(freq_min=1e-2, freq_max=1e8, per_decade=10):
    """Logarithmic grid [Hz] from ``freq_min`` to ``freq_max``, both included, ``per_decade`` points per decade."""
    if not (freq_min > 0.0 and freq_max >= freq_min and math.isfinite(freq_max)) or int(per_decade) < 1:
        raise ValueError("impedance: the frequency grid needs 0 < freq_min <= freq_max and freq_per_decade >= 1")
    n = int(round((math.log10(freq_max) - math.log10(freq_min)) * int(per_decade))) + 1
    if not count_valid(n):
        raise ValueError("impedance: the frequency grid has %d points (1 ... %d)" % (n, MAX_FREQUENCIES))
    return freq_min * (freq_max / freq_min) ** (np.arange(n) / max(n - 1, 1)) if n > 1 else np.array([float(freq_min)])


def sigma_from_frequency(ep, frequency):
    """sigma of a harmonic perturbation of ``frequency`` [Hz] on the 1D driver's scaling: 2 pi f time_constant / L_D, the factor
    between 1 / (physical step) and ``model.inv_dt`` = 1 / (h L_D), h = step / time_constant."""
    return 2.0 * math.pi * np.asarray(frequency, dtype=np.float64) * ep.time_constant / ep.L_D


def spectrum(ep, eps_0, frequency, response):
    """The physical spectrum of one ``DeviceSolver.frequency_response`` result at the frequencies [Hz] it was computed for:
    capacitance [F/m2] (complex), dI_dV (n, n_reactions) [S/m2], admittance [S/m2], impedance [Ohm m2]."""
    f = np.asarray(frequency, dtype=np.float64)
    cap = eps_0 / ep.L_n * np.asarray(response["C"])
    dI = np.asarray(response["dI"]).reshape(len(f), -1) / ep.thermal_voltage
    Y = 1j * 2.0 * math.pi * f * cap - dI.sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        Z = 1.0 / Y
    return {"frequency": f, "sigma": np.asarray(response["sigma"]), "capacitance": cap, "dI_dV": dI, "admittance": Y, "impedance": Z,
            "residual": np.asarray(response["residual"]), "status": np.asarray(response["status"])}


def high_frequency_capacitance(coords, u2d, model, stern):
    """The closed form of C at sigma -> infinity, scaled units: the concentrations cannot follow, and what is left is the Stern
    capacitor in series with the element capacitors between the OHP and the vertex that holds the potential,
    1 / (lam / g + sum_e h_e / eps_e), eps_e the element mean of eps(u) (the 1D mesh in path order, OHP first)."""
    from .stern import coupled_g
    ns = u2d.shape[1] - 1
    epsc = np.asarray(model.epsc, dtype=np.float64)[:ns]
    eps = float(model.eps0) + u2d[:, :ns] @ epsc
    x = np.asarray(coords, dtype=np.float64).reshape(-1)
    order = np.argsort(x)
    h = np.diff(x[order])
    eps_e = 0.5 * (eps[order][:-1] + eps[order][1:])
    g, _ = coupled_g(stern.model, float(eps[order][0]), stern.eps_surface)
    return 1.0 / (stern.lam / g + float(np.sum(h / eps_e)))


# ---- the 3D pore (gmpnp_frequency_response_3d) ----------------------------------------------------------------------
def facet_term(g, dg, lam, w_a, m_ab, se_fn, x_p):
    """One facet's share of (Stern row of J).x towards its node a from its node b (``response_facet_term``), applied to the real and
    to the imaginary part of x: g' se_fn w_a / lam - g m_ab / lam x_p, se_fn = sum_j epsc_j x_{b,j} / 3."""
    g, dg, lam = np.float64(g), np.float64(dg), np.float64(lam)
    return float(dg * np.float64(se_fn) * np.float64(w_a) / lam - g * np.float64(m_ab) / lam * np.float64(x_p))


def band_bytes_per_frequency(n_blocks, band, nf=9):
    """Bytes of complex band one frequency takes (``response_band_bytes_per_frequency``): n (2 b + 1) blocks of nf x nf pairs."""
    return float(n_blocks) * (2.0 * band + 1.0) * nf * nf * 16.0


def band_chunk(n, n_blocks, band, nf, cap_bytes):
    """Frequencies per chunk under the band LU's memory cap (``response_band_chunk``): at least one, at most n."""
    k = math.floor(cap_bytes / band_bytes_per_frequency(n_blocks, band, nf)) if math.isfinite(cap_bytes) else float("inf")
    if not k >= 1.0:
        k = 1.0
    return n if k >= n else int(k)


def block_inverse(A):
    """(inverse, pivot rows, bad) of one complex block by the rule's Gauss-Jordan (``response_block_inverse``): column k's pivot is the
    row r >= k with the largest |re| + |im|, ties to the lower row, and changes places with row k."""
    A = np.asarray(A, dtype=np.complex128)
    n = A.shape[0]
    row = np.concatenate([A, np.eye(n, dtype=np.complex128)], axis=1)
    piv, bad = [], False
    for k in range(n):
        idx, v = k, pivot_key(row[k, k])
        for r in range(k + 1, n):
            o = pivot_key(row[r, k])
            if o > v:
                idx, v = r, o
        bad = bad or not v > 0.0
        piv.append(idx)
        with np.errstate(all="ignore"):
            ip = 1.0 / row[idx, k]
            pr, old = row[idx].copy(), row[k].copy()
            for r in range(n):
                mine = old if r == idx else row[r].copy()
                row[r] = pr * ip if r == k else mine - (mine[k] * ip) * pr
                row[r, k] = 1.0 if r == k else 0.0
    return row[:, n:], piv, bad


def pore_sigma_from_frequency(pp, frequency):
    """sigma of a harmonic perturbation of ``frequency`` [Hz] on the pore driver's scaling: ``PoreParameters`` builds
    ``model.inv_dt`` = 1 / dt with dt = time_step / time_constant, so sigma = 2 pi f time_constant."""
    return 2.0 * math.pi * np.asarray(frequency, dtype=np.float64) * pp.time_constant


def pore_spectrum(pp, eps_0, wall_area, frequency, response):
    """The physical spectrum of one ``DeviceSolver.frequency_response_3d`` result, per wall area: the library's C and dI are sums over
    the wall, ``wall_area`` = sum_I w_I (scaled) makes them wall means as the polarisation curve reports its currents and capacitance.
    capacitance = eps_0 / L C / area [F/m2], dI_dV = dI / area / thermal_voltage [S/m2], Y = i omega C - sum_r dI_r/dV, Z = 1 / Y."""
    f = np.asarray(frequency, dtype=np.float64)
    cap = eps_0 / pp.L * np.asarray(response["C"]) / wall_area
    dI = np.asarray(response["dI"]).reshape(len(f), -1) / wall_area / pp.thermal_voltage
    Y = 1j * 2.0 * math.pi * f * cap - dI.sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        Z = 1.0 / Y
    return {"frequency": f, "sigma": np.asarray(response["sigma"]), "capacitance": cap, "dI_dV": dI, "admittance": Y, "impedance": Z,
            "residual": np.asarray(response["residual"]), "status": np.asarray(response["status"])}


def potential_block_capacitance(K, b, potential_rows, functional):
    """The high-frequency reference of C, scaled units: with the concentrations frozen (sigma -> infinity) x keeps its potential
    entries alone, and they solve the potential block of K: K_pp x_p = -b_p.  ``K`` a SciPy sparse matrix, ``potential_rows`` the
    potential dofs (Dirichlet identity rows included), ``functional(x)`` the real functional C of a real x (explicit part included)."""
    import scipy.sparse.linalg as spla
    rows = np.asarray(potential_rows, dtype=np.int64)
    Kpp = K.tocsr()[rows][:, rows].tocsc()
    x = np.zeros(K.shape[0])
    x[rows] = spla.splu(Kpp).solve(-np.asarray(b, dtype=np.float64)[rows])
    return functional(x), x


def pore_stern_terms(coords, wall_facets, model, stern, bc_dofs, u2d, x2d=None):
    """(C, b) facet by facet over the wall (the Python statement of the Stern part of ``k_cband_functional`` and of
    ``k_response_rhs<3, 9>``): C = dD/dp_M + (dD/du).x of the complex (or real) x, the explicit part g |f| / (3 lam) per free wall node
    of a facet in the real part alone, and b = the Stern rows of dF/dp_M (ndof,).  ``x2d`` None: x = 0 (C = dD/dp_M).  g and g' at
    the facet mean of eps(u), w_a = |f| (p_M / 3 - (sum p + p_a) / 12), the facet mass |f| (1 + delta_ab) / 12."""
    from .stern import coupled_g
    u2d = np.asarray(u2d, dtype=np.float64)
    nf, ns = u2d.shape[1], u2d.shape[1] - 1
    x2d = np.zeros(u2d.shape, dtype=np.complex128) if x2d is None else np.asarray(x2d, dtype=np.complex128).reshape(u2d.shape)
    eps0, epsc = float(model.eps0), np.asarray(model.epsc, dtype=np.float64)[:ns]
    bc = set(int(r) for r in bc_dofs)
    X = np.asarray(coords, dtype=np.float64)[np.asarray(wall_facets, dtype=np.int64)]
    areas = 0.5 * np.linalg.norm(np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]), axis=1)
    pM, lam = float(stern.p_electrode), float(stern.lam)
    C, b = 0j, np.zeros(u2d.size)
    for nd, area in zip(np.asarray(wall_facets, dtype=np.int64), areas):
        g, dg = coupled_g(stern.model, eps0 + float(epsc @ u2d[nd, :ns].mean(axis=0)), stern.eps_surface)
        p = u2d[nd, ns]
        se = [complex(epsc @ x2d[q, :ns].real, epsc @ x2d[q, :ns].imag) / 3.0 for q in nd]
        for a in range(3):
            if int(nd[a]) * nf + ns in bc:
                continue
            wa = area * (pM / 3.0 - (p.sum() + p[a]) / 12.0)
            b[int(nd[a]) * nf + ns] += g * (area / 3.0) / lam
            re, im = g * (area / 3.0) / lam, 0.0
            for q in range(3):
                mab = area * (2.0 if a == q else 1.0) / 12.0
                re += facet_term(g, dg, lam, wa, mab, se[q].real, x2d[nd[q], ns].real)
                im += facet_term(g, dg, lam, wa, mab, se[q].imag, x2d[nd[q], ns].imag)
            C += complex(re, im)
    return C, b


def add_pore_impedance_arguments(p):
    p.add_argument("--pore_impedance", action="store_true",
                   help="(addition) impedance spectrum of the pore at the last state (pore_impedance.npz); needs --electrode_voltage")
    p.add_argument("--freq_min", required=False, default=1e-2, type=float, help="(addition) lowest frequency of --pore_impedance [Hz]")
    p.add_argument("--freq_max", required=False, default=1e8, type=float, help="(addition) highest frequency of --pore_impedance [Hz]")
    p.add_argument("--freq_per_decade", required=False, default=10, type=int, help="(addition) points per decade of --pore_impedance")


def pore_impedance_keywords(a):
    """The keyword of a parsed command line (``add_pore_impedance_arguments``); empty without --pore_impedance."""
    if not a.pore_impedance:
        return {}
    return {"pore_impedance": dict(freq_min=a.freq_min, freq_max=a.freq_max, per_decade=a.freq_per_decade)}


def refuse_pore_impedance(kwargs, what, hint=""):
    """ValueError where ``kwargs`` asks for the pore's impedance spectrum (``pore_impedance``) in a driver that has none."""
    if kwargs.get("pore_impedance"):
        raise ValueError("pore_impedance: the 3D frequency response is not available in %s%s" % (what, hint))


# ---- keywords of the drivers -----------------------------------------------------------------------------------------------------
def add_impedance_arguments(p):
    p.add_argument("--impedance", action="store_true",
                   help="(addition) impedance spectrum of the interface at the last state (impedance.npz); needs --electrode_voltage")
    p.add_argument("--freq_min", required=False, default=1e-2, type=float, help="(addition) lowest frequency of --impedance [Hz]")
    p.add_argument("--freq_max", required=False, default=1e8, type=float, help="(addition) highest frequency of --impedance [Hz]")
    p.add_argument("--freq_per_decade", required=False, default=10, type=int, help="(addition) points per decade of --impedance")


def impedance_keywords(a):
    """The impedance keyword of a parsed command line (``add_impedance_arguments``); empty without --impedance."""
    if not a.impedance:
        return {}
    return {"impedance": dict(freq_min=a.freq_min, freq_max=a.freq_max, per_decade=a.freq_per_decade)}


def refuse_impedance(kwargs, what):
    """ValueError where ``kwargs`` asks for an impedance spectrum (``impedance``) in a driver that has none."""
    if kwargs.get("impedance"):
        raise ValueError("impedance: the frequency response is not available in %s" % what)
