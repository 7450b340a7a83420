"""Discrete problem description handed to a backend: mesh arrays, model tables,
boundary facet sets and the merged Dirichlet table, all in FILE vertex order with
``dof = vertex * n_fields + field`` (the node-interleaved layout of the reference's MixedElement,
3D/MPNP_CO2ER_pore.py:404-408, 1D/MPNP_CO2ER_EDL.py:300-304).

``pore_problem`` / ``edl_problem`` restate how the reference turns markers into boundary conditions
(3D:335-382,460-467; 1D:237-254,350-355).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from .mesh import Mesh, mark_pore_boundaries, pore_wall_tolerance
from .model import Model, Quadrature, default_quadrature


L_STERN_DEFAULT = 4.0e-10  # [m] stern.py: L_STERN
EPS_SURFACE_DEFAULT = 6.0


@dataclass
class SternLayer:
    """Stern-layer boundary condition of the potential (include/gmpnp.h): on the Stern boundary (1D:
    ``Problem.point_vertices``, 3D: ``Problem.wall_facets``) the potential's Dirichlet value is dropped and the row gains
    ``int g(eps) (p_M - p) / lam v ds``.  ``model``: "linear" (g = eps) or "BDM" (g = (eps - eps_s) / ln(eps / eps_s))."""
    model: str  # "linear" | "BDM"
    p_electrode: float  # p_M [thermal voltages]
    lam: float  # Stern length / length scale of the mesh
    eps_surface: float = EPS_SURFACE_DEFAULT

    def __post_init__(self):
        if self.model not in ("linear", "BDM"):
            raise ValueError("Stern model must be 'linear' or 'BDM', not %r" % (self.model,))
        if not (self.lam > 0.0 and np.isfinite(self.lam) and np.isfinite(self.p_electrode)):
            raise ValueError("Stern layer: lam > 0 and a finite electrode potential")
        if not (self.eps_surface > 0.0 and np.isfinite(self.eps_surface)):
            raise ValueError("Stern layer: eps_surface > 0")


STERN_KEYWORDS = ("electrode_voltage", "stern_model", "stern_length", "stern_eps_surface")


def pop_stern(kwargs, length_scale):
    """Takes the Stern keywords of a driver (``electrode_voltage`` [thermal voltages], ``stern_model`` = "BDM", ``stern_length`` =
    4e-10 m, ``stern_eps_surface`` = 6) out of ``kwargs``; returns the ``SternLayer`` with lam = stern_length / length_scale, or None
    without an electrode voltage.  ``electrode_voltage`` takes the place of ``voltage_multiplier``: giving both is a ValueError."""
    if "voltage_multiplier" in kwargs and kwargs["voltage_multiplier"] is None:   # a keyword surface's "not given"
        kwargs.pop("voltage_multiplier")
    v = kwargs.pop("electrode_voltage", None)
    model = kwargs.pop("stern_model", "BDM")
    length = kwargs.pop("stern_length", L_STERN_DEFAULT)
    eps_s = kwargs.pop("stern_eps_surface", EPS_SURFACE_DEFAULT)
    if v is None:
        return None
    if "voltage_multiplier" in kwargs:
        raise ValueError("electrode_voltage takes the place of voltage_multiplier: give one of them")
    return SternLayer(model=model, p_electrode=float(v), lam=float(length) / float(length_scale), eps_surface=float(eps_s))


def refuse_stern(kwargs, what):
    """ValueError if a keyword dict asks for the Stern boundary condition where it does not exist (before anything touches the device)."""
    if kwargs.get("electrode_voltage") is not None:
        raise ValueError("electrode_voltage: the Stern boundary condition is not available in %s" % what)


def add_stern_arguments(p):
    """The drivers' command-line flags of the Stern boundary condition (additions, not reference flags)."""
    p.add_argument("--electrode_voltage", required=False, default=None, type=float,
                   help="(addition) electrode potential in thermal voltages, applied through a Stern layer; takes the place of --voltage_multiplier")
    p.add_argument("--stern_model", required=False, default="BDM", type=str, choices=("linear", "BDM"), help="(addition) Stern-layer model")
    p.add_argument("--stern_length", required=False, default=L_STERN_DEFAULT, type=float, help="(addition) Stern-layer thickness [m]")
    p.add_argument("--stern_eps_surface", required=False, default=EPS_SURFACE_DEFAULT, type=float, help="(addition) relative permittivity at the surface (BDM)")


def stern_keywords(a):
    """The Stern keywords of a parsed command line (``add_stern_arguments``)."""
    return {k: getattr(a, k) for k in STERN_KEYWORDS}


MAX_SURFACE_REACTIONS = 4  # GMPNP_MAX_SURFACE_REACTIONS (include/gmpnp.h)


@dataclass
class SurfaceReaction:
    """One reaction of ``SurfaceKinetics``: rate = k (u_reactant or 1) exp(-alpha (p_M - p - p_eq)); ``nu``: species name -> flux weight."""
    k: float
    alpha: float = 0.5
    p_eq: float = 0.0  # [thermal voltages]
    reactant: str = None  # species name, None = no reactant
    nu: dict = field(default_factory=dict)


@dataclass
class SurfaceKinetics:
    """Potential-dependent surface kinetics on the Stern boundary (include/gmpnp.h ``gmpnp_kinetics_t`` with the
    species by name): the species rows of the boundary nodes gain ``w_I sum_r nu[r][i] rate_r``.  ``p_electrode``: the kinetics' own p_M."""
    reactions: list
    p_electrode: float

    def __post_init__(self):
        self.reactions = list(self.reactions)
        if not 1 <= len(self.reactions) <= MAX_SURFACE_REACTIONS:
            raise ValueError("surface kinetics: 1 ... %d reactions, not %d" % (MAX_SURFACE_REACTIONS, len(self.reactions)))
        vals = [self.p_electrode] + [v for r in self.reactions for v in (r.k, r.alpha, r.p_eq, *r.nu.values())]
        if not np.isfinite(np.asarray(vals, dtype=np.float64)).all():
            raise ValueError("surface kinetics: k, alpha, p_eq, nu and the electrode potential must be finite")

    def check_species(self, species):
        """ValueError where a reactant or a flux weight names a species the model does not have."""
        for r in self.reactions:
            for name in ([] if r.reactant is None else [r.reactant]) + list(r.nu):
                if name not in species:
                    raise ValueError("surface kinetics: no species %r in the model (%s)" % (name, ", ".join(species)))


KINETICS_KEYWORDS = ("kinetics", "i0_CO", "i0_H2", "alpha_CO", "alpha_H2", "p_eq_CO", "p_eq_H2")


def pop_kinetics(kwargs):
    """Takes the kinetics keywords of a driver (``kinetics`` = "tafel", ``i0_CO`` / ``i0_H2`` [A/m2], ``alpha_CO`` / ``alpha_H2`` = 0.5,
    ``p_eq_CO`` / ``p_eq_H2`` = 0 thermal voltages) out of ``kwargs``; returns them as a dict, or None without ``kinetics``."""
    kind = kwargs.pop("kinetics", None)
    par = {k: kwargs.pop(k, None) for k in KINETICS_KEYWORDS[1:]}
    if kind is None:
        return None
    if kind != "tafel":
        raise ValueError("kinetics must be 'tafel', not %r" % (kind,))
    if par["i0_CO"] is None or par["i0_H2"] is None:
        raise ValueError("kinetics tafel: i0_CO and i0_H2 [A/m2] are required")
    for k, default in (("alpha_CO", 0.5), ("alpha_H2", 0.5), ("p_eq_CO", 0.0), ("p_eq_H2", 0.0)):
        par[k] = default if par[k] is None else par[k]
    par = {k: float(v) for k, v in par.items()}
    if not all(np.isfinite(v) for v in par.values()):
        raise ValueError("kinetics tafel: the parameters must be finite")
    return par


def refuse_kinetics(kwargs, what):
    """ValueError if a keyword dict asks for the surface kinetics where they do not exist (before anything touches the device)."""
    if kwargs.get("kinetics") is not None:
        raise ValueError("kinetics: the potential-dependent surface kinetics are not available in %s" % what)


def add_kinetics_arguments(p):
    """The drivers' command-line flags of the surface kinetics (additions, not reference flags)."""
    p.add_argument("--kinetics", required=False, default=None, type=str, choices=("tafel",),
                   help="(addition) potential-dependent Tafel currents at the OHP in place of the prescribed current; needs --electrode_voltage")
    p.add_argument("--i0_CO", required=False, default=None, type=float, help="(addition) rate constant of CO2 -> CO [A/m2], required with --kinetics")
    p.add_argument("--i0_H2", required=False, default=None, type=float, help="(addition) rate constant of the hydrogen evolution [A/m2], required with --kinetics")
    p.add_argument("--alpha_CO", required=False, default=0.5, type=float, help="(addition) transfer coefficient of CO2 -> CO")
    p.add_argument("--alpha_H2", required=False, default=0.5, type=float, help="(addition) transfer coefficient of the hydrogen evolution")
    p.add_argument("--p_eq_CO", required=False, default=0.0, type=float, help="(addition) equilibrium offset of CO2 -> CO [thermal voltages]")
    p.add_argument("--p_eq_H2", required=False, default=0.0, type=float, help="(addition) equilibrium offset of the hydrogen evolution [thermal voltages]")


def kinetics_keywords(a):
    """The kinetics keywords of a parsed command line (``add_kinetics_arguments``); empty without --kinetics."""
    if a.kinetics is None:
        return {}
    return {k: getattr(a, k) for k in KINETICS_KEYWORDS}


@dataclass
class Galvanostat:
    """Galvanostatic mode (include/gmpnp.h ``gmpnp_galvanostat_t``): the electrode potential is an unknown and
    ``sum_r weights[r] sum_I w_I rate_r = target`` the extra equation.  ``target`` is in the units of the integrated rates."""
    target: float
    weights: tuple = (1.0, 1.0)

    def __post_init__(self):
        self.weights = tuple(float(w) for w in self.weights)
        if not (np.isfinite(self.target) and self.target > 0.0):
            raise ValueError("galvanostat: the target current must be positive and finite, not %r" % (self.target,))
        if not 1 <= len(self.weights) <= MAX_SURFACE_REACTIONS or not np.isfinite(self.weights).all() or not any(self.weights):
            raise ValueError("galvanostat: 1 ... %d finite weights, not all zero" % MAX_SURFACE_REACTIONS)


GALVANOSTAT_KEYWORDS = ("target_current",)


def pop_galvanostat(kwargs):
    """Takes ``target_current`` [A/m2, the area mean of i_CO + i_H2] of a driver out of ``kwargs``; returns it as a float, or None."""
    x = kwargs.pop("target_current", None)
    if x is None:
        return None
    x = float(x)
    if not (np.isfinite(x) and x > 0.0):
        raise ValueError("target_current: the galvanostat's target must be positive and finite, not %r" % (x,))
    return x


def refuse_galvanostat(kwargs, what):
    """ValueError if a keyword dict asks for the galvanostat where it does not exist (before anything touches the device)."""
    if kwargs.get("target_current") is not None:
        raise ValueError("target_current: the galvanostat is not available in %s" % what)


def add_galvanostat_arguments(p):
    """The drivers' command-line flag of the galvanostatic mode (an addition, not a reference flag)."""
    p.add_argument("--target_current", required=False, default=None, type=float,
                   help="(addition) total current density i_CO + i_H2 [A/m2] to hold: the electrode potential is solved for, "
                        "--electrode_voltage is its starting guess; needs --kinetics tafel")


def galvanostat_keywords(a):
    """The galvanostat keyword of a parsed command line (``add_galvanostat_arguments``); empty without --target_current."""
    if a.target_current is None:
        return {}
    return {"target_current": a.target_current}


@dataclass
class Problem:
    coords: np.ndarray  # (nv,d)
    cells: np.ndarray  # (nc,d+1)
    model: Model
    quad: Quadrature = None
    wall_facets: np.ndarray = None  # (nw,3) ds(2) facets (3D)
    exit_facets: np.ndarray = None  # (ne,3) ds(3) facets (3D)
    point_vertices: np.ndarray = None  # 1D: vertices carrying the point fluxes (the OHP vertex)
    bc_dofs: np.ndarray = None  # Dirichlet dofs (unique, sorted; the last DirichletBC in the list wins)
    bc_vals: np.ndarray = None
    # SUPG stabilisation of the PNP model (reference 1D:597-722): nodal rho_i (nv, ns), zero where a species is not
    # stabilised, and the species whose gradient enters species i's strong residual (identity except the reference's
    # OH term, which takes grad(u_H): SURVEY Q7).  None = no stabilisation.
    supg_rho: np.ndarray = None
    supg_w: np.ndarray = None
    stern: SternLayer = None  # Stern-layer boundary condition of the potential; None = the potential is prescribed (Dirichlet)
    kinetics: SurfaceKinetics = None  # potential-dependent surface kinetics on the Stern boundary; None = the constant fluxes alone
    galvanostat: Galvanostat = None  # the electrode potential as an unknown at a set total current (needs kinetics); None = potentiostatic

    def __post_init__(self):
        d = self.coords.shape[1]
        if self.quad is None:
            self.quad = default_quadrature(d)
        e3 = np.zeros((0, 3), dtype=np.int32)
        if self.wall_facets is None:
            self.wall_facets = e3
        if self.exit_facets is None:
            self.exit_facets = e3
        if self.point_vertices is None:
            self.point_vertices = np.zeros(0, dtype=np.int32)
        if self.bc_dofs is None:
            self.bc_dofs, self.bc_vals = np.zeros(0, dtype=np.int64), np.zeros(0)

    @property
    def nf(self) -> int:
        return self.model.n_fields

    @property
    def ndof(self) -> int:
        return self.coords.shape[0] * self.nf


def merge_dirichlet(bcs, nf):
    """``bcs``: list of (vertices, field, value) in the reference's list order (3D:467, 1D:355).
    DOLFIN applies them in order, so on a shared dof the LAST one wins."""
    dof_parts, val_parts = [], []
    for verts, fld, val in bcs:
        d = np.asarray(verts, dtype=np.int64).ravel() * nf + int(fld)
        dof_parts.append(d)
        val_parts.append(np.full(d.shape, float(val)))
    if not dof_parts:
        return np.zeros(0, dtype=np.int64), np.zeros(0)
    dofs, vals = np.concatenate(dof_parts), np.concatenate(val_parts)
    # keep the last occurrence of each dof
    rev_dofs, rev_vals = dofs[::-1], vals[::-1]
    uniq, first = np.unique(rev_dofs, return_index=True)
    return uniq, rev_vals[first]


def pore_dirichlet(pp, bnd, co2_value=None, stern=False):
    """bcs = [bc1..bc6] of reference 3D:460-467 (bc4 rebuilt every step, 3D:835-838).  ``stern``: the wall potential is not
    prescribed (the (s2, ns, voltage) entry is dropped; wall vertices shared with S1 / S3 keep p = 0)."""
    ns = len(pp.species)
    co2 = pp.eq_conc_CO2_scaled if co2_value is None else co2_value
    s1, s2, s3 = bnd.dirichlet_vertices[1], bnd.dirichlet_vertices[2], bnd.dirichlet_vertices[3]
    # Only the CO2 value changes between time steps: the merged dof set and the positions of the bc4 entries in it are
    # kept on the boundary record (keyed by everything else that enters), so the per-step rebuild is one fill.
    key = (ns, float(pp.voltage_scaled), float(pp.eq_conc_CO_scaled), float(pp.eq_conc_H2_scaled), bool(stern))
    cache = getattr(bnd, "_dirichlet_cache", None)
    if cache is None or cache[0] != key:
        bcs = [(s1, ns, 0.0), (s3, ns, 0.0)] + ([] if stern else [(s2, ns, pp.voltage_scaled)]) + [
               (s1, 4, co2), (s1, 5, pp.eq_conc_CO_scaled), (s1, 6, pp.eq_conc_H2_scaled)]
        dofs, vals = merge_dirichlet(bcs, ns + 1)
        # field 4 appears in bc4 only, so "later bc wins" never touches these entries
        idx = np.searchsorted(dofs, np.asarray(s1, dtype=np.int64).ravel() * (ns + 1) + 4)
        cache = (key, dofs, vals, idx)
        try:
            bnd._dirichlet_cache = cache
        except AttributeError:  # a record type without room for it: no caching
            return dofs, vals
    _, dofs, vals, idx = cache
    vals = vals.copy()
    vals[idx] = co2
    return dofs, vals


def pore_problem(pp, mesh: Mesh, quad: Quadrature = None, refine: int = 0, stern: SternLayer = None, kinetics: SurfaceKinetics = None,
                 galvanostat: Galvanostat = None):
    """Problem + boundary record for the 3D pore (reference 3D:329-382,460-467).  ``refine`` > 0 applies that many
    uniform refinements with inherited markers (gmpnp_amd.mesh.refine_pore); returns (problem, boundaries) of the
    mesh actually used (``problem.coords/cells``)."""
    bnd = mark_pore_boundaries(mesh, pp.aspect_pore, pore_wall_tolerance(pp.L, pp.R))
    for _ in range(refine):
        from .mesh import refine_pore
        mesh, bnd = refine_pore(mesh, bnd)
    dofs, vals = pore_dirichlet(pp, bnd, stern=stern is not None)
    prob = Problem(coords=mesh.coords, cells=mesh.cells, model=pp.model, quad=quad,
                   wall_facets=bnd.ds_facets[2], exit_facets=bnd.ds_facets[3], bc_dofs=dofs, bc_vals=vals, stern=stern, kinetics=kinetics, galvanostat=galvanostat)
    return prob, bnd


def pore_hierarchy(pp, mesh: Mesh, refine: int, quad: Quadrature = None):
    """The nested problems of a uniformly refined pore mesh, FINEST FIRST: [(problem, boundaries, parents), ...] with
    ``parents`` (nv, 2) = the vertices of the next-coarser mesh each vertex interpolates from (None on the coarsest, the
    reference mesh itself).  What the multilevel term of the preconditioner is built from (DeviceSolver.attach_coarse_level)."""
    bnd = mark_pore_boundaries(mesh, pp.aspect_pore, pore_wall_tolerance(pp.L, pp.R))
    levels = [(mesh, bnd)]
    for _ in range(refine):
        from .mesh import refine_pore
        levels.append(refine_pore(*levels[-1]))
    out = []
    for m, b in levels[::-1]:
        dofs, vals = pore_dirichlet(pp, b)
        prob = Problem(coords=m.coords, cells=m.cells, model=pp.model, quad=quad, wall_facets=b.ds_facets[2], exit_facets=b.ds_facets[3],
                       bc_dofs=dofs, bc_vals=vals)
        out.append((prob, b, getattr(m, "parents", None)))
    return out


def edl_problem(ep, mesh: Mesh, quad: Quadrature = None, stern: SternLayer = None, kinetics: SurfaceKinetics = None, galvanostat: Galvanostat = None):
    """Problem for the 1D EDL (reference 1D:237-254,350-355): all 7 fields pinned to
    (1,..,1,0) at x=1; p = voltage_multiplier at x=0; point fluxes at the x=0 vertex.  ``stern``: the OHP potential is not
    prescribed (the (left, ns, voltage) entry is dropped) and the record travels with the problem."""
    tol = 1.0e-14
    x = mesh.coords[:, 0]
    _, ext, _ = mesh.facets()
    right = np.nonzero(ext & (np.abs(x - 1.0) < tol))[0]
    left = np.nonzero(ext & (np.abs(x - 0.0) < tol))[0]
    ns = len(ep.species)
    bcs = [(right, f, 1.0) for f in range(ns)] + [(right, ns, 0.0)] + ([] if stern is not None else [(left, ns, ep.voltage_scaled)])
    dofs, vals = merge_dirichlet(bcs, ns + 1)
    return Problem(coords=mesh.coords, cells=mesh.cells, model=ep.model, quad=quad,
                   point_vertices=left.astype(np.int32), bc_dofs=dofs, bc_vals=vals, stern=stern, kinetics=kinetics, galvanostat=galvanostat)
