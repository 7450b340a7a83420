"""Potential-dependent electrode kinetics (``--kinetics tafel`` of the 1D and 3D MPNP drivers,
``gmpnp_set_kinetics``): the Python statement of the rate rule and the two Tafel reactions the drivers build from their parameters.

    CO2 + H2O + 2e- -> CO + 2OH-      first order in the scaled CO2 concentration at the boundary node
    2H2O + 2e-      -> H2 + 2OH-      no reactant

``rate_r = i0_r (u_CO2 or 1) exp(-alpha_r (p_M - p - p_eq_r))`` is a partial current density in A/m2; the flux weights ``nu`` are the
prefactors the constant ``point_flux`` / ``wall_flux`` are built from (gmpnp_amd/params.py), so that a rate equal to the prescribed
partial current gives the prescribed flux.  The constant fluxes of the species the reactions drive are zeroed; ``current_OHP_ss`` /
``current_rough`` and ``H2_FE`` are then unused for them.  No reference counterpart: the reference prescribes the current.
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np

from .problem import SurfaceKinetics, SurfaceReaction


def surface_rate(k, alpha, p_eq, p_M, p, has_reactant, u_reactant):
    """(rate, d rate / d u_reactant, d rate / d p, ok) of one reaction at one node: ``surface_rate`` of gmpnp_host_rules.h, operation
    for operation.  ok = False where the rate or a derivative is not finite (the library raises status bit 64)."""
    x = -alpha * (p_M - p - p_eq)
    try:
        E = math.exp(x)
    except OverflowError:
        E = math.inf
    with np.errstate(all="ignore"):
        kE = float(np.float64(k) * np.float64(E))
        rate = float(np.float64(kE) * np.float64(u_reactant)) if has_reactant else kE
        d_p = float(np.float64(alpha) * np.float64(rate))
    ok = math.isfinite(rate) and math.isfinite(kE) and math.isfinite(d_p)
    return rate, kE, d_p, ok


def galvanostat_step(I, I_target, cy, cz, d):
    """(G, dp, ok) of the galvanostat's constraint G = ln(I / I_target) and the potential's correction dp = (G - c.y) / (d - c.z) of
    the bordered Newton step: ``galvanostat_step`` of gmpnp_host_rules.h, operation for operation.  ok = False where I <= 0, where a
    term is not finite or where d - c.z == 0 (the library raises status bit 128 and applies no update)."""
    fin = math.isfinite
    with np.errstate(all="ignore"):
        G = 0.0
        if I > 0.0:
            q = float(np.float64(I) / np.float64(I_target))
            G = math.log(q) if 0.0 < q < math.inf else (math.inf if q > 0.0 else -math.inf)     # C's log at Inf and at an underflowed 0
        den = float(np.float64(d) - np.float64(cz))
        dp = float((np.float64(G) - np.float64(cy)) / np.float64(den)) if den != 0.0 else 0.0
    ok = bool(I > 0.0 and fin(I) and fin(G) and fin(cy) and fin(cz) and den != 0.0 and fin(den) and fin(dp))
    return G, dp, ok


def tafel_parameters(par):
    """The metadata keys that record the kinetic parameters of a run (``problem.pop_kinetics``)."""
    return {"kinetics": "tafel", **{k: par[k] for k in ("i0_CO", "i0_H2", "alpha_CO", "alpha_H2", "p_eq_CO", "p_eq_H2")}}


def edl_tafel(ep, par, p_electrode):
    """(SurfaceKinetics, model with the driven constant fluxes zeroed) of the 1D double-layer driver: ``nu`` from the prefactors of
    ``params.edl_parameters`` (J_CO2 = J_CO2_prefactor i 0.5 CO_FE, J_OH = -J_OH_prefactor i (1 - f_H), J_H = J_H_prefactor i f_H)."""
    f_H = ep.current_H_frac
    oh_h = {"OH": -ep.J_OH_prefactor * (1.0 - f_H), "H": ep.J_H_prefactor * f_H}
    reactions = [SurfaceReaction(k=par["i0_CO"], alpha=par["alpha_CO"], p_eq=par["p_eq_CO"], reactant="CO2",
                                 nu={"CO2": ep.J_CO2_prefactor * 0.5, **oh_h}),
                 SurfaceReaction(k=par["i0_H2"], alpha=par["alpha_H2"], p_eq=par["p_eq_H2"], reactant=None, nu=dict(oh_h))]
    flux = np.array(ep.model.point_flux, dtype=np.float64, copy=True)
    for name in ("CO2", "OH", "H"):
        flux[ep.species.index(name)] = 0.0
    return SurfaceKinetics(reactions, float(p_electrode)), dataclasses.replace(ep.model, point_flux=flux)


def pore_tafel(pp, par, p_electrode, farad):
    """The same for the 3D pore driver: the ``J_prefactor[...] / farad`` factors of ``J_wall`` (params.pore_parameters) with the CO and
    H2 product fluxes; the rates are planar partial current densities."""
    Jp = {k: v / farad for k, v in pp.scalars["J_prefactor"].items()}
    reactions = [SurfaceReaction(k=par["i0_CO"], alpha=par["alpha_CO"], p_eq=par["p_eq_CO"], reactant="CO2",
                                 nu={"CO2": Jp["CO2"] * 0.5, "CO": Jp["CO"] * 0.5 * (-1.0), "OH": Jp["OH"] * (-1.0)}),
                 SurfaceReaction(k=par["i0_H2"], alpha=par["alpha_H2"], p_eq=par["p_eq_H2"], reactant=None,
                                 nu={"H2": Jp["H2"] * 0.5 * (-1.0), "OH": Jp["OH"] * (-1.0)})]
    flux = np.array(pp.model.wall_flux, dtype=np.float64, copy=True)
    for name in ("CO2", "CO", "H2", "OH"):
        flux[pp.species.index(name)] = 0.0
    return SurfaceKinetics(reactions, float(p_electrode)), dataclasses.replace(pp.model, wall_flux=flux)


def current_summary(currents, area):
    """{i_CO, i_H2, FE_H2} from the integrated rates of the two Tafel reactions and sum_I w_I (the area mean)."""
    i_CO, i_H2 = float(currents[0]) / area, float(currents[1]) / area
    tot = i_CO + i_H2
    return {"i_CO": i_CO, "i_H2": i_H2, "FE_H2": i_H2 / tot if tot != 0.0 else float("nan")}
