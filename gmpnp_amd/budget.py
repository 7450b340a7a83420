"""Species budgets of a run: the per-step tables of ``species_budget()`` (gmpnp_species_budget, include/gmpnp.h) and what the
drivers write from them (``budget.npz``, three ``metadata.json`` keys).  No reference counterpart: the reference writes fields only.

A table has one row per field (the model's species, potential last) and the columns ``backend.BUDGET_COLUMNS`` in the scaled
units of the weak form, with ``storage + reaction + wall + exit + point = dirichlet + closure`` per row.

Physical units.  The species equations are scaled with x = x' / L, u_i = c_i / c_i^0 and fluxes J_i = J_i' L / (D_i c_i^0)
(``J_prefactor`` of 3D/MPNP_CO2ER_pore.py:290-295, the ``J_*_prefactor`` of the 1D scripts without the Faraday constant),
so with L the scaling length (pore length / Nernst layer thickness), D_i the (effective) diffusivity and c_i^0 the scaling
concentration in mol / m^3:

    3D   rate columns (storage ... closure)   [mol / s]        = table * D_i c_i^0 L          (flux density D c / L times area L^2)
         inventory                            [mol]            = table * c_i^0 L^3
    1D   rate columns, per unit electrode area [mol / (m^2 s)]  = table * D_i c_i^0 / L
         inventory, per unit electrode area    [mol / m^2]      = table * c_i^0 L

The potential row has no such conversion: its factors are 1 (scaled units)."""
from __future__ import annotations

import os

import numpy as np

from .backend import BUDGET_COLUMNS

RATE_COLUMNS = BUDGET_COLUMNS[1:]     # everything but the inventory is a rate


def pore_factors(pp):
    """(rate factors, inventory factors), one entry per field, of a 3D pore run (``params.PoreParameters``)."""
    rate = [pp.diff_coeff_eff[s] * pp.bulk_conc[s] * pp.L for s in pp.species] + [1.0]
    amount = [pp.bulk_conc[s] * pp.L ** 3 for s in pp.species] + [1.0]
    return np.array(rate), np.array(amount)


def interval_factors(species, diff_coeff, conc, L_n):
    """The same for a 1D run (per unit electrode area)."""
    rate = [diff_coeff[s] * conc[s] / L_n for s in species] + [1.0]
    amount = [conc[s] * L_n for s in species] + [1.0]
    return np.array(rate), np.array(amount)


class BudgetLog:
    """The tables of a run, one per time step, taken after the step's Newton solve and before the boundary values and ``u_n``
    move on (so ``storage`` is the step's own and ``dirichlet`` belongs to the Dirichlet values the step was solved with)."""

    def __init__(self, fields, rate_factor, amount_factor):
        self.fields = list(fields)
        self.rate_factor, self.amount_factor = np.asarray(rate_factor, dtype=float), np.asarray(amount_factor, dtype=float)
        self.tables = []

    def take(self, system):
        self.tables.append(system.species_budget())

    def array(self):
        nf = len(self.fields)
        return np.stack(self.tables) if self.tables else np.zeros((0, nf, len(BUDGET_COLUMNS)))

    def physical(self):
        """(steps, nf, 8) in the physical units of the module docstring."""
        f = np.concatenate([self.amount_factor[:, None], np.repeat(self.rate_factor[:, None], len(RATE_COLUMNS), axis=1)], axis=1)
        return self.array() * f[None]

    def summary(self):
        """The ``metadata.json`` keys: CO2 consumed at the wall (3D) or at the OHP point (1D) and CO2 supplied by its Dirichlet
        faces at the last step, in the physical rate units; the largest |closure| of the run in scaled units."""
        t, p = self.array(), self.physical()
        col = {c: k for k, c in enumerate(BUDGET_COLUMNS)}
        out = {"CO2_wall_uptake": None, "CO2_entry_supply": None, "max_abs_closure": None}
        if len(t):
            i = self.fields.index("CO2")
            out["CO2_wall_uptake"] = float(p[-1, i, col["wall"]] + p[-1, i, col["point"]])
            out["CO2_entry_supply"] = float(p[-1, i, col["dirichlet"]])
            out["max_abs_closure"] = float(np.abs(t[:, :, col["closure"]]).max())
        return out

    def save(self, directory):
        """Writes ``budget.npz`` into `directory`; returns the metadata keys."""
        p = self.physical()
        np.savez(os.path.join(directory, "budget.npz"), table=self.array(), columns=np.array(BUDGET_COLUMNS), fields=np.array(self.fields),
                 table_physical=p, rate_factor=self.rate_factor, inventory_factor=self.amount_factor,
                 **{c + "_physical": p[:, :, k] for k, c in enumerate(BUDGET_COLUMNS) if c in ("wall", "exit", "point", "dirichlet", "closure")})
        return self.summary()
