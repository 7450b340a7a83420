"""The NumPy restatement of the species-budget table (tests/budget_reference.py) against the closed-form flux balance of
tests/closed_forms.flux_case, the two new symbols of the C ABI, and the drivers' ``--budget`` flag.  No GPU."""
import os
import re

import numpy as np
import pytest

import budget_reference as B
import closed_forms as cf
import gmpnp_oracle as O
import hp_reference as H
from conftest import ROOT, box_pore_problem, random_state


def flux_balance(prob, u, un, i):
    """The balance ``closed_forms.flux_case``'s ``check(state)`` forms for species i, in its own terms (facet and cell MEANS of
    the P1 field times areas and volumes), with u^n as given instead of 1, plus the 1D point flux:
    (J_wall |S2| + kappa int_S3 (u - 1) ds + inv_dt int (u - u^n) dx + J_point n_points, sum of the terms' magnitudes)."""
    m = prob.model
    nv, nf = prob.coords.shape[0], prob.nf
    U, Un = u.reshape(nv, nf), un.reshape(nv, nf)
    vol = B.cell_volumes(prob.coords, prob.cells)
    stored = m.inv_dt * float((vol * (U[prob.cells, i].mean(axis=1) - Un[prob.cells, i].mean(axis=1))).sum())
    scale = m.inv_dt * float((vol * np.abs(U[prob.cells, i] - Un[prob.cells, i]).mean(axis=1)).sum())
    wall = excess = 0.0
    if len(prob.wall_facets):
        a2 = B.facet_areas(prob.coords, prob.wall_facets)
        wall = m.wall_flux[i] * a2.sum()
    if len(prob.exit_facets):
        a3 = B.facet_areas(prob.coords, prob.exit_facets)
        excess = m.exit_kappa[i] * float((a3 * (U[prob.exit_facets, i].mean(axis=1) - 1.0)).sum())
        scale += abs(m.exit_kappa[i]) * float((a3 * (np.abs(U[prob.exit_facets, i]).mean(axis=1) + 1.0)).sum())
    point = m.point_flux[i] * len(prob.point_vertices)
    return wall + excess + stored + point, abs(wall) + scale + abs(point)


def _problems():
    out = [("box2_3", box_pore_problem(2, 3)[2]), ("boxpore", box_pore_problem()[2]), ("1d_5", H.edl_generated(H.uniform_mesh_1d(5)))]
    return out


@pytest.mark.parametrize("k", range(3))
def test_restatement_reproduces_the_flux_balance(k):
    """wall + exit + storage (+ point in 1D) of the restatement = the facet-mean / cell-mean balance of flux_case's check, for the
    two gases of flux_case (CO, H2 in 3D; CO2 and OH, the species with a point flux, in 1D), on a random state; and the identity
    closes: ``dirichlet`` (the remainder) is the sum of the oracle's raw residual over the Dirichlet dofs.  Tolerance: 1e-12 of
    the sum of the terms' magnitudes (a few thousand additions of fp64 terms)."""
    name, prob = _problems()[k]
    nv, ns = prob.coords.shape[0], prob.model.n_species
    u, un = random_state(nv, ns, seed=11)
    table, scale = B.budget(prob, u, un)
    species = list(prob.model.species)
    for X in (("CO", "H2") if prob.coords.shape[1] == 3 else ("CO2", "OH")):
        i = species.index(X)
        want, mag = flux_balance(prob, u, un, i)
        got = table[i, B.WALL] + table[i, B.EXIT] + table[i, B.STO] + table[i, B.POINT]
        assert mag > 0.0 and abs(got - want) <= 1e-12 * mag, (name, X, got, want)
    raw, _ = O.assemble(prob, u, un, want_jacobian=False, apply_bc=False)
    raw = raw.reshape(nv, ns + 1)
    bc = np.zeros(prob.ndof, dtype=bool)
    bc[prob.bc_dofs] = True
    bc = bc.reshape(nv, ns + 1)
    for f in range(ns + 1):
        d = raw[bc[:, f], f].sum()
        assert abs(table[f, B.DIR] - d) <= 1e-12 * (scale[f, B.DIR] + np.abs(raw[:, f]).sum()), (name, f)
    # the potential row: no storage, no boundary flux; the space charge is what its rows sum to
    assert table[ns, B.STO] == 0.0 and not table[ns, [B.WALL, B.EXIT, B.POINT]].any()
    assert abs(table[ns, B.REA] - raw[:, ns].sum()) <= 1e-12 * (scale[ns, B.REA] + np.abs(raw[:, ns]).sum())


def test_restatement_reproduces_flux_case_check():
    """On flux_case's own problem (the small generated cylinder) and u^n = 1, which is what its ``check`` assumes: the literal
    J_X_wall |S2| + kappa_X int_S3 (u_X - 1) ds + (1 / dt) int (u_X - 1) dx of ``check(state)`` for CO and H2."""
    prob, u0, check = cf.flux_case(coarse=(2, 5))
    nv, ns = prob.coords.shape[0], prob.model.n_species
    u, _ = random_state(nv, ns, seed=11)
    table, scale = B.budget(prob, u, u0)
    out = check(u)
    species = list(prob.model.species)
    for X in ("CO", "H2"):
        i = species.index(X)
        got = table[i, B.WALL] + table[i, B.EXIT] + table[i, B.STO]
        mag = scale[i, B.WALL] + scale[i, B.EXIT] + scale[i, B.STO]
        assert abs(got - out[X][0]) <= 1e-12 * mag, (X, got, out[X][0])
        assert abs(abs(table[i, B.WALL]) - out[X][1]) <= 1e-12 * out[X][1]


def test_partition_shares_add_up():
    """Owned-row shares of a two-way split of the vertices add up to the whole table (every row counted once, no cell-ownership
    rule): what the group form's all-reduce relies on."""
    prob = box_pore_problem(2, 3)[2]
    nv, ns = prob.coords.shape[0], prob.model.n_species
    u, un = random_state(nv, ns, seed=11)
    whole, scale = B.budget(prob, u, un)
    own = prob.coords[:, 2] < 0.5
    a, _ = B.budget(prob, u, un, owned=own)
    b, _ = B.budget(prob, u, un, owned=~own)
    assert np.abs(a + b - whole).max() <= 1e-12 * scale.max()
    assert (np.abs(a).sum() > 0) and (np.abs(b).sum() > 0)


def test_abi_names_both_symbols():
    from gmpnp_amd import backend
    header = open(os.path.join(ROOT, "include", "gmpnp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("gmpnp_species_budget", "gmpnp_group_species_budget"):
        assert name in backend.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
    assert re.search(r"#define\s+GMPNP_BUDGET_COLUMNS\s+8\b", code)
    assert len(backend.BUDGET_COLUMNS) == 8 and backend.BUDGET_COLUMNS == B.COLUMNS
    for k, c in enumerate(backend.BUDGET_COLUMNS):   # the enum of column indices
        assert re.search(r"GMPNP_BUDGET_%s\s*=\s*%d\b" % (c.upper(), k), code), c


def test_budget_flag_parses_on_all_four_drivers():
    from gmpnp_amd import edl1d, pore3d, rxndiff1d, rxnpore3d
    for mod in (pore3d, rxnpore3d, edl1d, rxndiff1d):
        p = mod.build_parser()
        assert p.parse_args([]).budget is False
        assert p.parse_args(["--budget"]).budget is True
    from gmpnp_amd import edl_sweep
    assert edl_sweep.build_parser().parse_args(["--voltage_multiplier", "-1", "--budget"]).budget is True


def test_budget_log_units_and_summary():
    """The physical copies: rate columns times D_i c_i L (3D), inventory times c_i L^3; the summary keys from the last step."""
    from gmpnp_amd.budget import BudgetLog, pore_factors
    from gmpnp_amd.params import pore_parameters
    pp = pore_parameters(concentration_elec=0.5, L=10e-9, R=5e-9)
    log = BudgetLog(list(pp.species[:7]) + ["cat", "p"], *pore_factors(pp))
    rng = np.random.default_rng(0)

    class Sys:
        def species_budget(self):
            return rng.standard_normal((9, 8))

    for _ in range(3):
        log.take(Sys())
    t, p = log.array(), log.physical()
    assert t.shape == p.shape == (3, 9, 8)
    i = 4
    assert pp.species[i] == "CO2"
    f = pp.diff_coeff_eff["CO2"] * pp.bulk_conc["CO2"] * pp.L
    assert np.allclose(p[:, i, 1:], t[:, i, 1:] * f, rtol=1e-15) and np.allclose(p[:, i, 0], t[:, i, 0] * pp.bulk_conc["CO2"] * pp.L ** 3, rtol=1e-15)
    assert np.array_equal(p[:, 8], t[:, 8])
    s = log.summary()
    assert s["CO2_wall_uptake"] == float(p[-1, i, 3] + p[-1, i, 5]) and s["CO2_entry_supply"] == float(p[-1, i, 6])
    assert s["max_abs_closure"] == float(np.abs(t[:, :, 7]).max())
