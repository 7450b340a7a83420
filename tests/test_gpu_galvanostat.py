"""The galvanostatic mode on the GPU (gmpnp_set_galvanostat, csrc/gmpnp_galvanostat.h) against the NumPy
restatement of tests/galvanostat_reference.py: the terms of the bordered system on the mesh shapes where the gathers change form, the
option switched off again, the first-step table of the 1D driver, the 3D first step with the band LU, p_M across accept and reject,
the budgets, status bit 128, every refusal of the library and hook 26.  Every handle is closed by `with` / `finally`."""
import copy
import math

import numpy as np
import pytest

import galvanostat_reference as GR
import kinetics_reference as K
from conftest import random_state
from precond_reference import relerr
from step_limit_reference import first_step_state
from test_galvanostat_reference import CALIBRATION, FIRST_STEP, galvanostatic_first_step_problem
from test_gpu_kinetics import ASSEMBLY_CASES, PORE_TAFEL, _species_rows_close, edl_k, kinetic_problem  # noqa: F401 (fixture)
from test_gpu_stern_bc import SP_FIRST, _closes
from test_kinetics_reference import TAFEL, first_step_problem, two_reactions
from gmpnp_amd.problem import Galvanostat, SternLayer, edl_problem
from gmpnp_amd.stern import L_STERN

pytestmark = pytest.mark.gpu
P_M = -20.0


def galvanostatic_problem(case, model, pore10, edl_k, target_factor=0.7, weights=(1.0, 0.6)):
    """(problem with the galvanostat on, the same problem without it, random state) of an assembly case: two reactions at p_M = -20
    beside the Stern boundary condition, the target a fraction of the current at that state."""
    on, _ = kinetic_problem(case, "kin+" + model, pore10, edl_k, p_M=P_M)
    nv, ns = on.coords.shape[0], on.nf - 1
    u, un = random_state(nv, ns, seed=3)
    off = copy.copy(on)
    on = copy.copy(on)
    on.galvanostat = Galvanostat(1.0, weights)
    on.galvanostat = Galvanostat(target_factor * GR.total_current(on, u)[1], weights)
    return on, off, u, un


@pytest.mark.parametrize("model", ["linear", "BDM"])
@pytest.mark.parametrize("case", ASSEMBLY_CASES)
def test_terms_match_the_numpy_restatement(case, model, pore10, edl_k, gpu_lib):
    """b, G, d, I and c.x of gmpnp_galvanostat_terms at a random state for a random x: 1e-12 relative (the bound of the F / J tests of
    sections 5h and 5i); two calls give equal bits; F and J of the handle are bitwise those of a handle without the option that had
    the same p_electrode set directly."""
    on, off, u, un = galvanostatic_problem(case, model, pore10, edl_k)
    x = np.random.default_rng(11).standard_normal(on.ndof)
    nodes, _ = K.boundary_weights(on)
    if case == "pore10":
        assert len(nodes) > 256                                            # more boundary nodes than one workgroup has lanes
        assert np.intersect1d(nodes * on.nf + on.nf - 1, on.bc_dofs).size or np.intersect1d(nodes * on.nf + 4, on.bc_dofs).size   # Dirichlet rows on the wall
    with gpu_lib.DeviceSolver(off) as dev0:
        dev0.set_state(u, un)
        F0, _ = dev0.assemble(True)
        A0 = dev0.jacobian_csr()
    with gpu_lib.DeviceSolver(on) as dev:
        dev.set_state(u, un)
        b, sc = dev.galvanostat_terms(x)
        b2, sc2 = dev.galvanostat_terms(x)
        assert np.array_equal(b, b2) and sc == sc2
        F, _ = dev.assemble(True)
        A = dev.jacobian_csr()
        rep = dev.galvanostat_report()
        cur = dev.kinetics_currents()
    bo = GR.rhs_b(on, u)
    Go, co, do, Io, I_ro = GR.constraint(on, u)
    cxo = float(co @ x)
    errs = dict(b=relerr(b, bo), G=abs(sc["G"] - Go) / abs(Go), d=abs(sc["d"] - do) / abs(do), I=abs(sc["I"] - Io) / abs(Io),
                cx=abs(sc["cx"] - cxo) / abs(cxo))
    print(case, model, " ".join("%s %.2e" % kv for kv in errs.items()))
    assert max(errs.values()) < 1e-12
    assert np.count_nonzero(bo) >= 4 and not b[on.bc_dofs].any() and np.array_equal(b == 0.0, bo == 0.0)
    assert np.array_equal(F, F0) and np.array_equal(A.data, A0.data)
    assert rep["p_electrode"] == rep["p_electrode_n"] == P_M and rep["G"] == sc["G"] and rep["I"] == sc["I"]
    assert np.array_equal(rep["I_r"], cur) and np.all(np.abs(cur - I_ro) <= 1e-12 * np.abs(I_ro))


def test_off_after_on(edl_k, gpu_lib):
    """One galvanostatic solve moves p_M; on = 0 writes it into the Stern and kinetics options: F and J are then bitwise those of a
    handle that had that potential from the start, and a potentiostatic solve holds it.  on = 0 on a handle that never had the option
    changes nothing."""
    ep, mesh = edl_k
    case = (10.0, -5.0, "BDM", 0.9)
    prob = galvanostatic_first_step_problem(ep, mesh, case)
    u0, un = first_step_state(prob)
    opts = gpu_lib.newton_options(gpu_lib.with_step_fraction(SP_FIRST, 0.9), dim=1)
    with gpu_lib.DeviceSolver(prob) as dev:
        dev.set_state(u0, un)
        st = dev.newton_solve(opts)
        p_found = dev.galvanostat_report()["p_electrode"]
        u = dev.get_state()
        dev.set_galvanostat(None)
        with pytest.raises(gpu_lib.GmpnpError, match="galvanostat"):
            dev.galvanostat_report()
        F, _ = dev.assemble(True)
        A = dev.jacobian_csr()
        cur = dev.kinetics_currents()
        st2 = dev.newton_solve(opts)
    assert st["converged"] and abs(p_found - FIRST_STEP[case][1]) < 1e-6 and p_found != -5.0
    direct = GR.with_potential(prob, p_found)
    direct.galvanostat = None
    with gpu_lib.DeviceSolver(direct) as dev1:
        dev1.set_state(u, un)
        F1, _ = dev1.assemble(True)
        A1 = dev1.jacobian_csr()
        cur1 = dev1.kinetics_currents()
        before = (F1.copy(), A1.data.copy())
        dev1.set_galvanostat(None)                                       # never on: a no-op
        F1b, _ = dev1.assemble(True)
        assert np.array_equal(F1b, before[0]) and np.array_equal(dev1.jacobian_csr().data, before[1])
    assert np.array_equal(F, F1) and np.array_equal(A.data, A1.data) and np.array_equal(cur, cur1)
    assert st2["converged"] and st2["iterations"] <= 2 and abs(math.log(cur.sum() / 10.0)) < 1e-6


@pytest.mark.parametrize("case", sorted(FIRST_STEP))
def test_first_step_through_the_driver(case, edl_k, gpu_lib):
    """EDLRun's first step in galvanostatic mode (K+, 1 um mesh) against the NumPy bordered loop: the same Newton count and limiter
    factors, p_M and the state within 1e-8 (the bound of sections 5h and 5i for this comparison), the table's figures, and the
    calibration rows recover the potential their target was measured at within 1e-6."""
    from gmpnp_amd.edl1d import EDLRun
    target, p0, model, tau = case
    its, p_found, p_ohp, i_CO, i_H2, min_step = FIRST_STEP[case]
    ep, mesh = edl_k
    prob = galvanostatic_first_step_problem(ep, mesh, case)
    u_ref, p_ref, st_ref = GR.newton_loop(prob, *first_step_state(prob), p0, tau=tau)
    run = EDLRun(num_steps=1, solver_parameters=SP_FIRST, step_fraction=tau, electrode_voltage=p0, stern_model=model, L_n=1e-6, cation="K", kinetics="tafel",
                 target_current=target, **{k: TAFEL[k] for k in ("i0_CO", "i0_H2")})
    try:
        assert run.problem.kinetics == prob.kinetics and run.problem.stern == prob.stern and run.problem.galvanostat == prob.galvanostat
        st = run.step(verbose=False)
        u = run.sys.dev.get_state()
        rep = run.sys.dev.galvanostat_report()
        summary = run.kinetics_summary()
        meta = run.stern_summary()
    finally:
        run.sys.close()
    p_M = summary["electrode_voltage"][0]
    print(case, st["iterations"], st["min_step"], p_M, abs(p_M - p_ref), np.abs(u - u_ref).max(), rep["G"])
    assert st["converged"] and st["iterations"] == st_ref.iterations == its
    if tau:
        # the factors within 1e-8 relative, the bound of section 5i for factors of a plain Newton step, times what the bordered step
        # makes of an error of its two solves (galvanostat_reference.factor_amplification, from the NumPy loop's own terms); the
        # smallest one under the bound the table pins it to
        tol = 1e-8 * np.asarray(st_ref.amplification)
        err = np.abs(np.asarray(st["step_factor"][:its]) - st_ref.step_factor) / np.asarray(st_ref.step_factor)
        print("step factors: worst error / bound = %.2e, largest amplification %.2e" % ((err / tol).max(), max(st_ref.amplification)))
        assert (err <= tol).all() and abs(st["min_step"] - min_step) < 1e-6
    assert abs(p_M - p_ref) <= 1e-8 * max(1.0, abs(p_ref)) and np.abs(u - u_ref).max() <= 1e-8 * max(1.0, np.abs(u_ref).max())
    assert abs(p_M - p_found) < 1e-6 and abs(u.reshape(-1, 7)[0, 6] - p_ohp) < 1e-6
    assert np.allclose([summary["i_CO"][0], summary["i_H2"][0]], (i_CO, i_H2), rtol=1e-6, atol=0.0)
    assert rep["p_electrode"] == p_M == meta["electrode_voltage"] and rep["p_electrode_n"] == p_M       # the step was assigned
    assert abs(rep["G"]) < 1e-6 and rep["alpha"] == st["step_factor"][its - 1] if tau else rep["alpha"] == 1.0
    if target in CALIBRATION:
        assert abs(p_M - CALIBRATION[target]) < 1e-6


SP_TIGHT_3D = {"nonlinear_solver": "newton", "newton_solver": {"linear_solver": "band_lu", "maximum_iterations": 50, "relative_tolerance": 1.0e-12,
                                                                "absolute_tolerance": 1.0e-9}}


def test_first_step_3d_generated_cylinder(pore10, edl_k, gpu_lib):
    """The 259-vertex cylinder, first step from u = 0 with the band LU (one factorisation, two substitutions per iteration) against
    the NumPy bordered loop: the same Newton count, p_M and the state within 1e-8.  The target is half the current of the
    potentiostatic first step at p_M = -1 (its own NumPy loop), the start p_M = -1."""
    on, _ = kinetic_problem("cyl259", "kin+BDM", pore10, edl_k, p_M=-1.0)
    u_pot, st_pot = K.newton_loop(on, *first_step_state(on))
    assert st_pot.converged
    on.galvanostat = Galvanostat(0.5 * K.currents(on, u_pot).sum())
    u_ref, p_ref, st_ref = GR.newton_loop(on, *first_step_state(on), -1.0)
    assert st_ref.converged and st_ref.ok and abs(p_ref + 1.0) > 0.1
    sp = {"nonlinear_solver": "newton", "newton_solver": dict(SP_FIRST["newton_solver"], linear_solver="band_lu")}
    with gpu_lib.DeviceSolver(on) as dev:
        dev.set_state(*first_step_state(on))
        st = dev.newton_solve(gpu_lib.newton_options(sp, dim=3))
        u = dev.get_state()
        rep = dev.galvanostat_report()
    print("cyl259:", st["iterations"], st_ref.iterations, rep["p_electrode"], p_ref, np.abs(u - u_ref).max(), rep["G"])
    assert st["converged"] and st["iterations"] == st_ref.iterations and st["direct_solves"] == st["iterations"]
    assert abs(rep["p_electrode"] - p_ref) <= 1e-8 * max(1.0, abs(p_ref)) and np.abs(u - u_ref).max() <= 1e-8 * max(1.0, np.abs(u_ref).max())


def test_first_step_3d_calibration_on_the_pore(gpu_lib):
    """L_10_R_5 through PoreRun: the currents of the potentiostatic first step at p_M = -1 (i0_CO = 10, i0_H2 = 1) are the target of a
    galvanostatic first step from p_M = -0.5, which recovers -1 within 1e-6 and the potentiostatic state within 1e-8.  The
    galvanostatic first solve starts from the bulk state (PoreRun: from u = 0, where the CO2 current is exactly 0, the bordered
    iteration leaves the admissible set on this mesh, in the NumPy loop too)."""
    from gmpnp_amd.pore3d import PoreRun
    kw = dict(num_steps=1, solver_parameters=SP_TIGHT_3D, L=10e-9, R=5e-9, concentration_elec=0.5, **PORE_TAFEL)
    pot = PoreRun(electrode_voltage=-1.0, **kw)
    try:
        st0 = pot.step(verbose=False)
        k0 = pot.kinetics_summary()
        u_pot = pot.history[-1].copy()
    finally:
        pot.sys.close()
    target = float(k0["i_CO"][0] + k0["i_H2"][0])
    with pytest.raises(ValueError, match="target_current"):
        PoreRun(electrode_voltage=-0.5, target_current=target, **dict(kw, solver_parameters={"newton_solver": {"linear_solver": "bicgstab"}}))
    gal = PoreRun(electrode_voltage=-0.5, target_current=target, **kw)
    try:
        assert abs(gal.problem.galvanostat.target - target * gal.wall_area()) <= 1e-15 * target * gal.wall_area()
        st = gal.step(verbose=False)
        k1 = gal.kinetics_summary()
        u_gal = gal.history[-1].copy()
        meta = gal.stern_summary()
    finally:
        gal.sys.close()
    p_M = k1["electrode_voltage"][0]
    print("pore10 calibration:", st0["iterations"], st["iterations"], target, p_M, np.abs(u_gal - u_pot).max(), st["residuals"][-1])
    assert st0["converged"] and st["converged"] and st["direct_solves"] == st["iterations"] > 0
    assert abs(p_M + 1.0) < 1e-6 and meta["electrode_voltage"] == p_M
    assert np.abs(u_gal - u_pot).max() <= 1e-8 * max(1.0, np.abs(u_pot).max())
    assert abs(k1["i_CO"][0] + k1["i_H2"][0] - target) <= 1e-6 * target


def test_potential_across_accept_and_reject(edl_k, gpu_lib):
    """time_reject after a solve restores the pre-solve p_M bitwise (and the currents with it); time_accept and assign_previous move
    it to its twin at u_n.  A short adaptive run at a set current ends with finite outputs and |ln(I / I_target)| under the Newton
    tolerance at every accepted step."""
    from gmpnp_amd.edl1d import EDLRun
    ep, mesh = edl_k
    prob = galvanostatic_first_step_problem(ep, mesh, (10.0, -5.0, "BDM", 0.9))
    u0, un = first_step_state(prob)
    opts = gpu_lib.newton_options(gpu_lib.with_step_fraction(SP_FIRST, 0.9), dim=1)
    with gpu_lib.DeviceSolver(prob) as dev:
        dev.set_state(un, un)
        cur0 = dev.kinetics_currents()
        dev.set_state(u0, un)
        dev.newton_solve(opts)
        r = dev.galvanostat_report()
        assert r["p_electrode"] != -5.0 and r["p_electrode_n"] == -5.0
        dev.time_reject()
        r2 = dev.galvanostat_report()
        assert r2["p_electrode"] == -5.0 and r2["p_electrode_n"] == -5.0 and np.array_equal(dev.get_state(), un)
        assert np.array_equal(dev.kinetics_currents(), cur0)              # the kinetics' device option went back with it
        dev.set_state(u0, un)
        dev.newton_solve(opts)
        p1 = dev.galvanostat_report()["p_electrode"]
        assert p1 == r["p_electrode"]                                     # the same solve from the same start: equal bits
        dev.time_accept()
        assert dev.galvanostat_report()["p_electrode_n"] == p1
        dev.newton_solve(opts)
        p2 = dev.galvanostat_report()
        assert p2["p_electrode_n"] == p1 and p2["p_electrode"] != p1
        dev.assign_previous()
        assert dev.galvanostat_report()["p_electrode_n"] == p2["p_electrode"]
    run = EDLRun(adaptive_dt=True, max_steps=12, solver_parameters=SP_FIRST, step_fraction=0.9, electrode_voltage=-5.0, L_n=1e-6, cation="K",
                 kinetics="tafel", target_current=10.0, **{k: TAFEL[k] for k in ("i0_CO", "i0_H2")})
    try:
        run.run(verbose=False)
        k = run.kinetics_summary()
        last = run.history[-1]
    finally:
        run.sys.close()
    assert 1 <= len(k["i_CO"]) <= 12 and len(k["electrode_voltage"]) == len(k["i_CO"]) == run.n
    assert np.isfinite(last).all() and all(np.isfinite(v).all() for v in k.values())
    G = np.log((k["i_CO"] + k["i_H2"]) / 10.0)
    print("adaptive galvanostatic run: %d accepted steps, max |G| = %.2e, p_M %s" % (run.n, np.abs(G).max(), k["electrode_voltage"]))
    assert np.abs(G).max() < 1e-6


def test_budget_1d(edl_k, gpu_lib):
    """--budget with the option on, one 1D step: every row closes under the bound of test_gpu_kinetics.py, and the species rows' point
    entries carry the kinetic flux at the potential that was found."""
    from gmpnp_amd.edl1d import EDLRun
    import budget_reference as B
    run = EDLRun(num_steps=1, budget=True, electrode_voltage=-5.0, stern_model="BDM", L_n=1e-6, cation="K", kinetics="tafel", i0_CO=1.0, i0_H2=0.2,
                 target_current=10.0)
    try:
        st = run.step(verbose=False)
        t = run.budget.array()
        u = run.sys.dev.get_state()
        table_now = run.sys.species_budget()
        p_M = run.potentials[-1]
    finally:
        run.sys.close()
    _closes(t[0], run.problem, st["residuals"][-1])
    _species_rows_close(table_now, B.COLUMNS.index("point"), GR.with_potential(run.problem, p_M), u)


def test_budget_3d(gpu_lib):
    """The same for one L_10_R_5 step through PoreRun: the kinetic fluxes sit in the species rows' wall column."""
    from gmpnp_amd.pore3d import PoreRun
    import budget_reference as B
    run = PoreRun(num_steps=1, budget=True, electrode_voltage=-0.5, L=10e-9, R=5e-9, concentration_elec=0.5, target_current=80.0, **PORE_TAFEL)
    try:
        st = run.step(verbose=False)
        t = run.budget.array()
        u = run.sys.dev.get_state()
        table_now = run.sys.species_budget()
        p_M = run.potentials[-1]
    finally:
        run.sys.close()
    _closes(t[0], run.problem, st["residuals"][-1])
    _species_rows_close(table_now, B.COLUMNS.index("wall"), GR.with_potential(run.problem, p_M), u)


def test_a_current_that_is_not_positive_is_a_numeric_status(edl_k, gpu_lib):
    """i0_H2 = 0 and a negative CO2 value planted at the OHP make I < 0: gmpnp_newton_solve and the terms hook report
    GMPNP_ERR_NUMERIC and name the galvanostat (bit 128: an error code from a finite computation); the handle solves a good state
    afterwards."""
    ep, mesh = edl_k
    prob = first_step_problem(ep, mesh, -5.0, par=dict(TAFEL, i0_H2=0.0))
    prob.galvanostat = Galvanostat(10.0)
    nv = prob.coords.shape[0]
    u0, un = first_step_state(prob)
    bad = un.copy().reshape(nv, 7)
    bad[int(prob.point_vertices[0]), 4] = -0.25
    assert GR.total_current(prob, bad.ravel())[1] < 0.0
    opts = gpu_lib.newton_options(gpu_lib.with_step_fraction(SP_FIRST, 0.9), dim=1)
    with gpu_lib.DeviceSolver(prob) as dev:
        dev.set_state(bad.ravel(), un)
        for call in (lambda: dev.newton_solve(opts), lambda: dev.galvanostat_terms()):
            with pytest.raises(gpu_lib.GmpnpError, match="galvanostat") as ei:
                call()
            assert ei.value.code == gpu_lib.ERR_NUMERIC
        assert np.array_equal(dev.get_state(), bad.ravel()) and dev.galvanostat_report()["p_electrode"] == -5.0      # nothing was applied
        dev.set_state(un, un)                                             # (from u = 0 the CO2 current, the only one here, would be 0)
        st = dev.newton_solve(opts)
        rep = dev.galvanostat_report()
    assert st["converged"] and st["iterations"] > 0 and abs(rep["G"]) < 1e-6 and rep["I"] > 0.0


def test_library_refusals_and_hook_26(pore10, edl_k, gpu_lib):
    """gmpnp_set_galvanostat without the kinetics, with bad options, with a Stern potential that differs, on a partition handle and on
    a multilevel level; the BiCGStab solvers with the option on; the kinetics switched off under it; order 2; an ensemble with such a
    member; the calls that need the option on; hook 26."""
    from ctypes import byref
    from gmpnp_amd import dist
    from gmpnp_amd.problem import pore_hierarchy
    from gmpnp_amd.solver import GMPNPSystem
    pp, mesh, prob3, _ = pore10
    ep, m1 = edl_k
    g = Galvanostat(10.0)

    def refused(call, what="galvanostat"):
        with pytest.raises(gpu_lib.GmpnpError, match=what) as ei:
            call()
        assert ei.value.code == gpu_lib.ERR_INVALID

    dom, perm, part = dist.partition_plan(prob3, 2, 0)
    with gpu_lib.DeviceSolver(dom.problem, perm=perm, partition=part) as partitioned:
        refused(lambda: partitioned.set_galvanostat(g))
        partitioned.set_galvanostat(None)                              # off is always accepted
    levels = pore_hierarchy(pp, mesh, 1)
    ml = GMPNPSystem(levels[0][0], levels=levels)
    try:
        refused(lambda: ml.dev.set_galvanostat(g))
        refused(lambda: ml._coarse[0].set_galvanostat(g))
    finally:
        ml.close()
    kin1 = two_reactions(ep.species, -5.0)
    plain = edl_problem(ep, m1)
    with_kin = edl_problem(ep, m1, stern=SternLayer("BDM", -5.0, L_STERN / ep.L_n), kinetics=kin1)
    other_p = edl_problem(ep, m1, stern=SternLayer("BDM", -4.0, L_STERN / ep.L_n), kinetics=kin1)
    with gpu_lib.DeviceSolver(plain) as a, gpu_lib.DeviceSolver(with_kin) as b, gpu_lib.DeviceSolver(other_p) as c:
        u0, un = first_step_state(plain)
        for d in (a, b, c):
            d.set_state(u0, un)
        refused(lambda: a.set_galvanostat(g))                          # no kinetics
        refused(lambda: c.set_galvanostat(g))                          # two electrode potentials
        refused(lambda: b.galvanostat_report())
        refused(lambda: b.galvanostat_terms())
        b.assemble(True)
        refused(lambda: b.time_kernel(26, 1))                          # the option is off
        for target, weights in ((0.0, (1.0, 1.0)), (-1.0, (1.0, 1.0)), (float("nan"), (1.0, 1.0)), (float("inf"), (1.0, 1.0)), (1.0, (0.0, 0.0)),
                                (1.0, (1.0, float("nan")))):
            bad = gpu_lib.CGalvanostat()
            bad.on, bad.target = 1, target
            bad.weight[0], bad.weight[1] = weights
            assert b.lib.gmpnp_set_galvanostat(b._h, byref(bad)) == gpu_lib.ERR_INVALID and "galvanostat" in b.lib.gmpnp_last_error().decode()
        b.set_galvanostat(g)
        for lin in ("bicgstab",):
            refused(lambda: b.newton_solve(gpu_lib.newton_options({"newton_solver": {"linear_solver": lin}}, dim=3)))
        refused(lambda: b.newton_solve(gpu_lib.newton_options({"newton_solver": {"linear_solver": "bicgstab", "preconditioner": "jacobi"}}, dim=3)))
        refused(lambda: b.set_kinetics(None))
        refused(lambda: b.set_time_order(2))
        refused(lambda: gpu_lib.DeviceEnsemble([a, b]))
        b.set_galvanostat(None)
        refused(lambda: gpu_lib.DeviceEnsemble([a, b]), "Stern|kinetics")     # (b still has those: refused as before the option)
        b.set_galvanostat(g)
        refused(lambda: b.time_kernel(26, 1), "no Jacobian")
        b.assemble(True)
        before = (b.get_state(), b.galvanostat_report()["p_electrode"])
        assert b.time_kernel(26, 2) > 0.0
        assert np.array_equal(b.get_state(), before[0]) and b.galvanostat_report()["p_electrode"] == before[1]
        b.jacobian_csr()                                               # hook 26 leaves the Jacobian alone
    kin3 = two_reactions(list(prob3.model.species), -1.0)
    p3 = copy.copy(levels[0][0])
    p3.kinetics = kin3
    with gpu_lib.DeviceSolver(p3) as d3, gpu_lib.DeviceSolver(levels[1][0], shared_device=1) as coarse:
        d3.set_galvanostat(Galvanostat(1.0))
        d3.set_state(*first_step_state(p3))
        refused(lambda: d3.newton_solve(gpu_lib.newton_options({"newton_solver": {"linear_solver": "bicgstab"}}, dim=3)))
        refused(lambda: d3.attach_coarse_level(coarse, levels[0][2]), "galvanostat|kinetics")
