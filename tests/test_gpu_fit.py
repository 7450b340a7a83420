"""The parameter advance and the fit of the electrode kinetics on the GPU (gmpnp_parameter_advance / gmpnp_get_electrode_options,
csrc/gmpnp_tangent.h; gmpnp_amd/fit.py): the advance against the NumPy statement of its rule bit for bit (six
columns in two orders, tau = 0 and 0.9, ten columns, 3D), against gmpnp_electrode_advance for one p_M column, a twin handle given the
options read back and the new state, every refusal; the fit's Jacobian against differences of re-converged curves; the round trip
through ``EDLRun.fit`` with four and five parameters, with and without the predictor; the driver's --fit_data.  The fixtures are those
of test_gpu_tangent.py.  Every handle is closed by `with` / `finally`."""
import json
import math
import os

import numpy as np
import pytest

import fit_reference as FR
import response_reference as R
from conftest import random_state
from step_limit_reference import first_step_state
from test_gpu_kinetics import edl_k  # noqa: F401 (fixture)
from test_gpu_tangent import CASES, P_M, PARAMS, SHUFFLED, STEADY, four_reactions, inputs  # noqa: F401 (inputs: fixture)
from test_kinetics_reference import TAFEL, two_reactions
from gmpnp_amd import fit as ft
from gmpnp_amd.problem import Galvanostat, SternLayer, edl_problem
from gmpnp_amd.stern import L_STERN

pytestmark = pytest.mark.gpu
DTHETA = {0: -0.3, 16: 0.2, 17: -0.15, 32: 0.05, 33: -0.04, 48: 0.1}          # mixed signs
DTHETA_BIG = {**DTHETA, 0: -40.0}                                       # with tau = 0.9: a step the limiter has to damp


def rule_direction(z, dtheta):
    """-(dtheta_0 z_0 + dtheta_1 z_1 + ...), left to right, every product and sum rounded on its own."""
    d = np.float64(dtheta[0]) * z[0]
    for k in range(1, len(dtheta)):
        d = d + np.float64(dtheta[k]) * z[k]
    return -d


def rule_update(u, z, dtheta, alpha):
    """u + ((alpha dtheta_0) z_0 + (alpha dtheta_1) z_1 + ...)."""
    a = np.float64(alpha)
    d = (a * np.float64(dtheta[0])) * z[0]
    for k in range(1, len(dtheta)):
        d = d + (a * np.float64(dtheta[k])) * z[k]
    return u + d


def give_options(dev, options):
    stern, kinetics = ft.records_of(options[0], options[1], options[0]["p_electrode"])
    dev.set_stern(stern)
    dev.set_kinetics(kinetics)


def advance_once(dev, twin, q, u, order, dth, tau):
    """One advance from (q's options, u) on ``dev``; returns what the assertions need.  ``twin`` receives the options read back and
    the new state through the setters."""
    dev.set_stern(q.stern)
    dev.set_kinetics(q.kinetics)
    dev.set_state(u, u)
    d = [dth[p] for p in order]
    z = dev.electrode_tangent(order, want_z=True)["z"]
    alpha_ref = 1.0
    if tau != 0.0:
        alpha_ref = dev.step_limit(rule_direction(z, d), tau)[0]
        dev.electrode_tangent(order)
    alpha = dev.parameter_advance(order, d, tau)
    u1 = dev.get_state()
    opts = dev.electrode_options()
    give_options(twin, opts)
    twin.set_state(u1, u)
    same_F = np.array_equal(dev.assemble(True)[0], twin.assemble(True)[0]) and np.array_equal(dev.jacobian_csr().data, twin.jacobian_csr().data)
    return dict(z=z, d=d, alpha=alpha, alpha_ref=alpha_ref, u1=u1, opts=opts, same_F=same_F)


def check_options(q, opts, order, d):
    stern, kin = opts
    want_s, want_k, ok = ft.moved_options(dict(model=q.stern.model, p_electrode=q.stern.p_electrode, lam=q.stern.lam, eps_surface=q.stern.eps_surface),
                                          {"reactions": [dict(k=r.k, alpha=r.alpha, p_eq=r.p_eq, reactant=r.reactant, nu=dict(r.nu)) for r in q.kinetics.reactions],
                                           "p_electrode": q.kinetics.p_electrode}, q.nf - 1, order, d)
    assert ok
    assert stern["p_electrode"] == want_s["p_electrode"] == kin["p_electrode"] and stern["model"] == q.stern.model and stern["eps_surface"] == q.stern.eps_surface
    assert abs(stern["lam"] - want_s["lam"]) <= 2 * np.spacing(want_s["lam"])          # exp of the C library against Python's
    for got, want, rx in zip(kin["reactions"], want_k["reactions"], q.kinetics.reactions):
        assert got["alpha"] == want["alpha"] and abs(got["k"] - want["k"]) <= 2 * np.spacing(want["k"])
        assert got["p_eq"] == rx.p_eq and got["reactant"] == rx.reactant and got["nu"] == {n: v for n, v in rx.nu.items() if v != 0.0}


@pytest.mark.parametrize("name", CASES)
def test_advance_has_the_bits_of_the_rule(name, inputs, gpu_lib):  # noqa: F811
    """Six columns in two orders, dtheta of mixed signs, tau = 0 and 0.9: u afterwards is the NumPy statement of the rule formed from
    z_out, alpha is gmpnp_step_limit's for -d, the options are the moved ones, a twin given them and the new u through the setters
    has F and J bit for bit, and two runs give equal bits."""
    prob, states = inputs[name]
    u = states[0][0]
    q = R.with_inv_dt(prob, 0.0)
    with gpu_lib.DeviceSolver(q) as dev, gpu_lib.DeviceSolver(q) as twin:
        first = {}
        for run_no, order in enumerate((PARAMS, SHUFFLED, PARAMS)):
            for tau, dth in ((0.0, DTHETA), (0.9, DTHETA_BIG)):
                a = advance_once(dev, twin, q, u, order, dth, tau)
                print("%s order %s tau %g: alpha %.6g" % (name, order[:2], tau, a["alpha"]))
                assert a["alpha"] == a["alpha_ref"] and (tau != 0.0 or a["alpha"] == 1.0)
                assert a["u1"].tobytes() == rule_update(u, a["z"], a["d"], a["alpha"]).tobytes(), (name, order, tau)
                check_options(q, a["opts"], order, a["d"])
                assert a["same_F"], (name, order, tau)
                if run_no == 0:
                    first[tau] = a
                elif run_no == 2:                                             # a second run of the same call: equal bits
                    assert a["u1"].tobytes() == first[tau]["u1"].tobytes() and a["alpha"] == first[tau]["alpha"] and a["opts"] == first[tau]["opts"]
        if name == "edl1":
            assert first[0.9]["alpha"] < 1.0                                  # the damped branch was taken


@pytest.mark.parametrize("name", ("uniform65", "edl1"))
@pytest.mark.parametrize("tau,dp", ((0.0, -0.75), (0.9, -40.0)))
def test_one_p_M_column_is_the_electrode_advance(name, tau, dp, inputs, gpu_lib):  # noqa: F811
    """n = 1, param = {0}: u, alpha, the options, F and J of gmpnp_electrode_advance, bit for bit."""
    prob, states = inputs[name]
    u = states[0][0]
    q = R.with_inv_dt(prob, 0.0)
    with gpu_lib.DeviceSolver(q) as dev, gpu_lib.DeviceSolver(q) as twin:
        for d in (dev, twin):
            d.set_state(u, u)
            d.electrode_tangent([48, 0])
        a, b = dev.parameter_advance([0], [dp], tau), twin.electrode_advance(dp, tau)
        assert a == b and dev.get_state().tobytes() == twin.get_state().tobytes() and dev.electrode_options() == twin.electrode_options()
        assert np.array_equal(dev.assemble(True)[0], twin.assemble(True)[0]) and np.array_equal(dev.jacobian_csr().data, twin.jacobian_csr().data)
        assert dev.electrode_options()[0]["p_electrode"] == P_M + dp


def test_ten_columns(gpu_lib):
    """All ten columns of a four-reaction handle (the M = 8 chain plus the M = 2 chain), at tau = 0 and 0.9."""
    from gmpnp_amd.params import edl_parameters
    import hp_reference as H
    ep = edl_parameters(cation="Cs", voltage_multiplier=-10.0)
    prob = R.with_inv_dt(edl_problem(ep, H.uniform_mesh_1d(65), stern=SternLayer("BDM", P_M, L_STERN / ep.L_n), kinetics=four_reactions(ep.species, P_M)), 0.0)
    u = random_state(65, 6, seed=65)[0]
    ten = (48, 19, 0, 16, 35, 17, 18, 32, 33, 34)
    dth = dict(zip(ten, (0.1, -0.2, -0.3, 0.15, 0.02, -0.1, 0.25, -0.03, 0.04, -0.05)))
    with gpu_lib.DeviceSolver(prob) as dev, gpu_lib.DeviceSolver(prob) as twin:
        for tau, dd in ((0.0, dth), (0.9, {**dth, 0: -40.0})):
            a = advance_once(dev, twin, prob, u, ten, dd, tau)
            assert a["alpha"] == a["alpha_ref"] and a["u1"].tobytes() == rule_update(u, a["z"], a["d"], a["alpha"]).tobytes() and a["same_F"]
            check_options(prob, a["opts"], ten, a["d"])


def test_electrode_options(edl_k, gpu_lib):  # noqa: F811
    """Off: (None, None); on: the records that were set; with the galvanostat on p_electrode is the potential it holds."""
    ep, m1 = edl_k
    kin = two_reactions(ep.species, P_M)
    both = edl_problem(ep, m1, stern=SternLayer("BDM", P_M, L_STERN / ep.L_n), kinetics=kin)
    with gpu_lib.DeviceSolver(edl_problem(ep, m1)) as plain, gpu_lib.DeviceSolver(both) as b:
        assert plain.electrode_options() == (None, None)
        u0, un = first_step_state(both)
        b.set_state(u0, un)
        s, k = b.electrode_options()
        assert s == dict(model="BDM", p_electrode=P_M, lam=L_STERN / ep.L_n, eps_surface=both.stern.eps_surface)
        assert k["p_electrode"] == P_M and [r["k"] for r in k["reactions"]] == [r.k for r in kin.reactions] and k["reactions"][0]["reactant"] == "CO2"
        b.set_galvanostat(Galvanostat(2.0 * float(b.kinetics_currents().sum())))
        b.newton_solve(gpu_lib.newton_options({"newton_solver": {"maximum_iterations": 3, "relative_tolerance": 1e-9, "absolute_tolerance": 1e-6}}, dim=1),
                       error_on_nonconvergence=False)
        p = b.galvanostat_report()["p_electrode"]
        s, k = b.electrode_options()
        assert s["p_electrode"] == p == k["p_electrode"] and p != P_M
        u = b.get_state()
        b.electrode_options()
        assert np.array_equal(b.get_state(), u)
        b.set_galvanostat(None)
        assert b.electrode_options()[0]["p_electrode"] == p


def test_refusals(inputs, pore10, edl_k, gpu_lib):  # noqa: F811
    """Every refusal is GMPNP_ERR_INVALID and names the parameter advance; afterwards u, the options and a following
    gmpnp_electrode_advance are those of a twin that never made the refused calls."""
    from gmpnp_amd import dist
    prob, states = inputs["edl1"]
    u = states[0][0]
    q = R.with_inv_dt(prob, 0.0)

    def refused(call):
        with pytest.raises(gpu_lib.GmpnpError, match="parameter advance") as ei:
            call()
        assert ei.value.code == gpu_lib.ERR_INVALID

    with gpu_lib.DeviceSolver(q) as dev, gpu_lib.DeviceSolver(q) as twin:
        for d in (dev, twin):
            d.set_state(u, u)
        refused(lambda: dev.parameter_advance([16], [0.1]))                   # no tangent yet
        for d in (dev, twin):
            d.electrode_tangent([0, 16, 32, 48])
        refused(lambda: dev.parameter_advance([], []))                        # n = 0
        refused(lambda: dev.parameter_advance([0, 16, 32, 48] * 2 + [17, 33, 0], [0.1] * 11))   # n = 11
        refused(lambda: dev.parameter_advance([16, 32, 16], [0.1] * 3))       # repeated
        refused(lambda: dev.parameter_advance([16, 17], [0.1] * 2))           # 17 was not in the tangent call
        refused(lambda: dev.parameter_advance([16, 5], [0.1] * 2))            # no such code
        refused(lambda: dev.parameter_advance([16], [float("nan")]))
        refused(lambda: dev.parameter_advance([16, 32], [0.1, float("inf")]))
        refused(lambda: dev.parameter_advance([16], [0.1], 1.0))
        refused(lambda: dev.parameter_advance([16], [0.1], -0.5))
        refused(lambda: dev.parameter_advance([48], [-800.0]))                # lam would become 0: validated before anything moves
        refused(lambda: dev.parameter_advance([16], [800.0]))                 # k would become Inf
        assert dev.get_state().tobytes() == twin.get_state().tobytes() and dev.electrode_options() == twin.electrode_options()
        assert dev.electrode_advance(-0.75, 0.9) == twin.electrode_advance(-0.75, 0.9)           # the tangent survived every refusal
        assert dev.get_state().tobytes() == twin.get_state().tobytes() and dev.electrode_options() == twin.electrode_options()
        # what invalidates the tangent
        refused(lambda: dev.parameter_advance([16], [0.1]))                   # used up by the electrode advance
        dev.electrode_tangent([16, 48])
        assert dev.parameter_advance([48], [0.1]) == 1.0                      # a call without a p_M column permits its own columns
        refused(lambda: dev.parameter_advance([16], [0.1]))                   # used up by the parameter advance
        dev.electrode_tangent([16, 48])
        with pytest.raises(gpu_lib.GmpnpError, match="electrode tangent"):
            dev.electrode_advance(-0.5)                                       # still refused: no p_M column
        assert dev.parameter_advance([16], [0.1]) == 1.0                      # (that refusal left the tangent)
        for spoil in (lambda: dev.set_state(u, None), lambda: dev.newton_solve(gpu_lib.newton_options(STEADY, dim=1)), lambda: dev.set_kinetics(q.kinetics),
                      lambda: dev.set_stern(q.stern), lambda: dev.set_time_step(0.0)):
            dev.set_stern(q.stern)
            dev.set_kinetics(q.kinetics)
            dev.set_state(u, u)
            dev.electrode_tangent([16])
            spoil()
            refused(lambda: dev.parameter_advance([16], [0.1]))
        # what the tangent itself refuses of a handle
        dev.set_stern(q.stern)
        dev.set_kinetics(q.kinetics)
        dev.set_state(u, u)
        dev.electrode_tangent([16])
        dev.set_galvanostat(Galvanostat(10.0))
        refused(lambda: dev.parameter_advance([16], [0.1]))
        dev.set_galvanostat(None)
    ep, m1 = edl_k
    stern_only = edl_problem(ep, m1, stern=SternLayer("BDM", P_M, L_STERN / ep.L_n))
    with gpu_lib.DeviceSolver(edl_problem(ep, m1)) as plain, gpu_lib.DeviceSolver(stern_only) as c:
        refused(lambda: plain.parameter_advance([48], [0.1]))                 # the Stern option is off
        c.set_state(*[first_step_state(stern_only)[1]] * 2)
        c.electrode_tangent([0, 48])
        refused(lambda: c.parameter_advance([16], [0.1]))                     # a kinetic parameter with the kinetics off: not in the call
        c.set_supg(np.full((m1.num_vertices, 6), 0.1))
        refused(lambda: c.parameter_advance([48], [0.1]))
        c.set_supg(None)
        c.electrode_tangent([0, 48])
        assert c.parameter_advance([48, 0], [0.1, -0.2]) == 1.0 and c.electrode_options()[1] is None
    pp, mesh, prob3, _ = pore10
    dom, perm, part = dist.partition_plan(prob3, 2, 0)
    with gpu_lib.DeviceSolver(dom.problem, perm=perm, partition=part) as partitioned, gpu_lib.DeviceSolver(prob3) as d3:
        refused(lambda: partitioned.parameter_advance([0], [0.1]))
        refused(lambda: d3.parameter_advance([0], [0.1]))                     # 3D, the Stern option off


def test_3d_advance(gpu_lib):
    """L_10_R_5 after two steps of the pore driver (band LU, p_M = -1, Tafel kinetics): six columns in another order at tau = 0 and
    0.9 against the rule, and one p_M column against gmpnp_electrode_advance, bit for bit."""
    from gmpnp_amd.pore3d import SOLVER_PARAMETERS, PoreRun
    from test_gpu_tangent import PORE_TAFEL
    sp = {"nonlinear_solver": "newton", "newton_solver": dict(SOLVER_PARAMETERS["newton_solver"], linear_solver="band_lu")}
    run = PoreRun(num_steps=2, solver_parameters=sp, electrode_voltage=-1.0, L=10e-9, R=5e-9, concentration_elec=0.5, **PORE_TAFEL)
    try:
        run.run(verbose=False)
        dev = run.sys.dev
        u = dev.get_state()
        stern, kinetics = run.problem.stern, run.problem.kinetics
        for tau, scale in ((0.0, 1.0), (0.9, 1.0), (0.9, 5000.0)):
            dev.set_stern(stern)
            dev.set_kinetics(kinetics)
            dev.set_state(u, None)
            d = [scale * 0.1 * DTHETA[p] if p == 0 else 0.1 * DTHETA[p] for p in SHUFFLED]
            z = dev.electrode_tangent(SHUFFLED, want_z=True)["z"]
            alpha_ref = 1.0
            if tau != 0.0:
                alpha_ref = dev.step_limit(rule_direction(z, d), tau)[0]
                dev.electrode_tangent(SHUFFLED)
            alpha = dev.parameter_advance(SHUFFLED, d, tau)
            print("3D tau %g scale %g: alpha %.6g" % (tau, scale, alpha))
            assert alpha == alpha_ref and dev.get_state().tobytes() == rule_update(u, z, d, alpha).tobytes()
            assert (alpha < 1.0) == (scale > 1.0)                            # the last step is one the limiter damps
            s, k = dev.electrode_options()
            assert s["p_electrode"] == -1.0 + d[SHUFFLED.index(0)] == k["p_electrode"] and k["reactions"][1]["alpha"] == kinetics.reactions[1].alpha + d[SHUFFLED.index(33)]
        got = {}
        for which in ("parameter", "electrode"):
            dev.set_stern(stern)
            dev.set_kinetics(kinetics)
            dev.set_state(u, None)
            dev.electrode_tangent([0])
            alpha = dev.parameter_advance([0], [-0.25], 0.9) if which == "parameter" else dev.electrode_advance(-0.25, 0.9)
            got[which] = (alpha, dev.get_state().tobytes(), dev.electrode_options(), dev.assemble(True)[0].tobytes())
        assert got["parameter"] == got["electrode"]
    finally:
        run.sys.close()


# ---- the fit ---------------------------------------------------------------------------------------------------------------------------
KW = dict(L_n=1e-6, cation="K", electrode_voltage=P_M, kinetics="tafel", adaptive_dt=True, steady_tol=1e-5)
TRUE = dict(i0_CO=TAFEL["i0_CO"], i0_H2=TAFEL["i0_H2"], alpha_CO=TAFEL["alpha_CO"], alpha_H2=TAFEL["alpha_H2"], stern_length=4.0e-10)
# |theta - truth| measured on the MI355X: 1.39e-13 (four parameters), 1.41e-13 (without the predictor), 7.6e-15 (five, with the surface
# charge); the bound is 100 x the largest of them (the cap 1e-6 is far above it)
RECOVERY_BOUND = 1.4e-11


def displaced(names):
    kw = dict(TRUE)
    for n in names:
        kw[n] = TRUE[n] * math.exp(FR.DISPLACEMENT[n]) if not n.startswith("alpha") else TRUE[n] + FR.DISPLACEMENT[n]
    return kw


def truth_theta(names):
    return np.array([TRUE[n] if n.startswith("alpha") else math.log(TRUE[n]) for n in names])


def theta_error(out, names):
    """max |theta - truth| in ln i0, alpha and ln stern_length from the fitted physical values."""
    got = np.array([v if n.startswith("alpha") else math.log(v) for n, v in zip(names, out["fitted_values"])])
    return float(np.abs(got - truth_theta(names)).max())


@pytest.fixture(scope="module")
def fits(tmp_path_factory, gpu_lib):
    """The planted curve written by the driver (--polarisation at the planted parameters), then one run at the displaced start that is
    fitted three times from its own steady state there: four parameters, four without the predictor, five with the surface charge
    (the start is put back through the setters and set_state in between).  Then the driver with the fit keyword."""
    from gmpnp_amd import edl1d
    out_dir = tmp_path_factory.mktemp("fit")
    os.environ["GMPNP_OUT"] = str(out_dir)
    res = {}
    try:
        run = edl1d.EDLRun(polarisation=dict(v_end=-10.0, v_step=-1.0), **KW, **{k: TRUE[k] for k in FR.FOUR})
        try:
            run.run(verbose=False)
            res["data_path"] = os.path.join(run.write_outputs(stamp="planted"), "polarisation.npz")
        finally:
            run.sys.close()
        d5 = displaced(FR.FIVE)
        run = edl1d.EDLRun(**KW, **{k: d5[k] for k in FR.FOUR}, stern_length=d5["stern_length"])
        try:
            run.run(verbose=False)
            dev = run.sys.dev
            u5 = dev.get_state()
            stern5, kin5, par5 = run.stern, run.kinetics, dict(run.kinetic_par)

            def start(names):
                """The run back at the displaced start of ``names`` (the others at the truth), near its steady state."""
                import dataclasses
                lam = stern5.lam if "stern_length" in names else TRUE["stern_length"] / run.ep.L_n
                run.stern = dataclasses.replace(stern5, lam=lam)
                run.kinetics, run.kinetic_par = kin5, dict(par5)
                dev.set_stern(run.stern)
                dev.set_kinetics(run.kinetics)
                dev.set_state(u5, u5)

            data = ft.load_data(res["data_path"])
            res["data"] = data
            start(FR.FOUR)
            res["four"] = run.fit({k: v for k, v in data.items() if k != "surface_charge"}, FR.FOUR)
            # the sensitivities at the fitted curve: the fit's Jacobian against differences of re-converged curves
            eps_0 = edl1d._load_yaml(os.path.join(edl1d.utilities_dir(), "parameters.yaml"))["nat_const"]["eps_0"]
            codes = ft.param_codes(FR.FIVE)
            curve = ft.DeviceCurve(run, ft.check_data(data, P_M, 5), codes, eps_0 * run.ep.thermal_voltage / run.ep.L_n)
            inv_dt = float(run.sys.problem.model.inv_dt)
            curve.prepare()
            J, h = curve.kept["J"].copy(), 3e-4
            fd = np.zeros_like(J)
            for k in range(5):
                e = np.zeros(5); e[k] = h
                fd[:, k] = (curve.trial(None, e)["r"] - curve.trial(None, -e)["r"]) / (2 * h)
            curve.finish(P_M, inv_dt)
            res["J"], res["fd"] = J, fd
            start(FR.FOUR)
            res["four_off"] = run.fit({k: v for k, v in data.items() if k != "surface_charge"}, FR.FOUR, predictor=False)
            start(FR.FIVE)
            res["five"] = run.fit(data, FR.FIVE)
            res["after"] = dict(p=run.stern.p_electrode, inv_dt=float(run.sys.problem.model.inv_dt), i0=run.kinetics.reactions[0].k,
                                more=dev.newton_solve(gpu_lib.newton_options(edl1d.POLARISATION_NEWTON, dim=1))["iterations"])
        finally:
            run.sys.close()
        d4 = displaced(FR.FOUR)
        run = edl1d.EDLRun(fit=dict(data=res["data_path"]), polarisation=dict(v_end=-7.0, v_step=-1.0), **KW, **{k: d4[k] for k in FR.FOUR})
        try:
            run.run(verbose=False)
            res["driver_path"] = run.write_outputs(stamp="fitted")
        finally:
            run.sys.close()
        plain = edl1d.EDLRun(**KW, **{k: TRUE[k] for k in FR.FOUR})
        try:
            plain.run(verbose=False)
            res["plain_path"] = plain.write_outputs(stamp="plain")
        finally:
            plain.sys.close()
    finally:
        del os.environ["GMPNP_OUT"]
    return res


def test_fit_jacobian_against_differences_of_reconverged_curves(fits):
    """Every column of the fit's Jacobian (currents and surface charge, five parameters, six potentials) against central differences
    of two re-converged device curves at theta -+ 3e-4: below 1e-6 of the column's largest entry (5l's bound for this comparison)."""
    J, fd = fits["J"], fits["fd"]
    err = np.abs(J - fd).max(axis=0) / np.abs(J).max(axis=0)
    print("Jacobian against differences, per parameter:", err)
    assert J.shape == (18, 5) and err.max() < 1e-6


def test_round_trip_four_parameters(fits):
    """Data from the device at the planted parameters, the start displaced by (0.7, -0.5, 0.08, -0.06): converged, no rejected trial,
    at most 8 trials; |theta - truth| within the bound; without the predictor the same parameters within that bound.

    Measured on the MI355X: |theta - truth| 1.39e-13 with the predictor (4 trials, none rejected, costs 5.3, 7.8e-06, 6.4e-11, 6.1e-18,
    5.8e-27; 37 Newton iterations), 1.41e-13 without it (4 trials, 44 Newton iterations)."""
    on, off = fits["four"], fits["four_off"]
    e_on, e_off = theta_error(on, FR.FOUR), theta_error(off, FR.FOUR)
    print("four parameters: %s, %d trials, %d rejected, costs %s, |theta - truth| %.3e; Newton iterations %d with the predictor, %d without (|theta - truth| %.3e, %d trials)"
          % (on["result"]["stop_reason"], on["result"]["trials"], on["result"]["rejected_trials"], ["%.2g" % c for c in on["history_cost"]], e_on,
             on["result"]["newton_iterations"], off["result"]["newton_iterations"], e_off, off["result"]["trials"]))
    assert on["result"]["stop_reason"] == "converged" and on["result"]["rejected_trials"] == 0 and on["result"]["trials"] <= 8
    assert e_on <= RECOVERY_BOUND
    assert e_off <= RECOVERY_BOUND
    assert np.isfinite(on["standard_errors"]).all() and on["covariance"].shape == (4, 4)


def test_round_trip_five_parameters_with_the_surface_charge(fits):
    five = fits["five"]
    e = theta_error(five, FR.FIVE)
    print("five parameters: %s, %d trials, %d rejected, |theta - truth| %.3e, condition %.3g"
          % (five["result"]["stop_reason"], five["result"]["trials"], five["result"]["rejected_trials"], e, five["result"]["condition_number"]))
    assert five["result"]["stop_reason"] == "converged" and e <= RECOVERY_BOUND
    a = fits["after"]
    assert a["p"] == P_M and a["inv_dt"] > 0.0 and a["more"] <= 1 and abs(a["i0"] - TRUE["i0_CO"]) <= 1e-6 * TRUE["i0_CO"]


def test_driver_fit_data(fits):
    """--fit_data on the polarisation.npz the driver wrote at the planted parameters: fit.npz returns them, the metadata has the fit_*
    keys, the polarisation curve written afterwards is the fitted one; without the keyword the outputs have the parent's keys."""
    path = fits["driver_path"]
    z = np.load(os.path.join(path, "fit.npz"))
    meta = json.load(open(os.path.join(path, "metadata.json")))
    assert list(z["names"]) == list(FR.FOUR) and list(z["codes"]) == [16, 17, 32, 33]
    assert theta_error({"fitted_values": z["fitted_values"]}, FR.FOUR) <= RECOVERY_BOUND
    assert np.allclose(z["initial_values"], [displaced(FR.FOUR)[n] for n in FR.FOUR], rtol=1e-12)
    for key in ("standard_errors", "covariance", "correlation", "singular_values", "residuals", "data_i_CO", "model_i_CO", "data_i_H2", "model_i_H2",
                "history_cost", "history_lambda", "history_accepted", "history_newton_iterations", "history_step", "electrode_voltage"):
        assert key in z.files, key
    assert np.abs(z["model_i_CO"] / z["data_i_CO"] - 1.0).max() <= 1e-6
    assert all(k in meta for k in ft.METADATA_KEYS) and meta["fit_stop_reason"] == "converged" and meta["fit_parameters"] == list(FR.FOUR)
    assert meta["fit_trials"] == len(z["history_cost"]) - 1 and meta["fit_rejected_trials"] == 0
    curve, data = np.load(os.path.join(path, "polarisation.npz")), fits["data"]
    assert np.array_equal(curve["electrode_voltage"], [-5.0, -6.0, -7.0]) and curve["newton_iterations"][0] <= 1     # the run stood at its steady state
    assert np.abs(curve["i_CO"] / data["i_CO"][:3] - 1.0).max() <= 1e-6 and np.abs(curve["i_H2"] / data["i_H2"][:3] - 1.0).max() <= 1e-6
    plain = json.load(open(os.path.join(fits["plain_path"], "metadata.json")))
    assert "fit.npz" not in os.listdir(fits["plain_path"]) and not [k for k in plain if k.startswith("fit_")]
    assert sorted(k for k in meta if not k.startswith(("fit_", "polarisation_"))) == sorted(plain)
    for name in ("arrays_scaled.npz", "arrays_unscaled.npz"):
        assert sorted(np.load(os.path.join(path, name)).files) == sorted(np.load(os.path.join(fits["plain_path"], name)).files)
