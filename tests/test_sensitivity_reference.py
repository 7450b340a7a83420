"""The transient sensitivities on the CPU: J = K + inv_dt M with one M at two inv_dt, the NumPy recursion of
tests/sensitivity_reference.py against central differences of the whole fixed-mode march re-run at theta +- eps (a convergence
ratio, not a tolerance), the ctypes image against the header, the Python refusals, the command line and the unit conversions of
``programme_sensitivity.npz``.  No GPU."""
import ctypes
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import response_reference as R
import sensitivity_reference as S
from conftest import random_state
from gmpnp_amd import programme as P
from gmpnp_amd.polarisation import NEWTON
from test_kinetics_reference import TAFEL
from test_programme_reference import P_M, PULSE_KW, steady_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = (0, 16, 17, 32, 33, 48)                 # offset, ln i0_CO, ln i0_H2, alpha_CO, alpha_H2, ln stern_length
NEWTON_KW = dict(NEWTON["newton_solver"])
# The eps pair of the convergence criterion, chosen on the reference alone: central differences of the march have the truncation error
# O(eps^2) and a noise floor of about (Newton's tolerance) / eps.  Over both meshes, both programmes, both starts and all six
# parameters the deviation falls by 3.7 to 4.6 from 6.4e-2 to 3.2e-2 (truncation dominates); one halving further the weakest column
# (ln i0_H2, triangle, 65 vertices, steady start) falls by 1.4 only (the floor).  Final deviations at 3.2e-2: 1.2e-5 ... 1.4e-2.
EPS_PAIR = (6.4e-2, 3.2e-2)


def programme(kind):
    """A pulse with two jumps and a triangle (scaled time: the reference step of these cases is 9.5)."""
    return P.pulse([-5.5, -4.5, -5.25], [30.0, 20.0, 25.0], 1) if kind == "pulse" else P.triangle(P_M, -6.0, 1.0 / 35.0, 1)


@pytest.fixture(scope="module")
def cases():
    return {nv: steady_case(nv) for nv in (9, 65)}


@pytest.mark.parametrize("nv", [9, 65])
def test_the_jacobian_is_affine_in_inv_dt_with_one_mass_matrix(nv, cases):
    ep, prob, u, inv = cases[nv]
    ur = random_state(nv, 6, seed=nv)[0]
    a, b = inv(9.5), inv(0.37)
    Ma, Mb = S.step_mass(prob, ur, a) / a, S.step_mass(prob, ur, b) / b
    scale = abs(Ma).max()
    assert scale > 0.0 and abs(Ma - Mb).max() <= 1e-12 * scale
    assert abs(Ma - R.mass(prob)).max() <= 1e-12 * scale                    # the consistent P1 mass of the response's restatement
    nf = prob.nf
    rows = np.unique(Ma.tocoo().row[np.abs(Ma.tocoo().data) > 0.0])
    assert not np.any(rows % nf == nf - 1) and not set(rows) & set(int(r) for r in prob.bc_dofs)     # potential and Dirichlet rows: zero
    assert len(rows) == prob.ndof - nv - len([r for r in prob.bc_dofs if r % nf != nf - 1])


def deviation(A, S_end, fd, du, k):
    """The largest deviation of column k's records and final S from the differences, each relative to the largest value of its
    quantity: dD, dI and d_dD_dt over all steps, dQ and dQ_D of the last record (the combine step's derivative), the final S."""
    nr = 2
    return max(np.abs(fd["D"] - A["dD"][:, k]).max() / np.abs(A["dD"][:, k]).max(),
               np.abs(fd["I"][:, :nr] - A["dI"][:, k, :nr]).max() / np.abs(A["dI"][:, k, :nr]).max(),
               np.abs(fd["dD_dt"] - A["d_dD_dt"][:, k]).max() / np.abs(A["d_dD_dt"][:, k]).max(),
               np.abs(fd["Q"][-1, :nr] - A["dQ"][-1, k, :nr]).max() / np.abs(A["dQ"][-1, k, :nr]).max(),
               abs(fd["Q_D"][-1] - A["dQ_D"][-1, k]) / abs(A["dQ_D"][-1, k]),
               np.abs(fd["p_boundary"] - A["dp_boundary"][:, k]).max() / np.abs(A["dp_boundary"][:, k]).max(),
               np.abs(du - S_end[k]).max() / np.abs(S_end[k]).max())


@pytest.mark.parametrize("start", ["steady", "zero"])
@pytest.mark.parametrize("kind", ["pulse", "triangle"])
@pytest.mark.parametrize("nv", [9, 65])
def test_recursion_against_central_differences_of_the_march(nv, kind, start, cases):
    """"steady": the re-run re-converges the steady start at theta +- eps; "zero": it marches from the frozen state."""
    ep, prob, u, inv = cases[nv]
    segs = programme(kind)
    ref = S.NumpySensitivitySystem(prob, u, inv, PARAMS, start=start, newton=NEWTON_KW)
    P.run_programme(ref, segs, steps_per_segment=4)
    A = ref.sensitivity_arrays()
    assert A["dD"].shape == (4 * len(segs), len(PARAMS))
    for k, q in enumerate(PARAMS):
        d = [deviation(A, ref.S, *S.central_difference(prob, u, inv, segs, q, eps, start, newton=NEWTON_KW), k) for eps in EPS_PAIR]
        print("%d vertices, %s, %s, parameter %d: deviation %.2e at eps %.1e, %.2e at %.1e (ratio %.2f)"
              % (nv, kind, start, q, d[0], EPS_PAIR[0], d[1], EPS_PAIR[1], d[0] / d[1]))
        assert d[0] / d[1] > 3.0, (q, d)


def test_zero_start_takes_the_explicit_derivative_as_dD_prev(cases):
    """From S = 0 the first record's d_dD_dt is (dD_1 - dD/dtheta at the frozen start) / h, not dD_1 / h."""
    import tangent_reference as T
    ep, prob, u, inv = cases[9]
    ref = S.NumpySensitivitySystem(prob, u, inv, PARAMS, start="zero", newton=NEWTON_KW)
    first = [T.explicit(prob, u, q)[0] for q in PARAMS]
    assert [a["D_prev"] for a in ref.sacc] == pytest.approx(first, rel=1e-12) and first[0] != 0.0 and first[5] != 0.0 and first[1] == 0.0
    P.run_programme(ref, programme("pulse"), steps_per_segment=1)
    r = ref.srecords[0]
    for k in range(len(PARAMS)):
        assert r[k]["d_dD_dt"] == (r[k]["dD"] - first[k]) / r[k]["h"] or abs(r[k]["d_dD_dt"] - (r[k]["dD"] - first[k]) / r[k]["h"]) <= 1e-12 * abs(r[k]["d_dD_dt"])


# ---- the fit to transients over the NumPy system ---------------------------------------------------------------------------------------
# The bound tests/test_fit_reference.py puts on the steady fit's recovery, |theta - truth| <= 1e-9, measured first on the reference
# alone: the transient fit meets it (figures in DESIGN.md section 5p), so it is reused as it is.
RECOVERY_BOUND = 1e-9
TIME_CONSTANT = 2.0e-6


def transient_fit(cases, names, surface_charge):
    import fit_reference as FR
    from gmpnp_amd import fit as ft
    ep, prob, u, inv = cases[9]
    codes = ft.param_codes(names)
    segs = programme("pulse")
    truth = PR_system(prob, u, inv)
    P.run_programme(truth, segs, steps_per_segment=4)
    rec = truth.arrays()
    data = {"time_s": rec["t"] * TIME_CONSTANT, "i_CO": rec["I"][:, 0], "i_H2": rec["I"][:, 1]}
    if surface_charge:
        data["surface_charge"] = rec["D"].copy()
    table = ft.check_programme_data(data, len(codes))
    start = FR.moved(prob, codes, [FR.DISPLACEMENT[n] for n in names])
    system = S.NumpyTransient(start, u, inv, segs, 4, codes, time_constant=TIME_CONSTANT, newton=NEWTON_KW)
    curve = ft.TransientCurve(system, table, len(codes))
    res = ft.LevenbergMarquardt(curve, [ft.is_log(c) for c in codes]).run(FR.theta_of(start, codes))
    return res, FR.theta_of(prob, codes), FR.theta_of(system.kept["prob"], codes), system


def PR_system(prob, u, inv):
    import programme_reference as PR
    return PR.NumpyProgrammeSystem(prob, u, inv, newton=NEWTON_KW)


@pytest.mark.parametrize("names,surface_charge", [(("i0_CO", "i0_H2", "alpha_CO", "alpha_H2"), False),
                                                  (("i0_CO", "i0_H2", "alpha_CO", "alpha_H2", "stern_length"), True)])
def test_transient_fit_round_trip(names, surface_charge, cases):
    """Data synthesised at the truth (a pulse with two jumps, every step), the start displaced by ``fit_reference.DISPLACEMENT``: four
    parameters from the currents alone, five with the surface charge."""
    res, truth, kept, system = transient_fit(cases, names, surface_charge)
    err = float(np.abs(res["theta"] - truth).max())
    print("transient fit of %d parameters: %s, %d trials, %d rejected, %d marches, cost %.2g, |theta - truth| %.2e, condition %.3g"
          % (len(names), res["stop_reason"], res["trials"], res["rejected_trials"], system.marches, res["cost"], err, res["condition_number"]))
    assert res["stop_reason"] == "converged"
    assert err <= RECOVERY_BOUND
    assert np.array_equal(kept, res["theta"]) or np.abs(kept - res["theta"]).max() <= 1e-14       # what the system keeps is what the rule reports


def test_a_trial_that_is_not_accepted_leaves_nothing_behind(cases):
    import fit_reference as FR
    from gmpnp_amd import fit as ft
    ep, prob, u, inv = cases[9]
    codes = ft.param_codes(("i0_CO", "alpha_CO"))
    segs = programme("pulse")
    truth = PR_system(prob, u, inv)
    P.run_programme(truth, segs, steps_per_segment=1)
    rec = truth.arrays()
    table = ft.check_programme_data({"time_s": rec["t"], "i_CO": rec["I"][:, 0], "i_H2": rec["I"][:, 1]}, 2)
    system = S.NumpyTransient(prob, u, inv, segs, 1, codes, newton=NEWTON_KW)
    curve = ft.TransientCurve(system, table, 2)
    first = curve.trial(None, np.zeros(2))
    curve.accept()
    kept_prob, kept_u = system.kept["prob"], system.kept["u"].copy()
    assert np.abs(first["r"]).max() <= 1e-9                                          # the data are the model's own
    t = curve.trial(None, np.array([0.3, -0.05]))
    assert t is not None and np.abs(t["r"]).max() > 1e-3
    assert system.kept["prob"] is kept_prob and np.array_equal(system.kept["u"], kept_u) and curve.kept is first
    again = curve.trial(None, np.array([0.3, -0.05]))                                # the same trial from the same kept start: equal bits
    assert np.array_equal(again["r"], t["r"]) and np.array_equal(again["J"], t["J"])
    curve.accept()
    assert system.kept["prob"] is not kept_prob and FR.theta_of(system.kept["prob"], codes)[1] == pytest.approx(FR.theta_of(prob, codes)[1] - 0.05)


def test_data_times_must_be_step_ends(cases, tmp_path):
    from gmpnp_amd import fit as ft
    steps = np.array(P.fixed_step_times(programme("pulse"), 4)) * TIME_CONSTANT
    assert len(steps) == 12 and steps[3] == 30.0 * TIME_CONSTANT                    # landed on the breakpoint itself
    assert list(ft.match_times(steps[[2, 0, 11]], steps)) == [2, 0, 11]
    assert list(ft.match_times(steps[[5]] * (1.0 + 5e-10), steps)) == [5]           # inside the relative 1e-9
    bad = np.array([steps[1], steps[4] * (1.0 + 1e-8), 0.5 * (steps[6] + steps[7])])
    with pytest.raises(ValueError, match="fit_programme") as ei:
        ft.match_times(bad, steps)
    assert "%.17g" % bad[1] in str(ei.value) and "%.17g" % bad[2] not in str(ei.value)    # the FIRST time that is no step end
    # the data: what programme.npz holds is accepted as it is, other keys are not read
    np.savez(tmp_path / "programme.npz", time_s=steps, i_CO=np.ones(12), i_H2=np.ones(12), surface_charge=-np.ones(12), FE_H2=np.zeros(12))
    raw = ft.load_programme_data(tmp_path / "programme.npz")
    assert sorted(raw) == ["i_CO", "i_H2", "surface_charge", "time_s"]
    table = ft.check_programme_data(raw, 5)
    assert table["quantities"] == ("i_CO", "i_H2", "surface_charge") and np.array_equal(table["weight_i_CO"], np.ones(12))
    for broken in (dict(i_CO=np.ones(12)), dict(time_s=steps), dict(time_s=steps, i_CO=-np.ones(12)), dict(time_s=steps[:2], i_CO=np.ones(3)),
                   dict(time_s=np.r_[steps[:2], steps[:1]], i_CO=np.ones(3)), dict(time_s=steps[:1], i_CO=np.ones(1))):
        with pytest.raises(ValueError, match="fit_programme"):
            ft.check_programme_data(broken, 2)


def test_ctypes_image_has_the_layout_of_the_header(tmp_path):
    from gmpnp_amd import backend
    fields = ("t", "h", "param", "dD", "d_dD_dt", "dI", "dQ", "dQ_D", "dp_boundary", "residual", "status")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gmpnp.h"\nint main(void){printf("%zu", sizeof(gmpnp_sensitivity_record_t));\n'
                   + "".join('printf(" %%zu", offsetof(gmpnp_sensitivity_record_t,%s));\n' % f for f in fields) + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    C = backend.CSensitivityRecord
    assert got == [ctypes.sizeof(C)] + [getattr(C, f).offset for f in fields]
    dt = backend.SENSITIVITY_RECORD_DTYPE
    assert dt.itemsize == ctypes.sizeof(C) and [dt.fields[f][1] for f in fields] == got[1:]
    for name in ("gmpnp_sensitivity_open", "gmpnp_sensitivity_step", "gmpnp_sensitivity_read", "gmpnp_sensitivity_columns", "gmpnp_sensitivity_close"):
        assert name in backend.EXPORTS
    assert backend.SENSITIVITY_START == {"zero": 0, "steady": 1, "continue": 2}


def test_python_refusals():
    """Every refusal is a ValueError that names the programme, raised before anything touches the device (no GPU here)."""
    from gmpnp_amd import edl1d
    t = dict(electrode_voltage=-5.0, kinetics="tafel", i0_CO=TAFEL["i0_CO"], i0_H2=TAFEL["i0_H2"])
    s = dict(sensitivities=("i0_CO", "offset"))
    calls = {
        "unknown name": lambda: edl1d.EDLRun(programme=dict(PULSE_KW, sensitivities=("i0_CO", "k_CO")), **t),
        "repeated name": lambda: edl1d.EDLRun(programme=dict(PULSE_KW, sensitivities=("i0_CO", "i0_CO")), **t),
        "eleven names": lambda: P.sensitivity_codes(["offset"] * 11),
        "bad start": lambda: edl1d.EDLRun(programme=dict(PULSE_KW, sensitivity_start="warm", **s), **t),
        "start without names": lambda: edl1d.EDLRun(programme=dict(PULSE_KW, sensitivity_start="zero"), **t),
        "kinetic parameter without kinetics": lambda: edl1d.EDLRun(electrode_voltage=-5.0, programme=dict(PULSE_KW, **s)),
        # every combination the programme already refuses stays refused with the option on
        "target_current": lambda: edl1d.EDLRun(target_current=10.0, programme=dict(PULSE_KW, **s), **t),
        "polarisation": lambda: edl1d.EDLRun(polarisation=dict(v_end=-10.0, v_step=-1.0), programme=dict(PULSE_KW, **s), **t),
        "dt_order": lambda: edl1d.EDLRun(adaptive_dt=True, dt_order=2, programme=dict(PULSE_KW, **s), **t),
        "flags without --programme": lambda: edl1d.main(["--electrode_voltage", "-5", "--programme_sensitivities", "i0_CO"]),
    }
    fixed = dict(PULSE_KW, steps_per_segment=4)
    fp = dict(fit_programme=dict(data="no_such_file.npz"))
    calls.update({
        "fit_programme without a programme": lambda: edl1d.EDLRun(**fp, **t),
        "fit_programme in adaptive mode": lambda: edl1d.EDLRun(programme=dict(PULSE_KW), **fp, **t),
        "fit_programme with fit": lambda: edl1d.EDLRun(programme=fixed, fit=dict(data="no_such_file.npz"), **fp, **t),
        "fit_programme with polarisation": lambda: edl1d.EDLRun(programme=fixed, polarisation=dict(v_end=-10.0, v_step=-1.0), **fp, **t),
        "fit_programme without kinetics": lambda: edl1d.EDLRun(electrode_voltage=-5.0, programme=fixed, **fp),
        "fit_programme with an unknown name": lambda: edl1d.EDLRun(programme=fixed, fit_programme=dict(data="x.npz", params=("k_CO",)), **t),
        "fit_programme with an unknown field": lambda: edl1d.EDLRun(programme=fixed, fit_programme=dict(data="x.npz", predictor=False), **t),
        "fit_programme with the programme's own sensitivities": lambda: edl1d.EDLRun(programme=dict(fixed, **s), **fp, **t),
        "fit_programme with target_current": lambda: edl1d.EDLRun(target_current=10.0, programme=fixed, **fp, **t),
        "fit_programme with dt_order 2": lambda: edl1d.EDLRun(adaptive_dt=True, dt_order=2, programme=fixed, **fp, **t),
    })
    for name, call in calls.items():
        with pytest.raises(ValueError, match="programme"):
            call()
    assert P.sensitivity_codes(("i0_CO", "i0_H2", "alpha_CO", "alpha_H2", "stern_length", "offset")) == [16, 17, 32, 33, 48, 0]
    ok = P.check_programme(dict(PULSE_KW, sensitivity_start="zero", **s), dict(t))
    assert ok["sensitivities"] == ("i0_CO", "offset")
    assert P.check_programme(dict(PULSE_KW, sensitivities=("offset", "stern_length")), dict(electrode_voltage=-5.0))     # no kinetics needed


def test_command_line():
    from gmpnp_amd import edl1d, edl_sweep, pore3d, rxndiff1d, rxnpore3d
    a = edl1d.build_parser().parse_args([])
    assert a.programme_sensitivities is None and a.programme_sensitivity_start is None and P.programme_keywords(a) == {}
    a = edl1d.build_parser().parse_args(["--programme", "triangle", "--v_vertex", "-9", "--scan_rate", "0.1", "--programme_sensitivities", "i0_CO",
                                         "offset", "--programme_sensitivity_start", "zero"])
    assert P.programme_keywords(a) == {"programme": dict(kind="triangle", v_vertex=-9.0, scan_rate=0.1, cycles=1, sensitivities=["i0_CO", "offset"],
                                                         sensitivity_start="zero")}
    a = edl1d.build_parser().parse_args(["--programme", "triangle", "--v_vertex", "-9", "--scan_rate", "0.1"])
    assert "sensitivities" not in P.programme_keywords(a)["programme"]
    with pytest.raises(SystemExit):
        edl1d.build_parser().parse_args(["--programme_sensitivity_start", "warm"])
    from gmpnp_amd import fit as ft
    a = edl1d.build_parser().parse_args(["--fit_programme_data", "d.npz", "--fit_params", "i0_CO", "stern_length"])
    assert ft.programme_fit_keywords(a) == {"fit_programme": dict(data="d.npz", params=("i0_CO", "stern_length"))} and ft.fit_keywords(a) == {}
    a = edl1d.build_parser().parse_args(["--fit_programme_data", "d.npz"])
    assert ft.programme_fit_keywords(a) == {"fit_programme": dict(data="d.npz")}
    assert ft.programme_fit_keywords(edl1d.build_parser().parse_args([])) == {}
    for mod in (pore3d, rxndiff1d, rxnpore3d, edl_sweep):            # the other drivers' parsers do not know the flags
        for flag in (["--programme_sensitivities", "i0_CO"], ["--fit_programme_data", "d.npz"]):
            with pytest.raises(SystemExit):
                mod.build_parser().parse_args(flag)


def test_sensitivity_arrays_units_and_signs():
    """programme_sensitivity.npz from a hand-made record: the factors of ``output_arrays``, per volt for the offset."""
    from gmpnp_amd import backend
    ep = SimpleNamespace(thermal_voltage=0.025, time_constant=2e-6, L_n=1e-6)
    eps_0 = 8.8e-12
    names, codes = ("i0_CO", "offset"), [16, 0]
    rec = np.zeros((3, 2), dtype=backend.SENSITIVITY_RECORD_DTYPE)
    rec["t"], rec["h"], rec["param"] = np.array([1.0, 2.0, 3.0])[:, None], 1.0, np.array(codes)[None, :]
    rec["dD"] = [[-1.0, -4.0], [-2.0, -4.0], [-4.0, -5.0]]
    accs = [P.fresh_accumulators(-1.0), P.fresh_accumulators(-4.0)]
    for n in range(3):
        for k in range(2):
            rec["dI"][n, k, :2] = (1.0 + n + k, 0.5)
            rec["d_dD_dt"][n, k] = P.electrode_record_combine(accs[k], 1.0, rec["dD"][n, k], rec["dI"][n, k])
            rec["dQ"][n, k], rec["dQ_D"][n, k] = accs[k]["Q"], accs[k]["Q_D"]
    rec["dp_boundary"] = 0.5
    out = P.sensitivity_arrays(ep, eps_0, rec, names, codes)
    assert sorted(out) == sorted(P.SENSITIVITY_KEYS + ("time_s", "parameters", "status"))
    q, per = eps_0 * 0.025 / 1e-6, np.array([1.0, 1.0 / 0.025])
    assert np.array_equal(out["time_s"], np.array([1.0, 2.0, 3.0]) * 2e-6) and list(out["parameters"]) == list(names) and not out["status"].any()
    assert np.allclose(out["d_i_CO"], rec["dI"][:, :, 0] * per) and np.allclose(out["d_i_H2"], 0.5 * per * np.ones((3, 2)))
    assert np.allclose(out["d_surface_charge"], q * rec["dD"] * per)
    assert np.allclose(out["d_i_charging"][:, 0], [0.0, q / 2e-6, 2.0 * q / 2e-6])                    # -d(d_surface_charge)/dt
    assert np.allclose(out["d_i_charging"][1:], -np.diff(out["d_surface_charge"], axis=0) / 2e-6)
    assert np.allclose(out["d_charge_double_layer"], -(out["d_surface_charge"] - out["d_surface_charge"][0] + q * (rec["dD"][0] - [-1.0, -4.0]) * per))
    assert np.allclose(out["d_charge_CO"], np.cumsum(out["d_i_CO"], axis=0) * 2e-6) and np.allclose(out["d_charge_H2"], np.cumsum(out["d_i_H2"], axis=0) * 2e-6)
    assert np.allclose(out["d_potential_OHP"], 0.5 * 0.025 * per * np.ones((3, 2)))
