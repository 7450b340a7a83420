"""The fit of the electrode kinetics on the CPU: the Levenberg-Marquardt rule over scripted models, the reference
fit over the NumPy restatement of the tangent (tests/fit_reference.py; K+ on the 1 um mesh, Stern BDM, the TAFEL parameters, data = the
model's own currents at p_M = -5 ... -10, the start displaced by (0.7, -0.5, 0.08, -0.06) and 0.2 in ln lam), the data format and every
refusal, the command line, the ctypes images against the header, the metadata keys, and the host rule of a moved parameter (g++ alone)
against its Python statement."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import fit_reference as FR
import kinetics_reference as K
import tangent_reference as T
from gmpnp_amd import fit as ft
from step_limit_reference import first_step_state
from test_kinetics_reference import TAFEL, _edl_k, first_step_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_M = -5.0


# ---- the rule over scripted models ---------------------------------------------------------------------------------------------------
TRUTH = np.array([np.log(0.1), np.log(0.02), 0.5, 0.45])
START = TRUTH + np.array([0.7, -0.5, 0.08, -0.06])
LOGS = [True, True, False, False]


def test_rule_recovers_an_analytic_tafel_law():
    ev = FR.Scripted(FR.tafel_law(FR.POTENTIALS, TRUTH))
    res = ft.LevenbergMarquardt(ev, LOGS).run(START)
    assert res["stop_reason"] == "converged" and res["rejected_trials"] == 0
    assert np.abs(res["theta"] - TRUTH).max() <= 1e-12
    assert np.array_equal(ev.kept_theta, res["theta"])
    assert [h["accepted"] for h in res["history"]] == [True] * (res["trials"] + 1) and res["newton_iterations"] == res["trials"] + 1
    lams = [h["lam"] for h in res["history"]]
    assert lams[1] == 1e-3 and all(b == max(a / 10.0, 1e-12) for a, b in zip(lams[1:], lams[2:]))
    # N > n: the covariance is s^2 (J^T J)^-1, here with s^2 = |r|^2 / 8 ~ 0
    J = res["jacobian"]
    s2 = float(res["residuals"] @ res["residuals"]) / (12 - 4)
    assert np.allclose(res["covariance"], s2 * np.linalg.inv(J.T @ J), rtol=1e-12, atol=0.0)
    assert res["singular_values"].shape == (4,) and res["condition_number"] == res["singular_values"][0] / res["singular_values"][-1]


def test_a_failing_trial_is_rejected_and_lambda_grows_tenfold():
    """The first two trials fail (scripted), the third is evaluated: lambda 1e-3, 1e-2, 1e-1, nothing kept moves meanwhile."""
    count = {"n": 0}

    def fail(theta):
        count["n"] += 1
        return count["n"] in (2, 3)          # (call 1 is the start)
    ev = FR.Scripted(FR.tafel_law(FR.POTENTIALS, TRUTH), fail)
    res = ft.LevenbergMarquardt(ev, LOGS).run(START)
    h = res["history"]
    assert [x["accepted"] for x in h[:4]] == [True, False, False, True]
    assert [x["lam"] for x in h[1:4]] == [1e-3, 1e-2, 1e-1] and np.isnan(h[1]["cost"])
    assert all(np.array_equal(t[0], START) for t in ev.trials[:4])            # every rejected trial started from the kept parameters
    assert res["stop_reason"] == "converged" and res["rejected_trials"] == 2 and np.abs(res["theta"] - TRUTH).max() <= 1e-12


def test_the_step_cap_holds():
    """From a start 9 away in ln k and 1.5 in alpha no log parameter moves by more than 2 and no alpha by more than 0.25 per trial, and
    the direction is kept (the step is scaled as a whole)."""
    far = TRUTH + np.array([9.0, -7.0, 1.5, -0.9])
    ev = FR.Scripted(FR.tafel_law(FR.POTENTIALS, TRUTH))
    res = ft.LevenbergMarquardt(ev, LOGS).run(far)
    deltas = np.array([t[1] for t in ev.trials[1:]])
    assert np.abs(deltas[:, :2]).max() <= 2.0 * (1 + 1e-15) and np.abs(deltas[:, 2:]).max() <= 0.25 * (1 + 1e-15)
    capped = max(np.abs(deltas[0, :2]).max() / 2.0, np.abs(deltas[0, 2:]).max() / 0.25)
    assert abs(capped - 1.0) <= 1e-15                                          # the first step hits a cap exactly
    lm = ft.LevenbergMarquardt(ev, LOGS)
    raw = np.array([8.0, -1.0, 0.5, 0.1])
    assert np.allclose(lm.capped(raw), raw * 0.25, rtol=1e-15) and np.array_equal(lm.capped(raw * 0.01), raw * 0.01)
    assert res["stop_reason"] == "converged" and np.abs(res["theta"] - TRUTH).max() <= 1e-12


def test_one_potential_is_rank_deficient_and_nothing_moves():
    ev = FR.Scripted(FR.tafel_law([-5.0], TRUTH))
    res = ft.LevenbergMarquardt(ev, LOGS).run(START)
    assert res["stop_reason"] == "rank_deficient" and res["trials"] == 0 and len(ev.trials) == 1
    assert np.array_equal(res["theta"], START) and np.isnan(res["covariance"]).all() and np.isnan(res["standard_errors"]).all()


def test_stalled_and_max_iterations_are_reachable():
    always = FR.Scripted(FR.tafel_law(FR.POTENTIALS, TRUTH), fail=lambda th: not np.array_equal(th, START))
    res = ft.LevenbergMarquardt(always, LOGS).run(START)
    lam, want = 1e-3, 0
    while not lam > 1e8:                                                       # the rule's own arithmetic: tenfold per rejected trial
        lam, want = lam * 10.0, want + 1
    assert res["stop_reason"] == "stalled" and res["rejected_trials"] == res["trials"] == want and want in (11, 12)
    assert np.array_equal(res["theta"], START)

    def creeping(theta):      # a model whose steps stay long: r = exp(-theta) never reaches zero
        return np.array([np.exp(-theta[0])]), np.array([[-np.exp(-theta[0])]])
    res = ft.LevenbergMarquardt(FR.Scripted(creeping), [False], max_trials=50).run([0.0])
    assert res["stop_reason"] == "max_iterations" and res["trials"] == 50


# ---- the reference fit ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    """(problem at the planted parameters, its steady state at -5, the data with the surface charge), computed once."""
    ep, mesh = _edl_k()
    prob = first_step_problem(ep, mesh, P_M)
    u1, st = K.newton_loop(prob, *first_step_state(prob))
    assert st.converged
    u, _, ok = T.steady_state(prob, u1)
    assert ok
    u.setflags(write=False)
    data = FR.planted_data(prob, u, surface_charge=True)
    return prob, u, data


def reference_fit(planted, names, data, predictor=True):
    prob, u, _ = planted
    codes = ft.param_codes(names)
    start = FR.moved(prob, codes, [FR.DISPLACEMENT[n] for n in names])
    table = ft.check_data(data, P_M, len(codes))
    ev = FR.NumpyCurve(start, u, table, codes, predictor)
    res = ft.LevenbergMarquardt(ev, [ft.is_log(c) for c in codes]).run(FR.theta_of(start, codes))
    return res, FR.theta_of(prob, codes), ev


def currents_only(data):
    return {k: v for k, v in data.items() if k != "surface_charge"}


def test_reference_fit_four_parameters(planted):
    res, truth, _ = reference_fit(planted, FR.FOUR, currents_only(planted[2]))
    err = float(np.abs(res["theta"] - truth).max())
    print("four parameters: %d trials, %d rejected, costs %s, |theta - truth| %.2e, condition %.3g"
          % (res["trials"], res["rejected_trials"], ["%.2g" % h["cost"] for h in res["history"]], err, res["condition_number"]))
    assert res["stop_reason"] == "converged" and res["trials"] <= 8 and res["rejected_trials"] == 0
    assert err <= 1e-9


def test_reference_fit_five_parameters(planted):
    res, truth, _ = reference_fit(planted, FR.FIVE, currents_only(planted[2]))
    err = float(np.abs(res["theta"] - truth).max())
    print("five parameters: %d trials, %d rejected, cost %.2g, |theta - truth| %.2e, condition %.3g"
          % (res["trials"], res["rejected_trials"], res["cost"], err, res["condition_number"]))
    assert res["stop_reason"] == "converged" and res["trials"] <= 20
    assert err <= 1e-9


def test_reference_fit_with_noise(planted):
    """1 % log-normal noise (seed 1): every estimate within 3 reported standard errors of the truth; the covariance is
    s^2 (J^T J)^-1 recomputed here."""
    rng = np.random.default_rng(1)
    data = currents_only(planted[2])
    noisy = dict(data, i_CO=data["i_CO"] * np.exp(0.01 * rng.standard_normal(6)), i_H2=data["i_H2"] * np.exp(0.01 * rng.standard_normal(6)))
    res, truth, _ = reference_fit(planted, FR.FOUR, noisy)
    t = np.abs(res["theta"] - truth) / res["standard_errors"]
    print("noise: %s, estimates off by %s standard errors" % (res["stop_reason"], t))
    assert res["stop_reason"] in ("converged", "stalled") and t.max() <= 3.0
    J, r = res["jacobian"], res["residuals"]
    cov = float(r @ r) / (12 - 4) * np.linalg.inv(J.T @ J)
    assert np.allclose(res["covariance"], cov, rtol=1e-10, atol=0.0)
    assert np.allclose(res["correlation"], cov / np.sqrt(np.outer(np.diag(cov), np.diag(cov))), rtol=1e-10) and np.allclose(np.diag(res["correlation"]), 1.0)


# ---- data, refusals, command line, images ---------------------------------------------------------------------------------------------
def test_data_loading_and_ordering(tmp_path):
    V = np.array([-8.0, -5.0, -10.0, -6.0])
    cols = dict(electrode_voltage=V, i_CO=np.array([4.0, 1.0, 5.0, 2.0]), i_H2=np.array([0.4, 0.1, 0.5, 0.2]), surface_charge=np.array([-4.0, -1.0, -5.0, -2.0]),
                weight_i_CO=np.array([1.0, 2.0, 3.0, 4.0]))
    np.savez(tmp_path / "d.npz", FE_H2=np.zeros(4), **cols)                                     # other keys are not read
    with open(tmp_path / "d.csv", "w") as fh:
        fh.write(",".join(cols) + ",comment\n")
        for k in range(4):
            fh.write(",".join(repr(float(cols[c][k])) for c in cols) + ",0\n")
    for name in ("d.npz", "d.csv"):
        raw = ft.load_data(tmp_path / name)
        assert sorted(raw) == sorted(cols)
        d = ft.check_data(raw, -5.0, 4)
        assert d["quantities"] == ("i_CO", "i_H2", "surface_charge")
        assert d["electrode_voltage"].tolist() == [-5.0, -6.0, -8.0, -10.0] and d["i_CO"].tolist() == [1.0, 2.0, 4.0, 5.0]
        assert d["weight_i_CO"].tolist() == [2.0, 4.0, 1.0, 3.0] and d["weight_i_H2"].tolist() == [1.0] * 4
    r, J = ft.residual_rows(d, 1, {"i_CO": 2.0 * np.e, "i_H2": 0.2, "surface_charge": -3.0}, {"i_CO": np.array([1.0, 2.0]), "i_H2": np.zeros(2), "surface_charge": np.array([5.0, 0.0])})
    assert np.allclose(r, [4.0 * 1.0, 0.0, (-3.0 + 2.0) / 5.0], rtol=1e-15, atol=1e-16)
    assert np.allclose(J, [[4.0 / (2.0 * np.e), 8.0 / (2.0 * np.e)], [0.0, 0.0], [1.0, 0.0]], rtol=1e-15)


def test_data_refusals():
    good = dict(electrode_voltage=np.array([-5.0, -6.0, -7.0]), i_CO=np.array([1.0, 2.0, 3.0]), i_H2=np.array([0.1, 0.2, 0.3]))
    ft.check_data(good, -5.0, 4)
    ft.check_data(good, -4.0, 4)
    bad = {
        "not finite": dict(good, i_CO=np.array([1.0, np.nan, 3.0])),
        "infinite potential": dict(good, electrode_voltage=np.array([-5.0, -np.inf, -7.0])),
        "a current <= 0": dict(good, i_H2=np.array([0.1, 0.0, 0.3])),
        "repeated": dict(good, electrode_voltage=np.array([-5.0, -6.0, -6.0])),
        "weights": dict(good, weight_i_CO=np.array([1.0, np.inf, 1.0])),
        "lengths": dict(good, i_CO=np.array([1.0, 2.0])),
        "no currents": dict(electrode_voltage=good["electrode_voltage"], surface_charge=np.ones(3)),
        "no potentials": dict(i_CO=good["i_CO"]),
    }
    for name, d in bad.items():
        with pytest.raises(ValueError, match="fit"):
            ft.check_data(d, -5.0, 4)
    with pytest.raises(ValueError, match="fit.*one side"):
        ft.check_data(good, -6.0, 4)                                      # potentials on both sides of electrode_voltage
    with pytest.raises(ValueError, match="fit.*fewer"):
        ft.check_data({k: v[:2] for k, v in good.items()}, -5.0, 5)       # 4 residuals, 5 parameters
    for names in ((), ("i0_CO", "i0_CO"), ("p_eq_CO",), ("i0_CO", "k_2")):
        with pytest.raises(ValueError, match="fit"):
            ft.param_codes(names)
    assert ft.param_codes(FR.FIVE) == (16, 17, 32, 33, 48) and ft.DEFAULT_PARAMS == FR.FOUR


def test_python_refusals():
    """Every refusal is a ValueError that names the fit, raised before anything touches the device (no GPU here)."""
    from gmpnp_amd import edl1d, edl_ensemble, edl_sweep, pore3d, pore_ensemble, rxndiff1d, rxnpore3d, sweep
    t = dict(kinetics="tafel", i0_CO=TAFEL["i0_CO"], i0_H2=TAFEL["i0_H2"])
    c = dict(fit=dict(data="no_such_file.npz"))
    calls = {
        "no electrode voltage": lambda: edl1d.EDLRun(**c),
        "kinetics off": lambda: edl1d.EDLRun(electrode_voltage=-5.0, **c),
        "target_current": lambda: edl1d.EDLRun(electrode_voltage=-5.0, target_current=10.0, **t, **c),
        "stabilization": lambda: edl1d.EDLRun(electrode_voltage=-5.0, stabilization="Y", model="PNP", **c),
        "H_OHP": lambda: edl1d.EDLRun(electrode_voltage=-5.0, H_OHP=0.5, **t, **c),
        "dt_order": lambda: edl1d.EDLRun(electrode_voltage=-5.0, adaptive_dt=True, dt_order=2, **t, **c),
        "unknown name": lambda: edl1d.EDLRun(electrode_voltage=-5.0, fit=dict(data="x.npz", params=("i0_CO", "p_eq_CO")), **t),
        "repeated name": lambda: edl1d.EDLRun(electrode_voltage=-5.0, fit=dict(data="x.npz", params=("i0_CO", "i0_CO")), **t),
        "no data": lambda: edl1d.EDLRun(electrode_voltage=-5.0, fit=dict(params=("i0_CO",)), **t),
        "3D": lambda: pore3d.PoreRun(electrode_voltage=-5.0, **t, **c),
        "rxn 1D": lambda: rxndiff1d.RxnDiffRun(**c),
        "rxn 3D": lambda: rxnpore3d.RxnPoreRun(**c),
        "EDLEnsemble": lambda: edl_ensemble.EDLEnsemble([dict(voltage_multiplier=-1.0), dict(voltage_multiplier=-1.0, **c)]),
        "PoreEnsemble": lambda: pore_ensemble.PoreEnsemble([dict(**c)]),
        "edl sweep": lambda: edl_sweep.run_sweep([dict(**c)]),
        "edl sweep keywords": lambda: edl_sweep.run_sweep([dict(voltage_multiplier=-1.0)], **c),
        "pore sweep group": lambda: sweep.run_group(5, [-1.0], 1, **c),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError, match="fit"):
            call()
    with pytest.raises(ValueError, match="fit"):
        ft.refuse_fit(c, "a test")
    ft.refuse_fit({}, "a test")


def test_command_line():
    from gmpnp_amd import edl1d
    a = edl1d.build_parser().parse_args([])
    assert a.fit_data is None and a.fit_params is None and ft.fit_keywords(a) == {}
    a = edl1d.build_parser().parse_args(["--fit_data", "curve.npz"])
    assert ft.fit_keywords(a) == {"fit": dict(data="curve.npz")}
    a = edl1d.build_parser().parse_args(["--fit_data", "curve.csv", "--fit_params", "i0_CO", "alpha_CO", "stern_length"])
    assert ft.fit_keywords(a) == {"fit": dict(data="curve.csv", params=("i0_CO", "alpha_CO", "stern_length"))}
    with pytest.raises(ValueError, match="fit"):
        ft.fit_keywords(edl1d.build_parser().parse_args(["--fit_params", "i0_CO"]))
    with pytest.raises(ValueError, match="fit"):
        edl1d.main(["--fit_data", "curve.npz"])                                                  # no --electrode_voltage
    par = ft.check_fit(dict(data="x.npz"), dict(electrode_voltage=-5.0, kinetics="tafel"))
    assert par["params"] == ft.DEFAULT_PARAMS


def test_metadata_keys_and_units():
    codes = ft.param_codes(FR.FIVE)
    theta = np.array([np.log(0.1), np.log(0.02), 0.5, 0.45, np.log(4e-4)])
    vals = ft.physical_values(codes, theta, 1e-6)
    assert np.allclose(vals, [0.1, 0.02, 0.5, 0.45, 4e-10], rtol=1e-15)
    ev = FR.Scripted(FR.tafel_law(FR.POTENTIALS, TRUTH))
    res = ft.LevenbergMarquardt(ev, LOGS).run(START)
    data = ft.check_data(dict(electrode_voltage=np.array(FR.POTENTIALS), i_CO=np.ones(6), i_H2=np.ones(6)), -5.0, 4)
    arrays = ft.fit_arrays(FR.FOUR, codes[:4], data, START, res, [{"i_CO": 1.0, "i_H2": 1.0}] * 6, 1e-6)
    meta = ft.fit_metadata(FR.FOUR, arrays, res)
    assert tuple(meta) == ft.METADATA_KEYS and meta["fit_stop_reason"] == "converged" and meta["fit_parameters"] == list(FR.FOUR)
    assert np.allclose(arrays["fitted_values"], [0.1, 0.02, 0.5, 0.45], rtol=1e-11) and arrays["covariance"].shape == (4, 4)
    assert len(arrays["history_cost"]) == res["trials"] + 1 and arrays["model_i_CO"].shape == (6,)
    import json
    json.dumps(meta)
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for key in ft.METADATA_KEYS:
        assert "`%s`" % key in text, key


def test_ctypes_images_have_the_layout_of_the_header(tmp_path):
    from gmpnp_amd import backend
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gmpnp.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n",'
                   'sizeof(gmpnp_stern_t),offsetof(gmpnp_stern_t,p_electrode),offsetof(gmpnp_stern_t,lam),offsetof(gmpnp_stern_t,eps_surface),'
                   'sizeof(gmpnp_kinetics_t),offsetof(gmpnp_kinetics_t,reactant),offsetof(gmpnp_kinetics_t,k),offsetof(gmpnp_kinetics_t,alpha),'
                   'offsetof(gmpnp_kinetics_t,nu),offsetof(gmpnp_kinetics_t,p_electrode));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S, C = backend.CStern, backend.CKinetics
    assert got == [ctypes.sizeof(S), S.p_electrode.offset, S.lam.offset, S.eps_surface.offset,
                   ctypes.sizeof(C), C.reactant.offset, C.k.offset, C.alpha.offset, C.nu.offset, C.p_electrode.offset]
    for name in ("gmpnp_parameter_advance", "gmpnp_get_electrode_options"):
        assert name in backend.EXPORTS
    header = open(os.path.join(ROOT, "include", "gmpnp.h")).read()
    assert "int gmpnp_parameter_advance(gmpnp_solver* s, int32_t n, const int32_t* param" in header
    assert "int gmpnp_get_electrode_options(gmpnp_solver* s, gmpnp_stern_t* stern_out" in header
    assert hasattr(backend.DeviceSolver, "parameter_advance") and hasattr(backend.DeviceSolver, "electrode_options")


# ---- the host rule of a moved parameter against its Python statement ------------------------------------------------------------------
DRIVER = r"""
#include <cstdio>
#include <cstring>
#include "gmpnp_host_rules.h"
using namespace gmpnp;
int main() {
  char cmd[32];
  while (std::scanf("%31s", cmd) == 1) {
    if (!std::strcmp(cmd, "move")) {
      gmpnp_stern_t st{}; gmpnp_kinetics_t kin{};
      int n;
      if (std::scanf("%d %lf %lf %lf %d", &st.model, &st.p_electrode, &st.lam, &st.eps_surface, &kin.n_reactions) != 5) return 1;
      kin.p_electrode = st.p_electrode;
      for (int r = 0; r < kin.n_reactions; ++r) { kin.reactant[r] = -1; if (std::scanf("%lf %lf", &kin.k[r], &kin.alpha[r]) != 2) return 1; }
      if (std::scanf("%d", &n) != 1) return 1;
      int32_t param[16]; double d[16];
      for (int k = 0; k < n; ++k) if (std::scanf("%d %lf", &param[k], &d[k]) != 2) return 1;
      const bool ok = parameter_move(st, kin, 6, n, param, d);
      std::printf("%d %a %a", (int)ok, st.p_electrode, st.lam);
      for (int r = 0; r < kin.n_reactions; ++r) std::printf(" %a %a", kin.k[r], kin.alpha[r]);
      std::printf("\n");
    } else if (!std::strcmp(cmd, "refusal")) {
      int n, nl; double tau;
      int32_t param[16], last[16], status[16]; double d[16];
      if (std::scanf("%d", &n) != 1) return 1;
      for (int k = 0; k < n && k < 16; ++k) if (std::scanf("%d %lf", &param[k], &d[k]) != 2) return 1;
      if (std::scanf("%lf %d", &tau, &nl) != 2) return 1;
      for (int k = 0; k < nl; ++k) if (std::scanf("%d %d", &last[k], &status[k]) != 2) return 1;
      const char* why = parameter_advance_refusal(n, param, d, tau, nl, last, status);
      std::printf("%s\n", why ? why : "fine");
    }
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    d = tmp_path_factory.mktemp("fit_rule")
    src, exe = d / "rule.cpp", d / "rule"
    src.write_text(DRIVER)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "gmpnp_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True)

    def ask(lines):
        return subprocess.run([str(exe)], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
    return ask


def test_host_rule_of_a_moved_parameter_against_its_python_statement(rules):
    """parameter_move: the moved values (p_M and alpha bit for bit; k and lam within one rounding of exp, which the C library and
    Python's need not share) and the validity verdict; parameter_advance_refusal: what is refused."""
    base = dict(model="BDM", p_electrode=-5.0, lam=4e-4, eps_surface=6.0)
    kin = {"reactions": [dict(k=0.1, alpha=0.5, p_eq=0.0, reactant=None, nu={}), dict(k=0.02, alpha=0.45, p_eq=0.0, reactant=None, nu={})], "p_electrode": -5.0}
    steps = [[(16, 0.7), (17, -0.5), (32, 0.08), (33, -0.06)], [(48, 0.2), (0, -1.5)], [(33, 0.1), (48, -800.0)], [(16, 800.0)], [(17, -800.0)],
             [(32, float("inf"))], [(0, float("nan"))], [(48, 710.0)], [(16, 0.0), (48, 0.0)]]
    lines = []
    for st in steps:
        lines.append("move 2 %r %r %r 2 %r %r %r %r %d " % (base["p_electrode"], base["lam"], base["eps_surface"], 0.1, 0.5, 0.02, 0.45, len(st))
                     + " ".join("%d %r" % (p, d) for p, d in st))
    out = rules(lines)
    verdicts = []
    for st, line in zip(steps, out):
        s, k, ok = ft.moved_options(base, kin, 6, [p for p, _ in st], [d for _, d in st])
        got = line.split()
        verdicts.append(ok)
        assert int(got[0]) == int(ok), st
        vals = [float.fromhex(x) for x in got[1:]]
        want = [s["p_electrode"], s["lam"], k["reactions"][0]["k"], k["reactions"][0]["alpha"], k["reactions"][1]["k"], k["reactions"][1]["alpha"]]
        for j, (a, b) in enumerate(zip(vals, want)):
            if j in (0, 3, 5) or not np.isfinite(b) or b == 0.0:
                assert a == b or (np.isnan(a) and np.isnan(b)), (st, j)
            else:
                assert abs(a - b) <= 2.0 * np.spacing(abs(b)), (st, j)
    assert verdicts == [True, True, False, False, True, False, False, False, True]   # lam -> 0, k -> inf, (k -> 0 is a valid k), inf, nan, lam -> inf
    asks = ["refusal 1 0 -1.0 0.0 2 48 0 0 0", "refusal 0 0.0 1 0 0", "refusal 11 " + "0 0.0 " * 11 + "0.0 1 0 0", "refusal 2 16 0.1 16 0.1 0.0 2 16 0 17 0",
            "refusal 1 17 0.1 0.0 1 16 0", "refusal 1 16 nan 0.0 1 16 0", "refusal 1 16 0.1 1.0 1 16 0", "refusal 1 16 0.1 -0.5 1 16 0",
            "refusal 1 16 0.1 0.9 2 16 1 17 0", "refusal 2 17 0.1 16 -0.2 0.9 2 16 0 17 0"]
    got = rules(asks)
    assert got[0] == "fine" and got[9] == "fine"
    for line, word in zip(got[1:9], ("1 ... 10", "1 ... 10", "repeated", "last", "finite", "tau", "tau", "not finite")):
        assert word in line, (line, word)
