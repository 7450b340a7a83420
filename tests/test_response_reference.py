"""The small-signal frequency response on the CPU: the NumPy restatement (tests/response_reference.py) against
its own limits — J affine in inv_dt, the linearisation identity, the closed-form rows against central differences, the high-frequency
closed form, the zero-frequency response against differences of two steady states, the shape of the impedance —, the rule of the
library (gmpnp_host_rules.h, compiled with the host compiler alone) against its Python statement (gmpnp_amd/impedance.py), the unit
conversions, the ctypes image, every refusal of the Python layer and the command line.  The case throughout is K+ on the 1 um mesh
(1091 vertices), Stern BDM, p_M = -5, the TAFEL parameters of tests/test_kinetics_reference.py, at the steady state."""
import math
import os
import subprocess

import numpy as np
import pytest

import kinetics_reference as K
import response_reference as R
import stern_bc_reference as SR
from step_limit_reference import first_step_state
from test_kinetics_reference import TAFEL, _edl_k, first_step_problem, ulps
from gmpnp_amd import impedance as imp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_M = -5.0


@pytest.fixture(scope="module")
def case():
    """(ep, prob, steady state u, System) of the operating point: the first step's Newton solve, then Newton at inv_dt = 0."""
    ep, mesh = _edl_k()
    prob = first_step_problem(ep, mesh, P_M)
    u1, st = K.newton_loop(prob, *first_step_state(prob))
    assert st.converged
    u, its = R.steady_state(prob, u1)
    print("steady state: %d Newton iterations at inv_dt = 0" % its)
    assert its <= 6
    return ep, prob, u, R.system(prob, u)


def steady_at(prob, u, p_M):
    return R.steady_state(R.with_potential(prob, p_M), u)[0]


def test_mass_matrix_and_affine_jacobian(case):
    """M is the consistent mass of the species rows, its potential and Dirichlet rows are zero, and J(inv_dt) - K - inv_dt M is at
    rounding for inv_dt = 1 and the driver's value: every entry of J is a sum of fewer than 20 terms, so 20 eps max |J| bounds it."""
    ep, prob, u, S = case
    nf, ns = prob.nf, prob.nf - 1
    M = S.M.tocsr()
    assert not M[np.arange(ns, prob.ndof, nf)].nnz and not M[prob.bc_dofs].nnz
    x = prob.coords[:, 0]
    h = np.diff(np.sort(x))
    order = np.argsort(x)
    a, b = order[3], order[4]
    assert M[a * nf + 2, b * nf + 2] == h[3] / 6.0 and M[a * nf + 2, b * nf + 1] == 0.0
    assert abs(M[b * nf, b * nf] - (h[3] + h[4]) / 3.0) <= 2e-16 * h.max()
    assert abs((M - M.T)[np.setdiff1d(np.arange(prob.ndof), prob.bc_dofs)][:, np.setdiff1d(np.arange(prob.ndof), prob.bc_dofs)]).max() == 0.0
    for inv_dt in (1.0, float(prob.model.inv_dt)):
        J = R.jacobian(prob, u, inv_dt)
        d = abs(J - S.K - inv_dt * S.M).max()
        print("J(%g) - K - inv_dt M: %.2e of max |J| = %.2e" % (inv_dt, d, abs(J).max()))
        assert d <= 20 * np.finfo(float).eps * abs(J).max()
    # the difference J(1) - J(0) carries the digits |K| / |M| eats: M comes from the mesh
    lost = abs(R.jacobian(prob, u, 1.0) - S.K - S.M).max() / abs(S.M).max()
    assert lost < 1e-6


def test_linearisation_identity(case):
    """max |F(u + e x0, p_M + e) - F(u - e x0, p_M - e)| / 2e at inv_dt = 0 with x0 the zero-frequency response: <= 1e-7 max |b| at
    e = 1e-3 (K x0 + b = 0; what is left is the O(e^2) truncation)."""
    ep, prob, u, S = case
    x0 = np.asarray(R.solve(S, 0.0).real, dtype=np.float64)
    e = 1e-3
    Fp = R.residual(R.with_potential(prob, P_M + e), u + e * x0)
    Fm = R.residual(R.with_potential(prob, P_M - e), u - e * x0)
    got = np.abs(Fp - Fm).max() / (2 * e)
    print("linearisation identity: %.2e of max |b| = %.2e" % (got, np.abs(S.b).max()))
    assert got <= 1e-7 * np.abs(S.b).max()


def test_closed_form_rows_against_central_differences(case):
    """dD/dp_M, dD/du, dI_r/dp_M and dI_r/du against central differences of stern_displacement and of the currents: 1e-7 of the
    largest term, the bound of sections 5h - 5j for this procedure."""
    ep, prob, u, S = case
    dD, rowD = R.displacement_row(prob, u)
    dI, rowsI = R.current_rows(prob, u)
    h = 1e-6
    fd = (SR.stern_displacement(R.with_potential(prob, P_M + h), u) - SR.stern_displacement(R.with_potential(prob, P_M - h), u)) / (2 * h)
    e = [abs(fd - dD) / abs(dD)]
    fdI = (K.currents(R.with_potential(prob, P_M + h), u) - K.currents(R.with_potential(prob, P_M - h), u)) / (2 * h)
    e.append(np.abs(fdI - dI).max() / np.abs(dI).max())
    rng = np.random.default_rng(11)
    for _ in range(3):
        dv = rng.standard_normal(prob.ndof)
        fd = (SR.stern_displacement(prob, u + h * dv) - SR.stern_displacement(prob, u - h * dv)) / (2 * h)
        e.append(abs(fd - rowD @ dv) / np.abs(rowD * dv).max())
        fdI = (K.currents(prob, u + h * dv) - K.currents(prob, u - h * dv)) / (2 * h)
        e.append(np.abs(fdI - rowsI @ dv).max() / np.abs(rowsI * dv).max())
    print("closed-form rows against central differences:", " ".join("%.2e" % v for v in e))
    assert max(e) < 1e-7
    assert np.array_equal(dI, -np.array([r.alpha for r in prob.kinetics.reactions]) * K.currents(prob, u))   # dI_r/dp_M = -alpha_r I_r


def test_high_frequency_closed_form(case):
    """C(1e14) is the Stern capacitor in series with the element capacitors, 1 / (lam / g + sum_e h_e / eps_e): within 1e-6 (the
    O(1 / sigma) term)."""
    ep, prob, u, S = case
    _, C, dI = R.response(S, 1e14)
    closed = R.high_frequency_closed_form(prob, u)
    print("C(1e14) = %r, closed form %.10g" % (complex(C), closed))
    assert abs(complex(C) - closed) <= 1e-6 * closed


def test_zero_frequency_response_against_steady_state_differences(case):
    """C(0) and dI_r(0) against the central differences of D and I_r between two steady states at p_M -+ 1e-3: within 1e-6 (the
    truncation is O(delta^2))."""
    ep, prob, u, S = case
    _, C, dI = R.response(S, 0.0)
    d = 1e-3
    up, um = steady_at(prob, u, P_M + d), steady_at(prob, u, P_M - d)
    pp, pm = R.with_potential(prob, P_M + d), R.with_potential(prob, P_M - d)
    fdC = (SR.stern_displacement(pp, up) - SR.stern_displacement(pm, um)) / (2 * d)
    fdI = (K.currents(pp, up) - K.currents(pm, um)) / (2 * d)
    eC, eI = abs(fdC - C.real) / abs(fdC), np.abs(fdI - np.asarray(dI.real, dtype=float)).max() / np.abs(fdI).max()
    print("zero frequency: C %.10g (differences %.10g, %.2e), dI %s (%.2e)" % (float(C.real), fdC, eC, np.asarray(dI.real, dtype=float), eI))
    assert eC < 1e-6 and eI < 1e-6 and abs(C.imag) == 0.0


def test_impedance_is_passive_and_ends_at_the_charge_transfer_resistance(case):
    """Re Z > 0 over 1e-2 ... 1e8 Hz, and Z(1e-2 Hz) = R_ct = 1 / (-dI/dV at sigma = 0) within omega (R_ct C(0) + L_n^2 / D_min): the
    first-order terms of Y = i omega C - sum dI/dV are the capacitive current and the lag of the slowest species' diffusion across the
    domain; both time constants are of the operating point, not of the solve."""
    ep, prob, u, S = case
    from gmpnp_amd.params import _load_yaml, utilities_dir
    eps_0 = _load_yaml(os.path.join(utilities_dir(), "parameters.yaml"))["nat_const"]["eps_0"]
    f = imp.frequency_grid(1e-2, 1e8, 2)
    sig = imp.sigma_from_frequency(ep, f)
    rows = [R.response(S, s, "splu") for s in sig]
    res = {"sigma": sig, "C": np.array([complex(r[1]) for r in rows]), "dI": np.array([np.asarray(r[2], dtype=complex) for r in rows]),
           "residual": np.zeros(len(f)), "status": np.zeros(len(f), dtype=np.int32)}
    sp_ = imp.spectrum(ep, eps_0, f, res)
    assert np.all(sp_["impedance"].real > 0.0)
    _, C0, dI0 = R.response(S, 0.0)
    R_ct = 1.0 / (-float(np.sum(dI0).real) / ep.thermal_voltage)
    tau = R_ct * eps_0 / ep.L_n * float(C0.real) + ep.L_n ** 2 / min(ep.diff_coeff.values())
    dev = abs(sp_["impedance"][0] - R_ct) / R_ct
    print("R_ct = %.6g Ohm m2, Z(%g Hz) = %r, deviation %.2e, bound %.2e" % (R_ct, f[0], complex(sp_["impedance"][0]), dev, 2 * math.pi * f[0] * tau))
    assert R_ct > 0.0 and dev <= 2 * math.pi * f[0] * tau
    assert abs(sp_["capacitance"][0].real - eps_0 / ep.L_n * float(C0.real)) <= 1e-3 * abs(sp_["capacitance"][0].real)


def test_models_agree_with_the_refined_solution(case):
    """Plain splu and the NumPy block-Thomas model of the device algorithm against the refined solution at the test frequencies of the
    GPU suite: within 1e-7 (the bound a device result has to meet whatever the model says), residual of the model <= 1e-13."""
    ep, prob, u, S = case
    for sg in (0.0, 1e4, 1e14):
        xr, Cr, dIr = R.response(S, sg)
        for how in ("splu", "thomas"):
            x, C, dI = R.response(S, sg, how)
            ex, eC = np.abs(x - xr).max() / np.abs(xr).max(), abs(C - Cr) / abs(Cr)
            print("sigma %g %s: x %.2e C %.2e residual %.2e" % (sg, how, ex, eC, R.relative_residual(S, sg, x)))
            assert ex < 1e-7 and eC < 1e-7
            if how == "thomas":
                assert R.relative_residual(S, sg, x) <= 1e-13
                Cb, dIb = R.functionals_by_rule(prob, u, x)
                assert abs(Cb - C) <= 1e-12 * abs(C) and np.abs(dIb - dI).max() <= 1e-12 * np.abs(dI).max()


# ---- the rule: C++ (g++ alone) against the Python statement ------------------------------------------------------------------------------
DRIVER = r"""
#include <cstdio>
#include "gmpnp_host_rules.h"
using namespace gmpnp;
int main() {
  double v[10];
  while (std::scanf("%lf %lf %lf %lf %lf %lf %lf %lf %lf", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8) == 9) {
    const Cx c = response_capacitance_term(v[0], v[1], v[2], v[3], v[4], Cx{v[5], v[6]}, Cx{v[7], v[8]});
    const Cx i = response_current_term(v[0], v[1], v[2], Cx{v[5], v[6]}, Cx{v[7], v[8]});
    const Cx q = cx_mul(cx_inv(Cx{v[5], v[6]}), Cx{v[5], v[6]});
    std::printf("%a %a %a %a %a %a %a\n", c.re, c.im, i.re, i.im, response_pivot_key(Cx{v[5], v[6]}), q.re, q.im);
  }
  std::printf("%d%d%d%d%d%d\n", (int)response_sigma_valid(0.0), (int)response_sigma_valid(1e14), (int)response_sigma_valid(-1e-300),
              (int)response_sigma_valid(1.0 / 0.0), (int)response_sigma_valid(0.0 / 0.0), (int)response_sigma_valid(-0.0));
  std::printf("%d%d%d%d\n", (int)response_count_valid(0), (int)response_count_valid(1), (int)response_count_valid(4096), (int)response_count_valid(4097));
  std::printf("%d %d %d %d %d %d\n", response_chunk(70, 1091, 1e9), response_chunk(70, 1091, 2.6e7), response_chunk(70, 1091, 1.0), response_chunk(1, 5990, 0.0),
              response_chunk(4096, 5990, 1073741824.0), response_chunk(70, 1091, 1.0 / 0.0));
  std::printf("%.0f\n", response_bytes_per_frequency(5990));
  std::printf("%s\n%s\n", status_message(256).c_str(), status_message(512).c_str());
  return 0;
}
"""
# (g | w, dg | d_u, lam | d_p, p_M, p, x_p.re, x_p.im, s.re, s.im): the first three are read as (w, d_u, d_p) by the current's term
TERM_CASES = [(75.2, 0.43, 4e-4, -5.0, -2.26, 0.61, 0.0, -0.011, 0.0), (75.2, 0.43, 4e-4, -5.0, -2.26, 0.52, -0.13, 3e-3, -2e-3),
              (6.0, 0.5, 8e-3, -20.0, -6.6, 1.0, 0.0, 0.0, 0.0), (1.0, 0.36, 0.18, 3.0, 0.5, -0.25, 0.75, 1.5, -0.5), (0.25, 1e-3, 14.4, 0.0, 0.0, 1e-12, 3e-14, -7.0, 2.0)]


@pytest.fixture(scope="module")
def rule_out(tmp_path_factory):
    d = tmp_path_factory.mktemp("response_rule")
    src = d / "rule.cpp"
    src.write_text(DRIVER)
    exe = d / "rule"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "gmpnp_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True)
    text = "".join(" ".join(repr(v) for v in c) + "\n" for c in TERM_CASES)
    return subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.split("\n")


def test_host_rule_against_its_python_statement(rule_out):
    """The two node terms of the library's host functions and of gmpnp_amd/impedance.py agree within 2 ulp of the larger part (a sum
    of two products each; the host compiler may contract them), the pivot key is |re| + |im| exactly, and the validity checks, the chunk
    rule and the two status lines are those of the Python statement."""
    for c, line in zip(TERM_CASES, rule_out):
        h = [float.fromhex(x) for x in line.split()]
        ct = imp.capacitance_term(c[0], c[1], c[2], c[3], c[4], complex(c[5], c[6]), complex(c[7], c[8]))
        it = imp.current_term(c[0], c[1], c[2], complex(c[5], c[6]), complex(c[7], c[8]))
        for got, want in ((complex(h[0], h[1]), ct), (complex(h[2], h[3]), it)):
            scale = max(abs(want.real), abs(want.imag))
            assert abs(got - want) <= 4 * math.ulp(scale), (c, got, want)
        assert h[4] == imp.pivot_key(complex(c[5], c[6])) == abs(c[5]) + abs(c[6])
        assert abs(complex(h[5], h[6]) - 1.0) <= 4e-16
    k = len(TERM_CASES)
    cases = (0.0, 1e14, -1e-300, math.inf, math.nan, -0.0)
    assert rule_out[k] == "".join(str(int(imp.sigma_valid(s))) for s in cases) == "110001"
    assert rule_out[k + 1] == "".join(str(int(imp.count_valid(n))) for n in (0, 1, 4096, 4097)) == "0110"
    want = [imp.chunk(70, 1091, 1e9), imp.chunk(70, 1091, 2.6e7), imp.chunk(70, 1091, 1.0), imp.chunk(1, 5990, 0.0), imp.chunk(4096, 5990, 1073741824.0),
            imp.chunk(70, 1091, math.inf)]
    assert [int(x) for x in rule_out[k + 2].split()] == want
    assert want[0] == 70 and want[1] == 16 and want[2] == 1 and want[3] == 1 and want[4] % 8 == 0 and 8 <= want[4] < 4096 and want[5] == 70
    assert float(rule_out[k + 3]) == imp.bytes_per_frequency(5990) == 5990 * 72 * 16
    assert "frequency response" in rule_out[k + 4] and "pivot" in rule_out[k + 4] and "frequency response" in rule_out[k + 5] and "not finite" in rule_out[k + 5]


# ---- units -------------------------------------------------------------------------------------------------------------------------------
def test_unit_conversions_on_a_hand_computed_row():
    """sigma of the frequency whose period is 2 pi time steps is the driver's model.inv_dt; one row of the spectrum by hand."""
    ep, _ = _edl_k()
    f_step = 1.0 / (2.0 * math.pi * ep.time_step)
    assert abs(imp.sigma_from_frequency(ep, f_step) - ep.model.inv_dt) <= 4e-16 * ep.model.inv_dt
    assert abs(ep.model.inv_dt - ep.time_constant / (ep.time_step * ep.L_D)) <= 4e-16 * ep.model.inv_dt     # EDLParameters: inv_dt = 1 / (dt L_D), dt = time_step / time_constant
    eps_0 = 8.8541878128e-12
    res = {"sigma": np.array([3.0]), "C": np.array([4.0e4 - 2.0e3j]), "dI": np.array([[-0.1 + 0.01j, -0.02 + 0.0j]]), "residual": np.array([1e-15]),
           "status": np.array([0], dtype=np.int32)}
    sp_ = imp.spectrum(ep, eps_0, [50.0], res)
    cap = eps_0 / ep.L_n * (4.0e4 - 2.0e3j)
    Y = 1j * 2.0 * math.pi * 50.0 * cap + (0.12 - 0.01j) / ep.thermal_voltage
    assert abs(sp_["capacitance"][0] - cap) <= 1e-15 * abs(cap) and abs(cap.real - 0.35416751) < 1e-6 * (1e-6 / ep.L_n)
    assert np.allclose(sp_["dI_dV"][0], np.array([-0.1 + 0.01j, -0.02]) / ep.thermal_voltage, rtol=1e-15, atol=0.0)
    assert abs(sp_["admittance"][0] - Y) <= 1e-15 * abs(Y) and abs(sp_["impedance"][0] * Y - 1.0) <= 1e-15
    assert sp_["admittance"][0].real > 0.0          # cathodic currents are positive: -dI/dV is a conductance
    g = imp.frequency_grid(1e-2, 1e8, 10)
    assert len(g) == 101 and g[0] == 1e-2 and abs(g[-1] - 1e8) <= 1e-7 and np.allclose(g[10::10] / g[:-10:10], 10.0)
    assert len(imp.frequency_grid(5.0, 5.0, 3)) == 1
    for bad in (dict(freq_min=0.0), dict(freq_min=10.0, freq_max=1.0), dict(per_decade=0), dict(freq_min=1e-300, freq_max=1e300, per_decade=10)):
        with pytest.raises(ValueError, match="impedance"):
            imp.frequency_grid(**bad)


def test_ctypes_image_has_the_layout_of_the_header(tmp_path):
    import ctypes
    from gmpnp_amd import backend
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gmpnp.h"\nint main(void){printf("%zu %zu %zu %zu %zu\\n",sizeof(gmpnp_response_t),'
                   'offsetof(gmpnp_response_t,C),offsetof(gmpnp_response_t,dI),offsetof(gmpnp_response_t,residual),offsetof(gmpnp_response_t,status));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    C = backend.CResponse
    assert got == [ctypes.sizeof(C), C.C.offset, C.dI.offset, C.residual.offset, C.status.offset] == [104, 8, 24, 88, 96]
    assert "gmpnp_frequency_response" in backend.EXPORTS and backend.RESPONSE_MAX_FREQUENCIES == imp.MAX_FREQUENCIES
    assert (backend.RESPONSE_SINGULAR, backend.RESPONSE_NONFINITE) == (imp.STATUS_SINGULAR, imp.STATUS_NONFINITE) == (256, 512)


# ---- refusals of the Python layer: ValueError before anything touches the device (there is none here) and the command line -------------------
def test_python_refusals_and_command_line():
    from gmpnp_amd import edl1d, edl_ensemble, edl_sweep, pore3d, pore_ensemble, rxndiff1d, rxnpore3d, sweep
    want = dict(freq_min=1.0, freq_max=1e3, per_decade=2)
    calls = {
        "no electrode voltage": lambda: edl1d.EDLRun(impedance=want),
        "stabilization": lambda: edl1d.EDLRun(electrode_voltage=-5.0, stabilization="Y", model="PNP", impedance=want),
        "bad grid": lambda: edl1d.EDLRun(electrode_voltage=-5.0, impedance=dict(freq_min=-1.0)),
        "PoreRun": lambda: pore3d.PoreRun(electrode_voltage=-5.0, impedance=want),
        "rxn 1D": lambda: rxndiff1d.RxnDiffRun(impedance=want),
        "rxn 3D": lambda: rxnpore3d.RxnPoreRun(impedance=want),
        "EDLEnsemble": lambda: edl_ensemble.EDLEnsemble([dict(voltage_multiplier=-1.0), dict(voltage_multiplier=-1.0, impedance=want)]),
        "PoreEnsemble": lambda: pore_ensemble.PoreEnsemble([dict(impedance=want)]),
        "edl sweep": lambda: edl_sweep.run_sweep([dict(impedance=want)]),
        "edl sweep keywords": lambda: edl_sweep.run_sweep([dict(voltage_multiplier=-1.0)], impedance=want),
        "pore sweep job": lambda: sweep.run_job(5, -1.0, 1, impedance=want),
        "pore sweep group": lambda: sweep.run_group(5, [-1.0], 1, impedance=want),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError, match="impedance"):
            call()
    p = edl1d.build_parser()
    a = p.parse_args([])
    assert a.impedance is False and imp.impedance_keywords(a) == {}
    a = p.parse_args(["--impedance"])
    assert imp.impedance_keywords(a) == {"impedance": dict(freq_min=1e-2, freq_max=1e8, per_decade=10)}
    a = p.parse_args(["--impedance", "--freq_min", "1", "--freq_max", "1e4", "--freq_per_decade", "3"])
    assert imp.impedance_keywords(a) == {"impedance": dict(freq_min=1.0, freq_max=1e4, per_decade=3)}
    with pytest.raises(ValueError, match="impedance"):
        edl1d.main(["--impedance"])
    with pytest.raises(ValueError, match="impedance"):
        edl1d.main(["--impedance", "--electrode_voltage", "-5", "--freq_min", "0"])
    for mod in (pore3d, rxndiff1d, rxnpore3d):
        with pytest.raises(SystemExit):
            mod.build_parser().parse_args(["--impedance"])
