"""The small-signal frequency response of the 3D pore on the CPU: the NumPy restatement
(tests/pore_response_reference.py) against its own limits — J affine in inv_dt with the tetrahedron mass formed from the mesh, the
zero-frequency response against the tangent's p_M column, the high-frequency end against the potential-block solve —, the rule of the
library (gmpnp_host_rules.h, compiled with the host compiler alone) against its Python statement (gmpnp_amd/impedance.py), the pore's
unit conversions, every refusal of the Python layer and the command line.  Cases: the box pore ``box_pore_problem(2, 3)`` and the
generated cylinder (1, 2) (21 vertices), both with the Stern layer (BDM, p_M = -1), two Tafel reactions and a random state."""
import math
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import galvanostat_reference as GR
import pore_response_reference as P
import response_reference as R
import tangent_reference as T
from conftest import box_pore_problem, random_state
from gmpnp_amd import impedance as imp
from gmpnp_amd import polarisation as pol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=["box", "cylinder"])
def case(request):
    """(name, prob, u, K, M, b)"""
    prob = P.with_stern_and_kinetics(box_pore_problem(2, 3)[2]) if request.param == "box" else P.cylinder_case((1, 2))
    u, _ = random_state(prob.coords.shape[0], prob.nf - 1, seed=3)
    return (request.param, prob, u) + P.system(prob, u)


def test_mass_matrix_and_affine_jacobian(case):
    """M is the consistent tetrahedron mass of the free species rows (potential and Dirichlet rows zero, symmetric on the free rows, its
    sum the volume per species), and J(inv_dt) - K - inv_dt M is at rounding.  What the NumPy assembly itself shows: the two sides
    differ only where M has entries, by the rounding of adding inv_dt M_ij into the element sums of that entry, eps (|K_ij| + inv_dt
    |M_ij|) per addition; the bound is 100 times eps times the largest such entry (the species blocks: 2.4 on the cylinder, far below
    max |J|, which sits on the potential rows)."""
    name, prob, u, K, M, b = case
    nf, ns = prob.nf, prob.nf - 1
    assert not M[np.arange(ns, prob.ndof, nf)].nnz and not M[prob.bc_dofs].nnz
    free = np.setdiff1d(np.arange(prob.ndof), np.r_[prob.bc_dofs, np.arange(ns, prob.ndof, nf)])
    Mf = M[free][:, free]
    assert abs(Mf - Mf.T).max() == 0.0
    full = P.mass(type("Q", (), dict(coords=prob.coords, cells=prob.cells, nf=nf, ndof=prob.ndof, bc_dofs=np.zeros(0, dtype=np.int64)))())
    assert abs(full.sum() - ns * P.cell_volumes(prob).sum()) <= 1e-13 * full.sum()
    for inv_dt in (1.0, float(prob.model.inv_dt)):
        J = R.jacobian(prob, u, inv_dt)
        d = abs(J - K - inv_dt * M).max()
        print("%s: J(%g) - K - inv_dt M: %.2e, max |J| = %.2e (%.1f eps)" % (name, inv_dt, d, abs(J).max(), d / abs(J).max() / np.finfo(float).eps))
        shows = np.finfo(float).eps * float((abs(K).multiply(M != 0) + inv_dt * abs(M)).max())
        print("%s: the assembly's own rounding on M's pattern %.2e, bound %.2e" % (name, shows, 100 * shows))
        assert d <= 100 * shows


def test_zero_frequency_response_is_the_tangents_p_M_column(case):
    """C(0) and dI_r(0) of the complex route (the real 2N system at sigma = 0) equal the functionals of the tangent's p_M column at
    inv_dt = 0 (K z = -b, refined; tangent_reference.functionals) to 1e-10, and the imaginary parts are zero."""
    name, prob, u, K, M, b = case
    x = np.asarray(P.solve(K, M, b, 0.0), dtype=complex)
    z = np.asarray(GR.refined_solve(K.tocsc(), spla.splu(K.tocsc()), -b), dtype=np.float64)
    C, dI = P.functionals(prob, u, x)
    dD, dIt, _ = T.functionals(prob, u, z, pol.PARAM_P_M)
    print("%s: C(0) %r tangent dD %.12g; dI(0) %s tangent %s" % (name, C, dD, dI, dIt))
    assert C.imag == 0.0 and not np.any(dI.imag)
    assert abs(C.real - dD) <= 1e-10 * abs(dD) and np.all(np.abs(dI.real - dIt) <= 1e-10 * np.abs(dIt))
    assert dD > 0.0    # a capacitance


def high_frequency_figures(prob, u, K, M, b):
    """(C(1e14) refined, closed form, the reference's own error: plain splu against its refined solution, relative)"""
    xr = np.asarray(P.solve(K, M, b, 1e14), dtype=complex)
    xs = P.solve(K, M, b, 1e14, "splu")
    Cr, Cs = P.functionals(prob, u, xr)[0], P.functionals(prob, u, xs)[0]
    closed, _ = P.potential_block_capacitance(prob, u, K, b)
    return Cr, closed, abs(Cs - Cr) / abs(Cr)


def test_high_frequency_end_against_the_potential_block(case):
    """C at sigma = 1e14 is the potential block of K alone (the concentrations cannot follow): within 10 times the reference's own
    error (splu against its refined solution), floor 1e-9 — this end is ill-conditioned (sigma M against K), section 5k."""
    name, prob, u, K, M, b = case
    Cr, closed, own = high_frequency_figures(prob, u, K, M, b)
    bound = max(10.0 * own, 1e-9)
    print("%s: C(1e14) = %r, potential block %.12g, deviation %.2e, reference's own error %.2e" % (name, Cr, closed, abs(Cr - closed) / abs(closed), own))
    assert abs(Cr - closed) <= bound * abs(closed)
    assert imp.pore_stern_terms(prob.coords, prob.wall_facets, prob.model, prob.stern, prob.bc_dofs, u.reshape(-1, prob.nf))[0].imag == 0.0


def test_python_statement_of_the_wall_terms(case):
    """gmpnp_amd/impedance.py's facet loop (pore_stern_terms) against tangent_reference.functionals on a complex x, and its b against
    the Stern rows of the restatement's b: 1e-13 (the same terms in another order)."""
    name, prob, u, K, M, b = case
    x = np.asarray(P.solve(K, M, b, 1e2, "splu"), dtype=complex)
    C, _, (aR, _, aI, _) = P.functionals(prob, u, x, want_scale=True)
    Cp, bp = imp.pore_stern_terms(prob.coords, prob.wall_facets, prob.model, prob.stern, prob.bc_dofs, u.reshape(-1, prob.nf), x.reshape(-1, prob.nf))
    assert abs(Cp.real - C.real) <= 1e-13 * aR and abs(Cp.imag - C.imag) <= 1e-13 * aI
    rows = np.arange(prob.nf - 1, prob.ndof, prob.nf)
    assert np.abs(bp[rows] - b[rows]).max() <= 1e-13 * np.abs(b[rows]).max() and not bp[np.setdiff1d(np.arange(prob.ndof), rows)].any()


# ---- the rule: C++ (g++ alone) against the Python statement --------------------------------------------------------------------------
DRIVER = r"""
#include <cstdio>
#include "gmpnp_host_rules.h"
using namespace gmpnp;
int main() {
  // 3678 node blocks, band 182, nf 9: one frequency takes 3678 * 365 * 81 * 16 bytes
  const double per = response_band_bytes_per_frequency(3678, 182, 9);
  std::printf("%.0f\n", per);
  std::printf("%d %d %d %d %d %d\n", response_band_chunk(40, 3678, 182, 9, 0.5 * per), response_band_chunk(40, 3678, 182, 9, per),
              response_band_chunk(40, 3678, 182, 9, 2.9 * per), response_band_chunk(40, 3678, 182, 9, 41.0 * per),
              response_band_chunk(1, 3678, 182, 9, 0.0), response_band_chunk(40, 3678, 182, 9, 1.0 / 0.0));
  Cx A[81], inv[81];
  int piv[9];
  double v[18];
  for (int r = 0; r < 9; ++r) {
    if (std::scanf("%lf %lf %lf %lf %lf %lf %lf %lf %lf %lf %lf %lf %lf %lf %lf %lf %lf %lf", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8, v + 9,
                   v + 10, v + 11, v + 12, v + 13, v + 14, v + 15, v + 16, v + 17) != 18) return 1;
    for (int j = 0; j < 9; ++j) A[r * 9 + j] = Cx{v[2 * j], v[2 * j + 1]};
  }
  const bool bad = response_block_inverse<9>(A, inv, piv);
  for (int k = 0; k < 9; ++k) std::printf("%d ", piv[k]);
  std::printf("%d\n", (int)bad);
  for (int q = 0; q < 81; ++q) std::printf("%a %a\n", inv[q].re, inv[q].im);
  std::printf("%a\n", response_facet_term(75.2, 0.43, 4e-4, 0.013, 2.5e-3, -0.011, 0.61));
  return 0;
}
"""


def tie_block():
    """A 9 x 9 complex block whose pivot search meets ties: column 0 holds 2, 2i, 1 + i and -2 (key 2 four times: the lowest row
    wins), and later columns are built so that a row exchange is needed."""
    rng = np.random.default_rng(5)
    A = rng.integers(-3, 4, (9, 9)).astype(float) + 1j * rng.integers(-3, 4, (9, 9)).astype(float)
    A[:, 0] = [0.5, 2.0, 2.0j, 1.0 + 1.0j, -2.0, 0.25, 0.0, -1.0j, 1.0]
    A[1, 1], A[2, 1], A[5, 1] = 0.0, 3.0 - 3.0j, 3.0 + 3.0j
    return A


@pytest.fixture(scope="module")
def rule_out(tmp_path_factory):
    d = tmp_path_factory.mktemp("pore_response_rule")
    src = d / "rule.cpp"
    src.write_text(DRIVER)
    exe = d / "rule"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "gmpnp_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True)
    text = "".join(" ".join("%r %r" % (float(z.real), float(z.imag)) for z in row) + "\n" for row in tie_block())
    return subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.split("\n")


def test_host_rule_against_its_python_statement(rule_out):
    """The chunk rule at caps below one frequency, exactly one, between, above n, zero and infinite; the pivot order of the complex
    9 x 9 inverse on a block with ties; its inverse (the host compiler may contract: 1e-13 of the largest entry, and A inv = I); the
    facet term within 4 ulp."""
    per = imp.band_bytes_per_frequency(3678, 182, 9)
    assert float(rule_out[0]) == per == 3678 * 365 * 81 * 16 and abs(per / 1e9 - 1.74) < 0.01
    want = [imp.band_chunk(40, 3678, 182, 9, c) for c in (0.5 * per, per, 2.9 * per, 41.0 * per)] + [imp.band_chunk(1, 3678, 182, 9, 0.0),
                                                                                                   imp.band_chunk(40, 3678, 182, 9, math.inf)]
    assert [int(x) for x in rule_out[1].split()] == want == [1, 1, 2, 40, 1, 40]
    A = tie_block()
    inv, piv, bad = imp.block_inverse(A)
    got = [int(x) for x in rule_out[2].split()]
    assert got[:9] == piv and got[9] == int(bad) == 0
    assert piv[0] == 1 and any(p != k for k, p in enumerate(piv[1:], start=1))       # the tie goes to the lower row; a later exchange
    host = np.array([complex(float.fromhex(a), float.fromhex(b)) for a, b in (ln.split() for ln in rule_out[3:84])]).reshape(9, 9)
    assert np.abs(host - inv).max() <= 1e-13 * np.abs(inv).max() and np.abs(A @ host - np.eye(9)).max() <= 1e-13
    want_t = imp.facet_term(75.2, 0.43, 4e-4, 0.013, 2.5e-3, -0.011, 0.61)
    assert abs(float.fromhex(rule_out[84]) - want_t) <= 4 * math.ulp(abs(want_t))


# ---- units ---------------------------------------------------------------------------------------------------------------------------
def test_unit_conversions_of_the_pore():
    """sigma of the frequency whose period is 2 pi time steps is the driver's model.inv_dt (PoreParameters: inv_dt = 1 / dt, dt =
    time_step / time_constant); one row of the spectrum by hand: the library's sums over the wall become wall means."""
    from gmpnp_amd.params import pore_parameters
    pp = pore_parameters(concentration_elec=0.5, L=10e-9, R=5e-9)
    f_step = 1.0 / (2.0 * math.pi * pp.time_step)
    assert abs(imp.pore_sigma_from_frequency(pp, f_step) - pp.model.inv_dt) <= 4e-16 * pp.model.inv_dt
    assert abs(pp.model.inv_dt - pp.time_constant / pp.time_step) <= 4e-16 * pp.model.inv_dt
    eps_0, area = 8.8541878128e-12, 3.2
    res = {"sigma": np.array([3.0]), "C": np.array([4.0e2 - 2.0e1j]), "dI": np.array([[-0.1 + 0.01j, -0.02 + 0.0j]]), "residual": np.array([1e-15]),
           "status": np.array([0], dtype=np.int32)}
    sp_ = imp.pore_spectrum(pp, eps_0, area, [50.0], res)
    cap = eps_0 / pp.L * (4.0e2 - 2.0e1j) / area
    Y = 1j * 2.0 * math.pi * 50.0 * cap + (0.12 - 0.01j) / area / pp.thermal_voltage
    assert abs(sp_["capacitance"][0] - cap) <= 1e-15 * abs(cap)
    assert np.allclose(sp_["dI_dV"][0], np.array([-0.1 + 0.01j, -0.02]) / area / pp.thermal_voltage, rtol=1e-15, atol=0.0)
    assert abs(sp_["admittance"][0] - Y) <= 1e-15 * abs(Y) and abs(sp_["impedance"][0] * Y - 1.0) <= 1e-15
    assert sp_["admittance"][0].real > 0.0          # cathodic currents are positive: -dI/dV is a conductance


# ---- refusals of the Python layer and the command line -----------------------------------------------------------------------------
def test_python_refusals_and_command_line():
    from gmpnp_amd import backend, edl1d, edl_ensemble, edl_sweep, pore3d, pore_ensemble, rxndiff1d, rxnpore3d, sweep
    want = dict(freq_min=1.0, freq_max=1e3, per_decade=2)
    calls = {
        "no electrode voltage": lambda: pore3d.PoreRun(pore_impedance=want),
        "partitions": lambda: pore3d.PoreRun(electrode_voltage=-1.0, partition=(2, None), pore_impedance=want),
        "multilevel": lambda: pore3d.PoreRun(electrode_voltage=-1.0, multilevel=True, refine=1, pore_impedance=want),
        "device glue": lambda: pore3d.PoreRun(electrode_voltage=-1.0, glue="device", pore_impedance=want),
        "bad grid": lambda: pore3d.PoreRun(electrode_voltage=-1.0, pore_impedance=dict(freq_min=-1.0)),
        "EDLRun": lambda: edl1d.EDLRun(electrode_voltage=-5.0, pore_impedance=want),
        "rxn 1D": lambda: rxndiff1d.RxnDiffRun(pore_impedance=want),
        "rxn 3D": lambda: rxnpore3d.RxnPoreRun(pore_impedance=want),
        "EDLEnsemble": lambda: edl_ensemble.EDLEnsemble([dict(voltage_multiplier=-1.0), dict(voltage_multiplier=-1.0, pore_impedance=want)]),
        "PoreEnsemble": lambda: pore_ensemble.PoreEnsemble([dict(pore_impedance=want)]),
        "edl sweep": lambda: edl_sweep.run_sweep([dict(pore_impedance=want)]),
        "edl sweep keywords": lambda: edl_sweep.run_sweep([dict(voltage_multiplier=-1.0)], pore_impedance=want),
        "pore sweep job": lambda: sweep.run_job(5, -1.0, 1, pore_impedance=want),
        "pore sweep group": lambda: sweep.run_group(5, [-1.0], 1, pore_impedance=want),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError, match="pore_impedance"):
            call()
    with pytest.raises(ValueError, match=r"impedance \(--impedance\)"):      # the 1D driver points to its own keyword
        edl1d.EDLRun(electrode_voltage=-5.0, pore_impedance=want)
    with pytest.raises(ValueError, match="impedance"):                        # the 1D keyword stays refused in the pore driver
        pore3d.PoreRun(electrode_voltage=-1.0, impedance=want)
    p = pore3d.build_parser()
    a = p.parse_args([])
    assert a.pore_impedance is False and imp.pore_impedance_keywords(a) == {}
    a = p.parse_args(["--pore_impedance"])
    assert imp.pore_impedance_keywords(a) == {"pore_impedance": dict(freq_min=1e-2, freq_max=1e8, per_decade=10)}
    a = p.parse_args(["--pore_impedance", "--freq_min", "1", "--freq_max", "1e4", "--freq_per_decade", "3"])
    assert imp.pore_impedance_keywords(a) == {"pore_impedance": dict(freq_min=1.0, freq_max=1e4, per_decade=3)}
    with pytest.raises(SystemExit):
        p.parse_args(["--impedance"])
    assert not any(s.startswith("--impedance") for act in p._actions for s in act.option_strings)
    with pytest.raises(ValueError, match="pore_impedance"):
        pore3d.main(["--pore_impedance"])
    assert "gmpnp_frequency_response_3d" in backend.EXPORTS and hasattr(backend.DeviceSolver, "frequency_response_3d")
