"""The small-signal frequency response of the 3D pore on the device (``gmpnp_frequency_response_3d``): the complex
block-banded LU against splu on the device's own K = jacobian_csr at inv_dt = 0 and b = galvanostat_terms, the functionals against the
NumPy rule on the device's own x, the bits across batching, calls and chunking, both ends of the spectrum, the handle after a call,
every refusal and the driver.

Shapes: generated cylinders ``coarse`` = (rings, layers) — (1, 1): 14 vertices, fewer than one panel of 16 block rows and a stored
band wider than the matrix; (1, 2): 21, a full panel and a partial one; (1, 15): 112, seven whole panels; (2, 3): 76; (3, 6): 259, the
'cyl259' of the other suites — and the L_10_R_5 mesh once (more than 256 boundary nodes, Dirichlet rows on the wall).  Random state,
two Tafel reactions, Stern BDM, p_M = -1, sigma in {0, 1, 1e2, 1e4, 1e6, 1e14}.  On the CPU K is regular on every shape and the
reference's own refined error stays below 1e-8 (the largest: 1.6e-8 at sigma = 0 on (3, 6)), so no shape was replaced.  (1, 1) has
every wall potential on a rim: its C is 0 and only the currents respond."""
import copy
import json
import os

import numpy as np
import pytest

import pore_response_reference as P
from conftest import random_state
from gmpnp_amd import impedance as imp
from gmpnp_amd.problem import Galvanostat, SternLayer
from gmpnp_amd.stern import L_STERN

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
CYLINDERS = {"c1x1": (1, 1), "c1x2": (1, 2), "c1x15": (1, 15), "c2x3": (2, 3), "c3x6": (3, 6)}
PORE10_SIGMAS = (0.0, 1e2, 1e14)
PORE10_SPLU = (1e2,)           # the sigma of L_10_R_5 that is compared with splu: one complex factorisation takes about ten seconds
P_M = -1.0
NEWTON = {"newton_solver": {"linear_solver": "band_lu", "maximum_iterations": 3, "relative_tolerance": 1e-30, "absolute_tolerance": 1e-30}}


def problem_of(name, pore10):
    if name != "pore10":
        return P.cylinder_case(CYLINDERS[name], p_M=P_M)
    from test_kinetics_reference import two_reactions
    from gmpnp_amd.problem import pore_problem
    pp, mesh = pore10[0], pore10[1]
    prob, _ = pore_problem(pp, mesh, stern=SternLayer("BDM", P_M, L_STERN / pp.L))
    prob = copy.copy(prob)
    prob.kinetics = two_reactions(list(prob.model.species), P_M)
    return prob


def same_bits(a, b, ka=None, kb=None):
    """Every array of two results (or of entry ka of a and kb of b) is bitwise equal."""
    return all(np.ascontiguousarray(a[q] if ka is None else a[q][ka]).tobytes() == np.ascontiguousarray(b[q] if kb is None else b[q][kb]).tobytes()
               for q in a)


_RESULTS = {}


def results(name, gpu_lib, pore10):
    """Everything one shape needs from the device and from the CPU, computed once: the call with every sigma, a second call, the
    single calls, the device's K and b, splu's and the refined solutions on them."""
    if name in _RESULTS:
        return _RESULTS[name]
    prob = problem_of(name, pore10)
    nv = prob.coords.shape[0]
    u, un = random_state(nv, prob.nf - 1, seed=3)
    sigmas = PORE10_SIGMAS if name == "pore10" else P.SIGMAS
    with gpu_lib.DeviceSolver(prob) as dev:
        dev.set_state(u, un)
        res = dev.frequency_response_3d(sigmas, want_x=True)
        again = dev.frequency_response_3d(sigmas, want_x=True)
        singles = [dev.frequency_response_3d([sg], want_x=True) for sg in sigmas]
        dev.set_time_step(0.0)
        dev.assemble(True)
        K = dev.jacobian_csr()
        tan = dev.electrode_tangent([0])
        dev.set_galvanostat(Galvanostat(1.0))
        b = dev.galvanostat_terms()[0]
        dev.set_galvanostat(None)
    M = P.mass(prob)
    # (the real 2N system of L_10_R_5 takes splu minutes; one complex splu of its N system about ten seconds: one sigma has one)
    if name != "pore10":
        ref = [P.solve(K, M, b, sg, "both") for sg in sigmas]
    else:
        ref = [P.solve_complex(K, M, b, sg) if sg in PORE10_SPLU else None for sg in sigmas]
    _RESULTS[name] = dict(prob=prob, u=u, sigmas=sigmas, res=res, again=again, singles=singles, K=K, M=M, b=b, tan=tan, ref=ref)
    return _RESULTS[name]


SHAPES = list(CYLINDERS) + ["pore10"]


@pytest.mark.parametrize("name", list(CYLINDERS))
def test_solution_against_splu_on_the_devices_own_system(name, gpu_lib, pore10):
    """x against the extended-precision refinement of splu's solution of the device's own (K + i sigma M) x = -b: the device's forward
    error is at most 10 times splu's own (floor 1e-13), its extended-precision residual at most 10 times splu's (floor 1e-14), and the
    reported residual is the extended-precision one within the rounding of its fp64 evaluation.  No status bit."""
    d = results(name, gpu_lib, pore10)
    res = d["res"]
    assert not res["status"].any() and np.array_equal(res["sigma"], np.asarray(d["sigmas"]))
    for k, sg in enumerate(d["sigmas"]):
        xr, xs = d["ref"][k]
        x = res["x"][k]
        e_dev, e_splu = float(np.abs(x - xr).max() / np.abs(xr).max()), float(np.abs(xs - xr).max() / np.abs(xr).max())
        r_dev, rounding = P.residual(d["K"], d["M"], d["b"], sg, x)
        r_splu = P.residual(d["K"], d["M"], d["b"], sg, xs)[0]
        print("%s sigma %g: x against the refined solution %.2e (splu %.2e), residual %.2e (splu %.2e, reported %.2e, rounding %.1e)" %
              (name, sg, e_dev, e_splu, r_dev, r_splu, res["residual"][k], rounding))
        assert e_dev <= max(10.0 * e_splu, 1e-13), (name, sg)
        assert r_dev <= max(10.0 * r_splu, 1e-14), (name, sg)
        assert abs(res["residual"][k] - r_dev) <= rounding, (name, sg)


def test_pore10_against_splu(gpu_lib, pore10):
    """L_10_R_5 (1767 vertices): more boundary nodes than one workgroup has lanes and Dirichlet rows on wall vertices.  At sigma = 1e2
    the cylinders' bounds against one complex splu of the N system (refined in extended precision): forward error at most 10 times
    splu's own (floor 1e-13), extended-precision residual at most 10 times splu's (floor 1e-14).  That factorisation is what this
    test's ten seconds go to (the mesh is short and wide: no ordering brings it to a few seconds), as in the 3D tangent's test against
    splu.  At every sigma the reported residual is the extended-precision one within the rounding of its fp64 evaluation."""
    from kinetics_reference import boundary_weights
    d = results("pore10", gpu_lib, pore10)
    nodes, _ = boundary_weights(d["prob"])
    assert len(nodes) > 256 and np.isin(np.asarray(d["prob"].bc_dofs) // d["prob"].nf, nodes).any()
    assert not d["res"]["status"].any()
    for k, sg in enumerate(d["sigmas"]):
        x = d["res"]["x"][k]
        r_dev, rounding = P.residual(d["K"], d["M"], d["b"], sg, x)
        print("pore10 sigma %g: residual %.2e (reported %.2e, rounding %.1e)" % (sg, r_dev, d["res"]["residual"][k], rounding))
        assert abs(d["res"]["residual"][k] - r_dev) <= rounding, sg
        if d["ref"][k] is None:
            continue
        xr, xs = d["ref"][k]
        e_dev, e_splu = float(np.abs(x - xr).max() / np.abs(xr).max()), float(np.abs(xs - xr).max() / np.abs(xr).max())
        r_splu = P.residual(d["K"], d["M"], d["b"], sg, xs)[0]
        print("pore10 sigma %g: x against the refined solution %.2e (splu %.2e), residual splu %.2e" % (sg, e_dev, e_splu, r_splu))
        assert e_dev <= max(10.0 * e_splu, 1e-13), sg
        assert r_dev <= max(10.0 * r_splu, 1e-14), sg


@pytest.mark.parametrize("name", SHAPES)
def test_functionals_against_the_numpy_rule(name, gpu_lib, pore10):
    """C and dI_r against the NumPy rule applied facet by facet to the device's own x (pore_response_reference.functionals): 1e-12
    relative plus 64 eps of the sum of the absolute values of the terms (a sum taken in another order), real and imaginary parts."""
    d = results(name, gpu_lib, pore10)
    for k, sg in enumerate(d["sigmas"]):
        C, dI, (aCr, aIr, aCi, aIi) = P.functionals(d["prob"], d["u"], d["res"]["x"][k], want_scale=True)
        gC, gI = d["res"]["C"][k], d["res"]["dI"][k]
        print("%s sigma %g: C %r (rule %r), dI %s (rule %s)" % (name, sg, complex(gC), C, gI, dI))
        assert abs(gC.real - C.real) <= 1e-12 * abs(C.real) + 64 * EPS * aCr and abs(gC.imag - C.imag) <= 1e-12 * abs(C.imag) + 64 * EPS * aCi
        assert np.all(np.abs(gI.real - dI.real) <= 1e-12 * np.abs(dI.real) + 64 * EPS * aIr)
        assert np.all(np.abs(gI.imag - dI.imag) <= 1e-12 * np.abs(dI.imag) + 64 * EPS * aIi)


@pytest.mark.parametrize("name", SHAPES)
def test_bits_do_not_depend_on_the_batch_or_on_the_call(name, gpu_lib, pore10):
    d = results(name, gpu_lib, pore10)
    assert same_bits(d["res"], d["again"])
    for k in range(len(d["sigmas"])):
        assert same_bits(d["res"], d["singles"][k], k, 0), (name, k)


@pytest.mark.parametrize("name", SHAPES)
def test_both_ends_of_the_spectrum(name, gpu_lib, pore10):
    """C(0) and dI(0) against electrode_tangent([0]) of the same handle at inv_dt = 0 (two solvers on one system): 1e-8.  C(1e14)
    against the potential block of the device's K: within 10 times the reference's own error, floor 1e-9 (the bound the CPU test
    measures; on these shapes the reference's own error is below the floor)."""
    d = results(name, gpu_lib, pore10)
    res, tan = d["res"], d["tan"]
    assert res["C"][0].imag == 0.0 and not np.any(res["dI"][0].imag)
    print("%s: C(0) %.12g tangent %.12g, dI(0) %s tangent %s" % (name, res["C"][0].real, tan["dD"][0], res["dI"][0].real, tan["dI"][0]))
    assert abs(res["C"][0].real - tan["dD"][0]) <= 1e-8 * abs(tan["dD"][0])
    assert np.all(np.abs(res["dI"][0].real - tan["dI"][0]) <= 1e-8 * np.abs(tan["dI"][0]))
    k = list(d["sigmas"]).index(1e14)
    closed, _ = P.potential_block_capacitance(d["prob"], d["u"], d["K"], d["b"])
    own = 0.0      # (L_10_R_5 has no splu at this sigma: its bound is the floor, which no measured error of the reference can lower)
    if d["ref"][k] is not None:
        xr, xs = d["ref"][k]
        Cr, Cs = P.functionals(d["prob"], d["u"], xr)[0], P.functionals(d["prob"], d["u"], xs)[0]
        own = abs(Cs - Cr) / abs(Cr) if abs(Cr) > 0.0 else 0.0
    print("%s: C(1e14) %r, potential block %.12g, reference's own error %.2e" % (name, complex(res["C"][k]), closed, own))
    assert abs(res["C"][k] - closed) <= max(10.0 * own, 1e-9) * abs(closed)


def test_chunks_of_two_equal_one_chunk(gpu_lib, pore10):
    """A memory cap of 2.5 bands forces chunks of 2 frequencies: the bits are those of one chunk.  A cap below one band is refused
    with the size in the message; the band width the cap is computed from is gmpnp_band_lu_shape's."""
    d = results("c1x2", gpu_lib, pore10)
    prob, u = d["prob"], d["u"]
    with gpu_lib.DeviceSolver(prob, band_lu_max_gb=1e-9) as tiny:
        tiny.set_state(u, u)
        n_blocks, band = tiny.band_lu_shape()
        with pytest.raises(gpu_lib.GmpnpError, match=r"frequency response.*GB \(%d node blocks, band %d\)" % (n_blocks, band)) as ei:
            tiny.frequency_response_3d([1.0])
        assert ei.value.code == gpu_lib.ERR_INVALID
    assert n_blocks == 21 and 15 <= band <= 20
    per = imp.band_bytes_per_frequency(21, band, 9)
    assert imp.band_chunk(6, 21, band, 9, 2.5 * per) == 2
    with gpu_lib.DeviceSolver(prob, band_lu_max_gb=2.5 * per / 1e9) as dev:
        dev.set_state(u, random_state(21, prob.nf - 1, seed=3)[1])
        got = dev.frequency_response_3d(P.SIGMAS, want_x=True)
        assert dev.time_kernel(30, 1) > 0.0
    assert same_bits(d["res"], got)


def test_the_handle_is_left_as_it_was(gpu_lib, pore10):
    """After a call F, jacobian_csr, the state and the next newton_solve (band LU) are bitwise those of a twin handle that never made
    the call, with a valid Jacobian before the call and without one (there is none afterwards either)."""
    prob = P.cylinder_case((2, 3), p_M=P_M)
    un = np.tile(np.r_[np.ones(prob.nf - 1), 0.0], prob.coords.shape[0])
    u = un + 1e-3 * np.random.default_rng(5).standard_normal(prob.ndof) * (np.arange(prob.ndof) % prob.nf != prob.nf - 1)
    opts = gpu_lib.newton_options(NEWTON, dim=3)
    with gpu_lib.DeviceSolver(prob) as a, gpu_lib.DeviceSolver(prob) as twin, gpu_lib.DeviceSolver(prob) as c:
        for dev in (a, twin, c):
            dev.set_state(u, un)
        Fa, Ft = a.assemble(True)[0], twin.assemble(True)[0]
        assert np.array_equal(Fa, Ft)
        res = a.frequency_response_3d(P.SIGMAS)
        assert not res["status"].any()
        assert np.array_equal(a.jacobian_csr().data, twin.jacobian_csr().data)
        assert np.array_equal(a.assemble(False)[0], twin.assemble(False)[0]) and np.array_equal(a.get_state(), twin.get_state())
        sa, st = a.newton_solve(opts, error_on_nonconvergence=False), twin.newton_solve(opts, error_on_nonconvergence=False)
        assert sa["iterations"] == st["iterations"] == 3 and sa["residuals"] == st["residuals"]
        assert np.array_equal(a.get_state(), twin.get_state())
        again = a.frequency_response_3d([1e2])           # after the real band LU has been used: both live side by side
        assert again["status"][0] == 0
        sa, st = a.newton_solve(opts, error_on_nonconvergence=False), twin.newton_solve(opts, error_on_nonconvergence=False)
        assert sa["residuals"] == st["residuals"] and np.array_equal(a.get_state(), twin.get_state())
        c.frequency_response_3d([1.0, 1e6])
        with pytest.raises(gpu_lib.GmpnpError, match="no Jacobian"):
            c.jacobian_csr()


def test_library_refusals_and_hook_30(pore10, gpu_lib):
    """Every refusal of gmpnp_frequency_response_3d is GMPNP_ERR_INVALID and names the frequency response: a 1D handle (sent to
    gmpnp_frequency_response), a partition handle, a multilevel level, the Stern option off, the galvanostat on (off again: accepted,
    same bits), two electrode potentials, n = 0 and 4097, a negative, infinite or NaN sigma.  Hook 30 needs a call first, then times
    one chunk and leaves the state, F and the Jacobian alone."""
    from test_kinetics_reference import _edl_k, first_step_problem
    from gmpnp_amd import dist
    from gmpnp_amd.problem import pore_hierarchy
    from gmpnp_amd.solver import GMPNPSystem
    pp, mesh, prob3, _ = pore10

    def refused(call, what="frequency response"):
        with pytest.raises(gpu_lib.GmpnpError, match=what) as ei:
            call()
        assert ei.value.code == gpu_lib.ERR_INVALID

    dom, perm, part = dist.partition_plan(prob3, 2, 0)
    with gpu_lib.DeviceSolver(dom.problem, perm=perm, partition=part) as partitioned:
        refused(lambda: partitioned.frequency_response_3d([1.0]))
    levels = pore_hierarchy(pp, mesh, 1)
    ml = GMPNPSystem(levels[0][0], levels=levels)
    try:
        refused(lambda: ml.dev.frequency_response_3d([1.0]))
        refused(lambda: ml._coarse[0].frequency_response_3d([1.0]))
    finally:
        ml.close()
    ep, m1 = _edl_k()
    with gpu_lib.DeviceSolver(first_step_problem(ep, m1, -5.0)) as d1:
        refused(lambda: d1.frequency_response_3d([1.0]), "gmpnp_frequency_response")
    prob = P.cylinder_case((1, 2), p_M=P_M)
    plain = copy.copy(prob)
    plain.stern, plain.kinetics = None, None
    u, un = random_state(21, prob.nf - 1, seed=3)
    with gpu_lib.DeviceSolver(plain) as a, gpu_lib.DeviceSolver(prob) as b:
        a.set_state(u, un)
        b.set_state(u, un)
        refused(lambda: a.frequency_response_3d([1.0]))                      # the Stern option is off
        refused(lambda: b.time_kernel(30, 1), "30")                          # no call yet
        refused(lambda: b.frequency_response_3d([]))
        refused(lambda: b.frequency_response_3d(np.ones(gpu_lib.RESPONSE_MAX_FREQUENCIES + 1)))
        for bad in (-1.0, float("inf"), float("nan")):
            refused(lambda: b.frequency_response_3d([1.0, bad]))
        before = b.frequency_response_3d([1.0, 1e4])
        b.set_galvanostat(Galvanostat(1.0))
        refused(lambda: b.frequency_response_3d([1.0]))
        b.set_galvanostat(None)                                              # keeps the potential (5j): the same operating point
        after = b.frequency_response_3d([1.0, 1e4])
        assert same_bits(before, after)
        b.set_stern(SternLayer("BDM", P_M + 1.0, L_STERN / 10e-9))
        refused(lambda: b.frequency_response_3d([1.0]))                      # two electrode potentials
        b.set_stern(prob.stern)
        F0 = b.assemble(True)[0]
        J0 = b.jacobian_csr().data.copy()
        u_before = b.get_state()
        assert b.time_kernel(30, 2) > 0.0
        assert np.array_equal(b.get_state(), u_before) and np.array_equal(b.jacobian_csr().data, J0) and np.array_equal(b.assemble(False)[0], F0)
        assert same_bits(before, b.frequency_response_3d([1.0, 1e4]))
        b.set_kinetics(None)                                                 # the Stern option alone: no currents, the same C path
        alone = b.frequency_response_3d([1.0, 1e4])
        assert not np.any(alone["dI"]) and not alone["status"].any() and np.all(alone["C"].real > 0.0)


def test_driver_writes_the_spectrum(tmp_path, monkeypatch, gpu_lib):
    """Two PoreRun steps on L_10_R_5 with Tafel kinetics and a 4-point grid: pore_impedance.npz holds, bit for bit, what
    PoreRun.pore_impedance returns at the last state, and that is pore_spectrum's statement of the library's raw response over the run's
    wall area.  The reported residuals are the extended-precision ones of the device's x on the device's own K and b within the
    rounding of their fp64 evaluation; at the first frequency the residual is at most 10 times that of one complex splu of the same
    system (floor 1e-14), the bound of the accuracy tests above.  The metadata keys are there."""
    from gmpnp_amd.pore3d import SOLVER_PARAMETERS, PoreRun
    monkeypatch.setenv("GMPNP_OUT", str(tmp_path))
    grid = dict(freq_min=1e2, freq_max=1e5, per_decade=1)
    sp = {"nonlinear_solver": "newton", "newton_solver": dict(SOLVER_PARAMETERS["newton_solver"], linear_solver="band_lu")}
    run = PoreRun(num_steps=2, solver_parameters=sp, electrode_voltage=-1.0, L=10e-9, R=5e-9, concentration_elec=0.5, kinetics="tafel", i0_CO=10.0, i0_H2=1.0,
                  pore_impedance=grid)
    try:
        run.run(verbose=False)
        path = run.write_outputs(stamp="pore_spectrum")
        got = run.pore_impedance(imp.frequency_grid(**grid))
        dev = run.sys.dev
        raw = dev.frequency_response_3d(got["sigma"], want_x=True)
        area = run.wall_area()
        inv_dt = float(run.sys.problem.model.inv_dt)
        run.sys.set_time_step(0.0)
        dev.assemble(True)
        K = dev.jacobian_csr()
        dev.set_galvanostat(Galvanostat(1.0))
        b = dev.galvanostat_terms()[0]
        dev.set_galvanostat(None)
        run.sys.set_time_step(inv_dt)
        M = P.mass(run.problem)
    finally:
        run.sys.close()
    # the spectrum is the raw response over the wall area (sums over 1152 wall facets become wall means), in physical units
    from gmpnp_amd.params import _load_yaml, utilities_dir
    eps_0 = _load_yaml(os.path.join(utilities_dir(), "parameters_pore.yaml"))["nat_const"]["eps_0"]
    assert raw["residual"].tobytes() == got["residual"].tobytes() and abs(area - np.pi) < 0.05 * np.pi      # 2 pi (R / L) x 1, R / L = 0.5
    assert np.all(np.abs(got["capacitance"] - eps_0 / run.pp.L * raw["C"] / area) <= 4 * EPS * np.abs(got["capacitance"]))
    assert np.all(np.abs(got["dI_dV"] - raw["dI"] / area / run.pp.thermal_voltage) <= 4 * EPS * np.abs(got["dI_dV"]))
    for k, sg in enumerate(got["sigma"]):
        r_dev, rounding = P.residual(K, M, b, sg, raw["x"][k])
        print("driver sigma %g: residual %.2e (reported %.2e, rounding %.1e)" % (sg, r_dev, raw["residual"][k], rounding))
        assert abs(raw["residual"][k] - r_dev) <= rounding, sg
    xs = P.solve_complex(K, M, b, got["sigma"][0])[1]
    r0, r_splu = P.residual(K, M, b, got["sigma"][0], raw["x"][0])[0], P.residual(K, M, b, got["sigma"][0], xs)[0]
    print("driver sigma %g: residual %.2e, splu %.2e" % (got["sigma"][0], r0, r_splu))
    assert r0 <= max(10.0 * r_splu, 1e-14)
    z = np.load(os.path.join(path, "pore_impedance.npz"))
    assert sorted(z.files) == sorted(["frequency", "sigma", "capacitance", "admittance", "impedance", "dI_CO", "dI_H2", "residual"])
    assert len(z["frequency"]) == 4 and np.array_equal(z["sigma"], imp.pore_sigma_from_frequency(run.pp, z["frequency"]))
    for key in ("frequency", "sigma", "capacitance", "admittance", "impedance", "residual"):
        assert z[key].tobytes() == got[key].tobytes(), key
    assert z["dI_CO"].tobytes() == np.ascontiguousarray(got["dI_dV"][:, 0]).tobytes() and z["dI_H2"].tobytes() == np.ascontiguousarray(got["dI_dV"][:, 1]).tobytes()
    print("driver: Z %s residual %s" % (z["impedance"].tolist(), z["residual"].tolist()))
    assert np.all(z["impedance"].real > 0.0)
    meta = json.load(open(os.path.join(path, "metadata.json")))
    for key in ("pore_impedance_points", "pore_impedance_status", "capacitance_low", "capacitance_high", "capacitance_high_closed_form", "R_ct",
                "pore_impedance_last_step_change"):
        assert key in meta, key
    print("driver: metadata %s" % {k: meta[k] for k in meta if "capacitance" in k or "impedance" in k or k == "R_ct"})
    assert meta["pore_impedance_points"] == 4 and meta["pore_impedance_status"] == 0
    assert meta["capacitance_low"] == z["capacitance"][0].real and meta["capacitance_high"] == z["capacitance"][-1].real
    assert 0.0 < meta["capacitance_high_closed_form"] <= meta["capacitance_high"] < meta["capacitance_low"]
    assert abs(meta["R_ct"] - 1.0 / (-(z["dI_CO"][0] + z["dI_H2"][0]).real)) <= 1e-12 * meta["R_ct"] and meta["R_ct"] > 0.0
