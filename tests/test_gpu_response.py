"""The small-signal frequency response on the GPU (gmpnp_frequency_response, csrc/gmpnp_response.h) against the
NumPy restatement of tests/response_reference.py: x, C, dI and the residual on uniform meshes of 2, 3, 9, 64 and 65 vertices and on
the 1 um mesh (1091 vertices) at sigma in {0, 1, 1e2, 1e4, 1e6, 1e14}, once one frequency per call and once 70 per call; equal bits
across n, across calls and across chunkings; the two limits of the spectrum on the device; the handle left as it was; the kinetics
off; every refusal of the library; hook 27; the driver's impedance.npz.  Every handle is closed by `with` / `finally`."""
import ctypes
import json
import os

import numpy as np
import pytest

import hp_reference as H
import kinetics_reference as K
import response_reference as R
import stern_bc_reference as SR
from conftest import random_state
from step_limit_reference import first_step_state
from test_gpu_kinetics import edl_k  # noqa: F401 (fixture)
from test_kinetics_reference import TAFEL, first_step_problem, two_reactions
from gmpnp_amd import impedance as imp
from gmpnp_amd.params import edl_parameters
from gmpnp_amd.problem import Galvanostat, SternLayer, edl_problem
from gmpnp_amd.stern import L_STERN

pytestmark = pytest.mark.gpu
P_M = -5.0
SIGMAS = (0.0, 1.0, 1e2, 1e4, 1e6, 1e14)
N_MANY = 70                               # more than one wave of 8-lane groups, and not a multiple of anything
MANY = np.array([SIGMAS[k % len(SIGMAS)] for k in range(N_MANY)])
CASES = ("uniform2", "uniform3", "uniform9", "uniform64", "uniform65", "edl1")
STEADY = {"newton_solver": {"maximum_iterations": 50, "relative_tolerance": 1e-13, "absolute_tolerance": 1e-7}}


def generated_problem(nv, kinetics=True):
    """hp_reference.edl_generated's parameters on a uniform mesh, with a Stern layer and two reactions set on the problem."""
    ep = edl_parameters(cation="Cs", voltage_multiplier=-10.0)
    kin = two_reactions(ep.species, P_M) if kinetics else None
    return edl_problem(ep, H.uniform_mesh_1d(nv), stern=SternLayer("BDM", P_M, L_STERN / ep.L_n), kinetics=kin)


@pytest.fixture(scope="module")
def inputs(edl_k):
    """name -> (problem, u): a random state on the generated meshes, the steady state (NumPy Newton at inv_dt = 0) on the 1 um mesh."""
    out = {}
    for nv in (2, 3, 9, 64, 65):
        out["uniform%d" % nv] = (generated_problem(nv), random_state(nv, 6, seed=nv)[0])
    ep, mesh = edl_k
    prob = first_step_problem(ep, mesh, P_M)
    u1, st = K.newton_loop(prob, *first_step_state(prob))
    assert st.converged
    out["edl1"] = (prob, R.steady_state(prob, u1)[0])
    return out


def errors(x, C, dI, ref):
    xr, Cr, dIr = ref
    return (float(np.abs(x - xr).max() / np.abs(xr).max()), float(abs(C - Cr) / abs(Cr)),
            float(np.abs(np.asarray(dI) - dIr).max() / np.abs(dIr).max()) if len(dIr) else 0.0)


def device_system(gpu_lib, prob, u):
    """(System, vertex order) of the linearisation on the DEVICE'S OWN numbers, as test_gpu_shapes.py measures its limits on the device's
    own Jacobian: K = jacobian_csr of a handle whose model has inv_dt = 0, b = gmpnp_galvanostat_terms' b where the kinetics are on (the
    galvanostat is switched on for that one call; p_M stays), M from the mesh.  K and b of the NumPy assembly differ from these in the
    last bits, which the conditioning of K turns into the 1e-9 of x that separates two correct solvers."""
    with gpu_lib.DeviceSolver(R.with_inv_dt(prob, 0.0)) as dev:
        dev.set_state(u, u)
        dev.assemble(True)
        Kd = dev.jacobian_csr()
        order = np.array(dev.perm, dtype=np.int64)
        if prob.kinetics is not None:
            dev.set_galvanostat(Galvanostat(1.0))
            b = dev.galvanostat_terms()[0]
            dev.set_galvanostat(None)
        else:
            b = R.rhs_b(prob, u)
    Sn = R.system(prob, u)
    assert abs(Kd - Sn.K).max() <= 1e-12 * abs(Sn.K).max() and np.abs(b - Sn.b).max() <= 1e-12 * np.abs(Sn.b).max()
    return R.System(prob, np.asarray(u, dtype=np.float64), Kd.tocsr(), Sn.M, b), order


@pytest.fixture(scope="module")
def device_results(inputs, gpu_lib):
    """name -> what the device returned: one call per sigma with n = 1, two calls with n = 70, one with n = 70 under a memory cap that
    makes chunks of 8 frequencies; and the system the references are computed on.  One handle per case, closed before the tests look."""
    out = {}
    for name, (prob, u) in inputs.items():
        nv = prob.coords.shape[0]
        cap_mb = 9.5 * imp.bytes_per_frequency(nv) / 2 ** 20
        assert imp.chunk(N_MANY, nv, cap_mb * 2 ** 20) == 8
        with gpu_lib.DeviceSolver(prob) as dev:
            dev.set_state(u, u)
            single = [dev.frequency_response([sg], want_x=True) for sg in SIGMAS]
            many = dev.frequency_response(MANY, want_x=True)
            again = dev.frequency_response(MANY, want_x=True)
            os.environ["GMPNP_RESPONSE_CAP_MB"] = repr(cap_mb)
            try:
                chunked = dev.frequency_response(MANY, want_x=True)
            finally:
                del os.environ["GMPNP_RESPONSE_CAP_MB"]
        out[name] = dict(single=single, many=many, again=again, chunked=chunked, system=device_system(gpu_lib, prob, u))
    return out


@pytest.fixture(scope="module")
def references(device_results):
    """name -> per sigma: the refined solution, the errors of plain splu and of the NumPy model of the device algorithm against it
    (x, C, dI), and splu's residual.  Computed once; the tests below share it."""
    out = {}
    for name, d in device_results.items():
        S, order = d["system"]
        rows = []
        for sg in SIGMAS:
            ref = R.response(S, sg)
            xs, Cs, dIs = R.response(S, sg, "splu")
            xt, Ct, dIt = R.response(S, sg, "thomas", order)
            rows.append(dict(ref=ref, splu=errors(xs, Cs, dIs, ref), model=errors(xt, Ct, dIt, ref), res_splu=R.relative_residual(S, sg, xs)))
        out[name] = (S, rows)
    return out


def same_bits(a, b):
    return all(np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes() for k in ("sigma", "C", "dI", "residual", "status", "x"))


@pytest.mark.parametrize("name", CASES)
def test_response_against_the_refined_reference(name, references, device_results):
    """x, C and dI of every sigma against the refined reference, all three on the device's own K and b (``device_system``).  The limit
    is measured per input as test_gpu_shapes.py does: 10x the error of plain splu (floor 1e-13), or 2x the error of the NumPy
    block-Thomas model of the same algorithm (operation for operation, the handle's vertex order) where that model is itself further off; a device result beyond 1e-7 fails whatever the model says.  The residual max |(K + i sigma M) x + b| / max |b| of the
    device's x, formed in extended precision: <= 10x that of splu, floor 1e-14; the figure the device reports agrees with it within the
    rounding of its own fp64 evaluation, 30 eps max (|A| |x| + |b|) / max |b| (22 products per row).  Status 0 everywhere."""
    S, rows = references[name]
    for k, (sg, row) in enumerate(zip(SIGMAS, rows)):
        got = device_results[name]["single"][k]
        assert got["status"][0] == 0 and got["sigma"][0] == sg and got["dI"].shape == (1, len(row["ref"][2]))
        x = got["x"][0]
        e = errors(x, got["C"][0], got["dI"][0], row["ref"])
        limits = [H.forward_limit(max(10.0 * s, 1e-13), m) for s, m in zip(row["splu"], row["model"])]
        res = R.relative_residual(S, sg, x)
        A = S.matrix(sg)
        rounding = 30 * np.finfo(float).eps * float((abs(A) @ np.abs(x) + np.abs(S.b)).max() / np.abs(S.b).max())
        print("%s sigma %g: x %.2e (splu %.2e model %.2e) C %.2e (%.2e %.2e) dI %.2e (%.2e %.2e) residual %.2e (splu %.2e, reported %.2e)"
              % (name, sg, e[0], row["splu"][0], row["model"][0], e[1], row["splu"][1], row["model"][1], e[2], row["splu"][2], row["model"][2],
                 res, row["res_splu"], got["residual"][0]))
        for what, v, lim in zip(("x", "C", "dI"), e, limits):
            assert v <= min(lim, 1e-7), (name, sg, what, v, lim)
        assert res <= max(10.0 * row["res_splu"], 1e-14), (name, sg, res)
        assert abs(got["residual"][0] - res) <= rounding, (name, sg, got["residual"][0], res, rounding)


@pytest.mark.parametrize("name", CASES)
def test_bits_do_not_depend_on_n_on_the_call_or_on_the_chunking(name, device_results):
    """Every frequency of the n = 70 call holds the bits of its n = 1 call; a second call and a call in chunks of 8 give the bits of
    the first."""
    d = device_results[name]
    for k in range(N_MANY):
        one = d["single"][k % len(SIGMAS)]
        for key in ("sigma", "C", "dI", "residual", "status", "x"):
            a, b = np.ascontiguousarray(d["many"][key][k]), np.ascontiguousarray(one[key][0])
            assert a.tobytes() == b.tobytes(), (name, k, key)
    assert same_bits(d["many"], d["again"]) and same_bits(d["many"], d["chunked"])


def test_both_ends_of_the_spectrum_on_the_device(inputs, device_results, gpu_lib):
    """C(1e14) is the closed form 1 / (lam / g + sum_e h_e / eps_e) within 1e-6, and C(0), dI_r(0) are the central differences of
    stern_displacement and kinetics_currents between two steady states at p_M -+ 1e-3 within 1e-6 (the truncation is O(delta^2)); the
    steady states come from gmpnp_newton_solve at inv_dt = 0."""
    prob, u = inputs["edl1"]
    got = device_results["edl1"]["single"]
    closed = R.high_frequency_closed_form(prob, u)
    print("C(1e14) = %r, closed form %.10g" % (got[-1]["C"][0], closed))
    assert abs(got[-1]["C"][0] - closed) <= 1e-6 * closed
    d = 1e-3
    opts = gpu_lib.newton_options(STEADY, dim=1)
    D, I = {}, {}
    with gpu_lib.DeviceSolver(R.with_inv_dt(prob, 0.0)) as dev:
        for s in (+1, -1):
            q = R.with_potential(prob, P_M + s * d)
            dev.set_stern(q.stern)
            dev.set_kinetics(q.kinetics)
            dev.set_state(u, u)
            st = dev.newton_solve(opts)
            assert st["converged"]
            D[s], I[s] = dev.stern_displacement(), dev.kinetics_currents()
        # the response at the operating point of THIS handle's own steady state
        q = R.with_potential(prob, P_M)
        dev.set_stern(q.stern)
        dev.set_kinetics(q.kinetics)
        dev.set_state(u, u)
        assert dev.newton_solve(opts)["converged"]
        at0 = dev.frequency_response([0.0])
    fdC, fdI = (D[1] - D[-1]) / (2 * d), (I[1] - I[-1]) / (2 * d)
    eC = abs(at0["C"][0].real - fdC) / abs(fdC)
    eI = np.abs(at0["dI"][0].real - fdI).max() / np.abs(fdI).max()
    print("zero frequency on the device: C %.10g (differences %.10g, %.2e), dI %s (%s, %.2e)" % (at0["C"][0].real, fdC, eC, at0["dI"][0].real, fdI, eI))
    assert eC < 1e-6 and eI < 1e-6 and at0["C"][0].imag == 0.0 and at0["status"][0] == 0


def test_the_handle_is_left_as_it_was(edl_k, gpu_lib):
    """After a call F, jacobian_csr and the next newton_solve are bitwise those of a twin handle that never made the call, with a
    valid Jacobian before the call (it is valid afterwards, with its bits) and without one (there is none afterwards either)."""
    ep, mesh = edl_k
    prob = first_step_problem(ep, mesh, P_M)
    u0, un = first_step_state(prob)
    u0 = un + 1e-3 * np.random.default_rng(5).standard_normal(prob.ndof) * (np.arange(prob.ndof) % prob.nf != prob.nf - 1)
    opts = gpu_lib.newton_options({"newton_solver": {"maximum_iterations": 50, "relative_tolerance": 1e-9, "absolute_tolerance": 1e-6}}, dim=1)
    with gpu_lib.DeviceSolver(prob) as a, gpu_lib.DeviceSolver(prob) as twin, gpu_lib.DeviceSolver(prob) as c:
        for dev in (a, twin, c):
            dev.set_state(u0, un)
        Fa, Ft = a.assemble(True)[0], twin.assemble(True)[0]
        assert np.array_equal(Fa, Ft)
        res = a.frequency_response(SIGMAS)
        assert not res["status"].any()
        assert np.array_equal(a.jacobian_csr().data, twin.jacobian_csr().data)
        assert np.array_equal(a.assemble(False)[0], twin.assemble(False)[0])
        sa, st = a.newton_solve(opts), twin.newton_solve(opts)
        assert sa["converged"] and sa["iterations"] == st["iterations"] > 0 and sa["residuals"] == st["residuals"]
        assert np.array_equal(a.get_state(), twin.get_state())
        # no Jacobian before the call: none afterwards, and the next solve is the twin's all the same
        c.frequency_response([1.0, 1e6])
        with pytest.raises(gpu_lib.GmpnpError, match="no Jacobian"):
            c.jacobian_csr()
        sc = c.newton_solve(opts)
        assert sc["iterations"] == st["iterations"] and sc["residuals"] == st["residuals"] and np.array_equal(c.get_state(), twin.get_state())


def test_kinetics_off_gives_no_currents_and_the_same_capacitance_path(gpu_lib):
    """The Stern option alone: dI is empty (the library's dI is zero), C and x meet the limits of the reference test."""
    prob = generated_problem(65, kinetics=False)
    u = random_state(65, 6, seed=65)[0]
    S, order = device_system(gpu_lib, prob, u)
    with gpu_lib.DeviceSolver(prob) as dev:
        dev.set_state(u, u)
        got = dev.frequency_response(SIGMAS, want_x=True)
        raw = (gpu_lib.CResponse * 1)()
        sg = np.array([1e4])
        dev._check(dev.lib.gmpnp_frequency_response(dev._h, 1, sg.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), raw, None))
    assert got["dI"].shape == (len(SIGMAS), 0) and not got["status"].any()
    assert all(raw[0].dI[r][q] == 0.0 for r in range(4) for q in range(2)) and raw[0].C[0] == got["C"][3].real
    for k, sg in enumerate(SIGMAS):
        ref = R.response(S, sg)
        xs, Cs, dIs = R.response(S, sg, "splu")
        xt, Ct, dIt = R.response(S, sg, "thomas", order)
        e, es, em = errors(got["x"][k], got["C"][k], [], ref), errors(xs, Cs, [], ref), errors(xt, Ct, [], ref)
        print("kinetics off, sigma %g: x %.2e (splu %.2e model %.2e) C %.2e (%.2e %.2e)" % (sg, e[0], es[0], em[0], e[1], es[1], em[1]))
        for v, s, m in zip(e[:2], es[:2], em[:2]):
            assert v <= min(H.forward_limit(max(10.0 * s, 1e-13), m), 1e-7)


def test_library_refusals_and_hook_27(pore10, edl_k, gpu_lib):
    """Every refusal of gmpnp_frequency_response is GMPNP_ERR_INVALID and names the frequency response: a partition handle, a
    multilevel level, a 3D handle, SUPG terms, the Stern option off, the galvanostat on (off again: accepted, at the potential it
    holds), two electrode potentials, n = 0 and 4097, a negative, infinite or NaN sigma.  Hook 27 needs a call first, then times one
    chunk and leaves the state and the Jacobian alone."""
    from gmpnp_amd import dist
    from gmpnp_amd.problem import pore_hierarchy
    from gmpnp_amd.solver import GMPNPSystem
    pp, mesh, prob3, _ = pore10
    ep, m1 = edl_k

    def refused(call, what="frequency response"):
        with pytest.raises(gpu_lib.GmpnpError, match=what) as ei:
            call()
        assert ei.value.code == gpu_lib.ERR_INVALID

    dom, perm, part = dist.partition_plan(prob3, 2, 0)
    with gpu_lib.DeviceSolver(dom.problem, perm=perm, partition=part) as partitioned:
        refused(lambda: partitioned.frequency_response([1.0]))
    levels = pore_hierarchy(pp, mesh, 1)
    ml = GMPNPSystem(levels[0][0], levels=levels)
    try:
        refused(lambda: ml.dev.frequency_response([1.0]))
        refused(lambda: ml._coarse[0].frequency_response([1.0]))
    finally:
        ml.close()
    with gpu_lib.DeviceSolver(prob3) as d3:
        refused(lambda: d3.frequency_response([1.0]))
    kin = two_reactions(ep.species, P_M)
    plain = edl_problem(ep, m1)
    both = edl_problem(ep, m1, stern=SternLayer("BDM", P_M, L_STERN / ep.L_n), kinetics=kin)
    stern_only = edl_problem(ep, m1, stern=SternLayer("BDM", P_M, L_STERN / ep.L_n))
    with gpu_lib.DeviceSolver(plain) as a, gpu_lib.DeviceSolver(both) as b, gpu_lib.DeviceSolver(stern_only) as c:
        u0, un = first_step_state(plain)
        for d in (a, b, c):
            d.set_state(un, un)
        refused(lambda: a.frequency_response([1.0]))                      # the Stern option is off
        refused(lambda: b.time_kernel(27, 1))                             # no call yet
        c.set_supg(np.full((m1.num_vertices, 6), 0.1))
        refused(lambda: c.frequency_response([1.0]))
        c.set_supg(None)
        assert c.frequency_response([1.0])["status"][0] == 0
        refused(lambda: b.frequency_response([]))
        refused(lambda: b.frequency_response(np.ones(gpu_lib.RESPONSE_MAX_FREQUENCIES + 1)))
        for bad in (-1.0, float("inf"), float("nan")):
            refused(lambda: b.frequency_response([1.0, bad]))
        before = b.frequency_response([1.0, 1e4])
        b.set_galvanostat(Galvanostat(10.0))
        refused(lambda: b.frequency_response([1.0]))
        b.set_galvanostat(None)                                           # keeps the potential (5j): the same operating point
        after = b.frequency_response([1.0, 1e4])
        assert np.array_equal(before["C"], after["C"]) and np.array_equal(before["dI"], after["dI"])
        b.set_stern(SternLayer("BDM", P_M + 1.0, L_STERN / ep.L_n))
        refused(lambda: b.frequency_response([1.0]))                      # two electrode potentials
        b.set_stern(SternLayer("BDM", P_M, L_STERN / ep.L_n))
        F0 = b.assemble(True)[0]
        J0 = b.jacobian_csr().data.copy()
        u_before = b.get_state()
        assert b.time_kernel(27, 2) > 0.0
        assert np.array_equal(b.get_state(), u_before) and np.array_equal(b.jacobian_csr().data, J0) and np.array_equal(b.assemble(False)[0], F0)
        again = b.frequency_response([1.0, 1e4])
        assert np.array_equal(again["C"], before["C"])


def test_driver_writes_the_spectrum(tmp_path, monkeypatch, gpu_lib):
    """EDLRun with ``impedance``: impedance.npz holds, bit for bit, what EDLRun.impedance returns at the last state, and the metadata
    names both capacitance limits, R_ct and how steady the operating point was."""
    from gmpnp_amd import edl1d
    monkeypatch.setenv("GMPNP_OUT", str(tmp_path))
    grid = dict(freq_min=1.0, freq_max=1e6, per_decade=1)
    run = edl1d.EDLRun(num_steps=3, L_n=1e-6, cation="K", electrode_voltage=P_M, kinetics="tafel", i0_CO=TAFEL["i0_CO"], i0_H2=TAFEL["i0_H2"], impedance=grid)
    try:
        run.run(verbose=False)
        path = run.write_outputs(stamp="spectrum")
        sp = run.impedance(imp.frequency_grid(**grid))
    finally:
        run.sys.close()
    z = np.load(os.path.join(path, "impedance.npz"))
    assert sorted(z.files) == sorted(["frequency", "sigma", "capacitance", "admittance", "impedance", "dI_CO", "dI_H2", "residual"])
    assert len(z["frequency"]) == 7 and np.array_equal(z["sigma"], imp.sigma_from_frequency(run.ep, z["frequency"]))
    for key in ("frequency", "sigma", "capacitance", "admittance", "impedance", "residual"):
        assert z[key].tobytes() == sp[key].tobytes(), key
    assert z["dI_CO"].tobytes() == np.ascontiguousarray(sp["dI_dV"][:, 0]).tobytes() and z["dI_H2"].tobytes() == np.ascontiguousarray(sp["dI_dV"][:, 1]).tobytes()
    assert np.all(z["impedance"].real > 0.0) and z["residual"].max() < 1e-12
    meta = json.load(open(os.path.join(path, "metadata.json")))
    assert meta["impedance_points"] == 7 and meta["impedance_status"] == 0
    assert meta["capacitance_low"] == z["capacitance"][0].real and meta["capacitance_high"] == z["capacitance"][-1].real
    assert 0.0 < meta["capacitance_high"] < meta["capacitance_low"] and meta["capacitance_high_closed_form"] > 0.0
    assert abs(meta["R_ct"] - 1.0 / (-(z["dI_CO"][0] + z["dI_H2"][0]).real)) <= 1e-12 * meta["R_ct"] and meta["R_ct"] > 0.0
    assert meta["impedance_last_step_change"] == float(np.abs(run.history[-1] - run.history[-2]).max()) > 0.0
