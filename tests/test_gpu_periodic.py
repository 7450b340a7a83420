"""The accelerated cycle map on the GPU (gmpnp_cycle_*, csrc/gmpnp_cycle.h): the report of gmpnp_cycle_end against
tests/periodic_reference.py over mesh sizes around the workgroup's 256 nodes and windows of 1, 2, 5 and 9 pairs, the mix bit for bit
against NumPy in the stated order, the limiter's factor, the handle's state behind a mix against a twin given set_state(u, u), every
refusal of the library, hook 33, and the driver: ``run_periodic`` over ``DeviceProgrammeOps`` on case A's mesh and waveform against
the NumPy reference, and ``EDLRun.programme(periodic=...)`` against a plain device march of the recorded period.
EDLRun reads its own 1 um mesh (1091 vertices, where the NumPy Newton loop is out of reach), so the comparison with the reference runs
the driver's loop and ops over a bare handle on case A's 33 uniform vertices, and EDLRun itself is compared with the device.
Every handle is closed by `with` / `finally`."""
import copy
import dataclasses
import json
import math
import os

import numpy as np
import pytest

import periodic_reference as QR
import time_step_reference as T
from gmpnp_amd import periodic as PD
from gmpnp_amd import programme as P
from gmpnp_amd.polarisation import NEWTON
from test_gpu_programme import KW, STEADY, HandleRun
from test_gpu_time_step import estimator_problem, small_pore, triple
from test_periodic_reference import CASE_A, case_a_segments
from test_programme_reference import steady_case, uniform_problem

pytestmark = pytest.mark.gpu
RTOL = 1e-2
WINDOWS = (1, 2, 5, 9)


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def report_problem(name):
    return small_pore()[2] if name == "cyl259" else estimator_problem(name)


def admissible(prob, n, seed):
    """n random admissible states, (ndof,) each (``triple``'s: a steric sum of at most 0.9)."""
    out = []
    for k in range((n + 2) // 3):
        out += [u.ravel() for u in triple(prob, seed=seed + 17 * k)]
    return out[:n]


def plant(dev, pairs):
    """The pairs (x, g) through the window: x by ``set_state`` in front of ``begin``, g in front of ``end``; the last report."""
    rep = None
    for x, g in pairs:
        dev.set_state(x, x)
        dev.cycle_begin()
        dev.set_state(g, g)
        rep = dev.cycle_end()
    return rep


def compare(rep, want, tol=1e-12):
    assert rep["window"] == want["window"] and rep["nonfinite"] == want["nonfinite"] and rep["n_free"] == want["n_free"]
    assert rep["A"].shape == want["A"].shape and rep["b"].shape == want["b"].shape
    for key in ("err", "err_max"):
        assert abs(rep[key] - want[key]) <= tol * abs(want[key]), (key, rep[key], want[key])
    for key in ("A", "b"):
        assert np.all(np.abs(rep[key] - want[key]) <= tol * np.abs(want[key])), (key, rep[key], want[key])
    assert rep["worst_dof"] == want["worst_dof"], (rep["worst_dof"], want["worst_dof"])
    assert np.array_equal(rep["A"], rep["A"].T)


@pytest.mark.parametrize("name", ["2", "3", "255", "256", "257", "513", "cyl259"])
def test_report_against_the_numpy_model(gpu_lib, name):
    """err, err_max, A and b to 1e-12 relative (sums of at most 3,591 products in another order: n 2^-53 ~ 4e-13), worst_dof as an
    integer, for windows of 1, 2, 5 and 9 pairs; a term planted at the first node, the last free node and every field of a mid node;
    Dirichlet rows never count; a NaN in one stored vector; equal bits from two passes; the oldest pair leaves a full window."""
    prob = report_problem(name)
    nv, nf = prob.coords.shape[0], prob.nf
    assert nf == (9 if name == "cyl259" else 7) and nv == (259 if name == "cyl259" else int(name))
    free = T.free_mask(prob)
    atol = np.linspace(1e-4, 3e-4, nf)
    st = admissible(prob, 19, seed=nv)
    u0, pool = st[0], st[1:]
    w = QR.cycle_weights(u0, nf, RTOL, atol)
    with gpu_lib.DeviceSolver(prob) as dev:
        for m1 in WINDOWS:
            pairs = [(pool[2 * j], pool[2 * j + 1]) for j in range(m1)]
            dev.set_state(u0, u0)
            dev.cycle_open(max(m1 - 1, 1), RTOL, atol)
            rep = plant(dev, pairs)
            want = QR.cycle_report([p[0] for p in pairs], [p[1] for p in pairs], w, free.ravel())
            compare(rep, want)
            assert rep["window"] == m1 and rep["err"] > 0.0 and not rep["nonfinite"]
            assert bits(dev.cycle_vectors("w")) == bits(w)
            assert bits(dev.cycle_vectors("x", m1)) == bits(np.stack([p[0] for p in pairs]))
            assert bits(dev.cycle_vectors("g", m1)) == bits(np.stack([p[1] for p in pairs]))
            dev.cycle_restart()                                            # a second pass over the same pairs: equal bits
            again = plant(dev, pairs)
            assert again["err"] == rep["err"] and again["err_max"] == rep["err_max"] and bits(again["A"]) == bits(rep["A"]) and bits(again["b"]) == bits(rep["b"])
            assert again["worst_dof"] == rep["worst_dof"]
        # a dominant term planted in turn in the newest g (the weights are frozen: they do not see it); free dofs only
        dev.set_state(u0, u0)
        dev.cycle_open(1, RTOL, atol)
        x0, g0, x1, g1 = pool[:4]
        base = plant(dev, [(x0, g0), (x1, g1)])
        first = [(0, f) for f in range(nf) if free[0, f]][:1]
        I_last = int(np.nonzero(free.any(axis=1))[0][-1])
        last = [(I_last, f) for f in range(nf) if free[I_last, f]][-1:]
        mid = [(nv // 2, f) for f in range(nf) if free[nv // 2, f]]
        assert first and last and (nv < 3 or mid)
        for I, f in first + last + mid:
            gp = g1.copy()
            gp[I * nf + f] += 1e3
            dev.cycle_restart()
            rep = plant(dev, [(x0, g0), (x1, gp)])
            compare(rep, QR.cycle_report([x0, x1], [g0, gp], w, free.ravel()))
            assert rep["worst_dof"] == I * nf + f
        # Dirichlet rows with a 1e6 jump never count
        bc = np.asarray(prob.bc_dofs, dtype=np.int64)
        assert len(bc)
        gj = g1.copy()
        gj[bc] += 1e6
        dev.cycle_restart()
        rep = plant(dev, [(x0, g0), (x1, gj)])
        assert rep["err"] == base["err"] and rep["err_max"] == base["err_max"] and rep["worst_dof"] == base["worst_dof"]
        assert bits(rep["A"]) == bits(base["A"]) and bits(rep["b"]) == bits(base["b"])
        # a NaN in one stored vector (the older x): nonfinite, err NaN, the status stays OK
        xn = x0.copy()
        xn[(nv // 3) * nf + 1] = np.nan
        dev.cycle_restart()
        rep = plant(dev, [(xn, g0), (x1, g1)])
        want = QR.cycle_report([xn, x1], [g0, g1], w, free.ravel())
        assert rep["nonfinite"] and want["nonfinite"] and math.isnan(rep["err"]) and math.isnan(rep["err_max"]) and rep["worst_dof"] == -1
        with pytest.raises(gpu_lib.GmpnpError, match="cycle.*not finite") as ei:       # no mix behind such a report, with or without the limiter
            dev.cycle_mix(np.array([0.5, 0.5]), 0.0)
        assert ei.value.code == gpu_lib.ERR_INVALID
        # weights that are not finite (u_n at the open was not): nonfinite as well, though every vector of the window is finite
        dev.set_state(xn, xn)
        dev.cycle_open(1, RTOL, atol)
        rep = plant(dev, [(x0, g0), (x1, g1)])
        assert rep["nonfinite"] and math.isnan(rep["err"]) and QR.cycle_report([x0, x1], [g0, g1], QR.cycle_weights(xn, nf, RTOL, atol), free.ravel())["nonfinite"]
        with pytest.raises(gpu_lib.GmpnpError, match="cycle.*not finite"):
            dev.cycle_mix(np.array([0.5, 0.5]), 0.9)
        # the oldest pair leaves a full window: depth 2 holds three pairs
        dev.set_state(u0, u0)
        dev.cycle_open(2, RTOL, atol)
        pairs = [(pool[2 * j], pool[2 * j + 1]) for j in range(5)]
        rep = plant(dev, pairs)
        assert rep["window"] == 3
        assert bits(dev.cycle_vectors("x", 3)) == bits(np.stack([p[0] for p in pairs[2:]]))
        assert bits(dev.cycle_vectors("g", 3)) == bits(np.stack([p[1] for p in pairs[2:]]))
        compare(rep, QR.cycle_report([p[0] for p in pairs[2:]], [p[1] for p in pairs[2:]], w, free.ravel()))
        dev.cycle_close()


@pytest.mark.parametrize("name", ["3", "257", "cyl259"])
def test_mix_against_numpy_and_a_twin(gpu_lib, name):
    """The bits of g_k + alpha (sum_j gamma_j g_j - g_k) formed in NumPy in the stated order, Dirichlet rows g_k, the limiter's alpha
    from gmpnp_step_limit for that direction at g_k, and behind the mix F, the CSR Jacobian and the history levels of a twin handle
    given set_state(u, u)."""
    prob = report_problem(name)
    nv, nf = prob.coords.shape[0], prob.nf
    free = T.free_mask(prob).ravel()
    st = admissible(prob, 19, seed=3 * nv + 1)
    u0, pool = st[0], st[1:]
    rng = np.random.default_rng(nv)
    with gpu_lib.DeviceSolver(prob) as dev, gpu_lib.DeviceSolver(prob) as twin:
        for m1 in WINDOWS:
            pairs = [(pool[2 * j], pool[2 * j + 1]) for j in range(m1)]
            G = [p[1] for p in pairs]
            dev.set_state(u0, u0)
            dev.time_accept()                                              # a history level, which the mix drops
            assert dev.time_history_levels() == 1
            dev.cycle_open(max(m1 - 1, 1), RTOL, 1e-4)
            plant(dev, pairs)
            gamma = rng.dirichlet(np.ones(m1))                             # convex: the mixed state stays admissible
            gamma[-1] += 1.0 - math.fsum(gamma)
            assert PD.gamma_valid(gamma)
            dev.assemble(True)                                             # a Jacobian at the old state, to be invalidated
            alpha = dev.cycle_mix(gamma, 0.0)
            assert alpha == 1.0
            want = QR.cycle_mix(G, gamma, free, 1.0)
            got, got_n = dev.get_state(), dev.get_state(previous=True)
            assert bits(got) == bits(want) == bits(got_n)
            bc = np.asarray(prob.bc_dofs, dtype=np.int64)
            assert bits(got[bc]) == bits(G[-1][bc]) and (m1 == 1 or not np.array_equal(got[free], G[-1][free]))
            assert dev.time_history_levels() == 0
            with pytest.raises(gpu_lib.GmpnpError, match="no Jacobian"):
                dev.jacobian_csr()
            twin.set_state(want, want)
            (Fa, na), (Fb, nb) = dev.assemble(True), twin.assemble(True)
            assert bits(Fa) == bits(Fb) and na == nb and bits(dev.jacobian_csr().data) == bits(twin.jacobian_csr().data)
            with pytest.raises(gpu_lib.GmpnpError, match="cycle"):         # a second mix needs another end
                dev.cycle_mix(gamma, 0.0)
        # tau = 0.9 on a direction that leaves the admissible set: an extrapolation through two states whose steric sums differ
        lo, hi = pool[0].reshape(nv, nf).copy(), pool[1].reshape(nv, nf).copy()
        a = np.asarray(prob.model.a, dtype=np.float64)[:nf - 1]
        lo[:, :nf - 1] *= (0.3 / T.steric_sum(a, lo))[:, None]
        hi[:, :nf - 1] *= (0.9 / T.steric_sum(a, hi))[:, None]
        lo, hi = lo.ravel(), hi.ravel()
        gamma = np.array([-3.0, 4.0])                                      # g_k + 3 (g_k - g_0): the steric sum would reach 2.7
        dev.set_state(u0, u0)
        dev.cycle_open(1, RTOL, 1e-4)
        plant(dev, [(u0, lo), (u0, hi)])
        alpha = dev.cycle_mix(gamma, 0.9)
        dx = np.where(free, -QR.mix_direction([lo, hi], gamma), 0.0)
        twin.set_state(hi, hi)
        a_lib, lam, node = twin.step_limit(dx, 0.9)
        assert alpha == a_lib and 0.0 < alpha < 1.0 and lam < 1.0 and node >= 0
        assert alpha == QR.mix_alpha(prob, [lo, hi], gamma, free, 0.9)
        assert bits(dev.get_state()) == bits(QR.cycle_mix([lo, hi], gamma, free, alpha)) == bits(dev.get_state(previous=True))
        S = T.steric_sum(a, dev.get_state().reshape(nv, nf))
        assert S.max() < 1.0
        # a direction that limits nothing: alpha = 1 with the limiter on
        dev.cycle_restart()
        plant(dev, [(u0, hi), (u0, lo)])
        assert dev.cycle_mix(np.array([0.5, 0.5]), 0.9) == 1.0
        dev.cycle_close()


def test_refusals_and_hook_33(pore10, gpu_lib):
    from gmpnp_amd import dist
    from gmpnp_amd.problem import Galvanostat, pore_hierarchy
    from gmpnp_amd.solver import GMPNPSystem

    def refused(call, what="cycle"):
        with pytest.raises(gpu_lib.GmpnpError, match=what) as ei:
            call()
        assert ei.value.code == gpu_lib.ERR_INVALID

    prob = uniform_problem(9)[1]
    nf = prob.nf
    st = admissible(prob, 6, seed=4)
    one = np.array([1.0])
    with gpu_lib.DeviceSolver(prob) as dev:
        dev.set_state(st[0], st[0])
        for call in (dev.cycle_begin, dev.cycle_end, lambda: dev.cycle_mix(one, 0.0), dev.cycle_restart, dev.cycle_close,
                     lambda: dev.cycle_vectors("w")):
            refused(call)                                                  # no cycle is open
        refused(lambda: dev.time_kernel(33, 1), "33")
        for depth in (0, 9, -1):
            refused(lambda: dev.cycle_open(depth, RTOL, 1e-4))
        refused(lambda: dev.cycle_open(2, -1.0, 1e-4))
        refused(lambda: dev.cycle_open(2, RTOL, 0.0))
        refused(lambda: dev.cycle_open(2, math.nan, 1e-4))
        dev.cycle_open(2, RTOL, 1e-4)
        refused(dev.cycle_end)                                             # end without begin
        refused(lambda: dev.cycle_mix(one, 0.0))                           # mix before end
        refused(lambda: dev.time_kernel(33, 1), "33")                      # no pair in the window
        rep = plant(dev, [(st[1], st[2])])
        assert rep["window"] == 1
        refused(lambda: dev.cycle_mix(np.array([0.5, 0.5]), 0.0))          # a wrong n
        refused(lambda: dev.cycle_mix(np.array([1.0 + 1e-9]), 0.0))        # the weights do not sum to 1
        refused(lambda: dev.cycle_mix(np.array([math.nan]), 0.0))
        for tau in (1.0, -0.1, math.nan):
            refused(lambda: dev.cycle_mix(one, tau))
        dev.electrode_trace_open(4)                                        # an open trace: the driver closes it around a mix
        refused(lambda: dev.cycle_mix(one, 0.0))
        dev.electrode_trace_close()
        dev.sensitivity_open([0], "zero", 4)
        refused(lambda: dev.cycle_mix(one, 0.0))
        dev.sensitivity_close()
        # hook 33: the window, the state and the history stay
        dev.set_state(st[3], st[4])
        before = (dev.get_state(), dev.get_state(previous=True), dev.cycle_vectors("g", 1))
        assert dev.time_kernel(33, 3) > 0.0
        assert bits(dev.get_state()) == bits(before[0]) and bits(dev.get_state(previous=True)) == bits(before[1])
        assert bits(dev.cycle_vectors("g", 1)) == bits(before[2])
        assert dev.cycle_mix(one, 0.0) == 1.0 and bits(dev.get_state()) == bits(st[2])      # gamma = (1): the plain iteration, g_k itself
        refused(lambda: dev.cycle_mix(one, 0.0))                           # the report is used up
        dev.set_galvanostat(Galvanostat(1.0))
        for call in (dev.cycle_begin, lambda: dev.cycle_open(2, RTOL, 1e-4)):
            refused(call)
        dev.set_galvanostat(None)
        dev.set_time_order(2)
        for call in (dev.cycle_begin, lambda: dev.cycle_open(2, RTOL, 1e-4)):
            refused(call)
        dev.set_time_order(1)
        dev.cycle_begin()
        dev.cycle_close()
        refused(dev.cycle_begin)
    # an open wall profile at the mix, on a 3D handle with the Stern option (the library accepts 3D handles)
    import pore_response_reference as PP
    prob_w = PP.cylinder_case((1, 2), p_M=-1.0)
    sw = admissible(prob_w, 3, seed=8)
    with gpu_lib.DeviceSolver(prob_w) as dev3:
        dev3.set_state(sw[0], sw[0])
        dev3.cycle_open(1, RTOL, 1e-4)
        assert plant(dev3, [(sw[1], sw[2])])["window"] == 1
        dev3.wall_profile_open([0.0, 0.5, 1.0], 2)
        refused(lambda: dev3.cycle_mix(one, 0.0))
        assert bits(dev3.get_state()) == bits(sw[2])                       # nothing was applied (the state is the last one planted)
        dev3.wall_profile_close()
        assert dev3.cycle_mix(one, 0.9) == 1.0 and bits(dev3.get_state()) == bits(sw[2]) == bits(dev3.get_state(previous=True))
        dev3.cycle_close()
    pp, mesh, prob3, _ = pore10
    dom, perm, part = dist.partition_plan(prob3, 2, 0)
    with gpu_lib.DeviceSolver(dom.problem, perm=perm, partition=part) as partitioned:
        refused(lambda: partitioned.cycle_open(2, RTOL, 1e-4))
    levels = pore_hierarchy(pp, mesh, 1)
    ml = GMPNPSystem(levels[0][0], levels=levels)
    try:
        refused(lambda: ml.dev.cycle_open(2, RTOL, 1e-4))                  # a coarse level attached,
        refused(lambda: ml._coarse[0].cycle_open(2, RTOL, 1e-4))           # and the handle that serves as one
    finally:
        ml.close()


def test_a_twin_that_never_opens_a_cycle_solves_with_equal_bits(gpu_lib):
    """A handle that brackets its Newton solve with begin / end computes what a handle that never opened a cycle computes, and that
    one has no cycle storage (hook 33 is refused)."""
    ep, prob, u, inv = steady_case(9)
    opts = gpu_lib.newton_options(NEWTON, dim=1)
    with gpu_lib.DeviceSolver(prob) as a, gpu_lib.DeviceSolver(prob) as b:
        for d in (a, b):
            d.set_state(u, u)
            d.set_electrode_potential(-5.5)
            d.set_time_step(inv(7.5))
        a.cycle_open(4, RTOL, 1e-4)
        a.cycle_begin()
        sa, sb = a.newton_solve(opts), b.newton_solve(opts)
        a.time_accept(); b.time_accept()
        rep = a.cycle_end()
        assert sa["converged"] and sa["iterations"] == sb["iterations"] >= 1 and sa["residuals"] == sb["residuals"]
        assert bits(a.get_state()) == bits(b.get_state()) and rep["window"] == 1 and rep["err"] > 0.0
        with pytest.raises(gpu_lib.GmpnpError, match="33"):
            b.time_kernel(33, 1)


# ---- the driver --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reference_a():
    """The NumPy reference of case A: the accelerated run and plain marching under the same cap (its last two residuals give rho)."""
    ep, prob, u, inv = steady_case(CASE_A["nv"])
    segs, n = case_a_segments(), CASE_A["steps"]
    policy = PD.PeriodicPolicy(tol=CASE_A["tol"], depth=CASE_A["depth"], max_cycles=CASE_A["max_cycles"], tau=CASE_A["tau"])
    ref = QR.NumpyPeriodicSystem(prob, u, inv, cycle_tol=CASE_A["cycle_tol"])
    res = PD.run_periodic(ref, segs, policy, n)
    plain = QR.NumpyPeriodicSystem(prob, u, inv, cycle_tol=CASE_A["cycle_tol"])
    errs, _ = QR.plain_march(plain, segs, n, CASE_A["tol"], CASE_A["max_cycles"])
    return dict(prob=prob, u=u, inv=inv, segs=segs, policy=policy, ref=ref, res=res, rho=errs[-1] / errs[-2])


def test_driver_loop_against_the_reference_on_case_a(reference_a, gpu_lib):
    """``run_periodic`` over ``DeviceProgrammeOps`` on case A: the reference's cycle count, its first three residuals within 1e-6
    relative (later ones are amplified by gamma and are not compared digit for digit), the converged state within 2 tol / (1 - rho) of
    the reference's in the weighted norm, and the records of one period."""
    r = reference_a
    run = HandleRun(copy.copy(r["prob"]))
    try:
        run.sys.set_state(r["u"], r["u"])
        ops = P.DeviceProgrammeOps(run, dict(NEWTON), r["inv"], capacity=5, cycle_tol=CASE_A["cycle_tol"])     # smaller than a period: drained on the way
        res = PD.run_periodic(ops, r["segs"], r["policy"], CASE_A["steps"])
        rec = ops.records()
        with pytest.raises(gpu_lib.GmpnpError, match="no cycle is open"):
            run.sys.dev.cycle_begin()
    finally:
        run.sys.close()
    want = r["res"]
    errs, errs_ref = [h["err"] for h in res["history"]], [h["err"] for h in want["history"]]
    print("case A on the device: %d cycles (reference %d), residuals %s against %s" % (res["cycles"], want["cycles"], errs, errs_ref))
    assert res["converged"] and want["converged"] and res["cycles"] == want["cycles"] and res["restarts"] == 0
    for a, b in zip(errs[:3], errs_ref[:3]):
        assert abs(a - b) <= 1e-6 * b
    bound = 2.0 * CASE_A["tol"] / (1.0 - r["rho"])
    free = r["ref"].free.ravel()
    q = ((res["state"].ravel() - want["state"]) / r["ref"].w)[free]
    dist = math.sqrt(float((q * q).sum()) / free.sum())
    print("case A on the device: distance of the converged states %.3e (bound %.3e, rho %.4f)" % (dist, bound, r["rho"]))
    assert dist <= bound
    n = CASE_A["steps"] * len(r["segs"])
    assert len(rec) == n and np.array_equal(rec["t"], [rw["t"] for rw in r["ref"].records]) and np.all(rec["status"] == 0)
    assert res["record"]["breakpoints"] == [g[1] for g in r["segs"]] and [h["window"] for h in res["history"]] == [h["window"] for h in want["history"]]


def test_device_ops_restart_keeps_the_state_and_drops_window_and_records(reference_a, gpu_lib):
    """``DeviceProgrammeOps.cycle_restart`` (the loop's restart branch; the loop itself is scripted on the CPU): the window is emptied,
    the records of the cycle before are dropped, the trace is open again with D_prev at the state, and the state and its history are
    left alone, so the next period is the period a plain march would take next, bit for bit."""
    r = reference_a
    runs = [HandleRun(copy.copy(r["prob"])), HandleRun(copy.copy(r["prob"]))]
    try:
        ends = []
        for k, run in enumerate(runs):
            run.sys.set_state(r["u"], r["u"])
            ops = P.DeviceProgrammeOps(run, dict(NEWTON), r["inv"], cycle_tol=CASE_A["cycle_tol"])
            if k == 0:                                                     # with the cycle calls and a restart between two periods
                ops.cycle_open(CASE_A["depth"])
                ops.cycle_begin()
                P.run_programme(ops, r["segs"], steps_per_segment=CASE_A["steps"])
                first = ops.cycle_end()
                levels = run.sys.dev.time_history_levels()
                u_mid = run.sys.dev.get_state()
                ops.cycle_restart()
                assert ops.count == 0 and ops.chunks == [] and ops.segments == [] and ops.states == [] and ops.residuals == []
                assert bits(run.sys.dev.get_state()) == bits(u_mid) == bits(run.sys.dev.get_state(previous=True))
                assert run.sys.dev.time_history_levels() == levels == 1 and ops.D_first == run.sys.dev.stern_displacement()
                ops.cycle_begin()
                P.run_programme(ops, r["segs"], steps_per_segment=CASE_A["steps"])
                second = ops.cycle_end()
                assert first["window"] == 1 == second["window"] and second["err"] < first["err"]
                ops.cycle_close()
                rec = ops.records()
                assert len(rec) == CASE_A["steps"] * len(r["segs"]) and rec["Q_D"][0] == rec["h"][0] * rec["dD_dt"][0]
            else:                                                          # two plain periods
                P.run_programme(ops, r["segs"], steps_per_segment=CASE_A["steps"])
                P.run_programme(ops, r["segs"], steps_per_segment=CASE_A["steps"])
                ops.records()
            ends.append(run.sys.dev.get_state())
    finally:
        for run in runs:
            run.sys.close()
    assert bits(ends[0]) == bits(ends[1])


PERIOD_S = dict(kind="pulse", v_levels=[-5.5, -4.5], steps_per_segment=4)


def test_edl_run_records_the_converged_period(gpu_lib, tmp_path):
    """``EDLRun.programme(periodic=...)`` on the driver's own 1 um mesh with case A's waveform, from the steady stop at p_M = -5: it
    converges under case A's cap of 12 cycles where plain marching of 25 cycles does not reach the tolerance, the history is consistent, and the
    arrays of ``programme.npz`` are, bit for bit, those of a plain march of one period from the converged state.  Without the option
    the programme's outputs carry nothing of it."""
    from gmpnp_amd import edl1d
    os.environ["GMPNP_OUT"] = str(tmp_path)
    run = edl1d.EDLRun(**STEADY, **KW)
    try:
        run.run(verbose=False)
        tc = run.ep.time_constant
        par = dict(PERIOD_S, durations=[CASE_A["durations"][0] * tc, CASE_A["durations"][1] * tc])
        u_steady = run.sys.dev.get_state()
        w = QR.cycle_weights(u_steady, 7, 1e-2, 1e-4)
        free = T.free_mask(run.problem).ravel()
        # plain marching of 25 cycles from the steady state: the residuals between the period ends stay above the tolerance
        marched = run.programme(cycles=25, **par)
        ends = [u_steady] + [v.ravel() for k, (_, _, v) in enumerate(marched["states"]) if k % 2 == 1]
        plain_errs = [math.sqrt(float(((((b - a) / w)[free]) ** 2).sum()) / free.sum()) for a, b in zip(ends, ends[1:])]
        print("EDLRun plain marching: residual %.3e after 25 cycles" % plain_errs[-1])
        assert len(plain_errs) == 25 and min(plain_errs) > CASE_A["tol"]
        run.sys.set_state(u_steady, u_steady)                              # back to the steady state at p_M = -5
        run.sys.dev.set_electrode_potential(-5.0)
        run.stern = dataclasses.replace(run.stern, p_electrode=-5.0)
        run.kinetics = dataclasses.replace(run.kinetics, p_electrode=-5.0)
        run.problem.stern, run.problem.kinetics = run.stern, run.kinetics
        out = run.programme(periodic=dict(tol=CASE_A["tol"], depth=CASE_A["depth"], max_cycles=CASE_A["max_cycles"], tau=CASE_A["tau"]), **par)
        meta, search = out["metadata"], out["periodic"]
        print("EDLRun periodic: %d cycles, residuals %s, restarts %d" % (meta["programme_periodic_cycles"], search["err"].tolist(), meta["programme_periodic_restarts"]))
        assert meta["programme_periodic_converged"] and meta["programme_periodic_cycles"] == len(search["err"]) <= CASE_A["max_cycles"] < len(plain_errs)
        assert abs(search["err"][0] - plain_errs[0]) <= 1e-12 * plain_errs[0]      # the first cycle is the same march; the sums differ in order
        assert meta["programme_periodic_residual"] == search["err"][-1] <= CASE_A["tol"] and search["verdict"][-1] == PD.CONVERGED
        assert sorted(search) == sorted(PD.HISTORY_COLUMNS + ("state",)) and meta["programme_steps_accepted"] == 8 == len(out["time_s"])
        for key in PD.METADATA_KEYS:
            assert key in meta
        with pytest.raises(gpu_lib.GmpnpError, match="no cycle is open"):
            run.sys.dev.cycle_begin()
        with pytest.raises(gpu_lib.GmpnpError, match="no trace is open"):
            run.sys.dev.electrode_trace_append(1.0, 1.0)
        # the recorded period against a plain march of the same period from the converged state (the run stands at the last level)
        state = search["state"]
        run.sys.set_state(state.ravel(), state.ravel())
        plain = run.programme(**par)
        for key in P.OUTPUT_KEYS:
            assert bits(plain[key]) == bits(out[key]), key
        assert "periodic" not in plain and not [k for k in plain["metadata"] if "periodic" in k]
        off = run.programme(periodic=None, **par)                          # None is the option off: a march from where the run stands
        assert "periodic" not in off and len(off["time_s"]) == 8
        # the limit cycle repeats: the end of the recorded period is its start within the tolerance, which the steady state is not
        end = plain["states"][-1][2].ravel()
        q = ((end - state.ravel()) / w)[free]
        assert math.sqrt(float((q * q).sum()) / free.sum()) <= 2.0 * CASE_A["tol"]
        # the files of the driver
        run.programme_par = dict(par, periodic=dict(tol=CASE_A["tol"], max_cycles=25))
        run.sys.set_state(state.ravel(), state.ravel())
        path = run.write_outputs(stamp="periodic")
    finally:
        run.sys.close()
        del os.environ["GMPNP_OUT"]
    files = sorted(os.listdir(path))
    assert "programme_periodic.npz" in files and "programme.npz" in files
    z = np.load(os.path.join(path, "programme_periodic.npz"))
    assert sorted(z.files) == sorted(PD.HISTORY_COLUMNS + ("state",)) and z["state"].shape == state.shape
    meta = json.load(open(os.path.join(path, "metadata.json")))
    assert meta["programme_periodic_converged"] is True and meta["programme_periodic_cycles"] == len(z["err"]) <= 25
    assert meta["programme_periodic_residual"] == z["err"][-1] and meta["programme_periodic_restarts"] == int(z["restart"].sum())
    assert sorted(np.load(os.path.join(path, "programme.npz")).files) == sorted(P.OUTPUT_KEYS)
