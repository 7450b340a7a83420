"""Second-order adaptive time stepping on the GPU (include/gmpnp.h "second-order adaptive time stepping", csrc/gmpnp_time_order.h,
gmpnp_amd/timestep.py): the order-2 estimator against the NumPy model of tests/time_order_reference.py, u* and
the BDF2 set-up against handles created with the step, the three-deep shift and the level rules, the forwarding to attached coarse
levels, order-2 runs of the drivers against the reference loops pinned in tests/test_time_order_reference.py, the observed order
through the device, and the refusals.

Newton tolerances of the runs compared with the reference loops: tests/test_time_step_reference.py (relative 1e-9, absolute 1e-6)."""
import contextlib
import json
import os
import subprocess
import sys
import warnings
from ctypes import POINTER, byref, c_double, c_int32

import numpy as np
import pytest

import test_gpu_time_step as G
import test_time_order_reference as C
import time_order_reference as R
import time_step_reference as T
from conftest import ROOT

pytestmark = pytest.mark.gpu

RTOL = 1e-2
STEPS = (0.11, 0.07, 0.05)   # h, h_prev, h_prev2 of the estimator cases: unequal


def four(prob, seed):
    """Random admissible (u, u_n, u_nm1, u_nm2)."""
    return G.triple(prob, seed) + G.triple(prob, seed + 1000)[:1]


def load(dev, u, un, unm1, unm2=None):
    """The states onto an order-2 handle through accepts: levels 2 with ``unm2``, else 1 (u_nm2 stays what it was)."""
    dev.set_time_order(2)
    if unm2 is not None:
        dev.set_state(unm1.ravel(), unm2.ravel())
        dev.time_accept()
        dev.set_state(un.ravel(), None)
    else:
        dev.set_state(un.ravel(), unm1.ravel())
    dev.time_accept()
    dev.set_state(u.ravel(), None)   # (a set_state that leaves u_n alone keeps the history)


@pytest.mark.parametrize("name", ["2", "255", "256", "257", "513", "pore10"])
def test_order_2_estimator_against_the_numpy_model(gpu_lib, name):
    """err_field / rate_field to 1e-12 relative (5e's tolerance: both sum <= 1,767 squares in different orders), worst_dof as an
    integer with a dominant term planted at the first node, the last free node and every field of a mid node; two calls give equal
    bits; fewer than 2 levels: no history."""
    prob = G.estimator_problem(name)
    nv, nf = prob.coords.shape[0], prob.nf
    u, un, unm1, unm2 = four(prob, seed=nv)
    atol = np.linspace(1e-4, 3e-4, nf)
    free = T.free_mask(prob)
    h, h1, h2 = STEPS
    with gpu_lib.DeviceSolver(prob) as dev:
        dev.set_time_order(2)
        dev.set_state(u.ravel(), un.ravel())
        assert dev.time_history_levels() == 0
        e = dev.time_error_bdf2(h, h1, h2, RTOL, atol)
        G.compare(e, R.time_error2(u, un, None, None, h, h1, h2, RTOL, atol, free), nf)
        assert not e["has_history"] and e["err"] == 0.0 and e["rate"] > 0.0 and e["worst_dof"] == -1
        load(dev, u, un, unm1)   # one level: still none for order 2 (the order-1 estimator has its history)
        assert dev.time_history_levels() == 1
        e1 = dev.time_error_bdf2(h, h1, h2, RTOL, atol)
        assert not e1["has_history"] and e1["err"] == 0.0 and np.array_equal(e1["rate_field"], e["rate_field"])
        assert dev.time_error(h, h1, RTOL, atol)["has_history"]
        load(dev, u, un, unm1, unm2)
        assert dev.time_history_levels() == 2
        e = dev.time_error_bdf2(h, h1, h2, RTOL, atol)
        G.compare(e, R.time_error2(u, un, unm1, unm2, h, h1, h2, RTOL, atol, free), nf)
        assert e["has_history"] and e["err"] > 0.0
        e2 = dev.time_error_bdf2(h, h1, h2, RTOL, atol)
        assert e2["err"] == e["err"] and np.array_equal(e2["err_field"], e["err_field"]) and np.array_equal(e2["rate_field"], e["rate_field"])
        for hp in ((h1, 0.0), (0.0, h2)):   # a step <= 0: no history either
            e0 = dev.time_error_bdf2(h, hp[0], hp[1], RTOL, atol)
            assert not e0["has_history"] and e0["err"] == 0.0 and np.array_equal(e0["rate_field"], e["rate_field"])
        # the order-1 estimator on the same handle is 5e's (u_nm2 is not its business)
        G.compare(dev.time_error(h, h1, RTOL, atol), T.time_error(u, un, unm1, h, h1, RTOL, atol, free), nf)
        first = [(0, f) for f in range(nf) if free[0, f]][:1]
        I_last = int(np.nonzero(free.any(axis=1))[0][-1])
        last = [(I_last, f) for f in range(nf) if free[I_last, f]][-1:]
        mid = [(nv // 2, f) for f in range(nf) if free[nv // 2, f]]
        assert first and last and (nv < 3 or mid) and I_last >= nv - 2
        for k, (I, f) in enumerate(first + last + mid):   # planted in u_nm2 and u_nm1 in turn: the weights do not see either
            m1, m2 = unm1.copy(), unm2.copy()
            (m2 if k % 2 == 0 else m1)[I, f] += 1e3
            load(dev, u, un, m1, m2)
            ep = dev.time_error_bdf2(h, h1, h2, RTOL, atol)
            G.compare(ep, R.time_error2(u, un, m1, m2, h, h1, h2, RTOL, atol, free), nf)
            assert ep["worst_dof"] == I * nf + f
        load(dev, u, un, unm1, unm2)
        bc = np.asarray(prob.bc_dofs, dtype=np.int64)
        assert len(bc)
        uj = u.copy().ravel()
        uj[bc] += 1e6   # Dirichlet dofs with a jump are ignored
        dev.set_state(uj, None)
        ej = dev.time_error_bdf2(h, h1, h2, RTOL, atol)
        assert np.array_equal(ej["err_field"], e["err_field"]) and np.array_equal(ej["rate_field"], e["rate_field"]) and ej["worst_dof"] == e["worst_dof"]
        un_ = u.copy()
        un_[nv // 3, 1] = np.nan   # a planted NaN: nonfinite = 1, status OK, err NaN
        dev.set_state(un_.ravel(), None)
        en = dev.time_error_bdf2(h, h1, h2, RTOL, atol)
        assert en["nonfinite"] and np.isnan(en["err"]) and np.all(np.isnan(en["err_field"]))


@pytest.mark.parametrize("name", ["257", "pore10"])
def test_history_vector_and_the_bdf2_set_up(gpu_lib, name):
    """u* against a u_n - b u_nm1 from NumPy for omega in {0.3, 1, 2}: 4 ulp of the larger product (each product rounds to half an
    ulp of itself and so does the difference; a fused multiply-add on the device skips one of the three roundings — the difference
    itself may be small against the products).  After the set-up F and the CSR Jacobian are, bit for bit, those of a handle created
    with alpha0 inv_dt whose u_n is the downloaded u*; a plain set_time_step afterwards gives the order-1 F and J again."""
    prob = G.estimator_problem(name)
    u, un, unm1, _ = four(prob, seed=41)
    x = prob.model.inv_dt / 3.0
    with gpu_lib.DeviceSolver(prob) as a:
        load(a, u, un, unm1)
        for om in (0.3, 1.0, 2.0):
            a.assemble(True)   # a Jacobian at the old step, to be invalidated
            a.set_time_step_bdf2(x, om)
            star = a.get_time_history()
            wa, wb = R.history_weights(om)
            pa, pb = wa * un.ravel(), wb * unm1.ravel()
            tol = 4.0 * np.spacing(np.maximum(np.abs(pa), np.abs(pb)))
            assert np.all(np.abs(star - (pa - pb)) <= tol), float(np.abs(star - (pa - pb)).max())
            assert np.array_equal(a.get_state(previous=True), un.ravel())   # get_state sees the true u_n
            Fa, ra = a.assemble(True)
            Ja = a.jacobian_csr()
            with gpu_lib.DeviceSolver(G.with_inv_dt(prob, float(R.alpha0(om)) * x)) as b:
                b.set_state(u.ravel(), star)
                Fb, rb = b.assemble(True)
                Jb = b.jacobian_csr()
            assert np.array_equal(Fa, Fb) and ra == rb and np.all(np.isfinite(Fa))
            assert np.array_equal(Ja.indptr, Jb.indptr) and np.array_equal(Ja.indices, Jb.indices) and np.array_equal(Ja.data, Jb.data)
        a.set_time_step(x)   # an order-1 step again: reads u_n
        Fa, ra = a.assemble(True)
        Ja = a.jacobian_csr()
        with gpu_lib.DeviceSolver(G.with_inv_dt(prob, x)) as b:
            b.set_state(u.ravel(), un.ravel())
            Fb, rb = b.assemble(True)
            Jb = b.jacobian_csr()
        assert np.array_equal(Fa, Fb) and ra == rb and np.array_equal(Ja.data, Jb.data)
        assert not np.array_equal(Fa, Fb * 0.0)
        for bad in ((np.nan, 1.0), (np.inf, 1.0), (-1.0, 1.0), (x, 0.0), (x, -1.0), (x, np.nan), (x, np.inf)):
            with pytest.raises(gpu_lib.GmpnpError) as ei:
                a.set_time_step_bdf2(*bad)
            assert ei.value.code == gpu_lib.ERR_INVALID
    with gpu_lib.DeviceSolver(prob) as c:   # not at order 2; at order 2 without an accepted state
        for prepare in (lambda: None, lambda: c.set_time_order(2)):
            prepare()
            with pytest.raises(gpu_lib.GmpnpError) as ei:
                c.set_time_step_bdf2(x, 1.0)
            assert ei.value.code == gpu_lib.ERR_INVALID
        with pytest.raises(gpu_lib.GmpnpError):
            c.get_time_history()
        with pytest.raises(gpu_lib.GmpnpError):
            c.set_time_order(3)


@pytest.mark.parametrize("name", ["257", "pore10"])
def test_shift_and_level_rules(gpu_lib, name):
    prob = G.estimator_problem(name)
    nf = prob.nf
    free = T.free_mask(prob)
    s = [x for k in range(3) for x in G.triple(prob, seed=60 + k)][:6]   # six states
    h, h1, h2 = STEPS
    est = lambda dev: dev.time_error_bdf2(h, h1, h2, RTOL, 1e-4)
    with gpu_lib.DeviceSolver(prob) as dev:
        dev.set_time_order(2)
        dev.set_state(s[1].ravel(), s[0].ravel())
        assert dev.time_history_levels() == 0
        dev.time_accept()                       # u_n = s1, u_nm1 = s0
        assert dev.time_history_levels() == 1
        dev.set_state(s[2].ravel(), None)
        dev.time_accept()                       # u_n = s2, u_nm1 = s1, u_nm2 = s0
        assert dev.time_history_levels() == 2
        dev.set_state(s[3].ravel(), None)
        dev.time_accept()                       # u_n = s3, u_nm1 = s2, u_nm2 = s1: three deep, exact copies
        assert dev.time_history_levels() == 2
        assert np.array_equal(dev.get_state(), s[3].ravel()) and np.array_equal(dev.get_state(previous=True), s[3].ravel())
        dev.set_state(s[4].ravel(), None)
        e = est(dev)
        G.compare(e, R.time_error2(s[4], s[3], s[2], s[1], h, h1, h2, RTOL, 1e-4, free), nf)
        G.compare(dev.time_error(h, h1, RTOL, 1e-4), T.time_error(s[4], s[3], s[2], h, h1, RTOL, 1e-4, free), nf)
        # exact copies: u* of omega = 1 from (u_n, u_nm1) = (s3, s2) has no rounding in its weights' inputs but its own
        dev.set_time_step_bdf2(prob.model.inv_dt, 1.0)
        wa, wb = R.history_weights(1.0)
        pa, pb = wa * s[3].ravel(), wb * s[2].ravel()
        assert np.all(np.abs(dev.get_time_history() - (pa - pb)) <= 4.0 * np.spacing(np.maximum(np.abs(pa), np.abs(pb))))
        # a rejection copies the TRUE u_n (the time term reads u* now) and keeps the history
        dev.time_reject()
        assert np.array_equal(dev.get_state(), s[3].ravel()) and np.array_equal(dev.get_state(previous=True), s[3].ravel())
        assert dev.time_history_levels() == 2
        dev.set_state(s[4].ravel(), None)
        e2 = est(dev)
        assert e2["has_history"] and e2["err"] == e["err"] and np.array_equal(e2["err_field"], e["err_field"])
        # order 1 caps the levels at 1 and keeps u_nm1; back at order 2 the count goes on from there
        dev.set_time_order(1)
        assert dev.time_history_levels() == 1 and not est(dev)["has_history"]
        G.compare(dev.time_error(h, h1, RTOL, 1e-4), T.time_error(s[4], s[3], s[2], h, h1, RTOL, 1e-4, free), nf)
        dev.time_accept()                       # order 1: the two-deep shift, u_n = s4, u_nm1 = s3
        assert dev.time_history_levels() == 1
        dev.set_time_order(2)
        dev.set_state(s[5].ravel(), None)
        dev.time_accept()                       # u_n = s5, u_nm1 = s4, u_nm2 = s3
        assert dev.time_history_levels() == 2
        dev.set_state(s[0].ravel(), None)
        G.compare(est(dev), R.time_error2(s[0], s[5], s[4], s[3], h, h1, h2, RTOL, 1e-4, free), nf)
        # a set_state that writes u_n, and assign_previous, drop the history to zero levels
        dev.set_state(s[0].ravel(), s[5].ravel())
        assert dev.time_history_levels() == 0 and not est(dev)["has_history"] and not dev.time_error(h, h1, RTOL, 1e-4)["has_history"]
        dev.time_accept()
        dev.time_accept()
        assert dev.time_history_levels() == 2
        dev.assign_previous()
        assert dev.time_history_levels() == 0
    # a handle that never calls the new family: 5e's behaviour, and the order-2 storage does not exist
    with gpu_lib.DeviceSolver(prob) as dev:
        dev.set_state(s[1].ravel(), s[0].ravel())
        dev.time_accept()
        dev.set_state(s[2].ravel(), None)
        dev.time_accept()
        assert dev.time_history_levels() == 1   # order 1 counts one level
        dev.set_state(s[3].ravel(), None)
        G.compare(dev.time_error(h, h1, RTOL, 1e-4), T.time_error(s[3], s[2], s[1], h, h1, RTOL, 1e-4, free), nf)
        assert not est(dev)["has_history"]      # ... and an order-2 estimate finds no third state
        with pytest.raises(gpu_lib.GmpnpError):
            dev.get_time_history()


def test_bdf2_set_up_reaches_the_coarse_levels(gpu_lib):
    """5e's forwarding test with the BDF2 set-up: on the 114 / 671-vertex hierarchy the first Newton system after
    set_time_step_bdf2(x, omega) takes the BiCGStab iterations of a hierarchy built with alpha0 x on both levels.  Red when the
    set-up leaves the coarse level's model as it was."""
    import precond_reference as P
    hier = P.cylinder_hierarchy(1)
    assert [h[0].coords.shape[0] for h in hier] == [671, 114]
    om = 0.5
    x = hier[0][0].model.inv_dt / 50.0 / float(R.alpha0(om))
    eff = float(R.alpha0(om)) * x
    u, un = P.case_state("ml1", hier[0][0])
    its = []
    for late in (False, True):
        probs = [h[0] if late else G.with_inv_dt(h[0], eff) for h in hier]
        with contextlib.ExitStack() as stack:
            fine = stack.enter_context(gpu_lib.DeviceSolver(probs[0]))
            coarse = stack.enter_context(gpu_lib.DeviceSolver(probs[1], shared_device=1))
            gpu_lib.attach_level_chain([fine, coarse], [hier[0][1]], theta=P.ML_THETA, sweeps=P.ML_SWEEPS)
            if late:
                fine.set_time_order(2)
                fine.set_state(un, un)
                fine.time_accept()     # one level: u_n = u_nm1 = un, so u* = un for every omega up to rounding
                fine.set_state(u, None)
                fine.set_time_step_bdf2(x, om)
            else:
                fine.set_state(u, un)
            fine.assemble(True)
            b = fine.spmv(P.x_true(fine.ndof))
            _, st = fine.linear_solve(b, gpu_lib.LINEAR_TWOLEVEL, rtol=1e-10)
            assert st["converged"]
            its.append(st["iterations"])
    print("BiCGStab iterations: hierarchy built with alpha0 x %d, BDF2 set-up afterwards %d" % tuple(its))
    assert its[0] == its[1]


# ---- order-2 runs against the reference loops -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cation,voltage", sorted(C.CASES))
def test_order_2_edl_run_against_the_reference_loop(gpu_lib, cation, voltage):
    from gmpnp_amd.edl1d import EDLRun
    c = C.CASES[(cation, voltage)]
    ep, base, pert = C.reference_runs(cation, voltage)
    s_err, s_u = T.sensitivity(base, pert)
    run = EDLRun(solver_parameters=G.SOLVER_1D, adaptive_dt=True, dt_order=2, dt_rtol=c["dt_rtol"], dt_atol=C.DT_ATOL, t_end=np.inf,
                 steady_tol=c["steady_tol"], max_steps=c["attempts"], L_n=1e-6, cation=cation, voltage_multiplier=voltage)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            run.run(verbose=False)
        log = run.stepper.log
        got = "".join("A" if r["accepted"] else ("F" if r["reason"] == 2 else "R") for r in log)
        dh = max(abs(r["h"] - b["h"]) / b["h"] for r, b in zip(log, base.log))
        derr = max(abs(r["err"] - b["err"]) for r, b in zip(log, base.log) if not np.isnan(b["err"]))
        du = float(np.abs(run.sys.dev.get_state() - base.u).max())
        print("%s %g: %s s_err %.3e s_u %.3e | device against the oracle: max |dh|/h %.3e  max |derr| %.3e  final state %.3e" %
              (cation, voltage, got, s_err, s_u, dh, derr, du))
        assert got == C.letters(base) and [r["order"] for r in log] == [b["order"] for b in base.log]
        assert [r["newton"] for r in log if r["reason"] != 2] == [b["newton"] for b in base.log if b["reason"] != 2]
        assert dh <= 10.0 * s_err and derr <= 10.0 * s_err
        assert du <= 10.0 * s_u
        assert run.stepper.stop_reason == "max_steps" and run.sys.time_history_levels() == 2
        assert len(run.history) == 1 + run.stepper.accepted == len(run.times) and np.all(np.diff(run.times) > 0.0)
        assert list(run.stepper.log_arrays()["order"]) == [b["order"] for b in base.log] and run.stepper.summary()["dt_order"] == 2
    finally:
        run.sys.close()


def test_frozen_controller_is_fixed_step_bdf2(gpu_lib):
    """dt_max = the reference step and weights so wide that every step is accepted: 5 steps of K+ at -2.5 are backward Euler twice
    (the start-up) and BDF2 with omega = 1 three times.  Against the NumPy march within 10 s_u, s_u the sensitivity of 5e's
    reference loop of this case to a 1e-8 perturbation of its accepted states (5e's bound for the device's final state)."""
    import test_time_step_reference as C1
    from gmpnp_amd.edl1d import EDLRun
    from conftest import _edl
    _, base, pert = C1.reference_runs("K", -2.5)
    _, s_u = T.sensitivity(base, pert)
    ep, _, prob = _edl(L_n=1e-6, cation="K", voltage_multiplier=-2.5)
    dt = ep.dts[0]
    nv, nf = prob.coords.shape[0], prob.nf
    un = np.tile(np.r_[np.ones(nf - 1), 0.0], nv)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        states = [un]
        u = np.zeros(prob.ndof)   # the run's first solve starts from u = 0
        for k in range(5):
            u, _, ok = R.solve_step(prob, u, states[-1], states[-2] if k >= 2 else None, dt, dt, lambda h: 1.0 / (h * ep.L_D), k >= 2, **C.NEWTON)
            assert ok
            states.append(u)
    run = EDLRun(solver_parameters=G.SOLVER_1D, adaptive_dt=True, dt_order=2, dt_rtol=1e6, dt_atol=1e6, max_steps=5, L_n=1e-6, cation="K",
                 voltage_multiplier=-2.5)
    try:
        run.stepper.policy.h_max = dt
        run.run(verbose=False)
        log = run.stepper.log
        assert [r["accepted"] for r in log] == [True] * 5 and [r["h"] for r in log] == [dt] * 5 and [r["order"] for r in log] == [1, 1, 2, 2, 2]
        du = [float(np.abs(h.ravel() - s).max()) for h, s in zip(run.history, states)]
        print("frozen controller: |device - NumPy| per state %s, s_u %.3e" % (["%.2e" % x for x in du], s_u))
        assert max(du) <= 10.0 * s_u
        # not backward Euler: the third state differs from a first-order march's by far more
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            be, _, _ = R.solve_step(prob, states[2], states[2], None, dt, dt, lambda h: 1.0 / (h * ep.L_D), False, **C.NEWTON)
        assert np.abs(be - states[3]).max() > 1e3 * s_u
    finally:
        run.sys.close()


def test_order_2_pore_steps_against_the_reference_loop(gpu_lib):
    """3D: ``AdaptiveStepper(order=2)`` with the band LU on the generated 259-vertex cylinder against the order-2 reference loop."""
    from gmpnp_amd.problem import pore_dirichlet
    from gmpnp_amd.solver import GMPNPSystem, column_medians
    from gmpnp_amd.timestep import AdaptiveStepper, TimeStepPolicy
    base, pert = C.pore_reference(0.0), C.pore_reference(1e-8)
    s_err, s_u = T.sensitivity(base, pert)
    pp, bnd, prob = G.small_pore()
    params = {"nonlinear_solver": "newton", "newton_solver": {"linear_solver": "band_lu", "maximum_iterations": 50, "relative_tolerance": 1e-9,
                                                              "absolute_tolerance": 1e-6, "relaxation_parameter": 0.9}}
    sys_ = GMPNPSystem(prob)
    try:
        sys_.initialise([1.0] * 8 + [0.0])
        stepper = AdaptiveStepper(sys_, TimeStepPolicy(), (RTOL, C.DT_ATOL), lambda h: 1.0 / h, 10.0 * pp.dt, solver_parameters=params, order=2)

        def before_accept(st):
            row = sys_.vertex_values()
            sys_.set_bcs(*pore_dirichlet(pp, bnd, pp.sechenov_co2_scaled(*column_medians(row, (1, 2, 3, 7)))))
        for _ in range(C.PORE_ATTEMPTS):
            stepper.attempt(None, before_accept)
        log = stepper.log
        dh = max(abs(r["h"] - b["h"]) / b["h"] for r, b in zip(log, base.log))
        derr = max(abs(r["err"] - b["err"]) for r, b in zip(log, base.log) if not np.isnan(b["err"]))
        du = float(np.abs(sys_.dev.get_state(previous=True) - base.u).max())
        print("pore (259 vertices): %s orders %s s_err %.3e s_u %.3e | device against the oracle: max |dh|/h %.3e  max |derr| %.3e  final state %.3e" %
              (C.letters(base), [r["order"] for r in log], s_err, s_u, dh, derr, du))
        assert [r["accepted"] for r in log] == base.sequence() and [r["reason"] == 2 for r in log] == base.failures()
        assert [r["order"] for r in log] == [b["order"] for b in base.log]
        assert [r["newton"] for r in log if r["reason"] != 2] == [b["newton"] for b in base.log if b["reason"] != 2]
        assert dh <= 10.0 * s_err and derr <= 10.0 * s_err and du <= 10.0 * s_u
    finally:
        sys_.close()


def test_order_2_pore_run_with_budget(gpu_lib, tmp_path, monkeypatch):
    """PoreRun(adaptive_dt=True, dt_order=2, budget=True) on L_10_R_5 from 10 reference steps: the clock, the history and the CO2
    Dirichlet value survive rejections, the ``order`` column follows the levels, and on an accepted order-2 step the budget closes
    as on an order-1 step of the same run: |closure_f| <= sqrt(n_free_f) times the step's last Newton residual (its storage term
    reads alpha0 inv_dt and u*, the time derivative that was solved)."""
    import budget_reference as B
    from gmpnp_amd.pore3d import PoreRun
    monkeypatch.setenv("GMPNP_OUT", str(tmp_path))
    run = PoreRun(concentration_elec=0.5, L=10e-9, R=5e-9, adaptive_dt=True, dt_order=2, max_steps=10, budget=True)
    try:
        run.stepper.h = 10.0 * run.pp.dt
        residual = []
        while run.stepper.stop_reason is None and len(run.stepper.log) < 10:
            n, t, bc, levels = run.n, run.t, run.co2_bc, run.sys.time_history_levels()
            row = run.adaptive_step(verbose=False)
            assert row["order"] == (2 if levels >= 2 else 1)
            if row["accepted"]:
                assert run.n == n + 1 and run.t == t + row["h"] == run.times[-1] and run.co2_bc is not None
                assert run.sys.time_history_levels() == min(levels + 1, 2)
                residual.append((row["order"], run.sys.last_stats["residuals"][-1]))
            else:   # the clock, the history, the levels and the CO2 Dirichlet value stay
                assert run.n == n and run.t == t and run.co2_bc == bc and run.sys.time_history_levels() == levels
            assert len(run.history) == 1 + run.n == len(run.times) and len(run.budget.tables) == run.n
        log = run.stepper.log
        print("pore L_10_R_5 order 2:", "".join("A" if r["accepted"] else "R" for r in log), [r["order"] for r in log], [r["newton"] for r in log],
              ["%.3g" % r["err"] for r in log])
        orders = [o for o, _ in residual]
        assert orders.count(2) >= 2 and orders.count(1) == 2 and any(not r["accepted"] for r in log)
        assert np.array_equal(run.sys.dev.get_state(previous=True), run.history[-1].ravel())
        t = run.budget.array()
        nfree = B.n_free(run.problem)
        ratio = {1: 0.0, 2: 0.0}
        for k, (o, res) in enumerate(residual):
            bound = np.sqrt(nfree) * res
            ratio[o] = max(ratio[o], float((np.abs(t[k, :, B.CLO]) / np.where(bound > 0, bound, 1.0)).max()))
            assert (np.abs(t[k, :, B.CLO]) <= bound).all(), (k, o)
        print("max |closure| / (sqrt(n_free) residual): order 1 %.3e, order 2 %.3e" % (ratio[1], ratio[2]))
        # the second accepted order-2 step against the estimator on the history rows (pins u_nm2 and the order of the glue)
        acc = [r for r in log if r["accepted"]]
        free = T.free_mask(run.problem)
        m = R.time_error2(run.history[4], run.history[3], run.history[2], run.history[1], acc[3]["h"], acc[2]["h"], acc[1]["h"], 1e-2, 1e-4, free)
        assert acc[3]["order"] == 2 and abs(acc[3]["err"] - m["err"]) <= 1e-10 * m["err"] and acc[3]["worst_dof"] == m["worst_dof"]
        out = run.write_outputs()
        meta = json.load(open(os.path.join(out, "metadata.json")))
        assert meta["dt_order"] == 2 and meta["steps_accepted"] == run.n
        assert list(np.load(os.path.join(out, meta["timestep_log"]))["order"]) == [r["order"] for r in log]
    finally:
        run.sys.close()


@pytest.mark.parametrize("name", ["rxn_diff", "rxn_pore"])
def test_reaction_diffusion_drivers_at_order_2(gpu_lib, name):
    """The two reaction-diffusion drivers carry ``dt_order`` through ``pop_adaptive``: 12 attempts from 10 reference steps, the
    ``order`` column follows the levels (BDF2 from the third accepted state on) and the bookkeeping holds."""
    make, ref_step = G.driver_cases()[name]
    run = make(adaptive_dt=True, dt_order=2, max_steps=12)
    try:
        run.stepper.h = 10.0 * ref_step(run)
        levels = []
        while run.stepper.stop_reason is None and len(run.stepper.log) < 12:
            levels.append(run.sys.time_history_levels())
            run.step(verbose=False)
        log = run.stepper.log
        print(name, "".join("A" if r["accepted"] else "R" for r in log), [r["order"] for r in log], [r["newton"] for r in log], ["%.3g" % r["err"] for r in log])
        assert len(log) == 12 and [r["order"] for r in log] == [2 if lv >= 2 else 1 for lv in levels]
        assert sum(r["order"] == 2 for r in log) >= 1 and run.n == run.stepper.accepted >= 3
        assert run.sys.time_history_levels() == 2
        assert len(run.history) == 1 + run.n == len(run.times) and np.all(np.diff(run.times) > 0.0) and run.t == run.times[-1]
        assert run.stepper.summary()["dt_order"] == 2
    finally:
        run.sys.close()


def test_order_1_runs_have_no_order_column(gpu_lib):
    """The default: no ``order`` in the log rows, the log arrays or the metadata keys, and the levels are never asked for."""
    from gmpnp_amd.edl1d import EDLRun
    run = EDLRun(adaptive_dt=True, max_steps=3, L_n=1e-6, cation="K", voltage_multiplier=-2.5)
    try:
        run.run(verbose=False)
        assert all("order" not in r for r in run.stepper.log) and "order" not in run.stepper.log_arrays() and "dt_order" not in run.stepper.summary()
        assert run.sys.time_history_levels() == 1
        with pytest.raises(gpu_lib.GmpnpError):
            run.sys.dev.get_time_history()
    finally:
        run.sys.close()


def test_driver_command_line_with_order_2(gpu_lib, tmp_path):
    env = dict(os.environ, GMPNP_OUT=str(tmp_path))
    cmd = ["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "1D", "MPNP_CO2ER_EDL.py"), "--L_n=1e-6", "--voltage_multiplier=-2.5",
           "--adaptive_dt", "--dt_order", "2", "--max_steps", "20"]
    subprocess.run(cmd, check=True, env=env, cwd=str(tmp_path), capture_output=True, text=True)
    metas = [os.path.join(d, f) for d, _, fs in os.walk(str(tmp_path)) for f in fs if f == "metadata.json"]
    assert len(metas) == 1
    out = os.path.dirname(metas[0])
    meta = json.load(open(metas[0]))
    assert meta["adaptive_dt"] is True and meta["dt_order"] == 2 and meta["stop_reason"] == "max_steps"
    log = np.load(os.path.join(out, meta["timestep_log"]))
    assert len(log["order"]) == 20 == meta["steps_accepted"] + meta["steps_rejected"]
    assert list(log["order"][:5]) == [1] * 5 and set(log["order"][5:]) == {2}   # the reference loop's start-up (A R R R A)
    arr = np.load(os.path.join(out, "arrays_unscaled.npz"))
    assert len(arr["tau"]) == arr["H"].shape[0] == meta["steps_accepted"] + 1 and np.all(np.diff(arr["tau"]) > 0.0)


# ---- observed order on the device -----------------------------------------------------------------------------------------------------
def test_observed_order_on_the_device(gpu_lib):
    """tests/test_time_order_reference.py's refinement study through ``DeviceSolver``: the same start state, the same thresholds
    (above 3 at order 2, below 2.5 at order 1)."""
    ep, prob, u0 = C.order_start_state()
    dt = ep.dts[0]
    opts = gpu_lib.newton_options({"nonlinear_solver": "newton", "newton_solver": dict(C.TIGHT)}, dim=1)
    out = {}
    with gpu_lib.DeviceSolver(prob) as dev:
        def march(m, order):
            h = m * dt
            dev.set_time_order(order)
            dev.set_state(u0, u0)
            for k in range(64 // m):
                if order == 2 and k >= 1:
                    dev.set_time_step_bdf2(1.0 / (h * ep.L_D), 1.0)
                else:
                    dev.set_time_step(1.0 / (h * ep.L_D))
                st = dev.newton_solve(opts)
                assert st["converged"]
                dev.time_accept()
            return dev.get_state()
        for order in (2, 1):
            out[order] = C.refinement_ratios(lambda m: march(m, order))
            print("order %d on the device: differences %s ratios %.3f %.3f" % (order, out[order][2], out[order][0], out[order][1]))
    assert out[2][0] > 3.0 and out[2][1] > 3.0
    assert out[1][0] < 2.5 and out[1][1] < 2.5


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_partition_handles_and_ensembles_refuse_order_2(gpu_lib, pore10):
    from gmpnp_amd.dist import PartitionedSolver
    from gmpnp_amd.solver import PartitionedSystem
    ps = PartitionedSolver(pore10[2], 2)
    try:
        lib, h = ps.devs[0].lib, ps.devs[0]._h
        tol, out, lv = gpu_lib.CTimeTol(), gpu_lib.CTimeError(), c_int32()
        tol.rtol = 1e-2
        for f in range(9):
            tol.atol[f] = 1e-4
        star = np.zeros(ps.devs[0].ndof)
        assert lib.gmpnp_set_time_order(h, 2) == gpu_lib.ERR_INVALID
        assert lib.gmpnp_set_time_order(h, 1) == gpu_lib.ERR_INVALID
        assert lib.gmpnp_time_history_levels(h, byref(lv)) == gpu_lib.ERR_INVALID
        assert lib.gmpnp_set_time_step_bdf2(h, 1.0, 1.0) == gpu_lib.ERR_INVALID
        assert lib.gmpnp_time_error_bdf2(h, 1.0, 1.0, 1.0, byref(tol), byref(out)) == gpu_lib.ERR_INVALID
        assert lib.gmpnp_get_time_history(h, star.ctypes.data_as(POINTER(c_double))) == gpu_lib.ERR_INVALID
        with pytest.raises(gpu_lib.GmpnpError) as ei:
            ps.devs[0].time_kernel(23, 2)
        assert ei.value.code == gpu_lib.ERR_INVALID
    finally:
        ps.close()
    for name in ("set_time_order", "time_history_levels", "set_time_step_bdf2", "time_error_bdf2"):
        with pytest.raises(ValueError):
            getattr(PartitionedSystem, name)(None)
    # an ensemble with an order-2 member: every call that solves, estimates or advances
    prob = G.estimator_problem("257")
    u, un, _ = G.triple(prob, seed=77)
    opts = gpu_lib.newton_options(G.SOLVER_1D, dim=1)
    with contextlib.ExitStack() as stack:
        devs = [stack.enter_context(gpu_lib.DeviceSolver(prob)) for _ in range(2)]
        for d in devs:
            d.set_state(u.ravel(), un.ravel())
        ens = stack.enter_context(gpu_lib.DeviceEnsemble(devs))
        devs[1].set_time_order(2)
        for call in (lambda: ens.newton_solve(opts), lambda: ens.set_time_step([1.0, 1.0]),
                     lambda: ens.time_error([0.1, 0.1], [0.1, 0.1], [1e-2, 1e-2], [1e-4, 1e-4]), lambda: ens.time_advance([1, 1]),
                     lambda: ens.assign_previous()):
            with pytest.raises(gpu_lib.GmpnpError) as ei:
                call()
            assert ei.value.code == gpu_lib.ERR_INVALID and "order 2" in str(ei.value)
        devs[1].set_time_order(1)   # back at order 1 the member joins again
        ens.set_time_step([prob.model.inv_dt, prob.model.inv_dt])
        ens.time_advance([1, 1])
        assert [d.time_history_levels() for d in devs] == [1, 1]
