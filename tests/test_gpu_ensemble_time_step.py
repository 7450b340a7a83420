"""Adaptive time stepping of device ensembles on the GPU (include/gmpnp.h: gmpnp_ensemble_set_time_step / _time_error / _time_advance,
csrc/gmpnp_time_step_ens.h, gmpnp_amd/timestep.py ``EnsembleStepper``).

The batched estimator against the NumPy model (1e-12 relative, the single call's bound: both sum the same <= 1,767 squares in
different orders) and, bit for bit, against ``time_error`` on each member alone; the batched accept / reject against twin handles;
``set_time_step`` against handles created with the step; adaptive ensembles against each member's own serial adaptive run, bit for
bit (the arithmetic and the order of the sums are the same: a deviation means the bodies are not shared)."""
import contextlib
import ctypes
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import test_gpu_time_step as G
import test_time_step_reference as C
import time_step_reference as T
from conftest import ROOT

pytestmark = pytest.mark.gpu

estimator_problem, triple, load = G.estimator_problem, G.triple, G.load


def same(a, b):
    """``==`` on every field of two ``time_error`` dicts (NaN fields: both NaN)."""
    assert a.keys() == b.keys()
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True) for k in a)


def problem(name):
    if name == "small_pore":
        return G.small_pore()[2]
    return estimator_problem(name)


def device_kwargs(prob):
    return {"shared_device": 1} if prob.nf == 9 else {}   # 3D members keep to one stream


@contextlib.contextmanager
def members(gpu_lib, prob, n):
    with contextlib.ExitStack() as stack:
        devs = [stack.enter_context(gpu_lib.DeviceSolver(prob, **device_kwargs(prob))) for _ in range(n)]
        yield devs, stack.enter_context(gpu_lib.DeviceEnsemble(devs))


def member_arguments(k, nf):
    """Member k's own h, h_prev, rtol and per-field atol."""
    return G.H_STEP * (1.0 + 0.3 * k), G.H_PREV * (1.0 + 0.2 * (k % 5)), G.RTOL * (1.0 + k % 3), np.linspace(1e-4, 3e-4, nf) * (1.0 + 0.5 * (k % 4))


def plants(prob):
    """The dofs a dominant term is planted at: a field of the first node, one of the last free node, every field of a mid node."""
    nv, nf = prob.coords.shape[0], prob.nf
    free = T.free_mask(prob)
    I_last = int(np.nonzero(free.any(axis=1))[0][-1])
    out = [(0, f) for f in range(nf) if free[0, f]][:1] + [(I_last, f) for f in range(nf) if free[I_last, f]][-1:]
    return out + [(nv // 2, f) for f in range(nf) if free[nv // 2, f]]


def check_members(gpu_lib, prob, n, rounds):
    """n members with different states and arguments, the last of n > 1 without history; round r plants a dominant term at
    plants[(r + k) % len] of member k (in u_nm1: the weights do not see it).  Every report against the NumPy model and against the
    single call on that member alone."""
    nv, nf = prob.coords.shape[0], prob.nf
    free, P = T.free_mask(prob), plants(prob)
    states = [triple(prob, seed=100 * nv + k) for k in range(n)]
    args = [member_arguments(k, nf) for k in range(n)]
    no_history = n - 1 if n > 1 else None
    with members(gpu_lib, prob, n) as (devs, ens):
        for r in range(rounds):
            planted = []
            for k, (dev, (u, un, unm1)) in enumerate(zip(devs, states)):
                I, f = P[(r + k) % len(P)]
                mp = unm1.copy()
                mp[I, f] += 1e3
                planted.append((mp, I * nf + f))
                if k == no_history:
                    dev.set_state(u.ravel(), un.ravel())
                else:
                    load(dev, u, un, mp)
            h, hp, rtol, atol = (list(x) for x in zip(*args))
            got = ens.time_error(h, hp, rtol, atol)
            again = ens.time_error(h, hp, rtol, atol)
            for k, dev in enumerate(devs):
                u, un, _ = states[k]
                hist = None if k == no_history else planted[k][0]
                G.compare(got[k], T.time_error(u, un, hist, h[k], hp[k], rtol[k], atol[k], free), nf)
                assert got[k]["worst_dof"] == (-1 if k == no_history else planted[k][1])
                assert got[k]["has_history"] == (k != no_history)
                assert same(got[k], dev.time_error(h[k], hp[k], rtol[k], atol[k])), k
                assert same(got[k], again[k]), k


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("name", ["2", "255", "256", "257", "513"])
def test_member_reports_are_the_single_calls(gpu_lib, name, n):
    """Both sides of the 256-node workgroup boundary and the single-workgroup reduce, 1 ... 3 members; every plant visits every
    member once (as many rounds as plants)."""
    prob = estimator_problem(name)
    check_members(gpu_lib, prob, n, rounds=len(plants(prob)))


@pytest.mark.parametrize("name", ["2", "257"])
def test_sixty_four_members(gpu_lib, name):
    check_members(gpu_lib, estimator_problem(name), 64, rounds=1)


@pytest.mark.parametrize("name", ["small_pore", "pore10"])
def test_nine_fields(gpu_lib, name):
    prob = problem(name)
    assert prob.nf == 9 and prob.coords.shape[0] == {"small_pore": 259, "pore10": 1767}[name]
    check_members(gpu_lib, prob, 3, rounds=3)


def test_mask_and_isolation(gpu_lib):
    prob = estimator_problem("257")
    nv, nf = prob.coords.shape[0], prob.nf
    states = [triple(prob, seed=40 + k) for k in range(3)]
    h, hp, rtol, atol = (list(x) for x in zip(*[member_arguments(k, nf) for k in range(3)]))
    with members(gpu_lib, prob, 3) as (devs, ens):
        for dev, s in zip(devs, states):
            load(dev, *s)
        full = ens.time_error(h, hp, rtol, atol)
        # a masked-out member: its row is zero, its estimator storage is not written (its own next single call is unchanged, and a
        # call that lists it alone gives the bits of the full call)
        part = ens.time_error(h, hp, rtol, atol, mask=[1, 0, 1])
        assert same(part[0], full[0]) and same(part[2], full[2])
        z = part[1]
        assert z["err"] == 0.0 and z["rate"] == 0.0 and z["worst_dof"] == 0 and not z["has_history"] and not z["nonfinite"]
        assert not np.any(z["err_field"]) and not np.any(z["rate_field"])
        assert same(ens.time_error(h, hp, rtol, atol, mask=[0, 1, 0])[1], full[1])
        # a NaN planted in member 1: only its nonfinite flag, the others' reports are those of a call without it
        bad = states[1][0].copy()
        bad[nv // 3, 1] = np.nan
        devs[1].set_state(bad.ravel(), None)
        nan = ens.time_error(h, hp, rtol, atol)
        assert nan[1]["nonfinite"] and np.isnan(nan[1]["err"]) and np.all(np.isnan(nan[1]["err_field"])) and np.isnan(nan[1]["rate"])
        without = ens.time_error(h, hp, rtol, atol, mask=[1, 0, 1])
        for k in (0, 2):
            assert not nan[k]["nonfinite"] and same(nan[k], without[k]) and same(nan[k], full[k])


@pytest.mark.parametrize("name", ["257", "small_pore"])
def test_time_advance_against_twin_handles(gpu_lib, name):
    """Actions (0, 1, 2) on three members: member 0 keeps u and u_n and its next estimate, member 1 is a twin handle after
    time_accept, member 2 a twin after time_reject (states, next estimate, history)."""
    prob = problem(name)
    nf = prob.nf
    states = [triple(prob, seed=60 + k) for k in range(3)]
    u2 = triple(prob, seed=70)[0]
    h, hp, rtol, atol = (list(x) for x in zip(*[member_arguments(k, nf) for k in range(3)]))
    with members(gpu_lib, prob, 3) as (devs, ens), members(gpu_lib, prob, 3) as (twins, _):
        for dev, twin, s in zip(devs, twins, states):
            load(dev, *s)
            load(twin, *s)
        devs[2].set_state(None, states[2][1].ravel())   # member 2 has no history: the reject must not make one
        twins[2].set_state(None, states[2][1].ravel())
        before = ens.time_error(h, hp, rtol, atol)
        ens.time_advance([0, 1, 2])
        twins[1].time_accept()
        twins[2].time_reject()
        for k in range(3):
            assert np.array_equal(devs[k].get_state(), twins[k].get_state()), k
            assert np.array_equal(devs[k].get_state(previous=True), twins[k].get_state(previous=True)), k
        assert np.array_equal(devs[0].get_state(), states[0][0].ravel()) and np.array_equal(devs[0].get_state(previous=True), states[0][1].ravel())
        assert np.array_equal(devs[1].get_state(previous=True), states[1][0].ravel())
        assert np.array_equal(devs[2].get_state(), states[2][1].ravel())
        assert same(ens.time_error(h, hp, rtol, atol)[0], before[0])
        # the next estimate: u2 on every member; member 1's u_nm1 is its former u_n, member 2 still has no history
        for d in list(devs) + list(twins):
            d.set_state(u2.ravel(), None)
        after = ens.time_error(h, hp, rtol, atol)
        for k in range(3):
            assert same(after[k], twins[k].time_error(h[k], hp[k], rtol[k], atol[k])), k
        assert after[1]["has_history"] and not after[2]["has_history"]
        G.compare(after[1], T.time_error(u2, states[1][0], states[1][1], h[1], hp[1], rtol[1], atol[1], T.free_mask(prob)), nf)
        # the history is shared with the single-handle calls: an accept on the member alone is seen by the ensemble
        devs[2].time_accept()
        assert ens.time_error(h, hp, rtol, atol)[2]["has_history"]


@pytest.mark.parametrize("name", ["edl1", "pore10"])
def test_set_time_step_equals_handles_created_with_the_steps(gpu_lib, name):
    prob = estimator_problem(name)
    u, un, _ = triple(prob, seed=31)
    x = [prob.model.inv_dt / 7.0, 0.0, prob.model.inv_dt * 3.0]
    kw = device_kwargs(prob)
    with members(gpu_lib, prob, 3) as (devs, ens), contextlib.ExitStack() as stack:
        made = [stack.enter_context(gpu_lib.DeviceSolver(G.with_inv_dt(prob, xk), **kw)) for xk in x]
        for d in list(devs) + made:
            d.set_state(u.ravel(), un.ravel())
        F0, r0 = devs[0].assemble(True)   # Jacobians at the old step, to be invalidated
        J0 = devs[0].jacobian_csr().data.copy()
        # a NaN at member 1: refused, the message names the member, member 0 is unchanged
        with pytest.raises(gpu_lib.GmpnpError, match="member 1") as ei:
            ens.set_time_step([x[0], np.nan, x[2]])
        assert ei.value.code == gpu_lib.ERR_INVALID
        F, r = devs[0].assemble(True)
        assert np.array_equal(F, F0) and r == r0 and np.array_equal(devs[0].jacobian_csr().data, J0)
        ens.set_time_step(x)
        for a, b in zip(devs, made):
            Fa, ra = a.assemble(True)
            Fb, rb = b.assemble(True)
            assert np.array_equal(Fa, Fb) and ra == rb and np.all(np.isfinite(Fa))
            Ja, Jb = a.jacobian_csr(), b.jacobian_csr()
            assert np.array_equal(Ja.indptr, Jb.indptr) and np.array_equal(Ja.indices, Jb.indices) and np.array_equal(Ja.data, Jb.data)


def test_refusals_through_ctypes(gpu_lib):
    prob = estimator_problem("257")
    nf = prob.nf
    with members(gpu_lib, prob, 2) as (devs, ens):
        lib = ens.lib
        tol, out = (gpu_lib.CTimeTol * 2)(), (gpu_lib.CTimeError * 2)()
        for k in range(2):
            tol[k].rtol = 1e-2
            for f in range(nf):
                tol[k].atol[f] = 1e-4
        d2, i2 = ctypes.c_double * 2, ctypes.c_int32 * 2
        for dev in devs:
            dev.set_state(*[x.ravel() for x in triple(prob, seed=3)[:2]])
        u_before = devs[0].get_state()
        assert lib.gmpnp_ensemble_time_advance(ens._h, i2(1, 3)) == gpu_lib.ERR_INVALID and b"member 1" in lib.gmpnp_last_error()
        assert np.array_equal(devs[0].get_state(previous=True), triple(prob, seed=3)[1].ravel()) and np.array_equal(devs[0].get_state(), u_before)
        assert lib.gmpnp_ensemble_time_error(ens._h, d2(1.0, 0.0), d2(1.0, 1.0), tol, None, out) == gpu_lib.ERR_INVALID
        assert b"member 1" in lib.gmpnp_last_error()
        assert lib.gmpnp_ensemble_time_error(ens._h, d2(1.0, 0.0), d2(1.0, 1.0), tol, i2(1, 0), out) == gpu_lib.OK   # not listed: not judged
        tol[0].atol[2] = 0.0
        assert lib.gmpnp_ensemble_time_error(ens._h, d2(1.0, 1.0), d2(1.0, 1.0), tol, None, out) == gpu_lib.ERR_INVALID
        assert b"member 0" in lib.gmpnp_last_error() and b"atol" in lib.gmpnp_last_error()
        tol[0].atol[2] = 1e-4
        # SUPG set on a member after the ensemble was made: all three calls check the membership conditions again
        devs[1].set_supg(np.zeros((prob.coords.shape[0], nf - 1)), np.arange(nf - 1, dtype=np.int32))
        assert lib.gmpnp_ensemble_time_error(ens._h, d2(1.0, 1.0), d2(1.0, 1.0), tol, None, out) == gpu_lib.ERR_INVALID
        assert b"member 1" in lib.gmpnp_last_error() and b"SUPG" in lib.gmpnp_last_error()
        assert lib.gmpnp_ensemble_time_advance(ens._h, i2(1, 1)) == gpu_lib.ERR_INVALID
        assert lib.gmpnp_ensemble_set_time_step(ens._h, d2(1.0, 1.0)) == gpu_lib.ERR_INVALID


# ---- runs: every member against its own serial adaptive run -------------------------------------------------------------------------
ROW_KEYS = ("t", "h", "accepted", "reason", "err", "rate", "newton", "worst_dof", "steric_excursion")


def rows_equal(a, b, keys):
    assert len(a) == len(b), (len(a), len(b))
    for n, (x, y) in enumerate(zip(a, b)):
        for key in keys:
            assert x[key] == y[key] or (x[key] != x[key] and y[key] != y[key]), (n, key, x[key], y[key])


def letters(log):
    return "".join("A" if r["accepted"] else ("F" if r["reason"] == 2 else "R") for r in log)


EDL_MEMBERS = [dict(cation="K", voltage_multiplier=-2.5), dict(cation="Cs", voltage_multiplier=-10.0), dict(cation="K", voltage_multiplier=-5.0)]
EDL_ADAPTIVE = dict(dt_rtol=[5e-2, 1e-2, 5e-2], dt_atol=C.DT_ATOL, steady_tol=[1e-5, 0.0, 1e-5], t_end=np.inf, max_steps=[None, 12, 60])


def edl_adaptive(k):
    return {key: (v[k] if isinstance(v, list) else v) for key, v in EDL_ADAPTIVE.items()}


_serial_edl = {}


def serial_edl(k):
    """The serial adaptive ``EDLRun`` of member k (closed; its log, states, history and times kept), run once."""
    from gmpnp_amd.edl1d import EDLRun
    key = k
    if key not in _serial_edl:
        run = EDLRun(solver_parameters=G.SOLVER_1D, adaptive_dt=True, L_n=1e-6, **edl_adaptive(k), **EDL_MEMBERS[k])
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                run.run(verbose=False)
            _serial_edl[key] = dict(log=run.stepper.log, u=run.sys.dev.get_state(), un=run.sys.dev.get_state(previous=True), history=run.history,
                                    times=run.times, stop=run.stepper.stop_reason, newton_its=run.newton_its)
        finally:
            run.sys.close()
    return _serial_edl[key]


def assert_edl_member(run, ref):
    rows_equal(run.stepper.log, ref["log"], ROW_KEYS)
    assert np.array_equal(run.sys.dev.get_state(), ref["u"]) and np.array_equal(run.sys.dev.get_state(previous=True), ref["un"])
    assert len(run.history) == len(ref["history"]) and all(np.array_equal(a, b) for a, b in zip(run.history, ref["history"]))
    assert run.times == ref["times"] and run.stepper.stop_reason == ref["stop"] and run.newton_its == ref["newton_its"]


def test_adaptive_edl_ensemble_against_the_serial_runs(gpu_lib):
    """K -2.5 (38 attempts, steady), Cs -10 (FFARRRAAAAAA, max_steps) and K -5: Newton failures, error rejections and members leaving
    at different rounds."""
    from gmpnp_amd.edl_ensemble import EDLEnsemble
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with EDLEnsemble([dict(m, L_n=1e-6) for m in EDL_MEMBERS], adaptive_dt=True, solver_parameters=G.SOLVER_1D, **EDL_ADAPTIVE) as ens:
            ens.run()
            print([letters(r.stepper.log) for r in ens.runs], [r.stepper.stop_reason for r in ens.runs], "rounds", ens.stepper.rounds)
            for k, run in enumerate(ens.runs):
                assert ens.errors[k] is None
                assert_edl_member(run, serial_edl(k))
            assert len(ens.runs[0].stepper.log) == 38 and ens.runs[0].stepper.stop_reason == "steady"
            assert letters(ens.runs[1].stepper.log) == "FFARRRAAAAAA" and ens.runs[1].stepper.stop_reason == "max_steps"
            assert ens.stepper.rounds == max(len(r.stepper.log) for r in ens.runs)


def test_a_pnp_member_beside_mpnp_members(gpu_lib):
    """A PNP member at -5 V beside MPNP members (max_steps 20 each).  Whatever becomes of it — an ``errors`` text for a status outside
    ``timestep.RETRY_CODES``, or its own serial run's attempts (a Newton failure is a failed attempt, tried again) — the neighbours'
    logs and states are those of an ensemble without it."""
    from gmpnp_amd.edl_ensemble import EDLEnsemble
    from gmpnp_amd.timestep import RETRY_CODES
    mp = [dict(cation="K", voltage_multiplier=-2.5, L_n=1e-6), dict(cation="K", voltage_multiplier=-5.0, L_n=1e-6)]
    pnp = dict(model="PNP", voltage_multiplier=-5.0, L_n=1e-6)
    ad = dict(dt_rtol=5e-2, dt_atol=C.DT_ATOL, t_end=np.inf, max_steps=20)
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name, mem in (("with", [mp[0], pnp, mp[1]]), ("without", mp)):
            with EDLEnsemble(mem, adaptive_dt=True, solver_parameters=G.SOLVER_1D, **ad) as ens:
                ens.run()
                out[name] = [(r.stepper.log, r.sys.dev.get_state(), r.sys.dev.get_state(previous=True), r.stepper.stop_reason) for r in ens.runs]
                if name == "with":
                    err, log = ens.errors[1], ens.runs[1].stepper.log
                    print("PNP -5:", err or letters(log), ens.runs[1].stepper.stop_reason)
                    assert ens.errors[0] is None and ens.errors[2] is None
                    if err is not None:
                        assert ens.status[1] not in (0,) + tuple(RETRY_CODES) and ens.failed_step[1] is not None
    for a, b in zip([out["with"][0], out["with"][2]], out["without"]):
        rows_equal(a[0], b[0], ROW_KEYS)
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]


PORE = dict(concentration_elec=0.5, L=10e-9, R=5e-9)
PORE_MEMBERS = [dict(), dict(H2_FE=0.2), dict(current_rough=1500.0)]


def test_adaptive_pore_ensemble_against_the_serial_runs(gpu_lib):
    """L_10_R_5 at 0.5 M from dt_init = 10 reference steps, 8 attempts, with budgets: log rows (krylov too), states, the CO2
    Dirichlet value after every accepted step and the budget logs."""
    from gmpnp_amd.pore3d import PoreRun
    from gmpnp_amd.pore_ensemble import PoreEnsemble
    dt = None
    ref = []
    for m in PORE_MEMBERS:
        run = PoreRun(adaptive_dt=True, max_steps=8, budget=True, device_kwargs={"shared_device": 1}, **PORE, **m)
        try:
            dt = run.pp.dt
            run.stepper.h = 10.0 * dt
            co2 = []
            while run.stepper.stop_reason is None and len(run.stepper.log) < 8:
                if run.adaptive_step(verbose=False)["accepted"]:
                    co2.append(run.co2_bc)
            ref.append(dict(log=run.stepper.log, u=run.sys.dev.get_state(), un=run.sys.dev.get_state(previous=True), co2=co2, times=run.times,
                            budget=[np.array(t) for t in run.budget.tables], history=run.history))
        finally:
            run.sys.close()
    with PoreEnsemble([dict(PORE, **m) for m in PORE_MEMBERS], adaptive_dt=True, dt_init=10.0 * dt, max_steps=8, budget=True) as ens:
        co2 = [[] for _ in ens.runs]
        while ens.stepper.live():
            for k, row in ens.step().items():
                if row["accepted"]:
                    co2[k].append(ens.runs[k].co2_bc)
        print([letters(r.stepper.log) for r in ens.runs], [[q["krylov"] for q in r.stepper.log] for r in ens.runs])
        for k, run in enumerate(ens.runs):
            assert ens.errors[k] is None and run.stepper.stop_reason == "max_steps"
            rows_equal(run.stepper.log, ref[k]["log"], ROW_KEYS + ("krylov",))
            assert np.array_equal(run.sys.dev.get_state(), ref[k]["u"]) and np.array_equal(run.sys.dev.get_state(previous=True), ref[k]["un"])
            assert co2[k] == ref[k]["co2"] and run.times == ref[k]["times"]
            assert len(run.budget.tables) == len(ref[k]["budget"]) and all(np.array_equal(np.array(a), b) for a, b in zip(run.budget.tables, ref[k]["budget"]))
            assert len(run.history) == len(ref[k]["history"]) and all(np.array_equal(a, b) for a, b in zip(run.history, ref[k]["history"]))
        assert any(not r["accepted"] for r in ens.runs[0].stepper.log)


def test_fixed_step_ensembles_do_not_see_the_feature(gpu_lib):
    """Fixed-step ensembles over 3 steps with the ensemble estimator allocated and run between the steps: bitwise the same runs
    without it."""
    from gmpnp_amd.edl_ensemble import EDLEnsemble
    from gmpnp_amd.pore_ensemble import PoreEnsemble
    makers = (lambda: EDLEnsemble([dict(voltage_multiplier=-2.5, L_n=1e-6), dict(voltage_multiplier=-5.0, cation="Cs", L_n=1e-6)], num_steps=3),
              lambda: PoreEnsemble([dict(PORE), dict(PORE, H2_FE=0.2)], num_steps=3))
    for make in makers:
        with make() as a, make() as b:
            assert a.stepper is None and b.stepper is None
            n = len(a.runs)
            for _ in range(3):
                a.step()
                b.step()
                e = b._ensemble(b.live()).time_error([1.0] * n, [1.0] * n, [1e-2] * n, [1e-4] * n)
                assert len(e) == n and not any(x["has_history"] for x in e)
            for ra, rb in zip(a.runs, b.runs):
                assert np.array_equal(ra.sys.dev.get_state(), rb.sys.dev.get_state())
                assert np.array_equal(ra.sys.dev.get_state(previous=True), rb.sys.dev.get_state(previous=True))
                assert ra.newton_its == rb.newton_its


def test_sweep_command_line(gpu_lib, tmp_path):
    env = dict(os.environ, GMPNP_OUT=str(tmp_path), PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = ["timeout", "-k", "10", "120", sys.executable, "-m", "gmpnp_amd.edl_sweep", "--L_n", "1e-6", "--voltage_multiplier", "-2.5", "-5",
           "--adaptive_dt", "--dt_rtol", "5e-2", "--steady_tol", "1e-5", "--t_end", "1e9", "--max_steps", "60"]
    subprocess.run(cmd, check=True, env=env, cwd=str(tmp_path), capture_output=True, text=True)
    metas = sorted(os.path.join(d, f) for d, _, fs in os.walk(str(tmp_path)) for f in fs if f == "metadata.json")
    assert len(metas) == 2
    for m in metas:
        meta = json.load(open(m))
        assert os.path.exists(os.path.join(os.path.dirname(m), "timestep_log.npz"))
        assert meta["stop_reason"] in ("steady", "max_steps") and meta["steps_accepted"] >= 5 and meta["adaptive_dt"] is True
        log = np.load(os.path.join(os.path.dirname(m), "timestep_log.npz"))
        assert len(log["t"]) == meta["steps_accepted"] + meta["steps_rejected"]
