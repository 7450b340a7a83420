"""Transient sensitivities on the GPU (gmpnp_sensitivity_open / _step / _read / _columns / _close, csrc/gmpnp_sensitivity.h; DESIGN.md
section 5p): the right-hand side against -c_k + (J(inv_dt) - J(0)) S from the device's own Jacobians and columns, the first step from
S = 0 against gmpnp_electrode_tangent (bit for bit, both chain widths and ten columns), fixed-mode programmes against
tests/sensitivity_reference.py, column independence and repeatability, the twin handle that never opens the buffer, a planted
rejection against its accepted sequence replayed, the full buffer, the status bit, every refusal, hook 31 and the 1D driver.  Every
handle is closed by `with` / `finally`."""
import copy
import json
import math
import os

import numpy as np
import pytest

import response_reference as R
import sensitivity_reference as S
from conftest import random_state
from step_limit_reference import first_step_state
from test_gpu_kinetics import edl_k  # noqa: F401 (fixture)
from test_gpu_programme import KW, HandleRun, bits, reference_programme
from test_gpu_response import generated_problem
from test_gpu_tangent import PARAMS, four_reactions
from test_kinetics_reference import first_step_problem
from test_programme_reference import P_M, steady_case
from gmpnp_amd import programme as P
from gmpnp_amd.polarisation import NEWTON
from gmpnp_amd.problem import SternLayer, edl_problem
from gmpnp_amd.stern import L_STERN

pytestmark = pytest.mark.gpu
NEWTON_KW = dict(NEWTON["newton_solver"])
REFERENCE_BOUND = 1e-8     # test_gpu_programme.py's bound against its reference
FIELDS = ("dD", "d_dD_dt", "dI", "dQ", "dQ_D", "dp_boundary")


def rhs_case(name, edl_k):
    if name == "edl1":
        prob = first_step_problem(edl_k[0], edl_k[1], P_M)
        u, un = first_step_state(prob)
        return prob, u + 1e-3 * random_state(prob.coords.shape[0], 6, seed=3)[0], un
    nv = int(name[7:])
    return generated_problem(nv), random_state(nv, 6, seed=nv)[0], random_state(nv, 6, seed=100 + nv)[0]


# ---- the right-hand side -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["uniform2", "uniform3", "uniform65", "edl1"])
def test_right_hand_side(name, edl_k, gpu_lib):
    """End rows with one neighbour (2 vertices), the smallest mesh with an interior row (3), more than one workgroup (65) and the
    graded 1 um mesh; a random S; both chains' storage (six columns, then two)."""
    prob, u, un = rhs_case(name, edl_k)
    inv_dt = float(prob.model.inv_dt)
    assert inv_dt > 0.0
    Sr = np.random.default_rng(11).standard_normal((len(PARAMS), prob.ndof))
    with gpu_lib.DeviceSolver(prob) as dev, gpu_lib.DeviceSolver(R.with_inv_dt(prob, 0.0)) as steady:
        steady.set_state(u, un)
        steady.assemble(True)
        J0 = steady.jacobian_csr()
        dev.set_state(u, un)
        worst = 0.0
        for cols in (slice(0, 6), slice(4, 6)):
            params = PARAMS[cols]
            dev.sensitivity_open(params, "zero", 2)
            dev.sensitivity_set_columns(Sr[cols])
            dev.sensitivity_step(1.0, 1.0)
            rhs = dev.sensitivity_columns(1)
            J1 = dev.jacobian_csr()                       # the step leaves the Jacobian of the current u
            dev.electrode_tangent(params)
            c = dev.tangent_columns(len(params))
            want = -c + ((J1 - J0) @ Sr[cols].T).T
            dev_ = float(np.abs(rhs - want).max() / np.abs(want).max())
            worst = max(worst, dev_)
            assert np.abs(want).max() > 0.0 and dev_ <= 1e-12, (name, dev_)
            dev.sensitivity_close()
    print("sensitivity right-hand side on %s: %.2e of the largest entry" % (name, worst))


# ---- the first step from S = 0 is the tangent ----------------------------------------------------------------------------------------------
def identity_check(dev, params, nr):
    dev.sensitivity_open(params, "zero", 1)
    dev.sensitivity_step(0.5, 0.25)
    Sd, rec = dev.sensitivity_columns(0), dev.sensitivity_read(0, 1)[0]
    t = dev.electrode_tangent(params, want_z=True)
    assert not rec["status"].any() and not t["status"].any()
    assert list(rec["param"]) == list(params)
    assert bits(Sd) == bits(t["z"])
    assert bits(rec["dD"]) == bits(t["dD"]) and bits(rec["dI"][:, :nr]) == bits(t["dI"]) and bits(rec["dp_boundary"]) == bits(t["dp_boundary"])
    assert bits(rec["residual"]) == bits(t["residual"]) and np.all(rec["dI"][:, nr:] == 0.0)
    dev.sensitivity_close()


@pytest.mark.parametrize("n", [1, 2, 3, 6])
def test_first_step_from_zero_is_the_tangent(n, gpu_lib):
    prob = generated_problem(65)
    u, un = random_state(65, 6, seed=65)[0], random_state(65, 6, seed=165)[0]
    with gpu_lib.DeviceSolver(prob) as dev:
        dev.set_state(u, un)
        identity_check(dev, PARAMS[:n], 2)


def test_first_step_with_ten_columns(gpu_lib):
    from gmpnp_amd.params import edl_parameters
    import hp_reference as H
    ep = edl_parameters(cation="Cs", voltage_multiplier=-10.0)
    prob = edl_problem(ep, H.uniform_mesh_1d(65), stern=SternLayer("BDM", P_M, L_STERN / ep.L_n), kinetics=four_reactions(ep.species, P_M))
    u, un = random_state(65, 6, seed=65)[0], random_state(65, 6, seed=165)[0]
    with gpu_lib.DeviceSolver(prob) as dev:
        dev.set_state(u, un)
        identity_check(dev, (0, 16, 17, 18, 19, 32, 33, 34, 35, 48), 4)


# ---- fixed-mode programmes against the NumPy recursion -------------------------------------------------------------------------------------
def device_march(prob, u, inv, segs, params, start, capacity=5, sensitivities=True, **kw):
    """(ops, electrode records, sensitivity records, final S, final u) of a programme on a fresh handle."""
    run = HandleRun(copy.copy(prob))
    try:
        run.sys.set_state(u, u)
        if sensitivities and start == "steady":
            run.sys.set_time_step(0.0)
            assert not run.sys.dev.electrode_tangent(params)["status"].any()
        ops = P.DeviceProgrammeOps(run, dict(NEWTON), inv, capacity=capacity, sensitivities=params if sensitivities else None,
                                   sensitivity_start=start)
        out = P.run_programme(ops, segs, **kw)
        srec = Sd = None
        if sensitivities:
            srec = ops.sensitivity_records()
            Sd = run.sys.dev.sensitivity_columns(0)
            run.sys.dev.sensitivity_close()
        rec = ops.records()
        return ops, out, rec, srec, Sd, run.sys.dev.get_state()
    finally:
        run.sys.close()


@pytest.mark.parametrize("start", ["steady", "zero"])
@pytest.mark.parametrize("kind", ["pulse", "triangle"])
@pytest.mark.parametrize("nv", [9, 65])
def test_fixed_programme_against_the_reference_recursion(nv, kind, start, gpu_lib):
    ep, prob, u, inv = steady_case(nv)
    segs = reference_programme(kind)
    ref = S.NumpySensitivitySystem(prob, u, inv, PARAMS, start=start, newton=NEWTON_KW)
    P.run_programme(ref, segs, steps_per_segment=4)
    want = ref.sensitivity_arrays()
    ops, _, rec, srec, Sd, _ = device_march(prob, u, inv, segs, PARAMS, start, steps_per_segment=4)
    n = 4 * len(segs)
    assert srec.shape == (n, len(PARAMS)) and len(ops.sensitivity_chunks) >= 2 and len(rec) == n      # drained on the way (capacity 5)
    assert np.array_equal(srec["t"], want["t"]) and np.array_equal(srec["h"], want["h"]) and not srec["status"].any()
    assert np.all(srec["param"] == np.array(PARAMS)[None, :])
    # Per column, relative to the largest reference value of that quantity.  The bound is REFERENCE_BOUND for every field but the
    # difference quotient d_dD_dt = (dD - dD_prev) / h.  The states of the two marches agree to 1e-13 (test_gpu_programme.py), and S to
    # 1e-11 of max |S|; but dD and dp_boundary read the boundary entries of S, which are small beside max |S|, so the rounding of the
    # two linear solvers (cyclic reduction, sparse LU) times the condition of J shows there: up to 3e-9 of max |dD|, inside the bound.
    # Two values of dD that each differ by up to the bound times max |dD| give a quotient that differs by up to 2 bound max |dD| / h:
    # d_dD_dt is held to that, in absolute form and with every step's own h.  (A bound relative to max |d_dD_dt| would say little:
    # the offset column from the steady start has a dD that barely moves, so its d_dD_dt is close to zero throughout.)
    worst, quotient = {}, 0.0
    for k in range(len(PARAMS)):
        for key in FIELDS:
            got = srec[key][:, k, :want[key].shape[2]] if srec[key].ndim == 3 else srec[key][:, k]
            w = want[key][:, k]
            worst[key] = max(worst.get(key, 0.0), float(np.abs(got - w).max() / np.abs(w).max()))
        worst["S"] = max(worst.get("S", 0.0), float(np.abs(Sd[k] - ref.S[k]).max() / np.abs(ref.S[k]).max()))
        # the absolute form, step by step: |delta d_dD_dt| <= 2 bound max |dD| / h
        room = 2.0 * REFERENCE_BOUND * np.abs(want["dD"][:, k]).max() / want["h"][:, k]
        quotient = max(quotient, float((np.abs(srec["d_dD_dt"][:, k] - want["d_dD_dt"][:, k]) / room).max()))
    print("sensitivities of the %s on %d vertices from %s against the reference: %s (d_dD_dt uses %.2f of its absolute bound), residual %.2e"
          % (kind, nv, start, {k: "%.2e" % v for k, v in worst.items()}, quotient, srec["residual"].max()))
    assert max(v for k, v in worst.items() if k != "d_dD_dt") <= REFERENCE_BOUND, worst
    assert quotient <= 1.0, (quotient, worst)


# ---- column independence, repeatability, the handle untouched ------------------------------------------------------------------------------
def test_columns_do_not_depend_on_each_other_and_runs_repeat(gpu_lib):
    ep, prob, u, inv = steady_case(9)
    segs = reference_programme("pulse")
    kw = dict(steps_per_segment=2)
    _, _, _, six, S6, _ = device_march(prob, u, inv, segs, PARAMS, "steady", **kw)
    _, _, _, again, S6b, _ = device_march(prob, u, inv, segs, PARAMS, "steady", **kw)
    assert bits(six) == bits(again) and bits(S6) == bits(S6b)
    for params in ((48, 16), (33,), (32, 0, 17)):            # a chain of 2 in another order, one column, a chain of 8 with three
        _, _, _, part, Sp, _ = device_march(prob, u, inv, segs, params, "steady", **kw)
        for j, q in enumerate(params):
            k = PARAMS.index(q)
            assert bits(np.ascontiguousarray(part[:, j])) == bits(np.ascontiguousarray(six[:, k])), (params, q)
            assert bits(Sp[j]) == bits(S6[k]), (params, q)


def test_a_twin_that_never_opens_the_buffer_has_the_same_bits(gpu_lib):
    ep, prob, u, inv = steady_case(65)
    segs = P.triangle(P_M, -6.0, 1.0 / 35.0, 1)
    a = device_march(prob, u, inv, segs, PARAMS, "steady", steps_per_segment=5)
    b = device_march(prob, u, inv, segs, PARAMS, "steady", sensitivities=False, steps_per_segment=5)
    assert len(a[2]) == 10 and bits(a[2]) == bits(b[2])                   # the electrode-trace records
    assert bits(a[5]) == bits(b[5])                                      # the state
    assert a[0].residuals == b[0].residuals and a[0].newton_iterations == b[0].newton_iterations      # the Newton solves on the way
    assert [bits(v) for _, _, v in a[0].states] == [bits(v) for _, _, v in b[0].states]


# ---- rejected attempts ---------------------------------------------------------------------------------------------------------------------
class FailingOps(P.DeviceProgrammeOps):
    """``DeviceProgrammeOps`` whose Newton solve number ``fail`` (counted over all solves) is made to fail."""

    def __init__(self, *a, fail=(), **kw):
        super().__init__(*a, **kw)
        self.fail, self.solves = set(fail), 0

    def solve(self):
        k, self.solves = self.solves, self.solves + 1
        return (False, 0) if k in self.fail else super().solve()


def test_a_rejected_attempt_never_touches_the_sensitivities(gpu_lib):
    from gmpnp_amd.timestep import TimeStepPolicy
    ep, prob, u, inv = steady_case(9)
    segs = P.pulse([-5.5, -4.5], [30.0, 20.0], 1)
    run = HandleRun(copy.copy(prob))
    try:
        run.sys.set_state(u, u)
        ops = FailingOps(run, dict(NEWTON), inv, capacity=64, sensitivities=PARAMS, sensitivity_start="zero", fail=(2,))
        out = P.run_programme(ops, segs, TimeStepPolicy(), dt_init=1.5)
        srec, Sd = ops.sensitivity_records(), run.sys.dev.sensitivity_columns(0)
    finally:
        run.sys.close()
    log = out["log"]
    assert sum(not r["accepted"] for r in log) >= 1 and len(srec) == sum(r["accepted"] for r in log)
    run = HandleRun(copy.copy(prob))
    try:                                                     # the accepted sequence replayed in fixed steps of those sizes
        run.sys.set_state(u, u)
        ops2 = P.DeviceProgrammeOps(run, dict(NEWTON), inv, capacity=64, sensitivities=PARAMS, sensitivity_start="zero")
        for r, t_end in zip([r for r in log if r["accepted"]], out["times"]):
            ops2.set_potential(r["potential"])
            ops2.set_step(r["h"])
            assert ops2.solve()[0]
            ops2.record(t_end, r["h"], r["segment"], r["potential"])
            ops2.accept()
        srec2, Sd2 = ops2.sensitivity_records(), run.sys.dev.sensitivity_columns(0)
    finally:
        run.sys.close()
    assert bits(srec) == bits(srec2) and bits(Sd) == bits(Sd2) and not srec["status"].any()


# ---- robustness ----------------------------------------------------------------------------------------------------------------------------
def test_full_buffer_status_bit_refusals_and_hook_31(pore10, edl_k, gpu_lib):
    from gmpnp_amd.problem import Galvanostat

    def refused(call, what="sensitivities"):
        with pytest.raises(gpu_lib.GmpnpError, match=what) as ei:
            call()
        assert ei.value.code == gpu_lib.ERR_INVALID

    prob = generated_problem(9)
    u, un = random_state(9, 6, seed=9)[0], random_state(9, 6, seed=109)[0]
    params = (16, 48, 0)
    with gpu_lib.DeviceSolver(prob) as dev:
        dev.set_state(u, un)
        for call in (lambda: dev.sensitivity_step(1.0, 1.0), lambda: dev.sensitivity_read(0, 1), lambda: dev.sensitivity_columns(0),
                     lambda: dev.sensitivity_close(), lambda: dev.sensitivity_open(params, "zero", 0), lambda: dev.sensitivity_open((), "zero", 2),
                     lambda: dev.sensitivity_open(tuple(range(16, 20)) + tuple(range(32, 36)) + (0, 48, 1), "zero", 2),
                     lambda: dev.sensitivity_open((16, 16), "zero", 2), lambda: dev.sensitivity_open((5,), "zero", 2),
                     lambda: dev.sensitivity_open((18,), "zero", 2),                       # a reaction the kinetics do not hold
                     lambda: dev.sensitivity_open(params, 3, 2), lambda: dev.sensitivity_open(params, "continue", 2),
                     lambda: dev.sensitivity_open(params, "steady", 2)):                   # no tangent
            refused(call)
        refused(lambda: dev.time_kernel(31, 1), "31")
        dev.electrode_tangent((0, 16))
        refused(lambda: dev.sensitivity_open(params, "steady", 2))                         # the tangent lacks a parameter
        dev.electrode_tangent(params)
        dev.set_state(u, un)
        refused(lambda: dev.sensitivity_open(params, "steady", 2))                         # stale
        dev.sensitivity_open(params, "zero", 2)
        for h in (0.0, -1.0, math.nan, math.inf):
            refused(lambda: dev.sensitivity_step(1.0, h))
        refused(lambda: dev.sensitivity_step(math.nan, 1.0))
        refused(lambda: dev.sensitivity_read(0, 1))                                        # nothing written yet
        refused(lambda: dev.sensitivity_columns(1))
        refused(lambda: dev.sensitivity_columns(2))
        dev.sensitivity_step(1.0, 1.0)
        # a NaN planted in one column marks that column's record only
        Sd = dev.sensitivity_columns(0)
        bad = Sd.copy()
        bad[1, 3 * prob.nf + 2] = np.nan
        dev.sensitivity_set_columns(bad)
        dev.sensitivity_step(2.0, 1.0)
        before = dev.sensitivity_read(0, 2)
        assert list(before["status"][0]) == [0, 0, 0] and list(before["status"][1]) == [0, gpu_lib.SENSITIVITY_NONFINITE, 0]
        for key in FIELDS:
            assert np.isfinite(before[key][:, [0, 2]]).all(), key
        refused(lambda: dev.sensitivity_step(3.0, 1.0))                                    # full: refused,
        assert bits(dev.sensitivity_read(0, 2)) == bits(before)                            # and nothing is overwritten
        refused(lambda: dev.sensitivity_read(1, 2))
        refused(lambda: dev.sensitivity_read(-1, 1))
        S_before = dev.sensitivity_columns(0)
        assert dev.time_kernel(31, 3) > 0.0                                                # the hook works on storage of its own
        assert bits(dev.sensitivity_read(0, 2)) == bits(before) and bits(dev.sensitivity_columns(0)) == bits(S_before)
        dev.sensitivity_set_columns(Sd)
        dev.sensitivity_open(params, "continue", 3)                                        # the driver reads and goes on: S and the sums stay
        assert bits(dev.sensitivity_columns(0)) == bits(Sd)
        dev.sensitivity_step(3.0, 1.0)
        r = dev.sensitivity_read(0, 1)[0]
        assert r["dQ_D"][0] == before["dQ_D"][1, 0] + 1.0 * r["d_dD_dt"][0] and r["d_dD_dt"][0] == (r["dD"][0] - before["dD"][1, 0]) / 1.0
        refused(lambda: dev.sensitivity_open((16, 48), "continue", 3))                     # other columns than the open before
        dev.set_galvanostat(Galvanostat(1.0))
        refused(lambda: dev.sensitivity_step(4.0, 1.0))
        refused(lambda: dev.sensitivity_open(params, "zero", 2))
        refused(lambda: dev.time_kernel(31, 1))
        dev.set_galvanostat(None)
        dev.sensitivity_close()
        refused(lambda: dev.sensitivity_step(4.0, 1.0))
        dev.set_stern(None)
        refused(lambda: dev.sensitivity_open(params, "zero", 2))
    with gpu_lib.DeviceSolver(edl_problem(edl_k[0], edl_k[1])) as plain:                   # a handle that never had the Stern option
        refused(lambda: plain.sensitivity_open((0,), "zero", 2))
    from gmpnp_amd.problem import pore_problem
    prob3, _ = pore_problem(pore10[0], pore10[1], stern=SternLayer("BDM", -1.0, L_STERN / 10e-9))
    with gpu_lib.DeviceSolver(prob3) as pore:                                              # 3D handles
        refused(lambda: pore.sensitivity_open((0,), "zero", 2))


# ---- the 1D driver -------------------------------------------------------------------------------------------------------------------------
PULSE_S = dict(kind="pulse", v_levels=[-5.5, -4.75], durations=[4.0e-5, 2.5e-5], cycles=2, steps_per_segment=6, capacity=8)
NAMES = ("i0_CO", "i0_H2", "alpha_CO", "stern_length", "offset")
STEADY = dict(adaptive_dt=True, steady_tol=1e-5)
EPS = 3.2e-2          # the smaller eps of the pair tests/test_sensitivity_reference.py establishes on the reference
MARGIN = 2.0e-2       # ... and the deviation it allows there (the reference's worst is 1.4e-2)


def driver_run(out_dir, stamp, programme, **kw):
    from gmpnp_amd import edl1d
    os.environ["GMPNP_OUT"] = str(out_dir)
    try:
        run = edl1d.EDLRun(programme=programme, **STEADY, **dict(KW, **kw))
        try:
            run.run(verbose=False)
            return run.write_outputs(stamp=stamp)
        finally:
            run.sys.close()
    finally:
        del os.environ["GMPNP_OUT"]


def test_driver_writes_the_sensitivities(tmp_path, gpu_lib):
    on = driver_run(tmp_path, "on", dict(PULSE_S, sensitivities=NAMES))
    off = driver_run(tmp_path, "off", dict(PULSE_S))
    z = np.load(os.path.join(on, "programme_sensitivity.npz"))
    assert sorted(z.files) == sorted(P.SENSITIVITY_KEYS + ("time_s", "parameters", "status"))
    assert list(z["parameters"]) == list(NAMES) and not z["status"].any() and z["d_i_CO"].shape == (24, len(NAMES))
    assert not os.path.exists(os.path.join(off, "programme_sensitivity.npz"))
    meta_on, meta_off = (json.load(open(os.path.join(p, "metadata.json"))) for p in (on, off))
    for key in P.SENSITIVITY_METADATA_KEYS:
        assert key in meta_on and key not in meta_off, key
    assert meta_on["programme_sensitivity_start"] == "steady" and meta_on["programme_sensitivity_status"] == 0
    assert set(meta_on) - set(P.SENSITIVITY_METADATA_KEYS) == set(meta_off)
    for key in P.METADATA_KEYS:                              # the programme's own keys are what they are without the option
        assert meta_on[key] == meta_off[key], key
    assert sorted(os.listdir(on)) == sorted(os.listdir(off) + ["programme_sensitivity.npz"])
    for name in ("programme.npz", "programme_states.npz"):
        a, b = np.load(os.path.join(on, name)), np.load(os.path.join(off, name))
        assert sorted(a.files) == sorted(b.files)
        for key in a.files:
            assert bits(a[key]) == bits(b[key]), (name, key)
    # d i_CO / d ln i0_CO against the central difference of two driver runs
    i0 = KW["i0_CO"]
    runs = [np.load(os.path.join(driver_run(tmp_path, "e%d" % s, dict(PULSE_S), i0_CO=i0 * math.exp(s * EPS)), "programme.npz")) for s in (+1, -1)]
    assert np.array_equal(runs[0]["time_s"], z["time_s"])
    fd = (runs[0]["i_CO"] - runs[1]["i_CO"]) / (2.0 * EPS)
    got = z["d_i_CO"][:, 0]
    dev_ = float(np.abs(got - fd).max() / np.abs(fd).max())
    print("driver: d i_CO / d ln i0_CO against the difference of two runs at eps %.1e: %.2e (margin %.1e)" % (EPS, dev_, MARGIN))
    assert dev_ <= MARGIN


# ---- the fit to transients -----------------------------------------------------------------------------------------------------------------
RECOVERY_BOUND = 1e-9       # measured on the reference alone (tests/test_sensitivity_reference.py): the steady fit's bound, reused


class FitRun(HandleRun):
    """``HandleRun`` with what ``fit.DeviceTransient`` reads of a driver run beside it."""
    step_fraction = 0.0


def test_device_round_trip_fit_of_four_parameters(gpu_lib):
    """65 vertices, a pulse with two jumps in fixed mode, data synthesised on the device at the truth (every step), the start displaced
    by ``fit_reference.DISPLACEMENT``: the four kinetic parameters from the currents alone."""
    import time
    import fit_reference as FR
    from gmpnp_amd import fit as ft
    ep, prob, u, inv = steady_case(65)
    names = FR.FOUR
    codes = ft.param_codes(names)
    segs = reference_programme("pulse")
    _, _, rec, _, _, _ = device_march(prob, u, inv, segs, PARAMS, "steady", capacity=64, sensitivities=False, steps_per_segment=4)
    tc = 2.0e-6
    table = ft.check_programme_data({"time_s": rec["t"] * tc, "i_CO": rec["I"][:, 0].copy(), "i_H2": rec["I"][:, 1].copy()}, len(codes))
    start = FR.moved(prob, codes, [FR.DISPLACEMENT[n] for n in names])
    run = FitRun(copy.copy(start))
    try:
        run.sys.set_state(u, u)
        system = ft.DeviceTransient(run, segs, 4, codes, 1.0, inv, tc, capacity=5)          # drained on the way
        curve = ft.TransientCurve(system, table, len(codes))
        theta0 = ft.theta_of(system.kept["stern"], system.kept["kinetics"], codes)
        t0 = time.perf_counter()
        res = ft.LevenbergMarquardt(curve, [ft.is_log(c) for c in codes]).run(theta0)
        wall = time.perf_counter() - t0
        kept = ft.theta_of(system.kept["stern"], system.kept["kinetics"], codes)
        u_kept = system.kept["u"].copy()
        # a trial that is not accepted leaves nothing behind: the same trial twice from the kept start has equal bits
        a = curve.trial(None, np.array([0.2, -0.1, 0.03, -0.02]))
        b = curve.trial(None, np.array([0.2, -0.1, 0.03, -0.02]))
        assert a is not None and bits(a["r"]) == bits(b["r"]) and bits(a["J"]) == bits(b["J"])
        assert bits(system.kept["u"]) == bits(u_kept) and np.array_equal(ft.theta_of(system.kept["stern"], system.kept["kinetics"], codes), kept)
        system.finish(inv(9.5))
        assert bits(run.sys.dev.get_state()) == bits(u_kept)
        back = ft.theta_of(*run.sys.dev.electrode_options(), codes)
        assert np.array_equal(back, kept)
    finally:
        run.sys.close()
    truth = FR.theta_of(prob, codes)
    err = float(np.abs(kept - truth).max())
    print("device transient fit: %s, %d trials, %d rejected, %d Newton iterations, %.2f s, |theta - truth| %.2e, condition %.3g"
          % (res["stop_reason"], res["trials"], res["rejected_trials"], res["newton_iterations"], wall, err, res["condition_number"]))
    assert np.allclose(theta0, FR.theta_of(start, codes), rtol=1e-15) and np.abs(theta0 - truth).max() > 0.05
    assert res["stop_reason"] == "converged"
    assert err <= RECOVERY_BOUND


def test_driver_fits_a_programme(tmp_path, gpu_lib):
    """The driver: data written by a programme run, then a run from a displaced i0_CO with ``fit_programme``: ``fit_programme.npz`` holds
    ``fit.npz``'s tables over time_s, the programme is marched with the fitted parameters afterwards, and a data time that is no
    step end is refused by name before a trial runs."""
    from gmpnp_amd import edl1d
    fixed = {k: v for k, v in PULSE_S.items()}
    data_dir = driver_run(tmp_path, "data", dict(fixed))
    data = os.path.join(data_dir, "programme.npz")
    out = driver_run(tmp_path, "fit", dict(fixed), i0_CO=KW["i0_CO"] * math.exp(0.3), fit_programme=dict(data=data, params=("i0_CO", "alpha_CO")))
    z = np.load(os.path.join(out, "fit_programme.npz"))
    for key in ("names", "codes", "initial_values", "fitted_values", "standard_errors", "covariance", "residuals", "history_cost", "time_s",
                "data_i_CO", "model_i_CO", "data_i_H2", "data_surface_charge"):
        assert key in z.files, key
    assert "electrode_voltage" not in z.files and list(z["names"]) == ["i0_CO", "alpha_CO"] and len(z["time_s"]) == 24
    meta = json.load(open(os.path.join(out, "metadata.json")))
    assert meta["fit_programme_parameters"] == ["i0_CO", "alpha_CO"] and meta["fit_programme_stop_reason"] in ("converged", "stalled")
    assert "fit_parameters" not in meta and meta["fit_programme_trials"] >= 2
    print("driver fit_programme: %s, %d trials, i0_CO %.6g -> %.6g (data %.6g), alpha_CO -> %.6g"
          % (meta["fit_programme_stop_reason"], meta["fit_programme_trials"], z["initial_values"][0], z["fitted_values"][0], KW["i0_CO"], z["fitted_values"][1]))
    # the data come from a run at the driver's Newton tolerance (1e-4) and the displacement is 0.3 in ln i0: the cost can fall by about
    # (1e-4 / 0.3)^2 = 1e-7; 1e-4 is asked
    assert z["history_cost"][-1] < 1e-4 * z["history_cost"][0]
    assert abs(z["fitted_values"][0] - KW["i0_CO"]) < 0.01 * KW["i0_CO"] < abs(z["initial_values"][0] - KW["i0_CO"])
    p = np.load(os.path.join(out, "programme.npz"))                                  # marched afterwards, with the fitted parameters
    assert np.array_equal(p["time_s"], z["time_s"]) and np.allclose(p["i_CO"], z["data_i_CO"], rtol=1e-2)
    shifted = dict(np.load(data))
    shifted["time_s"] = shifted["time_s"].copy()
    shifted["time_s"][3] *= 1.0 + 1e-6
    np.savez(tmp_path / "shifted.npz", **shifted)
    os.environ["GMPNP_OUT"] = str(tmp_path)
    try:
        run = edl1d.EDLRun(programme=dict(fixed), fit_programme=dict(data=str(tmp_path / "shifted.npz")), **STEADY, **KW)
        try:
            run.run(verbose=False)
            with pytest.raises(ValueError, match="%.17g" % shifted["time_s"][3]):
                run.fit_programme(**run.fit_programme_par)
        finally:
            run.sys.close()
    finally:
        del os.environ["GMPNP_OUT"]
