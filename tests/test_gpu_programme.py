"""Potential programmes on the GPU (gmpnp_set_electrode_potential, the electrode trace of csrc/gmpnp_trace.h):
the one-call potential against the two setters, the record kernel against gmpnp_stern_displacement, gmpnp_kinetics_currents, the node
values / NumPy means and the Python statement of the combine step, the full buffer, the status bit, every refusal of the library, hook
29, fixed-mode programmes against tests/programme_reference.py, the identity with a plain run, the driver and its quasi-steady limit.
Every handle is closed by `with` / `finally`."""
import copy
import dataclasses
import json
import math
import os

import numpy as np
import pytest

import kinetics_reference as K
import programme_reference as PR
import stern_bc_reference as SR
from conftest import random_state
from step_limit_reference import first_step_state
from test_kinetics_reference import TAFEL, _edl_k, first_step_problem, two_reactions
from test_programme_reference import P_M, steady_case, uniform_problem
from gmpnp_amd import programme as P
from gmpnp_amd.polarisation import NEWTON
from gmpnp_amd.problem import SternLayer, pore_problem
from gmpnp_amd.stern import L_STERN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def edl_k():
    return _edl_k()


def bits(a):
    return np.ascontiguousarray(a).tobytes()


# ---- gmpnp_set_electrode_potential ---------------------------------------------------------------------------------------------------------
def twin_problem(name, edl_k, pore10):
    """(problem with Stern + Tafel kinetics, start state, u_n, Newton options) of the 1 um K+ case and of L_10_R_5."""
    from gmpnp_amd.kinetics import pore_tafel
    if name == "edl1um":
        ep, mesh = edl_k
        prob = first_step_problem(ep, mesh, P_M)
        u, un = first_step_state(prob)
        return prob, u, un, dict(NEWTON), 1
    pp, mesh = copy.copy(pore10[0]), pore10[1]
    kin, pp.model = pore_tafel(pp, dict(TAFEL, i0_CO=10.0, i0_H2=1.0), -1.0, 96485.33212)
    prob, _ = pore_problem(pp, mesh, stern=SternLayer("BDM", -1.0, L_STERN / 10e-9), kinetics=kin)
    nv = mesh.num_vertices
    un = np.tile(np.r_[np.ones(8), 0.0], nv)
    sp = {"newton_solver": {"linear_solver": "band_lu", "maximum_iterations": 25, "relative_tolerance": 1e-9, "absolute_tolerance": 1e-9,
                            "relaxation_parameter": 0.9}}
    return prob, un.copy(), un, sp, 3


@pytest.mark.parametrize("name", ["edl1um", "pore10"])
def test_one_call_sets_the_potential_of_both_options(name, edl_k, pore10, gpu_lib):
    prob, u, un, sp, dim = twin_problem(name, edl_k, pore10)
    p_new = float(prob.stern.p_electrode) - 0.37
    opts = gpu_lib.newton_options(sp, dim=dim)
    with gpu_lib.DeviceSolver(prob) as a, gpu_lib.DeviceSolver(prob) as b:
        for d in (a, b):
            d.set_state(u, un)
            d.assemble(True)                                             # a Jacobian at the old potential, to be invalidated
        a.set_electrode_potential(p_new)
        b.set_stern(dataclasses.replace(prob.stern, p_electrode=p_new))
        b.set_kinetics(dataclasses.replace(prob.kinetics, p_electrode=p_new))
        with pytest.raises(gpu_lib.GmpnpError, match="no Jacobian"):
            a.jacobian_csr()
        assert a.electrode_options() == b.electrode_options() and a.electrode_options()[0]["p_electrode"] == p_new
        assert a.electrode_options()[1]["p_electrode"] == p_new
        (Fa, na), (Fb, nb) = a.assemble(True), b.assemble(True)
        assert bits(Fa) == bits(Fb) and na == nb
        assert bits(a.jacobian_csr().data) == bits(b.jacobian_csr().data)
        sa, sb = a.newton_solve(opts), b.newton_solve(opts)
        assert sa["converged"] and sa["iterations"] == sb["iterations"] >= 1
        assert bits(a.get_state()) == bits(b.get_state())
        assert bits(a.kinetics_currents()) == bits(b.kinetics_currents()) and a.stern_displacement() == b.stern_displacement()


# ---- the record kernel -----------------------------------------------------------------------------------------------------------------
def record_problem(name, pore10, kinetics=True):
    if name.startswith("uniform"):
        prob = uniform_problem(int(name[7:]), kinetics)[1]
    elif name == "pore10":
        prob, _ = pore_problem(pore10[0], pore10[1], stern=SternLayer("BDM", -1.0, L_STERN / 10e-9))
        prob.kinetics = two_reactions(list(prob.model.species), -1.0) if kinetics else None
    else:
        prob = SR.bessel_stern_case(refine=0)[0]
        prob.kinetics = two_reactions(list(prob.model.species), float(prob.stern.p_electrode)) if kinetics else None
    return prob


def states_of(prob, n, seed):
    nv, ns = prob.coords.shape[0], prob.nf - 1
    return [random_state(nv, ns, seed=seed + k)[0] for k in range(n)]


RECORD_CASES = ["uniform2", "uniform3", "uniform65", "pore10", "bessel"]
STEPS = [(0.5, 0.5), (0.75, 0.25), (2.0, 1.25), (2.0 + 1e-3, 1e-3), (7.0, 4.999)]     # (t, h) of five appends


def run_trace(dev, states, capacity=8):
    dev.electrode_trace_open(capacity)
    direct = []
    for (t, h), u in zip(STEPS, states[1:]):
        dev.set_state(u, None)
        dev.electrode_trace_append(t, h)
        direct.append((dev.stern_displacement(), dev.kinetics_currents() if dev._n_reactions else np.zeros(0)))
    return dev.electrode_trace_read(0, len(STEPS)), direct


@pytest.mark.parametrize("name", RECORD_CASES)
def test_records_against_the_direct_calls_and_the_combine_step(name, pore10, gpu_lib):
    prob = record_problem(name, pore10)
    dim, nf = prob.coords.shape[1], prob.nf
    ns = nf - 1
    nodes, w = K.boundary_weights(prob)
    if dim == 3:
        assert len(nodes) % 256 != 0 and len(nodes) > 256         # more than one pass of the workgroup, and a ragged last one
    states = states_of(prob, len(STEPS) + 1, seed=17)
    with gpu_lib.DeviceSolver(prob) as dev:
        dev.set_state(states[0], states[0])
        D0 = dev.stern_displacement()
        rec, direct = run_trace(dev, states)
        rec2, _ = run_trace(dev, states)
        dev.set_state(states[0], None)
        rec3, _ = run_trace(dev, states)
        dev.electrode_trace_close()
    assert rec.dtype == gpu_lib.ELECTRODE_RECORD_DTYPE and len(rec) == len(STEPS)
    acc = P.fresh_accumulators(D0)
    for k, ((t, h), u, (D, I)) in enumerate(zip(STEPS, states[1:], direct)):
        r = rec[k]
        assert (r["t"], r["h"], r["p_M"], r["status"]) == (t, h, float(prob.stern.p_electrode), 0)
        assert r["D"] == D and bits(r["I"][:len(I)]) == bits(I) and np.all(r["I"][len(I):] == 0.0)      # the bits of the two calls
        u2d = u.reshape(-1, nf)
        if dim == 1:
            assert r["p_boundary"] == u2d[nodes[0], ns] and bits(r["u_boundary"][:ns]) == bits(u2d[nodes[0], :ns])
        else:
            mean = (w[:, None] * u2d[nodes]).sum(axis=0) / w.sum()
            assert abs(r["p_boundary"] - mean[ns]) <= 1e-13 * abs(mean[ns])
            assert np.all(np.abs(r["u_boundary"][:ns] - mean[:ns]) <= 1e-13 * np.abs(mean[:ns]))
        assert np.all(r["u_boundary"][ns:] == 0.0)
        dD = P.electrode_record_combine(acc, h, r["D"], r["I"])     # the Python statement on the record's own D and I
        assert r["dD_dt"] == dD and bits(r["Q"]) == bits(np.array(acc["Q"])) and r["Q_D"] == acc["Q_D"]
    # a second trace of the same sequence: the first started from D_prev = D(states[-1]), the third from D(states[0]) again
    assert bits(rec3) == bits(rec)
    for key in ("D", "I", "p_boundary", "u_boundary"):
        assert bits(rec2[key]) == bits(rec[key]), key
    assert rec2["dD_dt"][0] != rec["dD_dt"][0] and bits(rec2["dD_dt"][1:]) == bits(rec["dD_dt"][1:])


@pytest.mark.parametrize("name", ["uniform3", "pore10"])
def test_kinetics_off_gives_zero_currents(name, pore10, gpu_lib):
    prob = record_problem(name, pore10, kinetics=False)
    on = record_problem(name, pore10, kinetics=True)
    states = states_of(prob, len(STEPS) + 1, seed=5)
    with gpu_lib.DeviceSolver(prob) as dev, gpu_lib.DeviceSolver(on) as dev_on:
        for d in (dev, dev_on):
            d.set_state(states[0], states[0])
        rec, _ = run_trace(dev, states)
        rec_on, _ = run_trace(dev_on, states)
    assert np.all(rec["I"] == 0.0) and np.all(rec["Q"] == 0.0) and np.all(rec["status"] == 0)
    for key in ("D", "dD_dt", "Q_D", "p_boundary", "u_boundary"):       # the kinetics change no other field of a record at a given u
        assert bits(rec[key]) == bits(rec_on[key]), key
    assert np.all(rec_on["I"][:, :2] != 0.0)


def test_a_value_that_is_not_finite_marks_its_record_only(gpu_lib):
    """A NaN in the OH value of the Stern node: OH is no reactant and does not enter eps(u) (epsc = 0), so D, I and the accumulated
    charges stay finite and the record behind it is clean again; an interior NaN is read by nothing."""
    prob = uniform_problem(9)[1]
    nf = prob.nf
    assert prob.model.epsc[1] == 0.0
    states = states_of(prob, 4, seed=2)
    bad = states[2].copy()
    bad[(prob.coords.shape[0] // 2) * nf + 1] = np.nan
    bad[int(prob.point_vertices[0]) * nf + 1] = np.nan
    with gpu_lib.DeviceSolver(prob) as dev:
        dev.set_state(states[0], states[0])
        dev.electrode_trace_open(3)
        for k, u in enumerate((states[1], bad, states[3])):
            dev.set_state(u, None)
            dev.electrode_trace_append(1.0 + k, 1.0)
        rec = dev.electrode_trace_read(0, 3)
    assert list(rec["status"]) == [0, gpu_lib.ELECTRODE_RECORD_NONFINITE, 0]
    assert np.isnan(rec["u_boundary"][1, 1]) and np.isfinite(np.delete(rec["u_boundary"][1], 1)).all()
    for key in ("D", "dD_dt", "I", "Q", "Q_D", "p_boundary"):
        assert np.isfinite(rec[key]).all(), key


def test_full_buffer_refusals_and_hook_29(pore10, edl_k, gpu_lib):
    from gmpnp_amd import dist
    from gmpnp_amd.problem import Galvanostat, edl_problem, pore_hierarchy
    from gmpnp_amd.solver import GMPNPSystem

    def refused(call, what="electrode trace"):
        with pytest.raises(gpu_lib.GmpnpError, match=what) as ei:
            call()
        assert ei.value.code == gpu_lib.ERR_INVALID

    prob = uniform_problem(9)[1]
    states = states_of(prob, 5, seed=9)
    with gpu_lib.DeviceSolver(prob) as dev:
        dev.set_state(states[0], states[0])
        for call in (lambda: dev.electrode_trace_append(1.0, 1.0), lambda: dev.electrode_trace_read(0, 1), lambda: dev.electrode_trace_close(),
                     lambda: dev.electrode_trace_open(0), lambda: dev.electrode_trace_open(-3)):
            refused(call)
        refused(lambda: dev.time_kernel(29, 1), "29")                    # no open trace
        dev.electrode_trace_open(2)
        for h in (0.0, -1.0, math.nan, math.inf):
            refused(lambda: dev.electrode_trace_append(1.0, h))
        refused(lambda: dev.electrode_trace_append(math.nan, 1.0))
        refused(lambda: dev.electrode_trace_read(0, 1))                   # nothing written yet
        for k in (1, 2):
            dev.set_state(states[k], None)
            dev.electrode_trace_append(float(k), 1.0)
        before = dev.electrode_trace_read(0, 2)
        dev.set_state(states[3], None)
        refused(lambda: dev.electrode_trace_append(3.0, 1.0))             # full: refused,
        assert bits(dev.electrode_trace_read(0, 2)) == bits(before)       # and nothing is overwritten
        refused(lambda: dev.electrode_trace_read(1, 2))
        refused(lambda: dev.electrode_trace_read(-1, 1))
        assert dev.time_kernel(29, 3) > 0.0                               # the hook writes a slot and accumulators of its own
        assert bits(dev.electrode_trace_read(0, 2)) == bits(before)
        dev.electrode_trace_open(4)                                       # the driver drains and opens again: D_prev is D of this state
        dev.set_state(states[4], None)
        dev.electrode_trace_append(4.0, 2.0)
        r = dev.electrode_trace_read(0, 1)[0]
        dev.set_state(states[3], None)
        assert r["dD_dt"] == (r["D"] - dev.stern_displacement()) / 2.0 and r["Q_D"] == 0.0 + 2.0 * r["dD_dt"]
        for p in (math.nan, math.inf):
            refused(lambda: dev.set_electrode_potential(p), "electrode potential")
        dev.set_galvanostat(Galvanostat(1.0))
        refused(lambda: dev.set_electrode_potential(-4.0), "electrode potential")
        refused(lambda: dev.electrode_trace_append(5.0, 1.0))
        refused(lambda: dev.electrode_trace_open(4))
        refused(lambda: dev.time_kernel(29, 1))
        dev.set_galvanostat(None)
        dev.set_stern(None)
        refused(lambda: dev.set_electrode_potential(-4.0), "electrode potential")
        refused(lambda: dev.electrode_trace_open(4))
        refused(lambda: dev.electrode_trace_append(5.0, 1.0))
    ep, m1 = edl_k
    with gpu_lib.DeviceSolver(edl_problem(ep, m1)) as plain:             # a handle that never had the Stern option
        refused(lambda: plain.electrode_trace_open(4))
        refused(lambda: plain.set_electrode_potential(-4.0), "electrode potential")
    pp, mesh, prob3, _ = pore10
    dom, perm, part = dist.partition_plan(prob3, 2, 0)
    with gpu_lib.DeviceSolver(dom.problem, perm=perm, partition=part) as partitioned:
        refused(lambda: partitioned.electrode_trace_open(4))
    levels = pore_hierarchy(pp, mesh, 1)
    ml = GMPNPSystem(levels[0][0], levels=levels)
    try:
        refused(lambda: ml.dev.electrode_trace_open(4))                   # a coarse level attached,
        refused(lambda: ml._coarse[0].electrode_trace_open(4))            # and the handle that serves as one
    finally:
        ml.close()


# ---- fixed-mode programmes against the NumPy system ---------------------------------------------------------------------------------------
class HandleRun:
    """What ``DeviceProgrammeOps`` reads of a driver run, over a bare problem."""

    def __init__(self, prob):
        from gmpnp_amd.solver import GMPNPSystem
        self.problem, self.stern, self.kinetics, self.budget = prob, prob.stern, prob.kinetics, None
        self.sys = GMPNPSystem(prob)


def reference_programme(kind):
    """Scaled time: the reference step of these cases is 9.5.  A pulse with two jumps, a triangle with two legs."""
    if kind == "pulse":
        return P.pulse([-5.5, -4.5, -5.25], [30.0, 20.0, 25.0], 1)
    return P.triangle(P_M, -6.0, 1.0 / 35.0, 1)


# The bound test_gpu_kinetics.py puts on a driver step against kinetics_reference.newton_loop: 1e-8 of the largest value.  Measured
# over these four cases (9 and 65 vertices, pulse and triangle, 4 steps per segment): see DESIGN.md section 5n.
REFERENCE_BOUND = 1e-8
COMPARED = ("p_boundary", "D", "dD_dt", "I", "Q", "Q_D", "u_boundary")


@pytest.mark.parametrize("kind", ["pulse", "triangle"])
@pytest.mark.parametrize("nv", [9, 65])
def test_fixed_programme_against_the_reference(nv, kind, gpu_lib):
    ep, prob, u, inv = steady_case(nv)
    segs = reference_programme(kind)
    ref = PR.NumpyProgrammeSystem(prob, u, inv)
    P.run_programme(ref, segs, steps_per_segment=4)
    want = ref.arrays()
    run = HandleRun(copy.copy(prob))
    try:
        run.sys.set_state(u, u)
        ops = P.DeviceProgrammeOps(run, dict(NEWTON), inv, capacity=5)      # smaller than the run: the trace is drained on the way
        out = P.run_programme(ops, segs, steps_per_segment=4)
        rec = ops.records()
        u_end = run.sys.dev.get_state()
    finally:
        run.sys.close()
    n = 4 * len(segs)
    assert len(rec) == n == len(want["t"]) and len(ops.chunks) >= 2
    assert np.array_equal(rec["t"], want["t"]) and np.array_equal(rec["h"], want["h"]) and np.array_equal(rec["p_M"], want["p_M"])
    assert [t for _, t, _ in ops.states] == [g[1] for g in segs] == out["breakpoints"] and np.all(rec["status"] == 0)
    ns = prob.nf - 1
    worst = {}
    for key in COMPARED:
        got = rec[key][:, :want[key].shape[1]] if rec[key].ndim == 2 else rec[key]
        worst[key] = float(np.abs(got - want[key]).max() / np.abs(want[key]).max())
    worst["u"] = float(np.abs(u_end - ref.u).max() / max(1.0, np.abs(ref.u).max()))
    print("programme %s on %d vertices against the reference: %s" % (kind, nv, {k: "%.2e" % v for k, v in worst.items()}))
    assert max(worst.values()) <= REFERENCE_BOUND, worst
    assert run.stern.p_electrode == segs[-1][3] and run.kinetics.p_electrode == segs[-1][3]


# ---- the 1D driver ---------------------------------------------------------------------------------------------------------------------
KW = dict(L_n=1e-6, cation="K", electrode_voltage=P_M, kinetics="tafel", i0_CO=TAFEL["i0_CO"], i0_H2=TAFEL["i0_H2"])


def test_a_constant_segment_is_a_plain_run(gpu_lib):
    """One constant segment in fixed mode gives the state bits of the same number of plain fixed steps of EDLRun at that inv_dt."""
    from gmpnp_amd import edl1d
    plain = edl1d.EDLRun(num_steps=4, **KW)
    try:
        plain.run(verbose=False)
        u_plain = plain.sys.dev.get_state()
    finally:
        plain.sys.close()
    run = edl1d.EDLRun(num_steps=0, **KW)
    try:
        run.run(verbose=False)
        ep = run.ep
        L_D = ep.L_D
        ops = P.DeviceProgrammeOps(run, run.solver_parameters, lambda h: 1.0 / (h * L_D))
        P.run_programme(ops, [(0.0, 4.0 * ep.dts[0], P_M, P_M)], steps_per_segment=4)
        rec = ops.records()
        u_prog = run.sys.dev.get_state()
    finally:
        run.sys.close()
    assert np.array_equal(rec["h"], [ep.dts[0]] * 4)
    assert bits(u_prog) == bits(u_plain)


PULSE_S = dict(kind="pulse", v_levels=[-5.5, -4.75], durations=[4.0e-5, 2.5e-5], cycles=2)     # seconds; time_constant is 1.05e-6 s
STEADY = dict(adaptive_dt=True, steady_tol=1e-5)


@pytest.fixture(scope="module")
def pulse_run(tmp_path_factory, gpu_lib):
    """EDLRun on the 1 um mesh to its steady stop at p_M = -5, then a pulse programme of two cycles written by write_outputs (with the
    budget log and the impedance at the state the programme ends at); and the same run without the option."""
    from gmpnp_amd import edl1d
    out_dir = tmp_path_factory.mktemp("programme")
    os.environ["GMPNP_OUT"] = str(out_dir)
    try:
        run = edl1d.EDLRun(programme=dict(PULSE_S, capacity=8, dt_init=1.0), budget=True, impedance=dict(freq_min=1.0, freq_max=1e4, per_decade=1), **STEADY, **KW)
        try:
            run.run(verbose=False)
            n_schedule = run.n
            path = run.write_outputs(stamp="pulse")
            after = dict(stern=run.stern.p_electrode, kinetics=run.kinetics.p_electrode, options=run.sys.dev.electrode_options(),
                         budget=run.budget.array(), residuals=run.programme_residuals, problem=run.problem, n_schedule=n_schedule, ep=run.ep,
                         D=run.sys.dev.stern_displacement(), u=run.sys.dev.get_state())
        finally:
            run.sys.close()
        off = edl1d.EDLRun(**STEADY, **KW)
        try:
            off.run(verbose=False)
            path_off = off.write_outputs(stamp="off")
        finally:
            off.sys.close()
    finally:
        del os.environ["GMPNP_OUT"]
    return dict(path=path, path_off=path_off, **after)


def test_driver_writes_the_programme(pulse_run):
    z = np.load(os.path.join(pulse_run["path"], "programme.npz"))
    assert sorted(z.files) == sorted(P.OUTPUT_KEYS)                                  # exactly the listed keys
    ep = pulse_run["ep"]
    segs = P.build(PULSE_S, P_M, ep.time_constant, ep.thermal_voltage)
    n = len(z["time_s"])
    meta = json.load(open(os.path.join(pulse_run["path"], "metadata.json")))
    for key in P.METADATA_KEYS:
        assert key in meta, key
    assert meta["programme_kind"] == "pulse" and meta["programme_cycles"] == 2 and meta["programme_segments"] == 4
    assert meta["programme_steps_accepted"] == n and meta["programme_stop_reason"] == "end" and meta["programme_status"] == 0
    assert np.all(z["status"] == 0)
    # the breakpoints are landed exactly, with the level of the segment that ends there
    t_scaled = z["time_s"] / ep.time_constant
    for k, g in enumerate(segs):
        last = np.nonzero(z["segment"] == k)[0][-1]
        assert z["time_s"][last] == g[1] * ep.time_constant and z["electrode_voltage"][last] == g[3]
        assert np.all(z["electrode_voltage"][z["segment"] == k] == g[3])
    assert np.all(np.diff(t_scaled) > 0.0) and z["segment"].tolist() == sorted(z["segment"].tolist())
    st = np.load(os.path.join(pulse_run["path"], "programme_states.npz"))
    assert np.array_equal(st["time_s"], [g[1] * ep.time_constant for g in segs]) and st["states"].shape == (4, len(st["coor"]), 7)
    assert bits(st["states"][-1].ravel()) == bits(pulse_run["u"])
    # the run ends at the last level, and says so
    assert pulse_run["stern"] == pulse_run["kinetics"] == -4.75 == meta["electrode_voltage"]
    assert pulse_run["options"][0]["p_electrode"] == pulse_run["options"][1]["p_electrode"] == -4.75
    assert meta["stern_displacement"] == pulse_run["D"]
    # Q_D closes on D_last - D_first within 4 ulp of max |D| per accepted step (the trace was drained on the way: capacity 8 < n)
    from gmpnp_amd.params import _load_yaml, utilities_dir
    eps_0 = _load_yaml(os.path.join(utilities_dir(), "parameters.yaml"))["nat_const"]["eps_0"]
    q = eps_0 * ep.thermal_voltage / ep.L_n
    assert n > 8
    D = z["surface_charge"] / q
    bound = 4.0 * n * float(np.spacing(np.abs(D).max()))
    print("programme: %d accepted, %d rejected, closure %.3e (bound %.3e)" % (n, meta["programme_steps_rejected"], meta["programme_charge_closure"], bound))
    assert abs(meta["programme_charge_closure"]) <= bound
    # the charging current is minus the rate of the surface charge, and the total the sum of the three
    h_s = np.diff(np.r_[0.0, z["time_s"]])
    assert np.allclose(z["i_charging"][1:], -np.diff(z["surface_charge"]) / h_s[1:], rtol=1e-6, atol=1e-9 * np.abs(z["i_charging"]).max())
    assert np.array_equal(z["i_total"], z["i_CO"] + z["i_H2"] + z["i_charging"])
    assert np.allclose(z["FE_H2"], z["i_H2"] / (z["i_CO"] + z["i_H2"]), rtol=1e-15) and z["FE_H2_cycle"].shape == (2,)
    assert np.all((z["FE_H2_cycle"] > z["FE_H2"].min()) & (z["FE_H2_cycle"] < z["FE_H2"].max()))
    assert np.all(np.diff(z["charge_CO"]) > 0.0) and np.all(np.diff(z["charge_H2"]) > 0.0)
    # behind the jump to the lower level the layer charges cathodically (section 5k's sign), behind the jump up it discharges
    first = [np.nonzero(z["segment"] == k)[0][0] for k in range(4)]
    assert z["i_charging"][first[0]] > 0.0 and z["i_charging"][first[1]] < 0.0 and z["i_charging"][first[2]] > 0.0
    # the attempts, the budget rows and the impedance at the last state
    log = np.load(os.path.join(pulse_run["path"], "timestep_log.npz"))
    assert int(log["programme_accepted"].sum()) == n and "t" in log.files and log["programme_restart"].sum() >= 4
    import budget_reference as B
    t = pulse_run["budget"]
    assert len(t) == pulse_run["n_schedule"] + n                                  # a row per accepted step of the programme too
    col = {c: k for k, c in enumerate(B.COLUMNS)}
    # the rows of the programme close as test_gpu_stern_bc._closes asks of a step: the potential row is the identity to rounding,
    # and every field's closure stays below sqrt(n_free) x the step's last Newton residual
    rows, res = t[-n:], pulse_run["residuals"]
    assert len(res) == n and np.isfinite(rows).all()
    p = rows[:, -1]
    lhs = sum(p[:, col[c]] for c in ("storage", "reaction", "wall", "exit", "point"))
    assert np.all(np.abs(lhs - (p[:, col["dirichlet"]] + p[:, col["closure"]])) <= 1e-10 * np.abs(p[:, 1:]).max(axis=1))
    ratio = np.abs(rows[:, :, col["closure"]]) / (np.sqrt(B.n_free(pulse_run["problem"]))[None, :] * res[:, None])
    print("programme rows: max |closure| / (sqrt(n_free) x residual) =", ratio.max())
    assert ratio.max() < 1.0
    assert os.path.exists(os.path.join(pulse_run["path"], "impedance.npz")) and meta["impedance_points"] == 5


def test_without_the_option_a_run_writes_what_it_wrote(pulse_run):
    files = sorted(os.listdir(pulse_run["path_off"]))
    assert files == ["arrays_scaled.npz", "arrays_unscaled.npz", "metadata.json", "timestep_log.npz"]
    assert sorted(set(os.listdir(pulse_run["path"])) - set(files)) == ["budget.npz", "impedance.npz", "programme.npz", "programme_states.npz"]
    meta = json.load(open(os.path.join(pulse_run["path_off"], "metadata.json")))
    assert not [k for k in meta if k.startswith("programme")]
    log = np.load(os.path.join(pulse_run["path_off"], "timestep_log.npz"))
    assert not [k for k in log.files if k.startswith("programme")]
    assert sorted(np.load(os.path.join(pulse_run["path_off"], "arrays_unscaled.npz")).files) == sorted(
        ["H", "OH", "HCO3", "CO32", "CO2", "cat", "p", "coor", "tau", "field_values", "i_CO", "i_H2", "FE_H2"])


def test_command_line(gpu_lib, tmp_path):
    import subprocess
    import sys
    env = dict(os.environ, GMPNP_OUT=str(tmp_path))
    cmd = [sys.executable, os.path.join(ROOT, "1D", "MPNP_CO2ER_EDL.py"), "--L_n=1e-6", "--electrode_voltage=-5", "--kinetics=tafel", "--i0_CO=0.1", "--i0_H2=0.02",
           "--num_steps=2", "--programme", "triangle", "--v_vertex=-5.5", "--scan_rate=400", "--cycles=1", "--programme_steps_per_segment=3"]
    subprocess.run(cmd, check=True, env=env, cwd=str(tmp_path), stdout=subprocess.DEVNULL)
    found = [os.path.join(d, "programme.npz") for d, _, files in os.walk(str(tmp_path)) if "programme.npz" in files]
    assert len(found) == 1
    z = np.load(found[0])
    assert len(z["time_s"]) == 6 and z["electrode_voltage"][2] == -5.5 and z["electrode_voltage"][5] == -5.0
    assert np.isclose(z["time_s"][-1], 2.0 * 0.5 * 0.025683333333333336 / 400.0, rtol=1e-12)


def test_quasi_steady_limit_on_the_device(gpu_lib):
    """The CPU test's criterion on the 1 um K+ case, against EDLRun.polarisation and the tangent's dD (its ``capacitance``): a ramp of
    -0.05 per leg in 8 fixed steps, legs of T = 200 and 10 T (scaled time); the reference alone gives (4.3e-5, 4.2e-4) and (4.9e-6,
    5.3e-5) for the currents and dD_dt / (dp/dt).  With the drivers' default Newton tolerances (1e-4) the second figure stalls at 4.5e-4:
    the solves' own error over a step of 0.006 in p_M, not a lag."""
    from gmpnp_amd import edl1d
    dv, T_leg, steps = -0.05, 200.0, 8
    run = edl1d.EDLRun(solver_parameters=dict(NEWTON), **STEADY, **KW)    # the tight Newton settings: dD_dt is a difference of two solves
    try:
        run.run(verbose=False)
        ep, dev = run.ep, run.sys.dev
        inv_dt = float(run.sys.problem.model.inv_dt)
        dev.set_time_step(0.0)                                              # from the steady stop to the steady state itself, as on the CPU
        assert dev.newton_solve(gpu_lib.newton_options(NEWTON, dim=1))["converged"]
        dev.set_time_step(inv_dt)
        u0 = dev.get_state()
        got = []
        for T in (T_leg, 10.0 * T_leg):
            run.sys.set_state(u0, u0)
            out = run.programme(kind="table", time_s=[0.0, T * ep.time_constant, 2.0 * T * ep.time_constant], electrode_voltage=[P_M, P_M + dv, P_M + 2 * dv],
                                steps_per_segment=steps)
            k = steps - 1
            assert out["electrode_voltage"][k] == P_M + dv
            dp_dt_V_per_s = dv * ep.thermal_voltage / (out["time_s"][k] - 0.0)
            got.append((out["i_CO"][k], out["i_H2"][k], -out["i_charging"][k] / dp_dt_V_per_s))     # d(surface charge)/dV [F/m2]
        run.sys.set_state(u0, u0)
        dev.set_electrode_potential(P_M)
        run.stern = dataclasses.replace(run.stern, p_electrode=P_M)
        run.kinetics = dataclasses.replace(run.kinetics, p_electrode=P_M)
        curve = run.polarisation(P_M + dv, dv)
    finally:
        run.sys.close()
    assert curve["electrode_voltage"][-1] == P_M + dv
    I_s, C_s = np.array([curve["i_CO"][-1], curve["i_H2"][-1]]), curve["capacitance"][-1]
    dev_I = [float(np.abs(np.array(g[:2]) - I_s).max() / I_s.max()) for g in got]
    dev_C = [float(abs(g[2] - C_s) / abs(C_s)) for g in got]
    print("quasi-steady on the device: currents %s, dD_dt / (dp/dt) %s" % (dev_I, dev_C))
    for a, b in (dev_I, dev_C):
        assert a > 1e-6 and b < a / 3.0


def test_an_exception_leaves_the_run_at_the_last_accepted_state(gpu_lib):
    """A Newton solve that cannot converge in fixed mode (one iteration, tolerances that are never met) is a RuntimeError naming the
    programme; afterwards the handle holds the last accepted state, no trace is open, the run's records and the handle's options
    agree on the potential, the run's own inv_dt is back, and a further programme runs."""
    from gmpnp_amd import edl1d
    run = edl1d.EDLRun(num_steps=2, **KW)
    try:
        run.run(verbose=False)
        dev = run.sys.dev
        u_before = dev.get_state()
        inv_dt = float(run.sys.problem.model.inv_dt)
        good = run.solver_parameters
        run.solver_parameters = {"newton_solver": {"maximum_iterations": 1, "relative_tolerance": 1e-30, "absolute_tolerance": 1e-30}}
        with pytest.raises(RuntimeError, match="programme"):
            run.programme(kind="pulse", v_levels=[-5.5, -4.75], durations=[4.0e-5, 2.5e-5], steps_per_segment=2)
        run.solver_parameters = good
        assert bits(dev.get_state()) == bits(u_before) == bits(dev.get_state(previous=True))   # u <- u_n: nothing was accepted
        with pytest.raises(gpu_lib.GmpnpError, match="no trace is open"):
            dev.electrode_trace_append(1.0, 1.0)
        opts = dev.electrode_options()
        assert run.stern.p_electrode == run.kinetics.p_electrode == opts[0]["p_electrode"] == opts[1]["p_electrode"] == -5.5
        assert float(run.sys.problem.model.inv_dt) == inv_dt
        out = run.programme(kind="pulse", v_levels=[-5.5, -4.75], durations=[4.0e-5, 2.5e-5], steps_per_segment=2)
        assert out["metadata"]["programme_steps_accepted"] == 4 and out["electrode_voltage"][-1] == -4.75
    finally:
        run.sys.close()
