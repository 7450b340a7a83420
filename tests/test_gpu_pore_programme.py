"""Potential programmes in the 3D pore on the device: the wall profile (``gmpnp_wall_profile_*``, k_wall_profile)
against the electrode record of the same step (bits), against the NumPy rule on the device's own u and against itself (bits across
profiles and numbers of bins), its status word, its refusals and hook 32; a handle that never opens it; fixed-mode programmes against
the NumPy system of tests/pore_programme_reference.py; the driver (``PoreRun.pore_programme``) and the command line.

Shapes: generated cylinders ``coarse`` = (rings, layers) — (1, 1): 14 vertices, every wall node on a rim, two layers; (1, 2): 21, three
layers; (2, 3): 76; (3, 6): 259, seven layers, so that 2, 3 and 7 uniform bins have edges ON node layers (1/2; 1/3 and 2/3) and between
them — and L_10_R_5 once (more wall nodes than a workgroup has lanes: a lane adds several entries).  Random admissible states, Stern
BDM, two reactions, five appends with the state changed in between."""
import copy
import json
import math
import os

import numpy as np
import pytest

import pore_programme_reference as PPR
import pore_response_reference as PP
from conftest import random_state
from gmpnp_amd import programme as P
from gmpnp_amd.polarisation import NEWTON
from gmpnp_amd.problem import Galvanostat, SternLayer
from gmpnp_amd.stern import L_STERN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(float).eps
CYLINDERS = {"c1x1": (1, 1), "c1x2": (1, 2), "c2x3": (2, 3), "c3x6": (3, 6)}
P_M = -1.0
HS = (0.5, 0.25, 1.0, 2.0, 0.125)          # the step lengths of the five appends
COMPARED_BITS = ("area", "D", "I", "Q", "p_mean", "u_mean", "count", "status")


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def problem_of(name, pore10):
    if name != "pore10":
        return PP.cylinder_case(CYLINDERS[name], p_M=P_M)
    from test_kinetics_reference import two_reactions
    from gmpnp_amd.problem import pore_problem
    pp, mesh = pore10[0], pore10[1]
    prob, _ = pore_problem(pp, mesh, stern=SternLayer("BDM", P_M, L_STERN / pp.L))
    prob = copy.copy(prob)
    prob.kinetics = two_reactions(list(prob.model.species), P_M)
    return prob


def states_of(prob, n=5, seed=20):
    return [random_state(prob.coords.shape[0], prob.nf - 1, seed=seed + k)[0] for k in range(n)]


def appended(dev, edges, states, capacity=5, trace=True):
    """Five appends to the trace and to the profile with the state changed in between: (trace records, profile records (5, bins))."""
    dev.set_state(states[0], states[0])
    if trace:
        dev.electrode_trace_open(capacity)
    dev.wall_profile_open(edges, capacity)
    t = 0.0
    for u, h in zip(states, HS):
        dev.set_state(u, None)
        t += h
        if trace:
            dev.electrode_trace_append(t, h)
        dev.wall_profile_append(t, h)
    rec = dev.electrode_trace_read(0, len(states)) if trace else None
    return rec, dev.wall_profile_read(0, len(states))


_RUNS = {}


def runs(name, gpu_lib, pore10):
    """Everything one shape needs from the device, computed once: one bin over the wall beside the trace, 2 / 3 / 7 bins where every bin
    holds a node, a second profile of the same sequence, and the NumPy profiles on the same states."""
    if name in _RUNS:
        return _RUNS[name]
    prob = problem_of(name, pore10)
    states = states_of(prob)
    _, _, z = PPR.wall_nodes_z(prob)
    lo, hi = float(z.min()), float(z.max())
    layers = len(np.unique(z))
    counts = [nb for nb in (2, 3, 7) if name != "pore10" and all(len(m) for m in P.wall_bin_lists(z, P.uniform_edges(lo, hi, nb)))]
    if name == "pore10":
        counts = [3]
    out = dict(prob=prob, states=states, z=z, lo=lo, hi=hi, layers=layers, counts=counts, dev={}, ref={})
    with gpu_lib.DeviceSolver(prob) as dev:
        out["trace"], out["one"] = appended(dev, [lo, hi], states)
        for nb in counts:
            edges = P.uniform_edges(lo, hi, nb)
            out["dev"][nb] = appended(dev, edges, states, trace=False)[1]
            out["ref"][nb] = [PPR.profile(prob, u, edges) for u in (states if name != "pore10" else states[:1])]
        out["again"] = appended(dev, [lo, hi], states)[1]
    _RUNS[name] = out
    return out


SHAPES = list(CYLINDERS) + ["pore10"]


# ---- the kernel ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPES)
def test_one_bin_over_the_wall_is_the_electrode_record(name, gpu_lib, pore10):
    """D and I are the bits of the same step's gmpnp_electrode_record_t (the means and the charges too: the same statements in the same
    order); a second profile of the same sequence has equal bits."""
    d = runs(name, gpu_lib, pore10)
    rec, one = d["trace"], d["one"]
    assert one.shape == (5, 1) and np.all(one["status"] == 0) and np.all(rec["status"] == 0)
    if name == "pore10":
        assert one["count"][0, 0] > 256
    assert bits(one["D"][:, 0]) == bits(rec["D"]) and bits(one["I"][:, 0]) == bits(rec["I"])
    assert bits(one["Q"][:, 0]) == bits(rec["Q"]) and bits(one["p_mean"][:, 0]) == bits(rec["p_boundary"])
    assert bits(one["u_mean"][:, 0]) == bits(rec["u_boundary"])
    assert np.array_equal(one["t"][:, 0], rec["t"]) and np.array_equal(one["h"][:, 0], HS)
    assert np.all(one["z_lo"] == d["lo"]) and np.all(one["z_hi"] == d["hi"]) and np.all(one["count"] == len(d["z"]))
    assert bits(d["again"]) == bits(one)
    assert np.any(one["I"][:, 0, :2] != 0.0) and not np.any(one["I"][:, 0, 2:])


@pytest.mark.parametrize("name", SHAPES)
def test_bins_against_the_numpy_rule_on_the_devices_own_state(name, gpu_lib, pore10):
    """Each bin agrees with the NumPy rule within 1e-12 + 64 eps x sum |terms| (5o's criterion for its functionals; the means: that over
    the bin's area, plus the quotient's rounding); count is exact; Q is the Python charge statement applied to the record's own I, bit
    for bit."""
    d = runs(name, gpu_lib, pore10)
    assert d["counts"], name
    if name == "c3x6":
        assert d["counts"] == [2, 3, 7]
    for nb in d["counts"]:
        got = d["dev"][nb]
        assert got.shape == (5, nb) and np.all(got["status"] == 0)
        edges = P.uniform_edges(d["lo"], d["hi"], nb)
        assert np.array_equal(got["z_lo"][0], edges[:-1]) and np.array_equal(got["z_hi"][0], edges[1:])
        for k, ref in enumerate(d["ref"][nb]):
            r = got[k]
            assert np.array_equal(r["count"], ref["count"]) and r["count"].sum() == len(d["z"])
            assert (np.abs(r["D"] - ref["D"]) <= 1e-12 + 64 * EPS * ref["scale_D"]).all()
            assert (np.abs(r["I"] - ref["I"]) <= 1e-12 + 64 * EPS * ref["scale_I"]).all()
            assert (np.abs(r["area"] - ref["area"]) <= 1e-12 + 64 * EPS * ref["area"]).all()
            mean_ref = np.c_[ref["u_mean"], ref["p_mean"]]
            mean_got = np.c_[r["u_mean"], r["p_mean"]]
            tol = (1e-12 + 64 * EPS * ref["scale_u"]) / ref["area"][:, None] + 4 * EPS * np.abs(mean_ref)
            worst = float((np.abs(mean_got - mean_ref) / tol).max())
            print("%s %d bins step %d: D %.1e I %.1e means %.2f of the bound" % (name, nb, k, np.abs(r["D"] - ref["D"]).max(), np.abs(r["I"] - ref["I"]).max(), worst))
            assert worst <= 1.0
        Q = [[0.0] * 4 for _ in range(nb)]
        for k in range(5):
            Q = [P.wall_profile_charge(Q[b], HS[k], got["I"][k, b]) for b in range(nb)]
            assert bits(np.array(Q)) == bits(got["Q"][k])


def test_a_bins_bits_do_not_depend_on_the_number_of_bins(gpu_lib, pore10):
    """[0, 1/2, 1] and [0, 1/4, 1/2, 1] on (3, 6): the last bin holds the same nodes (z >= 1/2, the edge ON a layer) and has equal bits."""
    d = runs("c3x6", gpu_lib, pore10)
    with gpu_lib.DeviceSolver(d["prob"]) as dev:
        two = appended(dev, [0.0, 0.5, 1.0], d["states"], trace=False)[1]
        three = appended(dev, [0.0, 0.25, 0.5, 1.0], d["states"], trace=False)[1]
    assert np.array_equal(two["count"][0], [int((d["z"] < 0.5).sum()), int((d["z"] >= 0.5).sum())])
    for key in COMPARED_BITS:
        assert bits(two[key][:, 1]) == bits(three[key][:, 2]), key
    assert bits(two) == bits(d["dev"][2])          # the uniform edges of two bins are these


def test_kinetics_off_gives_zero_currents(gpu_lib, pore10):
    d = runs("c3x6", gpu_lib, pore10)
    with gpu_lib.DeviceSolver(d["prob"]) as dev:
        dev.set_kinetics(None)
        off = appended(dev, P.uniform_edges(0.0, 1.0, 3), d["states"], trace=False)[1]
    on = d["dev"][3]
    assert not off["I"].any() and not off["Q"].any() and np.all(off["status"] == 0)
    for key in ("area", "D", "p_mean", "u_mean", "count", "t", "h", "z_lo", "z_hi"):
        assert bits(off[key]) == bits(on[key]), key


def test_a_value_that_is_not_finite_marks_its_bin_only(gpu_lib, pore10):
    """A NaN planted in one species value of a wall node of the layer z = 1/6 of (3, 6), with the edges [0, 1/2, 1]: every facet of that
    node lies in bin 0, which gets bit 1; bin 1 keeps the bits of the clean run."""
    d = runs("c3x6", gpu_lib, pore10)
    prob = d["prob"]
    nodes, _, z = PPR.wall_nodes_z(prob)
    I = int(nodes[np.argmin(np.abs(z - 1.0 / 6.0))])
    assert abs(prob.coords[I, 2] - 1.0 / 6.0) < 1e-12
    states = [u.copy() for u in d["states"]]
    states[2][I * prob.nf + 0] = math.nan
    with gpu_lib.DeviceSolver(prob) as dev:
        got = appended(dev, [0.0, 0.5, 1.0], states, trace=False)[1]
    clean = d["dev"][2]
    assert got["status"][:, 0].tolist() == [0, 0, 1, 0, 0] and not got["status"][:, 1].any()
    for key in COMPARED_BITS:
        assert bits(got[key][:, 1]) == bits(clean[key][:, 1]), key
    assert bits(got[:2]) == bits(clean[:2])


def test_full_buffer_empty_bin_refusals_and_hook_32(pore10, gpu_lib):
    from test_kinetics_reference import _edl_k, first_step_problem
    from gmpnp_amd import dist
    from gmpnp_amd.problem import pore_hierarchy
    from gmpnp_amd.solver import GMPNPSystem

    def refused(call, what="wall profile"):
        with pytest.raises(gpu_lib.GmpnpError, match=what) as ei:
            call()
        assert ei.value.code == gpu_lib.ERR_INVALID

    prob = PP.cylinder_case((1, 2), p_M=P_M)
    states = states_of(prob, 5, seed=9)
    E = [0.0, 0.5, 1.0]
    with gpu_lib.DeviceSolver(prob) as dev:
        dev.set_state(states[0], states[0])
        for call in (lambda: dev.wall_profile_append(1.0, 1.0), lambda: dev.wall_profile_read(0, 1), lambda: dev.wall_profile_close(),
                     lambda: dev.wall_profile_open(E, 0), lambda: dev.wall_profile_open(E, -3)):
            refused(call)
        refused(lambda: dev.time_kernel(32, 1), "32")                     # no open profile
        for edges in ([0.0, 0.6, 0.5, 1.0], [0.0, 0.5, 0.5, 1.0], [0.0, math.nan, 1.0], [0.0, math.inf], [0.0], list(np.linspace(0.0, 1.0, 258))):
            refused(lambda: dev.wall_profile_open(edges, 4))
        refused(lambda: dev.wall_profile_open(P.uniform_edges(0.0, 1.0, 4), 4), "bin 1 of 4")     # the layers are 0, 1/2, 1: [1/4, 1/2) is empty
        refused(lambda: dev.wall_profile_append(1.0, 1.0))                 # a refused open opens nothing
        dev.wall_profile_open(E, 2)
        for h in (0.0, -1.0, math.nan, math.inf):
            refused(lambda: dev.wall_profile_append(1.0, h))
        refused(lambda: dev.wall_profile_append(math.nan, 1.0))
        refused(lambda: dev.wall_profile_read(0, 1))                       # nothing written yet
        for k in (1, 2):
            dev.set_state(states[k], None)
            dev.wall_profile_append(float(k), 1.0)
        before = dev.wall_profile_read(0, 2)
        dev.set_state(states[3], None)
        refused(lambda: dev.wall_profile_append(3.0, 1.0), "full")         # full: refused,
        assert bits(dev.wall_profile_read(0, 2)) == bits(before)           # and nothing is overwritten
        refused(lambda: dev.wall_profile_read(1, 2))
        refused(lambda: dev.wall_profile_read(-1, 1))
        assert dev.time_kernel(32, 3) > 0.0                                # the hook writes a row and charges of its own
        assert bits(dev.wall_profile_read(0, 2)) == bits(before)
        dev.wall_profile_open(E, 2)                                        # opened again: the charges start at 0
        dev.wall_profile_append(4.0, 2.0)
        r = dev.wall_profile_read(0, 1)[0]
        assert bits(r["Q"]) == bits(np.array([P.wall_profile_charge([0.0] * 4, 2.0, r["I"][b]) for b in range(2)]))
        dev.wall_profile_close()
        refused(lambda: dev.wall_profile_append(5.0, 1.0))
        refused(lambda: dev.time_kernel(32, 1), "32")
        dev.wall_profile_open(E, 2)
        dev.set_galvanostat(Galvanostat(1.0))
        refused(lambda: dev.wall_profile_append(5.0, 1.0))
        refused(lambda: dev.wall_profile_open(E, 4))
        refused(lambda: dev.time_kernel(32, 1))
        dev.set_galvanostat(None)
        dev.set_stern(None)
        refused(lambda: dev.wall_profile_open(E, 4))
        refused(lambda: dev.wall_profile_append(5.0, 1.0))
    plain = copy.copy(prob)
    plain.stern, plain.kinetics = None, None
    with gpu_lib.DeviceSolver(plain) as never:                             # a handle that never had the Stern option
        refused(lambda: never.wall_profile_open(E, 4))
    ep, m1 = _edl_k()
    with gpu_lib.DeviceSolver(first_step_problem(ep, m1, -5.0)) as d1:     # 1D: the electrode record is its profile
        refused(lambda: d1.wall_profile_open([0.0, 1.0], 4), "electrode record")
    pp, mesh, prob3, _ = pore10
    dom, perm, part = dist.partition_plan(prob3, 2, 0)
    with gpu_lib.DeviceSolver(dom.problem, perm=perm, partition=part) as partitioned:
        refused(lambda: partitioned.wall_profile_open(E, 4))
    levels = pore_hierarchy(pp, mesh, 1)
    ml = GMPNPSystem(levels[0][0], levels=levels)
    try:
        refused(lambda: ml.dev.wall_profile_open(E, 4))                    # a coarse level attached,
        refused(lambda: ml._coarse[0].wall_profile_open(E, 4))             # and the handle that serves as one
    finally:
        ml.close()


# ---- a handle that never opens the profile ---------------------------------------------------------------------------------------------
def test_a_twin_that_never_opens_the_profile_has_equal_bits(gpu_lib):
    """The same three time steps on two handles, one with the profile open and appended to: equal bits of state, trace records and
    Newton residuals."""
    prob = PP.cylinder_case((2, 3), p_M=P_M)
    un = np.tile(np.r_[np.ones(prob.nf - 1), 0.0], prob.coords.shape[0])
    sp = {"newton_solver": dict(NEWTON["newton_solver"], linear_solver="band_lu")}
    opts = gpu_lib.newton_options(sp, dim=3)
    h = 1.0 / float(prob.model.inv_dt)
    got = []
    for with_profile in (True, False):
        with gpu_lib.DeviceSolver(prob) as dev:
            dev.set_state(un, un)
            dev.electrode_trace_open(4)
            if with_profile:
                dev.wall_profile_open([0.0, 1.0 / 3.0, 1.0], 4)
            res = []
            for k in range(3):
                dev.set_electrode_potential(P_M - 0.1 * k)
                dev.set_time_step(1.0 / h)
                st = dev.newton_solve(opts)
                res.append(list(st["residuals"]))
                dev.electrode_trace_append((k + 1) * h, h)
                if with_profile:
                    dev.wall_profile_append((k + 1) * h, h)
                dev.time_accept()
            if with_profile:
                assert dev.time_kernel(32, 2) > 0.0
                assert np.all(dev.wall_profile_read(0, 3)["status"] == 0)
            got.append((bits(dev.get_state()), bits(dev.electrode_trace_read(0, 3)), res))
    assert got[0][0] == got[1][0] and got[0][1] == got[1][1] and got[0][2] == got[1][2]


# ---- fixed-mode programmes against the NumPy system ------------------------------------------------------------------------------------
class HandleRun:
    """What ``DeviceProgrammeOps`` reads of a driver run, over a bare problem."""

    def __init__(self, prob):
        from gmpnp_amd.solver import GMPNPSystem
        self.problem, self.stern, self.kinetics, self.budget = prob, prob.stern, prob.kinetics, None
        self.sys = GMPNPSystem(prob)


# The bound test_gpu_kinetics.py puts on a driver step against kinetics_reference.newton_loop and 5n reused: 1e-8 of the largest
# reference value.  Measured values: DESIGN.md section 5q.
REFERENCE_BOUND = 1e-8
TRACE_COMPARED = ("p_boundary", "D", "dD_dt", "I", "Q", "Q_D", "u_boundary")
PROFILE_COMPARED = ("area", "D", "I", "Q", "p_mean", "u_mean")

_REFERENCE = {}


def reference_march(name):
    """The CPU side, once per cylinder: the reference marches of both programmes."""
    if name not in _REFERENCE:
        prob, u, dt = PPR.march_case(PPR.MARCH_CYLINDERS[name])
        edges = P.uniform_edges(0.0, 1.0, PPR.MARCH_BINS)
        out = {}
        for kind, segs in PPR.march_programmes(dt).items():
            ref = PPR.NumpyPoreProgrammeSystem(prob, u, lambda h: 1.0 / h, edges)
            P.run_programme(ref, segs, steps_per_segment=PPR.MARCH_STEPS_PER_SEGMENT)
            out[kind] = (segs, ref)
        _REFERENCE[name] = (prob, u, edges, out)
    return _REFERENCE[name]


@pytest.mark.parametrize("kind", ["pulse", "triangle"])
@pytest.mark.parametrize("name", list(PPR.MARCH_CYLINDERS))
def test_fixed_programme_against_the_reference(name, kind, gpu_lib):
    prob, u, edges, marches = reference_march(name)
    segs, ref = marches[kind]
    want = ref.arrays()
    run = HandleRun(copy.copy(prob))
    sp = {"newton_solver": dict(NEWTON["newton_solver"], linear_solver="band_lu")}
    try:
        run.sys.set_state(np.array(u), np.array(u))
        ops = P.DeviceProgrammeOps(run, sp, lambda h: 1.0 / h, capacity=5, profile_edges=edges)      # smaller than the run: both buffers drain
        out = P.run_programme(ops, segs, steps_per_segment=PPR.MARCH_STEPS_PER_SEGMENT)
        rec = ops.records()
        prof = ops.profile_records()
        u_end = run.sys.dev.get_state()
    finally:
        run.sys.close()
    n = PPR.MARCH_STEPS_PER_SEGMENT * len(segs)
    assert len(rec) == n == len(want["t"]) and prof.shape == (n, PPR.MARCH_BINS) and len(ops.chunks) >= 2 and len(ops.profile_chunks) >= 2
    assert np.array_equal(rec["t"], want["t"]) and np.array_equal(rec["h"], want["h"]) and np.array_equal(rec["p_M"], want["p_M"])
    assert np.array_equal(prof["t"][:, 0], want["t"]) and np.array_equal(prof["h"][:, 1], want["h"])
    assert [t for _, t, _ in ops.states] == [g[1] for g in segs] == out["breakpoints"] and np.all(rec["status"] == 0) and np.all(prof["status"] == 0)
    worst = {}
    for key in TRACE_COMPARED:
        got = rec[key][:, :want[key].shape[1]] if rec[key].ndim == 2 else rec[key]
        worst[key] = float(np.abs(got - want[key]).max() / np.abs(want[key]).max())
    for key in PROFILE_COMPARED:
        w = np.array([pr[key] for pr in ref.profiles])
        got = prof[key][..., :w.shape[-1]] if w.ndim == 3 else prof[key]
        worst["profile_" + key] = float(np.abs(got - w).max() / np.abs(w).max())
    worst["u"] = float(np.abs(u_end - ref.u).max() / max(1.0, np.abs(ref.u).max()))
    print("pore programme %s on %s against the reference: %s" % (kind, name, {k: "%.2e" % v for k, v in worst.items()}))
    assert max(worst.values()) <= REFERENCE_BOUND, worst
    assert np.array_equal(prof["count"][0], ref.profiles[0]["count"])
    assert run.stern.p_electrode == segs[-1][3] and run.kinetics.p_electrode == segs[-1][3]


# ---- the driver ------------------------------------------------------------------------------------------------------------------------
KW = dict(L=10e-9, R=5e-9, concentration_elec=0.5, electrode_voltage=-1.0, kinetics="tafel", i0_CO=10.0, i0_H2=1.0)     # the README's Tafel example
LEVELS = [-1.25, -0.75]


@pytest.fixture(scope="module")
def pulse_run(tmp_path_factory, gpu_lib):
    """PoreRun on L_10_R_5: two schedule steps, then two short pulse cycles in fixed mode written by write_outputs (budget on, capacity 3:
    the buffers drain on the way, 4 bins); and the same run without the option."""
    from gmpnp_amd.params import pore_parameters
    from gmpnp_amd.pore3d import SOLVER_PARAMETERS, PoreRun
    from gmpnp_amd.solver import column_medians
    out_dir = tmp_path_factory.mktemp("pore_programme")
    os.environ["GMPNP_OUT"] = str(out_dir)
    step_s = pore_parameters(concentration_elec=0.5, L=10e-9, R=5e-9).time_step
    par = dict(kind="pulse", v_levels=LEVELS, durations=[2.0 * step_s, step_s], cycles=2, steps_per_segment=2, capacity=3, bins=4)
    sp = {"nonlinear_solver": "newton", "newton_solver": dict(SOLVER_PARAMETERS["newton_solver"], linear_solver="band_lu")}
    try:
        run = PoreRun(num_steps=2, solver_parameters=sp, budget=True, pore_programme=par, **KW)
        try:
            run.run(verbose=False)
            n_schedule = run.n
            path = run.write_outputs(stamp="pulse")
            last = run.sys.vertex_values()
            after = dict(stern=run.stern.p_electrode, kinetics=run.kinetics.p_electrode, options=run.sys.dev.electrode_options(), budget=run.budget.array(),
                         n_schedule=n_schedule, pp=run.pp, D=run.sys.dev.stern_displacement(), u=last, co2_bc=run.co2_bc, wall_area=run.wall_area(),
                         co2_want=run.pp.sechenov_co2_scaled(*column_medians(last, (1, 2, 3, 7))), par=par)
        finally:
            run.sys.close()
        off = PoreRun(num_steps=2, solver_parameters=sp, budget=True, **KW)
        try:
            off.run(verbose=False)
            path_off = off.write_outputs(stamp="off")
        finally:
            off.sys.close()
    finally:
        del os.environ["GMPNP_OUT"]
    return dict(path=path, path_off=path_off, **after)


def test_driver_writes_the_programme(pulse_run):
    z = np.load(os.path.join(pulse_run["path"], "pore_programme.npz"))
    assert sorted(z.files) == sorted(P.PORE_OUTPUT_KEYS)                             # exactly the listed keys
    pp = pulse_run["pp"]
    segs = P.build(pulse_run["par"], -1.0, pp.time_constant, pp.thermal_voltage)
    n = len(z["time_s"])
    assert n == 2 * len(segs) == 8
    meta = json.load(open(os.path.join(pulse_run["path"], "metadata.json")))
    for key in P.PORE_METADATA_KEYS:
        assert key in meta, key
    assert meta["pore_programme_kind"] == "pulse" and meta["pore_programme_cycles"] == 2 and meta["pore_programme_segments"] == 4
    assert meta["pore_programme_steps_accepted"] == n and meta["pore_programme_stop_reason"] == "end" and meta["pore_programme_status"] == 0
    assert meta["pore_programme_bins"] == 4 and np.all(z["status"] == 0) and np.all(z["profile_status"] == 0)
    # the breakpoints are landed exactly, with the level of the segment that ends there
    for k, g in enumerate(segs):
        last = np.nonzero(z["segment"] == k)[0][-1]
        assert z["time_s"][last] == g[1] * pp.time_constant and z["electrode_voltage"][last] == g[3]
    st = np.load(os.path.join(pulse_run["path"], "pore_programme_states.npz"))
    assert np.array_equal(st["time_s"], [g[1] * pp.time_constant for g in segs]) and st["states"].shape == (4, len(st["coor"]), 9)
    assert bits(st["states"][-1]) == bits(pulse_run["u"])
    # the run, the handle's options and the metadata end at the last level
    assert pulse_run["stern"] == pulse_run["kinetics"] == LEVELS[1] == meta["electrode_voltage"] == meta["pore_programme_electrode_voltage"]
    assert pulse_run["options"][0]["p_electrode"] == pulse_run["options"][1]["p_electrode"] == LEVELS[1]
    assert meta["stern_displacement"] == pulse_run["D"]
    # the bins add up to the wall: sum_b profile_i_CO x bin area = i_CO x wall area within 64 eps x sum |terms|
    L2 = pp.L * pp.L
    assert z["profile_i_CO"].shape == (n, 4) and z["bin_area_m2"].shape == z["z_lo_m"].shape == z["z_hi_m"].shape == (4,)
    for a, b in (("profile_i_CO", "i_CO"), ("profile_i_H2", "i_H2"), ("profile_charge_CO", "charge_CO"), ("profile_surface_charge", "surface_charge")):
        terms = z[a] * z["bin_area_m2"][None, :]
        whole = z[b] * (pulse_run["wall_area"] * L2)
        gap = np.abs(terms.sum(axis=1) - whole)
        bound = 64 * EPS * np.abs(terms).sum(axis=1) * (n if "charge_C" in a else 1)     # (a charge is a sum over the steps so far)
        print("driver %s: worst gap / bound %.3f" % (a, float((gap / bound).max())))
        assert (gap <= bound).all(), a
    assert abs(z["bin_area_m2"].sum() - pulse_run["wall_area"] * L2) <= 64 * EPS * pulse_run["wall_area"] * L2
    assert z["z_lo_m"][0] == 0.0 and z["z_hi_m"][-1] == pp.L and np.array_equal(z["z_lo_m"][1:], z["z_hi_m"][:-1])
    assert np.all(np.abs(np.diff(z["profile_charge_CO"], axis=0)) > 0.0)
    # the lagged Sechenov update ran behind the last accepted step, from the medians of the last state
    assert pulse_run["co2_bc"] == pulse_run["co2_want"]
    # the attempts and one budget row per accepted step
    log = np.load(os.path.join(pulse_run["path"], "timestep_log.npz"))
    assert int(log["pore_programme_accepted"].sum()) == n and len(log["pore_programme_t"]) == n
    assert len(pulse_run["budget"]) == pulse_run["n_schedule"] + n and np.isfinite(pulse_run["budget"]).all()


def test_without_the_option_a_run_writes_what_it_wrote(pulse_run):
    on, off = set(os.listdir(pulse_run["path"])), set(os.listdir(pulse_run["path_off"]))
    assert sorted(on - off) == ["pore_programme.npz", "pore_programme_states.npz", "timestep_log.npz"]
    assert not off - on and "budget.npz" in off and "metadata.json" in off
    m_on, m_off = (json.load(open(os.path.join(pulse_run[p], "metadata.json"))) for p in ("path", "path_off"))
    assert not [k for k in m_off if k.startswith("pore_programme")] and "timestep_log" not in m_off
    assert set(m_on) - set(m_off) == set(P.PORE_METADATA_KEYS) | {"timestep_log"}
    for f in ("arrays_scaled.npz", "arrays_unscaled.npz", "budget.npz"):
        assert sorted(np.load(os.path.join(pulse_run["path"], f)).files) == sorted(np.load(os.path.join(pulse_run["path_off"], f)).files), f
    assert sorted(np.load(os.path.join(pulse_run["path_off"], "arrays_unscaled.npz")).files) == sorted(
        ["H", "OH", "HCO3", "CO32", "CO2", "CO", "H2", "cat", "p", "coor", "tau", "field_values", "H_grad", "OH_grad", "HCO3_grad", "CO32_grad",
         "CO2_grad", "CO_grad", "H2_grad", "cat_grad", "i_CO", "i_H2", "FE_H2"])
    # the schedule's arrays are those of the run without the option, bit for bit
    for key in ("CO2", "p", "i_CO"):
        a, b = (np.load(os.path.join(pulse_run[p], "arrays_unscaled.npz"))[key] for p in ("path", "path_off"))
        assert bits(a) == bits(b), key


def test_command_line(gpu_lib, tmp_path):
    import subprocess
    import sys
    from gmpnp_amd.params import pore_parameters
    pp = pore_parameters(concentration_elec=0.5, L=10e-9, R=5e-9)
    rate = 0.25 * pp.thermal_voltage / (2.0 * pp.time_step)          # V/s: a leg of a quarter thermal voltage takes two reference steps
    env = dict(os.environ, GMPNP_OUT=str(tmp_path))
    cmd = [sys.executable, os.path.join(ROOT, "3D", "MPNP_CO2ER_pore.py"), "--L=10e-9", "--R=5e-9", "--concentration_elec=0.5", "--electrode_voltage=-1",
           "--kinetics=tafel", "--i0_CO=10", "--i0_H2=1", "--num_steps=1", "--pore_programme", "triangle", "--v_vertex=-1.25", "--scan_rate=%r" % rate,
           "--cycles=1", "--pore_programme_steps_per_segment=2", "--pore_programme_bins=3"]
    subprocess.run(cmd, check=True, env=env, cwd=str(tmp_path), stdout=subprocess.DEVNULL)
    found = [os.path.join(d, "pore_programme.npz") for d, _, files in os.walk(str(tmp_path)) if "pore_programme.npz" in files]
    assert len(found) == 1
    z = np.load(found[0])
    assert len(z["time_s"]) == 4 and z["electrode_voltage"][1] == -1.25 and z["electrode_voltage"][3] == -1.0
    assert z["profile_i_CO"].shape == (4, 3) and np.all(z["profile_status"] == 0)
    assert np.isclose(z["time_s"][-1], 4.0 * pp.time_step, rtol=1e-12)
