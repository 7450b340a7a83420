"""Adaptive time stepping on the GPU (include/gmpnp.h "adaptive time stepping", csrc/gmpnp_time_step.h, gmpnp_amd/timestep.py): the
estimator kernels against the NumPy model of tests/time_step_reference.py, accept / reject, gmpnp_set_time_step against handles
created with the step (and its forwarding to attached coarse levels), adaptive runs against the reference loop over the oracle's
assembly, "off means off", the refusals and the 1D driver's command line.

Newton tolerances of the runs compared with the reference loop: tests/test_time_step_reference.py (relative 1e-9, absolute 1e-6, and
why not 1e-10).  Newton counts are compared on every attempt that is not a Newton failure: a failed solve's iterates are outside
the admissible set, where nothing pins them."""
import contextlib
import copy
import dataclasses
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import hp_reference as H
import test_time_step_reference as C
import time_step_reference as T
from conftest import ROOT, _edl

pytestmark = pytest.mark.gpu

RTOL = 1e-2
H_STEP, H_PREV = 0.11, 0.07   # unequal steps of the estimator cases


def estimator_problem(name):
    if name == "edl1":
        return _edl(L_n=1e-6, cation="Cs", voltage_multiplier=-10.0)[2]
    if name == "pore10":
        from conftest import _pore
        return _pore(10e-9, 5e-9)[2]
    return H.edl_generated(H.uniform_mesh_1d(int(name)))


def triple(prob, seed):
    """Random admissible (u, u_n, u_nm1), (nv, nf) each: species in (0.5, 1.5) scaled to a steric sum of at most 0.9, potential in
    (-1, 0)."""
    rng = np.random.default_rng(seed)
    nv, nf = prob.coords.shape[0], prob.nf
    a = np.asarray(prob.model.a, dtype=np.float64)[:nf - 1]
    out = []
    for _ in range(3):
        u = np.concatenate([rng.uniform(0.5, 1.5, (nv, nf - 1)), rng.uniform(-1.0, 0.0, (nv, 1))], axis=1)
        u[:, :nf - 1] *= np.minimum(1.0, 0.9 / T.steric_sum(a, u))[:, None]
        out.append(u)
    return out


def load(dev, u, un, unm1):
    """(u, u_n, u_nm1) onto a handle with the history flag set: u <- un, u_n <- unm1, accept, then u alone."""
    dev.set_state(un.ravel(), unm1.ravel())
    dev.time_accept()
    dev.set_state(u.ravel(), None)   # (a set_state that leaves u_n alone keeps the history)


def compare(e, m, nf, tol=1e-12):
    assert e["has_history"] == m["has_history"] and e["nonfinite"] == m["nonfinite"]
    for key in ("err_field", "rate_field"):
        a, b = np.asarray(e[key]), np.asarray(m[key])
        assert a.shape == (nf,)
        assert np.all(np.abs(a - b) <= tol * np.abs(b)), (key, a, b)   # (0 against 0 where a field has no free dof or no history)
    assert e["err"] == max(e["err_field"]) and e["rate"] == max(e["rate_field"])
    assert e["worst_dof"] == m["worst_dof"], (e["worst_dof"], m["worst_dof"])


@pytest.mark.parametrize("name", ["2", "255", "256", "257", "513", "edl1", "pore10"])
def test_estimator_against_the_numpy_model(gpu_lib, name):
    """err_field / rate_field to 1e-12 relative (both sum <= 1,767 squares in different orders: n 2^-53 ~ 2e-13), worst_dof as an
    integer with a dominant term planted at the first node, the last node and every field of a mid node."""
    prob = estimator_problem(name)
    nv, nf = prob.coords.shape[0], prob.nf
    assert nv == {"edl1": 1091, "pore10": 1767}.get(name, None) or nv == int(name)
    u, un, unm1 = triple(prob, seed=nv)
    atol = np.linspace(1e-4, 3e-4, nf)   # per-field atol
    free = T.free_mask(prob)
    with gpu_lib.DeviceSolver(prob) as dev:
        # no history before the first accept: err 0, the rates all the same
        dev.set_state(u.ravel(), un.ravel())
        e = dev.time_error(H_STEP, H_PREV, RTOL, atol)
        compare(e, T.time_error(u, un, None, H_STEP, H_PREV, RTOL, atol, free), nf)
        assert not e["has_history"] and e["err"] == 0.0 and e["rate"] > 0.0 and e["worst_dof"] == -1
        load(dev, u, un, unm1)
        e = dev.time_error(H_STEP, H_PREV, RTOL, atol)
        m = T.time_error(u, un, unm1, H_STEP, H_PREV, RTOL, atol, free)
        compare(e, m, nf)
        assert e["has_history"] and e["err"] > 0.0
        # two calls give identical bits
        e2 = dev.time_error(H_STEP, H_PREV, RTOL, atol)
        assert e2["err"] == e["err"] and np.array_equal(e2["err_field"], e["err_field"]) and np.array_equal(e2["rate_field"], e["rate_field"])
        # h_prev <= 0: no history either
        e0 = dev.time_error(H_STEP, 0.0, RTOL, atol)
        assert not e0["has_history"] and e0["err"] == 0.0 and np.array_equal(e0["rate_field"], e["rate_field"])
        # a dominant term planted in turn (in u_nm1: the weights do not see it): a field of the first node, one of the last node,
        # every field of a mid node; free dofs only
        first = [(0, f) for f in range(nf) if free[0, f]][:1]
        I_last = int(np.nonzero(free.any(axis=1))[0][-1])   # (the last vertex of an interval mesh is all Dirichlet: the one before it)
        last = [(I_last, f) for f in range(nf) if free[I_last, f]][-1:]
        mid = [(nv // 2, f) for f in range(nf) if free[nv // 2, f]]
        assert first and last and (nv < 3 or mid) and I_last >= nv - 2
        for I, f in first + last + mid:
            mp = unm1.copy()
            mp[I, f] += 1e3
            load(dev, u, un, mp)
            ep = dev.time_error(H_STEP, H_PREV, RTOL, atol)
            compare(ep, T.time_error(u, un, mp, H_STEP, H_PREV, RTOL, atol, free), nf)
            assert ep["worst_dof"] == I * nf + f
        load(dev, u, un, unm1)
        # Dirichlet dofs with a 1e6 jump are ignored
        bc = np.asarray(prob.bc_dofs, dtype=np.int64)
        assert len(bc)
        uj = u.copy().ravel()
        uj[bc] += 1e6
        dev.set_state(uj, None)
        ej = dev.time_error(H_STEP, H_PREV, RTOL, atol)
        assert np.array_equal(ej["err_field"], e["err_field"]) and np.array_equal(ej["rate_field"], e["rate_field"]) and ej["worst_dof"] == e["worst_dof"]
        # a planted NaN: nonfinite = 1, status OK, err NaN
        un_ = u.copy()
        un_[nv // 3, 1] = np.nan
        dev.set_state(un_.ravel(), None)
        en = dev.time_error(H_STEP, H_PREV, RTOL, atol)
        assert en["nonfinite"] and np.isnan(en["err"]) and np.all(np.isnan(en["err_field"]))
        # a set_state that writes u_n drops the history
        dev.set_state(u.ravel(), un.ravel())
        assert not dev.time_error(H_STEP, H_PREV, RTOL, atol)["has_history"]
        # ... and so does assign_previous after an accept
        dev.time_accept()
        assert dev.time_error(H_STEP, H_PREV, RTOL, atol)["has_history"]
        dev.assign_previous()
        assert not dev.time_error(H_STEP, H_PREV, RTOL, atol)["has_history"]


def test_a_field_whose_dofs_are_all_dirichlet_reports_zero(gpu_lib):
    prob = estimator_problem("257")
    nv, nf = prob.coords.shape[0], prob.nf
    u, un, unm1 = triple(prob, seed=5)
    with gpu_lib.DeviceSolver(prob) as dev:
        dofs = np.arange(nv, dtype=np.int64) * nf + 2
        dev.set_dirichlet(dofs, u[:, 2].copy())
        load(dev, u, un, unm1)
        e = dev.time_error(H_STEP, H_PREV, RTOL, 1e-4)
        free = np.ones((nv, nf), dtype=bool)
        free[:, 2] = False
        compare(e, T.time_error(u, un, unm1, H_STEP, H_PREV, RTOL, 1e-4, free), nf)
        assert e["err_field"][2] == 0.0 and e["rate_field"][2] == 0.0 and e["err"] > 0.0


@pytest.mark.parametrize("name", ["edl1", "pore10"])
def test_accept_and_reject(gpu_lib, name):
    prob = estimator_problem(name)
    nv, nf = prob.coords.shape[0], prob.nf
    u, un, unm1 = triple(prob, seed=21)
    u2 = triple(prob, seed=22)[0]
    free = T.free_mask(prob)
    with gpu_lib.DeviceSolver(prob) as dev:
        load(dev, u, un, unm1)
        dev.time_accept()
        assert np.array_equal(dev.get_state(previous=True), u.ravel()) and np.array_equal(dev.get_state(), u.ravel())
        dev.set_state(u2.ravel(), None)
        e = dev.time_error(H_STEP, H_PREV, RTOL, 1e-4)
        compare(e, T.time_error(u2, u, un, H_STEP, H_PREV, RTOL, 1e-4, free), nf)   # the former u_n is u_nm1 now
        dev.time_reject()
        assert np.array_equal(dev.get_state(), u.ravel()) and np.array_equal(dev.get_state(previous=True), u.ravel())
        dev.set_state(u2.ravel(), None)
        e2 = dev.time_error(H_STEP, H_PREV, RTOL, 1e-4)   # the history is unchanged
        assert e2["has_history"] and e2["err"] == e["err"] and np.array_equal(e2["err_field"], e["err_field"])


# ---- gmpnp_set_time_step ------------------------------------------------------------------------------------------------------------
def with_inv_dt(prob, x):
    p = copy.copy(prob)
    p.model = dataclasses.replace(prob.model, inv_dt=float(x))
    return p


@pytest.mark.parametrize("name", ["edl1", "pore10"])
def test_set_time_step_equals_a_handle_created_with_the_step(gpu_lib, name):
    prob = estimator_problem(name)
    u, un, _ = triple(prob, seed=31)
    for x in (prob.model.inv_dt / 7.0, 0.0):
        with gpu_lib.DeviceSolver(with_inv_dt(prob, prob.model.inv_dt)) as a, gpu_lib.DeviceSolver(with_inv_dt(prob, x)) as b:
            for d in (a, b):
                d.set_state(u.ravel(), un.ravel())
            a.assemble(True)                      # a Jacobian at the old step, to be invalidated
            a.set_time_step(x)
            Fa, ra = a.assemble(True)
            Fb, rb = b.assemble(True)
            assert np.array_equal(Fa, Fb) and ra == rb and np.all(np.isfinite(Fa))
            Ja, Jb = a.jacobian_csr(), b.jacobian_csr()
            assert np.array_equal(Ja.indptr, Jb.indptr) and np.array_equal(Ja.indices, Jb.indices) and np.array_equal(Ja.data, Jb.data)
    with gpu_lib.DeviceSolver(prob) as a:
        for bad in (np.nan, np.inf, -1.0):
            with pytest.raises(gpu_lib.GmpnpError) as ei:
                a.set_time_step(bad)
            assert ei.value.code == gpu_lib.ERR_INVALID


def test_set_time_step_reaches_the_coarse_levels(gpu_lib):
    """The generated 114-vertex cylinder under its refinement (671 vertices), the multilevel term attached: after
    set_time_step(inv_dt / 50) the first Newton system takes the BiCGStab iterations of a hierarchy built with that step.  Red when
    gmpnp_set_time_step leaves the coarse level's model as it was (the time term is the diagonal of the species blocks)."""
    import precond_reference as R
    hier = R.cylinder_hierarchy(1)
    assert [h[0].coords.shape[0] for h in hier] == [671, 114]
    x = hier[0][0].model.inv_dt / 50.0
    u, un = R.case_state("ml1", hier[0][0])
    its = []
    for late in (False, True):
        probs = [h[0] if late else with_inv_dt(h[0], x) for h in hier]
        with contextlib.ExitStack() as stack:
            fine = stack.enter_context(gpu_lib.DeviceSolver(probs[0]))
            coarse = stack.enter_context(gpu_lib.DeviceSolver(probs[1], shared_device=1))
            gpu_lib.attach_level_chain([fine, coarse], [hier[0][1]], theta=R.ML_THETA, sweeps=R.ML_SWEEPS)
            if late:
                fine.set_time_step(x)
            fine.set_state(u, un)
            F, _ = fine.assemble(True)
            b = fine.spmv(R.x_true(fine.ndof))
            _, st = fine.linear_solve(b, gpu_lib.LINEAR_TWOLEVEL, rtol=1e-10)
            assert st["converged"]
            its.append(st["iterations"])
    print("BiCGStab iterations: hierarchy built with the step %d, step set afterwards %d" % tuple(its))
    assert its[0] == its[1]


# ---- adaptive runs against the reference loop --------------------------------------------------------------------------------------
SOLVER_1D = {"nonlinear_solver": "newton", "newton_solver": {"maximum_iterations": 25, "relative_tolerance": 1e-9, "absolute_tolerance": 1e-6}}


@pytest.mark.parametrize("cation,voltage", sorted(C.CASES))
def test_adaptive_edl_run_against_the_reference_loop(gpu_lib, cation, voltage):
    from gmpnp_amd.edl1d import EDLRun
    c = C.CASES[(cation, voltage)]
    ep, base, pert = C.reference_runs(cation, voltage)
    s_err, s_u = T.sensitivity(base, pert)
    run = EDLRun(solver_parameters=SOLVER_1D, adaptive_dt=True, dt_rtol=c["dt_rtol"], dt_atol=C.DT_ATOL, t_end=np.inf,
                 steady_tol=c["steady_tol"], max_steps=c["attempts"], L_n=1e-6, cation=cation, voltage_multiplier=voltage)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            run.run(verbose=False)
        log = run.stepper.log
        got = "".join("A" if r["accepted"] else ("F" if r["reason"] == 2 else "R") for r in log)
        assert got == C.letters(base)
        dh = max(abs(r["h"] - b["h"]) / b["h"] for r, b in zip(log, base.log))
        derr = max(abs(r["err"] - b["err"]) for r, b in zip(log, base.log) if not np.isnan(b["err"]))
        du = float(np.abs(run.sys.dev.get_state() - base.u).max())
        print("%s %g: s_err %.3e s_u %.3e | device against the oracle: max |dh|/h %.3e  max |derr| %.3e  final state %.3e" %
              (cation, voltage, s_err, s_u, dh, derr, du))
        assert [r["newton"] for r in log if r["reason"] != 2] == [b["newton"] for b in base.log if b["reason"] != 2]
        assert dh <= 10.0 * s_err
        assert du <= 10.0 * s_u
        assert len(run.history) == 1 + run.stepper.accepted == len(run.times) and np.all(np.diff(run.times) > 0.0)
        if cation == "K":
            assert run.stepper.stop_reason == "steady"
        else:
            assert run.stepper.stop_reason == "max_steps"
            assert all(r["steric_excursion"] == 0 for r in log if r["accepted"])   # step_fraction off
    finally:
        run.sys.close()


_pore_ref = {}


def small_pore():
    """The generated 259-vertex cylinder (3 rings, 6 layers) with the 0.5 M pore model and its full Dirichlet set: (pp, bnd, problem)."""
    from gmpnp_amd.mesh import mark_pore_boundaries
    from gmpnp_amd.meshgen import cylinder_mesh
    from gmpnp_amd.params import pore_parameters
    from gmpnp_amd.problem import Problem, pore_dirichlet
    pp = pore_parameters(concentration_elec=0.5, L=10e-9, R=5e-9)
    mesh = cylinder_mesh(pp.aspect_pore, 3, 6)
    sag = pp.aspect_pore ** 2 * (1.0 - np.cos(np.pi / 18) ** 2)
    bnd = mark_pore_boundaries(mesh, pp.aspect_pore, 1.5 * sag)
    dofs, vals = pore_dirichlet(pp, bnd)
    prob = Problem(coords=mesh.coords, cells=mesh.cells, model=pp.model, wall_facets=bnd.ds_facets[2], exit_facets=bnd.ds_facets[3],
                   bc_dofs=dofs, bc_vals=vals)
    assert mesh.coords.shape[0] == 259
    return pp, bnd, prob


def sechenov(pp, u2d):
    return pp.sechenov_co2_scaled(*[float(np.median(u2d[:, c])) for c in (1, 2, 3, 7)])


def pore_reference(perturb):
    """The reference loop with the Sechenov glue (3D:817-838) on the small cylinder: 6 attempts from 10 reference steps, omega 0.9."""
    from gmpnp_amd.problem import pore_dirichlet
    if perturb not in _pore_ref:
        pp, bnd, prob = small_pore()

        def glue(p, u2d):
            p.bc_dofs, p.bc_vals = pore_dirichlet(pp, bnd, sechenov(pp, u2d))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _pore_ref[perturb] = T.adaptive_loop(prob, T.Policy(), RTOL, C.DT_ATOL, 10.0 * pp.dt, lambda h: 1.0 / h, 6, omega=0.9,
                                                 maximum_iterations=50, relative_tolerance=1e-9, absolute_tolerance=1e-6, perturb=perturb,
                                                 on_accept=glue)
    return _pore_ref[perturb]


def test_adaptive_pore_steps_against_the_reference_loop(gpu_lib):
    """3D: the 0.5 M pore model, omega = 0.9, 6 attempts from dt_init = 10 reference steps, on the generated 259-vertex cylinder (the
    sparse LU of L_10_R_5 takes ~10 s per Newton iteration on the CPU), the Sechenov update as the glue of an accepted step."""
    from gmpnp_amd.problem import pore_dirichlet
    from gmpnp_amd.solver import GMPNPSystem, column_medians
    from gmpnp_amd.timestep import AdaptiveStepper, TimeStepPolicy
    base, pert = pore_reference(0.0), pore_reference(1e-8)
    s_err, s_u = T.sensitivity(base, pert)
    assert T.decision_margin(base.log) > 100.0 * s_err
    pp, bnd, prob = small_pore()
    params = {"nonlinear_solver": "newton", "newton_solver": {"linear_solver": "band_lu", "maximum_iterations": 50, "relative_tolerance": 1e-9,
                                                              "absolute_tolerance": 1e-6, "relaxation_parameter": 0.9}}
    sys_ = GMPNPSystem(prob)
    try:
        sys_.initialise([1.0] * 8 + [0.0])
        stepper = AdaptiveStepper(sys_, TimeStepPolicy(), (RTOL, C.DT_ATOL), lambda h: 1.0 / h, 10.0 * pp.dt, solver_parameters=params)

        def before_accept(st):
            row = sys_.vertex_values()
            sys_.set_bcs(*pore_dirichlet(pp, bnd, pp.sechenov_co2_scaled(*column_medians(row, (1, 2, 3, 7)))))
        for _ in range(6):
            stepper.attempt(None, before_accept)
        log = stepper.log
        assert [r["accepted"] for r in log] == base.sequence() and [r["reason"] == 2 for r in log] == base.failures()
        assert [r["newton"] for r in log if r["reason"] != 2] == [b["newton"] for b in base.log if b["reason"] != 2]
        dh = max(abs(r["h"] - b["h"]) / b["h"] for r, b in zip(log, base.log))
        du = float(np.abs(sys_.dev.get_state(previous=True) - base.u).max())
        print("pore (259 vertices): %s newton %s s_err %.3e s_u %.3e | device against the oracle: max |dh|/h %.3e  final state %.3e" %
              (C.letters(base), [b["newton"] for b in base.log], s_err, s_u, dh, du))
        assert dh <= 10.0 * s_err and du <= 10.0 * s_u
    finally:
        sys_.close()


# ---- off means off, refusals --------------------------------------------------------------------------------------------------------
def test_fixed_step_runs_do_not_see_the_feature(gpu_lib):
    """EDLRun and PoreRun without the option: the states after 3 steps are those of a handle that never saw the new calls, bit for
    bit — and so are those of the same run on a handle whose estimator was allocated and run between the steps."""
    from gmpnp_amd.edl1d import EDLRun
    from gmpnp_amd.pore3d import PoreRun
    for make in (lambda: EDLRun(L_n=1e-6, cation="K", voltage_multiplier=-2.5), lambda: PoreRun(concentration_elec=0.5, L=10e-9, R=5e-9)):
        a, b = make(), make()
        try:
            assert a.stepper is None and b.stepper is None
            for _ in range(3):
                a.step(verbose=False)
                b.step(verbose=False)
                b.sys.time_error(1.0, 1.0, 1e-2, 1e-4)   # b: the estimator's storage exists and its kernels have run
            assert np.array_equal(a.sys.dev.get_state(), b.sys.dev.get_state())
            assert np.array_equal(a.sys.dev.get_state(previous=True), b.sys.dev.get_state(previous=True))
            assert a.newton_its == b.newton_its
        finally:
            a.sys.close()
            b.sys.close()


def test_refusals(gpu_lib, pore10):
    from gmpnp_amd import edl1d, pore3d
    from gmpnp_amd.dist import PartitionedSolver
    from gmpnp_amd.solver import PartitionedSystem
    with pytest.raises(ValueError):
        pore3d.PoreRun(adaptive_dt=True, partition=(2, None), concentration_elec=0.5, L=10e-9, R=5e-9)
    with pytest.raises(ValueError):
        pore3d.main(["--partitions", "2", "--adaptive_dt", "--L", "10e-9", "--concentration_elec", "0.5"])
    with pytest.raises(ValueError):
        edl1d.EDLRun(adaptive_dt=True, H_OHP=0.5, L_n=1e-6)
    with pytest.raises(ValueError):
        edl1d.main(["--adaptive_dt", "--H_OHP", "0.5", "--L_n", "1e-6"])
    ps = PartitionedSolver(pore10[2], 2)
    try:
        lib = ps.devs[0].lib
        tol, out = gpu_lib.CTimeTol(), gpu_lib.CTimeError()
        tol.rtol = 1e-2
        for f in range(9):
            tol.atol[f] = 1e-4
        h = ps.devs[0]._h
        from ctypes import byref
        assert lib.gmpnp_set_time_step(h, 1.0) == gpu_lib.ERR_INVALID
        assert lib.gmpnp_time_error(h, 1.0, 1.0, byref(tol), byref(out)) == gpu_lib.ERR_INVALID
        assert lib.gmpnp_time_accept(h) == gpu_lib.ERR_INVALID
        assert lib.gmpnp_time_reject(h) == gpu_lib.ERR_INVALID
    finally:
        ps.close()
    for name in ("set_time_step", "time_error", "time_accept", "time_reject"):
        with pytest.raises(ValueError):
            getattr(PartitionedSystem, name)(None)


# ---- the driver's command line ------------------------------------------------------------------------------------------------------
def test_driver_command_line(gpu_lib, tmp_path):
    env = dict(os.environ, GMPNP_OUT=str(tmp_path))
    cmd = ["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "1D", "MPNP_CO2ER_EDL.py"), "--L_n=1e-6", "--voltage_multiplier=-2.5",
           "--adaptive_dt", "--steady_tol", "1e-5"]
    subprocess.run(cmd, check=True, env=env, cwd=str(tmp_path), capture_output=True, text=True)
    metas = [os.path.join(d, f) for d, _, fs in os.walk(str(tmp_path)) for f in fs if f == "metadata.json"]
    assert len(metas) == 1
    out = os.path.dirname(metas[0])
    meta = json.load(open(metas[0]))
    for key in ("adaptive_dt", "dt_rtol", "dt_atol", "steps_accepted", "steps_rejected", "newton_failures", "t_reached", "stop_reason", "timestep_log"):
        assert key in meta, key
    assert meta["adaptive_dt"] is True and meta["stop_reason"] in ("steady", "t_end") and meta["steps_accepted"] >= 5
    log = np.load(os.path.join(out, meta["timestep_log"]))
    assert len(log["t"]) == meta["steps_accepted"] + meta["steps_rejected"]
    arr = np.load(os.path.join(out, "arrays_unscaled.npz"))
    assert len(arr["tau"]) == arr["H"].shape[0] == meta["steps_accepted"] + 1 and np.all(np.diff(arr["tau"]) > 0.0)
    assert abs(arr["tau"][-1] - meta["t_reached"]) <= 1e-12 * meta["t_reached"]


# ---- the drivers' own glue in adaptive mode -----------------------------------------------------------------------------------------
BAND_LU = {"nonlinear_solver": "newton", "newton_solver": {"linear_solver": "band_lu", "maximum_iterations": 50, "relative_tolerance": 1.0e-4,
                                                           "absolute_tolerance": 1.0e-4, "relaxation_parameter": 0.9}}


def driver_cases():
    """name -> (factory(**keywords) of the run, reference step of the run): all four drivers; the 3D ones on L_10_R_5 with the direct
    solver (bit-for-bit comparisons need a linear solve whose path does not depend on the preconditioner's reuse policy)."""
    from gmpnp_amd.edl1d import EDLRun
    from gmpnp_amd.pore3d import PoreRun
    from gmpnp_amd.rxndiff1d import RxnDiffRun
    from gmpnp_amd.rxnpore3d import RxnPoreRun
    pore = dict(concentration_elec=0.5, L=10e-9, R=5e-9, solver_parameters=BAND_LU)
    return {"edl": (lambda **kw: EDLRun(L_n=1e-6, cation="K", voltage_multiplier=-2.5, **kw), lambda r: r.ep.dts[0]),
            "rxn_diff": (lambda **kw: RxnDiffRun(**kw), lambda r: r.rp.dt),
            "pore": (lambda **kw: PoreRun(**pore, **kw), lambda r: r.pp.dt),
            "pore_device_glue": (lambda **kw: PoreRun(glue="device", **pore, **kw), lambda r: r.pp.dt),
            "rxn_pore": (lambda **kw: RxnPoreRun(**pore, **kw), lambda r: r.pp.dt)}


@pytest.mark.parametrize("name", ["edl", "rxn_diff", "pore", "pore_device_glue", "rxn_pore"])
def test_adaptive_mode_held_at_the_reference_step_is_the_fixed_step_run(gpu_lib, name):
    """A controller that cannot move (dt_max = the reference step, weights so wide that every step is accepted) runs the driver's
    adaptive glue — set_time_step, the accepted step's glue, time_accept in place of assign_previous — at the fixed-step run's
    steps: u, u_n and the history agree with the fixed-step run bit for bit after 3 steps, u_nm1 is the state before u_n, and the
    clock and the times are the steps'."""
    make, ref_step = driver_cases()[name]
    a, b = make(), make(adaptive_dt=True, dt_rtol=1e6, dt_atol=1e6, max_steps=3)
    try:
        dt = ref_step(a)
        b.stepper.policy.h_max = dt
        for _ in range(3):
            a.step(verbose=False)
        b.run(verbose=False)
        log = b.stepper.log
        assert [r["accepted"] for r in log] == [True] * 3 and [r["h"] for r in log] == [dt] * 3 and b.stepper.stop_reason == "max_steps"
        assert a.newton_its == b.newton_its == [r["newton"] for r in log] and a.n == b.n == 3
        assert np.array_equal(a.sys.dev.get_state(), b.sys.dev.get_state())
        assert np.array_equal(a.sys.dev.get_state(previous=True), b.sys.dev.get_state(previous=True))
        assert len(a.history) == len(b.history) == 4 == len(b.times)
        for ra, rb in zip(a.history, b.history):
            for xa, xb in zip(ra, rb) if isinstance(ra, list) else [(ra, rb)]:
                assert np.array_equal(xa, xb)
        assert b.times == [0.0, dt, dt + dt, dt + dt + dt] and b.t == b.times[-1] == a.t
        # u_nm1 is the state before u_n: the estimator of a further (zero-length-change) step sees the second difference of the last
        # three states; with u = u_n it is -(h/h_prev)(u_n - u_nm1) scaled, i.e. not zero unless u_nm1 == u_n
        e = b.sys.time_error(dt, dt, 1e-2, 1e-4)
        assert e["has_history"] and e["err"] > 0.0
    finally:
        a.sys.close()
        b.sys.close()


def test_adaptive_pore_run(gpu_lib, tmp_path, monkeypatch):
    """PoreRun(adaptive_dt=True) on L_10_R_5 from dt_init = 10 reference steps: the step is rejected and cut, the run's bookkeeping
    holds at every attempt, the logged err of an accepted step is the NumPy estimator's on the history rows (which pins u_nm1 and the
    order of the glue), both glue settings take the same attempts, and the outputs carry the actual times."""
    from gmpnp_amd.pore3d import PoreRun
    monkeypatch.setenv("GMPNP_OUT", str(tmp_path))
    runs = {}
    try:
        for glue in ("host", "device"):
            run = PoreRun(concentration_elec=0.5, L=10e-9, R=5e-9, glue=glue, adaptive_dt=True, max_steps=8, budget=(glue == "host"))
            runs[glue] = run
            run.stepper.h = 10.0 * run.pp.dt
            co2 = []
            while run.stepper.stop_reason is None and len(run.stepper.log) < 8:
                n, t, bc = run.n, run.t, run.co2_bc
                row = run.adaptive_step(verbose=False)
                if row["accepted"]:
                    assert run.n == n + 1 and run.t == t + row["h"] == run.times[-1] and run.co2_bc is not None
                    co2.append(run.co2_bc)
                else:   # the clock, the history and the CO2 Dirichlet value stay
                    assert run.n == n and run.t == t and run.co2_bc == bc
                assert len(run.history) == 1 + run.n == len(run.times)
                if run.budget is not None:
                    assert len(run.budget.tables) == run.n
        host, dev = runs["host"], runs["device"]
        log = host.stepper.log
        print("pore L_10_R_5:", "".join("A" if r["accepted"] else "R" for r in log), [r["newton"] for r in log], ["%.3g" % r["err"] for r in log])
        assert [r["accepted"] for r in log].count(True) >= 2 and [r["accepted"] for r in log].count(False) >= 1
        assert [(r["accepted"], r["newton"]) for r in log] == [(r["accepted"], r["newton"]) for r in dev.stepper.log]
        assert max(abs(r["h"] - q["h"]) / r["h"] for r, q in zip(log, dev.stepper.log)) <= 1e-6   # (BiCGStab to 1e-10 in both)
        assert np.array_equal(host.sys.dev.get_state(previous=True), host.history[-1].ravel())
        # the second accepted step against the estimator on the history rows
        acc = [r for r in log if r["accepted"]]
        free = T.free_mask(host.problem)
        m = T.time_error(host.history[2], host.history[1], host.history[0], acc[1]["h"], acc[0]["h"], 1e-2, 1e-4, free)
        assert abs(acc[1]["err"] - m["err"]) <= 1e-10 * m["err"] and acc[1]["worst_dof"] == m["worst_dof"]
        out = host.write_outputs()
        meta = json.load(open(os.path.join(out, "metadata.json")))
        arr = np.load(os.path.join(out, "arrays_unscaled.npz"))
        assert np.array_equal(arr["tau"], np.array(host.times)) and arr["H"].shape[0] == len(host.times)
        assert meta["steps_accepted"] == host.n and meta["steps_rejected"] == len(log) - host.n and meta["t_reached"] == host.t
        assert len(np.load(os.path.join(out, meta["timestep_log"]))["h"]) == len(log) and "budget" in "".join(os.listdir(out))
    finally:
        for r in runs.values():
            r.sys.close()


def test_pore_driver_command_line(gpu_lib, tmp_path):
    env = dict(os.environ, GMPNP_OUT=str(tmp_path))
    cmd = ["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "3D", "MPNP_CO2ER_pore.py"), "--L=10e-9", "--R=5e-9",
           "--concentration_elec=0.5", "--adaptive_dt", "--max_steps", "5"]
    subprocess.run(cmd, check=True, env=env, cwd=str(tmp_path), capture_output=True, text=True)
    metas = [os.path.join(d, f) for d, _, fs in os.walk(str(tmp_path)) for f in fs if f == "metadata.json"]
    assert len(metas) == 1
    out = os.path.dirname(metas[0])
    meta = json.load(open(metas[0]))
    for key in ("adaptive_dt", "dt_rtol", "dt_atol", "steps_accepted", "steps_rejected", "newton_failures", "t_reached", "stop_reason", "timestep_log"):
        assert key in meta, key
    assert meta["stop_reason"] == "max_steps" and meta["steps_accepted"] + meta["steps_rejected"] == 5 and meta["steps_accepted"] >= 1
    arr = np.load(os.path.join(out, "arrays_unscaled.npz"))
    assert len(arr["tau"]) == arr["H"].shape[0] == meta["steps_accepted"] + 1 and np.all(np.diff(arr["tau"]) > 0.0)
    assert arr["tau"][-1] == meta["t_reached"] and os.path.exists(os.path.join(out, meta["timestep_log"]))


@pytest.mark.parametrize("name", ["rxn_diff", "rxn_pore"])
def test_reaction_diffusion_drivers_adaptive_outputs(gpu_lib, name, tmp_path, monkeypatch):
    """The two reaction-diffusion drivers from dt_init = 10 reference steps: attempts, bookkeeping, outputs, and the flags."""
    from gmpnp_amd import rxndiff1d, rxnpore3d
    monkeypatch.setenv("GMPNP_OUT", str(tmp_path))
    mod = rxndiff1d if name == "rxn_diff" else rxnpore3d
    assert mod.build_parser().parse_args(["--adaptive_dt", "--steady_tol", "1e-5", "--max_steps", "7"]).max_steps == 7
    make, ref_step = driver_cases()[name]
    run = make(adaptive_dt=True, max_steps=6)
    try:
        run.stepper.h = 10.0 * ref_step(run)
        run.run(verbose=False)
        log = run.stepper.log
        print(name, "".join("A" if r["accepted"] else "R" for r in log), [r["newton"] for r in log], ["%.3g" % r["err"] for r in log])
        assert len(log) == 6 and run.stepper.stop_reason == "max_steps" and run.n == run.stepper.accepted >= 1
        assert len(run.history) == 1 + run.n == len(run.times) and np.all(np.diff(run.times) > 0.0) and run.t == run.times[-1]
        assert abs(run.t - sum(r["h"] for r in log if r["accepted"])) <= 1e-12 * run.t
        out = run.write_outputs()
        meta = json.load(open(os.path.join(out, "metadata.json")))
        arr = np.load(os.path.join(out, "arrays_unscaled.npz"))
        tau = arr["tau_array"] if "tau_array" in arr else arr["tau"]
        assert np.array_equal(tau, np.array(run.times)) and arr["H"].shape[0] == len(run.times)
        assert meta["adaptive_dt"] is True and meta["steps_accepted"] == run.n and meta["stop_reason"] == "max_steps"
        assert os.path.exists(os.path.join(out, meta["timestep_log"]))
    finally:
        run.sys.close()
