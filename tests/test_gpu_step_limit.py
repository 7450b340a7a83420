"""The fraction-to-boundary step limiter on the GPU (gmpnp_newton_options_t.step_fraction, csrc/gmpnp_step_limit.h): the kernels
against the NumPy rule of tests/step_limit_reference.py, the Newton drivers against the reference loop over the oracle's assembly,
the cases where the limiter never engages against the same solve without it, 1D ensembles against their members' serial runs, the
refusals, and the driver's command line.  Meshes: the 1 um interval mesh (1,091 vertices) and L_10_R_5 (1,767 vertices): neither
is a multiple of the wave or the workgroup, both need several workgroups."""
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import step_limit_reference as R
from conftest import ROOT, _edl

pytestmark = pytest.mark.gpu

TAU = 0.9
HARD = [("Cs", -10.0), ("Cs", -12.5), ("K", -10.0), ("Li", -10.0)]
MUMPS_09 = {"nonlinear_solver": "newton", "newton_solver": {
    "linear_solver": "mumps", "maximum_iterations": 50, "relative_tolerance": 1e-4, "absolute_tolerance": 1e-4, "relaxation_parameter": 0.9}}


def maxrel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def rel(x, y):
    return abs(x - y) / abs(y)


def species_a(prob):
    return np.asarray(prob.model.a, dtype=np.float64)[:prob.nf - 1]


def background(prob, seed):
    """Random (u, dx) whose every vertex is a candidate with a ratio in [2, 10]: S in (0.1, 0.9), dS < 0."""
    rng = np.random.default_rng(seed)
    nv, nf = prob.coords.shape[0], prob.nf
    a = species_a(prob)
    u = np.concatenate([rng.uniform(0.5, 1.5, (nv, nf - 1)), rng.uniform(-1.0, 0.0, (nv, 1))], axis=1)
    u[:, :nf - 1] *= (rng.uniform(0.1, 0.9, nv) / R.steric_sum(a, u))[:, None]
    dx = np.concatenate([rng.uniform(0.5, 1.5, (nv, nf - 1)), rng.normal(size=(nv, 1))], axis=1)
    want = (1.0 - R.steric_sum(a, u)) / rng.uniform(2.0, 10.0, nv)
    dx[:, :nf - 1] *= (-want / R.steric_sum(a, dx))[:, None]
    return u, dx


def check(dev, prob, u, dx, expect_node=None):
    a = species_a(prob)
    alpha, lam, node = dev.step_limit(dx, TAU)
    ra, rl, rn = R.step_limit(a, u, dx, TAU)
    assert node == rn, (node, rn, lam, rl)
    if expect_node is not None:
        assert node == expect_node
    if np.isinf(rl):
        assert np.isinf(lam) and lam > 0 and alpha == 1.0 == ra
    else:
        assert rel(lam, rl) <= 1e-14 and rel(alpha, ra) <= 1e-14, (lam, rl, alpha, ra)
    return alpha, lam, node


@pytest.mark.parametrize("which", ["interval", "pore"])
def test_kernels_against_the_numpy_rule(gpu_lib, pore10, which):
    prob = _edl(L_n=1e-6, cation="Cs", voltage_multiplier=-10.0)[2] if which == "interval" else pore10[2]
    nv, nf = prob.coords.shape[0], prob.nf
    assert nv in (1091, 1767) and nv % 64 and nv % 256
    a = species_a(prob)
    u, dx = background(prob, seed=11)
    un = np.random.default_rng(5).uniform(0.5, 1.5, prob.ndof)
    with gpu_lib.DeviceSolver(prob) as dev:
        dev.set_state(u.ravel(), un)
        # a plain random case: some vertex limits the step above 1 (alpha = 1, lambda finite) ...
        alpha, lam, node = check(dev, prob, u, dx)
        assert alpha == 1.0 and 2.0 <= lam <= 10.0
        # ... and below 1 after scaling the correction
        alpha, lam, node = check(dev, prob, u, 16.0 * dx)
        assert lam < 1.0 and alpha == TAU * lam
        # the limiting vertex at EVERY vertex in turn (every lane of every workgroup, the tail workgroup, vertex 0, the first and
        # the last vertex of the internal order whatever that order is)
        for v in range(nv):
            d = dx.copy()
            d[v, :nf - 1] *= 2.0 * lam_at(a, u, dx, v)   # ratio 0.5 at v, [2, 10] elsewhere
            al, lm, nd = check(dev, prob, u, d, expect_node=v)
            assert lm < 1.0 and al == TAU * lm
        for v in (int(dev.perm[0]), int(dev.perm[-1]), 0, nv - 1):
            d = dx.copy()
            d[v, :nf - 1] *= 2.0 * lam_at(a, u, dx, v)
            assert dev.step_limit(d, TAU) == dev.step_limit(d, TAU)   # two calls: the same bits
            check(dev, prob, u, d, expect_node=v)
        # inadmissible vertices (S >= 1) with a steep decrease are skipped
        rng = np.random.default_rng(3)
        bad = rng.choice(nv, 40, replace=False)
        ub, db = u.copy(), dx.copy()
        ub[bad, :nf - 1] *= (rng.uniform(1.0, 3.0, 40) / R.steric_sum(a, ub[bad]))[:, None]
        db[bad, :nf - 1] *= 1e6
        dev.set_state(ub.ravel(), None)
        alpha, lam, node = check(dev, prob, ub, db)
        assert node not in set(bad.tolist()) and lam >= 2.0
        dev.set_state(u.ravel(), None)
        # no limiting vertex: S does not grow anywhere
        dn = dx.copy()
        dn[:, :nf - 1] = np.abs(dn[:, :nf - 1])
        assert check(dev, prob, u, dn) == (1.0, np.inf, -1)
        # a NaN / Inf anywhere in dx (the potential's entry too) is reported, not ignored
        for v, f, val in ((0, 0, np.nan), (nv - 1, nf - 1, np.nan), (nv // 2, 1, np.inf), (int(dev.perm[-1]), nf - 1, -np.inf)):
            d = dx.copy()
            d[v, f] = val
            with pytest.raises(gpu_lib.GmpnpError) as ei:
                dev.step_limit(d, TAU)
            assert ei.value.code == gpu_lib.ERR_NUMERIC and "NaN / Inf" in str(ei.value)
        for tau in (0.0, 1.0, -0.5, float("nan")):
            with pytest.raises(gpu_lib.GmpnpError) as ei:
                dev.step_limit(dx, tau)
            assert ei.value.code == gpu_lib.ERR_INVALID and "step_fraction" in str(ei.value)
        check(dev, prob, u, dx)   # ... and the handle still answers
        # nothing on the handle moved
        assert np.array_equal(dev.get_state(), u.ravel()) and np.array_equal(dev.get_state(previous=True), un)
        us = dev.time_kernel(21, 20)
        assert us > 0.0 and np.array_equal(dev.get_state(), u.ravel())
        print("%s: k_step_limit + k_limited_update %.2f us" % (which, us))


def lam_at(a, u, dx, v):
    """ratio (1 - S) / (-dS) of vertex v"""
    return float((1.0 - R.steric_sum(a, u[v:v + 1])[0]) / -R.steric_sum(a, dx[v:v + 1])[0])


def reference_first_solve(prob):
    u0, un = R.first_step_state(prob)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return R.newton_loop(prob, u0, un, tau=TAU, relative_tolerance=1e-4, absolute_tolerance=1e-4)   # the 1D driver's tolerances


def limited_step(gpu_lib, **kw):
    from gmpnp_amd.edl1d import EDLRun
    run = EDLRun(num_steps=1, L_n=1e-6, step_fraction=TAU, **kw)
    try:
        st = run.step(verbose=False)
        return st, run.history[-1].copy(), run.problem
    finally:
        run.sys.close()


def test_config0_converges_with_the_limiter(gpu_lib):
    """BASELINE configs[0] (1 um mesh, Cs, V = -10), first time step: diverges without the option
    (test_gpu_parity.py::test_config0_diverges_on_the_gpu_as_in_the_oracle), converges with it, along the reference loop's path."""
    st, vals, prob = limited_step(gpu_lib, cation="Cs", voltage_multiplier=-10.0)
    u_ref, ref = reference_first_solve(prob)
    print("gpu", st["iterations"], st["step_factor"], st["residuals"], "reference", ref.iterations, ref.step_factor, ref.residuals,
          "state", maxrel(vals.ravel(), u_ref))
    assert ref.converged and st["converged"] and st["iterations"] == ref.iterations == 10
    assert np.allclose(st["step_factor"], ref.step_factor, rtol=1e-6, atol=0.0)
    assert st["limited_steps"] == ref.limited_steps == 2 and rel(st["min_step"], ref.min_step) <= 1e-6
    assert st["steric_excursion"] == 0
    assert maxrel(vals.ravel(), u_ref) <= 1e-8


def test_potassium_ends_inside_the_admissible_set(gpu_lib):
    """K, V = -10: plain Newton leaves the admissible set (the oracle "converges" to max S = 1.62, min u = -0.65); with the limiter the
    step ends with max S < 1 and every species above -1e-4 (twice the reference loop's own overshoot of -5e-5)."""
    from gmpnp_amd.edl1d import EDLRun
    run = EDLRun(num_steps=1, L_n=1e-6, cation="K", voltage_multiplier=-10.0)
    try:
        plain = run.step(verbose=False)   # today's end: "converged" through iterates outside the admissible set, and says so
        print("plain:", plain["iterations"], plain["steric_excursion"], plain["limited_steps"])
        assert plain["converged"] and plain["steric_excursion"] == 1 and plain["limited_steps"] == 0
    finally:
        run.sys.close()
    st, vals, prob = limited_step(gpu_lib, cation="K", voltage_multiplier=-10.0)
    S = R.steric_sum(species_a(prob), vals)
    print("limited:", st["iterations"], st["step_factor"], "max S", S.max(), "min species", vals[:, :6].min())
    assert st["converged"] and st["steric_excursion"] == 0 and st["limited_steps"] >= 1
    assert S.max() < 1.0 and vals[:, :6].min() >= -1e-4


def one_solve(gpu_lib, prob, params, tau, **device_kwargs):
    u0, un = R.first_step_state(prob)
    opts = gpu_lib.newton_options(gpu_lib.with_step_fraction(params, tau), dim=prob.coords.shape[1])
    with gpu_lib.DeviceSolver(prob, **device_kwargs) as dev:
        dev.set_state(u0, un)
        st = dev.newton_solve(opts)
        return st, dev.get_state()


def test_option_on_where_it_never_engages_1d(gpu_lib, edl1):
    from gmpnp_amd.edl1d import SOLVER_PARAMETERS
    off, u_off = one_solve(gpu_lib, edl1[2], SOLVER_PARAMETERS, 0.0)
    on, u_on = one_solve(gpu_lib, edl1[2], SOLVER_PARAMETERS, TAU)
    print("edl1", off["iterations"], on["iterations"], maxrel(u_on, u_off), np.array_equal(u_on, u_off))
    assert on["iterations"] == off["iterations"] and on["limited_steps"] == 0 and on["min_step"] == 1.0
    assert on["step_factor"] == [1.0] * on["iterations"] and off["step_factor"] == [0.0] * off["iterations"] and off["min_step"] == 1.0
    assert maxrel(u_on, u_off) <= 1e-12


@pytest.mark.parametrize("solver", ["two_level", "jacobi", "band_lu"])
def test_option_on_where_it_never_engages_3d(gpu_lib, pore10, solver):
    """The zero start of the limited solve's linear solves changes the Krylov iterates, not the Newton path."""
    params = {"nonlinear_solver": "newton", "newton_solver": dict(MUMPS_09["newton_solver"])}
    if solver == "jacobi":
        # The two solves start their BiCGStab passes differently, so their corrections differ by the linear solves' ERROR, which is
        # cond(J) times the residual tolerance: at 1e-10 the states differed by 2.0e-7.  Comparing the Newton paths at 1e-8 needs the
        # corrections to ~1e-5 of that, hence 1e-13 here (node-block Jacobi alone leaves the conditioning to BiCGStab).
        params["newton_solver"].update(linear_solver="bicgstab", preconditioner="jacobi", krylov_solver={"relative_tolerance": 1e-13})
    elif solver == "band_lu":
        params["newton_solver"]["linear_solver"] = "band_lu"
    off, u_off = one_solve(gpu_lib, pore10[2], params, 0.0)
    on, u_on = one_solve(gpu_lib, pore10[2], params, TAU)
    print(solver, off["iterations"], on["iterations"], off["krylov_iterations"], on["krylov_iterations"], maxrel(u_on, u_off))
    assert on["converged"] and on["iterations"] == off["iterations"] and on["limited_steps"] == 0
    assert on["step_factor"] == [1.0] * on["iterations"]
    if solver == "band_lu":
        assert on["direct_solves"] == on["iterations"] == off["direct_solves"]
    assert maxrel(u_on, u_off) <= 1e-8


def test_1d_ensemble_members_match_their_serial_runs(gpu_lib):
    from gmpnp_amd.edl_ensemble import EDLEnsemble
    members = [{"L_n": 1e-6, "cation": c, "voltage_multiplier": v} for c, v in HARD + [("Cs", -5.0)]]
    with EDLEnsemble(members, num_steps=1, step_fraction=TAU) as ens:
        ens.run()
        assert ens.errors == [None] * len(members)
        got = [(r.sys.last_stats, r.history[-1].copy()) for r in ens.runs]
    for k, kw in enumerate(members):
        st, vals, _ = limited_step(gpu_lib, **{f: v for f, v in kw.items() if f != "L_n"})
        g, gv = got[k]
        print(k, kw, g["iterations"], g["step_factor"], maxrel(gv, vals), np.array_equal(gv, vals))
        assert g["iterations"] == st["iterations"] and g["limited_steps"] == st["limited_steps"]
        assert np.allclose(g["step_factor"], st["step_factor"], rtol=1e-12, atol=0.0) and rel(g["min_step"], st["min_step"]) <= 1e-12
        assert maxrel(gv, vals) <= 1e-12 and g["steric_excursion"] == 0
    assert got[-1][0]["limited_steps"] == 0 and got[-1][0]["min_step"] == 1.0
    assert all(g["limited_steps"] >= 1 for g, _ in got[:-1])


def test_3d_ensembles_and_groups_refuse_the_option(gpu_lib, pore10):
    from gmpnp_amd import dist
    prob = pore10[2]
    u0, un = R.first_step_state(prob)
    on, off = gpu_lib.newton_options(gpu_lib.with_step_fraction(MUMPS_09, TAU)), gpu_lib.newton_options(MUMPS_09)
    devs = [gpu_lib.DeviceSolver(prob, shared_device=1) for _ in range(2)]
    try:
        for d in devs:
            d.set_state(u0, un)
        with gpu_lib.DeviceEnsemble(devs) as ens:
            with pytest.raises(gpu_lib.GmpnpError) as ei:
                ens.newton_solve(on)
            assert ei.value.code == gpu_lib.ERR_INVALID and "step_fraction" in str(ei.value)
            assert np.array_equal(devs[0].get_state(), u0)   # nothing ran
            stats, codes, _ = ens.newton_solve(off)
            assert codes == [0, 0] and all(s["converged"] for s in stats)
    finally:
        for d in devs:
            d.close()
    with dist.PartitionedSolver(prob, 1) as ps:
        ps.set_state(u0, un)
        with pytest.raises(gpu_lib.GmpnpError) as ei:
            ps.newton_solve(on)
        assert ei.value.code == gpu_lib.ERR_INVALID and "step_fraction" in str(ei.value)
        assert ps.newton_solve(off)["converged"]
    # the option's range is checked by every entry point
    bad = gpu_lib.newton_options(MUMPS_09)
    bad.step_fraction = 1.5
    with gpu_lib.DeviceSolver(prob) as dev:
        with pytest.raises(gpu_lib.GmpnpError) as ei:
            dev.newton_solve(bad)
        assert ei.value.code == gpu_lib.ERR_INVALID and "step_fraction" in str(ei.value)


def test_driver_command_line(gpu_lib, tmp_path):
    """1D/MPNP_CO2ER_EDL.py --voltage_multiplier=-10.0 --cation=Cs on the 1 um mesh, one step: the reference's output files, and the
    key in metadata.json."""
    env = dict(os.environ, GMPNP_OUT=str(tmp_path))
    cmd = [sys.executable, os.path.join(ROOT, "1D", "MPNP_CO2ER_EDL.py"), "--voltage_multiplier=-10.0", "--cation=Cs", "--L_n=1e-6",
           "--num_steps=1", "--step_fraction", "0.9"]
    subprocess.run(cmd, check=True, env=env, cwd=str(tmp_path), stdout=subprocess.DEVNULL)
    found = [d for d, _, files in os.walk(str(tmp_path)) if "metadata.json" in files]
    assert len(found) == 1
    assert {"arrays_unscaled.npz", "arrays_scaled.npz", "metadata.json"} <= set(os.listdir(found[0]))
    meta = json.load(open(os.path.join(found[0], "metadata.json")))
    assert meta["step_fraction"] == 0.9 and meta["cation"] == "Cs" and meta["num_steps_run"] == 1 and meta["newton_iterations"] == 10
    z = np.load(os.path.join(found[0], "arrays_unscaled.npz"))
    assert z["cat"].shape == (2, 1091) and np.all(np.isfinite(z["p"]))
