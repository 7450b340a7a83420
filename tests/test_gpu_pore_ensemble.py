"""3D pore ensembles on the GPU (gmpnp_ensemble_* with 3D members, gmpnp_amd.pore_ensemble, ``sweep --ensemble``): every member
computes bit for bit what its own serial PoreRun (created with shared_device=1) computes, a failing member stays alone, a member
whose linear solve leaves the batched path is finished by the serial code, refused configurations are refused before any launch,
and the ensemble's results are visible to the members' own calls at once."""
import copy
import os

import numpy as np
import pytest

from conftest import GOLDEN, box_pore_problem
from golden_cases import EXTRA_PORE

pytestmark = pytest.mark.gpu

P10 = dict(L=10e-9, R=5e-9)
# (the third member differs in current_rough, not in the cation: the 3D driver, like the reference, runs K only; its bulk-solution
# files have no other cation and parameters_pore.yaml no Sechenov constant for Cs, so pore_parameters raises KeyError: SURVEY Q9)
MEMBERS = [dict(P10, concentration_elec=0.5), dict(P10, concentration_elec=1.0), dict(P10, concentration_elec=0.5, current_rough=1000.0),
           dict(P10, concentration_elec=0.5, H2_FE=0.2)]
SHARED = {"shared_device": 1}
_SERIAL = {}


def relerr(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def serial(kw, num_steps, solver_parameters=None):
    """The serial PoreRun of one member on a handle with shared_device=1: per step the Newton count, the Krylov counts of its
    solves, the band-LU count and the state; the error text and the step of a failure.  Computed once per configuration."""
    from gmpnp_amd.pore3d import PoreRun
    key = (tuple(sorted(kw.items())), num_steps, repr(solver_parameters))
    if key not in _SERIAL:
        run = PoreRun(num_steps=num_steps, device_kwargs=dict(SHARED), solver_parameters=solver_parameters, **kw)
        out = {"krylov": [], "direct": [], "error": None}
        try:
            for _ in range(num_steps):
                try:
                    st = run.step(verbose=False)
                except RuntimeError as e:
                    out["error"] = str(e)
                    break
                out["krylov"].append(st["krylov_per_iteration"])
                out["direct"].append(st["direct_solves"])
            out.update(newton_its=list(run.newton_its), states=[h.copy() for h in run.history[1:]], n=run.n, CO2_min=run.CO2_min,
                       krylov_total=run.sys.krylov_iterations)
        finally:
            run.sys.close()
        _SERIAL[key] = out
    return _SERIAL[key]


def run_ensemble(members, num_steps, solver_parameters=None):
    """The same figures from a PoreEnsemble, per member."""
    from gmpnp_amd import backend
    from gmpnp_amd.pore_ensemble import PoreEnsemble
    with PoreEnsemble(members, num_steps=num_steps) as ens:
        if solver_parameters is not None:
            ens.opts = backend.newton_options(solver_parameters, dim=3)
        outs = [{"krylov": [], "direct": []} for _ in members]
        for _ in range(num_steps):
            before = [r.n for r in ens.runs]
            ens.step()
            for k, r in enumerate(ens.runs):
                if r.n > before[k]:
                    outs[k]["krylov"].append(r.sys.last_stats["krylov_per_iteration"])
                    outs[k]["direct"].append(r.sys.last_stats["direct_solves"])
        for k, r in enumerate(ens.runs):
            outs[k].update(newton_its=list(r.newton_its), states=[h.copy() for h in r.history[1:]], n=r.n, CO2_min=r.CO2_min,
                           krylov_total=r.sys.krylov_iterations, error=ens.errors[k], failed_step=ens.failed_step[k])
    return outs


def assert_member_is_serial(got, ref, steps=None):
    steps = ref["n"] if steps is None else steps
    assert got["newton_its"][:steps] == ref["newton_its"][:steps]
    assert got["krylov"][:steps] == ref["krylov"][:steps]
    assert got["direct"][:steps] == ref["direct"][:steps]
    assert len(got["states"]) >= steps and len(ref["states"]) >= steps
    for n in range(steps):
        assert np.array_equal(got["states"][n], ref["states"][n]), "state after step %d differs" % n


@pytest.fixture(scope="module")
def four_members(gpu_lib):
    return run_ensemble(MEMBERS, 5)


def test_members_equal_their_serial_runs(four_members):
    for kw, got in zip(MEMBERS, four_members):
        ref = serial(kw, 5)
        assert ref["error"] is None and got["error"] is None and got["n"] == ref["n"] == 5
        assert_member_is_serial(got, ref)
        assert got["CO2_min"] == ref["CO2_min"] and got["krylov_total"] == ref["krylov_total"]
        assert all(len(k) == n and all(v > 0 for v in k) for k, n in zip(got["krylov"], got["newton_its"]))   # every solve was a Krylov solve


def test_members_reproduce_the_golden_steps(four_members):
    """The tolerance and the Newton counts tests/test_gpu_parity.py applies to the serial run."""
    for k, case, nsteps in ((0, "pore10", 3), (1, "pore10_1M", EXTRA_PORE["pore10_1M"][1])):
        g = np.load(os.path.join(GOLDEN, case + "_steps.npz"))
        got = four_members[k]
        assert got["newton_its"][:nsteps] == list(g["newton_its"][:nsteps])
        for n in range(nsteps):
            assert relerr(got["states"][n].ravel(), g["states"][n]) < 1e-8


def test_a_failing_member_stays_alone(gpu_lib):
    """Members at voltage_multiplier -1, -2.5 and -7.5 with the wall fluxes (as_published=False), three steps.  On the L_10_R_5
    mesh of this suite the serial driver does NOT fail at -2.5 (8 / 6 / 6 Newton iterations on the MI355X; the divergence from the
    zero state that gmpnp_amd.sweep notes is that of the L_50 meshes), so the member that fails is the one at -7.5: its serial
    PoreRun raises at step 0 ("residual became NaN / Inf after an iterate left the admissible set"), and the ensemble freezes it
    there with the same text while the others run on bit for bit."""
    volts = (-1.0, -2.5, -7.5)
    members = [dict(P10, concentration_elec=0.5, voltage_multiplier=v) for v in volts]
    refs = [serial(MEMBERS[0], 5)] + [serial(kw, 3) for kw in members[1:]]
    got = run_ensemble(members, 3)
    for v, g, r in zip(volts, got, refs):
        print(v, "serial:", r["error"], r["n"], r["newton_its"], "ensemble:", g["error"], g["n"], g["newton_its"])
    for g, r in zip(got, refs):
        assert g["error"] == r["error"] and g["n"] == min(r["n"], 3)
        assert r["error"] is None or g["failed_step"] == r["n"]
        assert_member_is_serial(g, r, steps=g["n"])
    assert refs[2]["error"] is not None and "libgmpnp status" in refs[2]["error"] and got[2]["n"] == refs[2]["n"] < 3
    assert [g["n"] for g in got[:2]] == [3, 3]


def test_a_capped_first_pass_is_finished_by_the_serial_step(gpu_lib, four_members):
    """krylov_maximum_iterations between the two members' Krylov counts: the first pass of the member that needs more ends at the
    cap, it leaves the batch, the serial step finishes it (true residual, band LU: direct_solves > 0), the other one never notices."""
    from gmpnp_amd.pore3d import SOLVER_PARAMETERS
    # candidates: the four members and the one at -2.5 V (first solves of 79 ... 82 iterations on the MI355X)
    cands = MEMBERS + [dict(P10, concentration_elec=0.5, voltage_multiplier=-2.5)]
    counts = [serial(kw, 5 if k < 4 else 3)["krylov"][0] for k, kw in enumerate(cands)]
    # the pair with the widest gap between one member's first solve and the other's longest solve of step 0
    gap, hi, lo = max((counts[a][0] - max(counts[b]), a, b) for a in range(5) for b in range(5) if a != b)
    cap = max(counts[lo]) + 1
    print("krylov counts of step 0:", counts, "-> capped member", hi, "other", lo, "cap", cap)
    assert counts[hi][0] > cap, "no pair of members whose Krylov counts leave room for a cap"
    sp = copy.deepcopy(SOLVER_PARAMETERS)
    sp["newton_solver"]["krylov_solver"] = {"maximum_iterations": cap}
    members = [cands[hi], cands[lo]]
    refs = [serial(kw, 1, sp) for kw in members]
    got = run_ensemble(members, 1, sp)
    assert refs[0]["error"] is None and refs[0]["direct"][0] > 0 and refs[1]["direct"][0] == 0
    for g, r in zip(got, refs):
        assert g["error"] is None
        assert_member_is_serial(g, r)
    assert_member_is_serial(got[1], serial(members[1], 5 if lo < 4 else 3), steps=1)   # ... and the cap did not touch the other member


def _box_twins(gpu_lib, nx, nz, nmem):
    """`nmem` pairs of handles of the box pore with different wall potentials: (ensemble members, serial twins)."""
    pp, mesh, prob = box_pore_problem(nx=nx, nz=nz)
    nv = prob.coords.shape[0]
    u0, un = np.zeros(prob.ndof), np.tile(np.r_[np.ones(8), 0.0], nv)
    devs = []
    for k in range(2 * nmem):
        d = gpu_lib.DeviceSolver(prob, shared_device=1)
        vals = prob.bc_vals.copy()
        wall = (prob.bc_dofs % 9 == 8) & (vals != 0.0)
        vals[wall] *= 1.0 - 0.1 * (k % nmem)
        d.set_dirichlet(prob.bc_dofs, vals)
        d.set_state(u0, un)
        devs.append(d)
    return devs[:nmem], devs[nmem:]


def _stats_equal(a, b):
    return {k: v for k, v in a.items() if not k.startswith("ms_")} == {k: v for k, v in b.items() if not k.startswith("ms_")}


@pytest.mark.parametrize("nx,nz,nmem", [(4, 12, 1), (2, 3, 3), (4, 12, 3)])
def test_edge_sizes_equal_serial(gpu_lib, nx, nz, nmem):
    """One member, and the smallest shapes with a partly filled last tile and last aggregate chunk: two time steps each."""
    from gmpnp_amd.pore3d import SOLVER_PARAMETERS
    opts = gpu_lib.newton_options(SOLVER_PARAMETERS, dim=3)
    mem, twins = _box_twins(gpu_lib, nx, nz, nmem)
    try:
        with gpu_lib.DeviceEnsemble(mem) as ens:
            for _ in range(2):
                stats, codes, msgs = ens.newton_solve(opts)
                assert codes == [0] * nmem, msgs
                ens.assign_previous()
                U = ens.get_state()
                for k, t in enumerate(twins):
                    st = t.newton_solve(opts)
                    t.assign_previous()
                    assert _stats_equal(stats[k], st), (k, stats[k], st)
                    assert st["krylov_iterations"] > 0 and np.array_equal(U[k], t.get_state())
    finally:
        for d in mem + twins:
            d.close()


def test_refused_configurations_run_nothing(gpu_lib, pore10, edl1):
    from gmpnp_amd import dist
    from gmpnp_amd.pore3d import SOLVER_PARAMETERS
    from gmpnp_amd.problem import pore_hierarchy
    from gmpnp_amd.solver import GMPNPSystem
    pp, mesh, prob, _ = pore10
    opts = gpu_lib.newton_options(SOLVER_PARAMETERS, dim=3)
    box = box_pore_problem(nx=2, nz=3)[2]
    dom, perm, part = dist.partition_plan(prob, 2, 0)
    levels = pore_hierarchy(pp, mesh, 1)
    ok = gpu_lib.DeviceSolver(prob, shared_device=1)
    own_streams = gpu_lib.DeviceSolver(prob)
    partitioned = gpu_lib.DeviceSolver(dom.problem, perm=perm, partition=part)
    multilevel = GMPNPSystem(levels[0][0], levels=levels, shared_device=1)
    other_mesh = gpu_lib.DeviceSolver(box, shared_device=1)
    one_d = gpu_lib.DeviceSolver(edl1[2])
    try:
        u0 = ok.get_state()
        for devs, why in (([ok, own_streams], "shared_device"), ([ok, partitioned], "partitioned"), ([multilevel.dev], "coarse level"),
                          ([ok, other_mesh], "topology differs"), ([one_d, ok], "1D and 3D"), ([ok, one_d], "1D and 3D")):
            with pytest.raises(gpu_lib.GmpnpError, match=why) as ei:
                gpu_lib.DeviceEnsemble(devs)
            assert ei.value.code == gpu_lib.ERR_INVALID
        with gpu_lib.DeviceEnsemble([ok]) as ens:
            for solver in (gpu_lib.LINEAR_BAND_LU, gpu_lib.LINEAR_BLOCK_TRIDIAGONAL):
                bad = gpu_lib.newton_options(SOLVER_PARAMETERS, dim=3)
                bad.linear_solver = solver
                with pytest.raises(gpu_lib.GmpnpError) as ei:
                    ens.newton_solve(bad)
                assert ei.value.code == gpu_lib.ERR_INVALID
            assert np.array_equal(ok.get_state(), u0)   # nothing ran
            stats, codes, _ = ens.newton_solve(opts)    # ... and the ensemble is still good
            assert codes == [0] and stats[0]["converged"]
    finally:
        for d in (ok, own_streams, partitioned, other_mesh, one_d):
            d.close()
        multilevel.close()


def test_member_calls_see_the_ensembles_results_at_once(gpu_lib):
    from gmpnp_amd import backend
    from gmpnp_amd.pore3d import SOLVER_PARAMETERS, PoreRun
    runs = [PoreRun(num_steps=2, device_kwargs=dict(SHARED), **kw) for kw in MEMBERS[:2]]
    twin = PoreRun(num_steps=2, device_kwargs=dict(SHARED), **MEMBERS[1])
    try:
        opts = backend.newton_options(SOLVER_PARAMETERS, dim=3)
        with backend.DeviceEnsemble([r.sys.dev for r in runs]) as ens:
            stats, codes, _ = ens.newton_solve(opts)
            assert codes == [0, 0]
            ens.assign_previous()
            U = ens.get_state()
            for k, r in enumerate(runs):
                assert np.array_equal(r.sys.dev.get_state(previous=True), U[k])   # u_n right after the ensemble call
                assert np.array_equal(r.sys.dev.get_state(), U[k])
            # one solve of member 1 alone (the second time step) vs a twin handle in the same state: the same state vector AND the
            # same solver history (coarse reuse, predicted starts), so the twin takes the first step serially
            twin.sys.dev.newton_solve(opts)
            twin.sys.dev.assign_previous()
            assert np.array_equal(twin.sys.dev.get_state(), U[1])
            st1 = runs[1].sys.dev.newton_solve(opts)
            st2 = twin.sys.dev.newton_solve(opts)
            assert st1["residuals"] == st2["residuals"] and st1["krylov_per_iteration"] == st2["krylov_per_iteration"]
            assert st1["iterations"] > 0 and np.array_equal(runs[1].sys.dev.get_state(), twin.sys.dev.get_state())
            # ... and the next ensemble solve starts from the member's own state
            stats, codes, _ = ens.newton_solve(opts)
            assert codes == [0, 0] and stats[1]["residuals"][0] == pytest.approx(st1["residuals"][-1], rel=1e-12)
    finally:
        for r in runs + [twin]:
            r.sys.close()


def test_sweep_groups_give_what_the_serial_jobs_give(gpu_lib):
    """``sweep --ensemble`` on the L_10_R_5 mesh (the L_50 meshes take too long to read for a test): the jobs of a rank through the
    grouping function, each group as one PoreEnsemble, against run_job with shared_device=1."""
    from gmpnp_amd import sweep
    mine = sweep.jobs([5], [-1.0, -2.5])
    res = [None] * len(mine)
    for radius, idx in sweep.group_by_radius(mine):
        outs = sweep.run_group(radius, [mine[k][1] for k in idx], 2, as_published=True, L=10e-9)
        for k, out in zip(idx, outs):
            res[k] = out
    for job, out in zip(mine, res):
        ref = sweep.run_job(job[0], job[1], 2, as_published=True, L=10e-9, device_kwargs=dict(SHARED))
        assert set(out) == set(ref)
        for key in ("R_nm", "voltage_multiplier", "status", "steps_done", "newton_iterations", "krylov_iterations", "CO2_min", "n_dofs"):
            assert out[key] == ref[key], (job, key, out[key], ref[key])
        assert out["status"] == "ok" and out["newton_iterations"] > 0
