"""1D ensembles on the GPU (gmpnp_ensemble_*, gmpnp_amd.edl_ensemble, gmpnp_amd.edl_sweep): every member computes what its own
serial EDLRun computes, failures stay with their member, refused configurations are refused before any launch, and the
ensemble's results are visible to the members' own calls at once."""
import json
import os
import time

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

# voltages -1 / -5 / -10, K and Cs, 0.1 and 0.5 M, the H_OHP controller (a set_model every step), PNP.  On the 50 um mesh the
# serial driver fails 0.5 M (at -10 V: step 0, NaN after an inadmissible iterate) and PNP at -5 V (step 36, not converged): those
# members must fail the same way, at the same step.
MEMBERS = [{"voltage_multiplier": -1.0}, {"voltage_multiplier": -5.0, "cation": "Cs"},
           {"voltage_multiplier": -10.0, "concentration_elec": 0.5}, {"voltage_multiplier": -1.0, "concentration_elec": 0.5},
           {"voltage_multiplier": -5.0, "H_OHP": 1.0}, {"voltage_multiplier": -5.0, "model": "PNP"},
           {"voltage_multiplier": -1.0, "model": "PNP"}, {"voltage_multiplier": -10.0, "cation": "Cs"}]


def maxrel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def serial(kw, num_steps):
    from gmpnp_amd.edl1d import EDLRun
    run = EDLRun(num_steps=num_steps, **kw)
    try:
        err = None
        try:
            run.run(verbose=False)
        except RuntimeError as e:
            err = str(e)
        return run.newton_its, run.history[-1].copy(), err, run.n, run.current_H_frac
    finally:
        run.sys.close()


def compare_with_serial(ens, k, num_steps, report, may_fail=False):
    its, last, err, n, hfrac = serial(ens.kwargs[k], num_steps)
    r = ens.runs[k]
    assert may_fail or err is None
    assert ens.errors[k] == err and r.n == n and (err is None or ens.failed_step[k] == n), (k, ens.errors[k], err, r.n, n)
    assert r.newton_its == its, (k, r.newton_its, its)
    dev = maxrel(r.history[-1], last)
    report.append((k, dev, bool(np.array_equal(r.history[-1], last))))
    assert dev <= 1e-12, (k, dev)
    assert r.current_H_frac == pytest.approx(hfrac, rel=1e-12, abs=0.0)


def test_members_match_their_serial_runs(gpu_lib):
    from gmpnp_amd.edl_ensemble import EDLEnsemble
    report = []
    with EDLEnsemble(MEMBERS, num_steps=100) as ens:
        ens.run()
        assert sum(e is None for e in ens.errors) >= 5
        for k in range(len(ens)):
            compare_with_serial(ens, k, 100, report, may_fail=True)
    print("member, max rel deviation, bitwise:", report)


def test_recorded_digits_of_all_five_voltages_in_one_ensemble(gpu_lib):
    from gmpnp_amd.edl_ensemble import EDLEnsemble
    from test_gpu_parity import STERN_OHP
    with open(os.path.join(GOLDEN, "stern_oracle.json")) as fh:
        oracle = {r["voltage_multiplier"]: r["rows"][-1] for r in json.load(fh)["rows"]}
    volts = sorted(STERN_OHP)
    t0 = time.perf_counter()
    with EDLEnsemble([{"voltage_multiplier": v, "dry_run": False} for v in volts], keep_history=False) as ens:
        assert ens.tot_num_steps == 20000
        ens.run()
        wall = time.perf_counter() - t0
        print("staged schedule, 5 voltages in one ensemble: %.1f s (serially about 5 x 13 s)" % wall)
        for k, v in enumerate(volts):
            s, r = ens.ohp_summary(k), ens.runs[k]
            field, eps = STERN_OHP[v]
            assert ens.errors[k] is None
            assert abs(s["field_OHP"] / field - 1.0) < 5e-10, (v, s)
            assert abs(s["eps_rel_OHP"] / eps - 1.0) < 2e-10, (v, s)
            assert int(sum(r.newton_its)) == oracle[v]["newton_total"] and max(r.newton_its[-1000:]) == 2
            assert abs(s["field_OHP"] / oracle[v]["field_OHP"] - 1.0) < 5e-10 and abs(s["eps_rel_OHP"] / oracle[v]["eps_rel_OHP"] - 1.0) < 2e-10


def test_a_failing_member_is_isolated(gpu_lib):
    """BASELINE configs[0] (1 um, Cs, V = -10) fails at step 0 as the serial driver does; its partner goes on unharmed."""
    from gmpnp_amd import backend
    from gmpnp_amd.edl1d import EDLRun
    from gmpnp_amd.edl_ensemble import EDLEnsemble
    bad, good = {"L_n": 1e-6, "cation": "Cs", "voltage_multiplier": -10.0}, {"L_n": 1e-6, "cation": "Cs", "voltage_multiplier": -5.0}
    run = EDLRun(num_steps=1, **bad)
    try:
        with pytest.raises(RuntimeError) as ei:
            run.step(verbose=False)
        want_code = ei.value.code if isinstance(ei.value, backend.GmpnpError) else backend.ERR_NOT_CONVERGED
    finally:
        run.sys.close()
    report = []
    with EDLEnsemble([bad, good], num_steps=5) as ens:
        ens.run()
        assert ens.errors[0] == str(ei.value) and ens.status[0] == want_code and ens.failed_step[0] == 0
        assert ens.runs[0].n == 0 and ens.runs[1].n == 5
        compare_with_serial(ens, 1, 5, report)
    print("member, max rel deviation, bitwise:", report)


def test_edge_sizes_and_refusals(gpu_lib, pore10):
    from gmpnp_amd import backend
    from gmpnp_amd.edl1d import EDLRun
    from gmpnp_amd.edl_ensemble import EDLEnsemble
    report = []
    with EDLEnsemble([{"voltage_multiplier": -5.0}], num_steps=10) as ens:
        ens.run()
        compare_with_serial(ens, 0, 10, report)
    print("member, max rel deviation, bitwise:", report)
    volts = list(np.linspace(-1.0, -12.5, backend.MAX_ENSEMBLE))
    with EDLEnsemble([{"voltage_multiplier": float(v)} for v in volts], num_steps=1) as ens:
        ens.run()
        assert all(e is None for e in ens.errors) and all(r.n == 1 for r in ens.runs)
    a, b = EDLRun(num_steps=1, voltage_multiplier=-5.0), EDLRun(num_steps=1, voltage_multiplier=-5.0, L_n=1e-6)
    p3 = backend.DeviceSolver(pore10[2])
    try:
        u0 = a.sys.dev.get_state()
        for devs in ([a.sys.dev, b.sys.dev], [a.sys.dev, p3]):
            with pytest.raises(backend.GmpnpError) as ei:
                backend.DeviceEnsemble(devs)
            assert ei.value.code == backend.ERR_INVALID
        opts = backend.newton_options(a.solver_parameters, dim=1)
        with backend.DeviceEnsemble([a.sys.dev]) as e:
            kry = backend.newton_options(a.solver_parameters, dim=1)
            kry.linear_solver = backend.LINEAR_TWOLEVEL
            with pytest.raises(backend.GmpnpError) as ei:
                e.newton_solve(kry)
            assert ei.value.code == backend.ERR_INVALID
            a.sys.dev.set_supg(np.ones((a.mesh.num_vertices, 6)), None)
            with pytest.raises(backend.GmpnpError) as ei:
                e.newton_solve(opts)
            assert ei.value.code == backend.ERR_INVALID
            assert np.array_equal(a.sys.dev.get_state(), u0)   # nothing ran
        with pytest.raises(backend.GmpnpError) as ei:
            backend.DeviceEnsemble([a.sys.dev])   # SUPG set before create
        assert ei.value.code == backend.ERR_INVALID
    finally:
        a.sys.close(); b.sys.close(); p3.close()


def test_member_calls_see_the_ensembles_results_at_once(gpu_lib):
    from gmpnp_amd import backend
    from gmpnp_amd.edl1d import EDLRun
    runs = [EDLRun(num_steps=2, voltage_multiplier=v) for v in (-5.0, -10.0)]
    twin = EDLRun(num_steps=2, voltage_multiplier=-10.0)
    try:
        opts = backend.newton_options(runs[0].solver_parameters, dim=1)
        with backend.DeviceEnsemble([r.sys.dev for r in runs]) as ens:
            stats, codes, _ = ens.newton_solve(opts)
            assert codes == [0, 0]
            ens.assign_previous()
            U = ens.get_state()
            for k, r in enumerate(runs):
                assert np.array_equal(r.sys.dev.get_state(previous=True), U[k])   # u_n right after the ensemble call
                assert np.array_equal(r.sys.dev.get_state(), U[k])
            # set_model right after the ensemble call, then one solve of member 1 alone vs a twin handle in the same state
            model = runs[1].model
            model.point_flux[0] *= 1.5
            runs[1].sys.set_model(model)
            twin.sys.dev.set_state(U[1], U[1])
            twin.model.point_flux[0] = model.point_flux[0]
            twin.sys.set_model(twin.model)
            st1 = runs[1].sys.dev.newton_solve(opts)
            st2 = twin.sys.dev.newton_solve(opts)
            assert st1["residuals"] == st2["residuals"]
            assert np.array_equal(runs[1].sys.dev.get_state(), twin.sys.dev.get_state())
            # ... and the next ensemble solve starts from the member's own state
            stats, codes, _ = ens.newton_solve(opts)
            assert codes == [0, 0] and stats[1]["residuals"][0] == pytest.approx(st1["residuals"][-1], rel=1e-12)
    finally:
        for r in runs + [twin]:
            r.sys.close()


def test_sweep_cli_writes_what_the_serial_driver_writes(gpu_lib, tmp_path, monkeypatch):
    import glob
    from gmpnp_amd import edl1d, edl_sweep, stern
    monkeypatch.setenv("GMPNP_OUT", str(tmp_path / "sweep"))
    path = edl_sweep.main(["--voltage_multiplier", "-2.5", "-5", "--cation", "K", "Cs", "--num_steps", "5"])
    summary = json.load(open(path))
    assert summary["members"] == 4 and all(r["converged"] and r["output"] for r in summary["rows"])
    for row in summary["rows"]:
        kw = row["parameters"]
        monkeypatch.setenv("GMPNP_OUT", str(tmp_path / ("serial_%s_%s" % (kw["voltage_multiplier"], kw["cation"]))))
        ref = edl1d.solve_EDL(voltage_multiplier=kw["voltage_multiplier"], cation=kw["cation"], num_steps=5, verbose=False)
        assert os.path.basename(ref) == os.path.basename(row["output"])
        for f in ("arrays_unscaled.npz", "arrays_scaled.npz"):
            a, b = np.load(os.path.join(row["output"], f)), np.load(os.path.join(ref, f))
            assert a.files == b.files
            for key in a.files:
                assert a[key].shape == b[key].shape and (np.array_equal(a[key], b[key]) or maxrel(a[key], b[key]) <= 1e-12), (f, key)
        ma, mb = json.load(open(os.path.join(row["output"], "metadata.json"))), json.load(open(os.path.join(ref, "metadata.json")))
        assert set(ma) == set(mb)
        for key in ma:
            if key == "end_time":
                continue
            if isinstance(mb[key], float):
                assert ma[key] == pytest.approx(mb[key], rel=1e-12, abs=0.0), key
            else:
                assert ma[key] == mb[key], key
        assert row["field_OHP"] == pytest.approx(ma["field_OHP"], rel=1e-15) and row["newton_total"] == ma["newton_iterations"]
    monkeypatch.setenv("GMPNP_OUT", str(tmp_path / "stern"))
    (p,) = stern.main(["--from_run", summary["rows"][0]["output"], "--no_plots"])
    assert glob.glob(os.path.join(p, "*.npz"))
