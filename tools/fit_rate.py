"""Cost of a fit of the electrode kinetics and of the parameter advance, same process, same box.

Round trip: on the 1 um and the 50 um mesh (K+, Stern BDM, the Tafel parameters of the tests, --step_fraction 0.9, adaptive
steps to the steady stop with the end time lifted), with 6 potentials
(-5 ... -10) and 26 (-5 ... -30): the data are the driver's own polarisation curve at the planted parameters, the start is displaced by
(0.7, -0.5, 0.08, -0.06) in (ln i0_CO, ln i0_H2, alpha_CO, alpha_H2); the wall time, the trials and the Newton iterations of
``EDLRun.fit`` with the predictor (``gmpnp_parameter_advance``) and without it, from the same start.  A configuration that fails is
recorded, not hidden.
Advance: the wall time of one ``DeviceSolver.parameter_advance`` call with 1, 5 and 10 columns at tau = 0 and tau = 0.9 (median of
--repeats calls, each after a fresh tangent that is not timed) on a handle with four reactions.  Writes JSON (default
profiles/fit.json).

    python tools/fit_rate.py [--repeats 7] [--meshes 1e-6 50e-6] [--points 6 26] [--out FILE]
"""
import argparse
import dataclasses
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TRUE = dict(i0_CO=0.1, i0_H2=0.02, alpha_CO=0.5, alpha_H2=0.5)
DISPLACEMENT = dict(i0_CO=0.7, i0_H2=-0.5, alpha_CO=0.08, alpha_H2=-0.06)
NAMES = tuple(TRUE)
T_END, MAX_STEPS = 1.0e12, 4000               # scaled time units / attempted steps of the runs to the steady stop


def displaced():
    return {n: TRUE[n] + DISPLACEMENT[n] if n.startswith("alpha") else TRUE[n] * math.exp(DISPLACEMENT[n]) for n in NAMES}


def round_trip(L_n, points):
    from gmpnp_amd.edl1d import EDLRun
    kw = dict(L_n=L_n, cation="K", electrode_voltage=-5.0, kinetics="tafel", adaptive_dt=True, steady_tol=1e-5, step_fraction=0.9,
              t_end=T_END, max_steps=MAX_STEPS)   # to the steady stop, beyond the driver's own end time where the domain needs it
    run = EDLRun(**kw, **TRUE)
    try:
        run.run(verbose=False)
        curve = run.polarisation(-5.0 - (points - 1), -1.0)
    finally:
        run.sys.close()
    out = {"vertices": int(run.mesh.num_vertices), "data_run_stop_reason": run.stepper.stop_reason, "data_run_steps": int(run.n), "points": int(len(curve["electrode_voltage"])), "data_stop_reason": curve["stop_reason"]}
    data = {k: curve[k] for k in ("electrode_voltage", "i_CO", "i_H2")}
    run = EDLRun(**kw, **displaced())
    try:
        run.run(verbose=False)
        dev = run.sys.dev
        u0, stern0, kin0, par0 = dev.get_state(), run.stern, run.kinetics, dict(run.kinetic_par)
        for predictor in (True, False):
            run.stern, run.kinetics, run.kinetic_par = stern0, kin0, dict(par0)
            dev.set_stern(stern0)
            dev.set_kinetics(kin0)
            dev.set_state(u0, u0)
            t0 = time.perf_counter()
            res = run.fit(data, NAMES, predictor=predictor)
            dt = time.perf_counter() - t0
            r = res["result"]
            err = max(abs((v if n.startswith("alpha") else math.log(v)) - (TRUE[n] if n.startswith("alpha") else math.log(TRUE[n])))
                      for n, v in zip(NAMES, res["fitted_values"]))
            out["predictor_on" if predictor else "predictor_off"] = {
                "wall_s": dt, "stop_reason": r["stop_reason"], "trials": r["trials"], "rejected_trials": r["rejected_trials"],
                "newton_iterations": r["newton_iterations"], "newton_iterations_per_trial": [int(h["newton"]) for h in r["history"]],
                "final_cost": r["cost"], "theta_error": err, "condition_number": r["condition_number"]}
    finally:
        run.sys.close()
    return out


def advance(L_n, repeats):
    from gmpnp_amd.edl1d import EDLRun
    from gmpnp_amd.problem import SurfaceKinetics, SurfaceReaction
    run = EDLRun(num_steps=3, L_n=L_n, cation="K", electrode_voltage=-5.0, kinetics="tafel", **TRUE)
    try:
        run.run(verbose=False)
        dev = run.sys.dev
        more = [SurfaceReaction(k=1e-3, alpha=0.3, p_eq=0.0, reactant="OH", nu={"OH": 1e-3}), SurfaceReaction(k=1e-3, alpha=0.7, p_eq=0.0, reactant=None, nu={"H": 1e-3})]
        kin = SurfaceKinetics(list(run.kinetics.reactions) + more, run.kinetics.p_electrode)
        stern = dataclasses.replace(run.stern)
        u = dev.get_state()
        out = {"vertices": int(run.mesh.num_vertices)}
        for cols in ((16,), (16, 17, 32, 33, 48), (0, 16, 17, 18, 19, 32, 33, 34, 35, 48)):
            for tau in (0.0, 0.9):
                times = []
                for _ in range(repeats + 1):
                    dev.set_stern(stern)
                    dev.set_kinetics(kin)
                    dev.set_state(u, None)
                    dev.electrode_tangent(cols)
                    t0 = time.perf_counter()
                    dev.parameter_advance(cols, [1e-3] * len(cols), tau)
                    times.append((time.perf_counter() - t0) * 1e6)
                t = times[1:]   # (the first call of a shape pays for the step limiter's buffers)
                out["advance_us_%d_columns_tau_%g" % (len(cols), tau)] = {"median": statistics.median(t), "min": min(t), "max": max(t)}
        return out
    finally:
        run.sys.close()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--meshes", type=float, nargs="+", default=[1e-6, 50e-6])
    ap.add_argument("--points", type=int, nargs="+", default=[6, 26])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fit.json"))
    a = ap.parse_args(argv)
    from gmpnp_amd import backend
    lib = backend.load_library()
    res = {"build_id": lib.gmpnp_build_id().decode(), "repeats": a.repeats}
    for L_n in a.meshes:
        name = "%gum" % (L_n * 1e6)
        res[name] = {"advance": advance(L_n, a.repeats)}
        print(name, "advance", json.dumps(res[name]["advance"]), flush=True)
        for points in a.points:
            try:
                res[name]["fit_%d_points" % points] = round_trip(L_n, points)
            except Exception as e:   # recorded, not hidden (a HIP error ends the tool: nothing more is started on that device)
                if getattr(e, "code", None) == backend.ERR_HIP:
                    raise
                res[name]["fit_%d_points" % points] = {"error": "%s: %s" % (type(e).__name__, str(e)[:200])}
            print(name, points, json.dumps(res[name]["fit_%d_points" % points]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
