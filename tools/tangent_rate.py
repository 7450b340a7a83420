"""Cost of the electrode tangent and of a polarisation curve, same process, same box.

Hooks: gmpnp_time_kernel(28), the multi-column cyclic-reduction chain of the last gmpnp_electrode_tangent (extraction and application
included), for 1, 2 and 8 columns (one M = 2 chain, one M = 2 chain, one full M = 8 chain on a handle with four reactions) against hook 18, one whole one-column solve, on
the 1 um and the 50 um mesh (K+, Stern BDM, the Tafel parameters of the tests, the state after `--steps` driver steps): the median of
`--repeats` measurements of `--launches` chains each, with the smallest and the largest.  `--hook18-only` measures hook 18 alone: run from a checkout of
the commit before the tangent (this file copied into its tools/) with `--out profiles/tangent_parent_hook18.json`, it gives the
one-column solve the chain is compared with.
Curve: the wall time and the Newton iterations of the 26-point curve p_M = -5 ... -30 on the 1 um mesh by continuation from the steady
state at -5, against the same potentials as 26 separate runs with --adaptive_dt --steady_tol 1e-5 (all runs with --step_fraction 0.9; a separate
run that fails is recorded, not hidden).  Writes JSON (default
profiles/tangent.json).

    python tools/tangent_rate.py [--launches 50] [--repeats 3] [--steps 3] [--no-curve] [--hook18-only] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TAFEL = dict(kinetics="tafel", i0_CO=0.1, i0_H2=0.02)


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def hooks(L_n, steps, launches, repeats, hook18_only):
    from gmpnp_amd.edl1d import EDLRun
    run = EDLRun(num_steps=steps, L_n=L_n, cation="K", electrode_voltage=-5.0, **TAFEL)
    try:
        run.run(verbose=False)
        dev = run.sys.dev
        dev.assemble(True)
        out = {"vertices": int(run.mesh.num_vertices), "hook18_us": spread([dev.time_kernel(18, launches) for _ in range(repeats)])}
        if not hook18_only:
            # four reactions on the handle (two more beside the run's Tafel pair), so that eight distinct columns exist
            from gmpnp_amd.problem import SurfaceKinetics, SurfaceReaction
            more = [SurfaceReaction(k=1e-3, alpha=0.3, p_eq=0.0, reactant="OH", nu={"OH": 1e-3}), SurfaceReaction(k=1e-3, alpha=0.7, p_eq=0.0, reactant=None, nu={"H": 1e-3})]
            dev.set_kinetics(SurfaceKinetics(list(run.kinetics.reactions) + more, run.kinetics.p_electrode))
            for cols in ((0,), (0, 48), (0, 16, 17, 18, 19, 32, 33, 48)):
                dev.electrode_tangent(cols)
                out["hook28_us_%d_columns" % len(cols)] = spread([dev.time_kernel(28, launches) for _ in range(repeats)])
        return out
    finally:
        run.sys.close()


def curve(v_end, v_step):
    from gmpnp_amd.edl1d import EDLRun
    kw = dict(L_n=1e-6, cation="K", adaptive_dt=True, steady_tol=1e-5, step_fraction=0.9, **TAFEL)
    run = EDLRun(electrode_voltage=-5.0, **kw)
    try:
        t0 = time.perf_counter()
        run.run(verbose=False)
        t_first = time.perf_counter() - t0
        first_newton = int(sum(run.newton_its))
        t0 = time.perf_counter()
        out = run.polarisation(v_end, v_step)
        t_curve = time.perf_counter() - t0
    finally:
        run.sys.close()
    n = len(out["electrode_voltage"])
    separate_s, separate_newton, separate_failed = 0.0, 0, []
    for p in out["electrode_voltage"]:
        one = EDLRun(electrode_voltage=float(p), **kw)
        try:
            t0 = time.perf_counter()
            try:
                one.run(verbose=False)
            except Exception as e:   # a transient run from the bulk state may fail where the continuation does not
                separate_failed.append({"electrode_voltage": float(p), "error": str(e)[:120]})
            separate_s += time.perf_counter() - t0
            separate_newton += int(sum(one.newton_its))
        finally:
            one.sys.close()
    return {"points": n, "stop_reason": out["stop_reason"], "first_point_run_s": t_first, "first_point_run_newton": first_newton,
            "curve_s": t_curve, "curve_newton": int(out["newton_iterations"].sum()), "curve_substeps": int(out["substeps"].sum()),
            "separate_runs_s": separate_s, "separate_runs_newton": separate_newton, "separate_runs_failed": separate_failed, "i_CO_last": float(out["i_CO"][-1]),
            "worst_tangent_residual": float(out["tangent_residual"].max())}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--no-curve", action="store_true")
    ap.add_argument("--hook18-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tangent.json"))
    a = ap.parse_args(argv)
    from gmpnp_amd import backend
    lib = backend.load_library()
    res = {"build_id": lib.gmpnp_build_id().decode(), "launches": a.launches, "repeats": a.repeats,
           "1um": hooks(1e-6, a.steps, a.launches, a.repeats, a.hook18_only), "50um": hooks(50e-6, a.steps, a.launches, a.repeats, a.hook18_only)}
    if not a.no_curve and not a.hook18_only:
        res["curve_1um_-5_to_-30"] = curve(-30.0, -1.0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
