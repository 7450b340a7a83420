"""Cycles and wall time to the limit cycle of a pulse train: plain marching against the accelerated cycle map,
same process, same box.

K+ with a BDM Stern layer and the Tafel parameters of the tests, on the 1 um mesh and on the 50 um mesh: adaptive steps to the steady
stop at p_M = -5, then from that state, each time, the pulse -5.5 / -4.5 with holds of ``--holds`` (scaled time) in 4 fixed steps per
segment

    plain      ``EDLRun.programme`` over ``--cap`` cycles; the residual of cycle k is the weighted RMS of x_{k+1} - x_k over the free dofs
               with the weights of the steady state (rtol 1e-2, atol 1e-4), from the states the programme keeps at the period ends.
               The whole march is timed once: the time to the tolerance is that time x cycles to the tolerance / cap, a pro-rata
               figure (every cycle takes the same 8 solves), and the contraction is the ratio of the last two residuals at the
               crossing (at the cap where the tolerance is not reached: far below it the ratio is rounding noise)
    depth d    ``EDLRun.programme(periodic=dict(depth=d, max_cycles=cap, tol=...))`` for d = 2, 4, 8

and records the cycles and the wall time to the residual ``--tol`` (None where the cap is reached first), the residual histories, and
hook 33 (``gmpnp_time_kernel``: residual + reduce + mix on a full window of depth 4).  Writes JSON (default profiles/periodic.json).

    python tools/periodic_rate.py [--meshes 1um 50um] [--cap 300] [--tol 1e-3] [--holds 30 20] [--out FILE]
"""
import argparse
import dataclasses
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(cation="K", electrode_voltage=-5.0, kinetics="tafel", i0_CO=0.1, i0_H2=0.02, adaptive_dt=True, steady_tol=1e-5)
L_N = {"1um": 1e-6, "50um": 50e-6}
RTOL, ATOL, STEPS = 1e-2, 1e-4, 4


def stand_at(run, u, p):
    """The run back at the state ``u`` and the potential ``p``."""
    run.sys.set_state(u, u)
    run.sys.dev.set_electrode_potential(p)
    run.stern = dataclasses.replace(run.stern, p_electrode=p)
    run.problem.stern = run.stern
    run.kinetics = dataclasses.replace(run.kinetics, p_electrode=p)
    run.problem.kinetics = run.kinetics


def measure(name, a):
    from gmpnp_amd.edl1d import EDLRun
    run = EDLRun(L_n=L_N[name], **KW)
    try:
        t0 = time.perf_counter()
        run.run(verbose=False)
        u0 = run.sys.dev.get_state()
        res = {"vertices": int(run.mesh.num_vertices), "steady_run_wall_s": time.perf_counter() - t0,
               "steady_run_accepted_steps": int(run.stepper.accepted), "time_constant_s": float(run.ep.time_constant)}
        tc = run.ep.time_constant
        par = dict(kind="pulse", v_levels=[-5.5, -4.5], durations=[a.holds[0] * tc, a.holds[1] * tc], steps_per_segment=STEPS)
        nf = run.problem.nf
        free = np.ones(run.problem.ndof, dtype=bool)
        free[np.asarray(run.problem.bc_dofs, dtype=np.int64)] = False
        w = (ATOL + RTOL * np.abs(u0))
        # plain marching, capped
        stand_at(run, u0, -5.0)
        t0 = time.perf_counter()
        out = run.programme(cycles=a.cap, **par)
        wall = time.perf_counter() - t0
        ends = [u0] + [v.ravel() for k, (seg, t, v) in enumerate(out["states"]) if k % 2 == 1]
        errs = [float(math.sqrt((((y - x) / w)[free] ** 2).sum() / free.sum())) for x, y in zip(ends, ends[1:])]
        hit = next((k + 1 for k, e in enumerate(errs) if e <= a.tol), None)
        at = len(errs) if hit is None else hit
        res["plain"] = {"cap": a.cap, "cycles_to_tol": hit, "wall_s": wall, "wall_s_to_tol_prorated": None if hit is None else wall * hit / a.cap,
                        "wall_ms_per_cycle": 1e3 * wall / a.cap, "residuals": errs,
                        "contraction": errs[at - 1] / errs[at - 2] if at > 1 else None, "contraction_at_cycle": at,
                        "newton_iterations": out["metadata"]["programme_newton_iterations"], "nf": int(nf)}
        # the accelerated cycle map
        for depth in (2, 4, 8):
            stand_at(run, u0, -5.0)
            t0 = time.perf_counter()
            out = run.programme(periodic=dict(depth=depth, max_cycles=a.cap, tol=a.tol, rtol=RTOL, atol=ATOL), **par)
            wall = time.perf_counter() - t0
            meta, h = out["metadata"], out["periodic"]
            res["depth_%d" % depth] = {"converged": bool(meta["programme_periodic_converged"]), "cycles": int(meta["programme_periodic_cycles"]),
                                       "restarts": int(meta["programme_periodic_restarts"]), "wall_s": wall, "residuals": h["err"].tolist(),
                                       "alpha": h["alpha"].tolist(), "dropped": h["dropped"].tolist(),
                                       "newton_iterations": meta["programme_newton_iterations"],
                                       "FE_H2_cycle": float(out["FE_H2_cycle"][0]) if len(out["FE_H2_cycle"]) else None}
        # hook 33 on a full window of depth 4
        dev = run.sys.dev
        dev.cycle_open(4, RTOL, ATOL)
        for _ in range(5):
            dev.cycle_begin()
            dev.cycle_end()
        res["hook_33_us"] = dev.time_kernel(33, 200)
        dev.cycle_close()
        return res
    finally:
        run.sys.close()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--meshes", nargs="+", default=["1um", "50um"], choices=sorted(L_N))
    ap.add_argument("--cap", type=int, default=300)
    ap.add_argument("--tol", type=float, default=1e-3)
    ap.add_argument("--holds", type=float, nargs=2, default=[30.0, 20.0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "periodic.json"))
    a = ap.parse_args(argv)
    sys.path.insert(0, ROOT)
    from gmpnp_amd import backend
    res = {"build_id": backend.load_library().gmpnp_build_id().decode(), "tol": a.tol, "holds_scaled": a.holds, "steps_per_segment": STEPS,
           "weights": {"rtol": RTOL, "atol": ATOL}}
    for name in a.meshes:
        res[name] = measure(name, a)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:      # (written after every mesh: a later one may run long)
            json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
