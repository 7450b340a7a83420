"""Adaptive 1D ensembles (gmpnp_amd.edl_ensemble, adaptive_dt=True: every member on its own clock) against the same members as
serial adaptive EDLRuns, one after another, same process, same box.

Sweep: the 50 um mesh, K+, voltages spread over -1 ... -12.5, to `--steady_tol` (1e-5) with the default tolerances, B = 1, 2, 4, 8,
16 members; wall time of `run()` (construction not counted), the median of `--repeats` with the spread.  Per member: attempts,
accepted and rejected steps, Newton failures, stop reason.  `--max_steps` caps a member that never gets there.  `--step_fraction`:
the fraction-to-boundary limiter of the Newton updates, for both sides.
Round cost: wall time around one `time_error` + one `time_advance` of an ensemble (200 rounds) for B = 1, 8, 32, beside B times the
single handle's `gmpnp_time_kernel(22)` (estimator + reduce + shift, HIP events) measured in the same job.
Writes JSON (default profiles/ensemble_adaptive_rate.json).

    python tools/ensemble_adaptive_rate.py [--sizes 1 2 4 8 16] [--repeats 3] [--step_fraction TAU] [--max_steps N] [--out FILE]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def voltages(B):
    return [float(v) for v in np.linspace(-1.0, -12.5, B)] if B > 1 else [-1.0]


def member_row(run):
    s = run.stepper
    return {"voltage_multiplier": run.kwargs["voltage_multiplier"], "attempts": len(s.log), "accepted": s.accepted, "rejected": s.rejected,
            "newton_failures": s.newton_failures, "newton_iterations": int(sum(r["newton"] for r in s.log if r["newton"] > 0)),
            "stop_reason": s.stop_reason, "t_reached": s.t, "last_h": s.log[-1]["h"] if s.log else None}


def spread(w):
    return {"median_s": sorted(w)[len(w) // 2], "min_s": min(w), "max_s": max(w), "windows_s": w}


def sweep(B, a):
    from gmpnp_amd.edl1d import EDLRun
    from gmpnp_amd.edl_ensemble import EDLEnsemble
    volts = voltages(B)
    adaptive = dict(steady_tol=a.steady_tol, t_end=np.inf, max_steps=a.max_steps)
    dk = {"device_id": a.device_id}
    ens_w, ser_w, ens_rows, ser_rows, rounds = [], [], None, None, None
    for _ in range(a.repeats):
        with EDLEnsemble([{"voltage_multiplier": v} for v in volts], device_kwargs=dk, keep_history=False, step_fraction=a.step_fraction,
                         adaptive_dt=True, **adaptive) as ens:
            t0 = time.perf_counter()
            ens.run()
            ens_w.append(time.perf_counter() - t0)
            ens_rows, rounds = [member_row(r) for r in ens.runs], ens.stepper.rounds
            for k, e in enumerate(ens.errors):
                if e is not None:
                    ens_rows[k]["error"] = e[:200]
        runs = [EDLRun(device_kwargs=dk, step_fraction=a.step_fraction, adaptive_dt=True, voltage_multiplier=v, **adaptive) for v in volts]
        try:
            t0 = time.perf_counter()
            for r in runs:
                r.run(verbose=False)
            ser_w.append(time.perf_counter() - t0)
            ser_rows = [member_row(r) for r in runs]
        finally:
            for r in runs:
                r.sys.close()
    out = {"members": B, "voltages": volts, "rounds": rounds, "ensemble": spread(ens_w), "serial": spread(ser_w),
           "speedup_vs_serial": spread(ser_w)["median_s"] / spread(ens_w)["median_s"], "per_member": ens_rows,
           "same_attempts_as_serial": [(x["attempts"], x["accepted"], x["newton_failures"]) for x in ens_rows] ==
                                      [(x["attempts"], x["accepted"], x["newton_failures"]) for x in ser_rows]}
    return out


def round_cost(B, a, rounds=200):
    """One round's estimate + advance: wall time around the two calls, all members accepting."""
    from gmpnp_amd import backend
    from gmpnp_amd.edl1d import EDLRun
    runs = [EDLRun(device_kwargs={"device_id": a.device_id}, voltage_multiplier=v) for v in voltages(B)]
    try:
        for r in runs:
            r.step(verbose=False)
        single_us = runs[0].sys.dev.time_kernel(22, 200)
        with backend.DeviceEnsemble([r.sys.dev for r in runs]) as ens:
            h, tol, at, act = [1.0] * B, [1e-2] * B, [1e-4] * B, [1] * B
            for _ in range(5):
                ens.time_error(h, h, tol, at)
                ens.time_advance(act)
            t0 = time.perf_counter()
            for _ in range(rounds):
                ens.time_error(h, h, tol, at)
                ens.time_advance(act)
            us = (time.perf_counter() - t0) / rounds * 1e6
        return {"members": B, "round_us": us, "single_time_kernel_22_us": single_us, "B_times_single_us": B * single_us}
    finally:
        for r in runs:
            r.sys.close()


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--sizes", type=int, nargs="+", default=[1, 2, 4, 8, 16])
    p.add_argument("--round_sizes", type=int, nargs="*", default=[1, 8, 32])
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--steady_tol", type=float, default=1e-5)
    p.add_argument("--max_steps", type=int, default=400)
    p.add_argument("--step_fraction", type=float, default=0.0)
    p.add_argument("--device_id", type=int, default=0)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_adaptive_rate.json"))
    a = p.parse_args(argv)
    import __graft_entry__ as ge
    ge.build()
    warnings.simplefilter("ignore")
    out = {"case": "50 um mesh, K+, 0.1 M, voltages spread over -1 ... -12.5, steady_tol %g, default dt_rtol / dt_atol, max_steps %d, "
                   "step_fraction %g, median of %d" % (a.steady_tol, a.max_steps, a.step_fraction, a.repeats), "sweeps": [], "rounds": []}
    for B in a.sizes:
        r = sweep(B, a)
        out["sweeps"].append(r)
        print("B = %2d: ensemble %.3f s (%.3f ... %.3f), serial %.3f s (%.3f ... %.3f), %.2fx; rounds %d; attempts %s; stops %s" %
              (B, r["ensemble"]["median_s"], r["ensemble"]["min_s"], r["ensemble"]["max_s"], r["serial"]["median_s"], r["serial"]["min_s"],
               r["serial"]["max_s"], r["speedup_vs_serial"], r["rounds"], [m["attempts"] for m in r["per_member"]],
               sorted(set(m["stop_reason"] for m in r["per_member"]))), flush=True)
    for B in a.round_sizes:
        r = round_cost(B, a)
        out["rounds"].append(r)
        print("round cost B = %2d: %.1f us per time_error + time_advance; B x gmpnp_time_kernel(22) = %d x %.1f = %.1f us" %
              (B, r["round_us"], B, r["single_time_kernel_22_us"], r["B_times_single_us"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(a.out)


if __name__ == "__main__":
    main()
