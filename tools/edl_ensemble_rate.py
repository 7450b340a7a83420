"""Aggregate Newton iterations/s of 1D ensembles (gmpnp_amd.edl_ensemble) against the serial driver, same process, same box.

Window: the edl50 window of bench.py (the 1D script's 100 dry-run steps on the 50 um mesh) after `--warmup` steps, the median of
`--repeats` windows.  Ensembles of B = 1, 2, 4, 8, 16, 32 members with voltages spread over -1 ... -12.5 (K+, 0.1 M); the serial
figure is EDLRun with the reference's defaults (V = -1), as bench.py --case edl50 times it.  Writes JSON (default
profiles/edl_ensemble_rate.json).

    python tools/edl_ensemble_rate.py [--sizes 1 2 4 8 16 32] [--steps 100] [--warmup 3] [--repeats 3] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/edl_ensemble_rate.py --sizes 8 --no-serial --repeats 1
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def reset(run):
    run.sys.initialise([1.0] * 6 + [0.0])
    run.history = run.history[:1]
    run.newton_its, run.n, run.t = [], 0, 0.0
    run.current_H_frac = run.ep.current_H_frac


def serial_rate(steps, warmup, repeats, device_id):
    from gmpnp_amd.edl1d import EDLRun
    run = EDLRun(device_kwargs={"device_id": device_id})
    try:
        for _ in range(warmup):
            run.step(verbose=False)
        windows, its = [], 0
        for _ in range(repeats):
            reset(run)
            t0 = time.perf_counter()
            for _ in range(steps):
                run.step(verbose=False)
            windows.append(time.perf_counter() - t0)
            its = int(sum(run.newton_its))
        dt = sorted(windows)[len(windows) // 2]
        return {"newton_iterations": its, "seconds": dt, "its_per_s": its / dt, "windows_s": windows}
    finally:
        run.sys.close()


def ensemble_rate(B, steps, warmup, repeats, device_id):
    from gmpnp_amd.edl_ensemble import EDLEnsemble
    volts = [float(v) for v in np.linspace(-1.0, -12.5, B)] if B > 1 else [-1.0]
    with EDLEnsemble([{"voltage_multiplier": v} for v in volts], num_steps=steps, device_kwargs={"device_id": device_id}) as ens:
        for _ in range(warmup):
            ens.step()
        windows, its = [], 0
        for _ in range(repeats):
            for r in ens.runs:
                reset(r)
            ens.n = 0
            t0 = time.perf_counter()
            ens.run()
            windows.append(time.perf_counter() - t0)
            its = int(sum(sum(r.newton_its) for r in ens.runs))
            assert all(e is None for e in ens.errors), ens.errors
        dt = sorted(windows)[len(windows) // 2]
        return {"members": B, "voltages": volts, "newton_iterations": its, "seconds": dt, "its_per_s": its / dt,
                "windows_s": windows, "per_member_its": [int(sum(r.newton_its)) for r in ens.runs]}


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--sizes", type=int, nargs="+", default=[1, 2, 4, 8, 16, 32])
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--device_id", type=int, default=0)
    p.add_argument("--no-serial", action="store_true")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "edl_ensemble_rate.json"))
    a = p.parse_args(argv)
    import __graft_entry__ as ge
    ge.build()
    out = {"window": "edl50: %d dry-run steps, 50 um mesh, after %d warm-up steps, median of %d" % (a.steps, a.warmup, a.repeats)}
    if not a.no_serial:
        out["serial"] = serial_rate(a.steps, a.warmup, a.repeats, a.device_id)
        print("serial EDLRun: %.0f Newton its/s" % out["serial"]["its_per_s"], flush=True)
    out["ensembles"] = []
    for B in a.sizes:
        r = ensemble_rate(B, a.steps, a.warmup, a.repeats, a.device_id)
        if "serial" in out:
            r["speedup_vs_serial"] = r["its_per_s"] / out["serial"]["its_per_s"]
        out["ensembles"].append(r)
        print("B = %2d: %.0f Newton its/s%s" % (B, r["its_per_s"], "  (%.2fx serial)" % r["speedup_vs_serial"] if "serial" in out else ""),
              flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(a.out)


if __name__ == "__main__":
    main()
