"""Aggregate Newton iterations/s of 3D pore ensembles (gmpnp_amd.pore_ensemble) against the serial driver, same process, same box.

Meshes L_50_R_5 and L_10_R_5; ensembles of B = 1, 2, 4, 8 members at 0.5 M and voltage_multiplier = -1 that differ in H2_FE and
current_rough (the 3D driver runs K+ only).  A run = the state reset to the initial one, `--warmup` steps, then `--steps` timed
steps; the figure is the median of `--repeats` runs and the spread (max - min) / median of their rates is printed beside it.
Baselines, measured in the same job:
  (a) the default serial PoreRun (fast two-launch BiCGStab form, side streams): B runs one after another run at this rate;
  (b) the serial PoreRun with shared_device=1 (what an ensemble member is);
  (c) three PoreRuns on three host threads, each handle on one stream (what ``sweep --jobs_per_gpu 3`` does).
Writes JSON (default profiles/pore_ensemble_rate.json).

    python tools/pore_ensemble_rate.py [--meshes 50 10] [--sizes 1 2 4 8] [--steps 10] [--warmup 2] [--repeats 3] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/pore_ensemble_rate.py --meshes 50 --sizes 4 --no-serial --repeats 1
"""
import argparse
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def member(i, L):
    return dict(concentration_elec=0.5, voltage_multiplier=-1.0, L=L, R=5e-9, H2_FE=0.05 + 0.05 * (i % 4), current_rough=3000.0 - 500.0 * (i // 4))


def reset(run):
    from gmpnp_amd.problem import pore_dirichlet
    run.sys.initialise([1.0] * 8 + [0.0])
    run.co2_bc, run.CO2_min = None, None
    run.sys.set_bcs(*pore_dirichlet(run.pp, run.bnd, None))
    run.history = run.history[:1]
    run.newton_its, run.n, run.t = [], 0, 0.0


def summary(rates, its, extra=None):
    rates = sorted(rates)
    med = rates[len(rates) // 2]
    out = {"newton_iterations": its, "its_per_s": med, "runs_its_per_s": rates, "spread": (rates[-1] - rates[0]) / med}
    out.update(extra or {})
    return out


def serial_rate(L, steps, warmup, repeats, device_kwargs):
    from gmpnp_amd.pore3d import PoreRun
    run = PoreRun(num_steps=steps + warmup, device_kwargs=device_kwargs, **member(0, L))
    try:
        rates, its = [], 0
        for _ in range(repeats):
            reset(run)
            for _ in range(warmup):
                run.step(verbose=False)
            t0 = time.perf_counter()
            for _ in range(steps):
                run.step(verbose=False)
            dt = time.perf_counter() - t0
            its = int(sum(run.newton_its[warmup:]))
            rates.append(its / dt)
        return summary(rates, its)
    finally:
        run.sys.close()


def threads_rate(L, nthreads, steps, warmup, repeats, device_id):
    """`nthreads` runs in flight from threads of this process, the handles configured as ``sweep --jobs_per_gpu`` configures them."""
    from gmpnp_amd.pore3d import PoreRun
    runs = [PoreRun(num_steps=steps + warmup, device_kwargs={"device_id": device_id, "coarse_refresh": 3, "warm_in_stream": 1}, **member(i, L))
            for i in range(nthreads)]
    try:
        rates, its = [], 0
        for _ in range(repeats):
            start, t_begin = threading.Barrier(nthreads + 1), [0.0]

            def work(run):
                reset(run)
                for _ in range(warmup):
                    run.step(verbose=False)
                start.wait()
                for _ in range(steps):
                    run.step(verbose=False)

            ths = [threading.Thread(target=work, args=(r,)) for r in runs]
            for t in ths:
                t.start()
            start.wait()
            t_begin[0] = time.perf_counter()
            for t in ths:
                t.join()
            dt = time.perf_counter() - t_begin[0]
            its = int(sum(sum(r.newton_its[warmup:]) for r in runs))
            rates.append(its / dt)
        return summary(rates, its, {"threads": nthreads})
    finally:
        for r in runs:
            r.sys.close()


def ensemble_rate(L, B, steps, warmup, repeats, device_id):
    from gmpnp_amd.pore_ensemble import PoreEnsemble
    with PoreEnsemble([member(i, L) for i in range(B)], num_steps=steps + warmup, device_kwargs={"device_id": device_id}) as ens:
        rates, its = [], 0
        for _ in range(repeats):
            for r in ens.runs:
                reset(r)
            ens.n = 0
            for _ in range(warmup):
                ens.step()
            t0 = time.perf_counter()
            for _ in range(steps):
                ens.step()
            dt = time.perf_counter() - t0
            assert all(e is None for e in ens.errors), ens.errors
            its = int(sum(sum(r.newton_its[warmup:]) for r in ens.runs))
            rates.append(its / dt)
        return summary(rates, its, {"members": B, "per_member_its": [int(sum(r.newton_its[warmup:])) for r in ens.runs]})


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--meshes", type=int, nargs="+", default=[50, 10], help="pore lengths in nm (L_<n>_R_5)")
    p.add_argument("--sizes", type=int, nargs="+", default=[1, 2, 4, 8])
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--device_id", type=int, default=0)
    p.add_argument("--no-serial", action="store_true")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "pore_ensemble_rate.json"))
    a = p.parse_args(argv)
    import __graft_entry__ as ge
    ge.build()
    out = {"window": "%d steps after %d warm-up steps from the initial state, median of %d runs; 0.5 M, V = -1, K+" % (a.steps, a.warmup, a.repeats),
           "meshes": {}}
    for Lnm in a.meshes:
        L = Lnm * 1e-9
        m = out["meshes"]["L_%d_R_5" % Lnm] = {}
        if not a.no_serial:
            m["serial_default"] = serial_rate(L, a.steps, a.warmup, a.repeats, {"device_id": a.device_id})
            m["serial_shared_device"] = serial_rate(L, a.steps, a.warmup, a.repeats, {"device_id": a.device_id, "shared_device": 1})
            m["threads_3"] = threads_rate(L, 3, a.steps, a.warmup, a.repeats, a.device_id)
            for key in ("serial_default", "serial_shared_device", "threads_3"):
                print("L_%d_R_5 %-22s %7.1f Newton its/s  (spread %.1f %%)" % (Lnm, key, m[key]["its_per_s"], 100 * m[key]["spread"]), flush=True)
        m["ensembles"] = []
        for B in a.sizes:
            r = ensemble_rate(L, B, a.steps, a.warmup, a.repeats, a.device_id)
            if "serial_default" in m:
                for key in ("serial_default", "serial_shared_device", "threads_3"):
                    r["vs_" + key] = r["its_per_s"] / m[key]["its_per_s"]
            m["ensembles"].append(r)
            print("L_%d_R_5 ensemble B = %d         %7.1f Newton its/s  (spread %.1f %%)%s" % (
                Lnm, B, r["its_per_s"], 100 * r["spread"],
                "  %.2fx default serial, %.2fx shared_device serial, %.2fx three threads" % (r["vs_serial_default"], r["vs_serial_shared_device"], r["vs_threads_3"])
                if "serial_default" in m else ""), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(a.out)


if __name__ == "__main__":
    main()
