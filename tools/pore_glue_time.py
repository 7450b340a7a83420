"""Per-step glue of the partitioned pore driver, PoreRun(glue="host") against glue="device" (DESIGN.md section 6), and the Newton
iterations per second of the CLI (pore3d --partitions) on the same case.

  python tools/pore_glue_time.py [--L 50e-9] [--refine 2] [--parts 4] [--steps 3] [--warmup 1] [--out FILE]

A step is timed on the host around PoreRun.step; its glue is that time minus the time of its Newton solve (the system's solve
call, which returns after the library's last synchronisation).  The CLI figure is the Newton iterations of its time loop over
the wall time of PoreRun.run (set-up and output files excluded)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def glue_run(glue, a):
    from gmpnp_amd.pore3d import PoreRun
    run = PoreRun(num_steps=a.warmup + a.steps, concentration_elec=0.5, L=a.L, R=5e-9, refine=a.refine, multilevel=a.refine > 0,
                  partition=(a.parts, None), glue=glue)
    solve, t_solve, t_step = run.sys.solve, [], []

    def timed_solve(*args, **kw):
        t0 = time.perf_counter()
        st = solve(*args, **kw)
        t_solve.append(time.perf_counter() - t0)
        return st

    run.sys.solve = timed_solve
    try:
        for _ in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            run.step(verbose=False)
            t_step.append(time.perf_counter() - t0)
    finally:
        run.sys.close()
    glue_ms = [1e3 * (s - v) for s, v in zip(t_step, t_solve)][a.warmup:]
    its = run.newton_its[a.warmup:]
    return {"glue": glue, "n_vertices": int(run.mesh.num_vertices), "glue_ms_median": float(np.median(glue_ms)), "glue_ms": glue_ms,
            "step_ms": [1e3 * t for t in t_step[a.warmup:]], "newton_iterations": its,
            "newton_its_per_s": float(sum(its) / sum(t_step[a.warmup:]))}


def cli_run(a):
    from gmpnp_amd import pore3d
    run_fn, timing = pore3d.PoreRun.run, {}

    def timed(self, verbose=True):
        t0 = time.perf_counter()
        r = run_fn(self, verbose)
        timing.update(seconds=time.perf_counter() - t0, newton_iterations=int(sum(self.newton_its)))
        return r

    pore3d.PoreRun.run = timed
    argv = ["--L=%g" % a.L, "--R=5e-9", "--concentration_elec=0.5", "--num_steps=%d" % (a.warmup + a.steps), "--refine", str(a.refine),
            "--partitions", str(a.parts)] + (["--multilevel"] if a.refine > 0 else [])
    with tempfile.TemporaryDirectory() as d:
        os.environ["GMPNP_OUT"] = d
        t0 = time.perf_counter()
        pore3d.main(argv)
        total = time.perf_counter() - t0
    pore3d.PoreRun.run = run_fn
    return {"argv": argv, "newton_iterations": timing["newton_iterations"], "loop_seconds": timing["seconds"], "total_seconds": total,
            "newton_its_per_s": timing["newton_iterations"] / timing["seconds"]}


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--L", type=float, default=50e-9)
    p.add_argument("--refine", type=int, default=2)
    p.add_argument("--parts", type=int, default=4)
    p.add_argument("--steps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import __graft_entry__ as ge
    ge.build()
    res = {"case": {"L": a.L, "R": 5e-9, "refine": a.refine, "multilevel": a.refine > 0, "partitions": a.parts, "steps": a.steps,
                    "warmup": a.warmup}}
    for glue in ("host", "device"):
        res[glue] = glue_run(glue, a)
        print(json.dumps({glue: {k: res[glue][k] for k in ("glue_ms_median", "newton_its_per_s")}}), flush=True)
    res["cli"] = cli_run(a)
    print(json.dumps({"cli": res["cli"]}), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
