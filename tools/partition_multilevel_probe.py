"""Multilevel term across mesh partitions (gmpnp_group_attach_coarse_group): Newton iterations per second, BiCGStab iterations per
linear solve and Newton counts of the two-level and the multilevel form, for P = 1, 2, 4 in-process partitions on the twice-refined
L_50_R_5 mesh.  The in-process partitions time-share one GPU: only the ratio of the two forms at the same P means anything.
Step 1 (from the zero state) is run untimed; the timed figures are those of the following steps.

    python tools/partition_multilevel_probe.py [refine=2] [steps=2] [out.json]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402
ge.build()
from gmpnp_amd.pore3d import PoreRun  # noqa: E402

R = int(sys.argv[1]) if len(sys.argv) > 1 else 2
steps = max(2, int(sys.argv[2]) if len(sys.argv) > 2 else 2)
path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "partition_multilevel_refine%d.json" % R)
parts = [int(p) for p in os.environ.get("PROBE_PARTS", "1,2,4").split(",")]
forms = os.environ.get("PROBE_FORMS", "two-level,multilevel").split(",")   # (one form alone: a profiler run)
out = {"mesh": "L_50_R_5", "refine": R, "steps": steps, "timed_steps": steps - 1, "partitions": "in-process, one GPU", "runs": {}}
for P in parts:
    for name, kw in (("two-level", {}), ("multilevel", {"multilevel": True})):
        if name not in forms:
            continue
        run = PoreRun(num_steps=steps, concentration_elec=0.5, L=50e-9, R=5e-9, refine=R, partition=(P, None), **kw)
        try:
            per = [run.step(verbose=False)]
            t0 = time.perf_counter()
            for _ in range(steps - 1):
                per.append(run.step(verbose=False))
            wall = time.perf_counter() - t0
            timed = per[1:]
            its = sum(st["iterations"] for st in timed)
            kry = sum(st["krylov_iterations"] for st in timed)
            rec = {"n_vertices": run.mesh.num_vertices, "newton_per_step": [st["iterations"] for st in per],
                   "krylov_per_solve_by_step": [list(st["krylov_per_iteration"][:st["iterations"]]) for st in per],
                   "timed_newton_iterations": its, "timed_krylov_iterations": kry, "seconds": wall,
                   "newton_its_per_s": its / wall, "krylov_per_solve": kry / max(its, 1), "ms_per_krylov_iteration": 1e3 * wall / max(kry, 1)}
        finally:
            run.sys.close()
        out["runs"]["P%d %s" % (P, name)] = rec
        print("P=%d %-10s" % (P, name), json.dumps({k: v for k, v in rec.items() if k != "krylov_per_solve_by_step"}), flush=True)
    if len(forms) < 2:
        continue
    a, b = out["runs"]["P%d two-level" % P], out["runs"]["P%d multilevel" % P]
    out["runs"]["P%d multilevel" % P]["speedup_newton_its_per_s"] = b["newton_its_per_s"] / a["newton_its_per_s"]
    print("P=%d multilevel / two-level Newton its/s: %.2f" % (P, b["newton_its_per_s"] / a["newton_its_per_s"]), flush=True)
os.makedirs(os.path.dirname(path), exist_ok=True)
with open(path, "w") as fh:
    json.dump(out, fh, indent=1)
print("wrote", path)
