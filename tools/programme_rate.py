"""Rate of a pulse train on the 1 um mesh and the cost of one electrode record, same process, same box.

K+ on the 1 um mesh, Stern BDM, the Tafel parameters of the tests: adaptive steps to the steady stop at p_M = -5 (the plain
``--adaptive_dt`` run: its wall time per accepted step is recorded), then a pulse train between -5.5 and -4.75 (40 us / 25 us holds,
``--cycles`` cycles) by ``EDLRun.programme``: accepted steps per second, the wall time per accepted step, the attempts, and hook 29
(``gmpnp_time_kernel``: the launches of one ``gmpnp_electrode_trace_append``).  ``--plain_only`` stops after the plain run and needs
nothing of section 5n, so the same file measures the parent commit's tree; ``--parent FILE`` copies that figure in beside this tree's.
Writes JSON (default profiles/programme.json).

    python tools/programme_rate.py [--cycles 50] [--plain_only] [--parent FILE] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(L_n=1e-6, cation="K", electrode_voltage=-5.0, kinetics="tafel", i0_CO=0.1, i0_H2=0.02, adaptive_dt=True, steady_tol=1e-5)


def plain_run(root):
    """The plain adaptive run to its steady stop: (run, figures).  The caller closes run.sys."""
    sys.path.insert(0, root)
    from gmpnp_amd.edl1d import EDLRun
    run = EDLRun(**KW)
    t0 = time.perf_counter()
    run.run(verbose=False)
    run.sys.dev.get_state()
    dt = time.perf_counter() - t0
    acc = run.stepper.accepted
    return run, {"vertices": int(run.mesh.num_vertices), "accepted_steps": int(acc), "attempts": len(run.stepper.log), "wall_s": dt,
                 "wall_ms_per_accepted_step": 1e3 * dt / max(acc, 1), "stop_reason": run.stepper.stop_reason}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cycles", type=int, default=50)
    ap.add_argument("--plain_only", action="store_true")
    ap.add_argument("--root", default=ROOT, help="the tree whose package is measured")
    ap.add_argument("--parent", default=None, help="JSON written by --plain_only on the parent commit's tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "programme.json"))
    a = ap.parse_args(argv)
    run, plain = plain_run(a.root)
    from gmpnp_amd import backend
    res = {"build_id": backend.load_library().gmpnp_build_id().decode(), "plain_adaptive_run": plain}
    try:
        if not a.plain_only:
            t0 = time.perf_counter()
            out = run.programme(kind="pulse", v_levels=[-5.5, -4.75], durations=[4.0e-5, 2.5e-5], cycles=a.cycles, dt_init=1.0)
            dt = time.perf_counter() - t0
            meta = out["metadata"]
            n = meta["programme_steps_accepted"]
            res["pulse_train"] = {"cycles": a.cycles, "accepted_steps": n, "rejected_steps": meta["programme_steps_rejected"],
                                  "stop_reason": meta["programme_stop_reason"], "wall_s": dt, "accepted_steps_per_s": n / dt,
                                  "wall_ms_per_accepted_step": 1e3 * dt / max(n, 1), "newton_iterations": meta["programme_newton_iterations"],
                                  "charge_closure": meta["programme_charge_closure"], "FE_H2_first_cycle": float(out["FE_H2_cycle"][0]),
                                  "FE_H2_last_cycle": float(out["FE_H2_cycle"][-1])}
            run.sys.dev.electrode_trace_open(4)
            res["hook_29_us"] = run.sys.dev.time_kernel(29, 200)
            run.sys.dev.electrode_trace_close()
    finally:
        run.sys.close()
    if a.parent:
        with open(a.parent) as fh:
            res["parent_plain_adaptive_run"] = json.load(fh)["plain_adaptive_run"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
