"""Cost of the transient sensitivities on the 1 um mesh, same process, same box.

K+ on the 1 um mesh, Stern BDM, the Tafel parameters of the tests: adaptive steps to the steady stop at p_M = -5, then the pulse
train of tools/programme_rate.py (between -5.5 and -4.75, 40 us / 25 us holds, ``--cycles`` cycles) by ``EDLRun.programme`` three
times from that state: without sensitivities, with two columns and with six (``--columns``), each from the steady tangent: the wall
time per accepted step of each; then hook 31 (``gmpnp_time_kernel``: the launches of one ``gmpnp_sensitivity_step``) with six columns.
Writes JSON (default profiles/sensitivity.json).

    python tools/sensitivity_rate.py [--cycles 20] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(L_n=1e-6, cation="K", electrode_voltage=-5.0, kinetics="tafel", i0_CO=0.1, i0_H2=0.02, adaptive_dt=True, steady_tol=1e-5)
SIX = ("i0_CO", "i0_H2", "alpha_CO", "alpha_H2", "stern_length", "offset")


def back_to(run, u, p):
    """The run and its handle back at the state ``u`` and the potential ``p`` the pulse trains start from."""
    import dataclasses
    run.sys.set_state(u, u)
    run.sys.dev.set_electrode_potential(p)
    run.stern = dataclasses.replace(run.stern, p_electrode=float(p))
    run.kinetics = dataclasses.replace(run.kinetics, p_electrode=float(p))
    run.problem.stern, run.problem.kinetics = run.stern, run.kinetics


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cycles", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sensitivity.json"))
    a = ap.parse_args(argv)
    sys.path.insert(0, ROOT)
    from gmpnp_amd import backend
    from gmpnp_amd.edl1d import EDLRun
    run = EDLRun(**KW)
    res = {"build_id": backend.load_library().gmpnp_build_id().decode(), "cycles": a.cycles, "pulse_train": {}}
    try:
        run.run(verbose=False)
        u = run.sys.dev.get_state()
        res["vertices"] = int(run.mesh.num_vertices)
        for names in ((), SIX[:2], SIX, ()):          # the plain train twice: first and last, the scatter of the window
            back_to(run, u, KW["electrode_voltage"])
            par = dict(kind="pulse", v_levels=[-5.5, -4.75], durations=[4.0e-5, 2.5e-5], cycles=a.cycles, dt_init=1.0)
            if names:
                par["sensitivities"] = names
            t0 = time.perf_counter()
            out = run.programme(**par)
            dt = time.perf_counter() - t0
            meta = out["metadata"]
            n = meta["programme_steps_accepted"]
            key = "%d_columns" % len(names) + ("_again" if not names and "0_columns" in res["pulse_train"] else "")
            res["pulse_train"][key] = {"accepted_steps": n, "rejected_steps": meta["programme_steps_rejected"], "wall_s": dt,
                                       "wall_ms_per_accepted_step": 1e3 * dt / max(n, 1),
                                       "sensitivity_status": meta.get("programme_sensitivity_status"),
                                       "sensitivity_residual": meta.get("programme_sensitivity_residual")}
        run.sys.dev.sensitivity_open([16, 17, 32, 33, 48, 0], "zero", 4)
        res["hook_31_us_six_columns"] = run.sys.dev.time_kernel(31, 100)
        run.sys.dev.sensitivity_close()
        run.sys.dev.sensitivity_open([16, 17], "zero", 4)
        res["hook_31_us_two_columns"] = run.sys.dev.time_kernel(31, 100)
        run.sys.dev.sensitivity_close()
    finally:
        run.sys.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
