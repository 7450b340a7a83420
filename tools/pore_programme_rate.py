"""Cost of a potential programme in the 3D pore and of its wall profile on L_10_R_5, same process, same box.

The README's Tafel example (electrode_voltage -1, i0_CO 10, i0_H2 1, band LU): ``--schedule`` plain time steps (their wall time per
step is the plain run's figure), then from that state a pulse train between -1.25 and -0.75 with holds of two and one reference steps
(``--cycles`` cycles, fixed mode, two steps per segment, the Sechenov glue behind every accepted step) ``--repeats`` times with the
wall profile (``--bins`` bins) and as often without it, alternating: the wall time per accepted step of each with the spread of the
repeats; then hook 32 (``gmpnp_time_kernel``: the launches of one ``gmpnp_wall_profile_append`` back to back).  Nothing bounds these
figures.  Writes JSON (default profiles/pore_programme.json).

    python tools/pore_programme_rate.py [--cycles 5] [--repeats 3] [--bins 16] [--out FILE]
"""
import argparse
import dataclasses
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(L=10e-9, R=5e-9, concentration_elec=0.5, electrode_voltage=-1.0, kinetics="tafel", i0_CO=10.0, i0_H2=1.0)


def back_to(run, u, p, co2_bc):
    """The run and its handle back at the state, the potential and the CO2 Dirichlet value the pulse trains start from."""
    from gmpnp_amd.problem import pore_dirichlet
    run.sys.set_state(u, u)
    run.sys.dev.set_electrode_potential(p)
    run.stern = dataclasses.replace(run.stern, p_electrode=float(p))
    run.kinetics = dataclasses.replace(run.kinetics, p_electrode=float(p))
    run.problem.stern, run.problem.kinetics = run.stern, run.kinetics
    run.co2_bc = co2_bc
    run.sys.set_bcs(*pore_dirichlet(run.pp, run.bnd, co2_bc, stern=True))


def spread(values):
    return {"mean": sum(values) / len(values), "min": min(values), "max": max(values), "runs": list(values)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cycles", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--bins", type=int, default=16)
    ap.add_argument("--schedule", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pore_programme.json"))
    a = ap.parse_args(argv)
    sys.path.insert(0, ROOT)
    from gmpnp_amd import backend, programme as prg
    from gmpnp_amd.pore3d import SOLVER_PARAMETERS, PoreRun
    sp = {"nonlinear_solver": "newton", "newton_solver": dict(SOLVER_PARAMETERS["newton_solver"], linear_solver="band_lu")}
    run = PoreRun(num_steps=a.schedule, solver_parameters=sp, **KW)
    res = {"build_id": backend.load_library().gmpnp_build_id().decode(), "mesh": "L_10_R_5", "cycles": a.cycles, "bins": a.bins,
           "repeats": a.repeats}
    try:
        plain = []
        for _ in range(a.schedule):
            t0 = time.perf_counter()
            run.step(verbose=False)
            plain.append(1e3 * (time.perf_counter() - t0))
        res["vertices"] = int(run.mesh.num_vertices)
        res["plain_run_ms_per_step"] = spread(plain[1:] or plain)          # (the first step from the bulk state takes more iterations)
        u, p0, co2 = run.sys.dev.get_state(), run.stern.p_electrode, run.co2_bc
        pp = run.pp
        par = dict(kind="pulse", v_levels=[-1.25, -0.75], durations=[2.0 * pp.time_step, pp.time_step], cycles=a.cycles)
        segs = prg.build(par, p0, pp.time_constant, pp.thermal_voltage)
        edges = prg.resolve_bins(a.bins, run.wall_node_z(), pp.L)
        inv_dt = float(run.sys.problem.model.inv_dt)
        times = {"with_profile": [], "without_profile": []}
        steps = 0
        for _ in range(a.repeats):
            for key, e in (("with_profile", edges), ("without_profile", None)):
                back_to(run, u, p0, co2)
                t0 = time.perf_counter()
                ops = prg.DeviceProgrammeOps(run, run.solver_parameters, lambda h: 1.0 / h, after_accept=run.sechenov_glue, profile_edges=e)
                prg.run_programme(ops, segs, steps_per_segment=2)
                rec = ops.records()
                if e is not None:
                    ops.profile_records()
                dt = time.perf_counter() - t0
                run.sys.set_time_step(inv_dt)
                steps = len(rec)
                times[key].append(1e3 * dt / max(steps, 1))
        res["accepted_steps"] = steps
        res["pulse_train_ms_per_accepted_step"] = {k: spread(v) for k, v in times.items()}
        back_to(run, u, p0, co2)
        dev = run.sys.dev
        dev.wall_profile_open(edges, 4)
        res["hook_32_us_per_append"] = spread([dev.time_kernel(32, 50) for _ in range(a.repeats)])
        dev.wall_profile_close()
        dev.electrode_trace_open(4)
        res["hook_29_us_per_append"] = spread([dev.time_kernel(29, 50) for _ in range(a.repeats)])
        dev.electrode_trace_close()
    finally:
        run.sys.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
