"""Parameter sweep over pore radii and voltages, one independent pore problem per GPU at a time (BASELINE configs[4]:
"L_50_R_{1,2,2.5,4,5,7.5,10} x voltage ramp, 8 x MI355X one partition per GPU").

The reference runs such sweeps as a shell loop over ``python MPNP_CO2ER_pore.py --R=... --voltage_multiplier=...``
(3D/MPNP_CO2ER_pore.py:1088-1253 is the per-run CLI); every run is independent, so the multi-GPU mapping has no
data-path collective: rank r takes jobs r, r+world, r+2*world, ... and the per-job summaries are gathered on rank 0
at the end (one ``all_gather_object``).

  python -m gmpnp_amd.sweep --num_steps 20                                   # 1 GPU, all 35 jobs in turn
  python -m torch.distributed.run --nproc-per-node 8 -m gmpnp_amd.sweep      # one rank per GPU (RCCL only for the gather)
  python -m gmpnp_amd.sweep --ensemble --num_steps 20                        # the voltages of one mesh as one device ensemble
  python -m gmpnp_amd.sweep --ensemble --adaptive_dt --steady_tol 1e-5       # ... every member stepping adaptively on its own clock
"""
from __future__ import annotations

import argparse
import json
import time

RADII_NM = (1, 2, 2.5, 4, 5, 7.5, 10)                  # the seven L_50_R_* meshes of the reference's utilities/
VOLTAGES = (-1.0, -2.5, -5.0, -7.5, -10.0)             # the ramp recorded in 1D/Stern_CO2ER.py:66-68


def jobs(radii=RADII_NM, voltages=VOLTAGES):
    return [(r, v) for r in radii for v in voltages]


def my_jobs(all_jobs, rank, world):
    """Round-robin deal; the radii vary fastest across ranks so that every GPU sees small and large meshes."""
    return [j for k, j in enumerate(all_jobs) if k % world == rank]


def ramp_value(target, n, ramp_steps, start=-1.0):
    """Wall potential in force during time step n of a ramped run: linear from ``start`` to ``target`` over the
    first ``ramp_steps`` steps, ``target`` afterwards (ramp_steps = 0: the reference's behaviour, target from step 0)."""
    if ramp_steps <= 0 or abs(target) <= abs(start):
        return float(target)
    return float(start + (target - start) * min(n, ramp_steps) / ramp_steps)


def group_by_radius(job_list):
    """The jobs a rank holds, grouped by mesh: [(radius, [indices into job_list])] in order of first appearance, the jobs of a
    group in their original order; every job appears in exactly one group."""
    groups = {}
    for k, (r, _) in enumerate(job_list):
        groups.setdefault(r, []).append(k)
    return list(groups.items())


def run_group(radius_nm, voltages, num_steps, concentration_elec=0.5, device_id=0, write=False, as_published=False, ramp_steps=0,
              L=50e-9, device_kwargs=None, budget=False, **adaptive):
    """The runs of ``run_job`` for every voltage on ONE mesh as one ``PoreEnsemble`` (one launch chain per Newton iteration for all
    of them); returns their summaries in the order of ``voltages``, with the keys ``run_job`` gives (``seconds``: the group's).
    ``adaptive``: the adaptive-stepping keywords of ``PoreEnsemble``; with ``adaptive_dt`` every member runs until it stops
    (``num_steps`` is not used) and its summary gets ``stop_reason``, ``steps_accepted`` and ``steps_rejected``."""
    if adaptive.get("adaptive_dt") and ramp_steps > 0:
        raise ValueError("--adaptive_dt: the voltage ramp (--ramp_steps) counts fixed steps")
    from .impedance import refuse_impedance, refuse_pore_impedance
    from .polarisation import refuse_polarisation
    from .fit import refuse_fit
    from .programme import refuse_pore_programme, refuse_programme
    from .problem import refuse_galvanostat, refuse_kinetics, refuse_stern
    refuse_impedance(adaptive, "the pore sweep")
    refuse_pore_impedance(adaptive, "the pore sweep")
    refuse_polarisation(adaptive, "the pore sweep")
    refuse_fit(adaptive, "the pore sweep")
    refuse_programme(adaptive, "the pore sweep")
    refuse_pore_programme(adaptive, "the pore sweep")
    refuse_galvanostat(adaptive, "the pore sweep")
    refuse_stern(adaptive, "the pore sweep")
    refuse_kinetics(adaptive, "the pore sweep")
    from .pore_ensemble import PoreEnsemble
    from .problem import pore_dirichlet
    t0 = time.perf_counter()
    outs = [{"R_nm": radius_nm, "voltage_multiplier": v, "steps_requested": num_steps, "ramp_steps": ramp_steps} for v in voltages]
    members = [dict(concentration_elec=concentration_elec, L=L, R=radius_nm * 1e-9, voltage_multiplier=ramp_value(v, 0, ramp_steps),
                    as_published=as_published) for v in voltages]
    with PoreEnsemble(members, num_steps=num_steps, device_kwargs=dict({"device_id": device_id}, **(device_kwargs or {})),
                      keep_history=write, budget=budget, **adaptive) as ens:
        if ens.stepper is not None:
            ens.run()
        for n in range(0 if ens.stepper is not None else num_steps):
            ens.step()
            for k in ens.live():   # --ramp_steps, per member: the Dirichlet set of the NEXT step
                run = ens.runs[k]
                v_next = ramp_value(voltages[k], n + 1, ramp_steps)
                if v_next != run.pp.voltage_scaled:
                    run.pp.voltage_scaled = v_next
                    run.sys.set_bcs(*pore_dirichlet(run.pp, run.bnd, run.co2_bc))
        paths = ens.write_outputs() if write else None
        for k, (out, run) in enumerate(zip(outs, ens.runs)):
            out.update(n_vertices=run.mesh.num_vertices, n_dofs=run.problem.ndof)
            if ens.errors[k] is None:
                out.update(wall_potential=float(run.pp.voltage_scaled), status="ok")
                if write:
                    out["directory"] = paths[k]
            else:
                out.update(status="newton_failed", error=ens.errors[k][:200])
            out.update(steps_done=run.n, newton_iterations=int(sum(run.newton_its)), krylov_iterations=int(run.sys.krylov_iterations),
                       CO2_min=None if run.CO2_min is None else float(run.CO2_min))
            if run.budget is not None:
                out.update(run.budget.summary())
            if run.stepper is not None:
                out.update(stop_reason=run.stepper.stop_reason, steps_accepted=run.stepper.accepted, steps_rejected=run.stepper.rejected)
    dt = time.perf_counter() - t0
    for out in outs:
        out["seconds"] = dt
    return outs


def run_job(radius_nm, voltage, num_steps, concentration_elec=0.5, device_id=0, write=False, as_published=False, ramp_steps=0,
            one_stream=False, L=50e-9, device_kwargs=None, budget=False, electrode_voltage=None, kinetics=None, target_current=None, impedance=None, pore_impedance=None, pore_programme=None):
    """One pore run of ``num_steps`` time steps; returns a small summary dict (never raises for a diverged Newton).

    ``ramp_steps`` > 0 is a continuation the reference does not have: the wall potential Dirichlet value (bc3 of
    3D:460-467) moves from -1 to the target over that many time steps, every step starting from the previous state;
    Newton from the zero state diverges for |voltage_multiplier| >= 5 (as published) or > 1 (with the wall fluxes),
    in the CPU oracle exactly as on the GPU.  ``electrode_voltage`` (the Stern boundary condition of ``PoreRun``) is refused
    with ValueError: the sweep prescribes and ramps the wall potential itself; so is ``kinetics`` (the surface kinetics need it)."""
    from .impedance import refuse_impedance, refuse_pore_impedance
    from .problem import refuse_galvanostat, refuse_kinetics, refuse_stern
    refuse_impedance({"impedance": impedance}, "the pore sweep")
    refuse_pore_impedance({"pore_impedance": pore_impedance}, "the pore sweep")
    from .programme import refuse_pore_programme
    refuse_pore_programme({"pore_programme": pore_programme}, "the pore sweep")
    refuse_galvanostat({"target_current": target_current}, "the pore sweep")
    refuse_stern({"electrode_voltage": electrode_voltage}, "the pore sweep")
    refuse_kinetics({"kinetics": kinetics}, "the pore sweep")
    from .pore3d import PoreRun
    from .problem import pore_dirichlet
    t0 = time.perf_counter()
    out = {"R_nm": radius_nm, "voltage_multiplier": voltage, "steps_requested": num_steps, "ramp_steps": ramp_steps}
    run = None
    try:
        run = PoreRun(num_steps=num_steps, concentration_elec=concentration_elec, L=L, R=radius_nm * 1e-9,
                      voltage_multiplier=ramp_value(voltage, 0, ramp_steps), as_published=as_published, budget=budget,
                      # several runs in flight on one GPU: every handle keeps to ONE stream (coarse rebuild and warm-start test in
                      # the main stream): with side streams K handles are 2K streams on the process's four hardware queues
                      device_kwargs=dict({"device_id": device_id}, **dict({"coarse_refresh": 3, "warm_in_stream": 1} if one_stream else {},
                                                                          **(device_kwargs or {}))))
        out.update(n_vertices=run.mesh.num_vertices, n_dofs=run.problem.ndof)
        for n in range(num_steps):
            run.step(verbose=False)
            v_next = ramp_value(voltage, n + 1, ramp_steps)
            if v_next != run.pp.voltage_scaled:  # the Dirichlet set of the NEXT step (3D:835-838 rebuilds bc4 the same way)
                run.pp.voltage_scaled = v_next
                run.sys.set_bcs(*pore_dirichlet(run.pp, run.bnd, run.co2_bc))
        out.update(wall_potential=float(run.pp.voltage_scaled))
        out.update(status="ok")
        if write:
            out["directory"] = run.write_outputs()
    except RuntimeError as e:  # DOLFIN's behaviour: a non-converged Newton aborts THAT run (3D:789-799)
        out.update(status="newton_failed", error=str(e)[:200])
    if run is not None:
        out.update(steps_done=run.n, newton_iterations=int(sum(run.newton_its)), krylov_iterations=int(run.sys.krylov_iterations),
                   CO2_min=None if run.CO2_min is None else float(run.CO2_min))
        if run.budget is not None:   # CO2_wall_uptake [mol / s], CO2_entry_supply, max_abs_closure of the last step run
            out.update(run.budget.summary())
        run.sys.close()
    out["seconds"] = time.perf_counter() - t0
    return out


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--num_steps", type=int, default=20)
    p.add_argument("--concentration_elec", type=float, default=0.5)
    p.add_argument("--radii", type=float, nargs="*", default=list(RADII_NM))
    p.add_argument("--voltages", type=float, nargs="*", default=list(VOLTAGES))
    p.add_argument("--as_published", action="store_true",
                   help="the weak form exactly as published (no ds(2)/ds(3) flux terms, SURVEY Q1); the intended form with "
                        "the wall fluxes only converges from the zero initial guess at voltage_multiplier = -1")
    p.add_argument("--ramp_steps", type=int, default=0,
                   help="move the wall potential from -1 to the target over this many time steps (continuation; 0 = the "
                        "reference's behaviour, the target applies from step 0)")
    p.add_argument("--jobs_per_gpu", type=int, default=1, help="independent runs kept in flight on each GPU (separate streams; 3 gives 1.56x the throughput of 1)")
    p.add_argument("--ensemble", action="store_true",
                   help="run the jobs of one mesh (its voltages) as one device ensemble: one launch chain per Newton iteration for all "
                        "of them (gmpnp_amd.pore_ensemble; every handle on one stream, four launches per BiCGStab iteration)")
    p.add_argument("--budget", action="store_true", help="record the species budgets of every step; each job summary gets the CO2 wall uptake, the "
                   "CO2 supplied by its Dirichlet face and the largest closure (gmpnp_amd/budget.py); with --write also budget.npz")
    p.add_argument("--write", action="store_true", help="write the reference's output files of every run under $GMPNP_OUT")
    p.add_argument("--backend", default=None, help="torch.distributed backend for the final gather (default: nccl)")
    from .timestep import adaptive_keywords, add_adaptive_arguments
    add_adaptive_arguments(p)   # (with --ensemble)
    a = p.parse_args(argv)
    if a.adaptive_dt and not a.ensemble:
        raise ValueError("--adaptive_dt: the sweep steps adaptively as a device ensemble only (add --ensemble); a single adaptive "
                         "run is gmpnp_amd.pore3d --adaptive_dt")
    if a.dt_order != 1:   # (before anything touches the device)
        from .timestep import ORDER2_ENSEMBLE_REFUSAL
        raise ValueError("--" + ORDER2_ENSEMBLE_REFUSAL)
    adaptive = adaptive_keywords(a) if a.adaptive_dt else {}
    from .dist import init_process_group_from_env
    rank, world, local, dist = init_process_group_from_env(a.backend or "nccl")
    radii = [int(r) if float(r).is_integer() else r for r in a.radii]
    mine = my_jobs(jobs(radii, a.voltages), rank, world)
    t0 = time.perf_counter()
    def one(job):
        return run_job(job[0], job[1], a.num_steps, a.concentration_elec, device_id=local, write=a.write,
                       as_published=a.as_published, ramp_steps=a.ramp_steps, one_stream=a.jobs_per_gpu > 1, budget=a.budget)

    if a.ensemble:
        res = [None] * len(mine)
        for radius, idx in group_by_radius(mine):
            outs = run_group(radius, [mine[k][1] for k in idx], a.num_steps, a.concentration_elec, device_id=local, write=a.write,
                             as_published=a.as_published, ramp_steps=a.ramp_steps, budget=a.budget, **adaptive)
            for k, out in zip(idx, outs):
                res[k] = out
    elif a.jobs_per_gpu > 1:
        # A 3.7k-vertex problem is launch-latency bound: independent problems on separate HIP streams
        # overlap on one GPU.  Measured (tools/concurrent_runs_probe.py, profiles/r03/concurrent_runs*.json): 2 / 3 / 4 runs from
        # threads of one process = 1.40 / 1.56 / 1.38 x the throughput of one (3 is the sweet spot: a launch needs 537 of the
        # GPU's 768 workgroup slots, so launches of different problems overlap by their tails only).  One host thread per job;
        # ctypes releases the GIL inside the library.
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=a.jobs_per_gpu) as pool:
            res = list(pool.map(one, mine))
    else:
        res = [one(j) for j in mine]
    dt = time.perf_counter() - t0
    if dist is not None:
        gathered = [None] * world
        dist.all_gather_object(gathered, {"rank": rank, "seconds": dt, "results": res})
        dist.barrier()
        dist.destroy_process_group()
    else:
        gathered = [{"rank": 0, "seconds": dt, "results": res}]
    if rank == 0:
        allres = [r for g in gathered for r in g["results"]]
        wall = max(g["seconds"] for g in gathered)
        its = sum(r.get("newton_iterations", 0) for r in allres)
        print(json.dumps({"jobs": len(allres), "ok": sum(r["status"] == "ok" for r in allres), "world_size": world,
                          "wall_seconds": wall, "newton_iterations": its, "newton_iterations_per_sec": its / wall if wall else None,
                          "results": allres}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
