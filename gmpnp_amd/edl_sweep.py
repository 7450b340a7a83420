"""Sweep of the 1D EDL model (voltage x cation x concentration) as device ensembles (gmpnp_amd.edl_ensemble):

    python -m gmpnp_amd.edl_sweep --voltage_multiplier -2.5 -5 -7.5 -10 -12.5 --cation K Cs [--concentration_elec 0.1 0.5]
                                  [--staged] [--num_steps N] [--device_id D] [--step_fraction TAU]
                                  [--adaptive_dt --steady_tol TOL --t_end T ...]

The Cartesian product (voltage outermost, then cation, then concentration) runs as one ensemble, or as consecutive ensembles
of at most 64 members.  Every member writes the directory ``EDLRun.write_outputs`` writes (``1D/Stern_CO2ER.py --from_run``
reads it); ``ensemble_summary.json`` next to them has one row per member.  ``--staged`` runs the reference's two-stage
schedule (``--dry_run`` false), which ends every run with the reference's NameError: recorded per member.
``--adaptive_dt`` (with the flags of ``timestep.add_adaptive_arguments``): every member steps adaptively on its own clock until it
stops (end time, steady state, ``--max_steps``); its directory also gets ``timestep_log.npz`` and the adaptive metadata keys."""
from __future__ import annotations

import argparse
import json
import os
import sys
from datetime import datetime

from . import backend
from .edl1d import output_root
from .impedance import refuse_impedance, refuse_pore_impedance
from .polarisation import refuse_polarisation
from .fit import refuse_fit
from .programme import refuse_pore_programme, refuse_programme
from .problem import refuse_galvanostat, refuse_kinetics, refuse_stern
from .edl_ensemble import EDLEnsemble, sweep_members
from .timestep import adaptive_keywords, add_adaptive_arguments


def build_parser():
    p = argparse.ArgumentParser(description="1D EDL sweep as device ensembles")
    p.add_argument("--voltage_multiplier", nargs="+", type=float, required=True)
    p.add_argument("--cation", nargs="+", type=str, default=["K"])
    p.add_argument("--concentration_elec", nargs="+", type=float, default=[0.1])
    p.add_argument("--model", default="MPNP", type=str)
    p.add_argument("--mesh_structure", default="variable", type=str)
    p.add_argument("--H2_FE", default=0.2, type=float)
    p.add_argument("--current_OHP_ss", default=10.0, type=float)
    p.add_argument("--L_n", default=50e-6, type=float)
    p.add_argument("--H_OHP", default=None, type=float)
    p.add_argument("--params_file", default="parameters", type=str)
    p.add_argument("--staged", action="store_true", help="the reference's two-stage schedule instead of the dry run")
    p.add_argument("--num_steps", default=None, type=int, help="run only the first N steps")
    p.add_argument("--device_id", default=0, type=int)
    p.add_argument("--budget", action="store_true", help="record the species budgets of every step: budget.npz per member, the CO2 uptake in each row")
    p.add_argument("--step_fraction", default=0.0, type=float, help="fraction-to-boundary step limiter of the Newton updates: tau in (0, 1), 0 = off")
    add_adaptive_arguments(p)
    return p


def run_sweep(members, num_steps=None, device_id=0, stamp=None, log=None, budget=False, step_fraction=0.0, **adaptive):
    """Run the members in ensembles of at most backend.MAX_ENSEMBLE; returns (summary rows, path of ensemble_summary.json).
    ``adaptive``: the adaptive-stepping keywords of ``EDLEnsemble`` (scalars: the same for every member)."""
    for k, m in enumerate(members):
        refuse_impedance(m, "the ensemble sweep (member %d)" % k)
        refuse_pore_impedance(m, "the ensemble sweep (member %d)" % k)
        refuse_polarisation(m, "the ensemble sweep (member %d)" % k)
        refuse_fit(m, "the ensemble sweep (member %d)" % k)
        refuse_programme(m, "the ensemble sweep (member %d)" % k)
        refuse_pore_programme(m, "the ensemble sweep (member %d)" % k)
        refuse_galvanostat(m, "the ensemble sweep (member %d)" % k)
        refuse_stern(m, "the ensemble sweep (member %d)" % k)
        refuse_kinetics(m, "the ensemble sweep (member %d)" % k)
    refuse_impedance(adaptive, "the ensemble sweep")
    refuse_pore_impedance(adaptive, "the ensemble sweep")
    refuse_polarisation(adaptive, "the ensemble sweep")
    refuse_fit(adaptive, "the ensemble sweep")
    refuse_programme(adaptive, "the ensemble sweep")
    refuse_pore_programme(adaptive, "the ensemble sweep")
    refuse_galvanostat(adaptive, "the ensemble sweep")
    refuse_stern(adaptive, "the ensemble sweep")
    refuse_kinetics(adaptive, "the ensemble sweep")
    stamp = stamp or datetime.now().strftime("%y-%m-%d-%H-%M-%S")
    rows = []
    for c0 in range(0, len(members), backend.MAX_ENSEMBLE):
        chunk = members[c0:c0 + backend.MAX_ENSEMBLE]
        chunk_stamp = stamp if c0 == 0 else "%s_part%d" % (stamp, c0 // backend.MAX_ENSEMBLE)
        with EDLEnsemble(chunk, num_steps=num_steps, device_kwargs={"device_id": device_id}, budget=budget, step_fraction=step_fraction,
                         **adaptive) as ens:
            ens.run()
            ohp = [None if ens.errors[k] is not None else ens.ohp_summary(k) for k in range(len(ens))]
            paths = ens.write_outputs(chunk_stamp)
            for k, kw in enumerate(ens.kwargs):
                r = ens.runs[k]
                row = {"parameters": kw, "converged": ens.errors[k] is None, "error": ens.errors[k],
                       "failed_step": ens.failed_step[k], "newton_total": int(sum(r.newton_its)), "steps_run": int(r.n)}
                row.update(ohp[k] or {"field_OHP": None, "eps_rel_OHP": None, "potential_OHP": None})
                if r.stepper is not None:
                    row.update(stop_reason=r.stepper.stop_reason, steps_accepted=r.stepper.accepted, steps_rejected=r.stepper.rejected,
                               newton_failures=r.stepper.newton_failures, t_reached=r.stepper.t)
                if r.budget is not None:   # CO2 consumed at the OHP [mol / (m^2 s)], CO2 supplied by the bulk face, largest closure
                    row.update(r.budget.summary())
                p = paths[k]
                if isinstance(p, BaseException):
                    row["output_error"] = "%s: %s" % (type(p).__name__, p)
                    row["output"] = None
                else:
                    row["output"] = p
                rows.append(row)
                if log:
                    log("%s %s c=%s: %s" % (kw["voltage_multiplier"], kw["cation"], kw["concentration_elec"],
                                            row["error"] or "field_OHP %.6g" % row["field_OHP"]))
    model = members[0].get("model", "MPNP")
    where = os.path.join(output_root(), model, stamp + "_experiment")
    os.makedirs(where, exist_ok=True)
    path = os.path.join(where, "ensemble_summary.json")
    with open(path, "w") as fh:
        json.dump({"members": len(rows), "rows": rows}, fh, indent=1)
    return rows, path


def main(argv=None):
    a = build_parser().parse_args(argv)
    common = dict(model=a.model, mesh_structure=a.mesh_structure, H2_FE=a.H2_FE, current_OHP_ss=a.current_OHP_ss, L_n=a.L_n,
                  H_OHP=a.H_OHP, params_file=a.params_file, dry_run=not a.staged)
    members = sweep_members(a.voltage_multiplier, a.cation, a.concentration_elec, **common)
    if a.dt_order != 1:   # (before anything touches the device)
        from .timestep import ORDER2_ENSEMBLE_REFUSAL
        raise ValueError("--" + ORDER2_ENSEMBLE_REFUSAL)
    rows, path = run_sweep(members, num_steps=a.num_steps, device_id=a.device_id, log=lambda s: print(s, flush=True), budget=a.budget, step_fraction=a.step_fraction,
                           **(adaptive_keywords(a) if a.adaptive_dt else {}))
    print(path)
    return path


if __name__ == "__main__":
    sys.exit(0 if main() else 1)
