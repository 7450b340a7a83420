"""Many 3D pore runs on one mesh in lock-step: the members' Newton solves run as ONE ensemble on the device
(``gmpnp_ensemble_newton_solve``: one launch chain per Newton iteration for all members, include/gmpnp.h).

Each member is an ordinary ``PoreRun`` (its own handle, model tables, Dirichlet values, state and history), created with
``shared_device=1`` so that its handle keeps to one stream and the four-launch BiCGStab form.  Per step the ensemble applies
exactly the host glue of ``PoreRun.step`` to every member (medians -> Sechenov -> ``set_bcs``, CO2 minimum, history row), reads
the state of all members with one copy, assigns ``u_n`` of the members that succeeded with one launch, and freezes a member whose
solve fails with the error text the serial driver would raise, while the others carry on.

``adaptive_dt=True`` on the ensemble: no lock-step; every member is its serial ADAPTIVE run on its own clock, and a step of the
ensemble is one round of ``timestep.EnsembleStepper``."""
from __future__ import annotations

import numpy as np

from . import backend
from .edl_ensemble import ADAPTIVE_REFUSAL, AdaptiveRounds, error_text
from .pore3d import SOLVER_PARAMETERS, PoreRun
from .impedance import refuse_impedance, refuse_pore_impedance
from .polarisation import refuse_polarisation
from .fit import refuse_fit
from .programme import refuse_pore_programme, refuse_programme
from .problem import refuse_galvanostat, refuse_kinetics, refuse_stern
from .solver import column_medians
from .timestep import member_adaptive_keywords, refuse_ensemble_order2

# what may differ between the members of one ensemble (keywords of ``solveEDL``, reference 3D:96-113) and their defaults
MEMBER_DEFAULTS = {"concentration_elec": 1.0, "voltage_multiplier": -1.0, "cation": "K", "H2_FE": 0.05, "current_rough": 3000.0,
                   "roughness_factor": 150.0, "y_CO2": 0.95}
# what every member must share: the mesh, the weak form and the step schedule
SHARED_DEFAULTS = {"L": 100.0e-9, "R": 5.0e-9, "params_file": "parameters_pore", "as_published": False, "refine": 0, "num_steps": None}
SHARED_FIELDS = tuple(SHARED_DEFAULTS)
REFUSED = ("multilevel", "partition")   # PoreRun features an ensemble member cannot have


def plan_members(members, num_steps=None):
    """Validate the members of one ensemble before anything touches the device.  Returns (member kwargs of ``PoreRun`` with
    defaults filled in, the number of steps or None for the schedule's own).  ValueError names the first shared field that
    differs; ``multilevel`` and ``partition`` are refused."""
    members = list(members)
    if not 1 <= len(members) <= backend.MAX_ENSEMBLE:
        raise ValueError("an ensemble holds 1 ... %d members, not %d" % (backend.MAX_ENSEMBLE, len(members)))
    full = []
    for k, m in enumerate(members):
        refuse_impedance(m, "an ensemble (member %d)" % k)
        refuse_pore_impedance(m, "an ensemble (member %d)" % k)
        refuse_polarisation(m, "an ensemble (member %d)" % k)
        refuse_fit(m, "an ensemble (member %d)" % k)
        refuse_programme(m, "an ensemble (member %d)" % k)
        refuse_pore_programme(m, "an ensemble (member %d)" % k)
        refuse_galvanostat(m, "an ensemble (member %d)" % k)
        refuse_stern(m, "an ensemble (member %d)" % k)
        refuse_kinetics(m, "an ensemble (member %d)" % k)
        for f in REFUSED:
            if m.get(f):
                raise ValueError("member %d: %s is not supported in an ensemble" % (k, f))
        unknown = set(m) - set(MEMBER_DEFAULTS) - set(SHARED_DEFAULTS) - set(REFUSED)
        if unknown:
            raise TypeError("member %d: unknown keyword(s) %s" % (k, sorted(unknown)))
        d = dict(MEMBER_DEFAULTS)
        d.update(SHARED_DEFAULTS)
        d.update({f: v for f, v in m.items() if f not in REFUSED})
        if d["num_steps"] is None:
            d["num_steps"] = num_steps
        full.append(d)
    for f in SHARED_FIELDS:
        vals = [bool(d[f]) if f == "as_published" else d[f] for d in full]
        if any(v != vals[0] for v in vals):
            k = next(i for i, v in enumerate(vals) if v != vals[0])
            raise ValueError("ensemble members differ in %s: member 0 has %r, member %d has %r" % (f, vals[0], k, vals[k]))
    steps = full[0]["num_steps"]
    for d in full:
        d.pop("num_steps")
    return full, (None if steps is None else int(steps))


class PoreEnsemble(AdaptiveRounds):
    """``members``: keyword dicts of ``PoreRun`` (concentration, voltage, cation, H2_FE, current_rough, roughness_factor, y_CO2 may
    differ; mesh, weak form and schedule may not).  ``keep_history=False`` keeps only the latest row of each member (long runs).
    ``budget=True``: every live member records its species-budget table after the step's solve (the single-handle call per member:
    the members are ordinary handles), as its serial ``PoreRun`` twin does.
    ``adaptive_dt=True``: every member is its serial adaptive run (``PoreRun(adaptive_dt=True, ...)``) on its OWN clock, driven in
    rounds (``timestep.EnsembleStepper``); the other adaptive-stepping keywords are scalars or sequences with one value per member."""

    def __init__(self, members, num_steps=None, device_kwargs=None, keep_history=True, budget=False, step_fraction=0.0, adaptive_dt=False,
                 **adaptive):
        """``step_fraction`` other than 0 is refused (ValueError, before anything touches the device): 3D ensembles have no step limiter."""
        if step_fraction:
            raise ValueError("step_fraction: the step limiter is not available in a 3D ensemble")
        members = [dict(m) for m in members]
        if any(m.get("adaptive_dt") for m in members):   # before anything touches the device
            raise ValueError(ADAPTIVE_REFUSAL)
        refuse_ensemble_order2(members, adaptive)
        self.adaptive = bool(adaptive_dt)
        per_member = member_adaptive_keywords(len(members), adaptive)
        self.kwargs, steps = plan_members(members, num_steps)
        self.keep_history = keep_history
        self.runs = []
        self._ens, self._ens_members = None, None
        self.stepper = None
        dk = dict(device_kwargs or {}, shared_device=1)
        try:
            for kw, ad in zip(self.kwargs, per_member):
                extra = dict(ad, adaptive_dt=True) if self.adaptive else {}
                self.runs.append(PoreRun(num_steps=steps, device_kwargs=dk, budget=budget, **extra, **kw))
        except BaseException:
            self.close()
            raise
        self.tot_num_steps = self.runs[0].tot_num_steps
        self.opts = backend.newton_options(SOLVER_PARAMETERS, dim=3)
        n = len(self.runs)
        self.errors = [None] * n        # RuntimeError text of a failed member
        self.status = [0] * n           # its gmpnp_status
        self.failed_step = [None] * n   # the step it failed at (frozen there)
        self.n = 0
        if self.adaptive:
            self.start_adaptive(None, lambda k, st, u: self.runs[k].adaptive_before_accept(
                st, u.reshape(self.runs[k].sys.nv, self.runs[k].sys.nf).copy(), verbose=False))

    def __len__(self):
        return len(self.runs)

    def _ensemble(self, live):
        if self._ens_members != live:
            if self._ens is not None:
                self._ens.close()
            self._ens = backend.DeviceEnsemble([self.runs[k].sys.dev for k in live])
            self._ens_members = list(live)
        return self._ens

    def live(self):
        return [k for k in range(len(self.runs)) if self.errors[k] is None]

    def step(self):
        if self.stepper is not None:   # adaptive: one round, every live member attempts one step of its own size
            self.n += 1
            return self.stepper.round()
        live = self.live()
        if not live:
            self.n += 1
            return
        ens = self._ensemble(live)
        for k in live:
            self.runs[k].t += self.runs[k].pp.dt
        stats, codes, msgs = ens.newton_solve(self.opts)
        U = ens.get_state()
        ok = []
        for i, k in enumerate(live):
            r = self.runs[k]
            if codes[i] != backend.OK:
                self.errors[k], self.status[k], self.failed_step[k] = error_text(codes[i], msgs[i]), codes[i], r.n
                continue
            r.sys.record(stats[i])
            if r.budget is not None:   # before set_bcs / assign_previous, as PoreRun.step
                r.budget.take(r.sys)
            row = U[i].reshape(r.sys.nv, r.sys.nf).copy()
            r.accept_solution(stats[i], row, column_medians(row, (1, 2, 3, 7)), float(np.amin(row[:, 4])), assign=False)
            if not self.keep_history:
                r.history = r.history[-1:]
            ok.append(k)
        # u_n.assign(u) of the members whose solve succeeded (a failed one stays as its failed solve left it)
        if ok:
            self._ensemble(ok).assign_previous()
        self.n += 1

    def run(self):
        if self.stepper is not None:
            return self.adaptive_run()
        while self.n < self.tot_num_steps:
            self.step()
        return self

    def write_outputs(self, stamp=None):
        """``PoreRun.write_outputs`` of every member that did not fail; members get their index appended to the stamp (the
        reference's directory name leaves out fields that members may differ in).  Returns the paths (None: failed member)."""
        from datetime import datetime
        stamp = stamp or datetime.now().strftime("%y-%m-%d-%H-%M-%S")
        return [None if self.errors[k] is not None else r.write_outputs("%s_m%d" % (stamp, k)) for k, r in enumerate(self.runs)]

    def close(self):
        if self._ens is not None:
            self._ens.close()
            self._ens = None
        for r in self.runs:
            r.sys.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
