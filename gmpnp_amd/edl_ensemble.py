"""Many 1D EDL runs on one mesh in lock-step: the members' Newton solves run as ONE ensemble on the device
(``gmpnp_ensemble_newton_solve``: one launch chain per Newton iteration for all members, include/gmpnp.h).

Each member is an ordinary ``EDLRun`` (its own handle, model tables, Dirichlet values, state, clock and H_OHP controller);
per step the ensemble applies exactly the host glue of ``EDLRun.step`` to every member (``advance_clock`` before the solve,
``accept_solution`` after it, then ``u_n.assign(u)``), reads the state of all members with one copy, and freezes a member
whose solve fails with the error text the serial driver would raise, while the others carry on.  Outputs are the members'
own ``EDLRun.write_outputs`` / ``ohp_summary``.

``adaptive_dt=True`` on the ensemble: no lock-step; every member is its serial ADAPTIVE run on its own clock, and a step of the
ensemble is one round of ``timestep.EnsembleStepper``."""
from __future__ import annotations

import itertools

from . import backend
from .edl1d import EDLRun, run_identifier
from .impedance import refuse_impedance, refuse_pore_impedance
from .polarisation import refuse_polarisation
from .fit import refuse_fit
from .programme import refuse_pore_programme, refuse_programme
from .problem import refuse_galvanostat, refuse_kinetics, refuse_stern
from .params import edl_parameters
from .timestep import member_adaptive_keywords, refuse_ensemble_order2

# keyword surface of solve_EDL / EDLRun (reference 1D:66-79) and its defaults
MEMBER_DEFAULTS = {"concentration_elec": 0.1, "model": "MPNP", "voltage_multiplier": -1.0, "H2_FE": 0.2,
                   "mesh_structure": "variable", "current_OHP_ss": 10.0, "L_n": 50.0e-6, "stabilization": "N",
                   "H_OHP": None, "cation": "K", "params_file": "parameters", "dry_run": True}
# what every member of one ensemble must share: the mesh and the step schedule
SHARED_FIELDS = ("L_n", "mesh_structure", "params_file", "dry_run", "num_steps")


def sweep_members(voltages, cations=("K",), concentrations=(0.1,), **common):
    """Member keyword dicts of the Cartesian product, voltage outermost, then cation, then concentration."""
    return [dict(common, voltage_multiplier=float(v), cation=c, concentration_elec=float(x))
            for v, c, x in itertools.product(voltages, cations, concentrations)]


def plan_members(members, num_steps=None):
    """Validate the members of one ensemble before anything touches the device.  Returns (member kwargs with defaults
    filled in, their EDLParameters, the number of steps).  ValueError names the field that differs."""
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
        unknown = set(m) - set(MEMBER_DEFAULTS) - {"num_steps"}
        if unknown:
            raise TypeError("member %d: unknown keyword(s) %s" % (k, sorted(unknown)))
        d = dict(MEMBER_DEFAULTS)
        d.update(m)
        d.setdefault("num_steps", num_steps)
        if num_steps is not None and d["num_steps"] is None:
            d["num_steps"] = num_steps
        if d["stabilization"] == "Y" and d["model"] == "PNP":
            raise ValueError("member %d: stabilization='Y' with PNP (SUPG terms) is not supported in an ensemble" % k)
        full.append(d)
    eps = [edl_parameters(**{f: d[f] for f in MEMBER_DEFAULTS}) for d in full]
    for f in SHARED_FIELDS:
        vals = [bool(d[f]) if f == "dry_run" else d[f] for d in full]
        if f == "num_steps":
            vals = [ep.tot_num_steps if v is None else int(v) for v, ep in zip(vals, eps)]
        if any(v != vals[0] for v in vals):
            k = next(i for i, v in enumerate(vals) if v != vals[0])
            raise ValueError("ensemble members differ in %s: member 0 has %r, member %d has %r" % (f, vals[0], k, vals[k]))
    # (the scaled time steps themselves are per member: they follow the concentration through the Debye length)
    sched = [(ep.mesh_name, tuple(ep.stage_steps)) for ep in eps]
    if any(s != sched[0] for s in sched):
        raise ValueError("ensemble members differ in mesh or in the steps per stage of their schedule")
    steps = eps[0].tot_num_steps if full[0]["num_steps"] is None else int(full[0]["num_steps"])
    for d in full:
        d.pop("num_steps")
    return full, eps, steps


def member_identifier(kwargs):
    """The output directory name ``EDLRun.write_outputs`` gives a run with these keyword arguments."""
    d = dict(MEMBER_DEFAULTS)
    d.update(kwargs)
    d.pop("num_steps", None)
    return run_identifier(edl_parameters(**d), d)


def error_text(code, message):
    """The RuntimeError text ``GMPNPSystem.solve`` raises for a failed solve with this status."""
    if code == backend.ERR_NOT_CONVERGED:
        return "Newton solver did not converge because maximum number of iterations reached"
    return str(backend.GmpnpError(code, message))



class AdaptiveRounds:
    """The adaptive mode of ``EDLEnsemble`` / ``PoreEnsemble`` (``timestep.EnsembleStepper`` drives the members' own
    ``DriverStepping``): every member follows its own clock, a step of the ensemble is one round."""

    def start_adaptive(self, before_solve, before_accept):
        from .timestep import EnsembleStepper

        def after_attempt(k, row):
            r = self.runs[k]
            r.stepping.attempted(row)
            r.t = r.stepper.t
            if not self.keep_history:
                r.history = r.history[-1:]

        def on_error(k, code, message):
            self.errors[k], self.status[k], self.failed_step[k] = error_text(code, message), code, self.runs[k].n

        self.stepper = EnsembleStepper([r.stepper for r in self.runs], self._ensemble, self.opts,
                                       max_steps=[r.stepping.max_steps for r in self.runs], before_solve=before_solve,
                                       before_accept=before_accept, after_attempt=after_attempt, on_error=on_error)

    def adaptive_run(self):
        while self.stepper.live():
            self.stepper.round()
            self.n += 1
        return self


ADAPTIVE_REFUSAL = ("adaptive_dt: a member dict cannot ask for it; adaptive time stepping is requested on the ensemble "
                    "(adaptive_dt=True and the adaptive-stepping keywords there, a scalar or one value per member)")


class EDLEnsemble(AdaptiveRounds):
    """``members``: keyword dicts of ``EDLRun`` (voltage, cation, concentration, H2_FE, current_OHP_ss, H_OHP, model may
    differ; mesh and schedule may not).  ``keep_history=False`` keeps only the latest state of each member (long runs).
    ``budget=True``: every live member records its species-budget table after the step's solve, as its serial ``EDLRun`` twin does.
    ``step_fraction``: tau of the step limiter, for all members (each gets its own step length; 0 = off), as ``EDLRun`` takes it.
    ``adaptive_dt=True``: every member is its serial adaptive run (``EDLRun(adaptive_dt=True, ...)``) on its OWN clock, driven in
    rounds (``timestep.EnsembleStepper``: one ensemble Newton solve, one batched estimate and one batched accept / reject per
    round); the other adaptive-stepping keywords (``timestep.ADAPTIVE_KEYWORDS``) are scalars or sequences with one value per
    member.  Members stop at different rounds; ``run`` ends when all have.  Not with ``H_OHP``, as in the serial driver.
    ``solver_parameters``: the Newton parameters of every member (default: the driver's), as ``EDLRun`` takes them."""

    def __init__(self, members, num_steps=None, device_kwargs=None, keep_history=True, budget=False, step_fraction=0.0, adaptive_dt=False,
                 solver_parameters=None, **adaptive):
        members = [dict(m) for m in members]
        if any(m.get("adaptive_dt") for m in members):   # before anything touches the device
            raise ValueError(ADAPTIVE_REFUSAL)
        refuse_ensemble_order2(members, adaptive)
        self.adaptive = bool(adaptive_dt)
        per_member = member_adaptive_keywords(len(members), adaptive)
        if self.adaptive and any(m.get("H_OHP") is not None for m in members):
            raise ValueError("adaptive_dt: the H_OHP flux controller is calibrated per fixed step")
        self.kwargs, self.eps, self.tot_num_steps = plan_members(members, num_steps)
        self.keep_history = keep_history
        self.runs = []
        self._ens, self._ens_members = None, None
        self.stepper = None
        try:
            for kw, ad in zip(self.kwargs, per_member):
                extra = dict(ad, adaptive_dt=True) if self.adaptive else {}
                self.runs.append(EDLRun(num_steps=self.tot_num_steps, device_kwargs=device_kwargs, budget=budget, step_fraction=step_fraction,
                                        solver_parameters=solver_parameters, **extra, **kw))
        except BaseException:
            self.close()
            raise
        self.opts = backend.newton_options(self.runs[0].solver_parameters, dim=1)
        n = len(self.runs)
        self.errors = [None] * n        # RuntimeError text of a failed member
        self.status = [0] * n           # its gmpnp_status
        self.failed_step = [None] * n   # the step it failed at (frozen there)
        self.n = 0
        if self.adaptive:
            self.start_adaptive(lambda k, t, h: self.runs[k].adaptive_before_solve(t, h, verbose=False),
                                lambda k, st, u: self.runs[k].adaptive_before_accept(st, u.reshape(self.runs[k].sys.nv, self.runs[k].sys.nf),
                                                                                     verbose=False))

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
            self.runs[k].advance_clock(verbose=False)
        stats, codes, msgs = ens.newton_solve(self.opts)
        U = ens.get_state()
        ok = []
        for i, k in enumerate(live):
            r = self.runs[k]
            if codes[i] != backend.OK:
                self.errors[k], self.status[k], self.failed_step[k] = error_text(codes[i], msgs[i]), codes[i], r.n
                continue
            r.sys.record(stats[i])
            if r.budget is not None:   # before set_model / assign_previous, as EDLRun.step
                r.budget.take(r.sys)
            r.accept_solution(stats[i], U[i].reshape(r.sys.nv, r.sys.nf), verbose=False)
            ok.append((k, stats[i]))
        # u_n.assign(u) of the members whose solve succeeded (a failed one stays as its failed solve left it)
        if ok:
            self._ensemble([k for k, _ in ok]).assign_previous()
        for k, st in ok:
            r = self.runs[k]
            r.newton_its.append(st["iterations"])
            r.n += 1
            if not self.keep_history:
                r.history = r.history[-1:]
        self.n += 1

    def run(self):
        if self.stepper is not None:
            return self.adaptive_run()
        while self.n < self.tot_num_steps:
            self.step()
        return self

    def ohp_summary(self, k):
        return self.runs[k].ohp_summary()

    def identifiers(self):
        return [member_identifier(kw) for kw in self.kwargs]

    def write_outputs(self, stamp=None):
        """``EDLRun.write_outputs`` of every member that did not fail.  Members that would share a directory (they differ
        only in fields the reference leaves out of the name, e.g. the concentration) get the concentration appended to
        the stamp, then their index.  Returns per member the path, or the exception the member's write raised (the
        staged schedule ends with the reference's NameError)."""
        from datetime import datetime
        stamp = stamp or datetime.now().strftime("%y-%m-%d-%H-%M-%S")
        names = [(kw["model"], i) for kw, i in zip(self.kwargs, self.identifiers())]
        stamps = [stamp] * len(self.runs)
        if len(set(names)) < len(names):
            stamps = [stamp + "_c" + str(kw["concentration_elec"]) for kw in self.kwargs]
            if len(set(zip(names, stamps))) < len(names):
                stamps = [s + "_m%d" % k for k, s in enumerate(stamps)]
        out = []
        for k, r in enumerate(self.runs):
            if self.errors[k] is not None:
                out.append(None)
                continue
            try:
                out.append(r.write_outputs(stamps[k]))
            except NameError as e:
                out.append(e)
        return out

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
