"""Adaptive time stepping of ensembles, the host side (gmpnp_amd/timestep.py ``EnsembleStepper``; no GPU here): the round over fake
systems with scripted Newton outcomes and estimator values takes, member by member, the decisions and log rows of independent
``AdaptiveStepper``s fed the same script; the refusals that come before anything touches the device."""
import math

import pytest

from gmpnp_amd import backend
from gmpnp_amd.timestep import AdaptiveStepper, EnsembleStepper, TimeStepPolicy, member_adaptive_keywords


def stats(its):
    return {"iterations": its, "krylov_iterations": 3 * its, "steric_excursion": 0}


class Script:
    """One member's script: per attempt (status of the Newton solve, Newton iterations, err, rate, worst_dof); the attempt count
    picks the entry, so the serial stepper and the ensemble read the same values whatever step sizes they arrive with."""

    def __init__(self, entries):
        self.entries = entries

    def at(self, n):
        return self.entries[min(n, len(self.entries) - 1)]


class FakeSystem:
    """What ``AdaptiveStepper`` calls on a system, answered from the script; records the calls."""

    def __init__(self, script):
        self.script, self.n, self.calls, self.history, self.recorded = script, 0, [], False, []

    def set_time_step(self, inv_dt):
        self.calls.append(("set_time_step", inv_dt))

    def solve(self, solver_parameters=None):
        code, its, *_ = self.script.at(self.n)
        if code == backend.OK:
            self.record(stats(its))
            return stats(its)
        err = backend.GmpnpError(code, "scripted", stats(its))
        if code == backend.ERR_NOT_CONVERGED:
            raise RuntimeError("Newton solver did not converge because maximum number of iterations reached") from err
        raise err

    def record(self, st):
        self.recorded.append(st["iterations"])

    def estimate(self, h, h_prev):
        _, _, err, rate, dof = self.script.at(self.n)
        hist = self.history and h_prev > 0.0
        return {"err": err if hist else 0.0, "rate": rate, "worst_dof": dof if hist else -1, "has_history": hist, "nonfinite": False}

    def time_error(self, h, h_prev, rtol, atol):
        self.calls.append(("time_error", h, h_prev, rtol, atol))
        return self.estimate(h, h_prev)

    def time_accept(self):
        self.calls.append(("accept",))
        self.history = True
        self.n += 1

    def time_reject(self):
        self.calls.append(("reject",))
        self.n += 1


class FakeEnsemble:
    """``backend.DeviceEnsemble`` over fake systems: counts its calls, so that one round is seen to make one of each."""

    def __init__(self, systems, counter):
        self.systems, self.counter = systems, counter

    def set_time_step(self, inv_dts):
        self.counter["set_time_step"] += 1
        assert len(inv_dts) == len(self.systems)
        for s, x in zip(self.systems, inv_dts):
            s.set_time_step(x)

    def newton_solve(self, options):
        self.counter["newton_solve"] += 1
        out = [s.script.at(s.n) for s in self.systems]
        return [stats(o[1]) for o in out], [o[0] for o in out], ["" if o[0] == backend.OK else "scripted" for o in out]

    def time_error(self, h, h_prev, rtol, atol, mask=None):
        self.counter["time_error"] += 1
        res = []
        for k, s in enumerate(self.systems):
            if mask is not None and not mask[k]:
                res.append({"err": 0.0, "rate": 0.0, "worst_dof": 0, "has_history": False, "nonfinite": False})
            else:
                s.calls.append(("time_error", h[k], h_prev[k], rtol[k], atol[k]))
                res.append(s.estimate(h[k], h_prev[k]))
        return res

    def get_state(self):
        self.counter["get_state"] += 1
        return [("u", id(s)) for s in self.systems]

    def time_advance(self, actions):
        self.counter["time_advance"] += 1
        assert len(actions) == len(self.systems)
        for s, a in zip(self.systems, actions):
            if a == 1:
                s.time_accept()
            elif a == 2:
                s.time_reject()
            else:
                assert a == 0


OK, NC, NUM, LIN, HIP = backend.OK, backend.ERR_NOT_CONVERGED, backend.ERR_NUMERIC, backend.ERR_LINEAR, backend.ERR_HIP

# member -> (script, policy, rtol, max_steps)
MEMBERS = {
    # fails Newton twice (not converged, then a numeric failure) before its first accept, then a rejection by the error
    "fails_twice": (Script([(NC, 25, 0, 0, 0), (NUM, 3, 0, 0, 0), (OK, 6, 0.0, 5.0, 0), (OK, 5, 0.3, 4.0, 11), (OK, 5, 2.5, 3.0, 12),
                            (OK, 4, 0.6, 2.0, 13), (LIN, 2, 0, 0, 0), (OK, 4, 0.2, 1.0, 14)]),
                    TimeStepPolicy(), 1e-2, 9),
    # goes steady at its fourth attempt while the others go on
    "steady": (Script([(OK, 5, 0.0, 1.0, 0), (OK, 4, 0.5, 1e-3, 3), (OK, 3, 0.1, 1e-6, 4), (OK, 2, 0.01, 1e-7, 5), (OK, 2, 0.01, 1e-8, 6)]),
               TimeStepPolicy(steady_tol=1e-5), 5e-2, None),
    # stopped by max_steps = 5
    "max_steps": (Script([(OK, 5, 0.0, 1.0, 0), (OK, 4, 0.4, 1.0, 7), (OK, 4, 1.7, 1.0, 8), (OK, 4, 0.9, 1.0, 9)]), TimeStepPolicy(h_max=3.0), 1e-2, 5),
    # lands on t_end = 10 exactly
    "t_end": (Script([(OK, 5, 0.0, 1.0, 0), (OK, 4, 0.05, 1.0, 21)]), TimeStepPolicy(t_end=10.0), 1e-2, None),
}


def make(name):
    script, policy, rtol, _ = MEMBERS[name]
    sys_ = FakeSystem(script)
    return AdaptiveStepper(sys_, policy, (rtol, 1e-4), lambda h: 1.0 / (2.0 * h), 1.0, solver_parameters=None)


def serial(name):
    s = make(name)
    max_steps = MEMBERS[name][3]
    glue = []
    while s.stop_reason is None:
        if max_steps is not None and len(s.log) >= max_steps:
            s.stop_reason = "max_steps"
            break
        s.attempt(lambda t, h: glue.append(("solve", t, h)), lambda st: glue.append(("accept", st["iterations"])))
    return s, glue


def test_round_takes_the_serial_steppers_decisions():
    names = list(MEMBERS)
    steppers = [make(n) for n in names]
    counter = dict.fromkeys(("set_time_step", "newton_solve", "time_error", "get_state", "time_advance", "built"), 0)
    glue = {n: [] for n in names}
    lives = []

    def ensemble_of(live):
        counter["built"] += 1
        lives.append(list(live))
        return FakeEnsemble([steppers[k].sys for k in live], counter)

    es = EnsembleStepper(steppers, ensemble_of, None, max_steps=[MEMBERS[n][3] for n in names],
                         before_solve=lambda k, t, h: glue[names[k]].append(("solve", t, h)),
                         before_accept=lambda k, st, u: glue[names[k]].append(("accept", st["iterations"])))
    es.run()
    for k, n in enumerate(names):
        ref, ref_glue = serial(n)
        got = steppers[k]
        assert len(got.log) == len(ref.log) and all(_same_row(a, b) for a, b in zip(got.log, ref.log)), n
        assert (got.t, got.h, got.h_prev, got.steady_run, got.stop_reason) == (ref.t, ref.h, ref.h_prev, ref.steady_run, ref.stop_reason), n
        assert glue[n] == ref_glue, n
        assert got.sys.calls == ref.sys.calls and got.sys.recorded == ref.sys.recorded, n
    by = dict(zip(names, steppers))
    letters = "".join("A" if r["accepted"] else ("F" if r["reason"] == 2 else "R") for r in by["fails_twice"].log)
    assert letters == "FFAARAFAA" and by["fails_twice"].stop_reason == "max_steps"
    assert by["steady"].stop_reason == "steady" and len(by["steady"].log) == 4
    assert by["max_steps"].stop_reason == "max_steps" and len(by["max_steps"].log) == 5
    assert by["t_end"].stop_reason == "t_end" and by["t_end"].t == 10.0
    # one ensemble call of each kind per round, and the ensemble is asked for again as members leave
    rounds = es.rounds
    assert rounds == max(len(s.log) for s in steppers) == 9
    assert counter["set_time_step"] == counter["newton_solve"] == counter["time_advance"] == rounds
    assert counter["time_error"] <= rounds and counter["get_state"] <= rounds
    assert lives[0] == [0, 1, 2, 3] and lives[-1] == [0] and all(len(a) >= len(b) for a, b in zip(lives, lives[1:]))


def _same_row(a, b):
    return a.keys() == b.keys() and all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in a)


def test_a_member_with_another_status_ends_alone():
    """A HIP error is no failed attempt: the member stops with its message, the neighbours' logs are those of a run without it."""
    def run(with_bad):
        names = ["steady", "t_end"]
        steppers = [make(n) for n in names]
        if with_bad:
            bad = AdaptiveStepper(FakeSystem(Script([(OK, 5, 0.0, 1.0, 0), (HIP, 1, 0, 0, 0)])), TimeStepPolicy(), (1e-2, 1e-4), lambda h: 1.0 / h, 1.0)
            steppers.insert(1, bad)
        counter = dict.fromkeys(("set_time_step", "newton_solve", "time_error", "get_state", "time_advance"), 0)
        seen = []
        es = EnsembleStepper(steppers, lambda live: FakeEnsemble([steppers[k].sys for k in live], counter), None,
                             on_error=lambda k, code, msg: seen.append((k, code, msg)))
        es.run()
        return steppers, es, seen
    (a0, bad, a1), es, seen = run(True)
    (b0, b1), _, none = run(False)
    assert seen == [(1, HIP, "scripted")] and none == [] and es.errors == [None, "scripted", None] and es.status == [0, HIP, 0]
    assert len(bad.log) == 1 and bad.stop_reason is None and bad.sys.calls[-1][0] == "set_time_step"   # left as the failed solve left it
    for a, b in ((a0, b0), (a1, b1)):
        assert len(a.log) == len(b.log) and all(_same_row(x, y) for x, y in zip(a.log, b.log)) and a.stop_reason == b.stop_reason


def test_member_keywords():
    out = member_adaptive_keywords(3, dict(dt_rtol=[5e-2, 1e-2, 5e-2], steady_tol=1e-5, max_steps=(None, 12, 60)))
    assert out == [dict(dt_rtol=5e-2, steady_tol=1e-5, max_steps=None), dict(dt_rtol=1e-2, steady_tol=1e-5, max_steps=12),
                   dict(dt_rtol=5e-2, steady_tol=1e-5, max_steps=60)]
    with pytest.raises(ValueError, match="dt_rtol"):
        member_adaptive_keywords(3, dict(dt_rtol=[5e-2, 1e-2]))
    with pytest.raises(TypeError):
        member_adaptive_keywords(2, dict(dt_tolerance=1.0))


def test_refusals_before_the_device():
    from gmpnp_amd import sweep
    from gmpnp_amd.edl_ensemble import EDLEnsemble
    from gmpnp_amd.pore_ensemble import PoreEnsemble
    two = [dict(voltage_multiplier=-1.0, L_n=1e-6), dict(voltage_multiplier=-2.0, L_n=1e-6)]
    with pytest.raises(ValueError, match="steady_tol"):
        EDLEnsemble(two, adaptive_dt=True, steady_tol=[1e-5, 1e-5, 1e-5])
    with pytest.raises(ValueError, match="max_steps"):
        PoreEnsemble([dict(concentration_elec=0.5, L=10e-9, R=5e-9)], adaptive_dt=True, max_steps=[3, 4])
    with pytest.raises(ValueError, match="H_OHP"):
        EDLEnsemble([two[0], dict(two[1], H_OHP=0.5)], adaptive_dt=True)
    with pytest.raises(ValueError, match="--ensemble"):
        sweep.main(["--adaptive_dt", "--steady_tol", "1e-5"])
    # a member dict that asks for it: the existing ValueError, now pointing at the ensemble's keyword
    with pytest.raises(ValueError, match="adaptive_dt.*ensemble"):
        EDLEnsemble([two[0], dict(two[1], adaptive_dt=True)], adaptive_dt=True)
    with pytest.raises(ValueError, match="adaptive_dt.*ensemble"):
        PoreEnsemble([dict(concentration_elec=0.5, L=10e-9, R=5e-9, adaptive_dt=True)])


def test_the_sweep_parsers_take_the_flags():
    from gmpnp_amd import edl_sweep
    a = edl_sweep.build_parser().parse_args(["--voltage_multiplier", "-2.5", "-5", "--adaptive_dt", "--dt_rtol", "5e-2", "--steady_tol", "1e-5",
                                             "--t_end", "1e9", "--max_steps", "60"])
    assert a.adaptive_dt and a.dt_rtol == 5e-2 and a.steady_tol == 1e-5 and a.t_end == 1e9 and a.max_steps == 60
    assert math.isclose(edl_sweep.build_parser().parse_args(["--voltage_multiplier", "-1"]).dt_rtol, 1e-2)
