"""Potential programmes: the electrode potential follows a waveform in time (pulsed electrolysis, cyclic voltammetry, potential steps;
not a reference feature).  The rule is stated in C++ in csrc/gmpnp_host_rules.h ("potential programmes") and here
in Python, operation for operation (tests/test_programme_reference.py compiles that one with the host compiler alone and compares the
bits); ``run_programme`` is the loop over an ``ops`` object, as ``polarisation.run_continuation`` is: the same loop runs over a NumPy
system on the CPU (tests/programme_reference.py) and over a device handle (``DeviceProgrammeOps``).

A programme is a list of segments (t0, t1, p0, p1), t1 > t0, contiguous in time, p linear inside a segment.  A breakpoint where p1 of a
segment equals p0 of the next is a corner, otherwise a jump.  Times are in the driver's scaled time, potentials in thermal voltages
(as ``electrode_voltage``); seconds and a scan rate in V/s are converted at the driver boundary (``scaled_time``, ``scaled_scan_rate``)
with ``time_constant`` and ``thermal_voltage`` only."""
from __future__ import annotations

import dataclasses
import math
from dataclasses import dataclass

import numpy as np

from .timestep import next_time_step

MAX_SURFACE_REACTIONS = 4   # GMPNP_MAX_SURFACE_REACTIONS
STOP_REASONS = {0: "running", 1: "end", 2: "h_min"}
KINDS = ("pulse", "triangle", "table")


# ---- the rule (csrc/gmpnp_host_rules.h states it in C++, statement for statement) -------------------------------------------------------
def _finite(*vals):
    return all(math.isfinite(float(v)) for v in vals)


def programme_valid(segs):
    if len(segs) == 0:
        return False
    for k, (t0, t1, p0, p1) in enumerate(segs):
        if not _finite(t0, t1, p0, p1) or not t1 > t0:
            return False
        if k > 0 and t0 != segs[k - 1][1]:
            return False
    return True


def programme_jump(segs, k):
    """The breakpoint behind segment ``k`` is a jump (the end of the programme is neither a jump nor a corner)."""
    return k + 1 < len(segs) and segs[k][3] != segs[k + 1][2]


def programme_value(seg, t_end):
    """The potential of an implicit step that ENDS at ``t_end`` inside ``seg``: p1 itself at t_end == t1 (landed values are exact, as
    ``Continuation`` lands on its targets), else the interpolated sum.  A step never straddles a breakpoint."""
    t0, t1, p0, p1 = seg
    if t_end >= t1:
        return p1
    return p0 + (p1 - p0) * ((t_end - t0) / (t1 - t0))


def pulse(levels, durations, cycles, rise_time=0.0):
    """``cycles`` times the holds ``levels[k]`` for ``durations[k]``, from t = 0.  ``rise_time`` > 0 replaces each jump by a ramp of
    that length taken from the following hold (which must be longer)."""
    levels, durations = [float(v) for v in levels], [float(v) for v in durations]
    rise_time, n = float(rise_time), len(levels)
    if n == 0 or len(durations) != n or int(cycles) < 1 or not rise_time >= 0.0 or not _finite(rise_time):
        raise ValueError("programme: a pulse needs levels and as many durations, cycles >= 1 and a finite rise_time >= 0")
    if not all(_finite(lv, d) and d > rise_time for lv, d in zip(levels, durations)):
        raise ValueError("programme: a pulse needs finite levels and finite durations, every duration above the rise_time")
    out, t, last = [], 0.0, levels[0]
    for _ in range(int(cycles)):
        for lv, d in zip(levels, durations):
            end, t_hold = t + d, t
            if rise_time > 0.0 and lv != last:
                t_hold = t + rise_time
                out.append((t, t_hold, last, lv))
            out.append((t_hold, end, lv, lv))
            t, last = end, lv
    return out


def triangle(v_start, v_vertex, scan_rate, cycles):
    """``cycles`` times v_start -> v_vertex -> v_start at ``scan_rate`` > 0 (potential per time), from t = 0: corners only."""
    v_start, v_vertex, scan_rate = float(v_start), float(v_vertex), float(scan_rate)
    if not _finite(v_start, v_vertex, scan_rate) or not scan_rate > 0.0 or int(cycles) < 1 or v_start == v_vertex:
        raise ValueError("programme: a triangle needs finite v_start != v_vertex, a finite scan_rate > 0 and cycles >= 1")
    leg = abs(v_vertex - v_start) / scan_rate
    if not leg > 0.0 or not _finite(leg):
        raise ValueError("programme: the legs of the triangle have no finite positive duration")
    out, t = [], 0.0
    for _ in range(int(cycles)):
        mid = t + leg
        end = mid + leg
        out.append((t, mid, v_start, v_vertex))
        out.append((mid, end, v_vertex, v_start))
        t = end
    return out


def table(times, potentials):
    """Straight lines through (times[k], potentials[k]); a time given twice in a row is a jump there (never three times, and not at
    either end)."""
    times, potentials = [float(v) for v in times], [float(v) for v in potentials]
    n = len(times)
    bad = ValueError("programme: a table needs >= 2 finite points with times that do not decrease (a time given twice is a jump)")
    if n < 2 or len(potentials) != n or not _finite(*times) or not _finite(*potentials):
        raise bad
    out = []
    for k in range(n - 1):
        if times[k + 1] == times[k]:
            if k == 0 or k + 2 >= n or times[k + 2] == times[k]:
                raise bad
            continue
        if not times[k + 1] > times[k]:
            raise bad
        out.append((times[k], times[k + 1], potentials[k], potentials[k + 1]))
    return out


@dataclass
class ProgrammeWalk:
    seg: int = 0
    t: float = 0.0
    h: float = 0.0
    h_prev: float = 0.0
    steady_run: int = 0
    stop: int = 0          # 0 running, 1 the end was reached, 2 h_min


def programme_break(segs, seg, run_end):
    """t_end of the policy handed to ``next_time_step``: the smaller of the segment's end and the run's end."""
    return segs[seg][1] if segs[seg][1] < run_end else run_end


def programme_clip(h, t, t_break):
    """``next_time_step``'s landing applied to a step that starts a segment: cut, or stretched by at most 1 %, to end on the
    breakpoint."""
    left = t_break - t
    return left if left <= 1.01 * h else h


def programme_step_end(t, h, t_break):
    """Where the attempt (t, h) ends: the breakpoint itself where ``next_time_step`` will say the step landed on it."""
    nxt = t + h
    left = t_break - nxt
    return nxt if left > 1e-12 * abs(t_break) else t_break


def programme_begin(segs, dt_init, run_end):
    w = ProgrammeWalk(t=segs[0][0])
    w.h = programme_clip(dt_init, w.t, programme_break(segs, 0, run_end))
    return w


def programme_after(segs, w, d, h_done, dt_restart, run_end):
    """The walk after the decision ``d`` of an attempt of step ``h_done``: True where the accepted step landed on a breakpoint or on
    the end.  A stop_end at a breakpoint that is not the end moves to the next segment and does not stop; behind a jump the next
    attempt is a first step (h = dt_restart, h_prev = 0), behind a corner nothing is reset; a failed or rejected attempt stays in its
    segment with the controller's smaller step."""
    w.steady_run = d.steady_run
    w.t, w.h = d.t_next, d.h_next
    if not d.accept or not d.stop_end:
        if d.accept:
            w.h_prev = h_done
        if d.give_up:
            w.stop = 2
        return False
    w.h_prev = h_done
    if w.seg + 1 >= len(segs) or not segs[w.seg][1] < run_end:
        w.stop = 1
        return True
    jump = programme_jump(segs, w.seg)
    w.seg += 1
    if jump:
        w.h, w.h_prev = dt_restart, 0.0
    w.h = programme_clip(w.h, w.t, programme_break(segs, w.seg, run_end))
    return True


def programme_fixed_step(seg, n):
    """Fixed mode: every step of a segment is (t1 - t0) / n long and the last one lands on t1."""
    return (seg[1] - seg[0]) / n


def fixed_step_times(segs, n):
    """The step ends of ``run_programme``'s fixed mode, by its own arithmetic (t + h, the last step of a segment on t1 itself)."""
    out = []
    for seg in segs:
        h, t = programme_fixed_step(seg, n), seg[0]
        for j in range(n):
            t = seg[1] if j == n - 1 else t + h
            out.append(t)
    return out


def electrode_record_combine(acc, h, D, I):
    """The combine step of one electrode record (``gmpnp_electrode_trace_append``), every product, quotient and sum rounded on its own:
    ``acc`` = dict(D_prev, Q (4,), Q_D) is updated in place; returns dD_dt."""
    h, D = float(h), float(D)
    dD_dt = (D - acc["D_prev"]) / h
    for r in range(MAX_SURFACE_REACTIONS):
        acc["Q"][r] = acc["Q"][r] + h * float(I[r])
    acc["Q_D"] = acc["Q_D"] + h * dD_dt
    acc["D_prev"] = D
    return dD_dt


def fresh_accumulators(D):
    return {"D_prev": float(D), "Q": [0.0] * MAX_SURFACE_REACTIONS, "Q_D": 0.0}


# ---- the wall profile's rule (csrc/gmpnp_host_rules.h "wall profile", statement for statement) -----------------------------------------------
WALL_PROFILE_MAX_BINS = 256   # GMPNP_WALL_PROFILE_MAX_BINS


def wall_bin(z, edges, n):
    """The axial bin of ``z`` among the n + 1 ascending ``edges``, by comparisons only: the largest b with edges[b] <= z; z == edges[n]
    goes to bin n - 1; z outside [edges[0], edges[n]] (or NaN) is bin -1 and belongs to no bin."""
    if not z >= edges[0] or not z <= edges[n]:
        return -1
    b = 0
    for k in range(1, n):
        if edges[k] <= z:
            b = k
    return b


def wall_bins_valid(edges, n):
    if n < 1 or n > WALL_PROFILE_MAX_BINS or edges is None or len(edges) != n + 1:
        return False
    if not all(math.isfinite(float(e)) for e in edges):
        return False
    return all(edges[k] < edges[k + 1] for k in range(n))


def uniform_edges(z_lo, z_hi, n):
    """n equal bins over [z_lo, z_hi]: z_lo + (z_hi - z_lo) * (k / n), every operation rounded on its own; the last edge is z_hi."""
    z_lo, z_hi = float(z_lo), float(z_hi)
    return [z_lo + (z_hi - z_lo) * (float(k) / float(n)) for k in range(n)] + [z_hi]


def wall_profile_charge(Q, h, I):
    """The charge statement of ``electrode_record_combine`` for one bin: Q[r] + h I[r], product and sum rounded on their own."""
    return [float(Q[r]) + float(h) * float(I[r]) for r in range(MAX_SURFACE_REACTIONS)]


def wall_bin_lists(z, edges):
    """The positions (ascending) of the values ``z`` in every bin of ``edges``: what ``gmpnp_wall_profile_open`` uploads as a CSR."""
    n = len(edges) - 1
    out = [[] for _ in range(n)]
    for k, zk in enumerate(z):
        b = wall_bin(float(zk), edges, n)
        if b >= 0:
            out[b].append(k)
    return out


def resolve_bins(bins, z_wall, L):
    """The edges (units of L) of a driver's ``bins``: a count, uniform over the z range of the wall nodes ``z_wall`` (units of L), or
    explicit edges in metres.  ValueError (``pore_programme``) where they are not valid or a bin holds no wall node."""
    if np.ndim(bins) == 0:
        check_bins(bins)
        edges = uniform_edges(float(np.min(z_wall)), float(np.max(z_wall)), int(bins))
    else:
        edges = [float(e) / float(L) for e in bins]
    n = len(edges) - 1
    if not wall_bins_valid(edges, n):
        raise ValueError("pore_programme: bins is a count 1 ... %d or finite, strictly ascending edges [m]" % WALL_PROFILE_MAX_BINS)
    for b, members in enumerate(wall_bin_lists(z_wall, edges)):
        if not members:
            raise ValueError("pore_programme: bin %d of %d holds no node of the wall: ask for fewer bins" % (b, n))
    return edges


def check_bins(bins):
    """The part of ``resolve_bins`` that needs no mesh (before anything touches the device)."""
    bad = ValueError("pore_programme: bins is a count 1 ... %d or finite, strictly ascending edges [m]" % WALL_PROFILE_MAX_BINS)
    if isinstance(bins, (bool, str)) or bins is None:
        raise bad
    if np.ndim(bins) == 0:
        if not float(bins).is_integer() or not 1 <= int(bins) <= WALL_PROFILE_MAX_BINS:
            raise bad
        return
    edges = [float(e) for e in np.asarray(bins, dtype=np.float64).ravel()]
    if np.ndim(bins) != 1 or not wall_bins_valid(edges, len(edges) - 1):
        raise bad


# ---- the loop ------------------------------------------------------------------------------------------------------------------------------
LOG_COLUMNS = ("t", "h", "accepted", "reason", "err", "newton", "segment", "potential", "restart")


def run_programme(ops, segs, policy=None, dt_init=None, dt_restart=None, steps_per_segment=None, run_end=math.inf, max_attempts=None):
    """Marches ``ops`` through the programme ``segs`` and returns dict(log, times, potentials, segments, breakpoints, stop_reason).
    ``ops`` supplies the operations of a handle:

        set_potential(p)               p_M = p exactly
        set_step(h)                    the time step of the next solve
        solve() -> (converged, iterations)
        estimate(h, h_prev) -> dict    the error estimator's report (err, rate, has_history) of the converged solve (adaptive mode)
        record(t, h, seg, p)           the accepted step's record (one trace append), while u_n is still the previous state
        accept() / reject()            u_n <- u with the history shifted / u <- u_n
        breakpoint(seg, t)             the accepted step landed on the end of segment ``seg``: the full state may be kept

    Adaptive mode (``policy``, a ``TimeStepPolicy``; ``dt_init``; ``dt_restart`` defaults to it): every attempt is judged by
    ``next_time_step`` with a copy of the policy whose t_end is the next breakpoint (or ``run_end``) and no steady stop, so steps land on
    the breakpoints; the potential of an attempt is ``programme_value`` at its end, evaluated again when a failed or rejected attempt
    retries with the controller's smaller step.  Fixed mode (``steps_per_segment`` = N): N equal steps per segment, no estimator; a
    Newton failure is a RuntimeError."""
    segs = [tuple(float(v) for v in s) for s in segs]
    if not programme_valid(segs):
        raise ValueError("programme: segments (t0, t1, p0, p1) with t1 > t0, finite values, contiguous in time")
    log, times, pots, seg_of, breaks = [], [], [], [], []

    def row(t, h, ok, reason, err, its, seg, p, restart):
        return {"t": t, "h": h, "accepted": bool(ok), "reason": int(reason), "err": err, "newton": int(its), "segment": int(seg),
                "potential": p, "restart": bool(restart)}

    if steps_per_segment is not None:
        n = int(steps_per_segment)
        if n < 1:
            raise ValueError("programme: steps_per_segment must be at least 1")
        for k, seg in enumerate(segs):
            h, t = programme_fixed_step(seg, n), seg[0]
            for j in range(n):
                t_new = seg[1] if j == n - 1 else t + h
                p = programme_value(seg, t_new)
                ops.set_potential(p)
                ops.set_step(h)
                ok, its = ops.solve()
                if not ok:
                    raise RuntimeError("programme: the Newton solve of a fixed step did not converge (segment %d, t = %g)" % (k, t_new))
                ops.record(t_new, h, k, p)
                ops.accept()
                log.append(row(t, h, True, 0, math.nan, its, k, p, False))
                times.append(t_new); pots.append(p); seg_of.append(k)
                t = t_new
            ops.breakpoint(k, seg[1])
            breaks.append(seg[1])
        return {"log": log, "times": times, "potentials": pots, "segments": seg_of, "breakpoints": breaks, "stop_reason": "end"}

    if policy is None or dt_init is None:
        raise ValueError("programme: the adaptive mode needs a policy and dt_init (or give steps_per_segment)")
    dt_init = float(dt_init)
    dt_restart = dt_init if dt_restart is None else float(dt_restart)
    if not (dt_init > 0.0 and dt_restart > 0.0 and _finite(dt_init, dt_restart)):
        raise ValueError("programme: dt_init and dt_restart must be finite and > 0")
    w = programme_begin(segs, dt_init, run_end)
    stop = None
    while w.stop == 0:
        if max_attempts is not None and len(log) >= max_attempts:
            stop = "max_steps"
            break
        if not w.h > 0.0:   # (h_min = 0 never gives up: a step that has shrunk to nothing ends the run all the same)
            stop = "h_min"
            break
        k, t, h, first = w.seg, w.t, w.h, w.h_prev == 0.0   # first: a first step (the start, or behind a jump): no estimate
        t_break = programme_break(segs, k, run_end)
        p = programme_value(segs[k], programme_step_end(t, h, t_break))
        ops.set_potential(p)
        ops.set_step(h)
        ok, its = ops.solve()
        est = ops.estimate(h, w.h_prev) if ok else None
        err = est["err"] if est else 0.0
        pol = dataclasses.replace(policy, t_end=t_break, steady_tol=0.0)
        d = next_time_step(pol, t, h, err, bool(est and est["has_history"]), not ok, est["rate"] if est else math.inf, w.steady_run)
        if d.accept:
            ops.record(d.t_next, h, k, p)
            ops.accept()
            times.append(d.t_next); pots.append(p); seg_of.append(k)
        else:
            ops.reject()
        log.append(row(t, h, d.accept, d.reason, err if est else math.nan, its, k, p, first))
        landed = programme_after(segs, w, d, h, dt_restart, run_end)
        if landed:
            ops.breakpoint(k, d.t_next)
            breaks.append(d.t_next)
    return {"log": log, "times": times, "potentials": pots, "segments": seg_of, "breakpoints": breaks,
            "stop_reason": stop or STOP_REASONS[w.stop]}


def log_arrays(log):
    """The log as arrays by column (the rows ``timestep_log.npz`` gains)."""
    out = {}
    for c in LOG_COLUMNS:
        kind = np.float64 if c in ("t", "h", "err", "potential") else (np.bool_ if c in ("accepted", "restart") else np.int64)
        out[c] = np.array([r[c] for r in log], dtype=kind)
    return out


# ---- units and keywords of the drivers ----------------------------------------------------------------------------------------------------
def scaled_time(seconds, time_constant):
    return float(seconds) / float(time_constant)


def scaled_scan_rate(volts_per_second, time_constant, thermal_voltage):
    """V/s -> thermal voltages per scaled time."""
    return float(volts_per_second) * float(time_constant) / float(thermal_voltage)


def build(par, electrode_voltage, time_constant, thermal_voltage):
    """The segments of a driver's ``programme`` keyword (``check_programme``'d): durations, rise time and table times in seconds, the scan
    rate in V/s, potentials in thermal voltages; a triangle starts at ``electrode_voltage``."""
    kind = par["kind"]
    if kind == "pulse":
        return pulse(par["v_levels"], [scaled_time(d, time_constant) for d in par["durations"]], par.get("cycles", 1),
                     scaled_time(par.get("rise_time", 0.0), time_constant))
    if kind == "triangle":
        return triangle(electrode_voltage, par["v_vertex"], scaled_scan_rate(par["scan_rate"], time_constant, thermal_voltage), par.get("cycles", 1))
    return table([scaled_time(t, time_constant) for t in par["time_s"]], par["electrode_voltage"])


PROGRAMME_FIELDS = {"pulse": ({"v_levels", "durations"}, {"cycles", "rise_time"}), "triangle": ({"v_vertex", "scan_rate"}, {"cycles"}),
                    "table": ({"time_s", "electrode_voltage"}, set())}
COMMON_FIELDS = {"kind", "dt_init", "dt_restart", "steps_per_segment", "capacity", "sensitivities", "sensitivity_start", "periodic"}


def sensitivity_codes(names):
    """The tangent's parameter codes of the names of ``fit.PARAMETERS`` plus "offset" (a potential offset of the whole waveform, code
    0): no new codes.  ValueError for an unknown or repeated name, none or more than ten."""
    from .fit import PARAMETERS
    names = [str(n) for n in names]
    known = dict(PARAMETERS, **{OFFSET: 0})
    bad = [n for n in names if n not in known]
    if bad:
        raise ValueError("programme: unknown sensitivity parameter %s (known: %s)" % (bad[0], ", ".join(sorted(known))))
    if len(set(names)) != len(names):
        raise ValueError("programme: a sensitivity parameter is repeated")
    if not 1 <= len(names) <= 10:
        raise ValueError("programme: 1 ... 10 sensitivity parameters")
    return [known[n] for n in names]


def check_programme(par, kwargs, dt_order=1):
    """The refusals of a driver's ``programme`` keyword, before anything touches the device; returns the checked dict."""
    par = dict(par)
    kind = par.get("kind")
    if kind not in KINDS:
        raise ValueError("programme: the keyword is dict(kind='pulse' | 'triangle' | 'table', ...)")
    need, may = PROGRAMME_FIELDS[kind]
    if not need <= set(par) or set(par) - need - may - COMMON_FIELDS:
        raise ValueError("programme: a %s takes %s%s and dt_init, dt_restart, steps_per_segment, capacity" %
                         (kind, sorted(need), (" " + str(sorted(may))) if may else ""))
    if kwargs.get("electrode_voltage") is None:
        raise ValueError("programme: a potential programme needs an electrode potential (electrode_voltage)")
    if kwargs.get("target_current") is not None:
        raise ValueError("programme: not available with target_current (the galvanostat owns the potential)")
    if kwargs.get("polarisation") or kwargs.get("fit"):
        raise ValueError("programme: not in one run with polarisation or fit (each leaves the run at a potential of its own)")
    if kwargs.get("stabilization", "N") == "Y":
        raise ValueError("programme: not available with stabilization Y")
    if kwargs.get("H_OHP") is not None:
        raise ValueError("programme: not available with the H_OHP flux controller")
    if int(dt_order) == 2:
        raise ValueError("programme: not available with dt_order 2")
    for key in ("dt_init", "dt_restart"):
        if par.get(key) is not None and not (_finite(par[key]) and float(par[key]) > 0.0):
            raise ValueError("programme: %s must be finite and > 0" % key)
    if par.get("steps_per_segment") is not None and int(par["steps_per_segment"]) < 1:
        raise ValueError("programme: steps_per_segment must be at least 1")
    if par.get("capacity") is not None and int(par["capacity"]) < 1:
        raise ValueError("programme: capacity must be at least 1")
    if par.get("sensitivities"):
        codes = sensitivity_codes(par["sensitivities"])
        if kwargs.get("kinetics") is None and any(16 <= c < 48 for c in codes):
            raise ValueError("programme: the sensitivity to a kinetic parameter needs the surface kinetics (kinetics='tafel')")
    if par.get("sensitivity_start") is not None:
        if not par.get("sensitivities"):
            raise ValueError("programme: sensitivity_start without sensitivities")
        if par["sensitivity_start"] not in ("steady", "zero"):
            raise ValueError("programme: sensitivity_start is 'steady' or 'zero'")
    if par.get("periodic") is not None and par.get("periodic") is not False:   # the limit cycle in the place of a march (section 5r)
        from .periodic import check_periodic
        check_periodic(par["periodic"], par)
    build(par, float(kwargs["electrode_voltage"]), 1.0, 1.0)   # a waveform that is not valid is refused here (the units do not matter)
    return par


def refuse_programme(kwargs, what):
    """ValueError where ``kwargs`` asks for a potential programme (``programme``) in a driver that has none."""
    if kwargs.get("programme"):
        raise ValueError("programme: potential programmes are not available in %s" % what)


def add_programme_arguments(p):
    p.add_argument("--programme", required=False, default=None, choices=KINDS,
                   help="(addition) potential programme after the run's own schedule, from its last state (programme.npz)")
    p.add_argument("--v_levels", required=False, default=None, type=float, nargs="+", help="(addition) levels of --programme pulse [thermal voltages]")
    p.add_argument("--durations", required=False, default=None, type=float, nargs="+", help="(addition) hold times of --programme pulse [s]")
    p.add_argument("--cycles", required=False, default=1, type=int, help="(addition) cycles of --programme pulse / triangle")
    p.add_argument("--rise_time", required=False, default=0.0, type=float, help="(addition) ramp in place of each jump of --programme pulse [s]")
    p.add_argument("--v_vertex", required=False, default=None, type=float, help="(addition) vertex potential of --programme triangle [thermal voltages]")
    p.add_argument("--scan_rate", required=False, default=None, type=float, help="(addition) scan rate of --programme triangle [V/s]")
    p.add_argument("--programme_file", required=False, default=None, type=str, help="(addition) CSV of --programme table: columns time_s, electrode_voltage")
    p.add_argument("--programme_dt_init", required=False, default=None, type=float, help="(addition) first step of the programme and after a jump (scaled time)")
    p.add_argument("--programme_steps_per_segment", required=False, default=None, type=int, help="(addition) fixed mode: equal steps per segment, no estimator")
    p.add_argument("--programme_sensitivities", required=False, default=None, type=str, nargs="+", metavar="NAMES",
                   help="(addition) carry the transient sensitivities to these parameters (i0_CO, i0_H2, alpha_CO, alpha_H2, stern_length, offset) "
                        "through the programme (programme_sensitivity.npz)")
    p.add_argument("--programme_sensitivity_start", required=False, default=None, choices=("steady", "zero"),
                   help="(addition) the sensitivities start from the steady state's dependence on the parameters (default) or from zero")
    p.add_argument("--programme_periodic", required=False, default=False, action="store_true",
                   help="(addition) look for the limit cycle of ONE period of the waveform by Anderson acceleration of the cycle map "
                        "(needs --programme_steps_per_segment; programme.npz holds the converged period, programme_periodic.npz the search)")
    p.add_argument("--periodic_tol", required=False, default=None, type=float, help="(addition) the cycle is converged at a weighted residual <= this (default 1)")
    p.add_argument("--periodic_depth", required=False, default=None, type=int, help="(addition) differences of a full Anderson window, 1 ... 8 (default 4)")
    p.add_argument("--periodic_max_cycles", required=False, default=None, type=int, help="(addition) cycles marched at the most (default 50)")


def load_table(path):
    """(time_s, electrode_voltage) of a CSV file with those two named columns."""
    data = np.genfromtxt(path, delimiter=",", names=True, dtype=np.float64)
    names = data.dtype.names or ()
    if "time_s" not in names or "electrode_voltage" not in names:
        raise ValueError("programme: %s needs the columns time_s and electrode_voltage" % path)
    return np.atleast_1d(data["time_s"]).tolist(), np.atleast_1d(data["electrode_voltage"]).tolist()


def programme_keywords(a):
    """The programme keyword of a parsed command line (``add_programme_arguments``); empty without --programme."""
    periodic = {k: getattr(a, "periodic_" + k) for k in ("tol", "depth", "max_cycles") if getattr(a, "periodic_" + k, None) is not None}
    if periodic and not getattr(a, "programme_periodic", False):
        raise ValueError("programme: --periodic_tol, --periodic_depth and --periodic_max_cycles need --programme_periodic")
    if a.programme is None:
        if getattr(a, "programme_sensitivities", None) or getattr(a, "programme_sensitivity_start", None):
            raise ValueError("programme: --programme_sensitivities and --programme_sensitivity_start need --programme")
        if getattr(a, "programme_periodic", False):
            raise ValueError("programme: --programme_periodic needs --programme")
        return {}
    par = {"kind": a.programme}
    if a.programme == "pulse":
        if a.v_levels is None or a.durations is None:
            raise ValueError("programme: --programme pulse needs --v_levels and --durations")
        par.update(v_levels=list(a.v_levels), durations=list(a.durations), cycles=a.cycles, rise_time=a.rise_time)
    elif a.programme == "triangle":
        if a.v_vertex is None or a.scan_rate is None:
            raise ValueError("programme: --programme triangle needs --v_vertex and --scan_rate")
        par.update(v_vertex=a.v_vertex, scan_rate=a.scan_rate, cycles=a.cycles)
    else:
        if a.programme_file is None:
            raise ValueError("programme: --programme table needs --programme_file")
        t, v = load_table(a.programme_file)
        par.update(time_s=t, electrode_voltage=v)
    if a.programme_dt_init is not None:
        par["dt_init"] = a.programme_dt_init
    if a.programme_steps_per_segment is not None:
        par["steps_per_segment"] = a.programme_steps_per_segment
    if getattr(a, "programme_sensitivities", None):
        par["sensitivities"] = list(a.programme_sensitivities)
    if getattr(a, "programme_sensitivity_start", None):
        par["sensitivity_start"] = a.programme_sensitivity_start
    if getattr(a, "programme_periodic", False):
        par["periodic"] = periodic
    return {"programme": par}


# ---- the operations of a device handle and the outputs of the 1D driver ------------------------------------------------------------------
class RecordStream:
    """One device buffer of per-step records behind ``DeviceProgrammeOps``: ``calls`` = the handle's bound (open, append, read, close),
    the list its chunks go to, the array that stands for no record, the arguments in front of the capacity at the first open and at an
    open behind a drained buffer, and ``carry``: the fields whose sums start at 0 with every open, each with the field it sums.  Behind
    a drained buffer the host goes on with the device's own statement, sum <- sum + h * rate (``electrode_record_combine``,
    ``wall_profile_charge``: product and sum rounded on their own, one record after the other), from the last sum of the chunk before,
    so the records are those of a buffer that was never drained, bit for bit.  (The chunk's sums added to the carried one as a whole
    round differently from its second record on.)"""

    def __init__(self, calls, chunks, empty, args=(), reopen_args=None, carry=None):
        self.open, self.append, self.read, self.close = calls
        self.chunks, self.empty, self.carry, self.base = chunks, empty, carry or {}, {}
        self.args, self.reopen_args = args, args if reopen_args is None else reopen_args

    def drain(self, count):
        rec = self.read(0, count)
        for f, rate in self.carry.items():
            if f in self.base:
                h = rec["h"].reshape(rec["h"].shape + (1,) * (rec[rate].ndim - rec["h"].ndim))
                rec[f] = np.add.accumulate(np.concatenate([self.base[f][None], h * rec[rate]]))[1:]   # (accumulate: strictly in order)
            self.base[f] = rec[f][-1].copy()
        self.chunks.append(rec)

    def records(self):
        return np.concatenate(self.chunks) if self.chunks else self.empty


class DeviceProgrammeOps:
    """What ``run_programme`` asks of a system, over a driver run (``EDLRun``: its ``sys``, ``stern``, ``kinetics``, ``budget``) and its
    device handle.  Per accepted step one ``electrode_trace_append`` (no synchronisation, no copy) and, with ``budget``, one row of the
    budget log; the trace is read when its ``capacity`` records are written and at the end (``drain``), so the host keeps the records
    and the states at the breakpoints, not a state per step.  The accumulated charges go on across a drained buffer: the host continues
    the device's sums from what the records before held (``RecordStream``)."""

    def __init__(self, run, solver_parameters, inv_dt_of_h, tol=(1e-2, 1e-4), capacity=4096, sensitivities=None, sensitivity_start="zero",
                 after_accept=None, profile_edges=None, cycle_tol=(1e-2, 1e-4)):
        """``after_accept`` (the pore driver's Sechenov glue; the 1D path passes none): called once per accepted step, in front of
        ``time_accept``; a rejected attempt never reaches it.  ``profile_edges`` (3D handles): ``record`` also appends to the wall
        profile with these edges and ``drain`` reads and reopens it with the trace; ``profile_records`` returns (steps, bins).
        ``cycle_tol`` = (rtol, atol) of the weights of the accelerated cycle map (``cycle_open``; section 5r)."""
        from . import backend
        self.backend = backend
        self.cycle_tol, self.cycle_is_open = (float(cycle_tol[0]), float(cycle_tol[1])), False
        self.run, self.sys, self.dev = run, run.sys, run.sys.dev
        self.solver_parameters, self.inv_dt_of_h, self.tol, self.capacity = solver_parameters, inv_dt_of_h, tol, int(capacity)
        self.chunks, self.profile_chunks, self.sensitivity_chunks, self.segments, self.states, self.count = [], [], [], [], [], 0
        self.after_accept = after_accept
        self.profile_edges = None if profile_edges is None else [float(e) for e in profile_edges]
        self.newton_iterations, self.residuals = 0, []   # residuals: the last Newton residual of every accepted step
        # the transient sensitivities (section 5p): parameter codes of the tangent; "steady" takes the columns of the tangent call the
        # caller has just made at inv_dt = 0, "zero" starts from S = 0.  The device keeps dQ and dQ_D across a drained buffer.
        self.sensitivities = None if sensitivities is None else [int(q) for q in sensitivities]
        if sensitivity_start not in ("zero", "steady"):
            raise ValueError("programme: sensitivity_start is 'steady' or 'zero'")
        dev = self.dev
        self.trace = RecordStream((dev.electrode_trace_open, dev.electrode_trace_append, dev.electrode_trace_read, dev.electrode_trace_close),
                                  self.chunks, np.zeros(0, backend.ELECTRODE_RECORD_DTYPE), carry={"Q": "I", "Q_D": "dD_dt"})
        self.sensitivity = None if sensitivities is None else RecordStream(
            (dev.sensitivity_open, dev.sensitivity_step, dev.sensitivity_read, dev.sensitivity_close), self.sensitivity_chunks,
            np.zeros((0, len(self.sensitivities)), backend.SENSITIVITY_RECORD_DTYPE), (self.sensitivities, sensitivity_start), (self.sensitivities, "continue"))
        self.profile = None if profile_edges is None else RecordStream(   # (the bins' charges go on across a drained buffer, as the trace's do)
            (dev.wall_profile_open, dev.wall_profile_append, dev.wall_profile_read, dev.wall_profile_close), self.profile_chunks,
            np.zeros((0, len(self.profile_edges) - 1), backend.WALL_PROFILE_RECORD_DTYPE), (self.profile_edges,), carry={"Q": "I"})
        self.trace.open(self.capacity)   # (launches the Stern term only: a steady tangent stays valid for the sensitivities' open below)
        self.D_first = dev.stern_displacement()   # the D_prev the trace starts from (the bits the open call took)
        self.streams = [self.trace]
        for st in filter(None, (self.sensitivity, self.profile)):
            try:
                st.open(*st.args, self.capacity)
            except BaseException:
                for done in self.streams:
                    done.close()
                raise
            self.streams.append(st)
        # appended to in this order (accepted steps only: a rejected attempt never touches S)
        self.streams.sort(key=(self.trace, self.profile, self.sensitivity).index)

    def set_potential(self, p):
        run = self.run
        self.dev.set_electrode_potential(p)
        run.stern = dataclasses.replace(run.stern, p_electrode=float(p))
        run.problem.stern = run.stern
        if run.kinetics is not None:
            run.kinetics = dataclasses.replace(run.kinetics, p_electrode=float(p))
            run.problem.kinetics = run.kinetics

    def set_step(self, h):
        self.sys.set_time_step(self.inv_dt_of_h(h))

    def solve(self):
        backend = self.backend
        try:
            st = self.sys.solve(self.solver_parameters)
        except backend.GmpnpError as e:
            if e.code not in (backend.ERR_NUMERIC, backend.ERR_LINEAR):
                raise
            st = e.stats
            if st is not None:
                self.sys.record(st)
            return False, (st or {}).get("iterations", 0)
        except RuntimeError as e:   # DOLFIN's "Newton solver did not converge"
            cause = e.__cause__
            if not (isinstance(cause, backend.GmpnpError) and cause.code == backend.ERR_NOT_CONVERGED):
                raise
            if cause.stats is not None:
                self.sys.record(cause.stats)
            return False, (cause.stats or {}).get("iterations", 0)
        self.newton_iterations += st["iterations"]
        return True, st["iterations"]

    def estimate(self, h, h_prev):
        return self.sys.time_error(h, h_prev, self.tol[0], self.tol[1])

    def record(self, t, h, seg, p):
        if self.run.budget is not None:   # while u_n is the previous state and inv_dt the step's
            self.run.budget.take(self.sys)
        for st in self.streams:
            st.append(t, h)
        self.residuals.append(float(self.sys.last_stats["residuals"][-1]))
        self.segments.append(int(seg))
        self.count += 1
        if self.count == self.capacity:   # u is still this step's state: the trace opened again takes its D as D_prev
            self.drain(reopen=True)

    def accept(self):
        if self.after_accept is not None:
            self.after_accept()
        self.sys.time_accept()

    def reject(self):
        self.sys.time_reject()

    def breakpoint(self, seg, t):
        self.states.append((int(seg), float(t), self.sys.vertex_values()))

    def drain(self, reopen=False):
        if self.count:
            for st in self.streams:
                st.drain(self.count)
            self.count = 0
        if reopen:
            for st in self.streams:
                st.open(*st.reopen_args, self.capacity)

    # ---- the accelerated cycle map (``periodic.run_periodic``; section 5r) ----
    def cycle_open(self, depth):
        if self.sensitivities is not None or self.profile_edges is not None:
            raise ValueError("programme: periodic runs carry neither sensitivities nor a wall profile")
        self.dev.cycle_open(depth, *self.cycle_tol)
        self.cycle_is_open = True

    def cycle_close(self):
        if self.cycle_is_open:
            self.cycle_is_open = False
            self.dev.cycle_close()

    def cycle_begin(self):
        self.dev.cycle_begin()

    def cycle_end(self):
        return self.dev.cycle_end()

    def _fresh_records(self, between=None):
        """Drops every record and breakpoint state taken so far and opens the trace again at the state ``between`` leaves (the mix, which
        the library refuses under an open trace): D_prev is that state's D and the charges start at 0."""
        self.count = 0
        self.dev.electrode_trace_close()
        try:
            return between() if between is not None else None
        finally:
            self.dev.electrode_trace_open(self.capacity)
            self.D_first = self.dev.stern_displacement()
            self.chunks.clear()
            self.trace.base, self.segments, self.states, self.residuals = {}, [], [], []

    def cycle_mix(self, gamma, tau):
        backend = self.backend

        def mix():
            try:
                return self.dev.cycle_mix(gamma, tau)
            except backend.GmpnpError as e:   # a value of the direction that is not finite: nothing was applied
                if e.code != backend.ERR_NUMERIC:
                    raise
                return math.nan
        return self._fresh_records(mix)

    def cycle_restart(self):
        self.dev.cycle_restart()
        self._fresh_records()

    def state(self):
        return self.sys.vertex_values()

    def abort(self):
        """After an exception inside the loop: the handle returns to the last accepted state (u <- u_n) and the trace is closed, so
        the run is left at the potential of the attempt that failed (``run.stern`` / ``run.kinetics`` and the handle agree) with no
        trace open.  The records written so far stay in ``chunks`` / on the device unread."""
        backend = self.backend
        for call in [self.sys.time_reject] + [st.close for st in self.streams]:
            try:
                call()
            except backend.GmpnpError as e:
                if e.code == backend.ERR_HIP:
                    raise

    def records(self):
        """Every record so far, in order (drains the trace and closes it)."""
        self.drain()
        self.trace.close()
        return self.trace.records()

    def profile_records(self):
        """Every record of the wall profile so far, (steps, bins), in order (after ``records``, which drained both buffers; closes the
        profile)."""
        if not self.profile:
            raise ValueError("programme: the run carries no wall profile")
        self.drain()
        self.profile.close()
        return self.profile.records()

    def sensitivity_records(self):
        """Every sensitivity record so far, (steps, columns), in order (drains both buffers; the sensitivities stay open, with S on the
        device, until ``sensitivity_close``)."""
        if not self.sensitivity:
            raise ValueError("programme: the run carries no sensitivities")
        self.drain()
        return self.sensitivity.records()


OUTPUT_KEYS = ("time_s", "electrode_voltage", "potential_OHP", "surface_charge", "i_CO", "i_H2", "i_charging", "i_total", "charge_CO",
               "charge_H2", "charge_double_layer", "FE_H2", "FE_H2_cycle", "OHP_H", "OHP_OH", "OHP_HCO3", "OHP_CO32", "OHP_CO2", "OHP_cat",
               "segment", "status")
SPECIES_KEYS = ("OHP_H", "OHP_OH", "OHP_HCO3", "OHP_CO32", "OHP_CO2", "OHP_cat")
METADATA_KEYS = ("programme_kind", "programme_cycles", "programme_segments", "programme_steps_accepted", "programme_steps_rejected",
                 "programme_stop_reason", "programme_t_reached", "programme_newton_iterations", "programme_charge_closure",
                 "programme_status", "programme_electrode_voltage", "programme_potential_OHP", "programme_surface_charge")


SENSITIVITY_KEYS = ("d_i_CO", "d_i_H2", "d_surface_charge", "d_i_charging", "d_charge_CO", "d_charge_H2", "d_charge_double_layer",
                    "d_potential_OHP")
SENSITIVITY_METADATA_KEYS = ("programme_sensitivity_parameters", "programme_sensitivity_start", "programme_sensitivity_status",
                             "programme_sensitivity_residual")
OFFSET = "offset"   # the name of parameter code 0 in the drivers: a potential offset of the whole waveform


def sensitivity_arrays(ep, eps_0, srec, names, codes):
    """The arrays of ``programme_sensitivity.npz`` from the sensitivity records (steps, columns): time_s, parameters, status (steps,
    columns) and, per quantity of ``SENSITIVITY_KEYS``, an array (steps, columns) in the units and signs of ``output_arrays``
    (d_i_CO, d_i_H2 [A/m2], d_surface_charge [C/m2], d_i_charging [A/m2], the charges [C/m2], d_potential_OHP [V]) per unit of the
    column's parameter: ln i0, alpha, ln stern_length, and volts for the offset (the library's column is per thermal voltage)."""
    V_T, tc = ep.thermal_voltage, ep.time_constant
    q = eps_0 * V_T / ep.L_n
    per = np.array([1.0 / V_T if int(c) == 0 else 1.0 for c in codes])[None, :]
    out = {"time_s": (srec["t"][:, 0] if len(srec) else np.zeros(0)) * tc, "parameters": np.array([str(n) for n in names]),
           "status": srec["status"].astype(np.int64),
           "d_i_CO": srec["dI"][:, :, 0] * per, "d_i_H2": srec["dI"][:, :, 1] * per, "d_surface_charge": q * srec["dD"] * per,
           "d_i_charging": -q * srec["d_dD_dt"] / tc * per, "d_charge_CO": srec["dQ"][:, :, 0] * tc * per,
           "d_charge_H2": srec["dQ"][:, :, 1] * tc * per, "d_charge_double_layer": -q * srec["dQ_D"] * per,
           "d_potential_OHP": srec["dp_boundary"] * V_T * per}
    assert set(out) == set(SENSITIVITY_KEYS) | {"time_s", "parameters", "status"}
    return out


def segment_cycles(segs, cycles):
    """The cycle of every segment.  The cycles are equal windows in time (all three waveforms repeat with one period: the sum of a
    pulse's durations, two legs of a triangle; a table is one cycle), and a segment belongs to the window that holds its midpoint: a
    step never straddles a breakpoint, so neither does it straddle two cycles.  Counting segments would not do: a pulse with a rise
    time has no ramp in front of its first hold, so its first cycle is one segment shorter than the others."""
    cycles = max(int(cycles), 1)
    t0, period = segs[0][0], (segs[-1][1] - segs[0][0]) / cycles
    mid = np.array([0.5 * (g[0] + g[1]) for g in segs])
    return np.minimum(np.floor((mid - t0) / period).astype(np.int64), cycles - 1)


def output_arrays(ep, eps_0, rec, segments, segs, cycles, species_index=(0, 1, 2, 3, 4, 5)):
    """The arrays of ``programme.npz`` (``OUTPUT_KEYS``) from the records of the trace.  The OHP is one point, so the integrated rates are
    current densities: i_CO, i_H2 [A/m2], their charges [C/m2] = Q_r x time_constant.  surface_charge [C/m2] = eps_0 V_T / L_n x D is
    the charge ON THE ELECTRODE (negative for a cathode); i_charging = -d(surface_charge)/dt [A/m2] is cathodic-positive like the
    kinetic currents — the sign of section 5k's Y = i omega C - sum dI/dV: a potential moving down charges the layer with a positive
    i_charging — and charge_double_layer its time integral, so i_total = i_CO + i_H2 + i_charging.  FE_H2_cycle: the charge-weighted
    mean of FE_H2 over each cycle, charge_H2 / (charge_CO + charge_H2) of the cycle's steps, one value per cycle (``segment_cycles``)."""
    V_T, tc = ep.thermal_voltage, ep.time_constant
    q = eps_0 * V_T / ep.L_n
    n = len(rec)
    i_CO, i_H2 = rec["I"][:, 0].copy(), rec["I"][:, 1].copy()
    tot = i_CO + i_H2
    with np.errstate(divide="ignore", invalid="ignore"):
        fe = np.where(tot != 0.0, i_H2 / tot, np.nan)
    i_ch = -q * rec["dD_dt"] / tc
    seg = np.asarray(segments, dtype=np.int64)
    cyc = segment_cycles(segs, cycles)[seg] if n else seg
    fe_cycle = np.full(max(int(cycles), 1), np.nan)
    for c in range(len(fe_cycle)):
        m = cyc == c
        qc, qh = float((rec["h"][m] * i_CO[m]).sum()), float((rec["h"][m] * i_H2[m]).sum())
        if m.any() and qc + qh != 0.0:
            fe_cycle[c] = qh / (qc + qh)
    out = {"time_s": rec["t"] * tc, "electrode_voltage": rec["p_M"].copy(), "potential_OHP": rec["p_boundary"] * V_T, "surface_charge": q * rec["D"],
           "i_CO": i_CO, "i_H2": i_H2, "i_charging": i_ch, "i_total": tot + i_ch, "charge_CO": rec["Q"][:, 0] * tc, "charge_H2": rec["Q"][:, 1] * tc,
           "charge_double_layer": -q * rec["Q_D"], "FE_H2": fe, "FE_H2_cycle": fe_cycle, "segment": seg, "status": rec["status"].astype(np.int64)}
    for j, key in zip(species_index, SPECIES_KEYS):   # (the 1D model's species order; the pore driver passes its own)
        out[key] = rec["u_boundary"][:, j].copy()
    assert set(out) == set(OUTPUT_KEYS) and all(len(out[k]) == n for k in OUTPUT_KEYS if k != "FE_H2_cycle")
    return out


# ---- potential programmes in the 3D pore: the keyword ``pore_programme`` of ``PoreRun`` ------------------------------
PORE_SPECIES_INDEX = (0, 1, 2, 3, 4, 7)   # H, OH, HCO3, CO32, CO2, cat among the pore model's eight species (``SPECIES_KEYS``' order)
PROFILE_GEOMETRY_KEYS = ("z_lo_m", "z_hi_m", "bin_area_m2")
PROFILE_KEYS = ("profile_i_CO", "profile_i_H2", "profile_FE_H2", "profile_surface_charge", "profile_potential_OHP", "profile_CO2",
                "profile_H", "profile_charge_CO", "profile_charge_H2", "profile_status")
PORE_OUTPUT_KEYS = OUTPUT_KEYS + PROFILE_GEOMETRY_KEYS + PROFILE_KEYS
PORE_METADATA_KEYS = tuple("pore_" + k for k in METADATA_KEYS) + ("pore_programme_bins",)
PORE_COMMON_FIELDS = {"kind", "dt_init", "dt_restart", "steps_per_segment", "capacity", "bins"}


def check_pore_programme(par, kwargs, dt_order=1, partition=None, multilevel=False, glue="host"):
    """The refusals of the pore driver's ``pore_programme`` keyword, before anything touches the device; returns the checked dict
    (``bins`` defaults to 16).  The waveform is ``check_programme``'s; order 1 only and no sensitivities."""
    par = dict(par)
    if set(par) & {"sensitivities", "sensitivity_start"}:
        raise ValueError("pore_programme: the transient sensitivities are 1D (programme)")
    if "periodic" in par:   # (the lagged Sechenov Dirichlet value would be part of the cycle map's state)
        raise ValueError("pore_programme: periodic (the limit cycle by the accelerated cycle map) is 1D (programme)")
    if kwargs.get("programme"):
        raise ValueError("pore_programme: not in one run with programme (which the 3D pore driver refuses)")
    if partition:
        raise ValueError("pore_programme: not available in a partitioned solve")
    if multilevel:
        raise ValueError("pore_programme: not available with the geometric multilevel term")
    if glue != "host":
        raise ValueError("pore_programme: the programme runs with the host glue")
    bins = par.pop("bins", 16)
    check_bins(bins)
    try:
        par = check_programme(par, kwargs, dt_order)
    except ValueError as e:
        raise ValueError("pore_" + str(e)) from None
    par["bins"] = bins
    return par


def refuse_pore_programme(kwargs, what, hint=""):
    """ValueError where ``kwargs`` asks for a potential programme of the pore (``pore_programme``) in a driver that has none."""
    if kwargs.get("pore_programme"):
        raise ValueError("pore_programme: potential programmes with a wall profile are not available in %s%s" % (what, hint))


def add_pore_programme_arguments(p):
    """The pore parser's flags.  None of them begins with --programme: argparse would take --programme for an abbreviation."""
    p.add_argument("--pore_programme", required=False, default=None, choices=KINDS,
                   help="(addition) potential programme after the run's own schedule, from its last state, with the wall resolved along "
                        "the axis (pore_programme.npz)")
    p.add_argument("--v_levels", required=False, default=None, type=float, nargs="+", help="(addition) levels of --pore_programme pulse [thermal voltages]")
    p.add_argument("--durations", required=False, default=None, type=float, nargs="+", help="(addition) hold times of --pore_programme pulse [s]")
    p.add_argument("--cycles", required=False, default=1, type=int, help="(addition) cycles of --pore_programme pulse / triangle")
    p.add_argument("--rise_time", required=False, default=0.0, type=float, help="(addition) ramp in place of each jump of --pore_programme pulse [s]")
    p.add_argument("--v_vertex", required=False, default=None, type=float, help="(addition) vertex potential of --pore_programme triangle [thermal voltages]")
    p.add_argument("--scan_rate", required=False, default=None, type=float, help="(addition) scan rate of --pore_programme triangle [V/s]")
    p.add_argument("--pore_programme_file", required=False, default=None, type=str,
                   help="(addition) CSV of --pore_programme table: columns time_s, electrode_voltage")
    p.add_argument("--pore_programme_dt_init", required=False, default=None, type=float,
                   help="(addition) first step of the programme and after a jump (scaled time)")
    p.add_argument("--pore_programme_steps_per_segment", required=False, default=None, type=int,
                   help="(addition) fixed mode: equal steps per segment, no estimator")
    p.add_argument("--pore_programme_bins", required=False, default=None, type=int, help="(addition) axial bins of the wall profile (default 16)")


def pore_programme_keywords(a):
    """The ``pore_programme`` keyword of a parsed command line (``add_pore_programme_arguments``); empty without --pore_programme."""
    kind = a.pore_programme
    if kind is None:
        return {}
    par = {"kind": kind}
    if kind == "pulse":
        if a.v_levels is None or a.durations is None:
            raise ValueError("pore_programme: --pore_programme pulse needs --v_levels and --durations")
        par.update(v_levels=list(a.v_levels), durations=list(a.durations), cycles=a.cycles, rise_time=a.rise_time)
    elif kind == "triangle":
        if a.v_vertex is None or a.scan_rate is None:
            raise ValueError("pore_programme: --pore_programme triangle needs --v_vertex and --scan_rate")
        par.update(v_vertex=a.v_vertex, scan_rate=a.scan_rate, cycles=a.cycles)
    else:
        if a.pore_programme_file is None:
            raise ValueError("pore_programme: --pore_programme table needs --pore_programme_file")
        t, v = load_table(a.pore_programme_file)
        par.update(time_s=t, electrode_voltage=v)
    if a.pore_programme_dt_init is not None:
        par["dt_init"] = a.pore_programme_dt_init
    if a.pore_programme_steps_per_segment is not None:
        par["steps_per_segment"] = a.pore_programme_steps_per_segment
    if a.pore_programme_bins is not None:
        par["bins"] = a.pore_programme_bins
    return {"pore_programme": par}


def wall_mean_records(rec, wall_area):
    """The records of the trace with the integrated quantities (D, dD_dt, I, Q, Q_D) divided by the wall area (scaled units): what
    ``output_arrays`` turns into wall means."""
    out = rec.copy()
    for key in ("D", "dD_dt", "I", "Q", "Q_D"):
        out[key] = rec[key] / float(wall_area)
    return out


def pore_output_arrays(pp, eps_0, wall_area, rec, prof, segments, segs, cycles):
    """The arrays of ``pore_programme.npz`` (``PORE_OUTPUT_KEYS``).  ``OUTPUT_KEYS`` as wall means: the currents [A/m2] and charges
    [C/m2] divided by the wall area (scaled, sum_I w_I), surface_charge = eps_0 V_T / L x D / wall area as ``polarisation.curve_arrays``
    has it for 3D.  From the profile records ``prof`` (steps, bins), every quantity divided by the bin's OWN area: z_lo_m, z_hi_m [m],
    bin_area_m2 [m2] (bins,); profile_i_CO, profile_i_H2 [A/m2], profile_FE_H2, profile_surface_charge [C/m2],
    profile_potential_OHP [V], profile_CO2 and profile_H (scaled concentrations, as arrays_unscaled.npz holds them),
    profile_charge_CO, profile_charge_H2 [C/m2] and profile_status, each (steps, bins)."""
    from types import SimpleNamespace
    ep = SimpleNamespace(thermal_voltage=pp.thermal_voltage, time_constant=pp.time_constant, L_n=pp.L)
    out = output_arrays(ep, eps_0, wall_mean_records(rec, wall_area), segments, segs, cycles, species_index=PORE_SPECIES_INDEX)
    V_T, tc, L = pp.thermal_voltage, pp.time_constant, pp.L
    q = eps_0 * V_T / L
    nb = prof.shape[1]
    if len(prof):
        area = prof["area"]
        out.update(z_lo_m=prof["z_lo"][0] * L, z_hi_m=prof["z_hi"][0] * L, bin_area_m2=area[0] * L * L)
    else:
        area = np.ones((0, nb))
        out.update(z_lo_m=np.full(nb, np.nan), z_hi_m=np.full(nb, np.nan), bin_area_m2=np.full(nb, np.nan))
    i_CO, i_H2 = prof["I"][:, :, 0] / area, prof["I"][:, :, 1] / area
    tot = i_CO + i_H2
    with np.errstate(divide="ignore", invalid="ignore"):
        fe = np.where(tot != 0.0, i_H2 / tot, np.nan)
    out.update(profile_i_CO=i_CO, profile_i_H2=i_H2, profile_FE_H2=fe, profile_surface_charge=q * prof["D"] / area,
               profile_potential_OHP=prof["p_mean"] * V_T, profile_CO2=prof["u_mean"][:, :, 4].copy(), profile_H=prof["u_mean"][:, :, 0].copy(),
               profile_charge_CO=prof["Q"][:, :, 0] * tc / area, profile_charge_H2=prof["Q"][:, :, 1] * tc / area,
               profile_status=prof["status"].astype(np.int64))
    assert set(out) == set(PORE_OUTPUT_KEYS)
    return out
