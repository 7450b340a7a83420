"""Potential programmes on the CPU: the host rule (g++ alone) against its Python statement
(gmpnp_amd/programme.py) bit for bit — programme_value, the builders, the walk, the combine step of the electrode record —,
``run_programme`` over the NumPy system of tests/programme_reference.py (landing, restart after a jump, retry after a planted Newton
failure), the charge identity, the quasi-steady limit, the ctypes image against the header, the Python refusals and the command lines.
The cases are K+ at L_n = 1 um on small uniform meshes with a BDM Stern layer and two reactions, from the steady state at p_M = -5."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import hp_reference as H
import kinetics_reference as K
import programme_reference as PR
import response_reference as R
import tangent_reference as T
from gmpnp_amd import programme as P
from gmpnp_amd.params import edl_parameters
from gmpnp_amd.problem import SternLayer, edl_problem
from gmpnp_amd.stern import L_STERN
from gmpnp_amd.timestep import TimeStepPolicy, next_time_step
from step_limit_reference import first_step_state
from test_kinetics_reference import TAFEL, two_reactions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_M = -5.0


def uniform_problem(nv, kinetics=True, p_M=P_M):
    """K+ at L_n = 1 um on a uniform mesh of ``nv`` vertices, BDM Stern layer, two reactions: (parameters, problem)."""
    ep = edl_parameters(cation="K", L_n=1e-6)
    kin = two_reactions(ep.species, p_M) if kinetics else None
    return ep, edl_problem(ep, H.uniform_mesh_1d(nv), stern=SternLayer("BDM", p_M, L_STERN / ep.L_n), kinetics=kin)


def steady_case(nv, kinetics=True):
    """(parameters, problem, steady state at p_M = -5 (read-only), inv_dt_of_h)."""
    ep, prob = uniform_problem(nv, kinetics)
    u1, st = K.newton_loop(prob, *first_step_state(prob))
    assert st.converged
    u, _, ok = T.steady_state(prob, u1)
    assert ok
    u.setflags(write=False)
    L_D = ep.L_D
    return ep, prob, u, (lambda h: 1.0 / (h * L_D))


@pytest.fixture(scope="module")
def case9():
    return steady_case(9)


@pytest.fixture(scope="module")
def case65():
    return steady_case(65)


# ---- the host rule against its Python statement -------------------------------------------------------------------------------------
DRIVER = r"""
#include <cstdio>
#include <cstring>
#include "gmpnp_host_rules.h"
using namespace gmpnp;
static void print_segments(const Programme& s) {
  std::printf("%d", (int)programme_valid(s));
  for (const auto& g : s) std::printf(" %a %a %a %a", g.t0, g.t1, g.p0, g.p1);
  std::printf("\n");
}
static bool read_list(std::vector<double>& v) {
  int n; if (std::scanf("%d", &n) != 1) return false;
  v.resize(n);
  for (int i = 0; i < n; ++i) if (std::scanf("%lf", &v[i]) != 1) return false;
  return true;
}
int main() {
  char cmd[32];
  while (std::scanf("%31s", cmd) == 1) {
    if (!std::strcmp(cmd, "value")) {
      ProgrammeSegment g; double t; if (std::scanf("%lf %lf %lf %lf %lf", &g.t0, &g.t1, &g.p0, &g.p1, &t) != 5) return 1;
      std::printf("%a\n", programme_value(g, t));
    } else if (!std::strcmp(cmd, "pulse")) {
      std::vector<double> lv, du; int cycles; double rise;
      if (!read_list(lv) || !read_list(du) || std::scanf("%d %lf", &cycles, &rise) != 2) return 1;
      print_segments(programme_pulse(lv, du, cycles, rise));
    } else if (!std::strcmp(cmd, "triangle")) {
      double a, b, rate; int cycles; if (std::scanf("%lf %lf %lf %d", &a, &b, &rate, &cycles) != 4) return 1;
      print_segments(programme_triangle(a, b, rate, cycles));
    } else if (!std::strcmp(cmd, "table")) {
      std::vector<double> t, p; if (!read_list(t) || !read_list(p)) return 1;
      print_segments(programme_table(t, p));
    } else if (!std::strcmp(cmd, "combine")) {
      ElectrodeAccum a{}; int n; if (std::scanf("%lf %d", &a.D_prev, &n) != 2) return 1;
      for (int i = 0; i < n; ++i) {
        double h, D, I[4]; if (std::scanf("%lf %lf %lf %lf %lf %lf", &h, &D, &I[0], &I[1], &I[2], &I[3]) != 6) return 1;
        const double d = electrode_record_combine(a, h, D, I);
        std::printf("%a %a %a %a %a %a %a;", d, a.Q[0], a.Q[1], a.Q[2], a.Q[3], a.Q_D, a.D_prev);
      }
      std::printf("\n");
    } else if (!std::strcmp(cmd, "walk")) {
      // a pulse programme, the walk's settings, then n scripted attempts (err, has_history, newton_failed)
      std::vector<double> lv, du; int cycles, n; double rise, dt_init, dt_restart, run_end, h_min;
      if (!read_list(lv) || !read_list(du) || std::scanf("%d %lf %lf %lf %lf %lf %d", &cycles, &rise, &dt_init, &dt_restart, &run_end, &h_min, &n) != 7) return 1;
      const Programme s = programme_pulse(lv, du, cycles, rise);
      ProgrammeWalk w = programme_begin(s, dt_init, run_end);
      for (int i = 0; i < n; ++i) {
        double err; int hist, failed; if (std::scanf("%lf %d %d", &err, &hist, &failed) != 3) return 1;
        if (w.stop) continue;
        TimeStepPolicy pol; pol.h_min = h_min; pol.t_end = programme_break(s, w.seg, run_end);
        const double t = w.t, h = w.h;
        const double p = programme_value(s[w.seg], programme_step_end(t, h, pol.t_end));
        const TimeStepDecision d = next_time_step(pol, t, h, err, hist != 0 && w.h_prev > 0.0, failed != 0, 1.0, w.steady_run);
        const int landed = programme_after(s, w, d, h, dt_restart, run_end);
        std::printf("%a %a %a %d %d %a %a %a %d;", t, h, p, landed, w.seg, w.t, w.h, w.h_prev, w.stop);
      }
      std::printf("\n");
    }
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    d = tmp_path_factory.mktemp("programme_rule")
    src, exe = d / "rule.cpp", d / "rule"
    src.write_text(DRIVER)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "gmpnp_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True)

    def ask(lines):
        return subprocess.run([str(exe)], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
    return ask


def _list(v):
    return "%d " % len(v) + " ".join(repr(float(x)) for x in v)


def _segments(line):
    tok = line.split()
    vals = [float.fromhex(x) for x in tok[1:]]
    return int(tok[0]), [tuple(vals[k:k + 4]) for k in range(0, len(vals), 4)]


def _python_or_invalid(build):
    try:
        return 1, build()
    except ValueError:
        return 0, []


def test_programme_value_has_the_bits_of_the_host_rule(rules):
    rng = np.random.default_rng(11)
    cases = []
    for _ in range(40):
        t0, dt, p0, p1 = rng.uniform(-3, 3), rng.uniform(1e-3, 7), rng.uniform(-30, 5), rng.uniform(-30, 5)
        t1 = t0 + dt
        for t in (t0, t1, t0 + rng.uniform(0, 1) * dt, t0 + dt / 3.0, np.nextafter(t1, -np.inf), np.nextafter(t1, np.inf)):
            cases.append((t0, t1, p0, p1, float(t)))
    out = rules(["value " + " ".join(repr(float(x)) for x in c) for c in cases])
    for c, line in zip(cases, out):
        assert float.fromhex(line) == P.programme_value(c[:4], c[4]), c
    assert P.programme_value((0.0, 0.3, -5.0, -7.1), 0.3) == -7.1            # the landed value is p1 itself,
    assert P.programme_value((0.0, 0.3, -5.0, -7.1), 0.31) == -7.1           # whatever the interpolated sum rounds to
    assert P.programme_value((0.0, 0.3, -5.0, -7.1), 0.0) == -5.0


def test_builders_have_the_bits_of_the_host_rule(rules):
    pulses = [([-5.0, -7.5], [0.3, 0.1], 3, 0.0), ([-5.0, -7.5], [0.3, 0.1], 2, 0.01), ([-5.0, -5.0, -6.0], [0.1, 0.2, 0.7], 2, 0.05),
              ([-5.0], [0.37], 1, 0.0), ([-5.0, -6.0], [0.3], 1, 0.0), ([-5.0, -6.0], [0.3, 0.1], 0, 0.0), ([-5.0, -6.0], [0.3, 0.1], 1, 0.1),
              ([-5.0, math.inf], [0.3, 0.1], 1, 0.0), ([-5.0, -6.0], [0.3, 0.1], 1, -1.0)]
    out = rules(["pulse %s %s %d %r" % (_list(lv), _list(du), c, r) for lv, du, c, r in pulses])
    for (lv, du, c, r), line in zip(pulses, out):
        ok, segs = _python_or_invalid(lambda: P.pulse(lv, du, c, r))
        got = _segments(line)
        assert got == (ok, segs) or (ok == 0 and got == (0, [])), (lv, du, c, r)
    triangles = [(-5.0, -9.0, 0.7, 2), (-5.0, -1.0, 3.3, 1), (0.1, 0.3, 0.1, 3), (-5.0, -5.0, 1.0, 1), (-5.0, -6.0, 0.0, 1), (-5.0, -6.0, 1.0, 0)]
    out = rules(["triangle %r %r %r %d" % t for t in triangles])
    for t, line in zip(triangles, out):
        ok, segs = _python_or_invalid(lambda: P.triangle(*t))
        assert _segments(line) == (ok, segs), t
    tables = [([0.0, 0.1, 0.35, 1.0], [-5.0, -5.0, -7.0, -6.5]), ([0.0, 0.1, 0.1, 0.4], [-5.0, -5.0, -7.0, -7.0]), ([0.0, 0.0, 0.4], [-5.0, -6.0, -6.0]),
              ([0.0, 0.2, 0.2, 0.2, 0.4], [-5.0] * 5), ([0.0, 0.3, 0.2], [-5.0] * 3), ([0.0], [-5.0]), ([0.0, 0.2, 0.2], [-5.0, -5.0, -6.0])]
    out = rules(["table %s %s" % (_list(t), _list(p)) for t, p in tables])
    for (t, p), line in zip(tables, out):
        ok, segs = _python_or_invalid(lambda: P.table(t, p))
        assert _segments(line) == (ok, segs), (t, p)
    segs = P.pulse([-5.0, -7.5], [0.3, 0.1], 2, 0.01)
    assert P.programme_valid(segs) and [P.programme_jump(segs, k) for k in range(len(segs))] == [False] * len(segs)
    segs = P.pulse([-5.0, -7.5], [0.3, 0.1], 2)
    assert [P.programme_jump(segs, k) for k in range(4)] == [True, True, True, False]
    assert not any(P.programme_jump(P.triangle(-5.0, -9.0, 0.7, 2), k) for k in range(4))
    assert P.table([0.0, 0.1, 0.1, 0.4], [-5.0, -5.0, -7.0, -7.0]) == [(0.0, 0.1, -5.0, -5.0), (0.1, 0.4, -7.0, -7.0)]


def test_combine_step_has_the_bits_of_the_host_rule(rules):
    rng = np.random.default_rng(5)
    rows = [(float(rng.uniform(1e-4, 3.0)), float(rng.normal() * 40.0)) + tuple(float(x) for x in rng.normal(size=4) * 3.0) for _ in range(25)]
    D0 = float(rng.normal() * 40.0)
    out = rules(["combine %r %d " % (D0, len(rows)) + " ".join(repr(x) for r in rows for x in r)])[0]
    acc = P.fresh_accumulators(D0)
    got = [tuple(float.fromhex(x) for x in part.split()) for part in out.split(";") if part.strip()]
    for r, g in zip(rows, got):
        d = P.electrode_record_combine(acc, r[0], r[1], r[2:])
        assert g == (d,) + tuple(acc["Q"]) + (acc["Q_D"], acc["D_prev"]), r


def test_walk_has_the_bits_of_the_host_rule(rules):
    rng = np.random.default_rng(3)
    scripts = []
    for lv, du, cyc, rise, dt_init, run_end, h_min in (([-5.0, -7.0], [0.3, 0.1], 2, 0.0, 0.013, math.inf, 0.0), ([-5.0, -7.0], [0.3, 0.1], 2, 0.02, 0.05, 0.55, 0.0),
                                                       ([-5.0, -6.0, -5.5], [0.11, 0.07, 0.2], 1, 0.0, 0.02, math.inf, 1e-3)):
        n = 60
        att = [(float(10.0 ** rng.uniform(-3, 0.6)), int(rng.uniform() < 0.9), int(rng.uniform() < 0.1)) for _ in range(n)]
        scripts.append((lv, du, cyc, rise, dt_init, dt_init / 2.0, run_end, h_min, att))
    lines = ["walk %s %s %d %r %r %r %s %r %d " % (_list(lv), _list(du), cyc, rise, a, b, "inf" if math.isinf(e) else repr(e), hm, len(att))
             + " ".join("%r %d %d" % x for x in att) for lv, du, cyc, rise, a, b, e, hm, att in scripts]
    out = rules(lines)
    for (lv, du, cyc, rise, dt_init, dt_restart, run_end, h_min, att), line in zip(scripts, out):
        segs = P.pulse(lv, du, cyc, rise)
        w = P.programme_begin(segs, dt_init, run_end)
        want = []
        for err, hist, failed in att:
            if w.stop:
                continue
            t_break = P.programme_break(segs, w.seg, run_end)
            t, h = w.t, w.h
            p = P.programme_value(segs[w.seg], P.programme_step_end(t, h, t_break))
            d = next_time_step(TimeStepPolicy(h_min=h_min, t_end=t_break), t, h, err, bool(hist) and w.h_prev > 0.0, bool(failed), 1.0, w.steady_run)
            landed = P.programme_after(segs, w, d, h, dt_restart, run_end)
            want.append((t, h, p, int(landed), w.seg, w.t, w.h, w.h_prev, w.stop))
        got = []
        for part in line.split(";"):
            g = part.split()
            if g:
                got.append((float.fromhex(g[0]), float.fromhex(g[1]), float.fromhex(g[2]), int(g[3]), int(g[4]), float.fromhex(g[5]),
                            float.fromhex(g[6]), float.fromhex(g[7]), int(g[8])))
        assert got == want and len(got) > 10
        assert want[-1][8] != 0 or len(want) == len(att)


def test_ctypes_image_has_the_layout_of_the_header(tmp_path):
    from gmpnp_amd import backend
    fields = ("t", "h", "p_M", "p_boundary", "D", "dD_dt", "I", "Q", "Q_D", "u_boundary", "status")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gmpnp.h"\nint main(void){printf("%zu", sizeof(gmpnp_electrode_record_t));\n'
                   + "".join('printf(" %%zu", offsetof(gmpnp_electrode_record_t,%s));\n' % f for f in fields) + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    C = backend.CElectrodeRecord
    assert got == [ctypes.sizeof(C)] + [getattr(C, f).offset for f in fields]
    dt = backend.ELECTRODE_RECORD_DTYPE
    assert dt.itemsize == ctypes.sizeof(C) and [dt.fields[f][1] for f in fields] == got[1:]
    assert P.MAX_SURFACE_REACTIONS == backend.MAX_SURFACE_REACTIONS
    for name in ("gmpnp_set_electrode_potential", "gmpnp_electrode_trace_open", "gmpnp_electrode_trace_append", "gmpnp_electrode_trace_read",
                 "gmpnp_electrode_trace_close"):
        assert name in backend.EXPORTS


# ---- run_programme over the NumPy system ------------------------------------------------------------------------------------------------
PULSE = dict(levels=[-5.5, -4.5], durations=[30.0, 20.0], cycles=2)     # scaled time: the reference step of this case is 9.5


def test_steps_land_on_the_breakpoints_and_restart_behind_a_jump(case9):
    ep, prob, u, inv = case9
    segs = P.pulse(**PULSE)
    s = PR.NumpyProgrammeSystem(prob, u, inv)
    out = P.run_programme(s, segs, TimeStepPolicy(), dt_init=1.5, dt_restart=0.75)
    assert out["stop_reason"] == "end"
    ends = [g[1] for g in segs]
    assert out["breakpoints"] == ends                                           # ==: every breakpoint is an accepted time
    assert all(t in out["times"] for t in ends) and out["times"][-1] == ends[-1]
    assert all(a < b for a, b in zip(out["times"], out["times"][1:]))
    for t, p, k in zip(out["times"], out["potentials"], out["segments"]):
        assert segs[k][0] < t <= segs[k][1]                                     # a step never straddles a breakpoint
        if t == segs[k][1]:
            assert p == segs[k][3]                                              # ==: the landed potential is the segment's p1
    acc = [r for r in out["log"] if r["accepted"]]
    first_of_segment = [next(r for r in out["log"] if r["segment"] == k) for k in range(len(segs))]
    assert first_of_segment[0]["h"] == 1.5 and first_of_segment[0]["restart"]
    for k in range(1, len(segs)):                                               # every breakpoint of this pulse is a jump
        r = first_of_segment[k]
        assert r["h"] == 0.75 and r["restart"] and r["t"] == segs[k][0]
    assert len(acc) == len(s.records) == len(out["times"])
    assert [st[1] for st in s.states] == ends                                   # full states at the breakpoints only


def test_no_estimate_behind_a_jump_and_none_reset_behind_a_corner(case9):
    ep, prob, u, inv = case9

    class Spy(PR.NumpyProgrammeSystem):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.estimates = []

        def estimate(self, h, h_prev):
            est = super().estimate(h, h_prev)
            self.estimates.append((h, h_prev, est["has_history"], est["err"]))
            return est

    s = Spy(prob, u, inv)
    out = P.run_programme(s, P.pulse(**PULSE), TimeStepPolicy(), dt_init=1.5)
    first = [k for k, r in enumerate(r for r in out["log"] if not math.isnan(r["err"])) if r["restart"]]
    assert len(first) >= 4
    for k in first:
        h, h_prev, hist, err = s.estimates[k]
        assert h_prev == 0.0 and not hist and err == 0.0 and h == 1.5         # dt_restart defaults to dt_init
    assert any(hist for _, _, hist, _ in s.estimates)
    # a triangle has corners only: one first step, at the start
    s = Spy(prob, u, inv)
    tri = P.triangle(P_M, -6.0, 1.0 / 25.0, 1)
    out = P.run_programme(s, tri, TimeStepPolicy(), dt_init=1.5)
    assert out["breakpoints"] == [g[1] for g in tri] and out["potentials"][-1] == P_M
    assert [r["restart"] for r in out["log"]].count(True) == 1 and [e[1] == 0.0 for e in s.estimates].count(True) == 1
    k = out["times"].index(tri[0][1])
    assert out["potentials"][k] == -6.0


def test_a_planted_newton_failure_retries_inside_the_segment(case9):
    ep, prob, u, inv = case9
    segs = P.pulse(**PULSE)
    clean = PR.NumpyProgrammeSystem(prob, u, inv)
    base = P.run_programme(clean, segs, TimeStepPolicy(), dt_init=1.5)
    k_fail = next(k for k, r in enumerate(base["log"]) if r["segment"] == 1 and not r["restart"])   # a solve inside segment 1
    s = PR.NumpyProgrammeSystem(prob, u, inv, fail_solves=[k_fail])
    out = P.run_programme(s, segs, TimeStepPolicy(), dt_init=1.5)
    bad, retry = out["log"][k_fail], out["log"][k_fail + 1]
    assert not bad["accepted"] and bad["reason"] == 2
    assert retry["segment"] == bad["segment"] == 1 and retry["t"] == bad["t"] and retry["h"] == 0.25 * bad["h"]
    assert retry["potential"] == P.programme_value(segs[1], retry["t"] + retry["h"])               # evaluated again at the new t + h
    assert out["breakpoints"] == [g[1] for g in segs] and out["stop_reason"] == "end"
    # with a ramp the retried potential differs from the failed attempt's
    ramp = P.pulse(rise_time=10.0, **PULSE)
    clean = PR.NumpyProgrammeSystem(prob, u, inv)
    base = P.run_programme(clean, ramp, TimeStepPolicy(), dt_init=1.5)
    k_fail = next(k for k, r in enumerate(base["log"]) if r["segment"] == 1 and not r["restart"])
    s = PR.NumpyProgrammeSystem(prob, u, inv, fail_solves=[k_fail])
    out = P.run_programme(s, ramp, TimeStepPolicy(), dt_init=1.5)
    bad, retry = out["log"][k_fail], out["log"][k_fail + 1]
    assert retry["segment"] == 1 and retry["potential"] != bad["potential"]
    assert retry["potential"] == P.programme_value(ramp[1], retry["t"] + retry["h"])
    assert out["breakpoints"] == [g[1] for g in ramp]


def test_fixed_mode_takes_equal_steps_and_lands(case9):
    ep, prob, u, inv = case9
    segs = P.pulse(rise_time=10.0, **PULSE)
    s = PR.NumpyProgrammeSystem(prob, u, inv)
    out = P.run_programme(s, segs, steps_per_segment=4)
    assert len(out["times"]) == 4 * len(segs) and out["breakpoints"] == [g[1] for g in segs]
    for k, g in enumerate(segs):
        hs = {r["h"] for r in out["log"] if r["segment"] == k}
        assert hs == {(g[1] - g[0]) / 4}
        assert out["times"][4 * k + 3] == g[1] and out["potentials"][4 * k + 3] == g[3]
    with pytest.raises(RuntimeError, match="programme"):
        P.run_programme(PR.NumpyProgrammeSystem(prob, u, inv, fail_solves=[2]), segs, steps_per_segment=4)
    with pytest.raises(ValueError, match="programme"):
        P.run_programme(s, [(0.0, 1.0, -5.0, -5.0), (1.5, 2.0, -5.0, -5.0)], steps_per_segment=2)


# ---- the charge identity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["pulse", "triangle"])
@pytest.mark.parametrize("mode", ["adaptive", "fixed"])
def test_accumulated_displacement_charge_closes(case65, kind, mode):
    """Q_D = sum h dD_dt = sum (D_k - D_{k-1}) telescopes: at the end it equals D_last - D_first within 4 ulp of max |D| per accepted
    step (each step rounds one difference, one quotient, one product and one sum)."""
    ep, prob, u, inv = case65
    segs = P.pulse(**PULSE) if kind == "pulse" else P.triangle(P_M, -6.5, 1.5 / 40.0, 2)
    s = PR.NumpyProgrammeSystem(prob, u, inv)
    if mode == "adaptive":
        P.run_programme(s, segs, TimeStepPolicy(), dt_init=1.5)
    else:
        P.run_programme(s, segs, steps_per_segment=6)
    a = s.arrays()
    n = len(a["t"])
    assert n >= 12
    bound = 4.0 * n * float(np.spacing(np.abs(np.r_[a["D"], s.D_first]).max()))
    assert abs(a["Q_D"][-1] - (a["D"][-1] - s.D_first)) <= bound
    assert np.abs(a["D"] - s.D_first).max() > 1e6 * bound                       # the charge moved: the identity is not 0 = 0
    # the kinetic charges are the backward-Euler sums of the currents
    assert np.allclose(a["Q"][-1], (a["h"][:, None] * a["I"]).sum(axis=0), rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("kind", ["pulse", "triangle"])
def test_budget_rows_close_during_a_programme(case9, kind):
    """With the budget on, every accepted step of a programme takes a row per field while u_n is the previous state and inv_dt the
    step's.  As tests/test_budget_reference.py asks of a table: ``dirichlet`` (the remainder of the identity) is the sum of the raw
    residual — Stern and kinetic terms in it — over the Dirichlet dofs, to 1e-12 of the sum of the terms' magnitudes; and as the
    device tests ask of a step (test_gpu_stern_bc._closes): every field's |closure| stays below sqrt(n_free) x the step's last Newton
    residual.  The rows move with the programme: the point entries carry the step's own Stern term and kinetic fluxes."""
    import budget_reference as B
    ep, prob, u, inv = case9
    segs = P.pulse(**PULSE) if kind == "pulse" else P.triangle(P_M, -6.5, 1.5 / 40.0, 1)
    s = PR.NumpyProgrammeSystem(prob, u, inv, budget=True)
    P.run_programme(s, segs, TimeStepPolicy(), dt_init=1.5)
    a = s.arrays()
    n, nf = len(a["t"]), prob.nf
    ns = nf - 1
    assert len(s.budgets) == len(s.residuals) == n >= 8
    bc = np.zeros(prob.ndof, dtype=bool)
    bc[prob.bc_dofs] = True
    bc = bc.reshape(-1, nf)
    n_free = B.n_free(prob)
    for k, ((table, scale, raw), res) in enumerate(zip(s.budgets, s.residuals)):
        assert np.isfinite(table).all()
        for f in range(nf):
            d = raw[bc[:, f], f].sum()
            assert abs(table[f, B.DIR] - d) <= 1e-12 * (scale[f, B.DIR] + np.abs(raw[:, f]).sum()), (k, f)
            assert abs(table[f, B.CLO]) < np.sqrt(n_free[f]) * res, (k, f, table[f, B.CLO], res)
        assert table[ns, B.POINT] == a["D"][k]                                   # the potential row's point entry is the record's D
        assert table[:ns, B.STO].any()                                           # the step stores: inv_dt is the step's, u_n the previous state
    point_CO2 = np.array([t[0][4, B.POINT] for t in s.budgets])
    assert np.ptp(point_CO2) > 1e-3 * np.abs(point_CO2).max()                    # the kinetic flux follows the waveform


# ---- the quasi-steady limit ----------------------------------------------------------------------------------------------------------------
# Scaled time of the short ramp's leg (the long one is 10 T), chosen on the CPU.  Two errors meet in dD_dt / (dp/dt): the lag, which falls
# with T, and the secant of D(p) over one step against the tangent at its end, which depends on dp alone (9 vertices, 8 steps per leg:
# 1.4e-6 at 10 T, 3.6e-6 at 100 T, where nothing but it is left).  T = 200 is where both figures of the reference still fall by more
# than 3 and stay above 1e-6: (I, dD_dt) = (4.7e-2, 2.8e-5) at T and (9.6e-3, 1.4e-6) at 10 T.
QUASI_T = 2.0e2


def quasi_steady_deviation(prob, u, inv, T_leg, steps=8, dv=-0.5):
    """A table programme that ramps from p_M to p_M + 2 dv in 2 T_leg and is read where it lands on the mid potential p_M + dv: (the
    relative deviation of I_r there from the steady state at that potential, the deviation of dD_dt / (dp/dt) from the tangent's dD at
    inv_dt = 0, relative)."""
    mid = P_M + dv
    segs = P.table([0.0, T_leg, 2.0 * T_leg], [P_M, mid, mid + dv])
    s = PR.NumpyProgrammeSystem(prob, u, inv)
    P.run_programme(s, segs, steps_per_segment=steps)
    rec = s.records[steps - 1]
    assert rec["t"] == T_leg and rec["p_M"] == mid
    q = R.with_potential(prob, mid)
    us, _, ok = T.steady_state(q, s.states[0][2])
    assert ok
    I_s = T.currents(q, us)
    _, dD, _, _ = T.tangent(q, us, [0])
    dev_I = float(np.abs(rec["I"][:len(I_s)] - I_s).max() / np.abs(I_s).max())
    dev_C = float(abs(rec["dD_dt"] / (dv / T_leg) - dD[0]) / abs(dD[0]))
    return dev_I, dev_C


def test_quasi_steady_limit(case9):
    """A slow ramp follows the line of steady states: first order in 1/T predicts a factor 10 between T and 10 T; a factor 3 guards
    against a lag that does not shrink.  T is chosen so that dev(T) stays above 1e-6 (rounding is not what is compared)."""
    ep, prob, u, inv = case9
    short = quasi_steady_deviation(prob, u, inv, QUASI_T)
    long_ = quasi_steady_deviation(prob, u, inv, 10.0 * QUASI_T)
    print("quasi-steady deviations (I, dD_dt / (dp/dt)): T %r, 10 T %r" % (short, long_))
    for a, b in zip(short, long_):
        assert a > 1e-6
        assert b < a / 3.0


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------
PULSE_KW = dict(kind="pulse", v_levels=[-5.5, -4.5], durations=[3e-5, 2e-5], cycles=2)


def test_python_refusals():
    """Every refusal is a ValueError that names the programme, raised before anything touches the device (no GPU here)."""
    from gmpnp_amd import edl1d, edl_ensemble, edl_sweep, pore3d, pore_ensemble, rxndiff1d, rxnpore3d, sweep
    t = dict(kinetics="tafel", i0_CO=TAFEL["i0_CO"], i0_H2=TAFEL["i0_H2"])
    c = dict(programme=dict(PULSE_KW))
    calls = {
        "no electrode voltage": lambda: edl1d.EDLRun(**c),
        "target_current": lambda: edl1d.EDLRun(electrode_voltage=-5.0, target_current=10.0, **t, **c),
        "polarisation": lambda: edl1d.EDLRun(electrode_voltage=-5.0, polarisation=dict(v_end=-10.0, v_step=-1.0), **c),
        "fit": lambda: edl1d.EDLRun(electrode_voltage=-5.0, fit=dict(data="no_such_file.npz"), **t, **c),
        "stabilization": lambda: edl1d.EDLRun(electrode_voltage=-5.0, stabilization="Y", model="PNP", **c),
        "H_OHP": lambda: edl1d.EDLRun(electrode_voltage=-5.0, H_OHP=0.5, **c),
        "dt_order": lambda: edl1d.EDLRun(electrode_voltage=-5.0, adaptive_dt=True, dt_order=2, **c),
        "unknown kind": lambda: edl1d.EDLRun(electrode_voltage=-5.0, programme=dict(kind="sine", amplitude=1.0)),
        "missing field": lambda: edl1d.EDLRun(electrode_voltage=-5.0, programme=dict(kind="pulse", v_levels=[-5.0, -6.0])),
        "unknown field": lambda: edl1d.EDLRun(electrode_voltage=-5.0, programme=dict(PULSE_KW, scan_rate=1.0)),
        "duration below the rise time": lambda: edl1d.EDLRun(electrode_voltage=-5.0, programme=dict(PULSE_KW, rise_time=2e-5)),
        "zero scan rate": lambda: edl1d.EDLRun(electrode_voltage=-5.0, programme=dict(kind="triangle", v_vertex=-6.0, scan_rate=0.0)),
        "vertex at the start": lambda: edl1d.EDLRun(electrode_voltage=-5.0, programme=dict(kind="triangle", v_vertex=-5.0, scan_rate=1.0)),
        "table going back": lambda: edl1d.EDLRun(electrode_voltage=-5.0, programme=dict(kind="table", time_s=[0.0, 2e-5, 1e-5], electrode_voltage=[-5.0] * 3)),
        "dt_init": lambda: edl1d.EDLRun(electrode_voltage=-5.0, programme=dict(PULSE_KW, dt_init=0.0)),
        "steps_per_segment": lambda: edl1d.EDLRun(electrode_voltage=-5.0, programme=dict(PULSE_KW, steps_per_segment=0)),
        "PoreRun": lambda: pore3d.PoreRun(electrode_voltage=-1.0, **c),
        "rxn 1D": lambda: rxndiff1d.RxnDiffRun(**c),
        "rxn 3D": lambda: rxnpore3d.RxnPoreRun(**c),
        "EDLEnsemble": lambda: edl_ensemble.EDLEnsemble([dict(voltage_multiplier=-1.0), dict(voltage_multiplier=-1.0, **c)]),
        "PoreEnsemble": lambda: pore_ensemble.PoreEnsemble([dict(**c)]),
        "edl sweep": lambda: edl_sweep.run_sweep([dict(**c)]),
        "edl sweep keywords": lambda: edl_sweep.run_sweep([dict(voltage_multiplier=-1.0)], **c),
        "pore sweep group": lambda: sweep.run_group(5, [-1.0], 1, **c),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError, match="programme"):
            call()
    with pytest.raises(ValueError, match="programme"):
        edl1d.main(["--programme", "pulse", "--v_levels", "-5", "-6", "--durations", "1e-5", "1e-5"])     # no --electrode_voltage
    with pytest.raises(ValueError, match="programme"):
        edl1d.main(["--programme", "pulse", "--electrode_voltage", "-5"])                                  # no levels
    with pytest.raises(ValueError, match="programme"):
        edl1d.main(["--programme", "triangle", "--electrode_voltage", "-5", "--v_vertex", "-6"])           # no scan rate
    with pytest.raises(ValueError, match="programme"):
        edl1d.main(["--programme", "table", "--electrode_voltage", "-5"])                                  # no file
    with pytest.raises(ValueError, match="programme"):
        P.refuse_programme(c, "a test")
    P.refuse_programme({}, "a test")


def test_command_lines(tmp_path):
    from gmpnp_amd import edl1d, edl_sweep, pore3d, rxndiff1d, rxnpore3d, sweep
    a = edl1d.build_parser().parse_args([])
    assert a.programme is None and P.programme_keywords(a) == {}
    a = edl1d.build_parser().parse_args(["--programme", "pulse", "--v_levels", "-5.5", "-4.5", "--durations", "3e-5", "2e-5", "--cycles", "3", "--rise_time", "1e-6",
                                         "--programme_dt_init", "0.5", "--programme_steps_per_segment", "4"])
    assert P.programme_keywords(a) == {"programme": dict(kind="pulse", v_levels=[-5.5, -4.5], durations=[3e-5, 2e-5], cycles=3, rise_time=1e-6, dt_init=0.5,
                                                         steps_per_segment=4)}
    a = edl1d.build_parser().parse_args(["--programme", "triangle", "--v_vertex", "-9", "--scan_rate", "0.1", "--cycles", "2"])
    assert P.programme_keywords(a) == {"programme": dict(kind="triangle", v_vertex=-9.0, scan_rate=0.1, cycles=2)}
    f = tmp_path / "table.csv"
    f.write_text("time_s,electrode_voltage\n0,-5\n1e-5,-5\n1e-5,-6\n4e-5,-6\n")
    a = edl1d.build_parser().parse_args(["--programme", "table", "--programme_file", str(f)])
    kw = P.programme_keywords(a)
    assert kw == {"programme": dict(kind="table", time_s=[0.0, 1e-5, 1e-5, 4e-5], electrode_voltage=[-5.0, -5.0, -6.0, -6.0])}
    par = P.check_programme(kw["programme"], dict(electrode_voltage=-5.0))
    segs = P.build(par, -5.0, 1e-6, 0.025)
    assert [g[2:] for g in segs] == [(-5.0, -5.0), (-6.0, -6.0)] and P.programme_jump(segs, 0) and segs[0][1] == 1e-5 / 1e-6
    # the other drivers' parsers do not know the flags
    for mod in (pore3d, rxndiff1d, rxnpore3d, edl_sweep):
        with pytest.raises(SystemExit):
            mod.build_parser().parse_args(["--programme", "pulse"])
    with pytest.raises(SystemExit):
        sweep.main(["--programme", "pulse"])                                     # (its parser lives in main: refused before anything else)
    # units: seconds by time_constant, V/s by time_constant / thermal_voltage, and nothing else
    assert P.scaled_time(3e-5, 1.5e-6) == 3e-5 / 1.5e-6 and P.scaled_scan_rate(0.1, 1.5e-6, 0.025) == 0.1 * 1.5e-6 / 0.025
    tri = P.build(dict(kind="triangle", v_vertex=-9.0, scan_rate=0.1, cycles=1), -5.0, 1.5e-6, 0.025)
    assert tri[0][2:] == (-5.0, -9.0) and tri[0][1] == 4.0 / (0.1 * 1.5e-6 / 0.025) and tri[1][3] == -5.0


def test_output_arrays_units_and_signs():
    """programme.npz from a hand-made record: the units, i_charging = -d(surface_charge)/dt, the charges, the cycle averages."""
    from gmpnp_amd import backend
    from types import SimpleNamespace
    ep = SimpleNamespace(thermal_voltage=0.025, time_constant=2e-6, L_n=1e-6)
    eps_0 = 8.8e-12
    rec = np.zeros(4, dtype=backend.ELECTRODE_RECORD_DTYPE)
    rec["t"], rec["h"], rec["p_M"], rec["p_boundary"] = [1.0, 2.0, 3.0, 4.0], 1.0, [-5.0, -5.0, -6.0, -6.0], [-2.0, -2.0, -2.5, -2.5]
    rec["D"] = [-10.0, -10.0, -12.0, -13.0]
    acc = P.fresh_accumulators(-10.0)
    for k in range(4):
        rec["I"][k, :2] = (1.0 + k, 0.5)
        rec["dD_dt"][k] = P.electrode_record_combine(acc, 1.0, rec["D"][k], rec["I"][k])
        rec["Q"][k], rec["Q_D"][k] = acc["Q"], acc["Q_D"]
    rec["u_boundary"][:, 4] = 0.25
    segs = P.pulse([-5.0, -6.0], [2.0, 2.0], 1)
    out = P.output_arrays(ep, eps_0, rec, [0, 0, 1, 1], segs, 1)
    assert sorted(out) == sorted(P.OUTPUT_KEYS)
    q = eps_0 * 0.025 / 1e-6
    assert np.array_equal(out["time_s"], rec["t"] * 2e-6) and np.array_equal(out["potential_OHP"], rec["p_boundary"] * 0.025)
    assert np.array_equal(out["surface_charge"], q * rec["D"]) and np.all(out["surface_charge"] < 0.0)
    assert np.allclose(out["i_charging"], [0.0, 0.0, 2.0 * q / 2e-6, q / 2e-6]) and np.all(out["i_charging"] >= 0.0)     # the potential fell: cathodic
    assert np.allclose(out["i_charging"][1:], -np.diff(out["surface_charge"]) / np.diff(out["time_s"]))
    assert np.allclose(out["charge_double_layer"], -(out["surface_charge"] - q * -10.0))
    assert np.array_equal(out["i_total"], out["i_CO"] + out["i_H2"] + out["i_charging"])
    assert np.allclose(out["charge_CO"], np.cumsum(out["i_CO"]) * 2e-6) and np.allclose(out["charge_H2"], np.cumsum(out["i_H2"]) * 2e-6)
    assert np.allclose(out["FE_H2"], 0.5 / (np.array([1.0, 2.0, 3.0, 4.0]) + 0.5)) and np.allclose(out["FE_H2_cycle"], [2.0 / 12.0])
    assert np.array_equal(out["OHP_CO2"], [0.25] * 4) and np.array_equal(out["segment"], [0, 0, 1, 1])


def test_cycle_averages_with_a_rise_time():
    """FE_H2_cycle of a pulse with a rise time: the first cycle has one segment fewer than the others (no ramp in front of the first
    hold), so cycles are told apart by time, not by counting segments.  Each value is charge_H2 / (charge_CO + charge_H2) of that
    cycle's own steps, and every step belongs to a cycle."""
    from gmpnp_amd import backend
    from types import SimpleNamespace
    ep = SimpleNamespace(thermal_voltage=0.025, time_constant=2e-6, L_n=1e-6)
    for cycles in (2, 3, 50):
        segs = P.pulse([-5.0, -6.0], [3.0, 2.0], cycles, rise_time=0.5)
        assert len(segs) == 4 * cycles - 1
        want_cycle = [0, 0, 0] + [c for c in range(1, cycles) for _ in range(4)]
        assert P.segment_cycles(segs, cycles).tolist() == want_cycle
        steps = [(k, g[0] + (j + 1) * (g[1] - g[0]) / 2.0, (g[1] - g[0]) / 2.0) for k, g in enumerate(segs) for j in range(2)]   # two per segment
        rec = np.zeros(len(steps), dtype=backend.ELECTRODE_RECORD_DTYPE)
        rng = np.random.default_rng(cycles)
        rec["t"], rec["h"] = [t for _, t, _ in steps], [h for _, _, h in steps]
        rec["I"][:, 0], rec["I"][:, 1] = rng.uniform(1.0, 3.0, len(steps)), rng.uniform(0.1, 0.9, len(steps))
        seg = [k for k, _, _ in steps]
        out = P.output_arrays(ep, 8.8e-12, rec, seg, segs, cycles)
        assert out["FE_H2_cycle"].shape == (cycles,) and np.isfinite(out["FE_H2_cycle"]).all()
        period = 5.0
        used = np.zeros(len(steps), dtype=bool)
        for c in range(cycles):
            m = (rec["t"] > c * period + 1e-9) & (rec["t"] <= (c + 1) * period + 1e-9)       # the steps that end inside the cycle's window
            used |= m
            qc, qh = (rec["h"][m] * rec["I"][m, 0]).sum(), (rec["h"][m] * rec["I"][m, 1]).sum()
            assert m.sum() == (6 if c == 0 else 8) and abs(out["FE_H2_cycle"][c] - qh / (qc + qh)) <= 1e-15
        assert used.all()
    tri = P.triangle(-5.0, -6.0, 0.25, 3)
    assert P.segment_cycles(tri, 3).tolist() == [0, 0, 1, 1, 2, 2] and P.segment_cycles(P.table([0.0, 1.0, 1.0, 3.0], [-5.0, -5.0, -6.0, -6.0]), 1).tolist() == [0, 0]
