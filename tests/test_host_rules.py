"""gmpnp_host_rules.h — the Newton verdict, the predicted start, the policies of the linear solves inside Newton, the options'
resolution and the multilevel level tables — compiled with the host compiler alone (that it compiles without HIP is the assertion
that the header is device-free) and checked against the oracle's stop rule, the recorded reference histories and Python / NumPy
restatements written out here."""
import glob
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")
OK, ERR_NOT_CONVERGED, ERR_LINEAR, ERR_NUMERIC = 0, -3, -4, -5
MAX_HISTORY = 64
T_LIMIT = "Newton solver did not converge because maximum number of iterations reached"
T_NAN_FIRST = "residual is NaN before the first Newton iteration"
T_NAN = "residual became NaN"
T_NAN_STERIC = "residual became NaN / Inf after an iterate left the admissible set (1 - sum_j a_j u_j <= 0)"
BITS = {1: "1 - sum_j a_j u_j <= 0 at a quadrature point; ", 2: "singular diagonal node block; ", 4: "singular coarse operator; ",
        8: "in-launch hand-over timed out; "}

# One command per input line, one answer per output line:
#   judge rtol atol maxit strict n  r_0 flags_0 ... r_{n-1} flags_{n-1}     a driver's loop: first(), then iterations++ / next()
#   start warm_start omega iteration
#   accept wb ww bb
#   tables partitions f0 f1 c0 c1 nvf perm[nvf] nvc iperm[nvc] parents[2 nvf]
# The policies: a history of n events in one line, the decision and the whole state after every event in the answer (";" between events)
#   coarse async lag n  (newton_it jumped fell_back iters)*n          fresh(), solved() [, fell_back()]
#   gcoarse n  (newton_it jumped iters)*n                             rebuild(), solved()
#   direct n  (event arg)*n                                           0 use_direct()  1 krylov_converged(arg)  2 fell_back()  3 newton_done(arg)
#   burst krylov_batch B n  (event a b c)*n                           0 expect(a)  1 first(a, .., b)  2 solve_done(a, b, c)  3 record(a, b)
#   gburst n  (event a b c d)*n                                       0 predicted(a, b, c)  1 first(a, b)  2 record(a, b, c, d)  3 solve_done(a)
#   x0 n  (event a scale)*n                                           0 ready(a, scale)  1 left(a)
#   options dim  <the 16 int32 fields of gmpnp_options_t in order>  band_lu_max_gb
#   refine round finite rn best tol                                   band_refine_again: 1 = another refinement round of a band LU solve
#   records first n count capacity t h                                record_range_valid, record_can_append, record_step_valid, record_rows
DRIVER = r"""
#include <cstdio>
#include <iostream>
#include <sstream>
#include "gmpnp_host_rules.h"
using namespace gmpnp;
static void ints(const std::vector<int32_t>& v) { for (int32_t x : v) printf(" %d", x); printf(" ;"); }
int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd, tok; in >> cmd;
    auto num = [&]() { in >> tok; return std::stod(tok); };   // (reads "nan" and "inf" too)
    if (cmd == "judge") {
      gmpnp_newton_options_t o{}; gmpnp_newton_stats_t st{};
      o.relative_tolerance = num(); o.absolute_tolerance = num(); o.maximum_iterations = (int)num();
      const bool strict = num() != 0.0; const int n = (int)num();
      NewtonJudge j(o, st, strict);
      static const char* name[] = {"go_on", "converged", "limit", "failed"};
      NewtonJudge::Verdict v = NewtonJudge::go_on;
      for (int k = 0; k < n && v == NewtonJudge::go_on; ++k) {
        const double r = num(); const int flags = (int)num();
        if (k == 0) v = j.first(r, flags); else { st.iterations++; v = j.next(r, flags); }
        printf("%s ", name[v]);
      }
      printf("|%d|%d|%d|%d|%d|", j.code, st.n_residuals, st.converged, st.steric_excursion, st.iterations);
      for (int k = 0; k < st.n_residuals; ++k) printf("%.17g ", st.residuals[k]);
      printf("|%s\n", j.message.c_str());
    } else if (cmd == "start") {
      const int ws = (int)num(); const double omega = num(); const int it = (int)num();
      const std::pair<double, double> p = predicted_start(ws, 1.0 - omega, it);
      printf("%.17g %.17g\n", p.first, p.second);
    } else if (cmd == "accept") {
      const double wb = num(), ww = num(), bb = num(); double rn = -1.0;
      const bool ok = accept_predicted_start(wb, ww, bb, &rn);
      printf("%d %.17g\n", ok ? 1 : 0, rn);
    } else if (cmd == "tables") {
      const bool part = num() != 0.0;
      const int f0 = (int)num(), f1 = (int)num(), c0 = (int)num(), c1 = (int)num();
      std::vector<int32_t> perm((size_t)num()); for (auto& x : perm) x = (int32_t)num();
      std::vector<int32_t> iperm((size_t)num()); for (auto& x : iperm) x = (int32_t)num();
      std::vector<int32_t> parents(2 * perm.size()); for (auto& x : parents) x = (int32_t)num();
      LevelTables t;
      const std::string err = build_level_tables(perm, iperm, f0, f1, c0, c1, parents.data(), part, &t);
      if (!err.empty()) printf("ERR %s\n", err.c_str());
      else { printf("OK"); ints(t.par); ints(t.copy); ints(t.child_ptr); ints(t.child); printf("\n"); }
    } else if (cmd == "coarse") {
      const bool async = num() != 0.0; const int lag = (int)num(), n = (int)num();
      CoarseReuse c;
      for (int k = 0; k < n; ++k) {
        const int it = (int)num(); const bool jumped = num() != 0.0, fell = num() != 0.0; const int iters = (int)num();
        const bool fresh = c.fresh(async, lag, it, jumped);
        c.solved(fresh, iters);
        if (fell) c.fell_back();
        printf("%d %d %d;", fresh ? 1 : 0, c.refresh_due ? 1 : 0, c.fresh_iters);
      }
      printf("\n");
    } else if (cmd == "gcoarse") {
      const int n = (int)num();
      GroupCoarseReuse c;
      for (int k = 0; k < n; ++k) {
        const int it = (int)num(); const bool jumped = num() != 0.0; const int iters = (int)num();
        const bool rebuild = c.rebuild(it, jumped);
        c.solved(rebuild, iters);
        printf("%d %d %d %d;", rebuild ? 1 : 0, c.age, c.fresh_iters, c.slow ? 1 : 0);
      }
      printf("\n");
    } else if (cmd == "direct") {
      const int n = (int)num();
      DirectFallback d;
      for (int k = 0; k < n; ++k) {
        const int ev = (int)num(), arg = (int)num();
        if (ev == 1) d.krylov_converged(arg); else if (ev == 2) d.fell_back(); else if (ev == 3) d.newton_done(arg != 0);
        printf("%d %d %d;", d.use_direct() ? 1 : 0, d.sticky, d.backoff);
      }
      printf("\n");
    } else if (cmd == "burst") {
      const int batch = (int)num(), B = (int)num(), n = (int)num();
      BurstHint h;
      for (int k = 0; k < n; ++k) {
        const int ev = (int)num(), a = (int)num(), b = (int)num(), c = (int)num();
        int val = -1;
        if (ev == 0) h.expect(a); else if (ev == 1) val = h.first(a, batch, B, b != 0); else if (ev == 2) h.solve_done(a, b, c != 0); else h.record(a, b);
        printf("%d %d %d %d", val, h.hint, h.last[0], h.last[1]);
        for (int x : h.by_newton_it) printf(" %d", x);
        printf(";");
      }
      printf("\n");
    } else if (cmd == "gburst") {
      const int n = (int)num();
      GroupBurstHint h;
      for (int k = 0; k < n; ++k) {
        const int ev = (int)num(), a = (int)num(), b = (int)num(), c = (int)num(), d = (int)num();
        int val = -1;
        if (ev == 0) val = h.predicted(a, b != 0, c); else if (ev == 1) val = h.first(a, b != 0); else if (ev == 2) h.record(a, b != 0, c, d); else h.solve_done(a);
        printf("%d %d", val, h.last);
        for (int x : h.by_newton_it) printf(" %d", x);
        printf(";");
      }
      printf("\n");
    } else if (cmd == "x0") {
      const int n = (int)num();
      PredictedX0 x;
      for (int k = 0; k < n; ++k) {
        const int ev = (int)num(), a = (int)num(); const double scale = num();
        bool ready = false;
        if (ev == 0) ready = x.ready(a, scale); else x.left(a != 0);
        printf("%d %d;", ready ? 1 : 0, x.held ? 1 : 0);
      }
      printf("\n");
    } else if (cmd == "options") {
      const int dim = (int)num();
      gmpnp_options_t o{};
      int32_t* f[] = {&o.device_id, &o.n_aggregates, &o.shared_device, &o.krylov_batch, &o.profile_every, &o.launch_form, &o.warm_start, &o.coarse_refresh,
                      &o.progress_by_copy, &o.burst_iterations, &o.phase_timing, &o.no_direct_fallback, &o.warm_in_stream, &o.vector_form, &o.strict_steric,
                      &o.element_stores};
      for (int32_t* x : f) *x = (int32_t)num();
      o.band_lu_max_gb = num();
      Settings s;
      const std::string err = resolve_options(o, dim, &s);
      if (!err.empty()) printf("ERR %s\n", err.c_str());
      else printf("OK %d %d %d %d %d %d %d %d %d %.17g\n", s.coarse_async, s.coarse_lag, s.warm_async, s.warm_start, s.host_poll, s.burst_iters,
                  s.phase_timing ? 1 : 0, s.direct_fallback, s.strict_steric, s.lu_max_gb);
    } else if (cmd == "refine") {
      const int round = (int)num(); const bool finite = num() != 0.0; const double rn = num(), best = num(), tol = num();
      printf("%d\n", band_refine_again(round, finite, rn, best, tol) ? 1 : 0);
    } else if (cmd == "records") {
      const int32_t first = (int32_t)num(), n = (int32_t)num(); const int count = (int)num(), capacity = (int)num();
      const double t = num(), h = num();
      printf("%d %d %d %zu\n", record_range_valid(first, n, count) ? 1 : 0, record_can_append(count, capacity) ? 1 : 0,
             record_step_valid(t, h) ? 1 : 0, record_rows(capacity));
    }
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    """Compiles the driver with g++ (no HIP anywhere on the command line) and returns ask(lines) -> answer lines."""
    d = tmp_path_factory.mktemp("host_rules")
    src, exe = d / "rules.cpp", d / "rules"
    src.write_text(DRIVER)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "gmpnp_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True)

    def ask(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
        assert len(out) == len(lines), (len(out), len(lines))
        return out
    return ask


def judge_line(rtol, atol, maxit, strict, seq):
    """seq: (residual, status flags) of the evaluation before the first iteration and after every update."""
    return "judge %r %r %d %d %d " % (rtol, atol, maxit, strict, len(seq)) + " ".join("%r %d" % (float(r), f) for r, f in seq)


def parse_judge(line):
    verdicts, code, nres, conv, steric, its, res, msg = line.split("|")
    return {"verdicts": verdicts.split(), "code": int(code), "n_residuals": int(nres), "converged": int(conv), "steric": int(steric),
            "iterations": int(its), "residuals": np.array([float(x) for x in res.split()]), "message": msg}


def oracle_conv(res, r0, rtol, atol):
    """oracle/gmpnp_oracle.py, newton_solve.conv ([3P] dolfin::NewtonSolver, criterion "residual")."""
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.float64(res) / np.float64(r0)
    return bool(rel < rtol or res < atol)


def test_judge_reproduces_every_recorded_reference_history(rules):
    """Every row of every tests/golden/*_steps.npz (none left out): 'go on' for every residual before index newton_its[k],
    'converged' at it, with the tolerances of the driver that recorded the file; the oracle's rule says the same of each row."""
    cases = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, "*_steps.npz"))):
        z = np.load(path)
        tol = 1e-6 if os.path.basename(path).startswith("rxn1d_") else 1e-4
        for row, its in zip(z["residuals"], z["newton_its"]):
            cases.append((os.path.basename(path), tol, row, int(its)))
    assert len(cases) == 75
    answers = rules([judge_line(tol, tol, 50, 0, [(r, 0) for r in row[:its + 1]]) for _, tol, row, its in cases])
    for (name, tol, row, its), line in zip(cases, answers):
        assert np.all(np.isfinite(row[:its + 1])) and np.all(np.isnan(row[its + 1:])), name
        assert [oracle_conv(r, row[0], tol, tol) for r in row[:its + 1]] == [False] * its + [True], name
        a = parse_judge(line)
        assert a["verdicts"] == ["go_on"] * its + ["converged"], (name, a)
        assert (a["code"], a["converged"], a["steric"], a["iterations"], a["n_residuals"], a["message"]) == (OK, 1, 0, its, its + 1, ""), (name, a)
        assert np.array_equal(a["residuals"], row[:its + 1]), name


def test_judge_edges(rules):
    nan, inf = float("nan"), float("inf")
    go, conv, limit, failed = "go_on", "converged", "limit", "failed"
    # (rtol, atol, maxit, strict, sequence) -> (verdicts, code, message, converged, steric, recorded residuals)
    table = [
        # r0 = 0: 0/0 compares false, the absolute test decides; with atol = 0 nothing ever converges and the limit ends the solve
        ((1e-4, 1e-4, 50, 0, [(0.0, 0)]), ([conv], OK, "", 1, 0, 1)),
        ((1e-4, 0.0, 2, 0, [(0.0, 0), (0.0, 0), (0.0, 0)]), ([go, go, limit], ERR_NOT_CONVERGED, T_LIMIT, 0, 0, 3)),
        # NaN first; NaN / Inf later, with and without bit 1 in that evaluation's flags
        ((1e-4, 1e-4, 50, 0, [(nan, 0)]), ([failed], ERR_NUMERIC, T_NAN_FIRST, 0, 0, 1)),
        ((1e-4, 1e-4, 50, 0, [(1.0, 0), (nan, 0)]), ([go, failed], ERR_NUMERIC, T_NAN, 0, 0, 2)),
        ((1e-4, 1e-4, 50, 0, [(1.0, 0), (inf, 0)]), ([go, failed], ERR_NUMERIC, T_NAN, 0, 0, 2)),
        ((1e-4, 1e-4, 50, 0, [(1.0, 0), (nan, 1)]), ([go, failed], ERR_NUMERIC, T_NAN_STERIC, 0, 1, 2)),
        ((1e-4, 1e-4, 50, 0, [(1.0, 0), (inf, 1)]), ([go, failed], ERR_NUMERIC, T_NAN_STERIC, 0, 1, 2)),
        ((1e-4, 1e-4, 50, 0, [(1.0, 1), (0.5, 0), (nan, 0)]), ([go, go, failed], ERR_NUMERIC, T_NAN, 0, 1, 3)),   # bit 1 of an EARLIER evaluation
        # bit 1: information, fatal only with strict_steric (before the first iteration and after an update; nothing recorded then)
        ((1e-4, 1e-4, 50, 0, [(1.0, 1), (1e-6, 0)]), ([go, conv], OK, "", 1, 1, 2)),
        ((1e-4, 1e-4, 50, 0, [(1.0, 0), (1e-6, 1)]), ([go, conv], OK, "", 1, 1, 2)),
        ((1e-4, 1e-4, 50, 1, [(1.0, 1)]), ([failed], ERR_NUMERIC, BITS[1], 0, 1, 0)),
        ((1e-4, 1e-4, 50, 1, [(1.0, 0), (0.5, 1)]), ([go, failed], ERR_NUMERIC, BITS[1], 0, 1, 1)),
        ((1e-4, 1e-4, 50, 1, [(1.0, 0), (0.5, 3)]), ([go, failed], ERR_NUMERIC, BITS[1] + BITS[2], 0, 1, 1)),
        # maximum_iterations = 0
        ((1e-4, 1e-4, 0, 0, [(1.0, 0)]), ([limit], ERR_NOT_CONVERGED, T_LIMIT, 0, 0, 1)),
        ((1e-4, 1e-4, 0, 0, [(1e-5, 0)]), ([conv], OK, "", 1, 0, 1)),
        # the limit after updates; convergence at the limit wins
        ((1e-4, 1e-4, 2, 0, [(1.0, 0), (0.5, 0), (0.25, 0)]), ([go, go, limit], ERR_NOT_CONVERGED, T_LIMIT, 0, 0, 3)),
        ((1e-4, 1e-4, 2, 0, [(1.0, 0), (0.5, 0), (1e-5, 0)]), ([go, go, conv], OK, "", 1, 0, 3)),
        # relative test alone / absolute test alone
        ((1e-4, 0.0, 50, 0, [(1e3, 0), (1.0, 0), (0.05, 0)]), ([go, go, conv], OK, "", 1, 0, 3)),
        ((0.0, 1e-4, 50, 0, [(1e3, 0), (1.0, 0), (0.99e-4, 0)]), ([go, go, conv], OK, "", 1, 0, 3)),
    ]
    # bits 2 / 4 / 8: GMPNP_ERR_LINEAR after an update (the residual is not recorded), ignored before the first iteration
    for bit in (2, 4, 8):
        table.append(((1e-4, 1e-4, 50, 0, [(1.0, 0), (0.5, bit)]), ([go, failed], ERR_LINEAR, BITS[bit], 0, 0, 1)))
        table.append(((1e-4, 1e-4, 50, 0, [(1.0, bit), (1e-6, 0)]), ([go, conv], OK, "", 1, 0, 2)))
    table.append(((1e-4, 1e-4, 50, 0, [(1.0, 0), (nan, 14)]), ([go, failed], ERR_LINEAR, BITS[2] + BITS[4] + BITS[8], 0, 0, 1)))
    for (args, want), line in zip(table, rules([judge_line(*a) for a, _ in table])):
        a = parse_judge(line)
        got = (a["verdicts"], a["code"], a["message"], a["converged"], a["steric"], a["n_residuals"])
        assert got == want, (args, a)
        kept = [r for r, _ in args[4]][:a["n_residuals"]]
        assert np.array_equal(a["residuals"], np.array(kept), equal_nan=True), (args, a)


def test_judge_history_stops_growing_and_the_verdicts_do_not(rules):
    res = [0.99 ** k for k in range(80)] + [1e-9]   # 80 updates, converged at the last
    a = parse_judge(rules([judge_line(1e-4, 1e-4, 100, 0, [(r, 0) for r in res])])[0])
    assert a["verdicts"] == ["go_on"] * 80 + ["converged"] and a["code"] == OK and a["converged"] == 1 and a["iterations"] == 80
    assert a["n_residuals"] == MAX_HISTORY and np.array_equal(a["residuals"], np.array(res[:MAX_HISTORY]))
    a = parse_judge(rules([judge_line(1e-4, 1e-4, 70, 0, [(r, 0) for r in res[:71]])])[0])
    assert a["verdicts"] == ["go_on"] * 70 + ["limit"] and (a["code"], a["message"], a["converged"]) == (ERR_NOT_CONVERGED, T_LIMIT, 0)
    assert a["n_residuals"] == MAX_HISTORY


def test_predicted_start(rules):
    cases = [(ws, om, it) for ws in (0, 1, 2) for om in (0.9, 1.0) for it in (0, 1, 2, 3)]
    for (ws, om, it), line in zip(cases, rules(["start %d %r %d" % c for c in cases])):
        q = 1.0 - om
        if ws == 0 or q == 0.0 or it < 1:
            want = (0.0, 0.0)
        elif ws > 1 and it > 1:
            want = (q + q * q, -q * q * q)   # x0 = q dx_k + q^2 (dx_k - q dx_{k-1})
        else:
            want = (q, 0.0)
        assert tuple(float(x) for x in line.split()) == want, (ws, om, it, line)


def test_accept_predicted_start(rules):
    # ||b - w||^2 = bb - 2 wb + ww: taken when finite, non-negative and below a quarter of bb
    cases = [((1.0, 1.0, 1.0), (1, 0.0)), ((0.9, 0.9, 1.0), (1, np.sqrt(1.0 - 1.8 + 0.9))), ((0.5, 0.5, 1.0), (0, -1.0)),
             ((0.0, 0.0, 1.0), (0, -1.0)), ((2.0, 1.0, 1.0), (0, -1.0)), ((float("nan"), 1.0, 1.0), (0, -1.0)),
             ((0.0, 0.0, 0.0), (0, -1.0)), ((3.0, 4.0, 4.0), (0, -1.0)), ((0.8, 0.9, 1.0), (0, -1.0)),
             ((0.5, 0.25, 1.0), (0, -1.0)), ((0.5, 0.2499, 1.0), (1, np.sqrt(1.0 - 1.0 + 0.2499)))]   # the quarter itself is refused
    for (args, want), line in zip(cases, rules(["accept %r %r %r" % a for a, _ in cases])):
        ok, rn = line.split()
        assert (int(ok), float(rn)) == want, (args, line)


# ---- level tables: a path of 5 coarse vertices and its 9-vertex bisection ---------------------------------------------------
# global numbering along the path: fine vertex 2 i is the copy of coarse vertex i, fine vertex 2 i + 1 lies between i and i + 1
def nested_pair(fine_glob, coarse_glob):
    """Local parents table (coarse LOCAL file order, -1 = not local) of the handle pair holding these global vertices, in this
    local file order."""
    loc = {g: k for k, g in enumerate(coarse_glob)}
    par = []
    for g in fine_glob:
        a, b = (g // 2, g // 2) if g % 2 == 0 else (g // 2, g // 2 + 1)
        par += [loc.get(a, -1), loc.get(b, -1)]
    return par


def tables_line(part, f0, f1, c0, c1, perm, iperm, parents):
    return "tables %d %d %d %d %d %d %s %d %s %s" % (part, f0, f1, c0, c1, len(perm), " ".join(map(str, perm)), len(iperm),
                                                      " ".join(map(str, iperm)), " ".join(map(str, parents)))


def expected_tables(f0, f1, c0, c1, perm, iperm, parents):
    """par / copy / child_ptr / child in the internal orders (perm[internal] = file, iperm[file] = internal), owned rows only."""
    nvf, nvc = len(perm), len(iperm)
    P = np.array(parents).reshape(-1, 2)[np.array(perm)]                    # parents of internal fine vertex I, coarse file order
    PI = np.where(P >= 0, np.array(iperm)[np.maximum(P, 0)], -1)            # ... coarse internal order
    is_copy = (P[:, 0] == P[:, 1]) & (P[:, 0] >= 0)
    owned_f = (np.arange(nvf) >= f0) & (np.arange(nvf) < f1)
    par = np.where(owned_f[:, None], np.c_[PI[:, 0], np.where(is_copy, -1, PI[:, 1])], [0, -1])
    copy, ptr, child = [], [0], []
    for Ic in range(nvc):
        own = c0 <= Ic < c1
        copy.append(int(np.flatnonzero(is_copy & (PI[:, 0] == Ic))[0]) if own else -1)
        if own:   # every local fine vertex naming Ic, ascending internal index; low bit 0 = the copy (weight 1), 1 = a midpoint (1/2)
            child += [2 * I + (0 if is_copy[I] else 1) for I in range(nvf) if Ic in PI[I]]
        ptr.append(len(child))
    return [list(par.ravel()), copy, ptr, child]


def inverse(perm):
    inv = [0] * len(perm)
    for i, p in enumerate(perm):
        inv[p] = i
    return inv


# (partitions, fine global ids in local file order, fine perm, owned fine range, coarse global ids, coarse perm, owned coarse range)
LEVEL_CASES = {
    "unpartitioned": (0, list(range(9)), [3, 0, 8, 5, 1, 6, 2, 7, 4], (0, 9), list(range(5)), [2, 4, 0, 3, 1], (0, 5)),
    # split in two, one ghost layer: rank 0 owns fine 0..4 / coarse 0..2, rank 1 the rest; internal order = owned range, then ghosts
    "rank0": (1, [5, 2, 0, 4, 1, 3], [2, 4, 1, 5, 3, 0], (0, 5), [3, 1, 0, 2], [2, 1, 3, 0], (0, 3)),
    "rank1": (1, [8, 4, 6, 5, 7], [1, 3, 2, 4, 0], (1, 5), [4, 2, 3], [1, 2, 0], (1, 3)),
    # ... and rank 0 with no ghost on the coarse level: the ghost fine vertex 5 has one parent that is not local (-1)
    "rank0_coarse_without_ghost": (1, [5, 2, 0, 4, 1, 3], [2, 4, 1, 5, 3, 0], (0, 5), [1, 0, 2], [1, 0, 2], (0, 3)),
}


@pytest.mark.parametrize("case", sorted(LEVEL_CASES))
def test_level_tables(rules, case):
    part, fglob, perm, (f0, f1), cglob, cperm, (c0, c1) = LEVEL_CASES[case]
    parents, iperm = nested_pair(fglob, cglob), inverse(cperm)
    if case == "rank0_coarse_without_ghost":
        assert -1 in parents
    line = rules([tables_line(part, f0, f1, c0, c1, perm, iperm, parents)])[0]
    assert line.startswith("OK"), line
    got = [[int(x) for x in grp.split()] for grp in line[2:].split(";")[:4]]
    assert got == expected_tables(f0, f1, c0, c1, perm, iperm, parents)


def test_level_tables_refusals(rules):
    part, fglob, perm, (f0, f1), cglob, cperm, (c0, c1) = LEVEL_CASES["unpartitioned"]
    good, iperm = nested_pair(fglob, cglob), inverse(cperm)
    part1, fglob1, perm1, (g0, g1), cglob1, cperm1, (d0, d1) = LEVEL_CASES["rank0"]
    good1, iperm1 = nested_pair(fglob1, cglob1), inverse(cperm1)

    def changed(par, k, v):
        out = list(par)
        out[k] = v
        return out
    two_copies = changed(changed(good, 2, 0), 3, 0)          # fine vertex 1 claims to be the copy of coarse vertex 0 as well
    no_copy = changed(good, 4 * 2 + 1, 3)                    # fine vertex 4 (the copy of coarse 2) becomes a midpoint of (2, 3)
    owned_nonlocal = changed(good1, 2 * fglob1.index(3), -1)   # owned fine vertex 3 of rank 0 loses a parent
    asks = [
        (tables_line(0, f0, f1, c0, c1, perm, iperm, changed(good, 6, 5)), "parent vertex out of range"),
        (tables_line(0, f0, f1, c0, c1, perm, iperm, changed(good, 6, -1)), "parent vertex out of range"),   # -1 exists on partitions only
        (tables_line(1, g0, g1, d0, d1, perm1, iperm1, changed(good1, 1, -2)), "parent vertex out of range"),
        (tables_line(0, f0, f1, c0, c1, perm, iperm, two_copies), "two fine vertices claim to be the copy of one coarse vertex"),
        (tables_line(0, f0, f1, c0, c1, perm, iperm, no_copy), "a coarse vertex has no copy on the fine level (the meshes are not nested)"),
        (tables_line(1, g0, g1, d0, d1, perm1, iperm1, changed(changed(good1, 2 * fglob1.index(4), cglob1.index(2)), 2 * fglob1.index(4) + 1, cglob1.index(3))),
         "multilevel term: an owned coarse vertex must have its copy among the owned fine vertices (the meshes are not nested, or the plans do not match)"),
        (tables_line(1, g0, g1, d0, d1, perm1, iperm1, owned_nonlocal),
         "multilevel term: both parents of an owned fine vertex must be local on the coarse level"),
    ]
    for (_, want), line in zip(asks, rules([a for a, _ in asks])):
        assert line == "ERR " + want, line


# ---- record streams: what RecordStream (gmpnp_api.hip) asks before it reads, appends or allocates -------------------------------------
def records_want(first, n, count, capacity, t, h):
    """The Python restatement: Python's integers do not wrap, so first + n is the sum the rule forms in 64 bits."""
    finite = not (np.isnan(t) or np.isinf(t) or np.isnan(h) or np.isinf(h))
    return "%d %d %d %d" % (first >= 0 and n >= 1 and first + n <= count, count < capacity, finite and h > 0.0, capacity + 1)


def test_record_stream_rules(rules):
    big = 2 ** 31 - 1
    cases = [(first, n, count, 4, 1.0, 0.5) for count in (0, 3) for first in (-1, 0, 1, 2, 3) for n in (-1, 0, 1, 2, 3, 4)]
    cases += [(0, 3, 3, 4, 1.0, 0.5), (1, 2, 3, 4, 1.0, 0.5), (1, 3, 3, 4, 1.0, 0.5), (0, 4, 3, 4, 1.0, 0.5)]     # first + n == count, count + 1
    cases += [(big, big, 3, 4, 1.0, 0.5), (big, big, big, big, 1.0, 0.5), (big, 1, big, big, 1.0, 0.5)]        # a 32-bit sum would wrap to -2
    cases += [(0, 1, count, 4, 1.0, 0.5) for count in (0, 3, 4, 5)]                                            # capacity - 1, capacity, beyond
    cases += [(0, 1, 1, 4, t, h) for t, h in ((np.nan, 1.0), (np.inf, 1.0), (-np.inf, 1.0), (1.0, np.nan), (1.0, np.inf), (1.0, -np.inf),
                                               (1.0, 0.0), (1.0, -0.0), (1.0, -1.0), (0.0, 1e-300), (-3.0, 1.0))]
    got = rules(["records %d %d %d %d %r %r" % c for c in cases])
    for c, line in zip(cases, got):
        assert line == records_want(*c), (c, line)
    assert records_want(big, big, 3, 4, 1.0, 0.5).startswith("0 ") and records_want(0, 1, 3, 4, 1.0, 0.5) == "1 1 1 5"
    assert records_want(0, 1, 4, 4, 1.0, 0.5).split()[1] == "0" and records_want(0, 1, 1, 4, 1.0, 0.0).split()[2] == "0"


def test_header_reaches_no_hip_include():
    """Every file the header pulls in, by the preprocessor's own list: the C / C++ library and gmpnp.h, nothing of HIP or ROCm."""
    out = subprocess.run(["g++", "-std=c++17", "-M", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "gmpnp_amd", "csrc", "gmpnp_host_rules.h")],
                         check=True, capture_output=True, text=True).stdout
    deps = [d for d in out.replace("\\\n", " ").split()[1:]]
    assert any(d.endswith("gmpnp.h") for d in deps)
    assert not [d for d in deps if "hip" in d.lower() or "rocm" in d.lower()], deps


# ---- the policies of the linear solves inside Newton ------------------------------------------------------------------------
# Each model below restates the PARENT commit's inline rule (975009e: gmpnp_api.hip / gmpnp_group.h, line numbers of that commit);
# the structs are driven with the same histories and must show the same decision and the same state after every event.
def events(line):
    return [[int(x) for x in ev.split()] for ev in line.split(";") if ev.strip()]


def history(cmd, head, evs):
    return "%s %s %d %s" % (cmd, " ".join(map(str, head)), len(evs), " ".join(" ".join(map(repr, e)) for e in evs))


def model_coarse(async_, lag, evs):
    due, fresh_iters, out = False, 0, []          # api.hip:122-123
    for it, jumped, fell, iters in evs:
        must = bool(jumped) or due                                                  # api.hip:1044
        fresh = must if async_ else (lag <= 1 or it % lag == 0 or must)             # api.hip:1046 (async_ok: 1045)
        if fresh:                                                                   # api.hip:1066
            fresh_iters, due = iters, False
        elif iters > 2 * fresh_iters + 10:                                          # api.hip:1067
            due = True
        if fell:                                                                    # api.hip:1081
            due = True
        out.append([int(fresh), int(due), fresh_iters])
    return out


def model_gcoarse(evs):
    age, fresh, slow, out = 1 << 20, 0, False, []   # group.h:114
    for it, jumped, iters in evs:
        rebuild = it == 0 or age >= 2 or slow or bool(jumped)                       # group.h:706 (two_level: the caller's)
        if rebuild:                                                                 # group.h:765
            age, fresh, slow = 0, iters, False
        else:                                                                       # group.h:766
            age, slow = age + 1, iters > fresh + fresh // 4 + 5
        out.append([int(rebuild), age, fresh, int(slow)])
    return out


def model_direct(evs):
    sticky, backoff, out = 0, 0, []                 # api.hip:153-154
    for ev, arg in evs:
        if ev == 1 and arg == 0:                    # api.hip:1065 (rc == GMPNP_OK: the event itself; arg = st.iterations)
            backoff //= 2
        elif ev == 2:                               # api.hip:1082-1083
            backoff = min(256, max(8, 2 * backoff))
            sticky = backoff
        elif ev == 3 and sticky > 0 and not arg:    # api.hip:1124 (arg: o.linear_solver == GMPNP_LINEAR_BAND_LU)
            sticky -= 1
        out.append([int(sticky > 0), sticky, backoff])   # api.hip:1008
    return out


def model_burst(batch, B, evs):
    hint, table, last, out = 0, [0] * 32, [0, 0], []   # api.hip:113-115
    for ev, a, b, c in evs:
        val = -1
        if ev == 0:                                 # api.hip:1052
            hint = table[a] if a < 32 else 0
        elif ev == 1:                               # api.hip:587-590
            expect = hint // 2 if hint > 0 else last[a] // 2
            val = batch if batch > 0 else max(B, expect)
            if b:
                val = B
            val = ((val + B - 1) // B) * B
        elif ev == 2:                               # api.hip:652
            if not c:
                last[a] = b
        else:                                       # api.hip:1063-1064
            if a < 32:
                table[a] = b
            hint = 0
        out.append([val, hint] + last + table)
    return out


def model_gburst(evs):
    last, table, out = 0, [0] * 16, []              # group.h:102, 107
    for ev, a, b, c, d in evs:
        val = -1
        if ev == 0:                                 # group.h:739
            val = table[c] if (a == 0 and not b and c < 16) else 0
        elif ev == 1:                               # group.h:651
            val = a + 1 if a > 0 else (max(2, (7 * last) // 8) if b else 4)
        elif ev == 2:                               # group.h:742
            if a == 0 and b and c < 16:
                table[c] = d
        else:                                       # group.h:664
            last = a
        out.append([val, last] + table)
    return out


def model_x0(evs):
    held, out = False, []                           # api.hip:147
    for ev, a, scale in evs:
        ready = False
        if ev == 0:
            ready = held and a > 0 and scale != 0.0            # api.hip:1030
        else:                                       # api.hip:1014, 1093, 1097, 1101; group.h:774
            held = bool(a)
        out.append([int(ready), int(held)])
    return out


def check(rules, cmd, cases, model):
    """cases: (head, events); model(*head, events) -> the expected answer of every event."""
    for (head, evs), line in zip(cases, rules([history(cmd, head, evs) for head, evs in cases])):
        assert events(line) == model(*head, evs), (cmd, head, evs, line)


def test_coarse_reuse_single_handle(rules):
    f = 7
    edges = [
        # reused solves at exactly 2 f + 10 (kept) and 2 f + 11 (refresh due, taken at the next iteration, cleared by it)
        ((1, 3), [(0, 1, 0, f), (1, 0, 0, 2 * f + 10), (2, 0, 0, 2 * f + 11), (3, 0, 0, 5), (4, 0, 0, 2 * 5 + 10), (5, 0, 0, 2 * 5 + 11), (6, 0, 0, 9)]),
        ((0, 3), [(0, 0, 0, f), (1, 0, 0, 2 * f + 10), (2, 0, 0, 2 * f + 11), (3, 0, 0, 5), (4, 0, 0, 2 * 5 + 11), (5, 0, 0, 9), (6, 0, 0, 9), (7, 0, 0, 40)]),
        # lag 0 / 1: fresh every time; lag 2; a jumped state in the asynchronous scheme
        ((0, 0), [(k, 0, 0, 100 * k) for k in range(4)]), ((0, 1), [(k, 0, 0, 100 * k) for k in range(4)]),
        ((0, 2), [(k, 0, 0, 10) for k in range(5)]), ((1, 3), [(k, int(k < 3), 0, 10) for k in range(6)]),
        # a direct fallback asks for a refresh whatever the solve was
        ((1, 3), [(0, 1, 1, 3), (1, 0, 0, 3), (2, 0, 0, 3)]), ((0, 3), [(0, 0, 1, 3), (1, 0, 0, 3), (2, 0, 1, 300), (3, 0, 0, 3)]),
    ]
    rng = random.Random(20260101)
    hist = [((rng.randint(0, 1), rng.randint(0, 4)), [(it, int(rng.random() < 0.1), int(rng.random() < 0.1), rng.choice([rng.randint(0, 40), rng.randint(0, 600)]))
                                                      for it in range(rng.randint(1, 30))]) for _ in range(300)]
    check(rules, "coarse", edges + hist, model_coarse)
    a = events(rules([history("coarse", *edges[0])])[0])   # and by hand: the edge itself, not only the agreement
    assert [e[:2] for e in a[:4]] == [[1, 0], [0, 0], [0, 1], [1, 0]]


def test_coarse_reuse_group(rules):
    edges = [
        # f + f / 4 + 5 with f not divisible by 4 (f = 7: 13 is not slow, 14 is); age 0 -> 1 -> 2 -> rebuild
        ([], [(0, 0, 7), (1, 0, 13), (2, 0, 13), (3, 0, 7), (4, 0, 14), (5, 0, 9), (6, 0, 9 + 2 + 5), (7, 0, 9 + 2 + 6), (8, 0, 1)]),
        ([], [(0, 0, 6), (1, 0, 6 + 1 + 5), (2, 0, 6 + 1 + 6), (3, 0, 5)]), ([], [(0, 0, 5), (1, 0, 5 + 1 + 6), (2, 0, 0)]),
        # the initial age rebuilds whatever the iteration; iteration 0 rebuilds whatever the age; a jumped state rebuilds every time
        ([], [(3, 0, 10), (4, 0, 10), (5, 0, 10), (6, 0, 10)]), ([], [(0, 0, 10), (0, 0, 10), (1, 0, 10), (0, 0, 10)]), ([], [(k, 1, 10) for k in range(5)]),
    ]
    rng = random.Random(20260102)
    hist = [([], [(rng.randint(0, 3) if rng.random() < 0.3 else it, int(rng.random() < 0.1), rng.choice([rng.randint(0, 30), rng.randint(0, 400)]))
                  for it in range(rng.randint(1, 30))]) for _ in range(300)]
    check(rules, "gcoarse", edges + hist, model_gcoarse)
    a = events(rules([history("gcoarse", *edges[0])])[0])
    assert [e[0] for e in a[:6]] == [1, 0, 0, 1, 0, 1] and [e[1] for e in a[:3]] == [0, 1, 2] and a[4][3] == 1 and a[1][3] == 0


def test_direct_fallback(rules):
    climb = [(2, 0)] * 8
    edges = [
        ([], climb),                                                         # back-off 0 -> 8 -> 16 ... -> 256 and staying there
        ([], [(2, 0), (2, 0), (1, 1), (1, 5), (1, 0), (1, 0), (1, 0), (1, 0), (1, 0)]),   # halving on Newton iteration 0 only, down to 0
        ([], [(2, 0), (3, 1), (3, 1), (3, 0), (0, 0)] + [(3, 0)] * 9 + [(0, 0)]),         # no decrement when the caller asked for the band LU
        ([], [(0, 0), (3, 0), (3, 1), (1, 0)]),                                           # nothing to decrement, nothing to halve
    ]
    rng = random.Random(20260103)
    hist = [([], [(rng.choice([0, 1, 1, 2, 3, 3, 3]), rng.randint(0, 2)) for _ in range(rng.randint(1, 60))]) for _ in range(300)]
    check(rules, "direct", edges + hist, model_direct)
    assert [e[2] for e in events(rules([history("direct", [], climb)])[0])] == [8, 16, 32, 64, 128, 256, 256, 256]
    a = events(rules([history("direct", *edges[2])])[0])
    assert [e[1] for e in a[:5]] == [8, 8, 8, 7, 7] and a[-1] == [0, 0, 8]


def test_burst_hint_single_handle(rules):
    edges = [
        # table indices 31 / 32: 31 is kept and read back, 32 is neither
        ((0, 1), [(3, 31, 77, 0), (3, 32, 99, 0), (0, 31, 0, 0), (1, 1, 0, 0), (0, 32, 0, 0), (1, 1, 0, 0)]),
        # krylov_batch overrides the hint and the last count; a restart pass takes B all the same
        ((5, 2), [(3, 0, 80, 0), (0, 0, 0, 0), (1, 1, 0, 0), (1, 1, 1, 0)]), ((0, 2), [(3, 0, 80, 0), (0, 0, 0, 0), (1, 1, 0, 0), (1, 1, 1, 0)]),
        # no hint: half the last first-pass count of the same mode; a restart pass does not count as the last
        ((0, 1), [(2, 1, 50, 0), (2, 0, 20, 0), (2, 1, 999, 1), (1, 1, 0, 0), (1, 0, 0, 0), (3, 4, 9, 0), (0, 4, 0, 0), (1, 1, 0, 0), (3, 4, 1, 0), (1, 1, 0, 0)]),
    ]
    for B in (1, 2, 3):                              # rounding up to a multiple of B
        edges.append(((0, B), [(2, 1, n, 0) if k == 0 else (1, 1, 0, 0) for n in range(0, 16) for k in (0, 1)]))
        edges.append(((7, B), [(1, 0, 0, 0), (1, 0, 1, 0)]))
    rng = random.Random(20260104)

    def ev():
        k = rng.randint(0, 3)
        it, n = rng.choice([rng.randint(0, 40), 31, 32]), rng.choice([rng.randint(0, 30), rng.randint(0, 1500)])
        return {0: (0, it, 0, 0), 1: (1, rng.randint(0, 1), int(rng.random() < 0.2), 0), 2: (2, rng.randint(0, 1), n, int(rng.random() < 0.2)), 3: (3, it, n, 0)}[k]
    hist = [((rng.choice([0, 0, 0, rng.randint(1, 40)]), rng.randint(1, 8)), [ev() for _ in range(rng.randint(1, 40))]) for _ in range(300)]
    check(rules, "burst", edges + hist, model_burst)
    a = events(rules([history("burst", *edges[0])])[0])
    assert a[1][4 + 31] == 77 and 99 not in a[1] and a[2][1] == 77 and a[3][0] == 38 and a[4][1] == 0 and a[5][0] == 1
    assert [e[0] for e in events(rules([history("burst", *edges[1])])[0])[2:]] == [6, 2]


def test_burst_hint_group(rules):
    edges = [
        # table indices 15 / 16; read only on attempt 0 of a state that has not jumped; written only by attempt 0 of a solve that succeeded
        ([], [(2, 0, 1, 15, 60), (2, 0, 1, 16, 61), (0, 0, 0, 15, 0), (0, 0, 0, 16, 0), (0, 1, 0, 15, 0), (0, 0, 1, 15, 0), (2, 1, 1, 3, 9), (2, 0, 0, 3, 9), (0, 0, 0, 3, 0)]),
        # predicted + 1; else 7/8 of the previous solve, at least 2; else 4
        ([], [(1, 60, 1, 0, 0), (1, 60, 0, 0, 0), (1, 0, 1, 0, 0), (1, 0, 0, 0, 0), (3, 85, 0, 0, 0), (1, 0, 1, 0, 0), (1, 0, 0, 0, 0), (3, 3, 0, 0, 0), (1, 0, 1, 0, 0),
              (3, 9, 0, 0, 0), (1, 0, 1, 0, 0)]),
    ]
    rng = random.Random(20260105)

    def ev():
        k = rng.randint(0, 3)
        it, n = rng.choice([rng.randint(0, 20), 15, 16]), rng.choice([rng.randint(0, 30), rng.randint(0, 1500)])
        return {0: (0, rng.randint(0, 2), int(rng.random() < 0.2), it, 0), 1: (1, rng.choice([0, n]), rng.randint(0, 1), 0, 0),
                2: (2, rng.randint(0, 2), int(rng.random() < 0.8), it, n), 3: (3, n, 0, 0, 0)}[k]
    hist = [([], [ev() for _ in range(rng.randint(1, 40))]) for _ in range(300)]
    check(rules, "gburst", edges + hist, model_gburst)
    assert [e[0] for e in events(rules([history("gburst", *edges[0])])[0])] == [-1, -1, 60, 0, 0, 0, -1, -1, 0]
    assert [e[0] for e in events(rules([history("gburst", *edges[1])])[0]) if e[0] >= 0] == [61, 61, 2, 4, 74, 4, 2, 7]


def test_predicted_x0(rules):
    edges = [([], [(0, 1, 0.1), (1, 1, 0.0), (0, 0, 0.1), (0, 1, 0.0), (0, 1, 0.1), (0, 2, -0.001), (1, 0, 0.0), (0, 1, 0.1)])]
    rng = random.Random(20260106)
    hist = [([], [(rng.randint(0, 1), rng.randint(0, 2), rng.choice([0.0, 0.1, -0.001])) for _ in range(rng.randint(1, 30))]) for _ in range(200)]
    check(rules, "x0", edges + hist, model_x0)
    assert [e[0] for e in events(rules([history("x0", *edges[0])])[0])] == [0, 0, 0, 0, 1, 1, 0, 0]


OPTION_FIELDS = ["device_id", "n_aggregates", "shared_device", "krylov_batch", "profile_every", "launch_form", "warm_start", "coarse_refresh", "progress_by_copy",
                 "burst_iterations", "phase_timing", "no_direct_fallback", "warm_in_stream", "vector_form", "strict_steric", "element_stores"]
T_NEGATIVE, T_FORM, T_RANGE = "negative option", "launch_form must be 0, 2 or 4", "option out of range"
T_STORES = "element_stores: 0 (automatic), 1 (direct), 2 (staged, 3D meshes)"


def model_options(dim, o):
    """create_impl of the parent: every refusal it can reach, in its order, or the settings."""
    gb = o["band_lu_max_gb"]
    errs = []
    if o["krylov_batch"] < 0 or o["profile_every"] < 0:                                              # api.hip:1225
        errs.append(T_NEGATIVE)
    if o["launch_form"] not in (0, 2, 4):                                                            # api.hip:1264
        errs.append(T_FORM)
    if (o["coarse_refresh"] < 0 or o["burst_iterations"] < 0 or o["warm_start"] < -1 or o["warm_start"] > 1 or not (gb >= 0.0)   # api.hip:1265-1267
            or o["vector_form"] < 0 or o["vector_form"] > 2):
        errs.append(T_RANGE)
    if o["element_stores"] < 0 or o["element_stores"] > 2 or (o["element_stores"] == 2 and dim != 3):   # api.hip:1365-1366
        errs.append(T_STORES)
    settings = [int(o["coarse_refresh"] == 0 and not o["shared_device"]),                            # api.hip:1268
                o["coarse_refresh"] if o["coarse_refresh"] > 0 else 3,                               # api.hip:1269
                0 if (o["warm_in_stream"] or o["shared_device"]) else 1,                             # api.hip:1270
                {0: 2, 1: 1}.get(o["warm_start"], 0),                                                # api.hip:1271
                0 if o["progress_by_copy"] else 1, max(1, o["burst_iterations"]), int(o["phase_timing"] != 0),   # api.hip:1272-1274
                0 if o["no_direct_fallback"] else 1, 1 if o["strict_steric"] else 0,                 # api.hip:1275-1276
                gb if gb > 0.0 else 48.0]                                                            # api.hip:151, 1277
    return errs, settings


def test_resolve_options(rules):
    nan = float("nan")
    cases = [(3, {}), (1, {})]
    # every option at and just outside its range (one option off its default at a time: the parent's error text exactly)
    at_edges = {"krylov_batch": (-1, 0, 1), "profile_every": (-1, 0, 1), "launch_form": (-1, 0, 1, 2, 3, 4, 5), "warm_start": (-2, -1, 0, 1, 2),
                "coarse_refresh": (-1, 0, 1, 2), "burst_iterations": (-1, 0, 1, 2), "vector_form": (-1, 0, 1, 2, 3), "element_stores": (-1, 0, 1, 2, 3),
                "band_lu_max_gb": (-1e-300, -0.0, 0.0, 1e-300, 31.5, nan, float("inf")),
                "shared_device": (0, 1, -1), "progress_by_copy": (0, 1, -1), "phase_timing": (0, 1, 2), "no_direct_fallback": (0, 1, -3),
                "warm_in_stream": (0, 1, 5), "strict_steric": (0, 1, -1), "device_id": (-1, 9), "n_aggregates": (-1, 99)}
    for dim in (1, 3):
        cases += [(dim, {name: v}) for name, vals in at_edges.items() for v in vals]
    cases += [(3, {"coarse_refresh": 2, "shared_device": 1, "warm_in_stream": 1}), (3, {"coarse_refresh": 0, "shared_device": 1})]
    n_single = len(cases)
    rng = random.Random(20260107)
    for _ in range(300):
        cases.append((rng.choice([1, 3]), {name: rng.choice(vals) for name, vals in at_edges.items() if rng.random() < 0.25}))
    full = [(dim, {**{name: 0 for name in OPTION_FIELDS}, "band_lu_max_gb": 0.0, **ch}) for dim, ch in cases]
    lines = ["options %d %s %r" % (dim, " ".join(str(o[name]) for name in OPTION_FIELDS), o["band_lu_max_gb"]) for dim, o in full]
    seen = set()
    for k, ((dim, o), line) in enumerate(zip(full, rules(lines))):
        errs, settings = model_options(dim, o)
        if not errs:
            assert line.startswith("OK "), (dim, o, line)
            got = line.split()[1:]
            assert [int(x) for x in got[:9]] == settings[:9] and float(got[9]) == settings[9], (dim, o, line)
        else:   # with several invalid options at once the first one reported may differ from the parent's; the text may not
            assert line.startswith("ERR ") and line[4:] in errs, (dim, o, line, errs)
            if k < n_single:
                assert len(errs) == 1 and line[4:] == errs[0], (dim, o, line)
            seen.add(line[4:])
    assert seen == {T_NEGATIVE, T_FORM, T_RANGE, T_STORES}


def test_band_refinement_rule(rules):
    """band_refine_again, the one continue/stop rule of the block-banded LU's refinement (the host's band_refined_substitute and the
    frequency response's k_cband_judge), against its restatement: another round while the residual is finite, above the tolerance and
    (after a refinement) less than half the one before; three rounds at the most.  Rounds 0-3 with residuals that halve, that do not,
    that equal the tolerance, NaN and Inf, and the device's finiteness flag down on an ordinary number."""
    nan, inf = float("nan"), float("inf")

    def again(rnd, finite, rn, best, tol):
        if not finite or rnd >= 3 or not rn > tol:
            return False
        return rnd == 0 or rn < 0.5 * best

    tol = 1e-10
    cases = []
    for rnd in range(4):
        for best in (1e-3, 1e-8):
            for rn in (0.4999 * best, 0.5 * best, 0.5001 * best, best, 2.0 * best, tol, tol * (1 + 2.0 ** -52), 0.5 * tol, 0.0, nan, inf):
                cases.append((rnd, int(np.isfinite(rn)), rn, best, tol))
            cases.append((rnd, 0, 0.1 * best, best, tol))
    answers = rules(["refine %d %d %r %r %r" % c for c in cases])
    assert [int(a) for a in answers] == [int(again(*c)) for c in cases]
    assert not any(int(a) for c, a in zip(cases, answers) if not c[1])   # NaN, Inf, the flag down: never another round
    # by hand: the plain solve refines whatever came before; halving goes on, not halving stops; the fourth judgement stops; rn = tol stops
    hand = [((0, 1, 2e-3, 1e-3, tol), 1), ((1, 1, 0.4e-3, 1e-3, tol), 1), ((2, 1, 0.5e-3, 1e-3, tol), 0), ((2, 1, 0.6e-3, 1e-3, tol), 0),
            ((3, 1, 0.4e-3, 1e-3, tol), 0), ((0, 1, tol, 1e-3, tol), 0), ((0, 1, tol * (1 + 2.0 ** -52), 1e-3, tol), 1), ((0, 0, inf, 0.0, tol), 0),
            ((0, 0, nan, 0.0, tol), 0), ((1, 0, inf, 1e-3, tol), 0)]
    assert [int(a) for a in rules(["refine %d %d %r %r %r" % c for c, _ in hand])] == [w for _, w in hand]
