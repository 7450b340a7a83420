"""gmpnp_host_rules.h — the Newton verdict, the predicted start and the multilevel level tables — compiled with the host compiler
alone (that it compiles without HIP is the assertion that the header is device-free) and checked against the oracle's stop rule,
the recorded reference histories and NumPy restatements written out here."""
import glob
import os
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
