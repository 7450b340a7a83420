"""The host rule of Newton's launch chain between two BiCGStab solves (gmpnp_host_rules.h, last_test_expected): whether the gather
of the next Jacobian is started beside a convergence test.  Compiled with the host compiler alone and checked against a Python
restatement on a table of residual histories, the edge values included, and against NewtonJudge on geometric histories: where the
residual really contracts by a constant factor the rule names exactly the test that ends the solve."""
import math
import os
import subprocess

import pytest

from conftest import ROOT

DRIVER = r"""
#include <cstdio>
#include <iostream>
#include <sstream>
#include "gmpnp_host_rules.h"
using namespace gmpnp;
int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd, tok; in >> cmd;
    auto num = [&]() { in >> tok; return std::stod(tok); };   // (reads "nan" and "inf" too)
    if (cmd == "last") {
      const double rp = num(), rn = num(), r0 = num(), rtol = num(), atol = num();
      const int it = (int)num(), maxit = (int)num();
      printf("%d\n", last_test_expected(rp, rn, r0, rtol, atol, it, maxit) ? 1 : 0);
    } else if (cmd == "history") {   // rtol atol maxit n r_0 ... r_{n-1}: per test k >= 2 "<expected last><verdict is not go_on>"
      gmpnp_newton_options_t o{}; gmpnp_newton_stats_t st{};
      o.relative_tolerance = num(); o.absolute_tolerance = num(); o.maximum_iterations = (int)num();
      const int n = (int)num();
      NewtonJudge j(o, st, false);
      NewtonJudge::Verdict v = NewtonJudge::go_on;
      for (int k = 0; k < n && v == NewtonJudge::go_on; ++k) {
        const double r = num();
        if (k == 0) { v = j.first(r, 0); continue; }
        st.iterations++;
        int guess = -1;
        if (st.n_residuals >= 2)
          guess = last_test_expected(st.residuals[st.n_residuals - 2], st.residuals[st.n_residuals - 1], j.r0, o.relative_tolerance,
                                     o.absolute_tolerance, st.iterations, o.maximum_iterations) ? 1 : 0;
        v = j.next(r, 0);
        if (guess >= 0) printf("%d%d ", guess, v == NewtonJudge::go_on ? 0 : 1);
      }
      printf(";\n");
    } else printf("?\n");
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    d = tmp_path_factory.mktemp("newton_chain_rules")
    src, exe = d / "rules.cpp", d / "rules"
    src.write_text(DRIVER)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "gmpnp_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True)

    def ask(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
        assert len(out) == len(lines), (len(out), len(lines))
        return out
    return ask


def restated(rp, rn, r0, rtol, atol, it, maxit):
    if it >= maxit:
        return True
    if not rp > 0.0 or not rn >= 0.0 or not rn < rp:
        return False
    nxt = rn * (rn / rp)
    rel = nxt / r0 if r0 != 0.0 else (math.nan if nxt == 0.0 or math.isnan(nxt) else math.inf)
    return rel < rtol or nxt < atol


NAN, INF = math.nan, math.inf
TABLE = [
    # r_prev, r_now, r0, rtol, atol, iterations, maximum_iterations
    (1.0, 0.1, 1.0, 1e-4, 1e-4, 1, 50),          # next 1e-2: goes on
    (1e-2, 1e-3, 1.0, 1e-4, 1e-4, 3, 50),        # next 1e-4: not below 1e-4
    (1e-2, 9.9e-4, 1.0, 1e-4, 1e-4, 3, 50),      # just below
    (1e-3, 1e-4, 1.0, 1e-4, 1e-4, 4, 50),        # next 1e-5: ends
    (1e3, 1e2, 1e6, 1e-4, 0.0, 2, 50),           # relative test alone: 10 / 1e6 = 1e-5
    (1e3, 1e2, 1e4, 1e-4, 0.0, 2, 50),           # 10 / 1e4 = 1e-3: goes on
    (5.0, 1.0, 1e9, 0.0, 0.25, 2, 50),           # absolute test alone: 0.2 < 0.25
    (5.0, 1.0, 1e9, 0.0, 0.2, 2, 50),            # 0.2 < 0.2 is false
    (1.0, 1.0, 1.0, 1e-4, 1e-4, 2, 50),          # no contraction: no prediction
    (1.0, 2.0, 1.0, 1e-4, 1e-4, 2, 50),          # growth
    (0.0, 0.0, 1.0, 1e-4, 1e-4, 2, 50),          # r_prev = 0
    (1.0, 0.0, 1.0, 1e-4, 1e-4, 2, 50),          # r_now = 0: next 0 passes both tests
    (NAN, 0.1, 1.0, 1e-4, 1e-4, 2, 50),
    (1.0, NAN, 1.0, 1e-4, 1e-4, 2, 50),
    (INF, 1.0, 1.0, 1e-4, 1e-4, 2, 50),          # next 0
    (1.0, 0.1, 0.0, 1e-4, 0.0, 2, 50),           # r0 = 0: rel = inf
    (1.0, 0.1, NAN, 1e-4, 0.0, 2, 50),
    (1.0, 0.5, 1.0, 1e-4, 1e-4, 50, 50),         # at the limit whatever the residual
    (NAN, NAN, NAN, 1e-4, 1e-4, 7, 7),
    (1.0, 0.5, 1.0, 1e-4, 1e-4, 49, 50),
]


def test_rule_matches_its_restatement(rules):
    out = rules(["last %r %r %r %r %r %d %d" % row for row in TABLE])
    for row, line in zip(TABLE, out):
        assert int(line) == int(restated(*row)), (row, line)
    assert [int(x) for x in out[:4]] == [0, 0, 1, 1]
    assert [int(x) for x in out[8:11]] == [0, 0, 0] and int(out[12]) == 0 and int(out[13]) == 0 and int(out[17]) == 1


@pytest.mark.parametrize("q", [0.1, 0.5, 0.03])
@pytest.mark.parametrize("tols", [(1e-4, 1e-4), (1e-9, 1e-10), (1e-6, 0.0)])
def test_on_a_geometric_history_the_rule_names_the_last_test(rules, q, tols):
    """r_k = r_0 q^k with a pinch of noise well inside the distance to the thresholds: from the third residual on the guess equals
    'the verdict of this test is not go_on', so no gather is started for nothing and none is missed."""
    rtol, atol = tols
    r0 = 37.0
    hist = [r0 * q ** k * (1.0 + 1e-3 * ((-1) ** k)) for k in range(60)]
    (line,) = rules(["history %r %r 50 %d %s" % (rtol, atol, len(hist), " ".join(repr(r) for r in hist))])
    pairs = line.split()[:-1]
    assert len(pairs) >= 2 and pairs[-1][1] == "1"
    # thresholds a noisy prediction straddles are excluded by construction: q^k passes a decade boundary only for q = 0.1, where
    # the factor 1 +- 1e-3 decides; there the guess may be off by one test either way, never more
    wrong = [p for p in pairs if p[0] != p[1]]
    assert len(wrong) <= (1 if q == 0.1 else 0), pairs
