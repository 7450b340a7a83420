"""value_pair_offset (gmpnp_host_rules.h): where vals_s keeps entry (j, lane) of a block position — the one index rule of the
writer (scale_columns_body) and of every reader (TileRows, coarse_rows_body).  Compiled with g++ alone, as tests/test_host_rules.py
compiles its driver, and checked for NF = 1 .. 9: a bijection onto [0, NF * 64), pairs adjacent with the even member first and on
an even offset (16-byte aligned behind an even slice offset), the last column of an odd NF in the final 64 entries."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

LANES = 64
DRIVER = r"""
#include <cstdio>
#include "gmpnp_host_rules.h"
using namespace gmpnp;
static_assert(kValueLanes == 64, "one wave per slice");
static_assert(value_pair_offset(9, 0, 0) == 0 && value_pair_offset(9, 1, 0) == 1 && value_pair_offset(9, 8, 63) == 9 * 64 - 1, "usable in constant expressions");
int main() {
  for (int nf = 1; nf <= 9; ++nf)
    for (int j = 0; j < nf; ++j)
      for (int lane = 0; lane < kValueLanes; ++lane) printf("%d %d %d %d %d\n", nf, j, lane, value_pair_offset(nf, j, lane), value_plain_offset(nf, j, lane));
  return 0;
}
"""


@pytest.fixture(scope="module")
def offsets(tmp_path_factory):
    """{nf: (pair[j, lane], plain[j, lane])} as the compiled header gives them."""
    d = tmp_path_factory.mktemp("value_pairs")
    src, exe = d / "pairs.cpp", d / "pairs"
    src.write_text(DRIVER)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "gmpnp_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True)
    rows = np.array([[int(v) for v in line.split()] for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()])
    out = {}
    for nf in range(1, 10):
        r = rows[rows[:, 0] == nf]
        assert len(r) == nf * LANES
        pair, plain = np.full((nf, LANES), -1), np.full((nf, LANES), -1)
        pair[r[:, 1], r[:, 2]] = r[:, 3]
        plain[r[:, 1], r[:, 2]] = r[:, 4]
        out[nf] = (pair, plain)
    return out


@pytest.mark.parametrize("nf", range(1, 10))
def test_bijection_onto_the_position(nf, offsets):
    pair, plain = offsets[nf]
    assert np.array_equal(np.sort(pair.ravel()), np.arange(nf * LANES))
    assert np.array_equal(plain, np.arange(nf)[:, None] * LANES + np.arange(LANES)[None, :])   # the layout of vals: [j][lane]


@pytest.mark.parametrize("nf", range(1, 10))
def test_pairs_are_adjacent_even_member_first_on_an_even_offset(nf, offsets):
    pair, _ = offsets[nf]
    for m in range(nf // 2):
        assert np.array_equal(pair[2 * m + 1], pair[2 * m] + 1), (nf, m)
        assert not (pair[2 * m] & 1).any(), (nf, m)
        # [j / 2][lane][j & 1]: pair m of lane l starts at (m * 64 + l) * 2
        assert np.array_equal(pair[2 * m], (m * LANES + np.arange(LANES)) * 2), (nf, m)


@pytest.mark.parametrize("nf", [1, 3, 5, 7, 9])
def test_last_column_of_an_odd_nf_fills_the_final_entries(nf, offsets):
    pair, _ = offsets[nf]
    assert np.array_equal(pair[nf - 1], (nf - 1) * LANES + np.arange(LANES))
