"""Pins of the partition planner (gmpnp_amd/dist.py ``partition_hierarchy``): the planner is pure NumPy, so a change that is meant
to leave it alone leaves every table it makes bit-identical.  tests/golden/partition_plans.json holds one SHA-256 per
(case, partitions, rank, level) over dtype, shape and bytes of everything a plan carries; the cases are L_10_R_5 at refine 0, 1, 2
(``problem.pore_hierarchy``) and ``box_pore_problem(nx=4, nz=16)``, on 1, 2, 3, 4 and 8 partitions (refine 2, whose plans take the
longest to make: 2 and 4), every rank and every level of each.

The fixture is written by ``python tests/test_partition_plan_pins.py`` FROM A COMMIT WHOSE PLANNER IS TRUSTED, never from the code
under test; the file names the commit that produced it."""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, _pore, box_pore_problem

PINS = os.path.join(GOLDEN, "partition_plans.json")
CASES = {"L_10_R_5_refine0": (1, 2, 3, 4, 8), "L_10_R_5_refine1": (1, 2, 3, 4, 8), "L_10_R_5_refine2": (2, 4), "box_nx4_nz16": (1, 2, 3, 4, 8)}


def _levels(case):
    if case == "box_nx4_nz16":
        return [(box_pore_problem(nx=4, nz=16)[2], None, None)]
    from gmpnp_amd.problem import pore_hierarchy
    pp, mesh, _, _ = _pore(10e-9, 5e-9)
    return pore_hierarchy(pp, mesh, int(case[-1]))


def _feed(h, name, a):
    h.update(name.encode())
    if a is None:
        h.update(b"<none>")
        return
    a = np.ascontiguousarray(a)
    h.update(("%s%s" % (a.dtype.str, a.shape)).encode())
    h.update(a.tobytes())


def plan_digest(plan):
    """SHA-256 of one ``LevelPlan``: every array the library or the next level gets from it."""
    h = hashlib.sha256()
    dom = plan.domain
    _feed(h, "perm", plan.perm)
    for key in sorted(plan.part):
        _feed(h, "part." + key, np.asarray(plan.part[key]))
    _feed(h, "owned", dom.owned)
    _feed(h, "ghosts", dom.ghosts)
    for name in ("coords", "cells", "wall_facets", "exit_facets", "point_vertices", "bc_dofs", "bc_vals"):
        _feed(h, "problem." + name, getattr(dom.problem, name))
    for name in ("parents", "owner", "pos", "aggregate"):
        _feed(h, name, getattr(plan, name))
    for name in ("send", "recv"):
        table = getattr(dom, name)
        for q in sorted(table):
            _feed(h, "%s[%d]" % (name, q), table[q])
    return h.hexdigest()


def case_digests(case):
    """{"P<partitions>/rank<r>/level<k>": digest} of every partition count that has a default coarse-slab count."""
    from gmpnp_amd import dist
    levels = _levels(case)
    out = {}
    for nparts in CASES[case]:
        try:
            dist.default_global_aggregates(nparts)
        except ValueError:
            continue
        for r in range(nparts):
            for k, plan in enumerate(dist.partition_hierarchy(levels, nparts, r)):
                out["P%d/rank%d/level%d" % (nparts, r, k)] = plan_digest(plan)
    return out


@pytest.mark.parametrize("case", CASES)
def test_partition_plans_are_the_pinned_ones(case):
    with open(PINS) as fh:
        want = json.load(fh)["plans"][case]
    got = case_digests(case)
    assert sorted(got) == sorted(want)
    nlevels = 1 + max(int(key.rsplit("level", 1)[1]) for key in want)
    assert len(want) == nlevels * sum(CASES[case])                           # every rank and level of every partition count
    differ = [key for key in sorted(want) if got[key] != want[key]]
    assert not differ, "plans that changed: %s" % differ


if __name__ == "__main__":
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    commit = subprocess.run(["git", "-C", root, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    dirty = subprocess.run(["git", "-C", root, "status", "--porcelain", "gmpnp_amd"], capture_output=True, text=True).stdout.strip()
    if dirty:
        raise SystemExit("gmpnp_amd/ differs from %s: the pins come from a commit, not from a working tree" % commit)
    with open(PINS, "w") as fh:
        json.dump({"produced_by_commit": commit, "plans": {case: case_digests(case) for case in CASES}}, fh, indent=0, sort_keys=True)
        fh.write("\n")
