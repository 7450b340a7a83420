"""Host-side planning of 3D pore ensembles (gmpnp_amd.pore_ensemble.plan_members) and the sweep's grouping by mesh: no GPU."""
import pytest

from gmpnp_amd import backend, sweep
from gmpnp_amd.pore_ensemble import MEMBER_DEFAULTS, SHARED_DEFAULTS, plan_members


def test_plan_fills_defaults_and_keeps_member_fields():
    full, steps = plan_members([{"concentration_elec": 0.5, "L": 10e-9}, {"cation": "Cs", "L": 10e-9, "H2_FE": 0.2}], num_steps=7)
    assert steps == 7 and len(full) == 2
    for d in full:
        assert set(d) == (set(MEMBER_DEFAULTS) | set(SHARED_DEFAULTS)) - {"num_steps"}
        assert d["L"] == 10e-9 and d["R"] == SHARED_DEFAULTS["R"] and d["as_published"] is False and d["refine"] == 0
    assert full[0]["concentration_elec"] == 0.5 and full[0]["cation"] == "K" and full[0]["H2_FE"] == MEMBER_DEFAULTS["H2_FE"]
    assert full[1]["concentration_elec"] == MEMBER_DEFAULTS["concentration_elec"] and full[1]["cation"] == "Cs" and full[1]["H2_FE"] == 0.2
    assert plan_members([{}])[1] is None                       # the schedule's own number of steps
    assert plan_members([{"num_steps": 3}, {"num_steps": 3}])[1] == 3


def test_plan_refuses_bad_sizes():
    with pytest.raises(ValueError, match="1 ... 64"):
        plan_members([])
    with pytest.raises(ValueError, match="1 ... 64"):
        plan_members([{}] * (backend.MAX_ENSEMBLE + 1))
    assert len(plan_members([{}] * backend.MAX_ENSEMBLE)[0]) == backend.MAX_ENSEMBLE


@pytest.mark.parametrize("field,other", [("L", 50e-9), ("R", 2e-9), ("params_file", "parameters"), ("as_published", True),
                                         ("refine", 1), ("num_steps", 4)])
def test_plan_names_the_shared_field_that_differs(field, other):
    with pytest.raises(ValueError, match="differ in %s: member 0 has .* member 2 has" % field):
        plan_members([{"cation": "K"}, {"cation": "Cs"}, {field: other}])


def test_plan_names_the_first_differing_field_in_the_documented_order():
    with pytest.raises(ValueError, match="differ in L:"):
        plan_members([{}, {"R": 1e-9, "L": 10e-9}])


@pytest.mark.parametrize("field,value", [("multilevel", True), ("partition", (2, None))])
def test_plan_refuses_multilevel_and_partition(field, value):
    with pytest.raises(ValueError, match="member 1: %s is not supported" % field):
        plan_members([{}, {field: value}])
    full, _ = plan_members([{field: None}, {field: False}])   # switched off explicitly: accepted, and not passed on
    assert all(field not in d for d in full)


def test_plan_refuses_unknown_keywords():
    with pytest.raises(TypeError, match="member 0: unknown keyword"):
        plan_members([{"porosity_eff": 0.4}])


def test_sweep_groups_jobs_by_radius_in_order():
    for rank, world in ((0, 1), (1, 3), (2, 8)):
        mine = sweep.my_jobs(sweep.jobs(), rank, world)
        groups = sweep.group_by_radius(mine)
        seen = [k for _, idx in groups for k in idx]
        assert sorted(seen) == list(range(len(mine)))                       # every job exactly once
        assert len({r for r, _ in groups}) == len(groups)                   # one group per radius
        for r, idx in groups:
            assert idx == sorted(idx) and all(mine[k][0] == r for k in idx)  # job order kept inside a group
        firsts = [idx[0] for _, idx in groups]
        assert firsts == sorted(firsts)                                      # groups in order of first appearance
    assert sweep.group_by_radius([(5, -1.0), (1, -1.0), (5, -2.5)]) == [(5, [0, 2]), (1, [1])]
    assert sweep.group_by_radius([]) == []
