"""Potential programmes in the 3D pore on the CPU: the bins rule (g++ alone) against its Python statement
(gmpnp_amd/programme.py) with ``==``, the NumPy wall profile of tests/pore_programme_reference.py against the wall sums of the other
restatements, ``run_programme`` over the NumPy system with the profile recorded beside the trace, the ctypes image against the header,
the units of the output arrays on a hand-made record, the Python refusals and the command lines.  Cases: the generated cylinders (1, 2),
(2, 3), (3, 6) and the box pore ``box_pore_problem(2, 3)``, random admissible states, BDM Stern layer, two reactions."""
import math
import os
import subprocess

import numpy as np
import pytest

import kinetics_reference as K
import pore_programme_reference as PPR
import pore_response_reference as PP
import stern_bc_reference as SR
from conftest import box_pore_problem, random_state
from gmpnp_amd import programme as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(float).eps


# ---- the bins rule: C++ (g++ alone) against the Python statement ---------------------------------------------------------------------
DRIVER = r"""
#include <cstdio>
#include <vector>
#include "gmpnp_host_rules.h"
using namespace gmpnp;
int main() {
  int n, m;
  if (std::scanf("%d", &n) != 1) return 1;
  std::vector<double> e(n + 1);
  for (int k = 0; k <= n; ++k) if (std::scanf("%la", &e[k]) != 1) return 1;
  std::printf("%d\n", (int)wall_bins_valid(e.data(), n));
  if (std::scanf("%d", &m) != 1) return 1;
  for (int k = 0; k < m; ++k) { double z; if (std::scanf("%la", &z) != 1) return 1; std::printf("%d ", wall_bin(z, e.data(), n)); }
  std::printf("\n");
  double lo, hi; int q;
  while (std::scanf("%la %la %d", &lo, &hi, &q) == 3) {
    const std::vector<double> u = uniform_edges(lo, hi, q);
    for (double v : u) std::printf("%a ", v);
    std::printf("\n");
  }
  double Q[4] = {0.1, -0.2, 0.3, 0.0};
  const double I[4] = {1.0 / 3.0, 2.0 / 7.0, -5.0 / 9.0, 0.0};
  wall_profile_charge(Q, 0.1, I);
  std::printf("%a %a %a %a\n", Q[0], Q[1], Q[2], Q[3]);
  return 0;
}
"""


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    d = tmp_path_factory.mktemp("wall_profile_rule")
    src, exe = d / "rule.cpp", d / "rule"
    src.write_text(DRIVER)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "gmpnp_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True)

    def ask(edges, zs, uniform=()):
        text = "%d %s\n%d %s\n" % (len(edges) - 1, " ".join(float(e).hex() for e in edges), len(zs), " ".join(float(z).hex() for z in zs))
        text += "".join("%s %s %d\n" % (float(a).hex(), float(b).hex(), q) for a, b, q in uniform)
        return subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    return ask


def test_wall_bin_over_edges_neighbours_ends_and_outside(rule):
    for edges in ([0.0, 1.0], [0.0, 1.0 / 3.0, 2.0 / 3.0, 1.0], P.uniform_edges(-0.25, 1.5, 7), [0.1, 0.1 + 1e-16 * 4, 0.5, 3.0]):
        n = len(edges) - 1
        assert P.wall_bins_valid(edges, n)
        zs = []
        for e in edges:
            zs += [np.nextafter(e, -np.inf), e, np.nextafter(e, np.inf)]
        zs += [0.5 * (a + b) for a, b in zip(edges, edges[1:])] + [edges[0] - 1.0, edges[-1] + 1.0, -math.inf, math.inf, math.nan]
        out = rule(edges, zs)
        want = [P.wall_bin(float(z), edges, n) for z in zs]
        assert int(out[0]) == 1 and [int(x) for x in out[1].split()] == want
        # what the statement says: the largest b with edges[b] <= z; the last edge in the last bin; outside in no bin
        assert want[0] == -1 and want[1] == 0 and want[2] == 0
        assert want[3 * n] == n - 1 and want[3 * n + 1] == n - 1 and want[3 * n + 2] == -1
        for k in range(1, n):
            assert want[3 * k] == k - 1 and want[3 * k + 1] == k and want[3 * k + 2] == k       # an interior edge belongs to the bin above
        assert want[-5:] == [-1] * 5


def test_uniform_edges_and_validity(rule):
    cases = [(0.0, 1.0, 1), (0.0, 1.0, 3), (0.0, 1.0, 7), (-0.3, 2.9, 16), (0.1, 0.7, 10), (1e-9, 5e-9, 256)]
    out = rule([0.0, 1.0], [], cases)
    for k, (lo, hi, q) in enumerate(cases):
        got = [float.fromhex(x) for x in out[2 + k].split()]
        want = P.uniform_edges(lo, hi, q)
        assert got == want and want[0] == lo and want[-1] == hi and len(want) == q + 1       # ==: bit for bit
        assert P.wall_bins_valid(want, q)
    assert [float.fromhex(x) for x in out[2 + len(cases)].split()] == P.wall_profile_charge([0.1, -0.2, 0.3, 0.0], 0.1, [1.0 / 3.0, 2.0 / 7.0, -5.0 / 9.0, 0.0])
    bad = {"descending": [0.0, 0.5, 0.4, 1.0], "equal": [0.0, 0.5, 0.5, 1.0], "nan": [0.0, math.nan, 1.0], "inf": [0.0, 0.5, math.inf]}
    for name, edges in bad.items():
        assert not P.wall_bins_valid(edges, len(edges) - 1), name
        assert int(rule(edges, [])[0]) == 0, name
    assert not P.wall_bins_valid([0.0], 0) and not P.wall_bins_valid(P.uniform_edges(0.0, 1.0, 257), 257)
    assert int(rule(P.uniform_edges(0.0, 1.0, 257), [])[0]) == 0 and int(rule(P.uniform_edges(0.0, 1.0, 256), [])[0]) == 1
    assert not P.wall_bins_valid([0.0, 0.5, 1.0], 3)          # n + 1 edges


# ---- the NumPy profile against the wall sums of the other restatements -----------------------------------------------------------------
def problems():
    out = {"c%dx%d" % c: PP.cylinder_case(c) for c in ((1, 2), (2, 3), (3, 6))}
    out["box"] = PP.with_stern_and_kinetics(box_pore_problem(2, 3)[2])
    return out


@pytest.fixture(scope="module", params=["c1x2", "c2x3", "c3x6", "box"])
def case(request):
    prob = problems()[request.param]
    u, _ = random_state(prob.coords.shape[0], prob.nf - 1, seed=11)
    u.setflags(write=False)
    return request.param, prob, u


def test_bins_that_cover_the_wall_add_up_to_the_wall_sums(case):
    """The sum over bins that cover the wall, and one bin, equal stern_displacement, currents and the total weight within 64 eps x the
    sum of |terms|; every node is counted once, also on an interior edge (the layers of the cylinders ARE edges of the uniform bins)."""
    name, prob, u = case
    nodes, w, z = PPR.wall_nodes_z(prob)
    D, I, A = SR.stern_displacement(prob, u), K.currents(prob, u), w.sum()
    layers = np.unique(z)
    for nb in (1, 2, 3, len(layers) - 1):
        edges = P.uniform_edges(0.0, 1.0, nb)
        pr = PPR.profile(prob, u, edges)
        assert pr["count"].sum() == len(nodes) and (pr["count"] > 0).all()
        assert abs(pr["D"].sum() - D) <= 64 * EPS * pr["scale_D"].sum()
        assert (np.abs(pr["I"].sum(axis=0)[:2] - I) <= 64 * EPS * pr["scale_I"].sum(axis=0)[:2]).all() and not pr["I"][:, 2:].any()
        assert abs(pr["area"].sum() - A) <= 64 * EPS * A
        mean = (w[:, None] * np.asarray(u).reshape(-1, prob.nf)[nodes]).sum(axis=0) / A
        tot = (pr["area"][:, None] * np.c_[pr["u_mean"], pr["p_mean"]]).sum(axis=0) / A
        assert (np.abs(tot - mean) <= 64 * EPS * pr["scale_u"].sum(axis=0) / A).all()
    # a node on an interior edge is counted once, in the bin above; edges between the layers give the same sets from either side
    if len(layers) > 2:
        on_edge = PPR.profile(prob, u, [0.0, float(layers[1]), 1.0])
        assert on_edge["count"][0] == int((z < layers[1]).sum()) and on_edge["count"][1] == int((z >= layers[1]).sum())
    # bins that leave a part of the wall out: the nodes outside belong to no bin
    part = PPR.profile(prob, u, [float(layers[0]), float(np.nextafter(layers[-1], -np.inf))])
    assert part["count"][0] == int((z < layers[-1]).sum())


# ---- run_programme with the profile recorded beside the trace -------------------------------------------------------------------------
@pytest.fixture(scope="module", params=list(PPR.MARCH_CYLINDERS))
def marched(request):
    prob, u, dt = PPR.march_case(PPR.MARCH_CYLINDERS[request.param])
    edges = P.uniform_edges(0.0, 1.0, PPR.MARCH_BINS)
    out = {}
    for kind, segs in PPR.march_programmes(dt).items():
        s = PPR.NumpyPoreProgrammeSystem(prob, u, lambda h: 1.0 / h, edges)
        out[kind] = (segs, s, P.run_programme(s, segs, steps_per_segment=PPR.MARCH_STEPS_PER_SEGMENT))
    return out


@pytest.mark.parametrize("kind", ["pulse", "triangle"])
def test_march_lands_and_the_charges_close(marched, kind):
    segs, s, res = marched[kind]
    assert res["breakpoints"] == [g[1] for g in segs] and res["times"][-1] == segs[-1][1]      # ==
    assert sum(P.programme_jump(segs, k) for k in range(len(segs))) == (2 if kind == "pulse" else 0)
    a = s.arrays()
    n = len(a["t"])
    assert n == PPR.MARCH_STEPS_PER_SEGMENT * len(segs)
    # 5n's bound: Q_D is D_last - D_first within 4 ulp of max |D| per accepted step
    bound = 4 * n * EPS * max(np.abs(a["D"]).max(), abs(s.D_first))
    assert abs(a["Q_D"][-1] - (a["D"][-1] - s.D_first)) <= bound
    # the bins' charges are the sums of h x I_b by the charge statement, and the bins add up to the record of the whole wall
    Q = np.zeros((PPR.MARCH_BINS, 4))
    for pr in s.profiles:
        for b in range(PPR.MARCH_BINS):
            Q[b] = P.wall_profile_charge(Q[b], pr["h"], pr["I"][b])
        assert np.array_equal(pr["Q"], Q)
    for k, pr in enumerate(s.profiles):
        assert abs(pr["D"].sum() - a["D"][k]) <= 64 * EPS * pr["scale_D"].sum()
        assert (np.abs(pr["I"].sum(axis=0) - a["I"][k]) <= 64 * EPS * pr["scale_I"].sum(axis=0)).all()
    hI = sum(pr["h"] * pr["I"] for pr in s.profiles)
    assert (np.abs(s.profiles[-1]["Q"] - hI) <= 4 * n * EPS * np.abs(hI).max()).all()


# ---- the Python layer --------------------------------------------------------------------------------------------------------------------
def test_ctypes_image_has_the_layout_of_the_header(tmp_path):
    from gmpnp_amd import backend
    fields = ("t", "h", "z_lo", "z_hi", "area", "D", "I", "Q", "p_mean", "u_mean", "count", "status")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gmpnp.h"\nint main(void){printf("%zu", sizeof(gmpnp_wall_profile_record_t));\n'
                   + "".join('printf(" %%zu", offsetof(gmpnp_wall_profile_record_t,%s));\n' % f for f in fields)
                   + 'printf(" %d\\n", GMPNP_WALL_PROFILE_MAX_BINS);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    dt = backend.WALL_PROFILE_RECORD_DTYPE
    assert dt.names == fields and dt.itemsize == got[0] and [dt.fields[f][1] for f in fields] == got[1:-1]
    assert dt["I"].shape == dt["Q"].shape == (backend.MAX_SURFACE_REACTIONS,) and dt["u_mean"].shape == (backend.MAX_SPECIES,)
    assert got[-1] == backend.WALL_PROFILE_MAX_BINS == P.WALL_PROFILE_MAX_BINS
    for name in ("gmpnp_wall_profile_open", "gmpnp_wall_profile_append", "gmpnp_wall_profile_read", "gmpnp_wall_profile_close"):
        assert name in backend.EXPORTS and hasattr(backend.DeviceSolver, name[len("gmpnp_"):])


def test_units_of_the_output_arrays_on_a_hand_made_record():
    from types import SimpleNamespace
    from gmpnp_amd import backend
    pp = SimpleNamespace(thermal_voltage=0.025, time_constant=2e-6, L=1e-8)
    eps_0, area = 8.8e-12, 4.0
    segs = P.pulse([-1.0, -2.0], [2.0, 2.0], 1)
    rec = np.zeros(2, dtype=backend.ELECTRODE_RECORD_DTYPE)
    rec["t"], rec["h"], rec["p_M"], rec["p_boundary"] = [2.0, 4.0], 2.0, [-1.0, -2.0], [-0.5, -0.75]
    rec["D"], rec["dD_dt"], rec["Q_D"] = [-8.0, -12.0], [0.0, -2.0], [0.0, -4.0]
    rec["I"][:, 0], rec["I"][:, 1] = [6.0, 2.0], [2.0, 2.0]
    rec["Q"][:, 0], rec["Q"][:, 1] = [12.0, 16.0], [4.0, 8.0]
    rec["u_boundary"] = np.arange(16.0).reshape(2, 8)
    prof = np.zeros((2, 2), dtype=backend.WALL_PROFILE_RECORD_DTYPE)
    prof["z_lo"], prof["z_hi"], prof["area"] = [0.0, 0.5], [0.5, 1.0], [1.0, 3.0]
    prof["D"] = [[-2.0, -6.0], [-3.0, -9.0]]
    prof["I"][:, :, 0], prof["I"][:, :, 1] = [[3.0, 3.0], [1.0, 1.0]], [[1.0, 1.0], [0.5, 1.5]]
    prof["Q"][:, :, 0], prof["Q"][:, :, 1] = [[6.0, 6.0], [8.0, 8.0]], [[2.0, 2.0], [3.0, 5.0]]
    prof["p_mean"] = [[-0.4, -0.6], [-0.7, -0.8]]
    prof["u_mean"][:, :, 4], prof["u_mean"][:, :, 0] = [[0.9, 0.8], [0.7, 0.6]], [[1.0, 1.1], [1.2, 1.3]]
    prof["status"][1, 1] = 1
    out = P.pore_output_arrays(pp, eps_0, area, rec, prof, [0, 1], segs, 1)
    assert set(out) == set(P.PORE_OUTPUT_KEYS) and set(P.OUTPUT_KEYS) < set(P.PORE_OUTPUT_KEYS)
    q = eps_0 * 0.025 / 1e-8
    assert np.array_equal(out["time_s"], np.array([2.0, 4.0]) * 2e-6) and np.array_equal(out["electrode_voltage"], [-1.0, -2.0])
    assert np.array_equal(out["i_CO"], [1.5, 0.5]) and np.array_equal(out["i_H2"], [0.5, 0.5]) and np.array_equal(out["FE_H2"], [0.25, 0.5])
    assert np.allclose(out["surface_charge"], q * np.array([-2.0, -3.0]), rtol=1e-15) and np.allclose(out["i_charging"], [0.0, q * 0.5 / 2e-6], rtol=1e-15)
    assert np.allclose(out["charge_CO"], np.array([3.0, 4.0]) * 2e-6, rtol=1e-15) and np.allclose(out["charge_double_layer"], [0.0, q * 1.0], rtol=1e-15)
    assert np.array_equal(out["potential_OHP"], np.array([-0.5, -0.75]) * 0.025)
    assert np.array_equal(out["OHP_CO2"], [4.0, 12.0]) and np.array_equal(out["OHP_cat"], [7.0, 15.0]) and np.array_equal(out["OHP_H"], [0.0, 8.0])
    # the profile: every quantity per the bin's own area
    assert np.array_equal(out["z_lo_m"], [0.0, 0.5e-8]) and np.array_equal(out["z_hi_m"], [0.5e-8, 1e-8])
    assert np.allclose(out["bin_area_m2"], [1e-16, 3e-16], rtol=1e-15)
    assert np.array_equal(out["profile_i_CO"], [[3.0, 1.0], [1.0, 1.0 / 3.0]]) and np.array_equal(out["profile_i_H2"], [[1.0, 1.0 / 3.0], [0.5, 0.5]])
    assert np.allclose(out["profile_FE_H2"], [[0.25, 0.25], [1.0 / 3.0, 0.6]], rtol=1e-15)
    assert np.allclose(out["profile_surface_charge"], q * np.array([[-2.0, -2.0], [-3.0, -3.0]]), rtol=1e-15)
    assert np.array_equal(out["profile_potential_OHP"], np.array([[-0.4, -0.6], [-0.7, -0.8]]) * 0.025)
    assert np.array_equal(out["profile_CO2"], [[0.9, 0.8], [0.7, 0.6]]) and np.array_equal(out["profile_H"], [[1.0, 1.1], [1.2, 1.3]])
    assert np.allclose(out["profile_charge_CO"], np.array([[6.0, 2.0], [8.0, 8.0 / 3.0]]) * 2e-6, rtol=1e-15)
    assert np.allclose(out["profile_charge_H2"], np.array([[2.0, 2.0 / 3.0], [3.0, 5.0 / 3.0]]) * 2e-6, rtol=1e-15)
    assert out["profile_status"].tolist() == [[0, 0], [0, 1]]
    # sum_b profile_i_CO x bin area is i_CO x wall area
    assert np.allclose((out["profile_i_CO"] * prof["area"]).sum(axis=1), out["i_CO"] * area, rtol=1e-15)
    assert set(P.PORE_METADATA_KEYS) == {"pore_" + k for k in P.METADATA_KEYS} | {"pore_programme_bins"}


def test_resolve_bins():
    z = np.array([0.0, 0.0, 0.25, 0.5, 0.75, 1.0])
    assert P.resolve_bins(4, z, 1e-8) == P.uniform_edges(0.0, 1.0, 4)
    assert P.resolve_bins([0.0, 0.3e-8, 1e-8], z, 1e-8) == [0.0, 0.3e-8 / 1e-8, 1.0]
    with pytest.raises(ValueError, match="pore_programme: bin 1 of 8 holds no node"):
        P.resolve_bins(8, z, 1e-8)
    for bad in (0, 257, 2.5, "4", None, True, [0.0, 1e-8, 0.5e-8], [0.0], [[0.0, 1.0]]):
        with pytest.raises(ValueError, match="pore_programme: bins"):
            P.check_bins(bad)


PULSE = dict(kind="pulse", v_levels=[-1.0, -2.0], durations=[1e-9, 1e-9], cycles=2)


def test_python_refusals():
    from gmpnp_amd import edl1d, edl_ensemble, edl_sweep, pore3d, pore_ensemble, rxndiff1d, rxnpore3d, sweep
    E = dict(electrode_voltage=-1.0)
    calls = {
        "no electrode voltage": lambda: pore3d.PoreRun(pore_programme=PULSE),
        "target_current": lambda: pore3d.PoreRun(**E, kinetics="tafel", i0_CO=1.0, i0_H2=1.0, target_current=10.0, pore_programme=PULSE),
        "polarisation": lambda: pore3d.PoreRun(**E, polarisation=dict(v_end=-2.0, v_step=-0.5), pore_programme=PULSE),
        "dt_order 2": lambda: pore3d.PoreRun(**E, adaptive_dt=True, dt_order=2, pore_programme=PULSE),
        "partitions": lambda: pore3d.PoreRun(**E, partition=(2, None), pore_programme=PULSE),
        "multilevel": lambda: pore3d.PoreRun(**E, multilevel=True, refine=1, pore_programme=PULSE),
        "device glue": lambda: pore3d.PoreRun(**E, glue="device", pore_programme=PULSE),
        "bad waveform": lambda: pore3d.PoreRun(**E, pore_programme=dict(kind="pulse", v_levels=[-1.0], durations=[1e-9, 2e-9])),
        "bad kind": lambda: pore3d.PoreRun(**E, pore_programme=dict(kind="saw")),
        "unknown field": lambda: pore3d.PoreRun(**E, pore_programme=dict(PULSE, v_vertex=-3.0)),
        "sensitivities": lambda: pore3d.PoreRun(**E, pore_programme=dict(PULSE, sensitivities=["offset"])),
        "bad bins": lambda: pore3d.PoreRun(**E, pore_programme=dict(PULSE, bins=0)),
        "bad edges": lambda: pore3d.PoreRun(**E, pore_programme=dict(PULSE, bins=[0.0, 2e-9, 1e-9])),
        "EDLRun": lambda: edl1d.EDLRun(electrode_voltage=-5.0, pore_programme=PULSE),
        "rxn 1D": lambda: rxndiff1d.RxnDiffRun(pore_programme=PULSE),
        "rxn 3D": lambda: rxnpore3d.RxnPoreRun(pore_programme=PULSE),
        "EDLEnsemble": lambda: edl_ensemble.EDLEnsemble([dict(voltage_multiplier=-1.0), dict(voltage_multiplier=-1.0, pore_programme=PULSE)]),
        "PoreEnsemble": lambda: pore_ensemble.PoreEnsemble([dict(pore_programme=PULSE)]),
        "edl sweep": lambda: edl_sweep.run_sweep([dict(pore_programme=PULSE)]),
        "edl sweep keywords": lambda: edl_sweep.run_sweep([dict(voltage_multiplier=-1.0)], pore_programme=PULSE),
        "pore sweep job": lambda: sweep.run_job(5, -1.0, 1, pore_programme=PULSE),
        "pore sweep group": lambda: sweep.run_group(5, [-1.0], 1, pore_programme=PULSE),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError, match="pore_programme"):
            call()
    with pytest.raises(ValueError, match="use programme"):                     # the 1D driver points to its own keyword
        edl1d.EDLRun(electrode_voltage=-5.0, pore_programme=PULSE)
    with pytest.raises(ValueError, match="programme"):                          # the 1D keyword stays refused in the pore driver
        pore3d.PoreRun(**E, programme=dict(kind="pulse", v_levels=[-1.0, -2.0], durations=[1e-9, 1e-9]))
    P.refuse_pore_programme({}, "a test")
    P.refuse_pore_programme({"pore_programme": None}, "a test")


def test_command_lines(tmp_path):
    from gmpnp_amd import edl1d, pore3d, rxnpore3d
    p = pore3d.build_parser()
    assert P.pore_programme_keywords(p.parse_args([])) == {}
    a = p.parse_args(["--pore_programme", "pulse", "--v_levels", "-1", "-2", "--durations", "1e-9", "2e-9", "--cycles", "3", "--rise_time", "1e-10",
                      "--pore_programme_bins", "8", "--pore_programme_dt_init", "0.5", "--pore_programme_steps_per_segment", "4"])
    assert P.pore_programme_keywords(a) == {"pore_programme": dict(kind="pulse", v_levels=[-1.0, -2.0], durations=[1e-9, 2e-9], cycles=3,
                                                                   rise_time=1e-10, bins=8, dt_init=0.5, steps_per_segment=4)}
    a = p.parse_args(["--pore_programme", "triangle", "--v_vertex", "-2", "--scan_rate", "1e6"])
    assert P.pore_programme_keywords(a) == {"pore_programme": dict(kind="triangle", v_vertex=-2.0, scan_rate=1e6, cycles=1)}
    csv = tmp_path / "table.csv"
    csv.write_text("time_s,electrode_voltage\n0,-1\n1e-9,-1\n1e-9,-2\n3e-9,-2\n")
    a = p.parse_args(["--pore_programme", "table", "--pore_programme_file", str(csv)])
    assert P.pore_programme_keywords(a) == {"pore_programme": dict(kind="table", time_s=[0.0, 1e-9, 1e-9, 3e-9], electrode_voltage=[-1.0, -1.0, -2.0, -2.0])}
    for argv in (["--pore_programme", "pulse"], ["--pore_programme", "triangle", "--v_vertex", "-2"], ["--pore_programme", "table"]):
        with pytest.raises(ValueError, match="pore_programme"):
            P.pore_programme_keywords(p.parse_args(argv))
    with pytest.raises(SystemExit):
        p.parse_args(["--pore_programme", "saw"])
    with pytest.raises(SystemExit):                                               # --programme stays refused by the pore parser
        p.parse_args(["--programme", "pulse"])
    assert not any(s.startswith("--programme") for act in p._actions for s in act.option_strings)
    with pytest.raises(ValueError, match="pore_programme"):                       # no --electrode_voltage: before anything touches the device
        pore3d.main(["--pore_programme", "triangle", "--v_vertex", "-2", "--scan_rate", "1e6"])
    for other in (edl1d.build_parser(), rxnpore3d.build_parser()):                 # the other parsers do not learn the new flags
        assert not any(s.startswith("--pore_programme") for act in other._actions for s in act.option_strings)
        with pytest.raises(SystemExit):
            other.parse_args(["--pore_programme", "pulse"])
