"""The partitioned 3D driver (pore3d --partitions, PoreRun(glue="device")) and the library's column select it rests on
(gmpnp_column_select / gmpnp_group_column_select, csrc/gmpnp_stats.h): exact order statistics of the state on every partition
count, the device glue's histories bit for bit those of the host glue, and the CLI's files those of the serial CLI."""
import glob
import json
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

MEDIAN_COLS = (1, 2, 3, 7)
PORE10 = dict(concentration_elec=0.5, L=10e-9, R=5e-9)
CLI = ["--L=10e-9", "--R=5e-9", "--concentration_elec=0.5", "--num_steps=3"]


def bits(a):
    """bit patterns, -0.0 taken as +0.0 (what the select returns for a zero)"""
    return (np.asarray(a, dtype=np.float64) + 0.0).view(np.uint64)


@pytest.fixture(scope="module")
def pore10_after_two_steps(gpu_lib):
    from gmpnp_amd.pore3d import PoreRun
    run = PoreRun(num_steps=2, **PORE10)
    try:
        run.run(verbose=False)
        return run.problem, run.sys.vertex_values().copy()
    finally:
        run.sys.close()


def make_system(problem, nparts):
    from gmpnp_amd.solver import GMPNPSystem, PartitionedSystem
    return GMPNPSystem(problem) if nparts == 0 else PartitionedSystem(problem, nparts)


def set_u(sys_, vals):
    sys_.set_state(np.ascontiguousarray(vals, dtype=np.float64).ravel(), None)


def adversarial(nv, rng):
    """columns with ties, both zeros, subnormals, infinities, a constant, huge and tiny magnitudes"""
    a = np.empty((nv, 9))
    a[:, 0] = rng.standard_normal(nv)
    a[:, 1] = rng.choice([0.0, -0.0, 1.0, -1.0], size=nv)
    a[:, 2] = rng.choice([5e-324, -5e-324, 1e-310, -2.2e-308, 0.0, -0.0], size=nv)
    a[:, 3] = np.where(rng.random(nv) < 0.2, rng.choice([np.inf, -np.inf], size=nv), rng.standard_normal(nv))
    a[:, 4] = 0.8125
    a[:, 5] = rng.integers(-3, 4, size=nv).astype(np.float64)
    a[:, 6] = rng.standard_normal(nv) * 10.0 ** rng.integers(-300, 300, size=nv)
    a[:, 7] = 1.0 + 1e-12 * rng.standard_normal(nv)
    a[:, 8] = -np.abs(rng.standard_normal(nv))
    return a


@pytest.mark.parametrize("nparts", [0, 1, 2, 4, 8])
def test_column_select_is_exact(pore10_after_two_steps, nparts):
    """L_10_R_5 after two steps on an unpartitioned handle (0) and on 1 / 2 / 4 / 8 in-process partitions: the medians bit for bit
    those of column_medians of the gathered state, the CO2 minimum np.min's, and any rank of any column np.sort's; the same on
    adversarial states; the NaN flag; a rank past the end refused."""
    from gmpnp_amd.backend import GmpnpError
    from gmpnp_amd.solver import column_medians, device_column_medians, device_medians_and_minima
    problem, vals = pore10_after_two_steps
    nv = vals.shape[0]
    ks = [0, 1, nv // 3, nv // 2 - 1, nv // 2, nv - 2, nv - 1]
    fields = [f for f in range(9) for _ in ks]
    ranks = ks * 9
    sys_ = make_system(problem, nparts)
    try:
        set_u(sys_, vals)
        assert np.array_equal(bits(device_column_medians(sys_, MEDIAN_COLS)), bits(column_medians(vals, MEDIAN_COLS)))
        meds, mins = device_medians_and_minima(sys_, MEDIAN_COLS, (4,))
        assert np.array_equal(bits(meds), bits(column_medians(vals, MEDIAN_COLS)))
        assert bits(mins[0]) == bits(np.min(vals[:, 4]))
        out, nan = sys_.column_select(fields, ranks)
        assert not nan
        assert np.array_equal(bits(out), bits(np.sort(vals, axis=0)[ranks, fields]))

        adv = adversarial(nv, np.random.default_rng(nparts))
        set_u(sys_, adv)
        out, nan = sys_.column_select(fields, ranks)
        assert not nan
        assert np.array_equal(bits(out), bits(np.sort(adv, axis=0)[ranks, fields]))
        assert np.array_equal(bits(device_column_medians(sys_, range(9))), bits(column_medians(adv, range(9))))

        adv[nv // 5, 5] = np.nan
        set_u(sys_, adv)
        assert sys_.column_select([5], [0])[1]
        assert not sys_.column_select([6, 0], [0, nv - 1])[1]
        assert np.array_equal(device_column_medians(sys_, (5, 6)), column_medians(adv, (5, 6)), equal_nan=True)
        with pytest.raises(GmpnpError):
            sys_.column_select([0], [nv])
    finally:
        sys_.close()


def test_device_glue_equals_host_glue(gpu_lib):
    """PoreRun(partition=(2, None)): glue="device" and glue="host" give the same histories, CO2 Dirichlet values, minima and Newton
    counts over three steps, bit for bit."""
    from gmpnp_amd.pore3d import PoreRun
    got = {}
    for glue in ("host", "device"):
        run = PoreRun(num_steps=3, partition=(2, None), glue=glue, **PORE10)
        try:
            co2, mins = [], []
            for _ in range(3):
                run.step(verbose=False)
                co2.append(run.co2_bc)
                mins.append(run.CO2_min)
            hist = np.stack([run.field_history(i) for i in range(9)], axis=2)
            got[glue] = (hist, co2, mins, list(run.newton_its))
        finally:
            run.sys.close()
    (h0, c0, m0, n0), (h1, c1, m1, n1) = got["host"], got["device"]
    assert h0.shape == h1.shape == (4, h0.shape[1], 9)
    assert np.array_equal(h0.view(np.uint64), h1.view(np.uint64))
    assert np.array_equal(bits(c0), bits(c1))
    assert m0 == m1 and n0 == n1


def run_cli(argv, out, monkeypatch):
    """pore3d.main(argv) with outputs under `out`; returns (output directory, Newton iterations per step)."""
    from gmpnp_amd import pore3d
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setenv("GMPNP_OUT", str(out))
    its = []
    step = pore3d.PoreRun.step

    def counting_step(self, verbose=True):
        st = step(self, verbose)
        its.append(st["iterations"])
        return st

    monkeypatch.setattr(pore3d.PoreRun, "step", counting_step)
    try:
        path = pore3d.main(argv)
    finally:
        monkeypatch.setattr(pore3d.PoreRun, "step", step)
    return path, its


def vtu_values(path):
    text = open(path).read()
    data = re.findall(r'<DataArray type="Float64" Name="[^"]+" format="ascii">([^<]*)</DataArray>', text)[-1]
    return np.array(data.split(), dtype=np.float64)


def compare_outputs(a, b, rtol):
    """same file set, npz keys, shapes and metadata keys; npz arrays and .vtu values within `rtol` (norm-wise relative)"""
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    assert fa == fb

    def close(x, y, what):
        assert x.shape == y.shape, what
        ny = np.linalg.norm(y)
        assert np.linalg.norm(x - y) <= rtol * ny if ny > 0 else np.array_equal(x, y), what

    for f in fa:
        pa, pb = os.path.join(a, f), os.path.join(b, f)
        if f.endswith(".npz"):
            za, zb = np.load(pa), np.load(pb)
            assert sorted(za.files) == sorted(zb.files), f
            for k in za.files:
                close(za[k], zb[k], "%s:%s" % (f, k))
        elif f.endswith(".vtu"):
            close(vtu_values(pa), vtu_values(pb), f)
        elif f == "metadata.json":
            ma, mb = json.load(open(pa)), json.load(open(pb))
            assert sorted(ma) == sorted(mb)
            assert ma["newton_iterations"] == mb["newton_iterations"] and ma["num_steps_run"] == mb["num_steps_run"]
            assert abs(ma["CO2_min"] - mb["CO2_min"]) <= rtol * abs(mb["CO2_min"])


@pytest.mark.parametrize("extra", [[], ["--refine", "1", "--multilevel"]], ids=["refine0", "refine1_multilevel"])
def test_cli_partitions_writes_the_serial_files(gpu_lib, tmp_path, monkeypatch, extra):
    """--partitions 2 (in this process) against the serial CLI: the same files, keys, shapes and metadata keys, values within 1e-8,
    the same Newton count in every step."""
    serial, its_s = run_cli(CLI + extra, tmp_path / "serial", monkeypatch)
    parted, its_p = run_cli(CLI + extra + ["--partitions", "2"], tmp_path / "parts", monkeypatch)
    assert its_p == its_s and len(its_s) == 3
    compare_outputs(parted, serial, 1e-8)


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_cli_under_torchrun_on_one_card(gpu_lib, tmp_path, monkeypatch):
    """torch.distributed.run --nproc-per-node 2 on one card (the ranks share it: gloo + the host-staged transport): rank 0's files
    equal the in-process two-partition run's within 1e-12, rank 1 prints and writes nothing."""
    inproc, _ = run_cli(CLI + ["--partitions", "2"], tmp_path / "inproc", monkeypatch)
    out, logs = tmp_path / "torchrun", tmp_path / "logs"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
    env["GMPNP_OUT"] = str(out)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), "--log-dir", str(logs), "--redirects", "3",
           os.path.join(ROOT, "3D", "MPNP_CO2ER_pore.py")] + CLI + ["--partitions", "2"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    dirs = glob.glob(os.path.join(str(out), "*_experiment", "*"))
    assert len(dirs) == 1, dirs
    compare_outputs(dirs[0], inproc, 1e-12)
    # (every rank's gloo group prints its own "[Gloo] Rank r is connected to ..." notice: not the driver's)
    logs_out = {int(os.path.basename(os.path.dirname(p))): [ln for ln in open(p).read().splitlines() if not ln.startswith("[Gloo]")]
                for p in glob.glob(os.path.join(str(logs), "**", "stdout.log"), recursive=True)}
    assert sorted(logs_out) == [0, 1], logs_out
    assert logs_out[1] == [], logs_out
    assert logs_out[0][-9:][2::3] == ["0", "1", "2"], logs_out   # rank 0's last nine lines: CO2_min, time stamp, step index per step
