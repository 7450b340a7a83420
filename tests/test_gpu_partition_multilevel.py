"""The geometric multilevel term across mesh partitions (gmpnp_attach_coarse_level on partition handles,
gmpnp_group_attach_coarse_group; csrc/gmpnp_group.h "multilevel term"): the same Newton iterates as the serial multilevel run, the
serial run's BiCGStab counts instead of the two-level ones, the host-staged transport between processes, and the refusals."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def relerr(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def _run(steps, L=10e-9, refine=1, **kw):
    from gmpnp_amd.pore3d import PoreRun
    run = PoreRun(num_steps=steps, concentration_elec=0.5, L=L, R=5e-9, refine=refine, **kw)
    try:
        run.run(verbose=False)
        return list(run.newton_its), int(run.sys.krylov_iterations), np.array(run.history[1:])
    finally:
        run.sys.close()


@pytest.fixture(scope="module")
def serial_refine1(gpu_lib):
    return _run(2, multilevel=True)


@pytest.mark.parametrize("nparts", [1, 2, 4])
def test_partitioned_multilevel_matches_the_serial_run(serial_refine1, nparts):
    """Once-refined L_10_R_5, 2 steps, in-process partitions: identical Newton counts, states to 1e-8, the serial multilevel BiCGStab
    count (within 25 %) and less than half of what the same partitions need without the term."""
    its, kits, hist = _run(2, multilevel=True, partition=(nparts, None))
    its2, kits2, hist2 = _run(2, partition=(nparts, None))
    s_its, s_kits, s_hist = serial_refine1
    print("P=%d: multilevel %d BiCGStab its (serial %d), two-level %d" % (nparts, kits, s_kits, kits2))
    assert its == s_its
    assert relerr(hist.ravel(), s_hist.ravel()) < 1e-8
    assert kits <= 1.25 * s_kits, (kits, s_kits)
    assert kits < 0.5 * kits2, (kits, kits2)


def test_twice_refined_pore50_on_four_partitions(gpu_lib):
    """Twice-refined L_50_R_5 (the mesh where the two-level form needs about 206 BiCGStab iterations a solve), 4 in-process
    partitions, one step: at most 40 iterations a solve, the serial multilevel run's Newton counts."""
    from gmpnp_amd.pore3d import PoreRun
    run = PoreRun(num_steps=1, concentration_elec=0.5, L=50e-9, R=5e-9, refine=2, multilevel=True, partition=(4, None))
    try:
        st = run.step(verbose=False)
        per = np.array(st["krylov_per_iteration"][:st["iterations"]])
        its = list(run.newton_its)
    finally:
        run.sys.close()
    s_its, _, _ = _run(1, L=50e-9, refine=2, multilevel=True)
    print("refine 2, 4 partitions: %s BiCGStab iterations per solve (mean %.1f)" % (per.tolist(), per.mean()))
    assert per.mean() <= 40, per
    assert its == s_its


def _hosted_worker(rank, world, port, out_dir):
    import sys
    from conftest import ROOT
    sys.path.insert(0, ROOT)
    import torch.distributed as tdist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    tdist.init_process_group("gloo", rank=rank, world_size=world)   # both ranks share the one GPU of the test box
    try:
        its, kits, hist = _run(2, multilevel=True, partition=(world, rank), device_kwargs={"transport": "host"})
        if rank == 0:
            np.savez(os.path.join(out_dir, "hosted.npz"), its=np.array(its), kits=kits, hist=hist)
    finally:
        tdist.destroy_process_group()


def test_host_staged_transport_between_processes(gpu_lib, tmp_path):
    """Two PROCESSES over the host-staged transport (torch.distributed / gloo), every level's collectives through the callbacks:
    the in-process two-partition run's Newton and BiCGStab counts, states to 1e-10."""
    import torch.multiprocessing as mp
    port = 29500 + (os.getpid() % 400) + 83
    mp.spawn(_hosted_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    d = np.load(os.path.join(str(tmp_path), "hosted.npz"))
    its, kits, hist = _run(2, multilevel=True, partition=(2, None))
    assert d["its"].tolist() == its
    assert int(d["kits"]) == kits
    assert relerr(d["hist"].ravel(), hist.ravel()) < 1e-10


def test_refusals(gpu_lib):
    """The peer-mailbox transport, a coarse group of another rank count and a coarse group of handles that are not the attached
    levels are refused with GMPNP_ERR_INVALID and a message that says why."""
    from ctypes import byref, c_void_p, create_string_buffer
    from gmpnp_amd import backend, dist
    from gmpnp_amd.mesh import read_dolfin_xml, resolve_mesh_path
    from gmpnp_amd.params import pore_parameters, utilities_dir
    from gmpnp_amd.problem import pore_hierarchy
    pp = pore_parameters(concentration_elec=0.5, L=10e-9, R=5e-9)
    levels = pore_hierarchy(pp, read_dolfin_xml(resolve_mesh_path(utilities_dir(), pp.mesh_name)), 1)
    lib = backend.load_library()

    def check(code):
        if code != backend.OK:
            raise backend.GmpnpError(code, lib.gmpnp_last_error().decode())

    def handles(nparts, attach=True):
        plans = [dist.partition_hierarchy(levels, nparts, r) for r in range(nparts)]
        fine = [backend.DeviceSolver(p[0].domain.problem, perm=p[0].perm, partition=p[0].part) for p in plans]
        coarse = [backend.DeviceSolver(p[1].domain.problem, perm=p[1].perm, partition=p[1].part, shared_device=1) for p in plans]
        if attach:
            for f, c, p in zip(fine, coarse, plans):
                f.attach_coarse_level(c, p[0].parents)
        return fine, coarse

    def group(devs):
        g = c_void_p()
        check(lib.gmpnp_group_create(len(devs), (c_void_p * len(devs))(*[d._h for d in devs]), None, byref(g)))
        return g

    made, groups = [], []
    try:
        fine, coarse = handles(2)
        made += fine + coarse
        # peer-mailbox groups of the two levels (each allocates its mailbox; nothing is exchanged)
        gp_f, gp_c = c_void_p(), c_void_p()
        check(lib.gmpnp_group_peer_begin(fine[0]._h, byref(gp_f), create_string_buffer(backend.PEER_HANDLE_BYTES)))
        groups.append(gp_f)
        check(lib.gmpnp_group_peer_begin(coarse[0]._h, byref(gp_c), create_string_buffer(backend.PEER_HANDLE_BYTES)))
        groups.append(gp_c)
        with pytest.raises(backend.GmpnpError, match="peer-mailbox"):
            check(lib.gmpnp_group_attach_coarse_group(gp_f, gp_c))
        g_fine = group(fine)
        groups.append(g_fine)
        # a coarse group of four ranks under a two-rank fine group
        _, coarse4 = handles(4, attach=False)
        made += coarse4
        g4 = group(coarse4)
        groups.append(g4)
        with pytest.raises(backend.GmpnpError, match="number of ranks"):
            check(lib.gmpnp_group_attach_coarse_group(g_fine, g4))
        # a coarse group of the right size whose handles are not the levels attached to the fine group's handles
        _, other = handles(2, attach=False)
        made += other
        g_other = group(other)
        groups.append(g_other)
        with pytest.raises(backend.GmpnpError, match="not the level attached"):
            check(lib.gmpnp_group_attach_coarse_group(g_fine, g_other))
        # levels of different ranks
        with pytest.raises(backend.GmpnpError, match="same rank"):
            fine[0].attach_coarse_level(other[1], np.zeros((fine[0].ndof // 9, 2), dtype=np.int32))
        # a fine group whose coarse group was never attached does not solve
        with pytest.raises(backend.GmpnpError, match="not attached"):
            check(lib.gmpnp_group_newton_solve(g_fine, byref(backend.newton_options(None, dim=3)), None))
    finally:
        for g in groups:
            lib.gmpnp_group_destroy(g)
        for d in made:
            d.close()
