"""The record streams of a programme on the GPU (the electrode trace, the wall profile, the transient sensitivities; RecordStream in
csrc/gmpnp_api.hip and in gmpnp_amd/programme.py): what a run records does not depend on the capacity of its buffers.  Five fixed steps
with capacity 2 are two drained and reopened buffers and a partly filled last chunk; with capacity 8 nothing is drained.  Every handle
is closed by `finally`."""
import copy

import numpy as np
import pytest

import pore_programme_reference as PPR
from test_gpu_programme import HandleRun, bits
from test_programme_reference import P_M, steady_case
from gmpnp_amd import programme as P
from gmpnp_amd.polarisation import NEWTON

pytestmark = pytest.mark.gpu
STEPS = 5


def stream_case(name):
    """(problem, start state, Newton options, inv_dt_of_h, one ramp of STEPS reference steps, the streams beside the trace)"""
    if name == "uniform9":      # the smallest 1D mesh of the programme tests, two sensitivity columns
        _, prob, u, inv = steady_case(9)
        return prob, u, dict(NEWTON), inv, [(0.0, STEPS * 9.5, P_M, P_M - 0.25)], dict(sensitivities=(0, 48))
    prob, u, dt = PPR.march_case((1, 1))      # the smallest generated cylinder, a profile of two bins
    sp = {"newton_solver": dict(NEWTON["newton_solver"], linear_solver="band_lu")}
    return prob, u, sp, (lambda h: 1.0 / h), [(0.0, STEPS * dt, PPR.MARCH_P_M, PPR.MARCH_P_M - 0.25)], dict(profile_edges=P.uniform_edges(0.0, 1.0, 2))


def march(case, capacity):
    prob, u, sp, inv, segs, streams = case
    run = HandleRun(copy.copy(prob))
    try:
        run.sys.set_state(np.array(u), np.array(u))
        ops = P.DeviceProgrammeOps(run, sp, inv, capacity=capacity, **streams)
        P.run_programme(ops, segs, steps_per_segment=STEPS)
        out = {}
        if "sensitivities" in streams:
            out["sensitivity"] = ops.sensitivity_records()
            run.sys.dev.sensitivity_close()
        out["electrode"] = ops.records()
        if "profile_edges" in streams:
            out["profile"] = ops.profile_records()
        return out, len(ops.chunks)
    finally:
        run.sys.close()


@pytest.mark.parametrize("name", ["uniform9", "c1x1"])
def test_records_do_not_depend_on_the_capacity(name, gpu_lib):
    """The charges are the fields at stake: the device starts Q and Q_D at 0 with every open, and behind a drained buffer the host
    continues the device's sums record by record from the chunk before (``programme.RecordStream``).  Adding a chunk's sums to the
    carried ones as a whole gives Q_2 + (h_3 I_3 + h_4 I_4) where the undrained run holds (Q_2 + h_3 I_3) + h_4 I_4: measured on the
    MI355X in that form, c1x1 missed ``Q`` of the electrode records of steps 3 and 4 (counted from 0) by the last bit, 5.8e-18 of
    the largest value, with every other field and uniform9 equal.  The sensitivities' device side keeps its own accumulators."""
    case = stream_case(name)
    (small, chunks_small), (large, chunks_large) = march(case, 2), march(case, 8)
    assert chunks_small == 3 and chunks_large == 1 and len(small) == 2
    differ = {}
    for key, rec in small.items():
        assert len(rec) == STEPS == len(large[key]) and rec.dtype == large[key].dtype and not rec["status"].any()
        for field in rec.dtype.names:
            a, b = rec[field], large[key][field]
            if not np.array_equal(a, b):
                steps = sorted({int(k) for k in np.argwhere(a != b)[:, 0]})
                differ[key + "." + field] = (steps, float(np.abs(a - b).max() / np.abs(b).max()))
    print("records of %s with capacity 2 against capacity 8: fields that differ (steps, largest difference / largest value): %s" % (name, differ))
    assert not differ
    assert all(bits(rec) == bits(large[key]) for key, rec in small.items())
