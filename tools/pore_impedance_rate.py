"""Cost of the 3D frequency response, same process, same box.

Per mesh (L_10_R_5 and L_50_R_5; Stern BDM at p_M = -1, Tafel kinetics, the state after `--steps` driver steps with the band LU; where
those steps fail on a mesh the bulk state stands in and the record says so: the cost does not depend on the state), for n = 1, 8
and one full chunk of frequencies (what gmpnp_options_t.band_lu_max_gb holds; `--cap-gb` sets it):
  call_s     wall time of one gmpnp_frequency_response_3d (set-up, every chunk launch, the read-back; it ends in a synchronise)
  hook30_s   gmpnp_time_kernel(30): every launch of the last chunk, by device events
beside the real solver of the same handle, timed the same way: band_lu_s = wall time of one gmpnp_linear_solve with the block-banded
LU (factorisation, substitution, true residual, refinement).  Each figure is the median of `--repeats` (7) measurements after one
warm-up, with the smallest and the largest.  `--nyquist` adds the spectrum of the last state on the driver's default grid.
Writes JSON (default profiles/pore_impedance.json).

    python tools/pore_impedance_rate.py [--repeats 7] [--steps 2] [--meshes 10,50] [--cap-gb 48] [--nyquist] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TAFEL = dict(kinetics="tafel", i0_CO=10.0, i0_H2=1.0)


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def timed(call, repeats):
    call()   # warm-up: first launches load code objects, the first call allocates
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        out.append(time.perf_counter() - t0)
    return spread(out)


def mesh_case(L_nm, steps, repeats, cap_gb, nyquist):
    import numpy as np
    from gmpnp_amd import backend
    from gmpnp_amd import impedance as imp
    from gmpnp_amd.pore3d import SOLVER_PARAMETERS, PoreRun
    sp = {"nonlinear_solver": "newton", "newton_solver": dict(SOLVER_PARAMETERS["newton_solver"], linear_solver="band_lu")}
    run = PoreRun(num_steps=steps, solver_parameters=sp, electrode_voltage=-1.0, L=L_nm * 1e-9, R=5e-9, concentration_elec=0.5,
                  device_kwargs=dict(band_lu_max_gb=cap_gb), **TAFEL)
    try:
        nv = int(run.mesh.num_vertices)
        state = "after %d driver steps" % steps
        try:
            run.run(verbose=False)
        except backend.GmpnpError as e:   # (the cost does not depend on the state: the bulk state stands in, and the record says so)
            state = "the bulk state (the driver's steps failed: %s)" % str(e)[:160]
            run.sys.set_state(np.tile(np.r_[np.ones(8), 0.0], nv), None)
            nyquist = False
        dev = run.sys.dev
        _, band = dev.band_lu_shape()
        per = imp.band_bytes_per_frequency(nv, band, 9)
        full = imp.band_chunk(imp.MAX_FREQUENCIES, nv, band, 9, cap_gb * 1e9)
        out = {"vertices": nv, "state": state, "band": band, "band_gb_per_frequency": per / 1e9, "cap_gb": cap_gb, "full_chunk": full}
        dev.assemble(True)
        rhs = np.random.default_rng(1).standard_normal(run.problem.ndof)
        out["band_lu_s"] = timed(lambda: dev.linear_solve(rhs, backend.LINEAR_BAND_LU), repeats)
        for n in sorted({1, min(8, full), full}):
            sig = imp.pore_sigma_from_frequency(run.pp, np.logspace(0, 6, n))
            res = {}
            wall = timed(lambda: res.update(dev.frequency_response_3d(sig)), repeats)
            hook = spread([dev.time_kernel(30, 1) * 1e-6 for _ in range(repeats)])
            out["n_%d" % n] = {"call_s": wall, "hook30_s": hook, "worst_residual": float(np.max(res["residual"])),
                               "status": int(np.bitwise_or.reduce(res["status"]))}
        if nyquist:
            f = imp.frequency_grid(1e0, 1e8, 2)
            spc = run.pore_impedance(f)
            out["nyquist"] = {"frequency": f.tolist(), "Z_re": spc["impedance"].real.tolist(), "Z_im": spc["impedance"].imag.tolist(),
                              "capacitance_re": spc["capacitance"].real.tolist(), "steps": steps}
        return out
    finally:
        run.sys.close()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--meshes", default="10,50", help="pore lengths in nm (R = 5 nm)")
    ap.add_argument("--cap-gb", type=float, default=48.0)
    ap.add_argument("--nyquist", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pore_impedance.json"))
    a = ap.parse_args(argv)
    from gmpnp_amd import backend
    lib = backend.load_library()
    res = {"build_id": lib.gmpnp_build_id().decode(), "repeats": a.repeats, "steps": a.steps, "nyquist": bool(a.nyquist)}
    for L in (int(v) for v in a.meshes.split(",")):
        res["L_%d_R_5" % L] = mesh_case(L, a.steps, a.repeats, a.cap_gb, a.nyquist)
        print(json.dumps({("L_%d_R_5" % L): res["L_%d_R_5" % L]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
