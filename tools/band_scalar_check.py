"""Bits of everything that runs the block-banded LU (gmpnp_band_lu.h), one library against another's: the record
profiles/band_scalar_refactor.json.

  band_scalar_check.py dump OUT.npz                 (GMPNP_LIB names the library) every item below from seeded states (the tests'
                                                    random_state), the arrays as the library returned them
  band_scalar_check.py compare A B C [EXTRA.json]   A, B: two dumps of the parent's library, C: the branch's.  Prints the record; the
                                                    keys of EXTRA.json (resource usage, speed) are merged into it.

Items: the real solve (gmpnp_linear_solve with the band LU, two right-hand sides) on the generated cylinders (1, 1), (1, 4), (2, 5) and
on L_10_R_5; the 3D frequency response with x at sigma = 0, 1e2, 1e6 on the same shapes, as one chunk and under a memory cap that makes
chunks of two; the electrode tangent's columns on one cylinder, a potentiostatic and a galvanostatic Newton solve on another; the state after two driver steps of
L_10_R_5 with the band LU.  Every array is compared with ==: no sum is reordered between the libraries, so there is no tolerance."""
import copy, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import numpy as np

CYLINDERS = {"c1x1": (1, 1), "c1x4": (1, 4), "c2x5": (2, 5)}
SIGMAS = (0.0, 1e2, 1e6)
P_M = -1.0


def random_state(nv, ns, seed=0):   # tests/conftest.py
    rng = np.random.default_rng(seed)
    u = np.concatenate([rng.uniform(.5, 1.5, (nv, ns)), rng.uniform(-1, 0, (nv, 1))], axis=1).ravel()
    un = np.concatenate([rng.uniform(.5, 1.5, (nv, ns)), rng.uniform(-1, 0, (nv, 1))], axis=1).ravel()
    return u, un


def problems():
    """name -> (the plain problem of the real solve, the Stern + Tafel problem of the response)"""
    import closed_forms as cf
    import pore_response_reference as P
    from test_kinetics_reference import two_reactions
    from gmpnp_amd.mesh import read_dolfin_xml, resolve_mesh_path
    from gmpnp_amd.params import pore_parameters, utilities_dir
    from gmpnp_amd.problem import SternLayer, pore_problem
    from gmpnp_amd.stern import L_STERN
    out = {}
    for name, coarse in CYLINDERS.items():
        plain = cf._base(10e-9, 5e-9, 0, reactions=True, wall_flux=True, steady=False, q_scale=1.0, coarse=coarse)[0]
        out[name] = (plain, P.cylinder_case(coarse, p_M=P_M))
    pp = pore_parameters(concentration_elec=0.5, L=10e-9, R=5e-9)
    mesh = read_dolfin_xml(resolve_mesh_path(utilities_dir(), pp.mesh_name))
    stern = copy.copy(pore_problem(pp, mesh, stern=SternLayer("BDM", P_M, L_STERN / pp.L))[0])
    stern.kinetics = two_reactions(list(stern.model.species), P_M)
    out["pore10"] = (pore_problem(pp, mesh)[0], stern)
    return out


def dump(path):
    from gmpnp_amd import backend
    from gmpnp_amd import impedance as imp
    from gmpnp_amd.pore3d import SOLVER_PARAMETERS, PoreRun
    from gmpnp_amd.problem import Galvanostat
    res = {"build_id": np.array(backend.load_library().gmpnp_build_id().decode())}

    def response(prefix, r):
        for k in ("x", "C", "dI", "residual", "status"):
            res[prefix + "/" + k] = np.asarray(r[k])

    probs = problems()
    for name, (plain, stern) in probs.items():
        nv = plain.coords.shape[0]
        u, un = random_state(nv, plain.nf - 1, seed=11)
        with backend.DeviceSolver(plain) as dev:
            dev.set_state(u, un)
            dev.assemble(True)
            rng = np.random.default_rng(3)
            for k, rhs in enumerate((rng.standard_normal(plain.ndof), rng.standard_normal(plain.ndof))):
                x, st = dev.linear_solve(rhs, backend.LINEAR_BAND_LU)
                res["solve/%s/rhs%d/x" % (name, k)] = x
                res["solve/%s/rhs%d/converged_residual" % (name, k)] = np.array([float(st["converged"]), st["residual_norm"], st["rhs_norm"]])
        u, un = random_state(nv, stern.nf - 1, seed=3)
        with backend.DeviceSolver(stern) as dev:
            dev.set_state(u, un)
            response("response/%s/one_chunk" % name, dev.frequency_response_3d(SIGMAS, want_x=True))
            _, band = dev.band_lu_shape()
        per = imp.band_bytes_per_frequency(nv, band, 9)
        with backend.DeviceSolver(stern, band_lu_max_gb=2.5 * per / 1e9) as dev:
            dev.set_state(u, un)
            response("response/%s/chunks_of_two" % name, dev.frequency_response_3d(SIGMAS, want_x=True))
        print(name, "done", flush=True)

    stern = probs["c2x5"][1]
    u, un = random_state(stern.coords.shape[0], stern.nf - 1, seed=3)
    with backend.DeviceSolver(stern) as dev:
        dev.set_state(u, un)
        t = dev.electrode_tangent([0, 16, 17, 32, 33, 48], want_z=True)
        for k in ("z", "dD", "dI", "residual", "status"):
            res["tangent/c2x5/" + k] = np.asarray(t[k])
    # galvanostat: the first step of the 259-vertex cylinder from u = 0 (tests/test_gpu_galvanostat.py), the target half the current of
    # the potentiostatic first step, which is an item of its own (Newton on band_solve); then Newton on the two refined substitutions
    import pore_response_reference as P
    pot = P.cylinder_case((3, 6), p_M=P_M)
    start = (np.zeros(pot.ndof), np.tile(np.r_[np.ones(pot.nf - 1), 0.0], pot.coords.shape[0]))
    sp = {"nonlinear_solver": "newton", "newton_solver": {"linear_solver": "band_lu", "maximum_iterations": 50, "relative_tolerance": 1e-9, "absolute_tolerance": 1e-6}}

    def newton_item(prefix, dev):
        try:
            st = dev.newton_solve(backend.newton_options(sp, dim=3), error_on_nonconvergence=False)
            res[prefix + "/iterations_direct_solves_converged"] = np.array([st["iterations"], st["direct_solves"], int(st["converged"])])
            res[prefix + "/residuals"] = np.asarray(st["residuals"], dtype=np.float64)
        except backend.GmpnpError as e:
            res[prefix + "/error"] = np.array(str(e))
        res[prefix + "/state"] = dev.get_state()

    with backend.DeviceSolver(pot) as dev:
        dev.set_state(*start)
        newton_item("newton/c3x6_potentiostatic", dev)
        dev.set_galvanostat(Galvanostat(1.0))
        current = dev.galvanostat_report()["I"]
    on = copy.copy(pot)
    on.galvanostat = Galvanostat(0.5 * current)
    with backend.DeviceSolver(on) as dev:
        dev.set_state(*start)
        newton_item("galvanostat/c3x6", dev)
        rep = dev.galvanostat_report()
        res["galvanostat/c3x6/p_electrode_I_G_target"] = np.array([rep["p_electrode"], rep["I"], rep["G"], 0.5 * current])
    print("tangent, galvanostat done", flush=True)

    band = {"nonlinear_solver": "newton", "newton_solver": dict(SOLVER_PARAMETERS["newton_solver"], linear_solver="band_lu")}
    run = PoreRun(num_steps=2, solver_parameters=band, concentration_elec=0.5, L=10e-9, R=5e-9)
    try:
        its = []
        for _ in range(2):
            st = run.step(verbose=False)
            its.append([st["iterations"], st.get("direct_solves", 0)])
        res["driver/pore10_two_steps/state"] = np.asarray(run.history[-1])
        res["driver/pore10_two_steps/iterations_direct_solves"] = np.array(its)
    finally:
        run.sys.close()
    np.savez(path, **res)
    print("wrote", path, len(res) - 1, "arrays", flush=True)


def compare(a, b, c, extra=None):
    A, B, C = (np.load(p) for p in (a, b, c))
    keys = [k for k in A.files if k != "build_id"]
    assert set(keys) == set(B.files) - {"build_id"} == set(C.files) - {"build_id"}
    out = {"what": "everything that runs the block-banded LU: the parent's library against itself (two processes) and against the branch's, "
                   "arrays compared with ==; tools/band_scalar_check.py",
           "build_id": {"parent": [str(A["build_id"]), str(B["build_id"])], "branch": str(C["build_id"])}, "items": {}}
    for k in keys:
        item = {"shape": list(A[k].shape), "parent_reproduces_itself": bool(np.array_equal(A[k], B[k])), "branch_equals_parent": bool(np.array_equal(A[k], C[k]))}
        if A[k].size <= 32 and A[k].dtype.kind in "fiub":   # statuses, residuals, counts
            item["parent"] = A[k].tolist(); item["branch"] = C[k].tolist()
        out["items"][k] = item
    out["all_bitwise_equal"] = all(i["parent_reproduces_itself"] and i["branch_equals_parent"] for i in out["items"].values())
    if extra:
        out.update(json.load(open(extra)))
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    dump(sys.argv[2]) if sys.argv[1] == "dump" else compare(*sys.argv[2:])
