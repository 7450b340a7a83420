"""Bits of the three record streams (the electrode trace, the wall profile, the transient sensitivities), one library against another's:
the record profiles/record_stream_refactor.json.

  record_stream_check.py dump OUT.npz                 (GMPNP_LIB names the library) every item below from seeded states (the tests'
                                                      random_state), the records as raw bytes of the structured arrays
  record_stream_check.py compare A B C [EXTRA.json]   A, B: two dumps of the parent's library, C: the branch's.  Prints the record; the
                                                      keys of EXTRA.json (resource usage, speed, size) are merged into it.

Cases: the uniform 1D meshes of 9 and 65 vertices (the programme tests'), the generated cylinders (1, 1) and (2, 5) and L_10_R_5, each
with the kinetics on and off.  Items, each five appends at five states through ``DeviceProgrammeOps``, once with capacity 2 (two drains
and reopens, a partly filled last chunk) and once with capacity 8 (no drain): the electrode records; in 3D the wall profile with 1, 3 and the largest number of uniform bins
that leaves no bin empty; in 1D the sensitivity records, S and the last right-hand sides with 2 and 10 columns (kinetics off: the 2 that
need none; 10 on the four-reaction problem of 65 vertices); the solver state behind each item and behind the timing hooks 29 / 31 / 32,
which must leave state and records alone.  Every array is compared byte for byte: no sum is reordered, so there is no tolerance.
One difference is meant and reported by field: behind a drained buffer the parent's ``DeviceProgrammeOps`` adds a chunk's charges to the
carried ones as a whole, this tree's continues the device's sums record by record, so Q and Q_D of the electrode records and Q of the
profile may differ in the last bits at capacity 2, where this tree's records equal its records at capacity 8 and the parent's need not."""
import copy, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import numpy as np

STEPS = [(0.5, 0.5), (0.75, 0.25), (2.0, 1.25), (2.0 + 1e-3, 1e-3), (7.0, 4.999)]     # (t, h) of the five appends
CAPACITIES = (2, 8)
TEN = (0, 16, 17, 18, 19, 32, 33, 34, 35, 48)


def random_state(nv, ns, seed=0):   # tests/conftest.py
    rng = np.random.default_rng(seed)
    u = np.concatenate([rng.uniform(.5, 1.5, (nv, ns)), rng.uniform(-1, 0, (nv, 1))], axis=1).ravel()
    un = np.concatenate([rng.uniform(.5, 1.5, (nv, ns)), rng.uniform(-1, 0, (nv, 1))], axis=1).ravel()
    return u, un


def raw(a):
    return np.frombuffer(np.ascontiguousarray(a).tobytes(), dtype=np.uint8)


class HandleRun:
    """What ``DeviceProgrammeOps`` reads of a driver run, over a bare problem (no Newton solve: the states are set)."""

    def __init__(self, prob):
        from gmpnp_amd.solver import GMPNPSystem
        self.problem, self.stern, self.kinetics, self.budget = prob, prob.stern, prob.kinetics, None
        self.sys = GMPNPSystem(prob)
        self.sys.last_stats = {"residuals": [0.0]}


def problems():
    """name -> problem"""
    import hp_reference as H
    import pore_response_reference as PP
    from test_gpu_tangent import four_reactions
    from test_kinetics_reference import two_reactions
    from test_programme_reference import P_M, uniform_problem
    from gmpnp_amd.mesh import read_dolfin_xml, resolve_mesh_path
    from gmpnp_amd.params import edl_parameters, pore_parameters, utilities_dir
    from gmpnp_amd.problem import SternLayer, edl_problem, pore_problem
    from gmpnp_amd.stern import L_STERN
    out = {}
    for kin in (True, False):
        tag = "kin" if kin else "nokin"
        for nv in (9, 65):
            out["uniform%d/%s" % (nv, tag)] = uniform_problem(nv, kin)[1]
        for name, coarse in (("c1x1", (1, 1)), ("c2x5", (2, 5))):
            out["%s/%s" % (name, tag)] = PP.cylinder_case(coarse, p_M=-1.0, kinetics=kin)
        pp = pore_parameters(concentration_elec=0.5, L=10e-9, R=5e-9)
        mesh = read_dolfin_xml(resolve_mesh_path(utilities_dir(), pp.mesh_name))
        prob = copy.copy(pore_problem(pp, mesh, stern=SternLayer("BDM", -1.0, L_STERN / pp.L))[0])
        prob.kinetics = two_reactions(list(prob.model.species), -1.0) if kin else None
        out["pore10/%s" % tag] = prob
    ep = edl_parameters(cation="Cs", voltage_multiplier=-10.0)
    out["uniform65/four"] = edl_problem(ep, H.uniform_mesh_1d(65), stern=SternLayer("BDM", P_M, L_STERN / ep.L_n), kinetics=four_reactions(ep.species, P_M))
    return out


def bin_counts(prob):
    """1, 3 and the largest number of uniform bins over [0, 1] that leaves no bin without a node of the wall"""
    import kinetics_reference as K
    from gmpnp_amd import programme as P
    z = np.asarray(prob.coords)[K.boundary_weights(prob)[0], 2]
    most = 1
    for n in range(256, 0, -1):
        edges = P.uniform_edges(0.0, 1.0, n)
        if len({P.wall_bin(float(v), edges, n) for v in z} - {-1}) == n:
            most = n
            break
    return sorted({1, min(3, most), most})


def dump(path):
    from gmpnp_amd import backend
    from gmpnp_amd import programme as P
    res = {"build_id": np.array(backend.load_library().gmpnp_build_id().decode())}

    def item(name, prob, hook, **kw):
        for capacity in CAPACITIES:
            one("%s/cap%d" % (name, capacity), prob, hook, capacity, **kw)

    def one(prefix, prob, hook, capacity, **kw):
        nv, ns = prob.coords.shape[0], prob.nf - 1
        states = [random_state(nv, ns, seed=17 + k)[0] for k in range(len(STEPS) + 1)]
        run = HandleRun(copy.copy(prob))
        try:
            dev = run.sys.dev
            run.sys.set_state(states[0], states[0])
            ops = P.DeviceProgrammeOps(run, {}, None, capacity=capacity, **kw)
            for k, ((t, h), u) in enumerate(zip(STEPS, states[1:])):
                dev.set_state(u, None)
                if k == 3:   # between two appends of one chunk
                    res[prefix + "/hook_us_positive"] = np.array(dev.time_kernel(hook, 2) > 0.0)
                ops.record(t, h, 0, float(prob.stern.p_electrode))
            if "sensitivities" in kw:
                res[prefix + "/sensitivity"] = raw(ops.sensitivity_records())
                res[prefix + "/S"] = raw(dev.sensitivity_columns(0))
                res[prefix + "/rhs"] = raw(dev.sensitivity_columns(1))
                dev.sensitivity_close()
            res[prefix + "/electrode"] = raw(ops.records())
            if "profile_edges" in kw:
                res[prefix + "/profile"] = raw(ops.profile_records())
            res[prefix + "/chunks"] = np.array(len(ops.chunks))
            res[prefix + "/state"] = raw(dev.get_state())
        finally:
            run.sys.close()

    for name, prob in problems().items():
        if name.endswith("/four"):
            item(name + "/sens10", prob, 31, sensitivities=TEN)
        elif prob.coords.shape[1] == 1:
            item(name + "/trace", prob, 29)
            item(name + "/sens2", prob, 31, sensitivities=(0, 48))
        else:
            item(name + "/trace", prob, 29)
            for n in bin_counts(prob):
                item(name + "/bins%d" % n, prob, 32, profile_edges=P.uniform_edges(0.0, 1.0, n))
        print(name, "done", flush=True)
    np.savez(path, **res)
    print("wrote", path, len(res) - 1, "arrays", flush=True)


def fields_that_differ(key, x, y):
    """The fields of a record item in which two dumps differ (None: not a record item)."""
    from gmpnp_amd import backend
    dtype = {"electrode": backend.ELECTRODE_RECORD_DTYPE, "profile": backend.WALL_PROFILE_RECORD_DTYPE,
             "sensitivity": backend.SENSITIVITY_RECORD_DTYPE}.get(key.rsplit("/", 1)[1])
    if dtype is None or x.size != y.size:
        return None
    x, y = x.view(dtype), y.view(dtype)
    return [f for f in dtype.names if x[f].tobytes() != y[f].tobytes()]


def compare(a, b, c, extra=None):
    A, B, C = (np.load(p) for p in (a, b, c))
    keys = [k for k in A.files if k != "build_id"]
    assert set(keys) == set(B.files) - {"build_id"} == set(C.files) - {"build_id"}
    out = {"what": "the electrode trace, the wall profile and the transient sensitivities through DeviceProgrammeOps with capacity 2 and 8: "
                   "the parent's tree and library against themselves (two processes) and against this tree's, arrays compared byte for "
                   "byte; tools/record_stream_check.py",
           "build_id": {"parent": [str(A["build_id"]), str(B["build_id"])], "branch": str(C["build_id"])}, "items": {}}
    carried, other, capacity = {}, [], {"parent": [], "branch": []}
    for k in keys:
        item = {"bytes": int(A[k].size), "parent_reproduces_itself": bool(np.array_equal(A[k], B[k])), "branch_equals_parent": bool(np.array_equal(A[k], C[k]))}
        if A[k].dtype != np.uint8:   # counts, flags
            item["parent"] = A[k].tolist(); item["branch"] = C[k].tolist()
        if not item["branch_equals_parent"]:
            item["fields_that_differ"] = fields_that_differ(k, A[k], C[k])
            if "/cap2/" in k and item["fields_that_differ"] and set(item["fields_that_differ"]) <= {"Q", "Q_D"}:
                carried[k] = item["fields_that_differ"]
            else:
                other.append(k)
        if "/cap2/" in k and A[k].dtype == np.uint8:
            k8 = k.replace("/cap2/", "/cap8/")
            item["equals_capacity_8"] = {"parent": bool(np.array_equal(A[k], A[k8])), "branch": bool(np.array_equal(C[k], C[k8]))}
            for who in capacity:
                if not item["equals_capacity_8"][who]:
                    capacity[who].append(k)
        out["items"][k] = item
    out["parent_reproduces_itself"] = all(i["parent_reproduces_itself"] for i in out["items"].values())
    out["differs_from_parent_in_carried_sums_only"] = carried       # item -> fields, capacity 2 only
    out["differs_from_parent_otherwise"] = other                    # must be empty
    out["capacity_2_differs_from_capacity_8"] = capacity            # the branch's list must be empty
    out["all_bitwise_equal_but_carried_sums"] = out["parent_reproduces_itself"] and not other and not capacity["branch"]
    if extra:
        out.update(json.load(open(extra)))
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    dump(sys.argv[2]) if sys.argv[1] == "dump" else compare(*sys.argv[2:])
