"""The electrode tangent and the polarisation curve on the GPU (gmpnp_electrode_tangent / gmpnp_electrode_advance,
csrc/gmpnp_tangent.h): the columns, the tangents of the multi-column cyclic reduction against gmpnp_linear_solve
(bit for bit) and against splu on the device's own Jacobian, the functionals against the NumPy rule, the zero-frequency response and
differences of steady states, equal bits across n, across calls and for a following Newton solve, the advance, every refusal, hook 28,
and the 1D driver's curve.  Uniform meshes of 2, 3, 9, 64 and 65 vertices with a random state and two reactions, and the 1 um case, at
inv_dt = 0 and at the first step's inv_dt; the 3D library call and the 3D driver on L_10_R_5.  Every handle is closed by `with` /
`finally`."""
import copy
import json
import os

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import kinetics_reference as K
import response_reference as R
import tangent_reference as T
from conftest import random_state
from step_limit_reference import first_step_state
from test_gpu_kinetics import edl_k  # noqa: F401 (fixture)
from test_gpu_response import generated_problem
from test_kinetics_reference import TAFEL, first_step_problem, two_reactions
from gmpnp_amd import polarisation as pol
from gmpnp_amd.problem import Galvanostat, SternLayer, SurfaceKinetics, SurfaceReaction, edl_problem
from gmpnp_amd.stern import L_STERN

pytestmark = pytest.mark.gpu
P_M = -5.0
PARAMS = (0, 16, 17, 32, 33, 48)          # one M = 8 chain
SHUFFLED = (48, 17, 0, 33, 16, 32)
CASES = ("uniform2", "uniform3", "uniform9", "uniform64", "uniform65", "edl1")
KEYS = ("param", "dD", "dI", "dp_boundary", "residual", "status", "z")
STEADY = {"newton_solver": {"maximum_iterations": 50, "relative_tolerance": 1e-13, "absolute_tolerance": 1e-7}}


@pytest.fixture(scope="module")
def inputs(edl_k):
    """name -> (problem, u, u_n): a random state on the generated meshes; on the 1 um mesh the steady state (NumPy Newton at
    inv_dt = 0) for the steady tangent and the first step's state with u_n = bulk for the one-step tangent."""
    out = {}
    for nv in (2, 3, 9, 64, 65):
        u = random_state(nv, 6, seed=nv)[0]
        out["uniform%d" % nv] = (generated_problem(nv), {0: (u, u), 1: (u, random_state(nv, 6, seed=100 + nv)[0])})
    ep, mesh = edl_k
    prob = first_step_problem(ep, mesh, P_M)
    u0, un = first_step_state(prob)
    u1, st = K.newton_loop(prob, u0, un)
    assert st.converged
    us = R.steady_state(prob, u1)[0]
    out["edl1"] = (prob, {0: (us, us), 1: (u1, un)})
    return out


def rel_residual(J, x, c):
    """max |J x + c| / max |c| with the terms formed in extended precision, and the rounding of its fp64 evaluation."""
    A = J.tocoo()
    r = c.astype(np.longdouble)
    np.add.at(r, A.row, A.data.astype(np.longdouble) * x.astype(np.longdouble)[A.col])
    rounding = 30 * np.finfo(float).eps * float((abs(J) @ np.abs(x) + np.abs(c)).max() / np.abs(c).max())
    return float(np.abs(r).max() / np.abs(c).max()), rounding


@pytest.fixture(scope="module")
def device_results(inputs, gpu_lib):
    """(name, steady or one-step) -> what the device returned; one handle per entry, closed before the tests look."""
    out = {}
    for name, (prob, states) in inputs.items():
        for which, inv_dt in ((0, 0.0), (1, float(prob.model.inv_dt))):
            u, un = states[which]
            q = R.with_inv_dt(prob, inv_dt)
            with gpu_lib.DeviceSolver(q) as dev:
                dev.set_state(u, un)
                six = dev.electrode_tangent(PARAMS, want_z=True)
                c = dev.tangent_columns(len(PARAMS))
                J = dev.jacobian_csr()
                F = dev.assemble(False)[0]
                again = dev.electrode_tangent(PARAMS, want_z=True)
                shuffled = dev.electrode_tangent(SHUFFLED, want_z=True)
                single = [dev.electrode_tangent([p], want_z=True) for p in PARAMS]          # M = 2 chains
                pair = dev.electrode_tangent(PARAMS[4:], want_z=True)
                dev.assemble(True)
                x = [dev.linear_solve(-c[k], gpu_lib.LINEAR_BLOCK_TRIDIAGONAL)[0] for k in range(len(PARAMS))]
                resp = dev.frequency_response([0.0]) if inv_dt == 0.0 else None
                dev.set_galvanostat(Galvanostat(1.0))
                b = dev.galvanostat_terms()[0]
                dev.set_galvanostat(None)
            out[name, which] = dict(prob=q, u=u, six=six, c=c, J=J, F=F, again=again, shuffled=shuffled, single=single, pair=pair, x=x, resp=resp, b=b)
    return out


def same_bits(a, b, k=None, j=None):
    for key in KEYS:
        if key == "param":
            continue
        x = np.ascontiguousarray(a[key] if k is None else a[key][k])
        y = np.ascontiguousarray(b[key] if j is None else b[key][j])
        if x.tobytes() != y.tobytes():
            return False
    return True


@pytest.mark.parametrize("which", (0, 1))
@pytest.mark.parametrize("name", CASES)
def test_columns_and_tangents(name, which, device_results):
    """The p_M column is gmpnp_galvanostat_terms' b bit for bit and the other columns the NumPy closed forms (1e-13 of the column's
    largest entry; zero on every Dirichlet row); every z_k is gmpnp_linear_solve(-c_k, block-tridiagonal) bit for bit (so its error
    against splu on the device's own Jacobian and its residual ARE the one-column solver's: the factor 2 of the bound is not used);
    the reported residual agrees with the extended-precision one within the rounding of its own fp64 evaluation; status 0."""
    import tangent_reference as T
    d = device_results[name, which]
    q, u, six, c, J = d["prob"], d["u"], d["six"], d["c"], d["J"]
    assert not six["status"].any() and list(six["param"]) == list(PARAMS)
    assert c[0].tobytes() == d["b"].tobytes()
    bc = np.asarray(q.bc_dofs, dtype=np.int64)
    lu = spla.splu(J.tocsc())
    for k, p in enumerate(PARAMS):
        ref = T.column(q, u, p)
        assert np.abs(c[k] - ref).max() <= 1e-13 * np.abs(ref).max() and not c[k][bc].any(), (name, p)
        assert six["z"][k].tobytes() == d["x"][k].tobytes() or np.array_equal(six["z"][k], d["x"][k]), (name, p)
        xs = lu.solve(-c[k])
        e_multi = float(np.abs(six["z"][k] - xs).max() / np.abs(xs).max())
        e_one = float(np.abs(d["x"][k] - xs).max() / np.abs(xs).max())
        res, rounding = rel_residual(J, six["z"][k], c[k])
        res_one = rel_residual(J, d["x"][k], c[k])[0]
        print("%s inv_dt %g param %d: z against splu %.2e (one column %.2e), residual %.2e (one column %.2e, reported %.2e)"
              % (name, q.model.inv_dt, p, e_multi, e_one, res, res_one, six["residual"][k]))
        assert e_multi <= 2.0 * e_one and res <= 2.0 * res_one
        assert abs(six["residual"][k] - res) <= rounding, (name, p, six["residual"][k], res, rounding)


@pytest.mark.parametrize("which", (0, 1))
@pytest.mark.parametrize("name", CASES)
def test_functionals_against_the_numpy_rule(name, which, device_results):
    """dD, dI_r and dp_boundary against the NumPy rule (tangent_reference.functionals) applied to the device's own z: 1e-12 relative
    (of the largest entry for dI)."""
    d = device_results[name, which]
    for k, p in enumerate(PARAMS):
        fD, fI, fp = T.functionals(d["prob"], d["u"], d["six"]["z"][k], p)
        assert abs(d["six"]["dD"][k] - fD) <= 1e-12 * abs(fD), (name, p)
        assert np.abs(d["six"]["dI"][k] - fI).max() <= 1e-12 * np.abs(fI).max(), (name, p)
        assert abs(d["six"]["dp_boundary"][k] - fp) <= 1e-12 * abs(fp), (name, p)


@pytest.mark.parametrize("name", CASES)
def test_p_M_column_is_the_zero_frequency_response(name, device_results):
    """dD and dI_r of the p_M column at inv_dt = 0 against gmpnp_frequency_response([0]): 1e-8 (two solvers on one system; 5k
    measured both at 5e-11 of x)."""
    d = device_results[name, 0]
    C, dI = d["resp"]["C"][0], d["resp"]["dI"][0]
    eC = abs(d["six"]["dD"][0] - C.real) / abs(C.real)
    eI = np.abs(d["six"]["dI"][0] - dI.real).max() / np.abs(dI.real).max()
    print("%s: against the zero-frequency response dD %.2e dI %.2e" % (name, eC, eI))
    assert eC <= 1e-8 and eI <= 1e-8


@pytest.mark.parametrize("which", (0, 1))
@pytest.mark.parametrize("name", CASES)
def test_bits_do_not_depend_on_n_on_the_order_or_on_the_call(name, which, device_results):
    """A column alone (an M = 2 chain), in a pair, among six in another order (M = 8 chains) and in a second call: equal bits of z
    and of every functional."""
    d = device_results[name, which]
    assert same_bits(d["six"], d["again"])
    for k, p in enumerate(PARAMS):
        assert same_bits(d["six"], d["single"][k], k, 0), (name, p)
        assert same_bits(d["six"], d["shuffled"], k, SHUFFLED.index(p)), (name, p)
    for j, p in enumerate(PARAMS[4:]):
        assert same_bits(d["six"], d["pair"], PARAMS.index(p), j)


def four_reactions(species, p_M):
    base = two_reactions(species, p_M).reactions
    return SurfaceKinetics(base + [SurfaceReaction(k=2e-2, alpha=0.3, p_eq=0.1, reactant="OH", nu={"OH": 0.5, "H": -0.2}),
                                   SurfaceReaction(k=3e-3, alpha=0.7, p_eq=0.0, reactant=None, nu={"CO2": -0.3})], p_M)


def test_ten_columns_in_two_chains(gpu_lib):
    """Four reactions: all ten parameters in one call (an M = 8 chain and an M = 2 chain); every column has the bits of its n = 1
    call and of gmpnp_linear_solve, and n = 11 is refused."""
    from gmpnp_amd.params import edl_parameters
    import hp_reference as H
    ep = edl_parameters(cation="Cs", voltage_multiplier=-10.0)
    prob = R.with_inv_dt(edl_problem(ep, H.uniform_mesh_1d(65), stern=SternLayer("BDM", P_M, L_STERN / ep.L_n), kinetics=four_reactions(ep.species, P_M)), 0.0)
    u = random_state(65, 6, seed=65)[0]
    ten = (0, 16, 17, 18, 19, 32, 33, 34, 35, 48)
    with gpu_lib.DeviceSolver(prob) as dev:
        dev.set_state(u, u)
        t = dev.electrode_tangent(ten, want_z=True)
        c = dev.tangent_columns(10)
        assert not t["status"].any() and t["dI"].shape == (10, 4)
        for k, p in enumerate(ten):
            one = dev.electrode_tangent([p], want_z=True)
            assert same_bits(t, one, k, 0), p
        dev.assemble(True)
        for k in (0, 7, 8, 9):
            assert np.array_equal(dev.linear_solve(-c[k], gpu_lib.LINEAR_BLOCK_TRIDIAGONAL)[0], t["z"][k])
        with pytest.raises(gpu_lib.GmpnpError, match="electrode tangent"):
            dev.electrode_tangent(ten + (0,))


def test_tangent_against_differences_of_two_device_steady_states(inputs, gpu_lib):
    """dD and dI_r of the p_M column at the device's own steady state against central differences of stern_displacement and
    kinetics_currents between two device steady states at p_M -+ 1e-3: 1e-6."""
    prob, states = inputs["edl1"]
    u = states[0][0]
    d = 1e-3
    opts = gpu_lib.newton_options(STEADY, dim=1)
    D, I = {}, {}
    with gpu_lib.DeviceSolver(R.with_inv_dt(prob, 0.0)) as dev:
        for s in (+1, -1, 0):
            q = R.with_potential(prob, P_M + s * d)
            dev.set_stern(q.stern)
            dev.set_kinetics(q.kinetics)
            dev.set_state(u, u)
            assert dev.newton_solve(opts)["converged"]
            D[s], I[s] = dev.stern_displacement(), dev.kinetics_currents()
        t = dev.electrode_tangent([0])
    fD, fI = (D[1] - D[-1]) / (2 * d), (I[1] - I[-1]) / (2 * d)
    eD, eI = abs(t["dD"][0] - fD) / abs(fD), np.abs(t["dI"][0] - fI).max() / np.abs(fI).max()
    print("device steady differences: dD %.10g (%.10g, %.2e), dI %s (%s, %.2e)" % (t["dD"][0], fD, eD, t["dI"][0], fI, eI))
    assert eD < 1e-6 and eI < 1e-6 and t["status"][0] == 0


def test_the_handle_after_a_call(edl_k, gpu_lib):
    """After a call u and u_n are untouched, F and jacobian_csr are those of gmpnp_assemble(want_jacobian = 1) on a twin, and the
    next newton_solve gives the twin's bits, with and without a Jacobian before the call."""
    ep, mesh = edl_k
    prob = first_step_problem(ep, mesh, P_M)
    u0, un = first_step_state(prob)
    u0 = un + 1e-3 * np.random.default_rng(5).standard_normal(prob.ndof) * (np.arange(prob.ndof) % prob.nf != prob.nf - 1)
    opts = gpu_lib.newton_options({"newton_solver": {"maximum_iterations": 50, "relative_tolerance": 1e-9, "absolute_tolerance": 1e-6}}, dim=1)
    with gpu_lib.DeviceSolver(prob) as a, gpu_lib.DeviceSolver(prob) as twin, gpu_lib.DeviceSolver(prob) as c:
        for dev in (a, twin, c):
            dev.set_state(u0, un)
        a.assemble(True)
        Ft = twin.assemble(True)[0]
        res = a.electrode_tangent(PARAMS)
        assert not res["status"].any()
        assert np.array_equal(a.get_state(), u0) and np.array_equal(a.jacobian_csr().data, twin.jacobian_csr().data)
        assert np.array_equal(a.assemble(False)[0], Ft)
        sa, st = a.newton_solve(opts), twin.newton_solve(opts)
        assert sa["converged"] and sa["iterations"] == st["iterations"] > 0 and sa["residuals"] == st["residuals"]
        assert np.array_equal(a.get_state(), twin.get_state())
        c.electrode_tangent([0, 48])
        assert c.jacobian_csr().nnz > 0                                  # the call leaves a valid Jacobian, as gmpnp_assemble does
        sc = c.newton_solve(opts)
        assert sc["iterations"] == st["iterations"] and sc["residuals"] == st["residuals"] and np.array_equal(c.get_state(), twin.get_state())


def test_advance(inputs, gpu_lib):
    """u + alpha dp z and both p_electrode values bit for bit; tau = 0.9 reproduces gmpnp_step_limit's alpha for the direction
    -dp z; the advance is refused without a tangent, after set_state, after a Newton solve, after a second advance and where the
    call held no p_M column; F after the advance is that of a twin set to the same state and potential."""
    prob, states = inputs["edl1"]
    u = states[0][0]
    q = R.with_inv_dt(prob, 0.0)

    def refused(call):
        with pytest.raises(gpu_lib.GmpnpError, match="electrode tangent") as ei:
            call()
        assert ei.value.code == gpu_lib.ERR_INVALID

    with gpu_lib.DeviceSolver(q) as dev, gpu_lib.DeviceSolver(q) as twin:
        dev.set_state(u, u)
        refused(lambda: dev.electrode_advance(-1.0))                     # no tangent yet
        z = dev.electrode_tangent([48, 0], want_z=True)["z"][1]
        dp = -0.75
        assert dev.electrode_advance(dp) == 1.0
        u1 = dev.get_state()
        assert u1.tobytes() == (u + 1.0 * dp * z).tobytes()
        refused(lambda: dev.electrode_advance(dp))                       # used up
        p1 = P_M + dp
        q1 = R.with_potential(q, p1)
        twin.set_stern(q1.stern)
        twin.set_kinetics(q1.kinetics)
        twin.set_state(u1, u)
        assert np.array_equal(dev.assemble(True)[0], twin.assemble(True)[0]) and np.array_equal(dev.jacobian_csr().data, twin.jacobian_csr().data)
        # damped: a step that would leave the admissible set
        big = -40.0
        z1 = dev.electrode_tangent([0], want_z=True)["z"][0]
        alpha_ref, lam, node = dev.step_limit(-(big * z1), 0.9)
        dev.electrode_tangent([0])
        alpha = dev.electrode_advance(big, 0.9)
        print("advance by %g with tau 0.9: alpha %.6g (lambda %.6g at vertex %d)" % (big, alpha, lam, node))
        assert alpha == alpha_ref and alpha < 1.0
        assert dev.get_state().tobytes() == (u1 + alpha * big * z1).tobytes()
        # what invalidates the tangent
        dev.set_stern(q.stern)
        dev.set_kinetics(q.kinetics)
        dev.set_state(u, u)
        dev.electrode_tangent([0])
        dev.set_state(u, None)
        refused(lambda: dev.electrode_advance(dp))
        dev.electrode_tangent([0])
        dev.newton_solve(gpu_lib.newton_options(STEADY, dim=1))
        refused(lambda: dev.electrode_advance(dp))
        dev.electrode_tangent([0])
        dev.set_kinetics(q.kinetics)
        refused(lambda: dev.electrode_advance(dp))
        dev.electrode_tangent([48])
        refused(lambda: dev.electrode_advance(dp))                       # no p_M column in the last call
        dev.electrode_tangent([0])
        refused(lambda: dev.electrode_advance(float("nan")))
        refused(lambda: dev.electrode_advance(dp, 1.5))
        assert dev.electrode_advance(dp) == 1.0


def test_library_refusals_and_hook_28(pore10, edl_k, gpu_lib):
    """Every refusal is GMPNP_ERR_INVALID and names the electrode tangent: a partition handle, a multilevel level, a 3D handle, SUPG
    terms, the Stern option off, the galvanostat on, two electrode potentials, a kinetic column with the kinetics off or with
    r >= n_reactions, n = 0 and 11, a repeated and an unknown parameter.  Hook 28 needs a call first, then times the chain and leaves
    the state and the Jacobian alone."""
    from gmpnp_amd import dist
    from gmpnp_amd.problem import pore_hierarchy
    from gmpnp_amd.solver import GMPNPSystem
    pp, mesh, prob3, _ = pore10
    ep, m1 = edl_k

    def refused(call, what="electrode tangent"):
        with pytest.raises(gpu_lib.GmpnpError, match=what) as ei:
            call()
        assert ei.value.code == gpu_lib.ERR_INVALID

    dom, perm, part = dist.partition_plan(prob3, 2, 0)
    with gpu_lib.DeviceSolver(dom.problem, perm=perm, partition=part) as partitioned:
        refused(lambda: partitioned.electrode_tangent([0]))
        refused(lambda: partitioned.electrode_advance(-1.0))
    levels = pore_hierarchy(pp, mesh, 1)
    ml = GMPNPSystem(levels[0][0], levels=levels)
    try:
        refused(lambda: ml.dev.electrode_tangent([0]))
        refused(lambda: ml._coarse[0].electrode_tangent([0]))
    finally:
        ml.close()
    with gpu_lib.DeviceSolver(prob3) as d3:
        refused(lambda: d3.electrode_tangent([0]))                        # 3D, the Stern option off
    import hp_reference as H
    from gmpnp_amd.params import edl_parameters
    epg = edl_parameters(cation="Cs", voltage_multiplier=-10.0)
    shuffled = edl_problem(epg, H.uniform_mesh_1d(9), stern=SternLayer("BDM", P_M, L_STERN / epg.L_n))
    with gpu_lib.DeviceSolver(shuffled, perm=np.array([3, 0, 7, 1, 8, 2, 5, 4, 6], dtype=np.int32)) as dperm:
        refused(lambda: dperm.electrode_tangent([0]), "block-tridiagonal")   # the internal order is not the path order
    kin = two_reactions(ep.species, P_M)
    plain = edl_problem(ep, m1)
    both = edl_problem(ep, m1, stern=SternLayer("BDM", P_M, L_STERN / ep.L_n), kinetics=kin)
    stern_only = edl_problem(ep, m1, stern=SternLayer("BDM", P_M, L_STERN / ep.L_n))
    with gpu_lib.DeviceSolver(plain) as a, gpu_lib.DeviceSolver(both) as b, gpu_lib.DeviceSolver(stern_only) as c:
        u0, un = first_step_state(plain)
        for d in (a, b, c):
            d.set_state(un, un)
        refused(lambda: a.electrode_tangent([0]))                         # the Stern option is off
        b.assemble(True)
        refused(lambda: b.time_kernel(28, 1))                             # no call yet
        refused(lambda: b.tangent_columns(1))
        c.set_supg(np.full((m1.num_vertices, 6), 0.1))
        refused(lambda: c.electrode_tangent([0]))
        c.set_supg(None)
        only = c.electrode_tangent([0, 48])
        assert not only["status"].any() and only["dI"].shape == (2, 0)   # the Stern option alone: no currents
        refused(lambda: c.electrode_tangent([0, 16]))                     # a kinetic column with the kinetics off
        refused(lambda: b.electrode_tangent([0, 18]))                     # r >= n_reactions
        refused(lambda: b.electrode_tangent([]))
        refused(lambda: b.electrode_tangent(list(PARAMS) + [0, 16, 17, 32, 33]))
        refused(lambda: b.electrode_tangent([0, 48, 0]))
        for bad in (1, 15, 20, 36, 47, 49, -1):
            refused(lambda: b.electrode_tangent([0, bad]))
        before = b.electrode_tangent(PARAMS, want_z=True)
        b.set_galvanostat(Galvanostat(10.0))
        refused(lambda: b.electrode_tangent([0]))
        b.set_galvanostat(None)
        b.set_stern(SternLayer("BDM", P_M + 1.0, L_STERN / ep.L_n))
        refused(lambda: b.electrode_tangent([0]))                         # two electrode potentials
        b.set_stern(SternLayer("BDM", P_M, L_STERN / ep.L_n))
        assert same_bits(b.electrode_tangent(PARAMS, want_z=True), before)
        F0 = b.assemble(True)[0]
        b.electrode_tangent(PARAMS)
        J0 = b.jacobian_csr().data.copy()
        u_before = b.get_state()
        assert b.time_kernel(28, 2) > 0.0
        assert np.array_equal(b.get_state(), u_before) and np.array_equal(b.jacobian_csr().data, J0) and np.array_equal(b.assemble(False)[0], F0)
        assert same_bits(b.electrode_tangent(PARAMS, want_z=True), before)


# ---- the driver ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def curve(tmp_path_factory, gpu_lib):
    """EDLRun on the 1 um mesh to its steady stop at p_M = -5, then: the curve to -10 in steps of -1 written by write_outputs, the
    same curve with the predictor off, and independent steady solves at the grid potentials from the run's own steady state."""
    from gmpnp_amd import edl1d
    out_dir = tmp_path_factory.mktemp("polarisation")
    os.environ["GMPNP_OUT"] = str(out_dir)
    kw = dict(L_n=1e-6, cation="K", electrode_voltage=P_M, kinetics="tafel", i0_CO=TAFEL["i0_CO"], i0_H2=TAFEL["i0_H2"], adaptive_dt=True, steady_tol=1e-5)
    try:
        run = edl1d.EDLRun(polarisation=dict(v_end=-10.0, v_step=-1.0, params=(0, 16, 17, 48)), **kw)
        try:
            run.run(verbose=False)
            dev = run.sys.dev
            u_start = dev.get_state()
            opts = gpu_lib.newton_options(edl1d.POLARISATION_NEWTON, dim=1)
            path = run.write_outputs(stamp="curve")
            u_end = dev.get_state()
            # independent steady solves, each from the run's own steady state at -5
            dev.set_time_step(0.0)
            independent = []
            for p in (-5.0, -6.0, -7.0, -8.0, -9.0, -10.0):
                q = R.with_potential(run.problem, p)
                dev.set_stern(q.stern)
                dev.set_kinetics(q.kinetics)
                dev.set_state(u_start, u_start)
                assert dev.newton_solve(opts)["converged"]
                independent.append((dev.get_state(), dev.kinetics_currents(), dev.stern_displacement()))
        finally:
            run.sys.close()
        plain = edl1d.EDLRun(**kw)
        try:
            plain.run(verbose=False)
            off = plain.polarisation(-10.0, -1.0, predictor=False)
            planted = plain.polarisation(-30.0, -20.0)
            with pytest.raises(ValueError, match="polarisation"):
                plain.polarisation(-10.0, -1.0)                       # the run stands at -30 now: the wrong direction
        finally:
            plain.sys.close()
    finally:
        del os.environ["GMPNP_OUT"]
    return dict(path=path, u_end=u_end, independent=independent, off=off, planted=planted, ep=run.ep)


def test_driver_curve_against_independent_steady_solves(curve):
    """Every point of the curve against an independent steady solve at that potential: the currents and the displacement to 1e-8,
    the last state too."""
    z = np.load(os.path.join(curve["path"], "polarisation.npz"))
    assert np.array_equal(z["electrode_voltage"], [-5.0, -6.0, -7.0, -8.0, -9.0, -10.0]) and z["substeps"].tolist() == [0, 1, 1, 1, 1, 1]
    from gmpnp_amd.params import _load_yaml, utilities_dir
    eps_0 = _load_yaml(os.path.join(utilities_dir(), "parameters.yaml"))["nat_const"]["eps_0"]
    ep = curve["ep"]
    for k, (u, I, D) in enumerate(curve["independent"]):
        eI = max(abs(z["i_CO"][k] - I[0]) / I[0], abs(z["i_H2"][k] - I[1]) / I[1])
        eD = abs(z["surface_charge"][k] - eps_0 * ep.thermal_voltage / ep.L_n * D) / abs(z["surface_charge"][k])
        eP = abs(z["potential_OHP"][k] - u[6] * ep.thermal_voltage) / abs(z["potential_OHP"][k])
        print("point %d: currents %.2e, surface charge %.2e, OHP potential %.2e" % (k, eI, eD, eP))
        assert eI <= 1e-8 and eD <= 1e-8 and eP <= 1e-8
    u_ind = curve["independent"][-1][0]
    assert np.abs(curve["u_end"] - u_ind).max() <= 1e-8 * np.abs(u_ind).max()


def test_driver_outputs_and_units(curve):
    """polarisation.npz: its keys, shapes and units; the metadata keys; the predictor saves Newton iterations."""
    z = np.load(os.path.join(curve["path"], "polarisation.npz"))
    keys = ["electrode_voltage", "electrode_voltage_V", "potential_OHP", "i_CO", "i_H2", "FE_H2", "surface_charge", "capacitance", "dI_dV", "tafel_slope",
            "sensitivity", "sensitivity_params", "newton_iterations", "substeps", "tangent_residual", "sechenov_rounds"]
    assert sorted(z.files) == sorted(keys)
    ep = curve["ep"]
    n = 6
    assert all(z[k].shape == (n,) for k in keys if k not in ("dI_dV", "tafel_slope", "sensitivity", "sensitivity_params"))
    assert z["dI_dV"].shape == (n, 2) and z["tafel_slope"].shape == (n, 2) and z["sensitivity"].shape == (n, 4, 4) and list(z["sensitivity_params"]) == [0, 16, 17, 48]
    assert np.array_equal(z["electrode_voltage_V"], z["electrode_voltage"] * ep.thermal_voltage)
    assert np.allclose(z["FE_H2"], z["i_H2"] / (z["i_CO"] + z["i_H2"]), rtol=1e-15)
    assert np.all(z["i_CO"] > 0.0) and np.all(np.diff(z["i_CO"]) > 0.0) and np.all(z["surface_charge"] < 0.0) and np.all(z["capacitance"] > 0.0)
    assert np.all(z["dI_dV"] < 0.0)                                   # cathodic currents grow as the potential falls
    I = np.stack([z["i_CO"], z["i_H2"]], axis=1)
    assert np.allclose(z["tafel_slope"], np.log(10.0) / (z["dI_dV"] / I), rtol=1e-14)
    assert np.all((z["tafel_slope"] < -0.1) & (z["tafel_slope"] > -0.4))     # alpha = 0.5: -118 mV/decade across the Stern layer, more at the electrode
    assert np.array_equal(z["sensitivity"][:, 0, 1:3] / ep.thermal_voltage, z["dI_dV"]) and z["tangent_residual"].max() < 1e-10
    # a larger rate constant raises its own current, by less than the current itself where the reactant is depleted
    print("d i_CO / d ln k_0 over i_CO:", (z["sensitivity"][:, 1, 1] / z["i_CO"]).tolist(), " d i_H2 / d ln k_1 over i_H2:", (z["sensitivity"][:, 2, 2] / z["i_H2"]).tolist())
    assert np.all(z["sensitivity"][:, 1, 1] > 0.0) and np.all(z["sensitivity"][:, 1, 1] < z["i_CO"]) and np.all(z["sensitivity"][:, 2, 2] > 0.0)
    # capacitance against the difference quotient of the surface charge along the curve (second order in the 1-unit step)
    fd = (z["surface_charge"][2:] - z["surface_charge"][:-2]) / (z["electrode_voltage_V"][2:] - z["electrode_voltage_V"][:-2])
    assert np.abs(fd - z["capacitance"][1:-1]).max() <= 0.02 * z["capacitance"].max()
    meta = json.load(open(os.path.join(curve["path"], "metadata.json")))
    assert meta["polarisation_points"] == n and meta["polarisation_stop_reason"] == "v_end" and meta["polarisation_params"] == [0, 16, 17, 48]
    assert meta["polarisation_newton_iterations"] == int(z["newton_iterations"].sum()) and meta["polarisation_substeps"] == 5
    assert (meta["polarisation_v_end"], meta["polarisation_v_step"]) == (-10.0, -1.0) and meta["electrode_voltage"] == P_M
    off = curve["off"]
    print("Newton iterations with the predictor %s, without %s" % (z["newton_iterations"].tolist(), off["newton_iterations"].tolist()))
    assert np.array_equal(off["electrode_voltage"], z["electrode_voltage"]) and z["newton_iterations"][1:].sum() <= off["newton_iterations"][1:].sum()
    assert np.abs(off["i_CO"] - z["i_CO"]).max() <= 1e-8 * z["i_CO"].max()


def test_driver_halves_a_step_that_fails(curve):
    """A planted failure, -10 to -30 in one step of -20: the step is halved, the curve still lands on -30 and the currents are
    positive (the spurious branch with a negative reactant is not accepted)."""
    p = curve["planted"]
    print("planted failure: substeps %s, Newton iterations %s" % (p["substeps"].tolist(), p["newton_iterations"].tolist()))
    assert p["stop_reason"] == "v_end" and np.array_equal(p["electrode_voltage"], [-10.0, -30.0]) and p["substeps"][1] > 1
    assert np.all(p["i_CO"] > 0.0) and np.all(p["i_H2"] > 0.0)


# ---- 3D: the library call on L_10_R_5 at the handle's own inv_dt > 0, and the driver ------------------------------------------------------
PORE_TAFEL = dict(kinetics="tafel", i0_CO=10.0, i0_H2=1.0)   # test_gpu_kinetics.py's
PORE_NEWTON = {"newton_solver": {"linear_solver": "band_lu", "maximum_iterations": 25, "relative_tolerance": 1e-13, "absolute_tolerance": 1e-9}}


@pytest.fixture(scope="module")
def pore_case(gpu_lib):
    """Two PoreRun steps on L_10_R_5 (band LU, p_M = -1, Tafel kinetics), then a third step's Newton solve from that u_n to the
    rounding floor, not accepted: the tangent of that implicit step with u_n frozen, and the same step solved at p_M -+ 1e-3."""
    from gmpnp_amd.pore3d import SOLVER_PARAMETERS, PoreRun
    sp = {"nonlinear_solver": "newton", "newton_solver": dict(SOLVER_PARAMETERS["newton_solver"], linear_solver="band_lu")}
    run = PoreRun(num_steps=2, solver_parameters=sp, electrode_voltage=-1.0, L=10e-9, R=5e-9, concentration_elec=0.5, **PORE_TAFEL)
    try:
        run.run(verbose=False)
        dev = run.sys.dev
        # to the rounding floor: eight iterations with tolerances that are never met (the quotient of two states stopped at a
        # residual tolerance carries that tolerance times |J^-1| over 2 delta, which is not the tangent's error)
        floor = gpu_lib.newton_options({"newton_solver": dict(PORE_NEWTON["newton_solver"], maximum_iterations=8, relative_tolerance=1e-30, absolute_tolerance=1e-30)}, dim=3)
        assert dev.newton_solve(floor, error_on_nonconvergence=False)["iterations"] == 8
        u = dev.get_state()
        six = dev.electrode_tangent(PARAMS, want_z=True)
        c = dev.tangent_columns(len(PARAMS))
        J = dev.jacobian_csr()
        again = dev.electrode_tangent(PARAMS, want_z=True)
        one = dev.electrode_tangent([0], want_z=True)
        d, D, I, U = 1e-3, {}, {}, {}
        for sgn in (+1, -1, +2, -2):
            q = R.with_potential(run.problem, -1.0 + sgn * d)
            dev.set_stern(q.stern)
            dev.set_kinetics(q.kinetics)
            dev.set_state(u, None)
            assert dev.newton_solve(floor, error_on_nonconvergence=False)["iterations"] == 8
            D[sgn], I[sgn], U[sgn] = dev.stern_displacement(), dev.kinetics_currents(), dev.get_state()
        dev.set_stern(run.problem.stern)
        dev.set_kinetics(run.problem.kinetics)
        dev.set_state(u, None)
        dev.set_galvanostat(Galvanostat(1.0))
        b = dev.galvanostat_terms()[0]
        dev.set_galvanostat(None)
        # the advance on a 3D handle
        z0 = dev.electrode_tangent([0], want_z=True)["z"][0]
        alpha = dev.electrode_advance(-0.25)
        u_adv = dev.get_state()
        prob = copy.copy(run.problem)
    finally:
        run.sys.close()
    return dict(prob=prob, u=u, six=six, c=c, J=J, again=again, one=one, d=d, D=D, I=I, U=U, b=b, z0=z0, alpha=alpha, u_adv=u_adv)


def test_3d_tangents_against_splu(pore_case):
    """Every z_k of the band LU (one factorisation, six refined substitutions) against splu on the device's own jacobian_csr.  Both
    are measured against the extended-precision refinement of splu's solution: the device's forward error is at most 10x splu's own
    (floor 1e-13: two correct solvers differ by their conditioning), its residual max |J z + c| / max |c| at most 10x splu's (floor
    1e-14), and the reported residual is the extended-precision one within the rounding of its fp64 evaluation.  The p_M column is
    gmpnp_galvanostat_terms' b bit for bit; two calls and n = 1 give equal bits."""
    import galvanostat_reference as GR
    d = pore_case
    six, c, J = d["six"], d["c"], d["J"]
    assert not six["status"].any() and c[0].tobytes() == d["b"].tobytes()
    assert same_bits(six, d["again"]) and same_bits(six, d["one"], 0, 0)
    A = J.tocsc()
    lu = spla.splu(A)
    bc = np.asarray(d["prob"].bc_dofs, dtype=np.int64)
    for k, p in enumerate(PARAMS):
        assert np.abs(c[k]).max() > 0.0 and not c[k][bc].any()
        xs = lu.solve(-c[k])
        xr = np.asarray(GR.refined_solve(A, lu, -c[k]), dtype=np.float64)
        e_dev, e_splu = float(np.abs(six["z"][k] - xr).max() / np.abs(xr).max()), float(np.abs(xs - xr).max() / np.abs(xr).max())
        res, rounding = rel_residual(J, six["z"][k], c[k])
        res_splu = rel_residual(J, xs, c[k])[0]
        print("3D param %d: z against the refined solution %.2e (splu %.2e), residual %.2e (splu %.2e, reported %.2e)" % (p, e_dev, e_splu, res, res_splu, six["residual"][k]))
        assert e_dev <= 10.0 * max(e_splu, 1e-13) and res <= 10.0 * max(res_splu, 1e-14)
        assert abs(six["residual"][k] - res) <= rounding


def test_3d_functionals_against_the_numpy_rule(pore_case):
    """dD, dI_r and dp_boundary against the NumPy rule applied facet by facet to the device's own z (tangent_reference.functionals):
    1e-12 relative plus the rounding of a sum of a few thousand terms taken in another order, 64 eps of the sum of their absolute
    values (the ln k and alpha columns of dD are small differences of large facet terms)."""
    d = pore_case
    eps = np.finfo(float).eps
    for k, p in enumerate(PARAMS):
        fD, fI, fp, aD, aI = T.functionals(d["prob"], d["u"], d["six"]["z"][k], p, want_scale=True)
        print("3D param %d: dD %.6e (rule %.6e), dI %s (rule %s), dp %.6e (%.6e)" % (p, d["six"]["dD"][k], fD, d["six"]["dI"][k], fI, d["six"]["dp_boundary"][k], fp))
        assert abs(d["six"]["dD"][k] - fD) <= 1e-12 * abs(fD) + 64 * eps * aD, p
        assert np.all(np.abs(d["six"]["dI"][k] - fI) <= 1e-12 * np.abs(fI) + 64 * eps * aI), p
        assert abs(d["six"]["dp_boundary"][k] - fp) <= 1e-12 * abs(fp) + 64 * eps * np.abs(d["six"]["z"][k]).max(), p


def test_3d_p_M_tangent_against_differences_of_two_one_step_solves(pore_case):
    """z, dD and dI_r of the p_M column against central differences of two solves of the same implicit step (same u_n) at
    p_M -+ 1e-3: 1e-6 relative (truncation O(delta^2), as in 1D).  And the advance: u + alpha dp z bit for bit."""
    d = pore_case
    h = d["d"]
    fD, fI = (d["D"][1] - d["D"][-1]) / (2 * h), (d["I"][1] - d["I"][-1]) / (2 * h)
    # the state's quotient is extrapolated from delta and 2 delta: the divalent ions at the wall go like exp(2 p), so the plain
    # quotient's own truncation (delta^2 / 6 times the third derivative, ~1.3e-6 of the first) is above the bound; the
    # extrapolated quotient's is O(delta^4)
    fz = (4.0 * (d["U"][1] - d["U"][-1]) / (2 * h) - (d["U"][2] - d["U"][-2]) / (4 * h)) / 3.0
    ez = float(np.abs(fz - d["six"]["z"][0]).max() / np.abs(fz).max())
    eD = abs(fD - d["six"]["dD"][0]) / abs(fD)
    eI = float(np.abs(fI - d["six"]["dI"][0]).max() / np.abs(fI).max())
    print("3D one-step differences: z %.2e, dD %.10g (%.10g, %.2e), dI %s (%s, %.2e)" % (ez, d["six"]["dD"][0], fD, eD, d["six"]["dI"][0], fI, eI))
    assert ez < 1e-6 and eD < 1e-6 and eI < 1e-6
    assert d["alpha"] == 1.0 and d["u_adv"].tobytes() == (d["u"] + 1.0 * -0.25 * d["z0"]).tobytes()


def test_3d_driver_three_points(tmp_path, monkeypatch, gpu_lib):
    """PoreRun on L_10_R_5 from its adaptive steady stop at p_M = -1: the curve to -1.5 in steps of -0.25 through write_outputs;
    wall means, the Sechenov rounds recorded, every point against an independent steady solve with the same Dirichlet value."""
    from gmpnp_amd.pore3d import SOLVER_PARAMETERS, PoreRun
    monkeypatch.setenv("GMPNP_OUT", str(tmp_path))
    sp = {"nonlinear_solver": "newton", "newton_solver": dict(SOLVER_PARAMETERS["newton_solver"], linear_solver="band_lu")}
    run = PoreRun(solver_parameters=sp, electrode_voltage=-1.0, L=10e-9, R=5e-9, concentration_elec=0.5, adaptive_dt=True, steady_tol=1e-5,
                  polarisation=dict(v_end=-1.5, v_step=-0.25, params=(0, 48)), **PORE_TAFEL)
    try:
        run.run(verbose=False)
        path = run.write_outputs(stamp="curve3d")
        dev = run.sys.dev
        u_end, I_end = dev.get_state(), dev.kinetics_currents()
        dev.set_time_step(0.0)
        dev.set_state(u_end + 1e-3 * np.abs(u_end) * np.random.default_rng(3).standard_normal(u_end.size) * (np.arange(u_end.size) % 9 != 8), None)
        assert dev.newton_solve(gpu_lib.newton_options(PORE_NEWTON, dim=3))["converged"]
        I_ind = dev.kinetics_currents()
        area = run.wall_area()
    finally:
        run.sys.close()
    z = np.load(os.path.join(path, "polarisation.npz"))
    meta = json.load(open(os.path.join(path, "metadata.json")))
    print("3D curve: newton %s substeps %s sechenov rounds %s i_CO %s capacitance %s" % (z["newton_iterations"].tolist(), z["substeps"].tolist(),
          z["sechenov_rounds"].tolist(), z["i_CO"].tolist(), z["capacitance"].tolist()))
    assert np.array_equal(z["electrode_voltage"], [-1.0, -1.25, -1.5]) and meta["polarisation_stop_reason"] == "v_end" and meta["polarisation_points"] == 3
    assert np.all(z["sechenov_rounds"] >= 1) and np.all(z["sechenov_rounds"] <= 10) and meta["polarisation_sechenov_rounds"] == int(z["sechenov_rounds"].max())
    assert np.all(z["i_CO"] > 0.0) and np.all(np.diff(z["i_CO"]) > 0.0) and np.all(z["capacitance"] > 0.0) and z["tangent_residual"].max() < 1e-8
    assert abs(z["i_CO"][-1] - I_end[0] / area) <= 1e-14 * z["i_CO"][-1]
    assert np.abs(I_ind - I_end).max() <= 1e-8 * np.abs(I_end).max()
