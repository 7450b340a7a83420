"""The BiCGStab preconditioners on the GPU against the restatement of M^-1 in tests/precond_reference.py: every other GPU test sees
the preconditioner through outcomes a wrong (but nonsingular) one also produces.  Here the first iterations of
gmpnp_linear_solve are compared with the model's BiCGStab on the DEVICE's matrix (required equal to the oracle's first):

(a) capped history: max_iterations = k ends the solve with ERR_LINEAR, and the statistics on the exception report k iterations
    and the TRUE residual ||b - J x_k||, which must equal the model's within tol_k;
(b) vectors: a loose rtol_k between two residuals of the history makes the solve stop after exactly k iterations ("rungs") and
    return x_k = M^-1 y_k, which must equal the model's within tol_k (max norm);
(c) the four-launch form is bitwise equal to the default wherever test_gpu_shapes.py asserts that; the materialised vector form
    (vector_form=1: k_vec_a / k_bicg_a_mat) and a shared device meet (a) and (b) on their own.

tol_k = max(1e-12, 100 d_k) with d_k the model's own sensitivity to rounding (test_precond_reference.py); steps with tol_k > 1e-6
are not compared (cyl3_9 in the two-level mode keeps none or one: precond_reference.ROUNDING_LIMITED).  Every test prints the worst device-to-model distance it saw, in units of tol_k and as a relative error.
Cases, seeds and right-hand sides: precond_reference.CASES_3D / CASES_1D / case_state / case_rhs.
"""
import numpy as np
import pytest

import hp_reference as H
import precond_reference as R

pytestmark = pytest.mark.gpu

FORMS = (dict(), dict(launch_form=4), dict(vector_form=1), dict(shared_device=1))


def _modes(gpu_lib):
    return (("two-level", gpu_lib.LINEAR_TWOLEVEL), ("jacobi", gpu_lib.LINEAR_JACOBI))


def _observe(gpu_lib, dev, b, mode, ob, what, conditions=True):
    """Checks (a) and (b) of one handle and mode against the model's observables; returns ({k: x of the rung k}, worst distance in
    units of the tolerance, worst relative distance).  ``conditions`` = False (precond_reference.ROUNDING_LIMITED): whatever steps
    keep a tolerance below 1e-6 are compared, none is required."""
    assert ob.meets_conditions() or not conditions, (what, ob.d_res, ob.d_x, ob.rel)
    worst, worst_rel = 0.0, 0.0
    for k in ob.capped:
        with pytest.raises(gpu_lib.GmpnpError) as e:
            dev.linear_solve(b, mode, 1e-300, 0.0, k)
        st = e.value.stats
        assert e.value.code == gpu_lib.ERR_LINEAR and st is not None and not st["converged"], (what, k)
        assert st["iterations"] == k, (what, k, st)
        rel = abs(st["residual_norm"] - ob.true[k]) / ob.true[k]
        worst, worst_rel = max(worst, rel / ob.tol_res[k]), max(worst_rel, rel)
        print(what, "capped k=%d: |device - model| / model = %.3g, tol %.3g" % (k, rel, ob.tol_res[k]))
        assert rel <= ob.tol_res[k], (what, "capped", k, rel, ob.tol_res[k], st["residual_norm"], ob.true[k])
    xs = {}
    for k, rtol in ob.rungs:
        x, st = dev.linear_solve(b, mode, rtol, 0.0, 100)
        assert st["converged"] and st["iterations"] == k, (what, k, rtol, st, ob.rel)
        rel = H.max_rel(x, ob.xs[k])
        worst, worst_rel = max(worst, rel / ob.tol_x[k]), max(worst_rel, rel)
        print(what, "rung k=%d (rtol %.3g): max_rel(x, x_k) = %.3g, tol %.3g" % (k, rtol, rel, ob.tol_x[k]))
        assert rel <= ob.tol_x[k], (what, "rung", k, rel, ob.tol_x[k])
        xs[k] = x
    return xs, worst, worst_rel


def _flat_case(gpu_lib, case, prob, requested, dim):
    nv, nf = prob.coords.shape[0], prob.nf
    u, un = R.case_state(case, prob)
    out, model, report = {}, {}, {}
    for opts in FORMS:
        key = tuple(opts.items())
        with gpu_lib.DeviceSolver(prob, n_aggregates=requested, **opts) as dev:
            dev.set_state(u, un)
            if not opts:
                nagg = dev.n_aggregates
                assert nagg == R.aggregate_count(dev.perm, prob.cells, nv, nf, requested), case
                Fo, A = R.assembly_matches(dev, prob, u, un)
                b = R.case_rhs(case, Fo, A)
                agg = R.aggregates(dev.perm, nv, nagg)
                model = {"two-level": R.Observables(A, R.two_level_factory(A, nf, agg), b),
                         "jacobi": R.Observables(A, R.jacobi_factory(A, nf), b)}
                default_launches = dev.krylov_launches_per_iteration
            else:
                assert dev.n_aggregates == nagg
                dev.assemble(True)
            if key == (("launch_form", 4),):
                assert dev.krylov_launches_per_iteration == 4
            for mname, mode in _modes(gpu_lib):
                xs, worst, worst_rel = _observe(gpu_lib, dev, b, mode, model[mname], (case, requested, key, mname),
                                                conditions=(case, mname) not in R.ROUNDING_LIMITED)
                out[(key, mname)] = xs
                report[(key, mname)] = (worst, worst_rel)
    print("%s n_aggregates=%d (granted %d): worst distance / tol_k %.3g, worst relative distance %.3g" %
          (case, requested, nagg, max(v[0] for v in report.values()), max(v[1] for v in report.values())))
    if dim == 1 or default_launches == 2:      # (c): what test_gpu_shapes.py asserts of the solutions at 1e-10, here of every x_k
        for mname, _ in _modes(gpu_lib):
            ref, four = out[((), mname)], out[((("launch_form", 4),), mname)]
            assert ref.keys() == four.keys() and all(np.array_equal(ref[k], four[k]) for k in ref), (case, mname)
    return nagg


@pytest.mark.parametrize("case,requested", R.CASES_3D)
def test_preconditioner_3d(case, requested, gpu_lib):
    """NF = 9: one aggregate (cyl1_1), four (box2_3: ncoarse = 36), eight with partial slices and nv mod 7 != 0 (box4_12, box5_17),
    the most the LDS-resident inverse takes (box5_17 with a request of 16: 15 are granted, kMaxCoarse = 140 bounds ncoarse at
    135) and the reference mesh (more than one tile per aggregate)."""
    nagg = _flat_case(gpu_lib, case, R.problem_3d(case), requested, 3)
    expect = {("cyl1_1", 0): 1, ("box2_3", 0): 4, ("box4_12", 0): 8, ("box5_17", 0): 8, ("box5_17", 16): 15, ("pore10", 0): 8}
    assert nagg == expect.get((case, requested), nagg)


@pytest.mark.parametrize("nv,requested", R.CASES_1D)
def test_preconditioner_1d(nv, requested, gpu_lib):
    """NF = 7 (SELL slices of 9 rows) with the default, one and the most aggregates."""
    nagg = _flat_case(gpu_lib, "1d%d" % nv, R.problem_1d(nv), requested, 1)
    assert nagg == max(1, min({0: 8, 1: 1, 16: 16}[requested], nv // 8))


@pytest.fixture(scope="module")
def hierarchies():
    cache = {}

    def get(refine):
        if refine not in cache:
            cache[refine] = R.cylinder_hierarchy(refine)
        return cache[refine]
    return get


@pytest.mark.parametrize("refine", [1, 2])
def test_preconditioner_multilevel(refine, hierarchies, gpu_lib):
    """The geometric multilevel term on a two- and a THREE-level hierarchy of the generated 114-vertex cylinder (671 and 4,557
    vertices on top; three levels are the only place k_ml_jacobi and the middle branch of the V-cycle run), attached as
    solver.py attaches it (coarser handles with shared_device=1, theta = 2, four sweeps).  The handles are first checked
    WITHOUT the term against the two-level model, then with it against multilevel_minv, in both modes (the Jacobi mode of a
    handle with a level attached applies Dinv + theta T); the level Jacobians of the model are the oracle's at the injected state."""
    import contextlib
    hier = hierarchies(refine)
    prob = hier[0][0]
    nv, nf = prob.coords.shape[0], prob.nf
    case = "ml%d" % refine
    u, un = R.case_state(case, prob)
    with contextlib.ExitStack() as stack:
        fine = stack.enter_context(gpu_lib.DeviceSolver(prob))
        coarse = [stack.enter_context(gpu_lib.DeviceSolver(h[0], shared_device=1)) for h in hier[1:]]
        fine.set_state(u, un)
        Fo, A = R.assembly_matches(fine, prob, u, un)
        b = R.case_rhs(case, Fo, A)
        agg = R.aggregates(fine.perm, nv, fine.n_aggregates)
        base = R.Observables(A, R.two_level_factory(A, nf, agg), b, K=3)
        _, w0, r0 = _observe(gpu_lib, fine, b, gpu_lib.LINEAR_TWOLEVEL, base, (case, "before attaching"))
        levels, parents = R.hierarchy_levels(hier, u, un, A0=A)
        uc, unc = u, un
        for l, dev in enumerate(coarse):       # the level handles' previous state, as the model injects it (u is injected by the library)
            ncv = hier[l + 1][0].coords.shape[0]
            uc, unc = (R.inject_state(v, hier[l][1], ncv, nf) for v in (uc, unc))
            dev.set_state(uc, unc)
            assert dev.n_aggregates == R.problem_aggregates(hier[l + 1][0])[1]
            assert np.array_equal(dev.perm, R.problem_perm(hier[l + 1][0]))
        gpu_lib.attach_level_chain([fine] + coarse, [h[1] for h in hier], theta=R.ML_THETA, sweeps=R.ML_SWEEPS)
        assert fine.krylov_launches_per_iteration == 4          # materialised vector form
        worst, worst_rel = [w0], [r0]
        for mname, mode in _modes(gpu_lib):
            ob = R.Observables(A, R.multilevel_factory(levels, parents, jacobi_base=(mname == "jacobi")), b, K=3)
            _, w, r = _observe(gpu_lib, fine, b, mode, ob, (case, "multilevel", mname))
            worst.append(w)
            worst_rel.append(r)
    print("%s (%s vertices): worst distance / tol_k %.3g, worst relative distance %.3g" %
          (case, [h[0].coords.shape[0] for h in hier], max(worst), max(worst_rel)))
