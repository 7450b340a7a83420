"""Host-side mirror of the reference's operator API for the hot path: ``solve(F == 0, u, bcs, solver_parameters)``
(reference 3D/MPNP_CO2ER_pore.py:789-799, 1D/MPNP_CO2ER_EDL.py:737-742) and the per-step glue around it
(``u_n.assign(u)``, ``compute_vertex_values``, Dirichlet rebuilds).  All arithmetic happens in libgmpnp.so."""
from __future__ import annotations

import numpy as np

from . import backend
from .problem import Problem


class _System:
    """What the two operator surfaces share: the problem, the iteration counters and the calls that go to `solver`, the object that
    holds the state and runs Newton (a ``DeviceSolver``, or a ``PartitionedSolver`` in GLOBAL file vertex order)."""

    def __init__(self, problem: Problem, solver):
        self.problem = problem
        self._solver = solver
        self.nv = problem.coords.shape[0]
        self.nf = problem.nf
        self.newton_iterations = 0
        self.krylov_iterations = 0
        self.last_stats = None

    # u = Function(V) is zero-initialised; u_n = interpolate(u_0, V)  (3D:425-432, 1D:320-326)
    def initialise(self, u0_values):
        u_n = np.tile(np.asarray(u0_values, dtype=np.float64), self.nv)
        self.set_state(np.zeros(self.problem.ndof), u_n)

    def set_state(self, u=None, un=None):
        """u and / or u_n from flat arrays in file vertex order (None: left as it is)."""
        self._solver.set_state(u, un)

    def set_bcs(self, dofs, vals):
        self.problem.bc_dofs, self.problem.bc_vals = dofs, vals
        self._solver.set_dirichlet(dofs, vals)

    def solve(self, solver_parameters=None):
        """``solve(F == 0, u, bcs, solver_parameters=...)``.  RuntimeError on non-convergence, as DOLFIN."""
        opts = backend.newton_options(solver_parameters, dim=self.problem.coords.shape[1])
        try:
            st = self._solver.newton_solve(opts)
        except backend.GmpnpError as e:
            if e.code == backend.ERR_NOT_CONVERGED:
                raise RuntimeError("Newton solver did not converge because maximum number of iterations reached") from e
            raise
        self.record(st)
        return st

    def record(self, st):
        """Account one Newton solve's statistics (also for solves an ensemble ran on this system's handle)."""
        self.newton_iterations += st["iterations"]
        self.krylov_iterations += st["krylov_iterations"]
        self.last_stats = st

    def vertex_values(self):
        """(nv, nf) array = compute_vertex_values() of every sub-function, file vertex order."""
        return self._solver.get_state().reshape(self.nv, self.nf)

    def column_select(self, fields, ranks):
        """k-th smallest values of vertex columns of u, on the device (gmpnp_column_select / gmpnp_group_column_select: over ALL
        ranks' owned rows, collective): (values, nan flag)."""
        return self._solver.column_select(fields, ranks)

    def species_budget(self):
        """(nf, 8) species budgets and consistent boundary fluxes of the current state, on the device (gmpnp_species_budget /
        gmpnp_group_species_budget: over ALL ranks' owned rows, collective); columns ``backend.BUDGET_COLUMNS``."""
        return self._solver.species_budget()

    def assign_previous(self):
        self._solver.assign_previous()


class GMPNPSystem(_System):
    """The objects a reference script holds between ``FunctionSpace`` and the time loop: mesh, forms (model tables),
    ``u``/``u_n`` (device resident) and the ``bcs`` list."""
    several_processes = False

    def __init__(self, problem: Problem, levels=None, ml_theta: float = 2.0, ml_sweeps: int = 4, **device_kwargs):
        """``levels`` (``problem.pore_hierarchy``, finest first, ``problem`` its finest): the geometric multilevel term of the
        preconditioner; the coarser levels are ordinary handles of the parent meshes on the same device, owned by this system."""
        if levels and getattr(problem, "stern", None) is not None:
            raise ValueError("multilevel: the Stern boundary condition is not available with the geometric multilevel term")
        if levels and getattr(problem, "kinetics", None) is not None:
            raise ValueError("multilevel: the surface kinetics are not available with the geometric multilevel term")
        if levels and getattr(problem, "galvanostat", None) is not None:
            raise ValueError("multilevel: the galvanostat is not available with the geometric multilevel term")
        self.dev = backend.DeviceSolver(problem, **device_kwargs)   # (hands problem.stern, .kinetics and .galvanostat to the handle)
        super().__init__(problem, self.dev)
        self._coarse = [backend.DeviceSolver(lv[0], device_id=device_kwargs.get("device_id", 0), shared_device=1) for lv in (levels or [])[1:]]
        backend.attach_level_chain([self.dev] + self._coarse, [lv[2] for lv in levels or []], ml_theta, ml_sweeps)

    def set_model(self, model):
        self.problem.model = model
        self.dev.set_model(model)

    # adaptive time stepping (include/gmpnp.h; the loop body lives in timestep.AdaptiveStepper)
    def set_time_step(self, inv_dt):
        self.dev.set_time_step(inv_dt)

    def time_error(self, h, h_prev, rtol, atol):
        return self.dev.time_error(h, h_prev, rtol, atol)

    def time_accept(self):
        self.dev.time_accept()

    def time_reject(self):
        self.dev.time_reject()

    # second order (variable-step BDF2)
    def set_time_order(self, order):
        self.dev.set_time_order(order)

    def time_history_levels(self):
        return self.dev.time_history_levels()

    def set_time_step_bdf2(self, inv_dt, ratio):
        self.dev.set_time_step_bdf2(inv_dt, ratio)

    def time_error_bdf2(self, h, h_prev, h_prev2, rtol, atol):
        return self.dev.time_error_bdf2(h, h_prev, h_prev2, rtol, atol)

    def owned_vertex_values(self):
        """[(vertex ids, (n, nf) values)] of the rows this process owns: here all of them."""
        return [(np.arange(self.nv), self.vertex_values())]

    # post-processing of the reference's drivers: project(+-grad(u_X), W) (3D:884-909, 1D:802-805) and the cell-wise
    # projections of the SUPG parameters (1D:599,651-653), on the device
    def project_gradient(self, f, sign=1.0):
        return self.dev.project_gradient(f, sign=sign)

    def project_cellwise(self, values):
        return self.dev.project_cellwise(values)

    def close(self):
        self.dev.close()
        for d in self._coarse:
            d.close()


class PartitionedSystem(_System):
    """The same operator surface on ONE problem cut into `nparts` mesh partitions (BASELINE configs[3]):
    the Newton and BiCGStab loops run inside libgmpnp.so across the ranks (gmpnp_group_newton_solve).  `rank` = None keeps
    every rank in this process (one GPU, rehearsal); `rank` = r is the one-process-per-GPU form over RCCL."""

    def __init__(self, problem: Problem, nparts: int, rank: int = None, levels=None, ml_theta: float = 2.0, ml_sweeps: int = 4, **device_kwargs):
        """``levels`` (``problem.pore_hierarchy``, finest first, ``problem`` its finest): the geometric multilevel term of the
        preconditioner across the partitions (``ml_theta`` / ``ml_sweeps`` as on one GPU)."""
        from .dist import PartitionedSolver
        self.ps = PartitionedSolver(problem, nparts, rank=rank, levels=levels, ml_theta=ml_theta, ml_sweeps=ml_sweeps, **device_kwargs)
        super().__init__(problem, self.ps)
        self.dev = self.ps.devs[0]            # this rank's LOCAL partition handle (local vertex numbering)
        self.several_processes = rank is not None and nparts > 1   # reading the whole state is then a collective
        self._device_kwargs = {k: v for k, v in device_kwargs.items() if k in ("device_id",)}
        self._post = None                     # unpartitioned handle on the global mesh, for post-processing only

    # adaptive time stepping is a single handle's: the groups' transports all-reduce sums, and the estimator's maximum and the
    # per-member step sizes are not built.  Refused here, before anything touches the device.
    def _no_adaptive(self, *args, **kwargs):
        raise ValueError("adaptive time stepping is not available on a partitioned system")

    set_time_step = time_error = time_accept = time_reject = _no_adaptive
    set_time_order = time_history_levels = set_time_step_bdf2 = time_error_bdf2 = _no_adaptive   # (order 2 no more than order 1)

    def owned_vertex_values(self):
        """[(global vertex ids, (n_owned, nf) values)] of this process's partitions: one device-to-host copy each, no collective."""
        return self.ps.owned_state()

    def _post_handle(self):
        """The projections of the drivers' output stage take GLOBAL vertex arrays: they run on an unpartitioned handle of
        the global mesh, created on first use (every rank that writes outputs holds one; it never solves)."""
        if self._post is None:
            self._post = backend.DeviceSolver(self.problem, shared_device=1, **self._device_kwargs)
        return self._post

    def project_gradient(self, f, sign=1.0):
        return self._post_handle().project_gradient(f, sign=sign)

    def project_cellwise(self, values):
        return self._post_handle().project_cellwise(values)

    def close(self):
        if self._post is not None:
            self._post.close()
            self._post = None
        self.ps.close()


def column_medians(vals, cols):
    """``[np.median(vals[:, c]) for c in cols]`` (reference 3D:817-824 takes the medians of four vertex arrays every
    time step) with one selection pass over a contiguous copy: 45 us instead of 230 us for 4 x 3,679 values.  Same
    values as ``np.median`` (middle element, or the mean of the two middle ones); NaNs fall back to it."""
    a = np.ascontiguousarray(np.asarray(vals)[:, list(cols)].T)
    n = a.shape[1]
    if n == 0 or np.isnan(a).any():
        return np.array([np.median(r) for r in a])
    h = n // 2
    if n % 2:
        return np.partition(a, h, axis=1)[:, h]
    p = np.partition(a, (h - 1, h), axis=1)
    return np.array([np.mean(p[i, h - 1:h + 1]) for i in range(p.shape[0])])


def device_column_medians(sys, cols):
    """``column_medians(sys.vertex_values(), cols)``, bit for bit, from the library's column select (one call, one host
    synchronisation; on a partitioned system collective over the ranks, no gather of the state).  A NaN in a selected column falls
    back to the gathered path, as ``column_medians`` falls back to ``np.median``."""
    return device_medians_and_minima(sys, cols, ())[0]


def device_medians_and_minima(sys, cols, min_cols):
    """(``column_medians`` of `cols`, ``[np.amin(column) for column in min_cols]``) of the state of `sys` in ONE
    ``column_select`` call: the middle element, or ``np.mean`` of the two middle ones, as ``column_medians``; the minimum is the
    smallest element (a zero minimum comes back as +0.0).  NaN in a selected column: the gathered state."""
    cols, min_cols = list(cols), list(min_cols)
    n = sys.nv
    if n == 0:
        vals = sys.vertex_values()
        return column_medians(vals, cols), [float(np.amin(vals[:, c])) for c in min_cols]
    h = n // 2
    mids = [h] if n % 2 else [h - 1, h]
    fields = [c for c in cols for _ in mids] + min_cols
    ranks = mids * len(cols) + [0] * len(min_cols)
    out, nan = sys.column_select(fields, ranks)
    if nan:
        vals = sys.vertex_values()
        return column_medians(vals, cols), [float(np.amin(vals[:, c])) for c in min_cols]
    k = len(mids)
    if k == 1:
        med = out[:len(cols)].copy()
    else:
        med = np.array([np.mean(out[2 * i:2 * i + 2]) for i in range(len(cols))])
    return med, [float(v) for v in out[k * len(cols):]]


def supg_parameters(coords, cells, z, p_prev, project_cellwise, h_vertex=None, fact=1.0, tol=1.0e-14):
    """Nodal SUPG parameters of the PNP stabilisation, reference 1D:597-670 (1D meshes): Pe_i = fact h |grad p| |z_i| / 2
    at the vertices (h = projected cell diameter, |grad p| = projected gradient norm of the PREVIOUS step's potential);
    rho_i = fact h / (2 |z_i| |grad p|) where Pe_i > 1 + tol, else fact^2 h^2 / 4; 0 for uncharged species.
    ``project_cellwise(values)`` is the consistent-mass P1 projection of a cell-wise constant field — in the drivers the
    device's (``DeviceSolver.project_cellwise`` = gmpnp_project_cellwise).  Returns (rho (nv, ns), h_vertex)."""
    assert coords.shape[1] == 1, "the reference stabilises the 1D script only"
    X = coords[cells]
    length = X[:, 1, 0] - X[:, 0, 0]
    if h_vertex is None:
        h_vertex = project_cellwise(np.abs(length))
    gradp = (p_prev[cells[:, 1]] - p_prev[cells[:, 0]]) / length
    norm = project_cellwise(np.abs(gradp))
    z = np.asarray(z, dtype=float)
    rho = np.zeros((coords.shape[0], len(z)))
    rho_small = fact ** 2 * h_vertex ** 2 / 4
    for i, zi in enumerate(z):
        if zi == 0:
            continue
        Pe = fact * h_vertex * norm * abs(zi) / 2
        with np.errstate(divide="ignore", invalid="ignore"):
            rho_large = fact * h_vertex / (2 * abs(zi) * norm)
        rho[:, i] = np.where(Pe > 1.0 + tol, rho_large, rho_small)
    return rho, h_vertex
