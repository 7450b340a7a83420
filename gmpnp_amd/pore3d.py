"""3D cylindrical-pore GMPNP driver on the MI355X backend — same CLI flags, YAML/XML inputs and output layout as
reference 3D/MPNP_CO2ER_pore.py (``solveEDL`` 3D:96-1085, CLI 3D:1088-1253).

Differences, all explicit: input/output roots come from ``$GMPNP_UTILITIES`` / ``$GMPNP_OUT`` instead of the
author's hard-coded macOS paths; ``--num_steps`` (not in the reference) shortens the 1000-step loop;
``--as_published`` drops the ds(2)/ds(3) flux terms that the published script never adds to F; ``--refine N`` /
``--multilevel`` run on the N times uniformly refined mesh (with the multilevel term of the preconditioner); ``--partitions N`` solves
the one problem on N mesh partitions (in this process on one GPU, or one rank per process under ``torch.distributed.run``)."""
from __future__ import annotations

import argparse
import json
import os
from datetime import datetime

import numpy as np

from . import backend
from .mesh import read_dolfin_xml, resolve_mesh_path
from .params import pore_parameters, utilities_dir
from .problem import (Galvanostat, add_galvanostat_arguments, add_kinetics_arguments, add_stern_arguments, galvanostat_keywords, kinetics_keywords,
                      pop_galvanostat, pop_kinetics, pop_stern, pore_dirichlet, pore_problem, stern_keywords)
from .solver import GMPNPSystem, column_medians, device_medians_and_minima
from .timestep import DriverStepping, adaptive_keywords, add_adaptive_arguments
from .polarisation import add_polarisation_arguments, polarisation_keywords
from .impedance import add_pore_impedance_arguments, pore_impedance_keywords
from .programme import add_pore_programme_arguments, pore_programme_keywords
from .vtk import write_pvd

SOLVER_PARAMETERS = {  # reference 3D:789-798
    "nonlinear_solver": "newton",
    "newton_solver": {"linear_solver": "mumps", "maximum_iterations": 50, "relative_tolerance": 1.0e-4,
                      "absolute_tolerance": 1.0e-4, "relaxation_parameter": 0.9},
}


def scale_conc_time(species="H", C=None, grad_c=None, bulk_conc=None, tau=None, diff_coeff_eff=None, L=0.0):
    """reference 3D:56-67"""
    c = C * bulk_conc[species]
    t = tau * (L ** 2) / diff_coeff_eff[species]
    grad_c_scaled = grad_c * bulk_conc[species] / L
    return c, t, grad_c_scaled


def output_root():
    return os.environ.get("GMPNP_OUT", os.path.join(os.getcwd(), "out"))


class PoreRun:
    """State of one pore simulation; ``step()`` is one pass of the reference's time loop body (3D:783-858)."""

    def __init__(self, num_steps=None, as_published=False, device_kwargs=None, solver_parameters=None, refine=0,
                 partition=None, multilevel=False, ml_theta=2.0, ml_sweeps=4, glue="host", budget=False, step_fraction=0.0,
                 adaptive_dt=False, dt_rtol=1e-2, dt_atol=1e-4, dt_init=None, dt_min=0.0, dt_max=None, t_end=None, steady_tol=0.0,
                 max_steps=None, dt_order=1, **kwargs):
        """``partition`` = (nparts, rank): solve this ONE problem across `nparts` mesh partitions (rank None: all of them in
        this process on one GPU; rank r: this process is rank r of a ``torch.distributed`` job, RCCL inside the library).
        ``multilevel`` (with ``refine`` > 0): the preconditioner gets the geometric multilevel term over the nested meshes
        (gmpnp_attach_coarse_level; with ``partition`` across the mesh partitions, every level partitioned alike) — not a reference
        feature; it changes iteration counts of the linear solves, not results.
        ``glue`` = "host": every step gathers the whole state to the host (with one rank per process: an all-reduce of it through
        torch.distributed) for the medians, the CO2 minimum and the history row; "device": the medians and the minimum come from the
        library's column select (csrc/gmpnp_stats.h: collective inside the library, identical values) and the history keeps this
        process's OWNED rows only (one device-to-host copy per local partition, no collective); ``write_outputs`` assembles the
        global history on rank 0, which alone prints and writes.
        ``budget`` = True: every step records the species-budget table of its solution (``species_budget()``: integrated storage,
        reaction, wall / exit fluxes and the consistent Dirichlet flux per field; on a partitioned run summed over the ranks inside
        the library, no gather of the state) and ``write_outputs`` adds ``budget.npz`` (gmpnp_amd/budget.py).  Off: nothing changes.
        ``step_fraction`` = tau in (0, 1): the Newton updates go through the fraction-to-boundary step limiter
        (``newton_solver["step_fraction"]``, include/gmpnp.h; not a reference feature); 0 = off.  Not with ``partition``: the
        partitioned solve has no limiter (ValueError, before anything touches the device).
        ``adaptive_dt`` = True: the step size is the error controller's (gmpnp_amd/timestep.py; not a reference feature), ``inv_dt`` =
        1/h in the driver's scaled time: ``dt_rtol`` / ``dt_atol`` its weights, ``dt_init`` the first step (default: the reference
        step), ``dt_min`` / ``dt_max`` its bounds, ``t_end`` the end time (default: the driver's T), ``steady_tol`` > 0 the steady
        stop, ``max_steps`` the largest number of attempted steps, ``dt_order`` = 2 variable-step BDF2 in backward Euler's place
        (after its start-up).  A rejected step leaves the clock, the history, the budget log and
        the CO2 Dirichlet value as they were.  Not with ``partition`` (ValueError, before anything touches the device).  Off: nothing
        changes.
        ``electrode_voltage`` = X (thermal voltages; in place of ``voltage_multiplier``, giving both is a ValueError): the electrode
        potential is applied on the wall through the Stern-layer boundary condition (``stern_model`` "BDM" or
        "linear", ``stern_length`` 4e-10 m, ``stern_eps_surface`` 6); the wall potential becomes a result.  Not with ``partition`` or
        ``multilevel`` (ValueError, before anything touches the device).  The metadata gains ``electrode_voltage``, ``stern_model``,
        ``stern_length``, ``stern_displacement`` (the Stern term integrated over the wall, scaled units) and ``surface_charge``
        [C/m2] = eps_0 thermal_voltage / L x stern_displacement / wall area (scaled): the mean charge per area on the electrode.
        ``kinetics`` = "tafel" (with ``electrode_voltage``; ``i0_CO`` / ``i0_H2`` [A/m2] required, ``alpha_CO`` / ``alpha_H2`` = 0.5,
        ``p_eq_CO`` / ``p_eq_H2`` = 0 thermal voltages): the wall fluxes of CO2, CO, H2 and OH follow the potential drop across the
        Stern layer and the CO2 concentration at the wall (gmpnp_amd/kinetics.py) in place of the prescribed
        ``current_rough`` / ``H2_FE``, which are then unused for them.  Not with ``partition`` or ``multilevel`` (ValueError, before
        anything touches the device).  Every step records the wall means ``i_CO``, ``i_H2`` [A/m2] and ``FE_H2``
        (arrays_unscaled.npz; the last values and the kinetic parameters in the metadata).
        ``target_current`` = X [A/m2] (with ``kinetics``): galvanostatic mode: every Newton solve also finds the
        electrode potential at which the wall mean of i_CO + i_H2 is X; ``electrode_voltage`` is the starting guess.  The linear solver
        is the block-banded LU (a ``solver_parameters`` that names bicgstab is a ValueError); the first solve starts from the bulk state.  Works with ``step_fraction``, ``budget``
        and ``adaptive_dt`` at order 1; not with ``dt_order`` 2, ``partition`` or ``multilevel``.  Every step records
        ``electrode_voltage``; the metadata gains ``target_current`` and reports the last potential found.
        ``polarisation`` = dict(v_end=X, v_step=Y[, params=(0, ...)]) (thermal voltages; with ``electrode_voltage``): ``write_outputs``
        walks the steady-state polarisation curve from the run's last state and potential (``polarisation()``)
        and adds ``polarisation.npz`` and the ``polarisation_*`` metadata keys.  Not with ``target_current``, ``dt_order`` 2,
        ``partition`` or ``multilevel`` (ValueError, before anything touches the device).
        ``pore_impedance`` = dict(freq_min=1e-2, freq_max=1e8, per_decade=10) [Hz] (with ``electrode_voltage``): ``write_outputs``
        computes the impedance spectrum of the pore at the run's last state (``pore_impedance()`` does the same at
        any time) and adds ``pore_impedance.npz`` (frequency, sigma, capacitance [F/m2], admittance [S/m2], impedance [Ohm m2], dI_CO,
        dI_H2 [S/m2], residual; all per wall area) and the metadata keys ``pore_impedance_points``, ``pore_impedance_status``,
        ``capacitance_low`` / ``capacitance_high``, ``capacitance_high_closed_form`` (the potential block alone), ``R_ct`` (None
        without kinetics) and ``pore_impedance_last_step_change``.  Not with ``partition``, ``multilevel`` or the device glue; a
        galvanostat is switched off for the call.  The keyword ``impedance`` is the 1D driver's and stays refused here.
        ``pore_programme`` = dict(kind="pulse", v_levels=[A, B], durations=[s, s], cycles=n[, rise_time=s]) | dict(kind="triangle",
        v_vertex=X, scan_rate=V/s, cycles=n) | dict(kind="table", time_s=[...], electrode_voltage=[...]), with ``bins`` (16: a count of
        axial bins, uniform over the z range of the wall nodes, or explicit edges [m]) and ``dt_init``, ``steps_per_segment``,
        ``capacity`` (with ``electrode_voltage``): ``write_outputs`` marches the electrode potential through the waveform from the run's
        last state, after the schedule and before ``pore_impedance`` and ``polarisation``, on a clock of its own that starts at 0
        (``pore_programme()`` does the same at any time).  Per accepted step the device forms one electrode record
        and one wall-profile record per bin (``gmpnp_wall_profile_append``) without a copy of the state, and the lagged Sechenov update
        of ``accept_solution`` is applied from the device's medians.  Adds ``pore_programme.npz`` (``programme.PORE_OUTPUT_KEYS``),
        ``pore_programme_states.npz``, the attempts as ``pore_programme_*`` arrays of ``timestep_log.npz`` and the metadata keys
        ``programme.PORE_METADATA_KEYS``; afterwards the run stands at the programme's last potential.  Order 1, no sensitivities; not
        with ``target_current``, ``polarisation``, ``dt_order`` 2, ``partition``, ``multilevel`` or the device glue (ValueError, before
        anything touches the device).  The keyword ``programme`` is the 1D driver's and stays refused here."""
        if glue not in ("host", "device"):
            raise ValueError("glue must be 'host' or 'device'")
        from .impedance import refuse_impedance
        refuse_impedance(kwargs, "the 3D pore driver (it needs a complex band LU)")
        from .fit import refuse_fit
        from .programme import refuse_programme
        refuse_fit(kwargs, "the 3D pore driver (the library's parameter advance works there, the fit's host glue is 1D)")
        refuse_programme(kwargs, "the 3D pore driver (potential programmes are 1D)")
        self.pore_programme_par = kwargs.pop("pore_programme", None) or None
        if self.pore_programme_par is not None:   # (while kwargs still holds polarisation, target_current and electrode_voltage)
            from .programme import check_pore_programme
            self.pore_programme_par = check_pore_programme(self.pore_programme_par, kwargs, dt_order, partition, multilevel, glue)
        self.polarisation_par = kwargs.pop("polarisation", None) or None
        if self.polarisation_par is not None:
            from .polarisation import check_polarisation
            if partition:
                raise ValueError("polarisation: the curve is not available in a partitioned solve")
            if multilevel:
                raise ValueError("polarisation: the curve is not available with the geometric multilevel term")
            self.polarisation_par = check_polarisation(self.polarisation_par, kwargs, dt_order)
        self.pore_impedance_par = kwargs.pop("pore_impedance", None) or None
        if self.pore_impedance_par is not None:
            from .impedance import frequency_grid
            if kwargs.get("electrode_voltage") is None:
                raise ValueError("pore_impedance: the frequency response needs an electrode potential (electrode_voltage)")
            if partition:
                raise ValueError("pore_impedance: the frequency response is not available in a partitioned solve")
            if multilevel:
                raise ValueError("pore_impedance: the frequency response is not available with the geometric multilevel term")
            if glue != "host":
                raise ValueError("pore_impedance: the frequency response runs with the host glue")
            self.pore_impedance_par = dict(self.pore_impedance_par)
            try:
                frequency_grid(**self.pore_impedance_par)   # a bad grid is refused before anything touches the device
            except ValueError as e:
                raise ValueError("pore_" + str(e)) from None
        self.stern = pop_stern(kwargs, kwargs.get("L", 100.0e-9))
        self.kinetic_par = pop_kinetics(kwargs)
        self.target_current = pop_galvanostat(kwargs)
        if self.target_current is not None:
            if self.kinetic_par is None:
                raise ValueError("target_current: the galvanostat needs the surface kinetics (kinetics='tafel')")
            if int(dt_order) == 2:
                raise ValueError("target_current: the galvanostat is not available with dt_order 2")
            if partition:
                raise ValueError("target_current: the galvanostat is not available in a partitioned solve")
            if multilevel:
                raise ValueError("target_current: the galvanostat is not available with the geometric multilevel term")
            lin = dict((solver_parameters or SOLVER_PARAMETERS).get("newton_solver", {})).get("linear_solver", "default")
            if lin == "bicgstab":
                raise ValueError("target_current: the galvanostat solves with the block-banded LU, not with bicgstab")
        if self.kinetic_par is not None:
            if self.stern is None:
                raise ValueError("kinetics: the surface kinetics need an electrode potential (electrode_voltage)")
            if partition:
                raise ValueError("kinetics: the surface kinetics are not available in a partitioned solve")
            if multilevel:
                raise ValueError("kinetics: the surface kinetics are not available with the geometric multilevel term")
        if self.stern is not None and partition:
            raise ValueError("electrode_voltage: the Stern boundary condition is not available in a partitioned solve")
        if self.stern is not None and multilevel:
            raise ValueError("electrode_voltage: the Stern boundary condition is not available with the geometric multilevel term")
        self.adaptive = bool(adaptive_dt)
        self.dt_tol, self.dt_bounds, self.max_steps, self.dt_order = (dt_rtol, dt_atol), (dt_min, dt_max), max_steps, int(dt_order)
        if self.adaptive and partition:
            raise ValueError("adaptive_dt: adaptive time stepping is not available in a partitioned solve")
        self.step_fraction = float(step_fraction)
        if self.step_fraction and partition:
            raise ValueError("step_fraction: the step limiter is not available in a partitioned solve")
        self.glue = glue
        self.rank = partition[1] if partition else None
        self.kwargs = kwargs
        self.pp = pore_parameters(as_published=as_published, **kwargs)
        self.mesh = read_dolfin_xml(resolve_mesh_path(utilities_dir(), self.pp.mesh_name))
        self._levels = None
        self.kinetics, self.currents = None, []
        if self.kinetic_par is not None:
            from .kinetics import pore_tafel
            from .params import _load_yaml
            farad = _load_yaml(os.path.join(utilities_dir(), kwargs.get("params_file", "parameters_pore") + ".yaml"))["nat_const"]["F"]
            self.kinetics, self.pp.model = pore_tafel(self.pp, self.kinetic_par, self.stern.p_electrode, farad)
            print("kinetics tafel: current_rough and H2_FE are not used for the CO2, CO, H2 and OH fluxes at the wall")
        if multilevel and refine > 0:
            from .problem import pore_hierarchy
            self._levels = pore_hierarchy(self.pp, self.mesh, refine)
            self.problem, self.bnd = self._levels[0][0], self._levels[0][1]
        else:
            self.problem, self.bnd = pore_problem(self.pp, self.mesh, refine=refine, stern=self.stern, kinetics=self.kinetics)
        self.galvanostat, self.potentials = None, []
        if self.target_current is not None:   # the library's target is the integrated current: X times sum_I w_I, the wall area
            self.galvanostat = Galvanostat(self.target_current * self.wall_area())
            self.problem.galvanostat = self.galvanostat
            solver_parameters = dict(solver_parameters or SOLVER_PARAMETERS)
            solver_parameters["newton_solver"] = dict(solver_parameters.get("newton_solver", {}), linear_solver="band_lu")
        if refine:  # uniformly refined copy of the reference mesh (not a reference feature: roofline studies)
            from .mesh import Mesh
            self.mesh = Mesh(dim=3, coords=self.problem.coords, cells=self.problem.cells)
        sys_kwargs = dict(levels=self._levels, ml_theta=ml_theta, ml_sweeps=ml_sweeps, **(device_kwargs or {}))
        if partition:
            from .solver import PartitionedSystem
            self.sys = PartitionedSystem(self.problem, partition[0], rank=partition[1], **sys_kwargs)
        else:
            self.sys = GMPNPSystem(self.problem, **sys_kwargs)
        self.solver_parameters = backend.with_step_fraction(solver_parameters or SOLVER_PARAMETERS, self.step_fraction)
        self.tot_num_steps = self.pp.tot_num_steps if num_steps is None else int(num_steps)
        nv = self.mesh.num_vertices
        self.sys.initialise([1.0] * 8 + [0.0])
        if self.galvanostat is not None:
            # The first Newton solve starts from the bulk state, not from u = 0: at u = 0 the CO2 current (first order in u_CO2) is
            # exactly 0, the constraint ln(I / target) is linearised where I is the hydrogen current alone, and with i_CO >> i_H2 its
            # first correction of p_M overshoots out of the admissible set (the 1D driver's first step keeps u = 0).
            self.sys.set_state(np.tile(np.r_[np.ones(8), 0.0], nv), None)
        # history rows: initial ones/zeros (3D:771-779), one row appended per step (3D:842-850); "device" glue: the rows this process
        # owns, one array per local partition (vertex ids in self.owned_ids)
        if glue == "device":
            self.owned_ids = [ids for ids, _ in self.sys.owned_vertex_values()]
            self.history = [[np.concatenate([np.ones((len(ids), 8)), np.zeros((len(ids), 1))], axis=1) for ids in self.owned_ids]]
        else:
            self.history = [np.concatenate([np.ones((nv, 8)), np.zeros((nv, 1))], axis=1)]
        self.CO2_min = None
        self.co2_bc = None  # CO2 Dirichlet value in force (None = the equilibrium value of the set-up)
        self.n = 0
        self.t = 0.0
        self.newton_its = []
        self.budget = None
        if budget:
            from .budget import BudgetLog, pore_factors
            self.budget = BudgetLog(list(self.pp.species[:7]) + ["cat", "p"], *pore_factors(self.pp))
        self.stepper = None
        if self.adaptive:
            self.stepping = DriverStepping(self.sys, self.solver_parameters, lambda h: 1.0 / h, self.pp.dt, self.pp.T, dt_rtol=dt_rtol,
                                           dt_atol=dt_atol, dt_init=dt_init, dt_min=dt_min, dt_max=dt_max, t_end=t_end, steady_tol=steady_tol,
                                           max_steps=max_steps, dt_order=dt_order)
            self.stepper, self.times = self.stepping.stepper, self.stepping.times   # times: the actual times of the history rows

    def adaptive_step(self, verbose=True):
        """One ATTEMPTED step of the adaptive run (``timestep.AdaptiveStepper.attempt``): the glue of ``step`` runs for an accepted
        step only, with ``time_accept`` in place of ``assign_previous``.  Returns the attempt's log row."""
        row = self.stepping.attempt(None, lambda st: self.adaptive_before_accept(st, None, verbose), verbose)
        self.t = self.stepper.t
        return row

    def adaptive_before_accept(self, st, row=None, verbose=True):
        """Host glue of an ACCEPTED step, while u_n is the previous state and inv_dt the step's.  ``row``: the (nv, nf) vertex
        values of u when the caller holds them already (``PoreEnsemble``: the member's row of one copy for all members)."""
        if self.budget is not None:
            self.budget.take(self.sys)
        if row is None and self.glue == "device":
            meds, (co2_min,) = device_medians_and_minima(self.sys, (1, 2, 3, 7), (4,))
            row = [v for _, v in self.sys.owned_vertex_values()]
        else:
            if row is None:
                row = self.sys.vertex_values()
            meds, co2_min = column_medians(row, (1, 2, 3, 7)), float(np.amin(row[:, 4]))
        self.accept_solution(st, row, meds, co2_min, verbose=verbose, assign=False)

    def step(self, verbose=True):
        """One time step.  The glue decides where the medians and the CO2 minimum come from and what a history row is; the two
        settings give the same values.  (The row and the minimum are taken in front of ``set_bcs`` under both: the device glue reads
        them from the device there, the host glue from the array it has gathered already, where the place makes no difference.)"""
        if self.stepper is not None:
            return self.adaptive_step(verbose)
        device = self.glue == "device"
        self.t += self.pp.dt
        st = self.sys.solve(self.solver_parameters)
        if self.budget is not None:   # after the Newton solve, before set_bcs / assign_previous
            self.budget.take(self.sys)
        if device:   # the library's column select, no gather of the state; the history keeps this process's owned rows
            meds, (co2_min,) = device_medians_and_minima(self.sys, (1, 2, 3, 7), (4,))
            row = [v for _, v in self.sys.owned_vertex_values()]
        else:
            row = self.sys.vertex_values()
            meds, co2_min = column_medians(row, (1, 2, 3, 7)), float(np.amin(row[:, 4]))
        self.accept_solution(st, row, meds, co2_min, verbose=verbose and (not device or self.rank in (None, 0)))
        return st

    def accept_solution(self, st, row, meds, co2_min, verbose=False, assign=True):
        """What follows the Newton solve of a step: history row, Sechenov, new Dirichlet set, ``u_n.assign(u)``, counters.
        ``assign=False``: the caller assigns (``PoreEnsemble`` does it for all its members with one launch)."""
        self.history.append(row)
        if self.kinetics is not None:
            self.currents.append(self.sys.dev.kinetics_currents())
        if self.galvanostat is not None:
            self.potentials.append(self.sys.dev.galvanostat_report()["p_electrode"])
        # medians of the scaled ion concentrations -> Sechenov -> new CO2 Dirichlet value at S1 (3D:817-838)
        self.co2_bc = self.pp.sechenov_co2_scaled(*meds)
        self.sys.set_bcs(*pore_dirichlet(self.pp, self.bnd, self.co2_bc, stern=self.stern is not None))
        self.CO2_min = co2_min
        if assign:
            self.sys.assign_previous()
        self.newton_its.append(st["iterations"])
        if verbose:
            print(self.CO2_min)
            print(datetime.now().strftime("%y-%m-%d-%H-%M-%S"))
            print(self.n)
        self.n += 1

    def field_history(self, i):
        """(steps + 1, nv) history of field i in file vertex order.  "device" glue with one rank per process: gathered to rank 0
        (collective: every rank calls it; None on the other ranks)."""
        if self.glue == "host":
            return np.stack([row[:, i] for row in self.history])
        parts = [(ids, np.stack([row[d][:, i] for row in self.history])) for d, ids in enumerate(self.owned_ids)]
        if self.sys.several_processes:
            import torch.distributed as tdist
            if not (tdist.is_available() and tdist.is_initialized()):
                raise RuntimeError("one rank per process: the history is gathered through torch.distributed, which is not initialised")
            got = [None] * tdist.get_world_size() if self.rank == 0 else None
            tdist.gather_object(parts, got, dst=0)
            if self.rank != 0:
                return None
            parts = [p for g in got for p in g]
        out = np.empty((len(self.history), self.mesh.num_vertices))
        for ids, h in parts:
            out[:, ids] = h
        return out

    def run(self, verbose=True):
        if self.stepper is not None:
            self.stepping.run(lambda: self.adaptive_step(verbose))
            return self
        for _ in range(self.n, self.tot_num_steps):
            self.step(verbose)
        return self

    def stern_summary(self):
        """The metadata keys of a run with the Stern boundary condition (see ``__init__``), from the device's current state."""
        from .params import _load_yaml
        pp, st = self.pp, self.stern
        X = self.problem.coords[self.problem.wall_facets]
        area = float((0.5 * np.linalg.norm(np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]), axis=1)).sum())
        d = self.sys.dev.stern_displacement()
        eps_0 = _load_yaml(os.path.join(utilities_dir(), self.kwargs.get("params_file", "parameters_pore") + ".yaml"))["nat_const"]["eps_0"]
        p_M = self.potentials[-1] if self.potentials else st.p_electrode   # galvanostatic mode: the potential that was found
        return {"electrode_voltage": p_M, "stern_model": st.model, "stern_length": st.lam * pp.L, "stern_displacement": d,
                "surface_charge": eps_0 * pp.thermal_voltage / pp.L * d / area}

    def polarisation(self, v_end, v_step, params=(0,), predictor=True, solver_parameters=None):
        """The steady-state polarisation curve from the run's LAST state and electrode potential to ``v_end`` on the grid
        electrode_voltage + k ``v_step`` (gmpnp_amd/polarisation.py: ``run_continuation``, ``DeviceOps``), as ``EDLRun.polarisation``
        walks it, with the block-banded LU.  At every point the Sechenov update of the CO2 Dirichlet value (as ``accept_solution``
        forms it from the medians of the ion concentrations) and the Newton solve are repeated until the value changes by less than
        1e-10 relative, for at most 10 rounds (recorded as ``sechenov_rounds``).  The tangent is taken at the final Dirichlet values:
        the slopes (capacitance, dI/dV, Tafel slopes, sensitivities) do NOT include the feedback of the potential on the CO2 value.
        Currents and charges are wall means (divided by ``wall_area``)."""
        from types import SimpleNamespace
        from . import polarisation as pol
        from .params import _load_yaml
        if self.stern is None:
            raise ValueError("polarisation: the curve needs an electrode potential (electrode_voltage)")
        if self.galvanostat is not None:
            raise ValueError("polarisation: the curve is not available with target_current (the galvanostat)")
        if self.glue != "host" or self._levels is not None or self.rank is not None:
            raise ValueError("polarisation: the curve runs on one unpartitioned handle without the multilevel term (host glue)")
        par = pol.check_polarisation(dict(v_end=v_end, v_step=v_step, params=params),
                                     dict(electrode_voltage=self.stern.p_electrode, kinetics=self.kinetic_par))
        sp = dict(solver_parameters or pol.NEWTON)
        sp["newton_solver"] = dict(sp.get("newton_solver", {}), linear_solver="band_lu")
        sp = backend.with_step_fraction(sp, self.step_fraction)
        wall = np.unique(np.asarray(self.problem.wall_facets, dtype=np.int64))
        nf = self.problem.nf

        def after_solve():
            new = self.pp.sechenov_co2_scaled(*column_medians(self.sys.vertex_values(), (1, 2, 3, 7)))
            old, self.co2_bc = self.co2_bc, new
            if old is not None and abs(new - old) <= 1e-10 * abs(new):
                return False
            self.sys.set_bcs(*pore_dirichlet(self.pp, self.bnd, new, stern=True))
            return True

        ops = pol.DeviceOps(self, backend.newton_options(sp, dim=3), par["params"],
                            lambda u: float(u.reshape(-1, nf)[wall, nf - 1].mean()), after_solve=after_solve)
        inv_dt = float(self.sys.problem.model.inv_dt)
        self.sys.set_time_step(0.0)
        try:
            records, substeps, newton, stop = pol.run_continuation(ops, self.stern.p_electrode, par["v_end"], par["v_step"], predictor)
        finally:
            self.sys.set_time_step(inv_dt)
        eps_0 = _load_yaml(os.path.join(utilities_dir(), self.kwargs.get("params_file", "parameters_pore") + ".yaml"))["nat_const"]["eps_0"]
        out = pol.curve_arrays(SimpleNamespace(thermal_voltage=self.pp.thermal_voltage, L_n=self.pp.L), eps_0, self.wall_area(), records,
                               par["params"], substeps, newton)
        out["stop_reason"] = stop
        return out

    def polarisation_outputs(self, newpath):
        """``polarisation.npz`` of the curve from the last state and the metadata keys that go with it."""
        out = self.polarisation(**self.polarisation_par)
        stop = out.pop("stop_reason")
        np.savez(os.path.join(newpath, "polarisation.npz"), **out)
        return {"polarisation_points": int(len(out["electrode_voltage"])), "polarisation_v_end": float(self.polarisation_par["v_end"]),
                "polarisation_v_step": float(self.polarisation_par["v_step"]), "polarisation_stop_reason": stop,
                "polarisation_newton_iterations": int(out["newton_iterations"].sum()), "polarisation_substeps": int(out["substeps"].sum()),
                "polarisation_worst_residual": float(np.max(out["tangent_residual"])),
                "polarisation_params": [int(q) for q in out["sensitivity_params"]],
                "polarisation_sechenov_rounds": int(out["sechenov_rounds"].max())}

    def pore_impedance(self, frequencies):
        """The impedance spectrum of the pore at the run's CURRENT state and electrode potential, at ``frequencies`` [Hz], per wall
        area (gmpnp_amd/impedance.py: ``pore_spectrum``; one ``gmpnp_frequency_response_3d`` call).  A
        galvanostatic run switches its galvanostat off for the call (that keeps the potential it found) and on again with the same
        target.  Refused where ``polarisation`` is: partitions, the multilevel term, the device glue."""
        from . import impedance as imp
        if self.stern is None:
            raise ValueError("pore_impedance: the frequency response needs an electrode potential (electrode_voltage)")
        if self.glue != "host" or self._levels is not None or self.rank is not None:
            raise ValueError("pore_impedance: the frequency response runs on one unpartitioned handle without the multilevel term (host glue)")
        f = np.atleast_1d(np.asarray(frequencies, dtype=np.float64))
        if not imp.count_valid(f.size) or not np.all(np.isfinite(f)) or np.any(f < 0.0):
            raise ValueError("pore_impedance: 1 ... %d finite frequencies >= 0" % imp.MAX_FREQUENCIES)
        dev = self.sys.dev
        if self.galvanostat is not None:
            dev.set_galvanostat(None)
        try:
            res = dev.frequency_response_3d(imp.pore_sigma_from_frequency(self.pp, f))
        finally:
            if self.galvanostat is not None:
                dev.set_galvanostat(self.galvanostat)
        return imp.pore_spectrum(self.pp, self._eps_0(), self.wall_area(), f, res)

    def _eps_0(self):
        from .params import _load_yaml
        return _load_yaml(os.path.join(utilities_dir(), self.kwargs.get("params_file", "parameters_pore") + ".yaml"))["nat_const"]["eps_0"]

    def pore_impedance_outputs(self, newpath):
        """``pore_impedance.npz`` of the last state and the metadata keys that go with it.  ``capacitance_high_closed_form``: the
        concentrations frozen, x_p solves the potential block of the device's own Jacobian (``impedance.potential_block_capacitance``)."""
        from . import impedance as imp
        sp = self.pore_impedance(imp.frequency_grid(**self.pore_impedance_par))
        nr = sp["dI_dV"].shape[1]
        zero = np.zeros(len(sp["frequency"]), dtype=complex)
        np.savez(os.path.join(newpath, "pore_impedance.npz"), frequency=sp["frequency"], sigma=sp["sigma"], capacitance=sp["capacitance"],
                 admittance=sp["admittance"], impedance=sp["impedance"], dI_CO=sp["dI_dV"][:, 0] if nr > 0 else zero,
                 dI_H2=sp["dI_dV"][:, 1] if nr > 1 else zero, residual=sp["residual"])
        eps_0 = self._eps_0()
        dev, prob = self.sys.dev, self.problem
        p_M = self.potentials[-1] if self.potentials else self.stern.p_electrode
        stern = type(self.stern)(self.stern.model, p_M, self.stern.lam, self.stern.eps_surface)
        nf = prob.nf
        u2d = dev.get_state().reshape(-1, nf)
        dev.assemble(True)   # (the potential block of J does not depend on inv_dt: the mass sits on the species rows)
        K = dev.jacobian_csr()
        bc = self.sys.problem.bc_dofs
        _, b = imp.pore_stern_terms(prob.coords, prob.wall_facets, prob.model, stern, bc, u2d)
        c_inf, _ = imp.potential_block_capacitance(K, b, np.arange(nf - 1, prob.ndof, nf),
                                                   lambda x: imp.pore_stern_terms(prob.coords, prob.wall_facets, prob.model, stern, bc, u2d, x.reshape(-1, nf))[0].real)
        c_inf = c_inf * eps_0 / self.pp.L / self.wall_area()
        g_ct = -float(sp["dI_dV"][0].sum().real) if nr else 0.0
        change = float(np.abs(self.history[-1] - self.history[-2]).max()) if len(self.history) > 1 else None
        return {"pore_impedance_points": int(len(sp["frequency"])), "capacitance_low": float(sp["capacitance"][0].real),
                "capacitance_high": float(sp["capacitance"][-1].real), "capacitance_high_closed_form": float(c_inf),
                "R_ct": (1.0 / g_ct) if g_ct != 0.0 else None, "pore_impedance_last_step_change": change,
                "pore_impedance_status": int(np.bitwise_or.reduce(sp["status"]))}

    def wall_node_z(self):
        """z (units of L) of the wall's nodes: what the bins of the wall profile sort."""
        wall = np.unique(np.asarray(self.problem.wall_facets, dtype=np.int64))
        return np.asarray(self.problem.coords, dtype=np.float64)[wall, 2]

    def sechenov_glue(self):
        """The lagged Sechenov update of ``accept_solution`` from the device's medians (no state is gathered) and the new Dirichlet
        set: what an accepted step of ``pore_programme`` runs."""
        meds, _ = device_medians_and_minima(self.sys, (1, 2, 3, 7), ())
        self.co2_bc = self.pp.sechenov_co2_scaled(*meds)
        self.sys.set_bcs(*pore_dirichlet(self.pp, self.bnd, self.co2_bc, stern=True))

    def pore_programme(self, verbose=False, **par):
        """Marches the electrode potential through the programme ``par`` (the ``pore_programme`` keyword of ``__init__``) from the
        run's CURRENT state, on a clock of its own from 0 (gmpnp_amd/programme.py: ``run_programme`` over ``DeviceProgrammeOps`` with
        the Sechenov glue behind every accepted step and the wall profile beside the trace).  Newton and the linear solver are the
        run's own ``solver_parameters``, inv_dt = 1 / h, seconds are converted with ``pp.time_constant``
        (``impedance.pore_sigma_from_frequency`` documents the relation), the tolerances and ``max_steps`` are the run's.  The run's
        own inv_dt is put back afterwards; the run and the handle end at the programme's last potential.  Returns the arrays of
        ``pore_programme.npz`` plus ``log``, ``states`` (segment, time_s, (nv, nf) values at the breakpoints and at the end) and
        ``metadata`` (the ``pore_programme_*`` keys)."""
        import math
        from . import programme as prg
        from .timestep import TimeStepPolicy
        if self.stern is None:
            raise ValueError("pore_programme: a potential programme needs an electrode potential (electrode_voltage)")
        if self.galvanostat is not None:
            raise ValueError("pore_programme: not available with target_current (the galvanostat owns the potential)")
        if self.glue != "host" or self._levels is not None or self.rank is not None:
            raise ValueError("pore_programme: the programme runs on one unpartitioned handle without the multilevel term (host glue)")
        par = prg.check_pore_programme(par, dict(electrode_voltage=self.stern.p_electrode, kinetics=self.kinetics),
                                       self.dt_order)
        pp = self.pp
        edges = prg.resolve_bins(par["bins"], self.wall_node_z(), pp.L)
        segs = prg.build(par, float(self.stern.p_electrode), pp.time_constant, pp.thermal_voltage)
        inv_dt = float(self.sys.problem.model.inv_dt)
        policy = TimeStepPolicy(h_min=float(self.dt_bounds[0]), h_max=math.inf if self.dt_bounds[1] is None else float(self.dt_bounds[1]))
        ops = prg.DeviceProgrammeOps(self, self.solver_parameters, lambda h: 1.0 / h, self.dt_tol, par.get("capacity") or 4096,
                                     after_accept=self.sechenov_glue, profile_edges=edges)
        try:
            res = prg.run_programme(ops, segs, policy, dt_init=par.get("dt_init") or pp.dt, dt_restart=par.get("dt_restart"),
                                    steps_per_segment=par.get("steps_per_segment"), max_attempts=self.max_steps)
            rec = ops.records()
            prof = ops.profile_records()
            last = self.sys.vertex_values()
        except BaseException:   # back to the last accepted state, no trace or profile left open
            ops.abort()
            raise
        finally:
            self.sys.set_time_step(inv_dt)
        out = prg.pore_output_arrays(pp, self._eps_0(), self.wall_area(), rec, prof, ops.segments, segs, par.get("cycles", 1))
        if verbose:
            print("pore_programme %s: %d accepted steps, %d attempts, %s" % (par["kind"], len(rec), len(res["log"]), res["stop_reason"]))
        states = list(ops.states)
        t_last = res["times"][-1] if res["times"] else 0.0
        if not states or states[-1][1] != t_last:   # the run ended between two breakpoints (max_steps, h_min): its last state is kept too
            states.append((ops.segments[-1] if ops.segments else 0, t_last, last))
        n = len(rec)
        meta = {"pore_programme_kind": par["kind"], "pore_programme_cycles": int(par.get("cycles", 1)), "pore_programme_segments": len(segs),
                "pore_programme_steps_accepted": int(n), "pore_programme_steps_rejected": int(len(res["log"]) - n),
                "pore_programme_stop_reason": res["stop_reason"], "pore_programme_t_reached": float(t_last * pp.time_constant),
                "pore_programme_newton_iterations": int(ops.newton_iterations),
                "pore_programme_charge_closure": float(rec["Q_D"][-1] - (rec["D"][-1] - ops.D_first)) if n else 0.0,
                "pore_programme_status": (int(np.bitwise_or.reduce(rec["status"])) | int(np.bitwise_or.reduce(prof["status"].ravel()))) if n else 0,
                "pore_programme_electrode_voltage": float(self.stern.p_electrode),
                "pore_programme_potential_OHP": float(out["potential_OHP"][-1]) if n else None,
                "pore_programme_surface_charge": float(out["surface_charge"][-1]) if n else None,
                "pore_programme_bins": int(len(edges) - 1)}
        assert set(meta) == set(prg.PORE_METADATA_KEYS)
        out.update(log=prg.log_arrays(res["log"]), states=[(k, t * pp.time_constant, v) for k, t, v in states], metadata=meta)
        return out

    def pore_programme_outputs(self, newpath):
        """``pore_programme.npz``, ``pore_programme_states.npz`` and the attempts for ``timestep_log.npz``; returns (metadata keys, log
        arrays)."""
        out = self.pore_programme(**self.pore_programme_par)
        meta, log, states = out.pop("metadata"), out.pop("log"), out.pop("states")
        np.savez(os.path.join(newpath, "pore_programme.npz"), **out)
        np.savez(os.path.join(newpath, "pore_programme_states.npz"), segment=np.array([k for k, _, _ in states], dtype=np.int64),
                 time_s=np.array([t for _, t, _ in states]), states=np.stack([v for _, _, v in states]), coor=self.mesh.coords)
        return meta, {"pore_programme_" + k: v for k, v in log.items()}

    def wall_area(self):
        X = self.problem.coords[self.problem.wall_facets]
        return float((0.5 * np.linalg.norm(np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]), axis=1)).sum())

    def kinetics_summary(self):
        """Per-step wall means ``i_CO``, ``i_H2`` [A/m2] and ``FE_H2`` of a run with the surface kinetics (sum_I w_I = the wall area)."""
        from .kinetics import current_summary
        area = self.wall_area()
        rows = [current_summary(c, area) for c in self.currents]
        out = {k: np.array([r[k] for r in rows]) for k in ("i_CO", "i_H2", "FE_H2")}
        if self.galvanostat is not None:
            out["electrode_voltage"] = np.array(self.potentials)
        return out

    # ---- outputs (3D:860-1085) -------------------------------------------------------------------
    def write_outputs(self, stamp=None):
        pp, mesh, k = self.pp, self.mesh, self.kwargs
        names = ["H", "OH", "HCO3", "CO32", "CO2", "CO", "H2", "cat", "p"]
        if self.glue == "device":
            # the global history, assembled once on rank 0 field by field (one field's rows per gather); other ranks write nothing
            H = {nme: self.field_history(i) for i, nme in enumerate(names)}
            if self.rank not in (None, 0):
                return None
            last = np.stack([H[nme][-1] for nme in names], axis=1)
        else:
            hist = np.stack(self.history)  # (steps+1, nv, 9)
            H = {nme: hist[:, :, i] for i, nme in enumerate(names)}
            last = hist[-1]
        stamp = stamp or datetime.now().strftime("%y-%m-%d-%H-%M-%S")
        end_time = datetime.now().strftime("%y-%m-%d-%H-%M-%S")
        L, R = pp.L, pp.R
        head = "v_" + str(pp.voltage_scaled) if self.stern is None else "electrode_" + str(self.stern.p_electrode) + "_" + self.stern.model
        if self.target_current is not None:   # a galvanostatic run is named by its target: no collision with a potentiostatic run's directory
            head = "target_current_" + str(self.target_current) + "_" + self.stern.model
        identifier = (head + "_L_" + str(int(L * 1e+9)) + "_R_" + str(int(R * 1e+9))
                      + "_P_g_" + str(k.get("press_gas", 1.0)) + "_D_eff_" + str(k.get("pore_geom_multiplier", 1.0))
                      + "_Re_" + str(k.get("electrolyte_flow_geom_multiplier", 1.0))
                      + "_rough_" + str(k.get("roughness_factor", 150.0)))
        newpath = os.path.join(output_root(), stamp + "_experiment", identifier) + "/"
        os.makedirs(newpath, exist_ok=True)
        for fname, col in (("CO", 5), ("K", 7), ("H2", 6), ("CO2", 4), ("OH", 1), ("H", 0), ("HCO3", 2), ("CO32", 3),
                           ("p", 8)):
            write_pvd(os.path.join(newpath, "solution_" + fname + ".pvd"), mesh.coords, mesh.cells, last[:, col],
                      "f_" + fname)
        # project(+-grad(u_n), W).compute_vertex_values(): flat, component-major (3D:884-909)
        grads = {}
        for i, nme in enumerate(names[:8]):
            grads[nme] = self.sys.project_gradient(last[:, i]).T.ravel()
        field_values = self.sys.project_gradient(last[:, 8], sign=-1.0).T.ravel()
        tau_array = np.linspace(0, pp.T, self.tot_num_steps) if self.stepper is None else np.array(self.times)
        np.savez(newpath + "arrays_unscaled.npz", H=H["H"], OH=H["OH"], HCO3=H["HCO3"], CO32=H["CO32"], CO2=H["CO2"],
                 CO=H["CO"], H2=H["H2"], cat=H["cat"], p=H["p"], coor=mesh.coords, tau=tau_array,
                 field_values=field_values, H_grad=grads["H"], OH_grad=grads["OH"], HCO3_grad=grads["HCO3"],
                 CO32_grad=grads["CO32"], CO2_grad=grads["CO2"], CO_grad=grads["CO"], H2_grad=grads["H2"],
                 cat_grad=grads["cat"], **(self.kinetics_summary() if self.kinetics is not None else {}))
        sc = {}
        for nme, sp in zip(names[:8], pp.species):
            sc[nme] = scale_conc_time(species=sp, C=H[nme], grad_c=grads[nme], bulk_conc=pp.bulk_conc, tau=tau_array,
                                      diff_coeff_eff=pp.diff_coeff_eff, L=L)
        c = {nme: sc[nme][0] for nme in sc}
        psi = H["p"] * pp.thermal_voltage
        nw = pp.n_water
        w = (nw[pp.cation] * c["cat"] + nw["H"] * c["H"]) * 1.0e-3
        eps_rel_conc_ss = pp.eps_rel * ((55 - w) / 55) + 6 * (w / 55)
        charge_density = c["cat"][-1] - c["HCO3"][-1] - 2 * c["CO32"][-1] - c["OH"][-1] + c["H"][-1]
        np.savez(newpath + "arrays_scaled.npz", coor_scaled=mesh.coords * L, psi=psi,
                 t_H=sc["H"][1], c_H=c["H"], t_OH=sc["OH"][1], c_OH=c["OH"], t_HCO3=sc["HCO3"][1], c_HCO3=c["HCO3"],
                 t_CO32=sc["CO32"][1], c_CO32=c["CO32"], t_CO2=sc["CO2"][1], c_CO2=c["CO2"], t_CO=sc["CO"][1],
                 c_CO=c["CO"], t_H2=sc["H2"][1], c_H2=c["H2"], t_cat=sc["cat"][1], c_cat=c["cat"],
                 eps_rel=eps_rel_conc_ss, field_values=field_values * pp.thermal_voltage / L,
                 charge_density=charge_density, H_grad=sc["H"][2], OH_grad=sc["OH"][2], HCO3_grad=sc["HCO3"][2],
                 CO32_grad=sc["CO32"][2], CO2_grad=sc["CO2"][2], CO_grad=sc["CO"][2], H2_grad=sc["H2"][2],
                 cat_grad=sc["cat"][2])
        metadata_dict = {
            "concentration_elec": k.get("concentration_elec", 1.0), "cation": pp.cation,
            "voltage_multiplier": pp.voltage_scaled, "H2_FE": k.get("H2_FE", 0.05), "L": L, "R": R,
            "time_step": pp.time_step, "total_sim_time": pp.total_sim_time, "porosity": k.get("porosity_eff", 0.5),
            "tortuosity": k.get("tortuosity_eff", 1.5), "constrictivity": k.get("constrictivity_eff", 0.9),
            "y_CO2": k.get("y_CO2", 0.95), "press_gas": k.get("press_gas", 1.0),
            "pore_geom_multiplier": k.get("pore_geom_multiplier", 1.0),
            "electrolyte_flow_geom_multiplier": k.get("electrolyte_flow_geom_multiplier", 1.0), "end_time": end_time,
            "eq_conc_CO": pp.eq_conc_CO, "eq_conc_H2": pp.eq_conc_H2, "current_planar": pp.current_planar,
            "CO2_min": self.CO2_min,
            # additions of this backend (new keys only)
            "newton_iterations": int(sum(self.newton_its)), "krylov_iterations": int(self.sys.krylov_iterations),
            "num_steps_run": int(self.n)}
        if self.step_fraction:
            metadata_dict["step_fraction"] = self.step_fraction
        # after the schedule, in front of everything that reads the handle: the metadata reports the state the programme ends at
        programme = self.pore_programme_outputs(newpath) if self.pore_programme_par is not None else None
        if self.stern is not None:
            metadata_dict.update(self.stern_summary())
        if self.kinetics is not None:
            from .kinetics import tafel_parameters
            metadata_dict.update(tafel_parameters(self.kinetic_par))
            metadata_dict.update({key: (float(v[-1]) if len(v) else None) for key, v in self.kinetics_summary().items()})
        if self.galvanostat is not None:
            metadata_dict["target_current"] = self.target_current
        if self.budget is not None:
            metadata_dict.update(self.budget.save(newpath))
        if self.stepper is not None:
            self.stepping.save(newpath, metadata_dict)
        if programme is not None:
            metadata_dict.update(programme[0])
            log_path = os.path.join(newpath, "timestep_log.npz")
            with_schedule = dict(np.load(log_path)) if os.path.exists(log_path) else {}
            np.savez(log_path, **with_schedule, **programme[1])
            metadata_dict["timestep_log"] = "timestep_log.npz"
        if self.pore_impedance_par is not None:   # at the run's last state, before the polarisation curve moves the handle
            metadata_dict.update(self.pore_impedance_outputs(newpath))
        if self.polarisation_par is not None:   # last: the handle leaves the run's operating point
            metadata_dict.update(self.polarisation_outputs(newpath))
        with open(newpath + "metadata.json", "w") as fh:
            fh.write(json.dumps(metadata_dict, indent=0))
        return newpath


def solveEDL(concentration_elec=1.0, voltage_multiplier=None, H2_FE=0.05, current_rough=3000.0, L=100.0e-9,
             cation="K", R=5.0e-9, press_gas=1.0, pore_geom_multiplier=1.0, porosity_eff=0.5, tortuosity_eff=1.5,
             constrictivity_eff=0.9, params_file="parameters_pore", y_CO2=0.95, electrolyte_flow_geom_multiplier=1.0,
             roughness_factor=150.0, num_steps=None, as_published=False, verbose=True, refine=0, multilevel=False, partition=None,
             device_kwargs=None, glue="host", budget=False, step_fraction=0.0, electrode_voltage=None, stern_model="BDM", stern_length=4.0e-10,
             stern_eps_surface=6.0, kinetics=None, i0_CO=None, i0_H2=None, alpha_CO=0.5, alpha_H2=0.5, p_eq_CO=0.0, p_eq_H2=0.0, target_current=None, polarisation=None,
             pore_impedance=None, pore_programme=None, **adaptive):
    """Same keyword surface as the reference's ``solveEDL`` (3D:96-113); returns the output directory.  Additions:
    ``num_steps``, ``as_published``, ``refine`` (uniform refinements of the mesh file), ``multilevel`` (with ``refine`` > 0: the
    geometric multilevel term of the preconditioner), ``partition`` / ``device_kwargs`` / ``glue`` / ``budget`` as ``PoreRun`` takes them (with
    one rank per process only rank 0 writes and returns the directory; the others return None); ``adaptive``: the adaptive-stepping
    keywords of ``PoreRun`` (adaptive_dt, dt_rtol, dt_atol, dt_init, dt_min, dt_max, t_end, steady_tol, max_steps).
    ``voltage_multiplier`` = None is the reference's default -1.0, unless ``electrode_voltage`` (with ``stern_model``, ``stern_length``,
    ``stern_eps_surface``: the Stern boundary condition of ``PoreRun``) takes its place."""
    stern = {}
    if electrode_voltage is not None:
        stern = dict(electrode_voltage=electrode_voltage, stern_model=stern_model, stern_length=stern_length, stern_eps_surface=stern_eps_surface)
    elif voltage_multiplier is None:
        voltage_multiplier = -1.0
    if kinetics is not None:   # (the surface kinetics of ``PoreRun``)
        stern.update(kinetics=kinetics, i0_CO=i0_CO, i0_H2=i0_H2, alpha_CO=alpha_CO, alpha_H2=alpha_H2, p_eq_CO=p_eq_CO, p_eq_H2=p_eq_H2)
    if target_current is not None:   # (the galvanostatic mode of ``PoreRun``)
        stern.update(target_current=target_current)
    if polarisation:   # (the polarisation curve of ``PoreRun``, after the last step)
        stern.update(polarisation=polarisation)
    if pore_impedance:   # (the impedance spectrum of ``PoreRun``, at the last state)
        stern.update(pore_impedance=pore_impedance)
    if pore_programme:   # (the potential programme of ``PoreRun``, after the last step)
        stern.update(pore_programme=pore_programme)
    run = PoreRun(**stern, num_steps=num_steps, as_published=as_published, refine=refine, multilevel=multilevel, partition=partition,
                  device_kwargs=device_kwargs, glue=glue, budget=budget, step_fraction=step_fraction, **adaptive, concentration_elec=concentration_elec,
                  voltage_multiplier=voltage_multiplier, H2_FE=H2_FE, current_rough=current_rough, L=L, cation=cation,
                  R=R, press_gas=press_gas, pore_geom_multiplier=pore_geom_multiplier, porosity_eff=porosity_eff,
                  tortuosity_eff=tortuosity_eff, constrictivity_eff=constrictivity_eff, params_file=params_file,
                  y_CO2=y_CO2, electrolyte_flow_geom_multiplier=electrolyte_flow_geom_multiplier,
                  roughness_factor=roughness_factor)
    try:
        run.run(verbose)
        return run.write_outputs()
    finally:
        run.sys.close()


def build_parser():
    """Flags, defaults and types of reference 3D:1089-1233."""
    p = argparse.ArgumentParser(description="experiment parameters")
    for name, default in (("concentration_elec", 1.0), ("voltage_multiplier", None), ("H2_FE", 0.05),
                          ("current_rough", 3000.0), ("L", 100e-9), ("R", 5e-9)):
        p.add_argument("--" + name, required=False, default=default, type=float)
    p.add_argument("--cation", required=False, default="K", type=str)
    for name, default in (("porosity_eff", 0.5), ("tortuosity_eff", 1.5), ("constrictivity_eff", 0.9),
                          ("press_gas", 1.0), ("pore_geom_multiplier", 1.0), ("electrolyte_flow_geom_multiplier", 1.0)):
        p.add_argument("--" + name, required=False, default=default, type=float)
    p.add_argument("--params_file", required=False, default="parameters_pore", type=str)
    p.add_argument("--y_CO2", required=False, default=0.95, type=float)
    p.add_argument("--roughness_factor", required=False, default=150.0, type=float)
    # additions (not in the reference)
    p.add_argument("--num_steps", required=False, default=None, type=int, help="run only the first N time steps")
    p.add_argument("--as_published", action="store_true", help="drop the ds(2)/ds(3) flux terms (SURVEY Q1)")
    p.add_argument("--refine", required=False, default=0, type=int, help="uniform (red) refinements of the mesh file, markers inherited")
    p.add_argument("--multilevel", action="store_true", help="with --refine > 0: geometric multilevel term of the preconditioner over the nested meshes")
    p.add_argument("--partitions", required=False, default=None, type=int,
                   help="solve on N mesh partitions: all in this process on one GPU, or one rank per process under torch.distributed.run "
                        "(WORLD_SIZE = N; rank 0 prints and writes)")
    p.add_argument("--budget", action="store_true", help="record the species budgets and consistent boundary fluxes of every step (budget.npz)")
    p.add_argument("--step_fraction", required=False, default=0.0, type=float,
                   help="fraction-to-boundary step limiter of the Newton update: tau in (0, 1), 0 = off (not with --partitions)")
    add_adaptive_arguments(p)   # (not with --partitions)
    add_stern_arguments(p)      # (not with --partitions / --multilevel; --voltage_multiplier defaults to -1.0 without --electrode_voltage)
    add_kinetics_arguments(p)   # (with --electrode_voltage; not with --partitions / --multilevel)
    add_polarisation_arguments(p)  # (with --electrode_voltage; not with --partitions / --multilevel / --target_current / --dt_order 2)
    add_galvanostat_arguments(p)   # (with --kinetics tafel; not with --partitions / --multilevel / --dt_order 2)
    add_pore_impedance_arguments(p)   # (with --electrode_voltage; not with --partitions / --multilevel)
    add_pore_programme_arguments(p)   # (with --electrode_voltage; not with --partitions / --multilevel / --target_current / --polarisation / --dt_order 2)
    return p


def partition_setup(nparts):
    """(partition, device_kwargs, torch.distributed or None) of ``--partitions nparts``.  Without torch.distributed.run: every
    partition in this process on one GPU.  Under it (WORLD_SIZE == nparts): one rank per process on device LOCAL_RANK, RCCL between
    the ranks; ranks that share a card (more local ranks than visible devices) run as ``shared_device`` handles over the
    host-staged transport on gloo (RCCL takes one rank per device)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world <= 1:
        return (nparts, None), {}, None
    if world != nparts:
        raise SystemExit("--partitions %d under torch.distributed.run needs WORLD_SIZE == %d (it is %d)" % (nparts, nparts, world))
    import torch   # before libgmpnp.so (README: two HIP runtimes on one GPU do not mix)
    from .dist import init_process_group_from_env
    ndev = max(1, torch.cuda.device_count())
    shared = int(os.environ.get("LOCAL_WORLD_SIZE", world)) > ndev
    local = int(os.environ.get("LOCAL_RANK", "0")) % ndev
    rank, _, _, tdist = init_process_group_from_env("gloo" if shared else "nccl", device=local)
    return (nparts, rank), {"device_id": local, "shared_device": int(shared), "transport": "host" if shared else "rccl"}, tdist


def main(argv=None):
    a = build_parser().parse_args(argv)
    extra, tdist = {}, None
    if a.partitions and a.adaptive_dt:
        raise ValueError("--adaptive_dt: adaptive time stepping is not available with --partitions")
    if a.partitions and a.electrode_voltage is not None:
        raise ValueError("--electrode_voltage: the Stern boundary condition is not available with --partitions")
    if a.partitions and a.kinetics is not None:
        raise ValueError("--kinetics: the surface kinetics are not available with --partitions")
    if a.partitions and a.target_current is not None:
        raise ValueError("--target_current: the galvanostat is not available with --partitions")
    if a.electrode_voltage is not None and a.voltage_multiplier is not None:
        raise ValueError("--electrode_voltage takes the place of --voltage_multiplier: give one of them")
    if a.partitions:
        partition, device_kwargs, tdist = partition_setup(a.partitions)
        extra = dict(partition=partition, device_kwargs=device_kwargs, glue="device", verbose=partition[1] in (None, 0))
    try:
        return solveEDL(concentration_elec=a.concentration_elec, voltage_multiplier=a.voltage_multiplier, H2_FE=a.H2_FE,
                        current_rough=a.current_rough, L=a.L, R=a.R, press_gas=a.press_gas, cation=a.cation,
                        porosity_eff=a.porosity_eff, tortuosity_eff=a.tortuosity_eff,
                        constrictivity_eff=a.constrictivity_eff, params_file=a.params_file, y_CO2=a.y_CO2,
                        pore_geom_multiplier=a.pore_geom_multiplier,
                        electrolyte_flow_geom_multiplier=a.electrolyte_flow_geom_multiplier,
                        roughness_factor=a.roughness_factor, num_steps=a.num_steps, as_published=a.as_published, refine=a.refine,
                        multilevel=a.multilevel, budget=a.budget, step_fraction=a.step_fraction, **adaptive_keywords(a), **stern_keywords(a), **kinetics_keywords(a), **galvanostat_keywords(a), **polarisation_keywords(a), **pore_impedance_keywords(a), **pore_programme_keywords(a), **extra)
    finally:
        if tdist is not None:
            tdist.barrier()
            tdist.destroy_process_group()


if __name__ == "__main__":
    main()
