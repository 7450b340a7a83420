"""1D electrical-double-layer GMPNP/PNP driver on the MI355X backend — same CLI flags, inputs and output layout as
reference 1D/MPNP_CO2ER_EDL.py (``solve_EDL`` 1D:66-989, CLI 1D:992-1118).

Kept quirks: ``--dry_run`` is ``type=bool`` so any value given on the command line is truthy; in
non-dry-run mode the form keeps the first time step while ``t`` advances by the second (Q2) — here: the model's
``inv_dt`` is never changed after the first stage; the run then ends with NameError for ``time_step`` as the
reference does (Q3).  ``--stabilization Y`` (1D:597-722): for MPNP the reference only prints a warning and solves the
unstabilised form, which is what happens here; for PNP the SUPG terms are added on the device (``gmpnp_set_supg``) with
the nodal parameters recomputed every step from the previous potential (``solver.supg_parameters``).  Paths: ``$GMPNP_UTILITIES`` / ``$GMPNP_OUT`` (Q10).

``--adaptive_dt`` (not a reference feature): backward Euler with the step chosen by the error controller of gmpnp_amd/timestep.py,
``inv_dt = 1/(h L_D)``.  The staged schedule and Q2 do not apply in adaptive mode: there is one clock, the controller's, from 0 to
``--t_end`` (default: the end of the driver's own schedule) or to the steady stop (``--steady_tol``)."""
from __future__ import annotations

import argparse
import copy
import dataclasses
import json
import math
import os
from datetime import datetime

import numpy as np

from . import backend
from .impedance import add_impedance_arguments, impedance_keywords
from .polarisation import add_polarisation_arguments, polarisation_keywords
from .fit import add_fit_arguments, fit_keywords, programme_fit_keywords
from .programme import add_programme_arguments, programme_keywords
from .mesh import read_dolfin_xml, resolve_mesh_path
from .params import _load_yaml, edl_parameters, utilities_dir
from .problem import (Galvanostat, add_galvanostat_arguments, add_kinetics_arguments, add_stern_arguments, edl_problem, galvanostat_keywords, kinetics_keywords,
                      pop_galvanostat, pop_kinetics, pop_stern, stern_keywords)
from .solver import GMPNPSystem, supg_parameters
from .timestep import adaptive_keywords, add_adaptive_arguments

SOLVER_PARAMETERS = {  # reference 1D:357-364
    "nonlinear_solver": "newton",
    "newton_solver": {"maximum_iterations": 50, "relative_tolerance": 1.0e-4, "absolute_tolerance": 1.0e-4},
}
from .polarisation import NEWTON as POLARISATION_NEWTON  # noqa: E402 (the Newton solves of a polarisation curve)


def scale(species="H", tau=None, C=None, initial_conc=None, diff_coeff=None, L_n=0.0, L_debye=0.0):
    """reference 1D:51-63"""
    t = (tau * L_debye * L_n) / diff_coeff[species]
    c = C * initial_conc[species]
    return t, c


def output_root():
    return os.environ.get("GMPNP_OUT", os.path.join(os.getcwd(), "out"))


class EDLRun:
    def __init__(self, num_steps=None, device_kwargs=None, solver_parameters=None, budget=False, step_fraction=0.0, adaptive_dt=False,
                 dt_rtol=1e-2, dt_atol=1e-4, dt_init=None, dt_min=0.0, dt_max=None, t_end=None, steady_tol=0.0, max_steps=None, dt_order=1,
                 **kwargs):
        """``budget`` = True: every step records its species-budget table; ``write_outputs`` adds ``budget.npz`` (gmpnp_amd/budget.py).
        ``step_fraction`` = tau in (0, 1): the Newton updates go through the fraction-to-boundary step limiter
        (``newton_solver["step_fraction"]``, include/gmpnp.h; not a reference feature); 0 = off, the reference's plain Newton.
        ``adaptive_dt`` = True: the step size is the error controller's (gmpnp_amd/timestep.py; all times in the driver's scaled
        units): ``dt_rtol`` / ``dt_atol`` its weights, ``dt_init`` the first step (default: the reference step), ``dt_min`` /
        ``dt_max`` its bounds, ``t_end`` the end time (default: the end of the schedule), ``steady_tol`` > 0 the steady stop,
        ``max_steps`` the largest number of attempted steps, ``dt_order`` = 2 variable-step BDF2 in backward Euler's place (after its
        start-up; the log gets an ``order`` column and the metadata ``dt_order``).  A rejected step leaves the clock, the history, the budget log and the
        SUPG parameters as they were.  Not with ``H_OHP``: its multiplicative flux controller is calibrated per fixed step
        (ValueError, before anything touches the device).  Off: nothing changes.
        ``electrode_voltage`` = X (thermal voltages; in place of ``voltage_multiplier``, giving both is a ValueError): the electrode
        potential is applied through the Stern-layer boundary condition (``stern_model`` "BDM" or "linear",
        ``stern_length`` 4e-10 m, ``stern_eps_surface`` 6): the OHP potential becomes a result.  Not with ``stabilization`` "Y" and not with
        ``H_OHP`` (ValueError, before anything touches the device).  The metadata gains ``electrode_voltage``, ``stern_model``,
        ``stern_length``, ``stern_displacement`` (the integrated Stern term g (p_M - p) / lam of the last state, scaled units) and
        ``surface_charge`` [C/m2] = eps_0 thermal_voltage / L_n x stern_displacement: the displacement eps_0 eps_r E pointing from the
        electrode into the electrolyte, i.e. the charge per area ON THE ELECTRODE (negative for a cathode, p_M < p_OHP).
        ``kinetics`` = "tafel" (with ``electrode_voltage``; ``i0_CO`` / ``i0_H2`` [A/m2] required, ``alpha_CO`` / ``alpha_H2`` = 0.5,
        ``p_eq_CO`` / ``p_eq_H2`` = 0 thermal voltages): the currents of CO2 -> CO and of the hydrogen evolution follow the potential
        drop across the Stern layer and the CO2 concentration at the OHP (gmpnp_amd/kinetics.py) in place of the
        prescribed ``current_OHP_ss`` / ``H2_FE``, which are then unused for the CO2, OH and H fluxes.  Not with ``stabilization`` "Y"
        and not with ``H_OHP`` (ValueError, before anything touches the device).  Every step records ``i_CO``, ``i_H2`` [A/m2] and
        ``FE_H2`` (arrays_unscaled.npz; the last values and the kinetic parameters in the metadata).
        ``target_current`` = X [A/m2] (with ``kinetics``): galvanostatic mode: every Newton solve also finds the
        electrode potential at which i_CO + i_H2 = X; ``electrode_voltage`` is the starting guess.  Works with ``step_fraction``,
        ``budget`` and ``adaptive_dt`` at order 1 (a rejected attempt restores the potential with the state); not with ``dt_order`` 2.
        Every step records ``electrode_voltage`` beside the currents; the metadata gains ``target_current`` and reports the last
        potential found as ``electrode_voltage``; the run directory is named by the target.
        ``impedance`` = dict(freq_min=1e-2, freq_max=1e8, per_decade=10) [Hz] (with ``electrode_voltage``): ``write_outputs`` computes the
        impedance spectrum of the interface at the run's last state (gmpnp_amd/impedance.py; ``impedance()``
        does the same at any time) and adds ``impedance.npz`` (frequency, sigma, capacitance [F/m2], admittance [S/m2], impedance
        [Ohm m2], dI_CO, dI_H2 [S/m2], residual); the metadata gains ``impedance_points``, ``capacitance_low`` / ``capacitance_high``
        (the real part of C at the lowest / highest frequency), ``capacitance_high_closed_form`` (the Stern capacitor in series with
        the elements'), ``R_ct`` [Ohm m2] (None without kinetics) and ``impedance_last_step_change`` = max |u - u_n| of the last step:
        how steady the operating point was.
        ``polarisation`` = dict(v_end=X, v_step=Y[, params=(0, ...)]) (thermal voltages; with ``electrode_voltage``): ``write_outputs``
        walks the steady-state polarisation curve from the run's last state and potential to ``v_end`` (DESIGN.md section 5l,
        gmpnp_amd/polarisation.py; ``polarisation()`` does the same at any time) and adds ``polarisation.npz``; the metadata gains
        ``polarisation_points``, ``polarisation_v_end``, ``polarisation_v_step``, ``polarisation_stop_reason``,
        ``polarisation_newton_iterations``, ``polarisation_substeps``, ``polarisation_worst_residual`` and ``polarisation_params``.
        Not with ``target_current``, ``stabilization`` "Y", ``H_OHP`` or ``dt_order`` 2 (ValueError, before anything touches the
        device).  The run should have reached its steady state (``adaptive_dt`` with ``steady_tol``): the first point is one Newton
        solve at inv_dt = 0 from the last state.
        ``fit`` = dict(data=path[, params=("i0_CO", "i0_H2", "alpha_CO", "alpha_H2")]) (with ``kinetics``): ``write_outputs`` fits the named
        electrode parameters (also ``stern_length``) to the polarisation data of the file (gmpnp_amd/fit.py;
        ``fit()`` does the same at any time), after the impedance and before the polarisation curve, which is then the fitted one;
        it adds ``fit.npz`` and the metadata keys ``fit_*``.  Afterwards the run stands at ``electrode_voltage`` with the fitted
        parameters at the steady state there.  Refused as ``polarisation`` is, and without ``kinetics``.
        ``programme`` = dict(kind="pulse", v_levels=[A, B], durations=[s, s], cycles=n[, rise_time=s]) | dict(kind="triangle", v_vertex=X,
        scan_rate=V/s, cycles=n) | dict(kind="table", time_s=[...], electrode_voltage=[...]) (potentials in thermal voltages; with
        ``electrode_voltage``; also dt_init, dt_restart [scaled time], steps_per_segment, capacity): ``write_outputs`` marches the
        electrode potential through the waveform AFTER the run's own schedule, from its last state, on a clock of its own that starts
        at 0 (gmpnp_amd/programme.py; ``programme()`` does the same at any time); it is meant to follow
        ``adaptive_dt`` with ``steady_tol``.  Steps land on the corners and jumps of the waveform; the error controller (the run's
        ``dt_rtol`` / ``dt_atol`` / ``dt_min`` / ``dt_max``) starts again behind a jump.  Per accepted step the device forms one record
        of the interface (``gmpnp_electrode_trace_append``); full states are kept at the breakpoints only.  Adds ``programme.npz``
        (``programme.OUTPUT_KEYS``), ``programme_states.npz``, the attempts as ``programme_*`` arrays of ``timestep_log.npz`` and the
        metadata keys ``programme_*``; works with ``kinetics``, ``step_fraction`` and ``budget`` (a row per accepted step).  Afterwards
        the run stands at the programme's last potential (``stern``, ``kinetics``, the metadata's ``electrode_voltage``), and
        ``impedance`` is taken there.  Not with ``target_current``, ``polarisation``, ``fit``, ``stabilization`` "Y", ``H_OHP`` or
        ``dt_order`` 2 (ValueError, before anything touches the device)."""
        from .programme import refuse_pore_programme
        refuse_pore_programme(kwargs, "the 1D driver", " (its electrode record is the profile: use programme)")
        self.programme_par = kwargs.pop("programme", None) or None
        if self.programme_par is not None:
            from .programme import check_programme
            self.programme_par = check_programme(self.programme_par, kwargs, dt_order)
        # ``fit_programme`` = dict(data=path[, params=(...)]) (with ``programme`` in fixed mode and ``kinetics``): ``write_outputs`` fits the
        # named electrode parameters to the transient data of the file (time_s, i_CO and / or i_H2[, surface_charge, weight_*]; what
        # ``programme.npz`` holds) over the programme, BEFORE the programme itself is marched with the fitted parameters (DESIGN.md
        # section 5p; ``fit_programme()`` does the same at any time); it adds ``fit_programme.npz`` (``fit.npz``'s tables over time_s) and
        # the metadata keys ``fit_programme_*``.  Not with ``fit`` or ``polarisation``, nor where the programme is refused.
        self.fit_programme_par = kwargs.pop("fit_programme", None) or None
        if self.fit_programme_par is not None:
            from .fit import check_fit_programme
            self.fit_programme_par = check_fit_programme(self.fit_programme_par, dict(kwargs, programme=self.programme_par), dt_order)
        self.programme_state = None   # the state a programme ended at (impedance_outputs reads it in the place of the history's last row)
        self.dt_tol, self.dt_bounds, self.max_steps = (dt_rtol, dt_atol), (dt_min, dt_max), max_steps
        self.fit_par = kwargs.pop("fit", None) or None
        if self.fit_par is not None:
            from .fit import check_fit
            self.fit_par = check_fit(self.fit_par, kwargs, dt_order)
        self.polarisation_par = kwargs.pop("polarisation", None) or None
        if self.polarisation_par is not None:
            from .polarisation import check_polarisation
            self.polarisation_par = check_polarisation(self.polarisation_par, kwargs, dt_order)
        from .impedance import refuse_pore_impedance
        refuse_pore_impedance(kwargs, "the 1D double-layer driver", hint=": its spectrum is the keyword impedance (--impedance)")
        self.impedance_par = kwargs.pop("impedance", None) or None
        if self.impedance_par is not None:
            from .impedance import frequency_grid
            if kwargs.get("electrode_voltage") is None:
                raise ValueError("impedance: the frequency response needs an electrode potential (electrode_voltage)")
            if kwargs.get("stabilization", "N") == "Y":
                raise ValueError("impedance: the frequency response is not available with stabilization Y")
            self.impedance_par = dict(self.impedance_par)
            frequency_grid(**self.impedance_par)   # a bad grid is refused before anything touches the device
        self.stern = pop_stern(kwargs, kwargs.get("L_n", 50.0e-6))
        self.kinetic_par = pop_kinetics(kwargs)
        self.target_current = pop_galvanostat(kwargs)
        if self.target_current is not None:
            if self.kinetic_par is None:
                raise ValueError("target_current: the galvanostat needs the surface kinetics (kinetics='tafel')")
            if int(dt_order) == 2:
                raise ValueError("target_current: the galvanostat is not available with dt_order 2")
            if kwargs.get("stabilization", "N") == "Y":
                raise ValueError("target_current: the galvanostat is not available with stabilization Y")
            if kwargs.get("H_OHP") is not None:
                raise ValueError("target_current: the galvanostat is not available with the H_OHP flux controller")
        if self.kinetic_par is not None:
            if self.stern is None:
                raise ValueError("kinetics: the surface kinetics need an electrode potential (electrode_voltage)")
            if kwargs.get("stabilization", "N") == "Y":
                raise ValueError("kinetics: the surface kinetics are not available with stabilization Y")
            if kwargs.get("H_OHP") is not None:
                raise ValueError("kinetics: the surface kinetics are not available with the H_OHP flux controller")
        if self.stern is not None and kwargs.get("stabilization", "N") == "Y":
            raise ValueError("electrode_voltage: the Stern boundary condition is not available with stabilization Y")
        if self.stern is not None and kwargs.get("H_OHP") is not None:
            raise ValueError("electrode_voltage: the Stern boundary condition is not available with the H_OHP flux controller")
        self.adaptive = bool(adaptive_dt)
        if self.adaptive and kwargs.get("H_OHP") is not None:
            raise ValueError("adaptive_dt: the H_OHP flux controller is calibrated per fixed step")
        self.kwargs = kwargs
        self.step_fraction = float(step_fraction)
        self.ep = edl_parameters(**kwargs)
        ep = self.ep
        stab = kwargs.get("stabilization", "N") == "Y"
        self.supg = stab and ep.model_name == "PNP"        # reference 1D:687-722
        self.warn_stab = stab and ep.model_name != "PNP"   # "Warning:stabilization not implemented for MPNP!", 1D:724-727
        self.h_vertex = None
        self.mesh = read_dolfin_xml(resolve_mesh_path(utilities_dir(), ep.mesh_name))
        self.kinetics, self.currents = None, []
        if self.kinetic_par is not None:
            from .kinetics import edl_tafel
            self.kinetics, ep.model = edl_tafel(ep, self.kinetic_par, self.stern.p_electrode)
            print("kinetics tafel: current_OHP_ss and H2_FE are not used for the CO2, OH and H fluxes at the OHP")
        self.galvanostat, self.potentials = None, []
        if self.target_current is not None:
            self.galvanostat = Galvanostat(self.target_current)   # the OHP is one point: sum_I w_I = 1
        self.problem = edl_problem(ep, self.mesh, stern=self.stern, kinetics=self.kinetics, galvanostat=self.galvanostat)
        self.model = copy.deepcopy(self.problem.model)
        self.sys = GMPNPSystem(self.problem, **(device_kwargs or {}))
        self.solver_parameters = backend.with_step_fraction(solver_parameters or SOLVER_PARAMETERS, self.step_fraction)
        self.tot_num_steps = ep.tot_num_steps if num_steps is None else int(num_steps)
        nv = self.mesh.num_vertices
        self.sys.initialise([1.0] * 6 + [0.0])
        self.history = [np.concatenate([np.ones((nv, 6)), np.zeros((nv, 1))], axis=1)]
        self.current_H_frac = ep.current_H_frac
        self.n, self.t, self.dt = 0, 0.0, ep.dts[0]
        self.newton_its = []
        self.budget = None
        if budget:
            from .budget import BudgetLog, interval_factors
            self.budget = BudgetLog(list(ep.species[:5]) + ["cat", "p"], *interval_factors(ep.species, ep.diff_coeff, ep.initial_conc, ep.L_n))
        self.stepper = None
        if self.adaptive:
            from .timestep import DriverStepping
            L_D = ep.L_D
            self.stepping = DriverStepping(self.sys, self.solver_parameters, lambda h: 1.0 / (h * L_D), ep.dts[0], ep.stage_T[-1],
                                           dt_rtol=dt_rtol, dt_atol=dt_atol, dt_init=dt_init, dt_min=dt_min, dt_max=dt_max, t_end=t_end,
                                           steady_tol=steady_tol, max_steps=max_steps, dt_order=dt_order)
            self.stepper, self.times = self.stepping.stepper, self.stepping.times   # times: the actual times of the history rows
            self._supg_stale = True    # the SUPG parameters follow u_n: recomputed after an accepted step only

    def adaptive_step(self, verbose=True):
        """One ATTEMPTED step of the adaptive run (``timestep.AdaptiveStepper.attempt``); the glue of ``step`` runs for an accepted
        step only, with ``time_accept`` in place of ``assign_previous``.  Returns the attempt's log row."""
        row = self.stepping.attempt(lambda t, h: self.adaptive_before_solve(t, h, verbose),
                                    lambda st: self.adaptive_before_accept(st, None, verbose), verbose)
        self.t = self.stepper.t
        return row

    def adaptive_before_solve(self, t, h, verbose=True):
        """Host glue of an attempted step in front of its Newton solve (also what ``EDLEnsemble`` runs per member)."""
        self.dt = h
        if self.warn_stab and verbose:
            print("Warning:stabilization not implemented for MPNP!")
        if self.supg and self._supg_stale:
            self.refresh_supg()
            self._supg_stale = False

    def adaptive_before_accept(self, st, vals=None, verbose=True):
        """Host glue of an ACCEPTED step, while u_n is the previous state and inv_dt the step's.  ``vals``: the (nv, nf) vertex
        values of u when the caller holds them already (``EDLEnsemble``: the member's row of one copy for all members)."""
        if self.budget is not None:
            self.budget.take(self.sys)
        self.accept_solution(st, self.sys.vertex_values() if vals is None else vals, verbose)
        self.newton_its.append(st["iterations"])
        self.n += 1
        self._supg_stale = True

    def refresh_supg(self):
        """rho_i from the previous step's potential (u_n), OH's strong residual with grad(u_H)."""
        ep = self.ep
        rho, self.h_vertex = supg_parameters(self.mesh.coords, self.mesh.cells, self.model.z, self.history[-1][:, 6],
                                             self.sys.project_cellwise, self.h_vertex)
        w = np.arange(6, dtype=np.int32)
        w[ep.species.index("OH")] = ep.species.index("H")
        self.sys.dev.set_supg(rho, w)

    def step(self, verbose=True):
        if self.stepper is not None:
            return self.adaptive_step(verbose)
        self.advance_clock(verbose)
        st = self.sys.solve(self.solver_parameters)
        if self.budget is not None:   # after the Newton solve, before set_model / assign_previous
            self.budget.take(self.sys)
        self.accept_solution(st, self.sys.vertex_values(), verbose)
        self.sys.assign_previous()
        self.newton_its.append(st["iterations"])
        self.n += 1
        return st

    def advance_clock(self, verbose=True):
        """Host glue of a step before its Newton solve: the clock (Q2 stage switch) and the SUPG parameters."""
        ep = self.ep
        if verbose:
            if ep.dry_run:
                print(int(self.t / self.dt))
            else:
                if self.t >= ep.stage_T[0]:
                    self.dt = ep.dts[1]  # only the clock changes: the form keeps the first Constant (Q2)
                    print(int(ep.stage_steps[0] + (self.t - ep.stage_T[0]) / self.dt))
                else:
                    print(int(self.t / self.dt))
        elif not ep.dry_run and self.t >= ep.stage_T[0]:
            self.dt = ep.dts[1]
        self.t += self.dt
        if self.warn_stab and verbose:
            print("Warning:stabilization not implemented for MPNP!")
        if self.supg:
            self.refresh_supg()

    def accept_solution(self, st, vals, verbose=True):
        """Host glue of a step after its Newton solve: the state joins the history and the H_OHP controller (reference
        1D:770-793) re-uploads the OHP fluxes.  u_n.assign(u) and the step count stay with the caller."""
        ep = self.ep
        self.history.append(vals)
        if self.kinetics is not None:
            self.currents.append(self.sys.dev.kinetics_currents())
        if self.galvanostat is not None:
            self.potentials.append(self.sys.dev.galvanostat_report()["p_electrode"])
        H_OHP_frac = vals[0, 0]
        H_OHP = ep.H_OHP
        if H_OHP is not None:  # reference 1D:770-793
            f = self.current_H_frac
            if H_OHP_frac < 0:
                f = f / 1.1
            elif H_OHP_frac < (H_OHP - 0.05):
                f = f / 1.05
            elif H_OHP_frac < (H_OHP - 0.025):
                f = f / 1.01
            elif (H_OHP_frac > H_OHP and H_OHP_frac <= (H_OHP + 0.4) and f <= 1.0):
                f = f * 1.04
            elif H_OHP_frac > (H_OHP + 0.4) and f <= 1.0:
                f = f * 1.15
            self.current_H_frac = f
            if verbose:
                print(H_OHP_frac)
                print(f)
            JH, JOH = ep.ohp_fluxes(f)
            self.model.point_flux[ep.species.index("H")] = JH
            self.model.point_flux[ep.species.index("OH")] = JOH
            self.sys.set_model(self.model)

    def run(self, verbose=True):
        if self.stepper is not None:
            self.stepping.run(lambda: self.adaptive_step(verbose))
            return self
        for _ in range(self.n, self.tot_num_steps):
            self.step(verbose)
        return self

    def ohp_summary(self):
        """field_OHP [V/nm] and eps_rel_OHP of the current state, as the reference derives them for metadata.json
        (1D:802-805 projection of -grad(p), 1D:893-954 rescaling): the two quantities 1D/Stern_CO2ER.py:66-68 records."""
        ep, mesh = self.ep, self.mesh
        last = self.history[-1]
        field = self.sys.project_gradient(last[:, 6], sign=-1.0)[:, 0] * ep.thermal_voltage / ep.L_n
        c_cat = last[0, 5] * ep.initial_conc[ep.cation]
        c_H = last[0, 0] * ep.initial_conc["H"]
        w = (ep.n_water[ep.cation] * c_cat + ep.n_water["H"] * c_H) * 1.0e-3
        return {"field_OHP": float(field[0] * 1.0e-9), "eps_rel_OHP": float(ep.eps_rel * ((55 - w) / 55) + 6 * (w / 55)),
                "potential_OHP": float(last[0, 6] * ep.thermal_voltage)}

    def stern_summary(self):
        """The metadata keys of a run with the Stern boundary condition (see ``__init__``), from the device's current state."""
        ep, st = self.ep, self.stern
        d = self.sys.dev.stern_displacement()
        EPS_0 = _load_yaml(os.path.join(utilities_dir(), self.kwargs.get("params_file", "parameters") + ".yaml"))["nat_const"]["eps_0"]
        p_M = self.potentials[-1] if self.potentials else st.p_electrode   # galvanostatic mode: the potential that was found
        return {"electrode_voltage": p_M, "stern_model": st.model, "stern_length": st.lam * ep.L_n, "stern_displacement": d,
                "surface_charge": EPS_0 * ep.thermal_voltage / ep.L_n * d}

    def impedance(self, frequencies):
        """The impedance spectrum of the interface at the run's CURRENT state and electrode potential, at ``frequencies`` [Hz]
        (gmpnp_amd/impedance.py: ``spectrum``; one ``gmpnp_frequency_response`` call).  A galvanostatic run switches its galvanostat
        off for the call (that keeps the potential it found) and on again with the same target."""
        from . import impedance as imp
        if self.stern is None:
            raise ValueError("impedance: the frequency response needs an electrode potential (electrode_voltage)")
        if self.supg:
            raise ValueError("impedance: the frequency response is not available with stabilization Y")
        f = np.atleast_1d(np.asarray(frequencies, dtype=np.float64))
        if not imp.count_valid(f.size) or not np.all(np.isfinite(f)) or np.any(f < 0.0):
            raise ValueError("impedance: 1 ... %d finite frequencies >= 0" % imp.MAX_FREQUENCIES)
        dev = self.sys.dev
        if self.galvanostat is not None:
            dev.set_galvanostat(None)
        try:
            res = dev.frequency_response(imp.sigma_from_frequency(self.ep, f))
        finally:
            if self.galvanostat is not None:
                dev.set_galvanostat(self.galvanostat)
        eps_0 = _load_yaml(os.path.join(utilities_dir(), self.kwargs.get("params_file", "parameters") + ".yaml"))["nat_const"]["eps_0"]
        return imp.spectrum(self.ep, eps_0, f, res)

    def impedance_outputs(self, newpath):
        """``impedance.npz`` of the last state and the metadata keys that go with it (see ``__init__``)."""
        from . import impedance as imp
        sp = self.impedance(imp.frequency_grid(**self.impedance_par))
        nr = sp["dI_dV"].shape[1]
        zero = np.zeros(len(sp["frequency"]), dtype=complex)
        np.savez(newpath + "/impedance.npz", frequency=sp["frequency"], sigma=sp["sigma"], capacitance=sp["capacitance"], admittance=sp["admittance"],
                 impedance=sp["impedance"], dI_CO=sp["dI_dV"][:, 0] if nr > 0 else zero, dI_H2=sp["dI_dV"][:, 1] if nr > 1 else zero,
                 residual=sp["residual"])
        eps_0 = _load_yaml(os.path.join(utilities_dir(), self.kwargs.get("params_file", "parameters") + ".yaml"))["nat_const"]["eps_0"]
        p_M = self.potentials[-1] if self.potentials else self.stern.p_electrode
        stern = type(self.stern)(self.stern.model, p_M, self.stern.lam, self.stern.eps_surface)
        last = self.history[-1] if self.programme_state is None else self.programme_state
        c_inf = imp.high_frequency_capacitance(self.mesh.coords, last, self.problem.model, stern) * eps_0 / self.ep.L_n
        g_ct = -float(sp["dI_dV"][0].sum().real) if nr else 0.0
        change = float(np.abs(self.history[-1] - self.history[-2]).max()) if len(self.history) > 1 else None
        return {"impedance_points": int(len(sp["frequency"])), "capacitance_low": float(sp["capacitance"][0].real),
                "capacitance_high": float(sp["capacitance"][-1].real), "capacitance_high_closed_form": float(c_inf),
                "R_ct": (1.0 / g_ct) if g_ct != 0.0 else None, "impedance_last_step_change": change,
                "impedance_worst_residual": float(np.max(sp["residual"])), "impedance_status": int(np.bitwise_or.reduce(sp["status"]))}

    def polarisation(self, v_end, v_step, params=(0,), predictor=True, solver_parameters=None):
        """The steady-state polarisation curve from the run's LAST state and electrode potential to ``v_end`` on the grid
        electrode_voltage + k ``v_step`` (thermal voltages; gmpnp_amd/polarisation.py: ``run_continuation``).  The time term is
        switched off (``set_time_step(0)``) and put back afterwards; one Newton solve finds the first point (RuntimeError where it
        fails: run to the steady stop first), then per point: tangent (``gmpnp_electrode_tangent`` for the parameter codes
        ``params``, p_M among them), predictor (``gmpnp_electrode_advance`` with the run's ``step_fraction``), Newton at inv_dt = 0
        (``solver_parameters``, default ``polarisation.NEWTON``-like tight tolerances, with the run's ``step_fraction``).  A failed
        attempt returns to the last converged point, kept in u_n.  The handle and the run's Stern / kinetics records end at the last
        converged potential.  Returns the arrays of ``polarisation.npz`` plus ``stop_reason``."""
        from . import polarisation as pol
        if self.stern is None:
            raise ValueError("polarisation: the curve needs an electrode potential (electrode_voltage)")
        if self.galvanostat is not None:
            raise ValueError("polarisation: the curve is not available with target_current (the galvanostat)")
        if self.supg:
            raise ValueError("polarisation: the curve is not available with stabilization Y")
        par = pol.check_polarisation(dict(v_end=v_end, v_step=v_step, params=params),
                                     dict(electrode_voltage=self.stern.p_electrode, kinetics=self.kinetic_par))
        sp = backend.with_step_fraction(solver_parameters or POLARISATION_NEWTON, self.step_fraction)
        ops = pol.DeviceOps(self, backend.newton_options(sp, dim=1), par["params"], lambda u: float(u[self.problem.nf - 1]))

        inv_dt = float(self.sys.problem.model.inv_dt)
        self.sys.set_time_step(0.0)
        try:
            records, substeps, newton, stop = pol.run_continuation(ops, self.stern.p_electrode, par["v_end"], par["v_step"], predictor)
        finally:
            self.sys.set_time_step(inv_dt)
        eps_0 = _load_yaml(os.path.join(utilities_dir(), self.kwargs.get("params_file", "parameters") + ".yaml"))["nat_const"]["eps_0"]
        out = pol.curve_arrays(self.ep, eps_0, 1.0, records, par["params"], substeps, newton)
        out["stop_reason"] = stop
        return out

    def polarisation_outputs(self, newpath):
        """``polarisation.npz`` of the curve from the last state and the metadata keys that go with it (see ``__init__``)."""
        out = self.polarisation(**self.polarisation_par)
        stop = out.pop("stop_reason")
        np.savez(newpath + "/polarisation.npz", **out)
        return {"polarisation_points": int(len(out["electrode_voltage"])), "polarisation_v_end": float(self.polarisation_par["v_end"]),
                "polarisation_v_step": float(self.polarisation_par["v_step"]), "polarisation_stop_reason": stop,
                "polarisation_newton_iterations": int(out["newton_iterations"].sum()), "polarisation_substeps": int(out["substeps"].sum()),
                "polarisation_worst_residual": float(np.max(out["tangent_residual"])),
                "polarisation_params": [int(q) for q in out["sensitivity_params"]]}

    def fit(self, data, params=None, predictor=True):
        """Fits the electrode parameters ``params`` (names of ``fit.PARAMETERS``; default the four kinetic ones) to the polarisation
        data ``data`` (a path, or a dict of the columns) by Levenberg-Marquardt on the log currents (and the surface charge, where
        given) with the tangent's exact sensitivities (gmpnp_amd/fit.py: ``LevenbergMarquardt`` over ``DeviceCurve``).  Afterwards
        the run and the handle stand at ``electrode_voltage`` with the FITTED parameters (``kinetics``, ``stern`` and the problem's
        records replaced) at the steady state there, with the run's own inv_dt put back.  Returns the arrays of ``fit.npz`` plus
        ``metadata`` (the ``fit_*`` keys) and ``result`` (``LevenbergMarquardt.run``'s)."""
        from . import fit as ft
        if self.stern is None or self.kinetics is None:
            raise ValueError("fit: the fit needs an electrode potential and the surface kinetics (electrode_voltage, kinetics='tafel')")
        if self.galvanostat is not None:
            raise ValueError("fit: the fit is not available with target_current (the galvanostat)")
        if self.supg:
            raise ValueError("fit: the fit is not available with stabilization Y")
        names = tuple(params or ft.DEFAULT_PARAMS)
        codes = ft.param_codes(names)
        V0 = float(self.stern.p_electrode)
        table = ft.check_data(ft.load_data(data) if not isinstance(data, dict) else data, V0, len(codes))
        eps_0 = _load_yaml(os.path.join(utilities_dir(), self.kwargs.get("params_file", "parameters") + ".yaml"))["nat_const"]["eps_0"]
        curve = ft.DeviceCurve(self, table, codes, eps_0 * self.ep.thermal_voltage / self.ep.L_n, predictor=predictor)
        inv_dt = float(self.sys.problem.model.inv_dt)
        try:
            curve.prepare()
            theta0 = ft.theta_of(curve.kept["stern"], curve.kept["kinetics"], codes)
            res = ft.LevenbergMarquardt(curve, [ft.is_log(c) for c in codes]).run(theta0)
            res["theta"] = ft.theta_of(curve.kept["stern"], curve.kept["kinetics"], codes)   # the numbers the handle holds
            curve.finish(V0, inv_dt)
        except BaseException:
            self.sys.set_time_step(inv_dt)
            raise
        self.stern, self.kinetics = ft.records_of(curve.kept["stern"], curve.kept["kinetics"], V0)
        self.problem.stern, self.problem.kinetics = self.stern, self.kinetics
        rx = self.kinetics.reactions
        self.kinetic_par = dict(self.kinetic_par, i0_CO=rx[0].k, i0_H2=rx[1].k, alpha_CO=rx[0].alpha, alpha_H2=rx[1].alpha)
        out = ft.fit_arrays(names, codes, table, theta0, res, [p[0] for p in curve.kept["points"]], self.ep.L_n)
        out["metadata"], out["result"] = ft.fit_metadata(names, out, res), res
        return out

    def fit_outputs(self, newpath):
        """``fit.npz`` and the metadata keys that go with it (see ``__init__``)."""
        out = self.fit(**self.fit_par)
        meta = out.pop("metadata")
        out.pop("result")
        np.savez(newpath + "/fit.npz", **out)
        return meta

    def fit_programme(self, data, params=None, programme=None):
        """Fits the electrode parameters ``params`` to the transient data ``data`` (a path, or a dict of the columns time_s, i_CO and /
        or i_H2, optional surface_charge and weight_*) of the potential programme ``programme`` (default: the run's own keyword) in
        fixed mode, by ``fit.LevenbergMarquardt`` over ``fit.TransientCurve``: every trial goes back to the start state, moves the
        parameters with ``gmpnp_parameter_advance`` as predictor, re-converges the steady state at the start potential, takes the
        tangent and marches with the sensitivities of section 5p.  The run must stand at its steady state.  Afterwards the run and
        the handle stand at the start potential with the FITTED parameters at the steady state there, the run's inv_dt put back.
        Returns the arrays of ``fit_programme.npz`` plus ``metadata`` and ``result``."""
        from . import fit as ft
        from . import programme as prg
        if self.stern is None or self.kinetics is None:
            raise ValueError("fit_programme: the fit needs an electrode potential and the surface kinetics (electrode_voltage, kinetics='tafel')")
        if self.galvanostat is not None:
            raise ValueError("fit_programme: not available with target_current (the galvanostat owns the potential)")
        if self.supg:
            raise ValueError("fit_programme: not available with stabilization Y")
        par = programme if programme is not None else self.programme_par
        if not par or par.get("steps_per_segment") is None:
            raise ValueError("fit_programme: the fit needs a programme in fixed mode (steps_per_segment)")
        par = prg.check_programme(par, dict(electrode_voltage=self.stern.p_electrode, kinetics=self.kinetics))
        names = tuple(params or ft.DEFAULT_PARAMS)
        codes = ft.param_codes(names)
        table = ft.check_programme_data(ft.load_programme_data(data) if not isinstance(data, dict) else data, len(codes))
        ep = self.ep
        segs = prg.build(par, float(self.stern.p_electrode), ep.time_constant, ep.thermal_voltage)
        n_seg = int(par["steps_per_segment"])
        ft.match_times(table["time_s"], np.array(prg.fixed_step_times(segs, n_seg)) * ep.time_constant)   # refused before a trial runs
        eps_0 = _load_yaml(os.path.join(utilities_dir(), self.kwargs.get("params_file", "parameters") + ".yaml"))["nat_const"]["eps_0"]
        L_D = ep.L_D
        system = ft.DeviceTransient(self, segs, n_seg, codes, eps_0 * ep.thermal_voltage / ep.L_n, lambda h: 1.0 / (h * L_D), ep.time_constant,
                                    par.get("capacity") or 4096)
        curve = ft.TransientCurve(system, table, len(codes))
        inv_dt = float(self.sys.problem.model.inv_dt)
        theta0 = ft.theta_of(system.kept["stern"], system.kept["kinetics"], codes)
        try:
            res = ft.LevenbergMarquardt(curve, [ft.is_log(c) for c in codes]).run(theta0)
            res["theta"] = ft.theta_of(system.kept["stern"], system.kept["kinetics"], codes)   # the numbers the handle holds
        finally:
            system.finish(inv_dt)
        rx = self.kinetics.reactions
        self.kinetic_par = dict(self.kinetic_par, i0_CO=rx[0].k, i0_H2=rx[1].k, alpha_CO=rx[0].alpha, alpha_H2=rx[1].alpha)
        out = ft.fit_arrays(names, codes, table, theta0, res, curve.kept["values"], ep.L_n, abscissa="time_s")
        meta = ft.fit_metadata(names, out, res)
        out["metadata"], out["result"] = {k.replace("fit_", "fit_programme_", 1): v for k, v in meta.items()}, res
        return out

    def fit_programme_outputs(self, newpath):
        """``fit_programme.npz`` and the metadata keys that go with it (see ``__init__``)."""
        out = self.fit_programme(**self.fit_programme_par)
        meta = out.pop("metadata")
        out.pop("result")
        np.savez(newpath + "/fit_programme.npz", **out)
        return meta

    def programme(self, verbose=False, **par):
        """Marches the electrode potential through the programme ``par`` (the ``programme`` keyword of ``__init__``) from the run's
        CURRENT state, on a clock of its own from 0 (gmpnp_amd/programme.py: ``run_programme`` over ``DeviceProgrammeOps``).  The
        run's own inv_dt is put back afterwards; the run, its records and the handle end at the programme's last potential.  Where the
        loop raises (a Newton failure in fixed mode, a library error) the handle goes back to the last accepted state, the trace is
        closed and the run stands at the potential of the failed attempt; the exception goes on to the caller.  Returns
        the arrays of ``programme.npz`` plus ``log`` (the attempts, by column), ``states`` (segment, time_s, (nv, nf) values at the
        breakpoints) and ``metadata`` (the ``programme_*`` keys)."""
        from . import periodic as prd
        from . import programme as prg
        from .timestep import TimeStepPolicy
        if self.stern is None:
            raise ValueError("programme: a potential programme needs an electrode potential (electrode_voltage)")
        if self.galvanostat is not None:
            raise ValueError("programme: not available with target_current (the galvanostat owns the potential)")
        if self.supg:
            raise ValueError("programme: not available with stabilization Y")
        par = prg.check_programme(par, dict(electrode_voltage=self.stern.p_electrode, kinetics=self.kinetics))
        ep = self.ep
        segs = prg.build(par, float(self.stern.p_electrode), ep.time_constant, ep.thermal_voltage)
        L_D = ep.L_D
        inv_dt = float(self.sys.problem.model.inv_dt)
        names = tuple(par.get("sensitivities") or ())
        codes, start = (prg.sensitivity_codes(names), par.get("sensitivity_start") or "steady") if names else (None, "zero")
        try:
            if names and start == "steady":   # S starts as the steady state's dependence on theta: the tangent at inv_dt = 0, still valid at the open
                self.sys.set_time_step(0.0)
                tan = self.sys.dev.electrode_tangent(codes)
                if tan["status"].any():
                    raise RuntimeError("programme: the steady tangent the sensitivities start from is not finite")
            # ``periodic``: the limit cycle of ONE period in the place of a march (gmpnp_amd/periodic.py, section 5r)
            periodic = par.get("periodic")
            periodic = None if periodic is None or periodic is False else prd.check_periodic(periodic, par)
            ops = prg.DeviceProgrammeOps(self, self.solver_parameters, lambda h: 1.0 / (h * L_D), self.dt_tol, par.get("capacity") or 4096,
                                         sensitivities=codes, sensitivity_start=start, cycle_tol=periodic[1:] if periodic else (1e-2, 1e-4))
        except BaseException:
            self.sys.set_time_step(inv_dt)
            raise
        policy = TimeStepPolicy(h_min=float(self.dt_bounds[0]), h_max=math.inf if self.dt_bounds[1] is None else float(self.dt_bounds[1]))
        srec, search = None, None
        try:
            if periodic:
                search = prd.run_periodic(ops, segs, periodic[0], par["steps_per_segment"])
                res = search["record"]   # the converged period, marched once more with records (not converged: the last marched period)
            else:
                res = prg.run_programme(ops, segs, policy, dt_init=par.get("dt_init") or ep.dts[0], dt_restart=par.get("dt_restart"),
                                        steps_per_segment=par.get("steps_per_segment"), max_attempts=self.max_steps)
            if names:
                srec = ops.sensitivity_records()
                self.sys.dev.sensitivity_close()
            rec = ops.records()
            last = self.sys.vertex_values()
        except BaseException:   # (a Newton failure in fixed mode, a library error): back to the last accepted state, no trace left open
            ops.abort()
            raise
        finally:
            self.sys.set_time_step(inv_dt)
        self.programme_state, self.programme_residuals = last, np.array(ops.residuals)
        eps_0 = _load_yaml(os.path.join(utilities_dir(), self.kwargs.get("params_file", "parameters") + ".yaml"))["nat_const"]["eps_0"]
        out = prg.output_arrays(ep, eps_0, rec, ops.segments, segs, par.get("cycles", 1))
        if verbose:
            print("programme %s: %d accepted steps, %d attempts, %s" % (par["kind"], len(rec), len(res["log"]), res["stop_reason"]))
        states = list(ops.states)
        t_last = res["times"][-1] if res["times"] else 0.0
        if not states or states[-1][1] != t_last:   # the run ended between two breakpoints (max_steps, h_min): its last state is kept too
            states.append((ops.segments[-1] if ops.segments else 0, t_last, last))
        meta = {"programme_kind": par["kind"], "programme_cycles": int(par.get("cycles", 1)), "programme_segments": len(segs),
                "programme_steps_accepted": int(len(rec)), "programme_steps_rejected": int(len(res["log"]) - len(rec)),
                "programme_stop_reason": res["stop_reason"], "programme_t_reached": float(res["times"][-1] * ep.time_constant) if res["times"] else 0.0,
                "programme_newton_iterations": int(ops.newton_iterations),
                "programme_charge_closure": float(rec["Q_D"][-1] - (rec["D"][-1] - ops.D_first)) if len(rec) else 0.0,
                "programme_status": int(np.bitwise_or.reduce(rec["status"])) if len(rec) else 0,
                # the interface where the programme ended, as one consistent set (potential_OHP, field_OHP, eps_rel_OHP and the run's
                # arrays describe the end of the schedule)
                "programme_electrode_voltage": float(self.stern.p_electrode),
                "programme_potential_OHP": float(out["potential_OHP"][-1]) if len(rec) else None,
                "programme_surface_charge": float(out["surface_charge"][-1]) if len(rec) else None}
        out.update(log=prg.log_arrays(res["log"]), states=[(k, t * ep.time_constant, v) for k, t, v in states], metadata=meta)
        if search is not None:   # only with the option on: the history of the search and the state the recorded period starts from
            out["periodic"] = dict(prd.history_arrays(search["history"]), state=search["state"])
            meta.update(prd.metadata(search))
        if names:
            out["sensitivity"] = prg.sensitivity_arrays(ep, eps_0, srec, names, codes)
            meta.update(programme_sensitivity_parameters=list(names), programme_sensitivity_start=start,
                        programme_sensitivity_status=int(np.bitwise_or.reduce(srec["status"].ravel())) if srec.size else 0,
                        programme_sensitivity_residual=float(srec["residual"].max()) if srec.size else 0.0)
        return out

    def programme_outputs(self, newpath):
        """``programme.npz``, ``programme_states.npz`` and the attempts for ``timestep_log.npz``; returns (metadata keys, log arrays)."""
        out = self.programme(**self.programme_par)
        meta, log, states = out.pop("metadata"), out.pop("log"), out.pop("states")
        sens = out.pop("sensitivity", None)
        if sens is not None:   # only with the option on
            np.savez(newpath + "/programme_sensitivity.npz", **sens)
        search = out.pop("periodic", None)
        if search is not None:   # only with the option on: programme.npz is then the recorded period of the limit cycle
            np.savez(newpath + "/programme_periodic.npz", **search)
        np.savez(newpath + "/programme.npz", **out)
        np.savez(newpath + "/programme_states.npz", segment=np.array([k for k, _, _ in states], dtype=np.int64),
                 time_s=np.array([t for _, t, _ in states]), states=np.stack([v for _, _, v in states]), coor=self.mesh.coords)
        return meta, {"programme_" + k: v for k, v in log.items()}

    def kinetics_summary(self):
        """Per-step ``i_CO``, ``i_H2`` [A/m2] and ``FE_H2`` of a run with the surface kinetics (the OHP is one point: w = 1)."""
        from .kinetics import current_summary
        rows = [current_summary(c, 1.0) for c in self.currents]
        out = {k: np.array([r[k] for r in rows]) for k in ("i_CO", "i_H2", "FE_H2")}
        if self.galvanostat is not None:
            out["electrode_voltage"] = np.array(self.potentials)
        return out

    def write_outputs(self, stamp=None):
        ep, mesh, k = self.ep, self.mesh, self.kwargs
        stamp = stamp or datetime.now().strftime("%y-%m-%d-%H-%M-%S")
        end_time = datetime.now().strftime("%y-%m-%d-%H-%M-%S")
        identifier = run_identifier(ep, k, self.stern, self.target_current)
        newpath = os.path.join(output_root(), ep.model_name, stamp + "_experiment", identifier)
        os.makedirs(newpath, exist_ok=True)
        # the fit to transients starts every trial at the steady state of the run's potential: before the programme, which is then
        # marched with the fitted parameters
        fit_programme = self.fit_programme_outputs(newpath) if self.fit_programme_par is not None else None
        programme = self.programme_outputs(newpath) if self.programme_par is not None else None   # first: the metadata reports the state it ends at
        hist = np.stack(self.history)
        names = ["H", "OH", "HCO3", "CO32", "CO2", "cat", "p"]
        Hh = {nme: hist[:, :, i] for i, nme in enumerate(names)}
        field_values = self.sys.project_gradient(hist[-1][:, 6], sign=-1.0)[:, 0]
        field_values_rescaled = field_values * ep.thermal_voltage / ep.L_n
        field_OHP = field_values_rescaled[0] * 1.0e-9
        if self.stepper is not None:
            tau_array = np.array(self.times)   # the actual times of the history rows
        elif ep.dry_run:
            tau_array = np.linspace(0, ep.stage_T[0], self.tot_num_steps)
        else:
            tau_array = np.concatenate((np.linspace(0, ep.stage_T[0], ep.stage_steps[0]),
                                        np.linspace(ep.stage_T[0] + ep.dts[1], ep.stage_T[1], ep.stage_steps[1])))
        np.savez(newpath + "/arrays_unscaled.npz", H=Hh["H"], OH=Hh["OH"], HCO3=Hh["HCO3"], CO32=Hh["CO32"],
                 CO2=Hh["CO2"], cat=Hh["cat"], p=Hh["p"], coor=mesh.coords, tau=tau_array, field_values=field_values,
                 **(self.kinetics_summary() if self.kinetics is not None else {}))
        sc = {nme: scale(species=sp, tau=tau_array, C=Hh[nme], initial_conc=ep.initial_conc, diff_coeff=ep.diff_coeff,
                         L_n=ep.L_n, L_debye=ep.L_debye) for nme, sp in zip(names[:6], ep.species)}
        c = {nme: sc[nme][1] for nme in sc}
        psi = Hh["p"] * ep.thermal_voltage
        pH_OHP = -math.log10(c["H"][-1][0] / 1000)
        w = (ep.n_water[ep.cation] * c["cat"] + ep.n_water["H"] * c["H"]) * 1.0e-3
        eps_rel_conc_ss = ep.eps_rel * ((55 - w) / 55) + 6 * (w / 55)
        eps_rel_OHP = eps_rel_conc_ss[-1][0]
        charge_density = c["cat"][-1] - c["HCO3"][-1] - 2 * c["CO32"][-1] - c["OH"][-1] + c["H"][-1]
        np.savez(newpath + "/arrays_scaled.npz", x=mesh.coords * ep.L_n, psi=psi, t_H=sc["H"][0], c_H=c["H"],
                 t_OH=sc["OH"][0], c_OH=c["OH"], t_HCO3=sc["HCO3"][0], c_HCO3=c["HCO3"], t_CO32=sc["CO32"][0],
                 c_CO32=c["CO32"], t_CO2=sc["CO2"][0], c_CO2=c["CO2"], t_cat=sc["cat"][0], c_cat=c["cat"],
                 eps_rel=eps_rel_conc_ss, field_values=field_values_rescaled, charge_density=charge_density)
        potential_OHP = float(psi[-1][0])
        CO2_OHP_frac = c["CO2"][-1][0] / ep.initial_conc["CO2"]
        pH_overpotential = -0.059 * (ep.bulk_pH - pH_OHP) * 1.0e+3
        CO2_overpotential = (0.059 / 2) * math.log10(1 / CO2_OHP_frac) * 1.0e+3
        current_H = self.current_H_frac * ep.current_OHP_ss
        if not ep.dry_run:
            # reference 1D:971-972: time_step / total_sim_time are undefined outside the dry-run branch (Q3)
            raise NameError("name 'time_step' is not defined")
        metadata_dict = {
            "concentration_elec": k.get("concentration_elec", 0.1), "cation": ep.cation, "model": ep.model_name,
            "stabilization": k.get("stabilization", "N"), "voltage_multiplier": ep.voltage_scaled,
            "H2_FE": k.get("H2_FE", 0.2), "L_n_EDL": ep.L_n, "time_constant": ep.time_constant,
            "time_step": ep.time_step, "total_sim_time": ep.total_sim_time, "mesh_number": ep.mesh_number,
            "mesh_structure": ep.mesh_structure, "eps_rel_OHP": float(eps_rel_OHP), "field_OHP": float(field_OHP),
            "current_OHP_ss": ep.current_OHP_ss, "current_H": current_H, "H_OHP_vs_bulk": ep.H_OHP,
            "potential_OHP": potential_OHP, "pH_OHP": pH_OHP, "CO2_OHP_frac": float(CO2_OHP_frac),
            "pH_overpotential": pH_overpotential, "CO2_overpotential": CO2_overpotential, "end_time": end_time,
            "newton_iterations": int(sum(self.newton_its)), "krylov_iterations": int(self.sys.krylov_iterations),
            "num_steps_run": int(self.n)}
        if self.step_fraction:
            metadata_dict["step_fraction"] = self.step_fraction
        if self.stern is not None:
            metadata_dict.update(self.stern_summary())
        if self.kinetics is not None:
            from .kinetics import tafel_parameters
            metadata_dict.update(tafel_parameters(self.kinetic_par))
            metadata_dict.update({key: (float(v[-1]) if len(v) else None) for key, v in self.kinetics_summary().items()})
        if self.galvanostat is not None:
            metadata_dict["target_current"] = self.target_current
        if self.impedance_par is not None:
            metadata_dict.update(self.impedance_outputs(newpath))
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
        if fit_programme is not None:
            metadata_dict.update(fit_programme)
        if self.fit_par is not None:   # before the curve, which is then the fitted one; the handle ends at the run's operating point
            metadata_dict.update(self.fit_outputs(newpath))
        if self.polarisation_par is not None:   # last: the handle leaves the run's operating point
            metadata_dict.update(self.polarisation_outputs(newpath))
        with open(newpath + "/metadata.json", "w") as fh:
            fh.write(json.dumps(metadata_dict, indent=0))
        return newpath


def run_identifier(ep, kwargs, stern=None, target_current=None):
    """Name of a run's output directory below ``<model>/<stamp>_experiment`` (reference 1D:862-866; a run with the Stern boundary
    condition is named by its electrode voltage and Stern model in the OHP voltage's place, a galvanostatic run by its target)."""
    if target_current is not None:
        head = "target_current_" + str(target_current) + "_" + stern.model
    elif stern is not None:
        head = "electrode_" + str(stern.p_electrode) + "_" + stern.model
    else:
        head = "voltage_" + str(ep.voltage_scaled)
    return (head + "_H2_FE_" + str(kwargs.get("H2_FE", 0.2)) + "_current_"
            + str(ep.current_OHP_ss) + "_H_OHP_" + str(ep.H_OHP) + "_cation_" + ep.cation)


def solve_EDL(concentration_elec=0.1, model="MPNP", voltage_multiplier=None, H2_FE=0.2, mesh_structure="variable",
              current_OHP_ss=10.0, L_n=50.0e-6, stabilization="N", H_OHP=None, cation="K", params_file="parameters",
              dry_run=True, num_steps=None, verbose=True, budget=False, step_fraction=0.0, electrode_voltage=None, stern_model="BDM",
              stern_length=4.0e-10, stern_eps_surface=6.0, kinetics=None, i0_CO=None, i0_H2=None, alpha_CO=0.5, alpha_H2=0.5, p_eq_CO=0.0,
              p_eq_H2=0.0, target_current=None, impedance=None, polarisation=None, fit=None, programme=None, **adaptive):
    """Same keyword surface as the reference's ``solve_EDL`` (1D:66-79); returns the output directory.  ``adaptive``: the
    adaptive-stepping keywords of ``EDLRun`` (adaptive_dt, dt_rtol, dt_atol, dt_init, dt_min, dt_max, t_end, steady_tol, max_steps).
    ``voltage_multiplier`` = None is the reference's default -1.0, unless ``electrode_voltage`` (with ``stern_model``, ``stern_length``,
    ``stern_eps_surface``: the Stern boundary condition of ``EDLRun``) takes its place."""
    stern = {}
    if electrode_voltage is not None:
        stern = dict(electrode_voltage=electrode_voltage, stern_model=stern_model, stern_length=stern_length, stern_eps_surface=stern_eps_surface)
    elif voltage_multiplier is None:
        voltage_multiplier = -1.0
    if kinetics is not None:   # (the surface kinetics of ``EDLRun``)
        stern.update(kinetics=kinetics, i0_CO=i0_CO, i0_H2=i0_H2, alpha_CO=alpha_CO, alpha_H2=alpha_H2, p_eq_CO=p_eq_CO, p_eq_H2=p_eq_H2)
    if target_current is not None:   # (the galvanostatic mode of ``EDLRun``)
        stern.update(target_current=target_current)
    if impedance:   # (the impedance spectrum of ``EDLRun``, after the last step)
        stern.update(impedance=impedance)
    if polarisation:   # (the polarisation curve of ``EDLRun``, after the last step)
        stern.update(polarisation=polarisation)
    if fit:   # (the fit of the electrode kinetics of ``EDLRun``, after the last step and before the curve)
        stern.update(fit=fit)
    if programme:   # (the potential programme of ``EDLRun``, after the last step)
        stern.update(programme=programme)
    run = EDLRun(num_steps=num_steps, budget=budget, step_fraction=step_fraction, **adaptive, **stern, concentration_elec=concentration_elec, model=model,
                 voltage_multiplier=voltage_multiplier, H2_FE=H2_FE, mesh_structure=mesh_structure,
                 current_OHP_ss=current_OHP_ss, L_n=L_n, stabilization=stabilization, H_OHP=H_OHP, cation=cation,
                 params_file=params_file, dry_run=dry_run)
    try:
        run.run(verbose)
        return run.write_outputs()
    finally:
        run.sys.close()


def build_parser():
    """Flags, defaults and types of reference 1D:993-1101 (``--dry_run`` keeps ``type=bool``, Q3)."""
    p = argparse.ArgumentParser(description="experiment parameters")
    p.add_argument("--concentration_elec", required=False, default=0.1, type=float)
    p.add_argument("--model", required=False, default="MPNP", type=str)
    p.add_argument("--voltage_multiplier", required=False, default=None, type=float, help="default -1.0 (without --electrode_voltage)")
    p.add_argument("--mesh_structure", required=False, default="variable", type=str)
    p.add_argument("--H2_FE", required=False, default=0.2, type=float)
    p.add_argument("--current_OHP_ss", required=False, default=10.0, type=float)
    p.add_argument("--L_n", required=False, default=50e-6, type=float)
    p.add_argument("--stabilization", required=False, default="N", type=str)
    p.add_argument("--H_OHP", required=False, default=None, type=float)
    p.add_argument("--cation", required=False, default="K", type=str)
    p.add_argument("--params_file", required=False, default="parameters", type=str)
    p.add_argument("--dry_run", required=False, default=True, type=bool)
    p.add_argument("--num_steps", required=False, default=None, type=int, help="(addition) run only the first N steps")
    p.add_argument("--budget", action="store_true", help="(addition) record the species budgets and consistent boundary fluxes of every step (budget.npz)")
    p.add_argument("--step_fraction", required=False, default=0.0, type=float, help="(addition) fraction-to-boundary step limiter of the Newton update: tau in (0, 1), 0 = off")
    add_adaptive_arguments(p)
    add_stern_arguments(p)
    add_kinetics_arguments(p)
    add_galvanostat_arguments(p)
    add_impedance_arguments(p)
    add_polarisation_arguments(p)
    add_fit_arguments(p)
    add_programme_arguments(p)
    return p


def main(argv=None):
    a = build_parser().parse_args(argv)
    return solve_EDL(concentration_elec=a.concentration_elec, model=a.model, voltage_multiplier=a.voltage_multiplier,
                     H2_FE=a.H2_FE, mesh_structure=a.mesh_structure, current_OHP_ss=a.current_OHP_ss, L_n=a.L_n,
                     stabilization=a.stabilization, H_OHP=a.H_OHP, cation=a.cation, params_file=a.params_file,
                     dry_run=a.dry_run, num_steps=a.num_steps, budget=a.budget, step_fraction=a.step_fraction, **adaptive_keywords(a), **stern_keywords(a), **kinetics_keywords(a), **galvanostat_keywords(a),
                     **impedance_keywords(a), **polarisation_keywords(a), **fit_keywords(a), **programme_keywords(a), **programme_fit_keywords(a))


if __name__ == "__main__":
    main()
