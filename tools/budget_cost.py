"""Cost of one species-budget call on L_50_R_5 against one residual evaluation: back-to-back launches between
HIP events (gmpnp_time_kernel: 19 = element kernel without J, 3 = residual gather, 20 = the budget's launch chain) and the host time
of a whole call (launch chain + the read-back of the table)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import __graft_entry__ as ge
ge.build()
from gmpnp_amd import backend
from gmpnp_amd.mesh import read_dolfin_xml, resolve_mesh_path
from gmpnp_amd.params import pore_parameters, utilities_dir
from gmpnp_amd.problem import pore_problem

pp = pore_parameters(concentration_elec=0.5, L=50e-9, R=5e-9)
mesh = read_dolfin_xml(resolve_mesh_path(utilities_dir(), pp.mesh_name))
prob, _ = pore_problem(pp, mesh)
nv = mesh.num_vertices
rng = np.random.default_rng(0)
u = np.concatenate([rng.uniform(.5, 1.5, (nv, 8)), rng.uniform(-1, 0, (nv, 1))], axis=1).ravel()
out = {"n_vertices": nv, "n_cells": int(len(mesh.cells))}
with backend.DeviceSolver(prob) as dev:
    dev.set_state(u, 0.9 * u)
    dev.species_budget()
    for rep in range(3):
        out["element_without_J_us_%d" % rep] = dev.time_kernel(19, 200)
        out["res_gather_us_%d" % rep] = dev.time_kernel(3, 200)
        out["budget_chain_us_%d" % rep] = dev.time_kernel(20, 200)
        t0 = time.perf_counter()
        for _ in range(200):
            dev.species_budget()
        out["budget_call_host_us_%d" % rep] = (time.perf_counter() - t0) / 200 * 1e6
print(json.dumps(out))
