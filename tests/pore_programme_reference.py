"""The wall profile (include/gmpnp.h "wall profile") restated in NumPy over the existing restatements
(kinetics_reference.boundary_weights, stern_bc_reference.stern_terms, kinetics_reference.node_rates), and a NumPy system for
``run_programme`` that records it beside the electrode record (imported like programme_reference.py; not a conftest).  Test
infrastructure only."""
import numpy as np

import kinetics_reference as K
import programme_reference as PR
import stern_bc_reference as SR
from gmpnp_amd import programme as P

R4 = P.MAX_SURFACE_REACTIONS


def wall_nodes_z(prob):
    """(nodes ascending, w_I, z_I) of the Stern boundary of a 3D problem."""
    nodes, w = K.boundary_weights(prob)
    return nodes, w, np.asarray(prob.coords, dtype=np.float64)[nodes, 2]


def node_terms(prob, u):
    """Per node of the Stern boundary (ascending): the Stern term of its potential row (0 on a Dirichlet row), w_I rate_r (4 columns, 0
    without kinetics), w_I u_{I,f} (nf columns) and w_I: what the bins of the profile add up."""
    nf = prob.nf
    nodes, w, _ = wall_nodes_z(prob)
    u2d = np.asarray(u, dtype=np.float64).reshape(-1, nf)
    Fs, _ = SR.stern_terms(prob, np.asarray(u, dtype=np.float64), want_jacobian=False)
    Fs[np.asarray(prob.bc_dofs, dtype=np.int64)] = 0.0
    d = Fs[nodes * nf + nf - 1]
    rates = np.zeros((len(nodes), R4))
    if getattr(prob, "kinetics", None) is not None:
        for k, (I, wI) in enumerate(zip(nodes, w)):
            r = [x[0] for x in K.node_rates(prob, u2d, I)]
            rates[k, :len(r)] = wI * np.array(r)
    return d, rates, w[:, None] * u2d[nodes], w


def profile(prob, u, edges):
    """The records of one append, per bin of ``edges``: dict of area, D, I (bins, 4), p_mean, u_mean (bins, ns), count, and ``scale``:
    the sums of |terms| of D, I and area (what a bound of 64 eps is taken of)."""
    nf, ns = prob.nf, prob.nf - 1
    _, _, z = wall_nodes_z(prob)
    d, rates, wu, w = node_terms(prob, u)
    lists = P.wall_bin_lists(z, list(edges))
    nb = len(lists)
    out = {"area": np.zeros(nb), "D": np.zeros(nb), "I": np.zeros((nb, R4)), "p_mean": np.zeros(nb), "u_mean": np.zeros((nb, ns)),
           "count": np.zeros(nb, dtype=np.int64), "scale_D": np.zeros(nb), "scale_I": np.zeros((nb, R4)), "scale_u": np.zeros((nb, nf))}
    for b, members in enumerate(lists):
        m = np.asarray(members, dtype=np.int64)
        out["count"][b] = len(m)
        out["area"][b], out["D"][b], out["I"][b] = w[m].sum(), d[m].sum(), rates[m].sum(axis=0)
        out["scale_D"][b], out["scale_I"][b], out["scale_u"][b] = np.abs(d[m]).sum(), np.abs(rates[m]).sum(axis=0), np.abs(wu[m]).sum(axis=0)
        with np.errstate(divide="ignore", invalid="ignore"):
            mean = wu[m].sum(axis=0) / w[m].sum()
        out["p_mean"][b], out["u_mean"][b] = mean[ns], mean[:ns]
    return out


class NumpyPoreProgrammeSystem(PR.NumpyProgrammeSystem):
    """``NumpyProgrammeSystem`` that also records the wall profile of every accepted step, with the charges of the bins accumulated by
    the Python charge statement (``profiles``: one dict per step, with ``Q`` (bins, 4) and h)."""

    def __init__(self, prob, u, inv_dt_of_h, edges, **kw):
        super().__init__(prob, u, inv_dt_of_h, **kw)
        self.edges = [float(e) for e in edges]
        self.Q = [[0.0] * R4 for _ in range(len(self.edges) - 1)]
        self.profiles = []

    def record(self, t, h, seg, p):
        super().record(t, h, seg, p)
        pr = profile(self.prob, self.u, self.edges)
        self.Q = [P.wall_profile_charge(self.Q[b], h, pr["I"][b]) for b in range(len(self.Q))]
        pr.update(t=t, h=h, Q=np.array(self.Q))
        self.profiles.append(pr)


# ---- the marched cases of the CPU and the GPU test: chosen on this reference alone so that every Newton solve converges ----------------
MARCH_CYLINDERS = {"c1x2": (1, 2), "c2x3": (2, 3)}
MARCH_P_M = -1.0
MARCH_STEPS_PER_SEGMENT = 2
MARCH_BINS = 2


def march_case(coarse):
    """(problem, start state (read-only), reference step dt): the generated cylinder at p_M = -1 and the state one backward-Euler step
    of the model's own inv_dt away from the bulk state."""
    import pore_response_reference as PP
    prob = PP.cylinder_case(coarse, p_M=MARCH_P_M)
    nv = prob.coords.shape[0]
    u0 = np.tile(np.r_[np.ones(prob.nf - 1), 0.0], nv)
    u, st = K.newton_loop(prob, u0, u0, maximum_iterations=25, relative_tolerance=1e-13, absolute_tolerance=1e-9)
    assert st.converged
    u.setflags(write=False)
    return prob, u, 1.0 / float(prob.model.inv_dt)


def march_programmes(dt):
    """A pulse with two jumps (three levels, one cycle) and two cycles of a triangle (corners only), in scaled time: segments of one or
    two reference steps, marched in fixed mode with two steps per segment: six and eight steps, more than the capacity of 5 the device
    test drains at.  (Three steps per segment leave the admissible set on the reference: eps <= 0 under BDM.)"""
    return {"pulse": P.pulse([-1.25, -0.75, -1.0], [2.0 * dt, dt, 2.0 * dt], 1),
            "triangle": P.triangle(MARCH_P_M, -1.5, 0.5 / (2.0 * dt), 2)}
