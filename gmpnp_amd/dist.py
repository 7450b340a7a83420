"""Mesh partitioning for the multi-GPU solve (BASELINE configs[3]): one process per GPU.

The reference is a serial script (no MPI call site), so there is no behaviour to match except the serial result itself: the
partitioned solve must give the serial Newton iterates.

Decomposition.  Vertices are ordered by `backend.slab_permutation` (slabs along the pore axis) and cut into P contiguous
ranges: rank p OWNS its range.  Its local mesh is every cell that touches an owned vertex; the other vertices of those cells
are GHOSTS (owned by a neighbouring slab).  Cut cells are assembled redundantly on both sides, so the rows of owned vertices
are complete without any matrix communication; ghost rows are replaced by identity rows (they are never used).

What this module is:
* ``slab_cut`` / ``build_local_domain`` / ``partition_hierarchy`` — the partition, the halo plan and the global coarse slabs handed
  to ``gmpnp_create_partition``, for every level of a nested hierarchy (the multilevel term across the partitions);
  ``partition_plan`` is the one-level case;
* ``PartitionedSolver`` — the product path: Newton, BiCGStab, ghost exchanges and all-reduces run INSIDE libgmpnp.so
  (``gmpnp_group_newton_solve``; RCCL, in-process, or host-staged transport); Python scatters / gathers states and the
  per-step boundary values;
* ``host_transport_callbacks`` — the two collectives of the library's host-staged transport on ``torch.distributed``.
(Round 1's host-driven Python BiCGStab / Newton is gone from the product; tests/partition_double.py keeps a NumPy double of the
partitioned iteration that drives ``partition_plan`` and these callbacks at world size 2 on ``gloo`` without a GPU.)
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .problem import Problem


# ---------------------------------------------------------------------------------------------
# partition
# ---------------------------------------------------------------------------------------------
def default_global_aggregates(nparts: int) -> int:
    """Coarse slabs over the whole mesh: 8 (the single-GPU default) when the ranks divide it, else one slab per rank
    rounded up to a multiple of the rank count; at most 15 (the 9-field coarse operator must fit the LDS-resident inverse)."""
    if 8 % nparts == 0:
        return 8
    n = nparts * max(1, 8 // nparts)
    if n > 15:
        raise ValueError("no coarse-slab count <= 15 is a multiple of %d ranks" % nparts)
    return n


def slab_cut(prob: Problem, nparts: int, n_global_aggregates: int = None):
    """The slab cut of a mesh: (position of every vertex in the slab order, its coarse slab, its owner).

    Global slab order (``backend.slab_permutation``: vertices sorted along the pore axis) is cut into `nparts` contiguous
    ownership ranges and into `n_global_aggregates` coarse slabs with the SAME integer boundaries, so a slab never
    straddles two ranks (and the ranges are those of `nparts` equal-count slabs: (nv k m) // (nparts m) == (nv k) // nparts)."""
    from .backend import slab_permutation
    nag = n_global_aggregates or default_global_aggregates(nparts)
    if nag % nparts:
        raise ValueError("n_global_aggregates must be a multiple of the number of ranks")
    nv = prob.coords.shape[0]
    gperm = slab_permutation(prob.coords, prob.cells, window=0)  # pure slab order: sharp partition interfaces
    pos = np.empty(nv, dtype=np.int64)
    pos[gperm] = np.arange(nv)
    bounds = (nv * np.arange(nag + 1, dtype=np.int64)) // nag
    aggregate = np.searchsorted(bounds[1:], pos, side="right").astype(np.int32)
    owner = (aggregate // (nag // nparts)).astype(np.int32)
    return pos, aggregate, owner


@dataclass
class LocalDomain:
    rank: int
    nparts: int
    owned: np.ndarray  # global (file) vertex ids, ascending
    ghosts: np.ndarray  # global vertex ids, ascending
    lverts: np.ndarray  # the local vertices in local order: [owned..., ghosts...]
    g2l: np.ndarray  # local index of every GLOBAL vertex, -1 = not local
    problem: Problem  # local problem on `lverts`
    n_owned: int
    send: dict  # neighbour rank -> local indices (into owned) to send, in the receiver's ghost order
    recv: dict  # neighbour rank -> local indices (n_owned + k) that receive

    @property
    def nf(self):
        return self.problem.nf


def build_local_domain(prob: Problem, owner: np.ndarray, rank: int, nparts: int, lcells: np.ndarray = None,
                       ghost_sets: list = None) -> LocalDomain:
    """Local problem of `rank` on the cells `lcells` (global vertex ids).  Deterministic and purely local (every rank can build any
    rank's domain), so the send lists need no negotiation: rank q's ghosts owned by p, in ascending global id, are what p sends to
    q.  The halo plan comes from every rank's ACTUAL ghost set (`ghost_sets[q]`, ascending), so ghosts that no owned cell touches
    (the transfer ghosts of a coarse level) are served too.  By default the local cells are those that touch an owned vertex and
    the ghosts of a rank are the other vertices of its such cells."""
    nf = prob.nf
    owned = np.nonzero(owner == rank)[0]
    if lcells is None:
        touched = [prob.cells[(owner[prob.cells] == q).any(axis=1)] for q in range(nparts)]
        lcells = touched[rank]
        ghost_sets = []
        for q in range(nparts):
            vq = np.unique(touched[q])
            ghost_sets.append(vq[owner[vq] != q])
        # these ids have always had the cells' integer type, the ones of explicit cell lists NumPy's index type: the plans are
        # pinned with their types (tests/golden/partition_plans.json)
        owned = owned.astype(prob.cells.dtype)
    ghosts = ghost_sets[rank]
    assert np.array_equal(np.union1d(owned, ghosts), np.unique(lcells)), "the local cells must cover exactly the owned and the ghost vertices"
    lverts = np.concatenate([owned, ghosts])
    g2l = -np.ones(prob.coords.shape[0], dtype=np.int64)
    g2l[lverts] = np.arange(len(lverts))

    def facets_local(fv):
        if len(fv) == 0:
            return np.zeros((0, 3), dtype=np.int32)
        keep = (owner[fv] == rank).any(axis=1)
        return g2l[fv[keep]].astype(np.int32)

    # Dirichlet: the global conditions restricted to local vertices + identity rows on every ghost dof
    gv = prob.bc_dofs // nf
    inloc = g2l[gv] >= 0
    table = dict(zip((g2l[gv[inloc]] * nf + prob.bc_dofs[inloc] % nf).tolist(), prob.bc_vals[inloc].tolist()))
    for d in range(len(owned) * nf, len(lverts) * nf):
        table[d] = 0.0  # value irrelevant: ghost rows are never used
    bd = np.array(sorted(table), dtype=np.int64)
    bvl = np.array([table[d] for d in bd])
    pv = prob.point_vertices
    pv_local = g2l[pv[owner[pv] == rank]].astype(np.int32) if len(pv) else np.zeros(0, dtype=np.int32)
    local = Problem(coords=prob.coords[lverts], cells=g2l[lcells].astype(np.int32), model=prob.model, quad=prob.quad,
                    wall_facets=facets_local(prob.wall_facets), exit_facets=facets_local(prob.exit_facets),
                    point_vertices=pv_local, bc_dofs=bd, bc_vals=bvl)
    # halo plan
    gowner = owner[ghosts]
    recv = {int(q): len(owned) + np.nonzero(gowner == q)[0] for q in np.unique(gowner)}
    send = {}
    for q in range(nparts):
        if q != rank:
            mine = ghost_sets[q][owner[ghost_sets[q]] == rank]   # ascending global id == q's ghost order restricted to my vertices
            if len(mine):
                send[q] = g2l[mine]
    return LocalDomain(rank=rank, nparts=nparts, owned=owned, ghosts=ghosts, lverts=lverts, g2l=g2l, problem=local,
                       n_owned=len(owned), send=send, recv=recv)


# ---------------------------------------------------------------------------------------------
# the partitioned solve INSIDE the library (gmpnp_create_partition / gmpnp_group_*): this module only partitions and plans
# ---------------------------------------------------------------------------------------------
def _part_dict(dom: LocalDomain, nag: int, aggregate: np.ndarray) -> dict:
    """What gmpnp_create_partition takes: the halo lists of `dom` neighbour by neighbour and the coarse slab of every local vertex."""
    nbrs = sorted(set(dom.send) | set(dom.recv))
    send_ptr, recv_ptr, send_v, recv_v = [0], [0], [], []
    for q in nbrs:
        send_v.extend(np.asarray(dom.send.get(q, []), dtype=np.int64).tolist())
        recv_v.extend(np.asarray(dom.recv.get(q, []), dtype=np.int64).tolist())
        send_ptr.append(len(send_v))
        recv_ptr.append(len(recv_v))
    owned_flag = np.zeros(len(dom.lverts), dtype=np.uint8)
    owned_flag[:dom.n_owned] = 1
    return {"rank": dom.rank, "size": dom.nparts, "n_global_aggregates": nag, "vertex_aggregate": aggregate[dom.lverts].astype(np.int32),
            "vertex_owned": owned_flag, "neighbour_rank": np.array(nbrs, dtype=np.int32), "send_ptr": np.array(send_ptr, dtype=np.int32),
            "send_vertices": np.array(send_v, dtype=np.int32), "recv_ptr": np.array(recv_ptr, dtype=np.int32),
            "recv_vertices": np.array(recv_v, dtype=np.int32)}


# ---------------------------------------------------------------------------------------------
# the nested levels of the multilevel term (gmpnp_attach_coarse_level on partitioned handles)
# ---------------------------------------------------------------------------------------------
@dataclass
class LevelPlan:
    domain: LocalDomain
    perm: np.ndarray          # local internal order (perm[internal] = local file index)
    part: dict                # what gmpnp_create_partition takes
    parents: np.ndarray       # (n_local, 2) parents of every local vertex in the NEXT-COARSER level's local file order, -1 = not
                              # local there (ghost rows only; equal entries = a copy); None on the coarsest level
    owner: np.ndarray         # owner of every GLOBAL vertex of the level (all ranks)
    pos: np.ndarray           # position of every global vertex in the level's slab order
    aggregate: np.ndarray     # coarse slab of every global vertex


def _level_plan(prob: Problem, pos, aggregate, owner, rank, nparts, nag, lcells=None, ghost_sets=None) -> LevelPlan:
    """The plan of one level from its slab cut.  The local vertex order handed to the library is the global slab order restricted to
    the local vertices: ghosts of the lower neighbour, owned vertices, ghosts of the upper neighbour."""
    dom = build_local_domain(prob, owner, rank, nparts, lcells, ghost_sets)
    perm = np.argsort(pos[dom.lverts], kind="stable").astype(np.int32)
    return LevelPlan(domain=dom, perm=perm, part=_part_dict(dom, nag, aggregate), parents=None, owner=owner, pos=pos, aggregate=aggregate)


def partition_hierarchy(levels, nparts: int, rank: int, n_global_aggregates: int = None):
    """Partition plans of a nested hierarchy (``problem.pore_hierarchy``: [(problem, boundaries, parents)], FINEST first) for rank
    `rank`: one ``LevelPlan`` per level (a single problem is a hierarchy of one level: ``partition_plan``).

    * The finest level is cut by ``slab_cut``; its local mesh is every cell that touches an owned vertex.
    * A coarse vertex is owned where its COPY (the fine vertex at the same place) is owned, lies in its copy's slab, and takes its
      copy's place in the slab order: the coarse slabs never straddle ranks and no tie along the axis reorders anything.
    * The coarse local mesh holds the cells that touch an owned vertex (its rows are complete) plus, for every parent of an owned
      fine vertex that those cells miss, one cell that contains it: both parents of every owned fine vertex are local (transfer
      ghosts), so the prolongation of the owned rows reads local values only.  Ghost rows are identity rows as on the finest level.
    * Every child of an owned coarse vertex is local on the finer level (the copy's one-cell ring): the restriction of the owned
      coarse rows reads local values only.  Asserted here."""
    nag = n_global_aggregates or default_global_aggregates(nparts)
    plans = [_level_plan(levels[0][0], *slab_cut(levels[0][0], nparts, nag), rank, nparts, nag)]
    for k in range(1, len(levels)):
        par_f = np.asarray(levels[k - 1][2], dtype=np.int64)
        prob_c = levels[k][0]
        assert len(prob_c.point_vertices) == 0, "point fluxes (1D problems) have no rule on a coarse level"
        fine = plans[-1]
        nvc = prob_c.coords.shape[0]
        is_copy = par_f[:, 0] == par_f[:, 1]
        copy = -np.ones(nvc, dtype=np.int64)
        copy[par_f[is_copy, 0]] = np.nonzero(is_copy)[0]
        if (copy < 0).any():
            raise ValueError("level %d: a coarse vertex has no copy on the finer level (the meshes are not nested)" % k)
        owner_c = fine.owner[copy]
        cells = prob_c.cells
        # the first (lowest cell id) cell that contains each vertex
        in_cells, at = np.unique(cells.ravel(), return_index=True)
        first_cell = np.full(nvc, -1, dtype=np.int64)
        first_cell[in_cells] = at // cells.shape[1]
        lcells, ghost_sets = [], []
        for q in range(nparts):
            need = np.unique(par_f[fine.owner == q].ravel())
            lc = cells[(owner_c[cells] == q).any(axis=1)]
            have = np.zeros(nvc, dtype=bool)
            have[lc.ravel()] = True
            missing = need[~have[need]]
            if len(missing):   # one cell per missing parent
                assert (first_cell[missing] >= 0).all(), "a parent vertex belongs to no cell"
                lc = np.concatenate([lc, cells[np.unique(first_cell[missing])]])
            lcells.append(lc)
            verts = np.unique(lc)
            ghost_sets.append(verts[owner_c[verts] != q])
        coarse = _level_plan(prob_c, fine.pos[copy], fine.aggregate[copy], owner_c, rank, nparts, nag, lcells[rank], ghost_sets)
        # parents of the finer level's local vertices in this level's local file order
        fine.parents = coarse.domain.g2l[par_f[fine.domain.lverts]].astype(np.int32)
        assert (fine.parents[:fine.domain.n_owned] >= 0).all(), "both parents of every owned fine vertex must be local"
        # children of the owned coarse vertices: every fine vertex naming one as a parent is local on the finer level
        kid_of_owned = (owner_c[par_f] == rank).any(axis=1)
        assert (fine.domain.g2l[np.nonzero(kid_of_owned)[0]] >= 0).all(), "every child of an owned coarse vertex must be local on the finer level"
        plans.append(coarse)
    return plans


def partition_plan(prob: Problem, nparts: int, rank: int, n_global_aggregates: int = None):
    """Everything rank `rank` needs for ``gmpnp_create_partition``: (LocalDomain, local perm, partition dict) of the one-level
    hierarchy of `prob`."""
    plan = partition_hierarchy([(prob, None, None)], nparts, rank, n_global_aggregates)[0]
    return plan.domain, plan.perm, plan.part


class PartitionedSolver:
    """One mesh-partitioned problem solved by libgmpnp.so across `nparts` ranks (SURVEY section 8e / BASELINE configs[3]).

    ``PartitionedSolver(prob, nparts)``                every rank in THIS process on one GPU (rehearsal: the exchanges are device
                                                       copies between the handles) — what a single-GPU box can run;
    ``PartitionedSolver(prob, nparts, rank=r, ...)``   one rank per process / GPU; the RCCL communicator is created inside the
                                                       library from an id that rank 0 makes and ``torch.distributed`` broadcasts.
    The Krylov and Newton loops run in the library; Python only scatters / gathers states and per-step boundary values."""

    def __init__(self, prob: Problem, nparts: int, rank: int = None, device_id: int = 0, n_global_aggregates: int = None,
                 use_torch_dist: bool = True, transport: str = "rccl", exchange_form: int = 0, levels=None, ml_theta: float = 2.0,
                 ml_sweeps: int = 4, **device_kwargs):
        """``transport`` (one rank per process only): "peer" — peer mailboxes: every collective is one kernel launch per rank
        that stores into the other ranks' IPC-mapped mailboxes (xGMI between GPUs; also works for ranks sharing a card);
        "rccl" — collectives inside the library over RCCL; "host" — the library stages every collective through pinned host
        memory and calls back into ``torch.distributed`` (any backend, e.g. gloo).  ``exchange_form`` (peer transport): 0 = the
        exchange of a half-iteration rides inside the next launch where that launch is resident (2 launches per BiCGStab iteration),
        1 = separate exchange launches (4); every rank must pass the same value (gmpnp_group_set_exchange_form).
        ``levels`` (``problem.pore_hierarchy``, finest first; ``prob`` is its finest problem): the geometric multilevel term of the
        preconditioner across the partitions (``partition_hierarchy``; gmpnp_attach_coarse_level + gmpnp_group_attach_coarse_group),
        ``ml_theta`` / ``ml_sweeps`` as on one GPU.  Not over the peer transport (refused by the library)."""
        if getattr(prob, "stern", None) is not None:
            raise ValueError("partition: the Stern boundary condition is not available in a partitioned solve")
        if getattr(prob, "kinetics", None) is not None:
            raise ValueError("partition: the surface kinetics are not available in a partitioned solve")
        if getattr(prob, "galvanostat", None) is not None:
            raise ValueError("partition: the galvanostat is not available in a partitioned solve")
        from ctypes import c_void_p
        if rank is not None:
            # one rank per process: torch.distributed carries the set-up (mailbox handles, communicator id, host-staged collectives).
            # PyTorch first, THEN libgmpnp.so: the library then binds to the HIP runtime PyTorch ships instead of bringing the
            # system's into the same process (README: two HIP runtimes on one GPU do not mix)
            import torch  # noqa: F401
        from . import backend
        self.backend = backend
        self.lib = backend.load_library()
        self.nparts, self.rank = nparts, rank
        self.nv_global, self.nf = prob.coords.shape[0], prob.nf
        self.ranks = list(range(nparts)) if rank is None else [rank]
        self._comm, self._group, self._level_groups = c_void_p(), c_void_p(), []
        self.transport = transport if rank is not None else "in-process"
        # handles: [local rank] of the finest level, [level k >= 1][local rank] of the coarse levels of the multilevel term
        plans = [partition_hierarchy(levels or [(prob, None, None)], nparts, r, n_global_aggregates) for r in self.ranks]
        self.doms = [pl[0].domain for pl in plans]
        self.devs = [backend.DeviceSolver(pl[0].domain.problem, device_id=device_id, perm=pl[0].perm, partition=pl[0].part, **device_kwargs)
                     for pl in plans]
        self.level_devs = [[backend.DeviceSolver(pl[k].domain.problem, device_id=device_id, perm=pl[k].perm, partition=pl[k].part, shared_device=1)
                            for pl in plans] for k in range(1, len(plans[0]))]
        for i, pl in enumerate(plans):   # every level attached below the next-finer one of its rank
            backend.attach_level_chain([self.devs[i]] + [devs[i] for devs in self.level_devs], [p.parents for p in pl], ml_theta, ml_sweeps)
        if self.transport == "peer":
            self._connect_peer(exchange_form)
        elif self.transport == "host":
            self._connect_host()
        elif rank is None:
            self._group = self._new_group(self.devs)   # in-process: the exchanges are device copies between the handles
        else:
            self._connect_rccl(device_id, use_torch_dist)
        # one group per coarse level over the same transport, attached below the next-finer level's group: it carries that level's
        # collectives (gmpnp_group_attach_coarse_group)
        finer = self._group
        for devs in self.level_devs:
            self._level_groups.append(self._new_group(devs))
            self._check(self.lib.gmpnp_group_attach_coarse_group(finer, self._level_groups[-1]))
            finer = self._level_groups[-1]

    def _new_group(self, devs, mailbox=None):
        """A group of the handles `devs` (one level of the local ranks) over this solver's transport: the peer form hands this
        rank's mailbox handle back in `mailbox`, the host form takes the callbacks, the others the communicator (none in-process)."""
        from ctypes import byref, c_void_p, create_string_buffer
        g = c_void_p()
        if self.transport == "peer":
            self._check(self.lib.gmpnp_group_peer_begin(devs[0]._h, byref(g), mailbox if mailbox is not None else create_string_buffer(self.backend.PEER_HANDLE_BYTES)))
        elif self.transport == "host":
            self._check(self.lib.gmpnp_group_create_hosted(devs[0]._h, byref(self._host_transport), byref(g)))
        else:
            handles = (c_void_p * len(devs))(*[d._h for d in devs])
            self._check(self.lib.gmpnp_group_create(len(devs), handles, self._comm if self.rank is not None else None, byref(g)))
        return g

    def _connect_peer(self, exchange_form):
        """Peer mailboxes: gather every rank's mailbox handle, map them, agree on the exchange form."""
        from ctypes import create_string_buffer
        import torch
        import torch.distributed as tdist
        backend, nparts = self.backend, self.nparts
        if not (tdist.is_available() and tdist.is_initialized() and tdist.get_world_size() == nparts):
            raise RuntimeError("the peer transport needs an initialised torch.distributed group of %d ranks (to gather the mailbox handles)" % nparts)
        # Every step is agreed on by ALL ranks before anyone goes on: a rank that cannot allocate or map a mailbox (no peer
        # access to a GPU, IPC refused) must not leave the others waiting in a collective it never joins.
        mine = create_string_buffer(backend.PEER_HANDLE_BYTES)
        err = None
        try:
            self._group = self._new_group(self.devs, mine)
        except backend.GmpnpError as e:
            err = e
        dev = _default_group_device(tdist)
        t = torch.tensor(list(mine.raw) + [0 if err is None else 1], dtype=torch.uint8, device=dev)
        parts = [torch.empty_like(t) for _ in range(nparts)]
        tdist.all_gather(parts, t)      # also the point after which every rank's mailbox exists
        rows = [x.cpu().tolist() for x in parts]
        if err is None and not any(r[-1] for r in rows):
            allh = create_string_buffer(backend.PEER_HANDLE_BYTES * nparts)
            allh.raw = b"".join(bytes(r[:-1]) for r in rows)
            try:
                self._check(self.lib.gmpnp_group_peer_connect(self._group, allh))
            except backend.GmpnpError as e:
                err = e
        elif err is None:
            err = RuntimeError("rank(s) %s could not set up a mailbox" % [q for q, r in enumerate(rows) if r[-1]])
        flag = torch.tensor([0 if err is None else 1], dtype=torch.int32, device=dev)
        tdist.all_reduce(flag, op=tdist.ReduceOp.MAX)   # (also: every mailbox is mapped everywhere from here on)
        if int(flag[0]):
            self.transport = "peer (failed)"
            self.close()
            raise RuntimeError("peer-mailbox transport not available: %s" % (err if err is not None else "another rank could not map a mailbox"))
        # All ranks must run the SAME form (form 2 leaves the exchange behind the last launch of a solve out, so the sequence
        # numbers of the two forms drift apart): a rank whose launch would not be resident with the exchange workgroups in
        # front takes everybody back to separate launches.
        self._check(self.lib.gmpnp_group_set_exchange_form(self._group, int(exchange_form)))
        form = torch.tensor([int(self.lib.gmpnp_group_exchange_form(self._group))], dtype=torch.int32, device=dev)
        tdist.all_reduce(form, op=tdist.ReduceOp.MIN)
        if int(form[0]) != 2:
            self._check(self.lib.gmpnp_group_set_exchange_form(self._group, 1))

    def _connect_host(self):
        """Host-staged collectives: the library calls back into torch.distributed."""
        self._make_host_transport(self.rank, self.nparts)
        self._group = self._new_group(self.devs)

    def _connect_rccl(self, device_id, use_torch_dist):
        """The RCCL communicator inside the library, from an id that rank 0 makes and torch.distributed broadcasts."""
        from ctypes import byref, create_string_buffer
        backend, rank, nparts = self.backend, self.rank, self.nparts
        idbuf = create_string_buffer(backend.COMM_ID_BYTES)
        if nparts > 1 or use_torch_dist:
            import torch
            import torch.distributed as tdist
            if tdist.is_available() and tdist.is_initialized():
                if rank == 0:
                    self._check(self.lib.gmpnp_comm_unique_id(idbuf))
                t = torch.tensor(list(idbuf.raw), dtype=torch.uint8, device=_default_group_device(tdist))
                tdist.broadcast(t, src=0)
                idbuf = create_string_buffer(backend.COMM_ID_BYTES)
                idbuf.raw = bytes(t.cpu().tolist())
            elif nparts == 1:
                self._check(self.lib.gmpnp_comm_unique_id(idbuf))
            else:
                raise RuntimeError("torch.distributed is not initialised: the communicator id cannot reach the other ranks")
        else:
            self._check(self.lib.gmpnp_comm_unique_id(idbuf))
        self._check(self.lib.gmpnp_comm_create(idbuf, rank, nparts, device_id, byref(self._comm)))
        self._group = self._new_group(self.devs)

    def _check(self, code):
        if code != self.backend.OK:
            raise self.backend.GmpnpError(code, self.lib.gmpnp_last_error().decode())

    def _make_host_transport(self, rank, nparts):
        """The two callbacks of gmpnp_host_transport_t on torch.distributed (CPU tensors that alias the library's pinned
        staging buffers: no copies on this side)."""
        import torch
        import torch.distributed as tdist
        backend = self.backend
        if not (tdist.is_available() and tdist.is_initialized() and tdist.get_world_size() == nparts):
            raise RuntimeError("the host transport needs an initialised torch.distributed group of %d ranks" % nparts)

        # host tensors need a CPU-capable backend: a gloo group next to an nccl default group
        grp = tdist.new_group(backend="gloo") if tdist.get_backend() == "nccl" else None
        self._host_group = grp

        def view(ptr, n):
            return np.ctypeslib.as_array(ptr, shape=(int(n),))

        ar, ex = host_transport_callbacks(grp)

        def allreduce(_user, buf, n):
            return ar(view(buf, n))

        def exchange(_user, n_nb, nb_rank, s_off, s_cnt, s_buf, r_off, r_cnt, r_buf):
            n_s = max([0] + [s_off[j] + s_cnt[j] for j in range(n_nb)])
            n_r = max([0] + [r_off[j] + r_cnt[j] for j in range(n_nb)])
            return ex([int(nb_rank[j]) for j in range(n_nb)], [int(s_off[j]) for j in range(n_nb)], [int(s_cnt[j]) for j in range(n_nb)],
                      view(s_buf, max(n_s, 1)), [int(r_off[j]) for j in range(n_nb)], [int(r_cnt[j]) for j in range(n_nb)], view(r_buf, max(n_r, 1)))

        self._cb = (backend.ALLREDUCE_FN(allreduce), backend.EXCHANGE_FN(exchange))   # keep the thunks alive
        t = backend.CHostTransport()
        t.rank, t.size, t.allreduce, t.exchange, t.user = rank, nparts, self._cb[0], self._cb[1], None
        self._host_transport = t

    # ---- state in GLOBAL (file) vertex order -------------------------------------------------------------------------
    def set_state(self, u_global=None, un_global=None):
        for dom, dev in zip(self.doms, self.devs):
            dev.set_state(None if u_global is None else scatter_local(dom, np.asarray(u_global)),
                          None if un_global is None else scatter_local(dom, np.asarray(un_global)))

    def set_dirichlet(self, dofs, vals):
        """The GLOBAL Dirichlet set (file-order dofs); every local handle gets its part + identity rows on its ghost dofs
        (their values never enter anything: ghost rows are masked out of the residual)."""
        nf = self.nf
        dofs, vals = np.asarray(dofs, dtype=np.int64), np.asarray(vals, dtype=np.float64)
        for dom, dev in zip(self.doms, self.devs):
            lv = dom.g2l[dofs // nf]
            keep = (lv >= 0) & (lv < dom.n_owned)
            gh = np.arange(dom.n_owned * nf, len(dom.lverts) * nf, dtype=np.int64)
            dev.set_dirichlet(np.concatenate([lv[keep] * nf + dofs[keep] % nf, gh]), np.concatenate([vals[keep], np.zeros(len(gh))]))

    def owned_state(self, previous=False):
        """[(owned global vertex ids, (n_owned, nf) values)] of the local ranks."""
        out = []
        for dom, dev in zip(self.doms, self.devs):
            out.append((dom.owned, dev.get_state(previous).reshape(-1, self.nf)[:dom.n_owned]))
        return out

    def get_state(self):
        """Global state (file order) — complete in the in-process form; with one rank per process all-gathered through
        torch.distributed when it is initialised, else only this rank's rows are filled."""
        out = np.zeros((self.nv_global, self.nf))
        for ids, vals in self.owned_state():
            out[ids] = vals
        if self.rank is not None and self.nparts > 1:
            import torch
            import torch.distributed as tdist
            if tdist.is_available() and tdist.is_initialized():
                t = torch.from_numpy(out).to(_default_group_device(tdist))
                tdist.all_reduce(t)
                out = t.cpu().numpy()
        return out.ravel()

    def column_select(self, fields, ranks):
        """k-th smallest values of vertex columns of u over every rank's OWNED rows (gmpnp_group_column_select: collective over the
        group's transport, the counts all-reduced inside the library): (values, nan flag), identical on every rank."""
        return self.backend.column_select_call(self.lib.gmpnp_group_column_select, self._group, fields, ranks, self._check)

    def species_budget(self):
        """(nf, 8) species-budget table of the WHOLE problem (gmpnp_group_species_budget: every rank's owned-row table summed over
        the group's transport inside the library, no gather of the state; collective, identical on every rank)."""
        return self.backend.species_budget_call(self.lib.gmpnp_group_species_budget, self._group, self.nf, self._check)

    def comm_selftest(self, n=4096):
        """Send-to-self + receive + all-reduce through the library's RCCL bindings; returns the largest error."""
        from ctypes import byref, c_double
        err = c_double()
        self._check(self.lib.gmpnp_comm_selftest(self._comm, n, byref(err)))
        return err.value

    def exchange_form(self):
        """2 = the peer exchange rides inside the next half-iteration's launch, 1 = separate launches, 0 = another transport."""
        return int(self.lib.gmpnp_group_exchange_form(self._group))

    def selftest(self):
        """One all-reduce and one ghost-row exchange with self-checking contents over this group's transport
        (gmpnp_group_selftest; collective); returns the largest deviation this process saw (0.0 expected)."""
        from ctypes import byref, c_double
        err = c_double(-1.0)
        self._check(self.lib.gmpnp_group_selftest(self._group, byref(err)))
        return err.value

    def newton_solve(self, options, error_on_nonconvergence=True):
        from ctypes import byref
        st = self.backend.CNewtonStats()
        code = self.lib.gmpnp_group_newton_solve(self._group, byref(options), byref(st))
        stats = self.backend.DeviceSolver.stats_dict(st)
        if code == self.backend.ERR_NOT_CONVERGED and not error_on_nonconvergence:
            return stats
        self._check(code)
        return stats

    def assign_previous(self):
        self._check(self.lib.gmpnp_group_assign_previous(self._group))

    def close(self):
        if getattr(self, "transport", None) == "peer" and getattr(self, "_group", None):
            try:   # no rank unmaps / frees a mailbox another rank may still store into
                import torch.distributed as tdist
                if tdist.is_available() and tdist.is_initialized():
                    tdist.barrier()
            except Exception:  # noqa: BLE001
                pass
        if getattr(self, "_group", None):
            self.lib.gmpnp_group_destroy(self._group)
            self._group = None
        for g in getattr(self, "_level_groups", []):
            self.lib.gmpnp_group_destroy(g)
        self._level_groups = []
        for d in getattr(self, "devs", []):
            d.close()
        self.devs = []
        for devs in getattr(self, "level_devs", []):
            for d in devs:
                d.close()
        self.level_devs = []
        if getattr(self, "_comm", None) and self._comm.value:
            self.lib.gmpnp_comm_destroy(self._comm)
            self._comm = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _default_group_device(tdist):
    """Where the tensors of a collective on the default group live: the GPU under nccl, else the host."""
    return "cuda" if tdist.get_backend() == "nccl" else "cpu"


def init_process_group_from_env(backend="nccl", device=None):
    """The process group of a process that ``torch.distributed.run`` started: RANK / WORLD_SIZE / LOCAL_RANK from the environment
    and, with a world size above 1, the default group initialised (``backend`` "nccl": bound to cuda:`device`, LOCAL_RANK by
    default; any other backend as it is).  Returns (rank, world, local rank, torch.distributed or None)."""
    import os
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world <= 1:
        return rank, world, local, None
    import torch
    import torch.distributed as tdist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if backend == "nccl":
        dev = local if device is None else device
        torch.cuda.set_device(dev)
        tdist.init_process_group(backend=backend, device_id=torch.device("cuda", dev))
    else:
        tdist.init_process_group(backend=backend)
    return rank, world, local, tdist


def host_transport_callbacks(group=None):
    """The two collectives of ``gmpnp_host_transport_t`` on ``torch.distributed`` (any backend with CPU tensors, e.g. gloo), as
    functions of NumPy arrays that ALIAS the caller's buffers (the library's pinned staging memory: no copies on this side):
    ``allreduce(buf)`` sums in place over the ranks; ``exchange(nb_rank, s_off, s_cnt, s_buf, r_off, r_cnt, r_buf)`` sends
    ``s_buf[s_off[j] : s_off[j] + s_cnt[j]]`` to neighbour j and receives ``r_buf[r_off[j] : ...]`` from it.  Both return 0, or 1
    after printing the traceback (the library turns that into GMPNP_ERR_HIP)."""
    import torch
    import torch.distributed as tdist

    def allreduce(buf):
        try:
            tdist.all_reduce(torch.from_numpy(buf), group=group)
            return 0
        except Exception:  # noqa: BLE001
            import traceback
            traceback.print_exc()
            return 1

    def exchange(nb_rank, s_off, s_cnt, s_buf, r_off, r_cnt, r_buf):
        try:
            sv, rv = torch.from_numpy(s_buf), torch.from_numpy(r_buf)
            ops = []
            for j, q in enumerate(nb_rank):
                if s_cnt[j]:
                    ops.append(tdist.P2POp(tdist.isend, sv[s_off[j]:s_off[j] + s_cnt[j]], int(q), group=group))
                if r_cnt[j]:
                    ops.append(tdist.P2POp(tdist.irecv, rv[r_off[j]:r_off[j] + r_cnt[j]], int(q), group=group))
            for req in (tdist.batch_isend_irecv(ops) if ops else []):
                req.wait()
            return 0
        except Exception:  # noqa: BLE001
            import traceback
            traceback.print_exc()
            return 1

    return allreduce, exchange


def scatter_local(dom: LocalDomain, u_global):
    return u_global.reshape(-1, dom.nf)[dom.lverts].ravel().copy()
