"""Partition plans of the nested levels of the multilevel term (gmpnp_amd/dist.py ``partition_hierarchy``), checked without a GPU:
the invariants the library's partitioned transfers rely on, and a NumPy model of the partitioned prolongation P and restriction
P^T (local tables, a modelled halo exchange over the plans' send / receive lists) against the serial P and P^T, bit for bit."""
import numpy as np
import pytest

from conftest import _pore


@pytest.fixture(scope="module", params=[1, 2], ids=["refine1", "refine2"])
def hierarchy(request):
    from gmpnp_amd.problem import pore_hierarchy
    pp, mesh, _, _ = _pore(10e-9, 5e-9)
    return pore_hierarchy(pp, mesh, request.param)


def _plans(levels, nparts):
    from gmpnp_amd import dist
    return [dist.partition_hierarchy(levels, nparts, r) for r in range(nparts)]


def _lverts(plan):
    return np.concatenate([plan.domain.owned, plan.domain.ghosts])


def _exchange(plans_k, local):
    """Ghost rows of every rank's local vector from their owners, through the plans' send / receive lists (what the library's
    halo exchange does with them)."""
    out = [v.copy() for v in local]
    for r, pl in enumerate(plans_k):
        part = pl.part
        for j, q in enumerate(part["neighbour_rank"]):
            qp = plans_k[q].part
            jj = list(qp["neighbour_rank"]).index(r)
            src = qp["send_vertices"][qp["send_ptr"][jj]:qp["send_ptr"][jj + 1]]
            dst = part["recv_vertices"][part["recv_ptr"][j]:part["recv_ptr"][j + 1]]
            assert len(src) == len(dst)
            out[r][dst] = local[q][src]
    return out


@pytest.mark.parametrize("nparts", [1, 2, 3, 4])
def test_level_plans_keep_the_invariants(hierarchy, nparts):
    from gmpnp_amd import dist
    plans = _plans(hierarchy, nparts)
    for r in range(nparts):   # the finest level is the two-level solve's plan, unchanged
        dom, perm, part = dist.partition_plan(hierarchy[0][0], nparts, r)
        assert np.array_equal(plans[r][0].perm, perm) and np.array_equal(plans[r][0].domain.ghosts, dom.ghosts)
        for key in ("vertex_aggregate", "send_ptr", "send_vertices", "recv_ptr", "recv_vertices", "neighbour_rank"):
            assert np.array_equal(plans[r][0].part[key], part[key]), key
    for k in range(len(hierarchy)):
        nv = hierarchy[k][0].coords.shape[0]
        seen = np.zeros(nv, dtype=int)
        slabs = []
        for r in range(nparts):
            pl = plans[r][k]
            lv = _lverts(pl)
            seen[pl.domain.owned] += 1
            ag, own = pl.part["vertex_aggregate"][pl.perm], pl.part["vertex_owned"][pl.perm]
            assert (np.diff(ag) >= 0).all()                                             # the local order runs through the slabs
            first, last = np.nonzero(own)[0][[0, -1]]
            assert own[first:last + 1].all() and own.sum() == pl.domain.n_owned
            assert set(ag[own == 1]).isdisjoint(set(ag[own == 0]))                      # a slab is all owned or all ghost
            slabs.append(set(ag[own == 1].tolist()))
            assert np.array_equal(pl.owner[lv[:pl.domain.n_owned]], np.full(pl.domain.n_owned, r))
            # halo lists: what r sends to q is, entry by entry, what q expects from r
            for j, q in enumerate(pl.part["neighbour_rank"]):
                qpl = plans[q][k]
                jj = list(qpl.part["neighbour_rank"]).index(r)
                mine = lv[pl.part["send_vertices"][pl.part["send_ptr"][j]:pl.part["send_ptr"][j + 1]]]
                theirs = _lverts(qpl)[qpl.part["recv_vertices"][qpl.part["recv_ptr"][jj]:qpl.part["recv_ptr"][jj + 1]]]
                assert len(mine) > 0 and np.array_equal(mine, theirs)
                assert (pl.owner[mine] == r).all()
        assert (seen == 1).all()
        for a in range(nparts):                                                         # no slab straddles two ranks
            for b in range(a + 1, nparts):
                assert slabs[a].isdisjoint(slabs[b])
        if k == 0:
            continue
        par = np.asarray(hierarchy[k - 1][2])
        copy = -np.ones(nv, dtype=np.int64)
        is_copy = par[:, 0] == par[:, 1]
        copy[par[is_copy, 0]] = np.nonzero(is_copy)[0]
        assert (copy >= 0).all()
        for r in range(nparts):
            fine, coarse = plans[r][k - 1], plans[r][k]
            assert np.array_equal(coarse.owner, fine.owner[copy])                       # ownership follows the copies
            assert np.array_equal(coarse.aggregate, fine.aggregate[copy])
            lvf, lvc = _lverts(fine), _lverts(coarse)
            lp = fine.parents
            assert lp.shape == (len(lvf), 2) and (lp[:fine.domain.n_owned] >= 0).all()  # both parents of an owned fine vertex are local
            ok = lp >= 0
            assert np.array_equal(lvc[lp[ok]], par[lvf][ok])                            # ... and they are the right ones
            kids = np.nonzero(np.isin(par, coarse.domain.owned).any(axis=1))[0]
            assert np.isin(kids, lvf).all()                                             # every child of an owned coarse vertex is local
            # the coarse local order is the fine slab order of the copies
            assert (np.diff(fine.pos[copy[lvc[coarse.perm]]]) > 0).all()


def _serial_transfers(par, pos_f, bc_f, bc_c, nf, wc, wf):
    """Serial mask_f P wc and mask_c P^T mask_f wf (children summed in ascending fine slab position)."""
    a, b = par[:, 0], par[:, 1]
    pw = np.where((a == b)[:, None], wc[a], 0.5 * (wc[a] + wc[b]))
    pw[bc_f] = 0.0
    src = np.where(bc_f, 0.0, wf)
    rt = np.zeros_like(wc)
    for I in np.argsort(pos_f, kind="stable"):
        if a[I] == b[I]:
            rt[a[I]] += src[I]
        else:
            rt[a[I]] += 0.5 * src[I]
            rt[b[I]] += 0.5 * src[I]
    rt[bc_c] = 0.0
    return pw, rt


@pytest.mark.parametrize("nparts", [1, 2, 3, 4])
def test_partitioned_transfers_equal_the_serial_ones(hierarchy, nparts):
    plans = _plans(hierarchy, nparts)
    rng = np.random.default_rng(7 + nparts)
    for k in range(1, len(hierarchy)):
        prob_f, prob_c = hierarchy[k - 1][0], hierarchy[k][0]
        nf = prob_f.nf
        par = np.asarray(hierarchy[k - 1][2])
        nvf, nvc = prob_f.coords.shape[0], prob_c.coords.shape[0]
        bc_f = np.zeros(nvf * nf, dtype=bool)
        bc_f[prob_f.bc_dofs] = True
        bc_c = np.zeros(nvc * nf, dtype=bool)
        bc_c[prob_c.bc_dofs] = True
        bc_f, bc_c = bc_f.reshape(nvf, nf), bc_c.reshape(nvc, nf)
        wc = rng.standard_normal((nvc, nf))
        wf = rng.standard_normal((nvf, nf))
        pos_f = plans[0][k - 1].pos
        want_p, want_r = _serial_transfers(par, pos_f, bc_f, bc_c, nf, wc, wf)
        fine = [pl[k - 1] for pl in plans]
        coarse = [pl[k] for pl in plans]
        # P: owned coarse rows, their ghost rows from the owners, then every rank prolongs onto its owned fine rows
        lc = []
        for pl in coarse:
            v = np.full((len(_lverts(pl)), nf), np.nan)
            v[:pl.domain.n_owned] = wc[pl.domain.owned]
            lc.append(v)
        lc = _exchange(coarse, lc)
        got_p = np.full((nvf, nf), np.nan)
        for fpl, v in zip(fine, lc):
            n = fpl.domain.n_owned
            a, b = fpl.parents[:n, 0], fpl.parents[:n, 1]
            pw = np.where((a == b)[:, None], v[a], 0.5 * (v[a] + v[b]))
            pw[bc_f[fpl.domain.owned]] = 0.0
            got_p[fpl.domain.owned] = pw
        assert np.array_equal(got_p, want_p)
        # P^T: owned fine rows and the true Dirichlet flags, their ghost rows from the owners, then every rank sums the children
        # of its owned coarse vertices (local on the finer level) in the local slab order
        lf, lm = [], []
        for fpl in fine:
            nl, n = len(_lverts(fpl)), fpl.domain.n_owned
            v = np.full((nl, nf), np.nan)
            v[:n] = wf[fpl.domain.owned]
            m = np.ones((nl, nf))          # a partition handle flags every ghost dof: the mask has to come from the owners
            m[:n] = bc_f[fpl.domain.owned]
            lf.append(v)
            lm.append(m)
        lf, lm = _exchange(fine, lf), _exchange(fine, lm)
        got_r = np.full((nvc, nf), np.nan)
        for fpl, cpl, v, m in zip(fine, coarse, lf, lm):
            src = np.where(m != 0.0, 0.0, v)
            nc = cpl.domain.n_owned
            acc = np.zeros((len(_lverts(cpl)), nf))
            lvf = _lverts(fpl)
            for I in np.argsort(fpl.pos[lvf], kind="stable"):
                a, b = fpl.parents[I]
                if a == b:
                    if 0 <= a < nc:
                        acc[a] += src[I]
                    continue
                for p in (a, b):
                    if 0 <= p < nc:
                        acc[p] += 0.5 * src[I]
            acc[:nc][bc_c[cpl.domain.owned]] = 0.0
            got_r[cpl.domain.owned] = acc[:nc]
        assert np.array_equal(got_r, want_r)
