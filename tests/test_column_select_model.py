"""The column select of csrc/gmpnp_stats.h restated in NumPy (order-preserving 64-bit keys, eight 8-bit radix passes, per-rank
histograms summed as an all-reduce would) and checked against np.sort; and the driver's --partitions flag."""
import numpy as np
import pytest

SIGN = np.uint64(1 << 63)


def keys(v):
    """The kernel's sel_key: -0.0 keys as +0.0; sign set -> all bits flipped, else the sign bit set."""
    b = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64).copy()
    b[b == SIGN] = np.uint64(0)
    neg = (b & SIGN) != 0
    return np.where(neg, ~b, b | SIGN)


def value(k):
    k = np.uint64(k)
    b = k & ~SIGN if k & SIGN else ~k
    return np.array([b], dtype=np.uint64).view(np.float64)[0]


def radix_select(parts, rank):
    """k-th smallest over the concatenation of `parts` (one array per rank): per pass every rank histograms the keys that match
    the prefix, the 256 counts are summed over the ranks, and the bucket holding the remaining rank extends the prefix."""
    ks = [keys(p) for p in parts]
    prefix, krem = np.uint64(0), int(rank)
    for pas in range(8):
        shift = np.uint64(56 - 8 * pas)
        himask = np.uint64(0) if pas == 0 else ~np.uint64(0) << (shift + np.uint64(8))
        counts = np.zeros(256, dtype=np.int64)
        for k in ks:
            m = k[((k ^ prefix) & himask) == 0]
            counts += np.bincount(((m >> shift) & np.uint64(255)).astype(np.int64), minlength=256)
        incl = np.cumsum(counts)
        b = int(np.searchsorted(incl, krem, side="right"))
        assert b < 256, "rank beyond the count"
        krem -= int(incl[b] - counts[b])
        prefix |= np.uint64(b) << shift
    return value(prefix)


def split(a, nranks, rng):
    """uneven contiguous pieces (some possibly empty) of a shuffled copy of `a`"""
    a = rng.permutation(a)
    cuts = np.sort(rng.integers(0, len(a) + 1, size=nranks - 1))
    return np.split(a, cuts)


COLUMNS = {
    "odd": lambda rng: rng.standard_normal(101),
    "even": lambda rng: rng.standard_normal(100) * 1e3,
    "ties": lambda rng: rng.integers(-3, 4, size=64).astype(np.float64),
    "constant": lambda rng: np.full(37, 0.8125),
    "signed_zeros": lambda rng: np.array([0.0, -0.0, -0.0, 0.0, 1.0, -1.0, -0.0]),
    "subnormals": lambda rng: np.array([5e-324, -5e-324, 2.2e-308, -2.2e-308, 1e-310, -1e-310, 0.0, -0.0, 1e-300]),
    "infinities": lambda rng: np.array([np.inf, -np.inf, 1.0, -np.inf, 0.0, np.inf, -1e308, 1e308]),
    "concentrations": lambda rng: 1.0 + 1e-6 * rng.standard_normal(257),
}


@pytest.mark.parametrize("nranks", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("name", sorted(COLUMNS))
def test_radix_select_equals_np_sort(name, nranks):
    rng = np.random.default_rng([len(name), nranks, sum(map(ord, name))])
    a = COLUMNS[name](rng)
    ref = np.sort(a)
    parts = split(a, nranks, rng)
    assert sum(len(p) for p in parts) == len(a)
    for k in range(len(a)):
        got = radix_select(parts, k)
        assert got == ref[k], (k, got, ref[k])
        assert not np.signbit(got) or got != 0.0, "a zero comes back as +0.0"


def test_medians_from_the_select_match_column_medians():
    """The middle element, or np.mean of the two middle ones, bit for bit what solver.column_medians gives."""
    from gmpnp_amd.solver import column_medians
    rng = np.random.default_rng(7)
    for n in (1, 2, 9, 10, 3679):
        vals = rng.standard_normal((n, 9)) * 10.0 ** rng.integers(-3, 3, size=9)
        parts = split(np.arange(n), 4, rng)
        want = column_medians(vals, (1, 2, 3, 7))
        h = n // 2
        got = []
        for c in (1, 2, 3, 7):
            cols = [vals[idx, c] for idx in parts]
            got.append(radix_select(cols, h) if n % 2 else np.mean(np.array([radix_select(cols, h - 1), radix_select(cols, h)])))
        assert np.array_equal(np.array(got).view(np.uint64), np.asarray(want).view(np.uint64))


def test_key_order_is_the_order_of_the_doubles():
    a = np.array([-np.inf, -1e308, -1.0, -5e-324, 0.0, 5e-324, 1.0, 1e308, np.inf])
    k = keys(a)
    assert all(int(k[i]) < int(k[i + 1]) for i in range(len(k) - 1))
    assert keys(np.array([-0.0]))[0] == keys(np.array([0.0]))[0]
    for v in a:
        assert value(keys(np.array([v]))[0]) == v


def test_driver_parser_has_partitions_and_defaults_to_serial():
    from gmpnp_amd import pore3d
    p = pore3d.build_parser()
    a = p.parse_args(["--L=10e-9", "--partitions", "4", "--refine", "2", "--multilevel"])
    assert a.partitions == 4 and a.refine == 2 and a.multilevel
    assert p.parse_args([]).partitions is None


def test_partition_setup_without_torchrun(monkeypatch):
    """No torch.distributed.run: every partition in this process, nothing initialised; a world of another size is refused."""
    from gmpnp_amd import pore3d
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert pore3d.partition_setup(3) == ((3, None), {}, None)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        pore3d.partition_setup(3)
