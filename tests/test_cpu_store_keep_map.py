"""The slab arithmetic behind the store policy of the CG's stencil launches (stencil.hip dirsplit_s_block, PipeArgs::keep_from; tunable cg_store_keep_mb) restated in
numpy: the slab q of a workgroup in dispatch order, forwards and under sweep_rev, with fdiv_nb's magic-number division, and the flag plain_store = (q >= keep_from).
Every virtual block is run once and lies in one slab of the map (pass * LT + t of pipe_map): slab q forwards, slab nslab - 1 - q backwards; the workgroups that store
plain are those of the last K_s slabs in dispatch order, whatever the direction.  Geometries: cpr = 1, 4 (two passes, both parities and one), 3 and 6 (no power of two)."""
import numpy as np
import pytest


def make_fastdiv(d):
    """make_fastdiv of lqcd_internal.h: (m, sh, d)"""
    if d == 1:
        return 0, 0, 1
    s = 0
    while (1 << s) < d:
        s += 1
    return ((1 << (31 + s)) // d + 1) & 0xFFFFFFFF, s - 1, d


def fdiv_nb(n, f):
    m, sh, d = f
    q = ((np.asarray(n, dtype=np.uint64) * np.uint64(m)) >> np.uint64(32)) >> np.uint64(sh)      # __umulhi(n, m) >> sh
    return np.asarray(n, dtype=np.int64) if d == 1 else q.astype(np.int64)


def block(b, both, cpr, nslab, sweep_rev, keep_from):
    """dirsplit_s_block: (virtual block, slab in dispatch order, keep) of the workgroups b; keep = -1 where keep_from < 0"""
    b = np.asarray(b, dtype=np.int64)
    j = b >> 3
    pb = (j & 1) if both else 0 * j
    j = (j >> 1) if both else j
    q = fdiv_nb(j, make_fastdiv(max(1, cpr)))
    keep = np.where(q >= keep_from, 1, 0) if keep_from >= 0 else np.full_like(b, -1)
    vb = b
    if sweep_rev:
        j = j + (nslab - 1 - 2 * q) * cpr
        vb = ((2 * j + pb if both else j) << 3) | (b & 7)
    return vb, q, keep


def slab_of(vb, both, cpr, LT):
    """pass * LT + t of pipe_map for the virtual block vb"""
    j = np.asarray(vb, dtype=np.int64) >> 3
    j = (j >> 1) if both else j
    per_pass = cpr * LT
    pas = j // per_pass
    return pas * LT + (j - pas * per_pass) // cpr


# (cpr, LT, passes = nsub / 8): 16.8.8.4, 16.16.16.8 with xcd_nsub = 8, 32^3 x 64 (two passes), and chunks per sub-domain and slice that are no power of two
GEOMETRIES = [(1, 4, 1), (4, 8, 1), (4, 64, 2), (3, 6, 1), (6, 4, 2)]


def keeps(nslab):
    return sorted({0, 1, 2, nslab // 2, nslab - 1, nslab})


@pytest.mark.parametrize("both", [1, 0])
@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: "cpr%d.LT%d.pass%d" % g)
def test_every_virtual_block_gets_one_slab_and_the_last_slabs_in_dispatch_order_store_plain(geo, both):
    cpr, LT, passes = geo
    nslab = passes * LT
    par = 2 if both else 1
    nvirt = 8 * par * cpr * nslab
    b = np.arange(nvirt)
    for rev in (0, 1):
        for K in keeps(nslab):
            keep_from = nslab - min(K, nslab)      # pipe_sweep_args
            vb, q, keep = block(b, both, cpr, nslab, rev, keep_from)
            assert np.array_equal(q, (b >> 3) // par // cpr)            # the magic-number division is exact on the launch's range
            assert np.all(np.diff(q) >= 0) and q[0] == 0 and q[-1] == nslab - 1      # q is the dispatch order
            assert np.array_equal(np.sort(vb), b)                         # a permutation: every virtual block exactly once
            assert np.array_equal(vb & 7, b & 7)                          # on its XCD
            want = nslab - 1 - q if rev else q
            assert np.array_equal(slab_of(vb, both, cpr, LT), want)     # one slab per virtual block: q forwards, its mirror backwards
            assert np.all(np.bincount(want, minlength=nslab) == 8 * par * cpr)
            assert set(np.unique(keep)) <= {0, 1}
            assert sorted(np.unique(q[keep == 1])) == list(range(nslab - K, nslab))      # exactly the last K slabs in dispatch order
            assert int(keep.sum()) == K * 8 * par * cpr
            if rev:                                                       # ... which are the first K slabs of the map: where the next forward launch starts
                assert sorted(np.unique(slab_of(vb[keep == 1], both, cpr, LT))) == list(range(0, K))
        vb, q, keep = block(b, both, cpr, nslab, rev, -1)
        assert np.all(keep == -1)                                         # off: the launch's own policy everywhere


def slabs_of_mb(mb, V, nslab):
    """cg_setup: MB of launch traffic -> slabs (864 B per site and launch), clamped to [0, nslab]; -1 stays off"""
    if mb < 0:
        return -1
    return min((mb << 20) // (864 * (V // nslab)), nslab)


def test_megabytes_to_slabs():
    V, nslab = 32 * 32 * 32 * 64, 128
    assert 864 * (V // nslab) == 14155776                                 # the 14 MB of traffic per slab at 32^3 x 64
    assert [slabs_of_mb(mb, V, nslab) for mb in (-1, 0, 13, 14, 64, 128, 256, 512, 2048)] == [-1, 0, 0, 1, 4, 9, 18, 37, 128]
    assert [slabs_of_mb(mb, 16 * 8 * 8 * 4, 4) for mb in (0, 1, 3, 4, 100)] == [0, 1, 3, 4, 4]
    assert [slabs_of_mb(mb, 16 * 16 * 16 * 8, 8) for mb in (0, 4, 24, 27, 100)] == [0, 1, 7, 8, 8]
