"""The lane map of the tile form of the staple sweep (csrc/staple.hip gauge_force_kernel_tile; restated in tests/staple_tile_map.py) against plain coordinate arithmetic.
A chunk of 64 checkerboard sites is 64 / XH whole x-rows of one (z, t) plane, so with the chunk of the same index of the other parity it is a closed (x, y) tile of 128
sites: the kernel copies both to LDS and reads the links at n + x and n - x from the other parity's copy at the lane tile_lane_px / tile_lane_mx name.  For every
XH in {1, 2, 4, 8, 16, 32, 64}, both parities and every chunk of the lattices tests/test_gpu_staple_tile.py runs, that lane must be the site n +- x (periodic in x) and
lie in the chunk of the same index; at Lx = 2 the two neighbours are one site.  The last tests pin the host gate (staple_tile_ok) for the GPU test's shape table and the
restated cb_to_coords to the library's own (lqcd_coords_cb: the same inline function the kernels call)."""
import ctypes as C

import numpy as np
import pytest

import staple_tile_map as tm

SHAPES = [(XH, L) for XH, Ls in sorted(tm.ACCEPTED.items()) for L in Ls]


def _lex_site(L, x, y, z, t):
    """(parity, checkerboard index) of a site by the layout rule of lqcd_internal.h, written out on its own"""
    return (x + y + z + t) % 2, x // 2 + (L[0] // 2) * (y + L[1] * (z + L[2] * t))


@pytest.mark.parametrize("XH,L", SHAPES)
def test_x_neighbours_are_the_named_lanes_of_the_same_chunk_of_the_other_parity(XH, L):
    assert L[0] == 2 * XH and tm.tile_ok(L)
    _, Vh, nch = tm.geom(L)
    assert Vh == 64 * nch
    rows, cpp = 64 // XH, XH * L[1] // 64                      # rows per chunk, chunks per (z, t) plane
    seen, zt_par = np.zeros((2, Vh), dtype=int), set()
    for p in (0, 1):
        for chunk in range(nch):
            m = tm.chunk_lanes(L, p, chunk)
            x, y, z, t = m["c"]
            # the chunk is whole x-rows of one plane, lane = yr * XH + xh
            plane = chunk // cpp
            assert np.all(z == plane % L[2]) and np.all(t == plane // L[2])
            assert np.array_equal(y, (chunk % cpp) * rows + m["yr"]) and np.array_equal(x >> 1, m["xh"])
            assert np.array_equal(m["yr"] * XH + m["xh"], tm.LANE) and np.all((x + y + z + t) % 2 == p)
            assert np.array_equal(m["q"], x % 2) and len(set((m["q"] + y) % 2)) == 1      # q alternates from row to row
            seen[p, m["i"]] += 1
            zt_par.add((p, int(z[0] + t[0]) % 2))
            for key, step in (("l_px", 1), ("l_mx", -1)):
                pn, cbn = _lex_site(L, (x + step) % L[0], y, z, t)
                assert np.all(pn == 1 - p), key
                assert np.array_equal(cbn // 64, np.full(64, chunk)), (key, "the neighbour leaves the chunk")
                assert np.array_equal(cbn % 64, m[key]), (key, p, chunk)
            # both copies are read at every lane exactly once per hop: the maps are permutations of the chunk
            assert sorted(m["l_px"]) == list(range(64)) and sorted(m["l_mx"]) == list(range(64))
            if XH > 1:
                assert not np.array_equal(m["l_px"], m["l_mx"])
    assert np.all(seen == 1)
    assert zt_par == {(0, 0), (0, 1), (1, 0), (1, 1)}           # both parities in planes of both (z + t) parities


def test_at_lx_2_forward_and_backward_are_the_same_lane():
    (L,) = tm.ACCEPTED[1]
    for p in (0, 1):
        for chunk in range(tm.geom(L)[2]):
            m = tm.chunk_lanes(L, p, chunk)
            assert np.array_equal(m["l_px"], m["l_mx"]) and np.array_equal(m["l_px"], tm.LANE)


def test_the_wrap_is_inside_the_row():
    """x = Lx - 1 forwards and x = 0 backwards stay in the lane's own row: lane -+ (XH - 1), never XH"""
    for XH in (2, 4, 8, 16, 32, 64):
        lane = tm.LANE
        xh = lane % XH
        q1, q0 = np.ones(64, dtype=int), np.zeros(64, dtype=int)
        px, mx = tm.tile_lane_px(lane, xh, q1, XH), tm.tile_lane_mx(lane, xh, q0, XH)
        assert np.array_equal(px // XH, lane // XH) and np.array_equal(mx // XH, lane // XH)
        assert np.array_equal(px % XH, (xh + 1) % XH) and np.array_equal(mx % XH, (xh - 1) % XH)
        assert px.min() >= 0 and px.max() <= 63 and mx.min() >= 0 and mx.max() <= 63      # the kernel's & 63 never changes a value
        assert np.array_equal(tm.tile_lane_px(lane, xh, q0, XH), lane) and np.array_equal(tm.tile_lane_mx(lane, xh, q1, XH), lane)


def test_gate_verdicts_for_the_gpu_tests_shapes():
    for XH, Ls in tm.ACCEPTED.items():
        for L in Ls:
            assert L[0] == 2 * XH and tm.tile_ok(L), L
            assert not tm.tile_ok(L, staple_tile=0) and not tm.tile_ok(L, partitioned=True)
            assert 512 <= tm.geom(L)[1] <= 1536
            assert (2 * tm.geom(L)[2]) % 8 == 0          # md_remap = 1 changes the order of the workgroups on every one of them (block_map) ...
    # ... through the per-XCD tile map on one lattice, through the plain interleave on the others
    assert [L for Ls in tm.ACCEPTED.values() for L in Ls if tm.xcd_tile_map(L)] == [(16, 16, 4, 2)]
    assert tm.xcd_tile_map((32, 32, 32, 64))
    assert sorted(tm.ACCEPTED) == [1, 2, 4, 8, 16, 32, 64]
    assert tm.geom(tm.ACCEPTED[8][1])[0] * tm.ACCEPTED[8][1][1] // 64 == 2      # (16,16,4,2): two chunks per plane
    assert tm.geom(tm.ACCEPTED[64][0])[0] == 64 and 64 // 64 == 1               # (128,2,2,4): one row per chunk
    for L in tm.REFUSED:
        assert not tm.tile_ok(L), L
    XH, Vh, _ = tm.geom((12, 4, 4, 4))
    assert 64 % XH != 0 and Vh % 64 == 0                                         # refused for the row width alone
    XH, Vh, _ = tm.geom((8, 4, 6, 4))
    assert 64 % XH == 0 and Vh % 64 == 0 and 4 % (64 // XH) != 0                 # ... for the rows of a plane alone
    assert tm.geom((4, 4, 6, 2))[1] == 96
    # the benchmark's lattice and the flow test's
    assert tm.tile_ok((32, 32, 32, 64)) and tm.tile_ok((8, 16, 4, 4))
    assert not tm.tile_ok((256, 2, 2, 2))                                        # XH = 128: a row is longer than a chunk


def test_restated_coordinates_are_the_librarys(lq):
    lib = lq.lib.lib()
    out = (C.c_int * 4)()
    for L in [Ls[0] for Ls in tm.ACCEPTED.values()] + tm.REFUSED:
        Lc = (C.c_int * 4)(*L)
        Vh = tm.geom(L)[1]
        for p in (0, 1):
            cb = np.unique(np.concatenate([np.arange(0, Vh, 7), [Vh - 1]]))
            x, y, z, t = tm.cb_to_coords(L, p, cb)
            for k, i in enumerate(cb):
                assert lib.lqcd_coords_cb(Lc, p, C.c_int64(int(i)), out) == 0
                assert tuple(out) == (x[k], y[k], z[k], t[k]), (L, p, i)
            assert np.array_equal(tm.coords_to_cb(L, x, y, z, t), cb)
