"""The lane map behind the y-share of the scalar-addressing Wilson kernel (stencil.hip sdir_wave, PipeArgs::yshare): pipe_map's and pipe_site<1>'s index arithmetic restated
in numpy for XH = 16.  A chunk of 64 sites is four y-rows of 16 lanes, so the forward y-neighbour of rows 0-2 is (same chunk, lane + 16) and the backward one of rows 1-3 is
(same chunk, lane - 16) of the opposite-parity block -- the chunk the x wave loads whole for the x-share.  Only row 3 forwards and row 0 backwards leave the chunk, for row 0 /
row 3 of the neighbouring chunk in y; at L1 = 4 that is the lane's own chunk."""
import numpy as np
import pytest

XH = 16
LANE = np.arange(64)
ROW = LANE >> 4


def pipe_map(b, both, pmode, per_pass, cpr, ysplit, ty, tz, cpp):
    """virtual block -> (parity, t, z, chunk inside the z-plane): pipe_map of stencil.hip"""
    xcd, j = b & 7, b >> 3
    p = (j & 1) if both else pmode
    j = (j >> 1) if both else j
    pas = j // per_pass
    j -= pas * per_pass
    t = j // cpr
    m, sd = j - t * cpr, xcd + 8 * pas
    sz = sd // ysplit
    sy = sd - sz * ysplit
    zz = m // ty
    yy = m - zz * ty
    s = (sz * tz + zz) * cpp + sy * ty + yy if ysplit > 1 else sd * cpr + m
    z = s // cpp
    return p, t, z, s - z * cpp


def pipe_site_y(L1, chunk, yc):
    """(nf, nb, wf, wb) of pipe_site<1> for the 64 lanes of a chunk: site indices inside the opposite parity block"""
    cbp = yc * 64 + LANE
    y = cbp // XH
    i = chunk * 64 + LANE
    wf, wb = y == L1 - 1, y == 0
    nf = np.where(wf, i - (L1 - 1) * XH, i + XH)
    nb = np.where(wb, i + (L1 - 1) * XH, i - XH)
    return nf, nb, wf, wb, y


def geometry(L1, xcd_ysplit, L2=8, LT=2):
    """the tile map of an unpartitioned 32 x L1 x L2 x LT lattice, both parities in one launch, as make_kargs of stencil.hip sets it up for xcd_nsub = 8 xcd_ysplit: the requested
    split, or the largest smaller one the geometry admits (an odd number of chunks per z-plane cannot be split in y)"""
    cpp = XH * L1 // 64                     # chunks per z-plane
    slice_chunks = cpp * L2
    nsub = 8 * xcd_ysplit
    while nsub > 8 and slice_chunks % nsub != 0:
        nsub -= 8
    assert slice_chunks % nsub == 0
    ysplit = 1
    for ys in range(xcd_ysplit, 1, -1):
        if cpp % ys == 0 and nsub % ys == 0 and L2 % (nsub // ys) == 0:
            ysplit = ys
            break
    cpr = slice_chunks // nsub              # chunks of a sub-domain per time slice
    ty = cpp // ysplit if ysplit > 1 else 1
    tz = cpr // ty
    return dict(cpp=cpp, L2=L2, LT=LT, ty=ty, tz=tz, cpr=cpr, per_pass=cpr * LT, nblocks=2 * slice_chunks * LT, cps=slice_chunks, ysplit=ysplit)


@pytest.mark.parametrize("xcd_ysplit", [1, 2])
@pytest.mark.parametrize("L1", [4, 8, 12])
def test_y_neighbours_are_rows_of_the_own_chunk_but_for_the_two_edges(L1, xcd_ysplit):
    g = geometry(L1, xcd_ysplit)
    assert g["ysplit"] == (2 if (xcd_ysplit == 2 and L1 == 8) else 1)
    cpp, cps = g["cpp"], g["cps"]
    seen, zt_par = set(), set()
    for b in range(g["nblocks"]):
        p, t, z, yc = pipe_map(b, True, 0, g["per_pass"], g["cpr"], g["ysplit"], g["ty"], g["tz"], cpp)
        assert 0 <= t < g["LT"] and 0 <= z < g["L2"] and 0 <= yc < cpp
        chunk = t * cps + z * cpp + yc
        seen.add((p, chunk))
        zt_par.add((p, (z + t) & 1))
        nf, nb, wf, wb, y = pipe_site_y(L1, chunk, yc)
        assert np.array_equal(y, 4 * yc + ROW)                         # a chunk is four whole y-rows
        # rows 0-2 forwards, rows 1-3 backwards: the same chunk, one row of 16 lanes up / down
        fin, bin_ = ROW < 3, ROW > 0
        assert np.array_equal((nf >> 6)[fin], np.full(48, chunk)) and np.array_equal((nf & 63)[fin], LANE[fin] + 16)
        assert np.array_equal((nb >> 6)[bin_], np.full(48, chunk)) and np.array_equal((nb & 63)[bin_], LANE[bin_] - 16)
        assert not wf[fin].any() and not wb[bin_].any()                # no boundary sign on an in-chunk operand
        # row 3 forwards / row 0 backwards: row 0 / row 3 of the neighbouring chunk in y, the wrap inside the z-plane
        cf = t * cps + z * cpp + (yc + 1) % cpp
        cb = t * cps + z * cpp + (yc - 1) % cpp
        assert np.array_equal((nf >> 6)[~fin], np.full(16, cf)) and np.array_equal((nf & 63)[~fin], LANE[~fin] - 48)
        assert np.array_equal((nb >> 6)[~bin_], np.full(16, cb)) and np.array_equal((nb & 63)[~bin_], LANE[~bin_] + 48)
        assert np.array_equal(wf[~fin], np.full(16, yc == cpp - 1)) and np.array_equal(wb[~bin_], np.full(16, yc == 0))
        if cpp > 1:
            assert cf != chunk and cb != chunk                         # only these leave the chunk ...
        else:
            assert cf == chunk and cb == chunk and wf[~fin].all() and wb[~bin_].all()      # ... and at L1 = 4 they wrap into it
    assert len(seen) == g["nblocks"]                                   # the map is a bijection onto (parity, chunk)
    assert zt_par == {(0, 0), (0, 1), (1, 0), (1, 1)}                  # both parities, both (z + t) parities


def test_the_rule_needs_rows_of_16_and_whole_chunks():
    # XH = 8: a chunk holds 8 rows and the neighbour is lane +- 8 -- the host gate declines every XH but 16
    i = LANE
    assert not np.array_equal((i + 8)[ROW < 3], LANE[ROW < 3] + 16)
    # L1 = 6 (XH = 16): 96 sites per plane, a chunk straddles two z-planes and y = cbp // 16 wraps in the middle of one -- the gate asks for L1 % 4 == 0
    assert (XH * 6) % 64 != 0
