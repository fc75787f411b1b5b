"""The lane map behind the x-share of the scalar-addressing Wilson kernel (stencil.hip sdir_wave, PipeArgs::xshare): pipe_site<0>'s index arithmetic restated in numpy for
XH = 16.  With q = (y + z + t + p) & 1 both x-neighbours of lane i lie in the opposite-parity chunk with the lane's own chunk index, at lane i or i + 1 (forward) and
i - 1 or i (backward), the wrap inside the lane's row of 16 -- which is what lets the x wave load that chunk once and shift lanes."""
import numpy as np
import pytest

XH = 16
SPC = 12 * 64 * 16      # bytes of a spinor chunk (fp64: 12 components x 64 lanes x 16 B)
LANE = np.arange(64)


def pipe_site_x(chunk, yc, z, t, p):
    """(nf, nb, wf, wb, q, xh) of pipe_site<0> for the 64 lanes of a chunk: site indices inside the opposite parity block"""
    cbp = yc * 64 + LANE
    y = cbp // XH
    xh = cbp - y * XH
    i = chunk * 64 + LANE
    q = (y + z + t + p) & 1
    wf = (q == 1) & (xh == XH - 1)
    wb = (q == 0) & (xh == 0)
    nf = np.where(q == 1, np.where(wf, i - (XH - 1), i + 1), i)
    nb = np.where(q == 1, i, np.where(wb, i + (XH - 1), i - 1))
    return nf, nb, wf, wb, q, xh


def rotate_rule(q):
    row, xh = LANE >> 4, LANE & 15
    src_f = np.where(q == 1, row * 16 + ((xh + 1) & 15), LANE)
    src_b = np.where(q == 1, LANE, row * 16 + ((xh - 1) & 15))
    return src_f, src_b


@pytest.mark.parametrize("L1", [4, 8, 16, 32])
@pytest.mark.parametrize("p", [0, 1])
@pytest.mark.parametrize("zt", [0, 1])
def test_x_neighbours_are_lane_shifts_inside_the_own_chunk(L1, p, zt):
    cpp = XH * L1 // 64          # chunks per z-plane
    L2 = 4
    cps = cpp * L2
    for t in (0, 3):
        for z in (zt, zt + 2):   # (y + z + t) takes both parities over the four rows of a chunk; z + t both parities over the loop
            for yc in range(cpp):
                chunk = t * cps + z * cpp + yc
                nf, nb, wf, wb, q, xh = pipe_site_x(chunk, yc, z, t, p)
                assert set(q[::16].tolist()) == {0, 1}       # the rows of a chunk alternate
                assert np.array_equal(nf >> 6, np.full(64, chunk)) and np.array_equal(nb >> 6, np.full(64, chunk))
                src_f, src_b = rotate_rule(q)
                assert np.array_equal(nf & 63, src_f) and np.array_equal(nb & 63, src_b)
                assert np.array_equal(src_f >> 4, LANE >> 4) and np.array_equal(src_b >> 4, LANE >> 4)      # the wrap stays inside the row of 16
                assert np.array_equal(wf, (q == 1) & (xh == 15)) and np.array_equal(wb, (q == 0) & (xh == 0))
                assert np.array_equal(np.flatnonzero(src_f < LANE), np.flatnonzero(wf))      # the lanes that wrap are exactly those
                assert np.array_equal(np.flatnonzero(src_b > LANE), np.flatnonzero(wb))
                # what the kernel does: the source lane is read back from the byte offset of the neighbour (chunk * SPC + lane * 16)
                off_f, off_b = (nf >> 6) * SPC + (nf & 63) * 16, (nb >> 6) * SPC + (nb & 63) * 16
                assert np.array_equal((off_f >> 4) & 63, src_f) and np.array_equal((off_b >> 4) & 63, src_b)


def test_the_rule_needs_a_row_of_16():
    # XH = 8: a chunk holds 8 rows and the rule above (rows of 16) names other lanes -- the host gate declines every XH but 16
    cbp = LANE
    y, xh = cbp // 8, cbp % 8
    q = y & 1
    nf = np.where(q == 1, np.where(xh == 7, LANE - 7, LANE + 1), LANE)
    src_f, _ = rotate_rule(q)
    assert not np.array_equal(nf & 63, src_f)
