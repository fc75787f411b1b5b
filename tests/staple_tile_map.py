"""The addressing of the tile form of the staple sweep (csrc/staple.hip gauge_force_kernel_tile, staple_plane_tile, staple_tile_ok) restated in numpy: which lattices take
the form, the coordinates of the 64 lanes of a chunk, and the lane of the other parity's LDS copy a lane reads for the links at n + x and n - x.  No GPU, no library:
tests/test_cpu_staple_tile_map.py checks the restatement by plain coordinate arithmetic, tests/test_gpu_staple_tile.py takes its shape table's verdicts from here."""
import numpy as np

LANE = np.arange(64)

# the lattices of tests/test_gpu_staple_tile.py by half-width XH of an x-row: 512 to 1536 sites per parity; z and t extents differ (but for (16,16,4,2),
# which has two chunks per plane instead) and are never both 2, where forward and backward neighbours coincide.  (16,16,4,2) is the one whose t-slice is a
# multiple of 8 chunks: the only one on which md_remap = 1 takes the per-XCD tile map of block_map (xcd_tile_map below) and not its plain interleave
ACCEPTED = {1: [(2, 64, 2, 4)], 2: [(4, 32, 2, 4)], 4: [(8, 16, 4, 6)], 8: [(16, 8, 6, 4), (16, 16, 4, 2)], 16: [(32, 4, 4, 6), (32, 8, 2, 4)], 32: [(64, 2, 4, 6)],
            64: [(128, 2, 2, 4)]}
# ... and the ones the form must refuse: XH = 6 does not divide 64; the rows of a plane do not fill chunks; Vh = 96
REFUSED = [(12, 4, 4, 4), (8, 4, 6, 4), (4, 4, 6, 2)]


def geom(L):
    """XH, sites per parity, chunks per parity"""
    XH = L[0] // 2
    Vh = XH * L[1] * L[2] * L[3]
    return XH, Vh, (Vh + 63) // 64


def tile_ok(L, staple_tile=1, partitioned=False):
    """staple_tile_ok: a chunk of 64 checkerboard sites is 64 / XH whole x-rows of one (z, t) plane -- XH divides 64, the rows of a plane divide into chunks,
    every chunk is full"""
    XH, Vh, _ = geom(L)
    return bool(staple_tile) and 1 <= XH <= 64 and 64 % XH == 0 and L[1] % (64 // XH) == 0 and Vh % 64 == 0 and not partitioned


def xcd_tile_map(L):
    """make_block_map of lqcd_internal.h: the per-XCD tile map (remap == 2) needs cps > 0 -- a t-slice of whole chunks whose number is a multiple of the sub-domain
    count, which the map lowers in steps of 8 down to 8; every other lattice takes the plain interleave of the blocks over the 8 XCDs"""
    slice_sites = (L[0] // 2) * L[1] * L[2]
    return slice_sites % 64 == 0 and (slice_sites // 64) % 8 == 0


def cb_to_coords(L, parity, cb):
    """cb_to_coords of lqcd_internal.h: cb = xh + XH (y + LY (z + LZ t)), x = 2 xh + ((y + z + t + parity) & 1); returns (x, y, z, t)"""
    XH = L[0] // 2
    cb = np.asarray(cb)
    q0 = cb // XH
    xh = cb - q0 * XH
    q1 = q0 // L[1]
    y = q0 - q1 * L[1]
    q2 = q1 // L[2]
    z = q1 - q2 * L[2]
    t = q2
    return 2 * xh + ((y + z + t + parity) & 1), y, z, t


def coords_to_cb(L, x, y, z, t):
    return (x >> 1) + (L[0] // 2) * (y + L[1] * (z + L[2] * t))


def tile_lane_px(lane, xh, q, XH):
    """lane of n + x inside the chunk of the other parity (staple.hip tile_lane_px)"""
    return np.where(q != 0, np.where(xh + 1 == XH, lane - (XH - 1), lane + 1), lane)


def tile_lane_mx(lane, xh, q, XH):
    """lane of n - x inside the chunk of the other parity (staple.hip tile_lane_mx)"""
    return np.where(q != 0, lane, np.where(xh == 0, lane + XH - 1, lane - 1))


def chunk_lanes(L, parity, chunk):
    """What the 64 lanes of workgroup (chunk, parity) compute in staple_links / staple_plane_tile: the coordinates c of site i = 64 chunk + lane, the row yr and the
    place xh of the lane inside the chunk, q = c[0] & 1, and the lanes l_px, l_mx of the other parity's copy (masked to 0..63 as in the kernel)."""
    XH = L[0] // 2
    i = chunk * 64 + LANE
    c = cb_to_coords(L, parity, i)
    yr = LANE // XH
    xh = LANE - yr * XH
    q = c[0] & 1
    return dict(i=i, c=c, yr=yr, xh=xh, q=q, l_px=tile_lane_px(LANE, xh, q, XH) & 63, l_mx=tile_lane_mx(LANE, xh, q, XH) & 63)
