"""The cache hints and the tile map a full-size context runs under, for tests on small lattices (tests/test_cpu_fullsize_hints.py, tests/test_gpu_fullsize_hints.py).

lqcd_ctx_create rewrites four tunables from the local volume (capi.hip, "Volume-adaptive defaults"): nt_gauge = 0 while the 12-real links take at most 256 MB, nt_store = 0
while an output spinor takes at most 64 MB, xcd_nsub = 8 / xcd_ysplit = 2 while a t-slice has at most 128 chunks per parity.  Every small test lattice is below all three, a
32^3 x 64 context is above all three and keeps the initialisers of lqcd_internal.h.  FULLSIZE is that state; on(lat) puts a small context into it, off(lat) takes the two cache
hints out again (the map stays: a hint changes no value, a map changes the order of nothing that is summed across workgroups in one launch, but it is the hints that are
compared here).

resolve restates make_kargs' map resolution (stencil.hip) for 64-site chunks; adaptive restates the rule of lqcd_ctx_create."""

FULLSIZE = {"nt_gauge": 1, "nt_store": 1, "xcd_nsub": 16, "xcd_ysplit": 4}
OFF = {"nt_gauge": 0, "nt_store": 0}
ADAPTED = {"nt_gauge": 0, "nt_store": 0, "xcd_nsub": 8, "xcd_ysplit": 2}      # what every small test lattice resolves to

NTB = 16                          # nt_active bit 4: the launched instance has the streamed backward-link loads compiled in
FULL_WORD = 1 | 4                 # nt_active bits 0-3 under FULLSIZE: backward-link loads and output stores stream


def on(lat):
    for k, v in FULLSIZE.items():
        lat.set_param(k, v)


def off(lat):
    for k, v in OFF.items():
        lat.set_param(k, v)


def chunks(L):
    """(chunks of 64 sites per parity and t-slice, per z-plane); 0 where the sites are no whole chunks"""
    XH = L[0] // 2
    sl, plane = XH * L[1] * L[2], XH * L[1]
    return (sl // 64 if sl % 64 == 0 else 0), (plane // 64 if plane % 64 == 0 else 0)


def resolve(L, nsub, ysplit):
    """(nsub, ysplit, ty, tz, cpr, passes) of make_kargs for the requested xcd_nsub / xcd_ysplit: the requested number of sub-domains per t-slice or the largest smaller
    multiple of 8 that divides the chunks of a slice; the requested (y,z) split or the largest smaller one the geometry admits"""
    cps_all, cpp = chunks(L)
    nsub = nsub if (nsub >= 8 and nsub % 8 == 0) else 8
    if cps_all:
        while nsub > 8 and cps_all % nsub != 0:
            nsub -= 8
    cps = cps_all if (cps_all and cps_all % nsub == 0) else 0
    ys = 1
    for cand in range(ysplit, 1, -1):
        if cps > 0 and cpp > 0 and cpp % cand == 0 and nsub % cand == 0 and L[2] % (nsub // cand) == 0:
            ys = cand
            break
    cpr = cps // nsub if cps > 0 else 1
    ty = cpp // ys if ys > 1 else 1
    tz = cpr // ty
    return nsub, ys, ty, tz, cpr, nsub // 8


def adaptive(L):
    """the four tunables of a fresh context of local volume L (lqcd_ctx_create)"""
    out = dict(FULLSIZE)
    V = L[0] * L[1] * L[2] * L[3]
    Vh = V // 2
    nch = -(-Vh // 64)
    XH = L[0] // 2
    sl = XH * L[1] * L[2]
    if sl % 64 == 0 and sl // 64 <= 128:
        out["xcd_nsub"], out["xcd_ysplit"] = 8, 2
    if 2 * nch * 24 * 64 * 16 <= 256 << 20:
        out["nt_gauge"] = 0
    if 24 * Vh * 16 <= 64 << 20:
        out["nt_store"] = 0
    return out
