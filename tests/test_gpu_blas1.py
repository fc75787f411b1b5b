"""BLAS-1 on fermion fields (csrc/blas.hip dot_kernel, norm2_kernel, axpy_kernel, axpby_kernel, scale_kernel and the final reduction behind the first two) through
the public entry points lqcd_dot, lqcd_norm2, lqcd_axpy, lqcd_axpby, lqcd_scale, on data for which fp64 arithmetic is exact: real and imaginary parts are non-zero
integers in [-15, 15], scalars are dyadic.  Every partial and every total is then an exact integer whatever the summation order, every assertion is ==, and an
element that is dropped, doubled or visited twice changes a norm by at least 1 (assert_exact keeps the bound: sites * 2 * 225 < 2^53, in fact < 2^29 here).

What a kernel sees is the DEVICE length n of a field in complex numbers, padding included: ncomp * Vs * (2 for FULL, 1 for a half lattice) * L5 with the component
stride Vs = 64 * ceil(Vh / 64) + 64 * LQCD_PAD_CHUNKS (csrc/capi.hip geom_from_L, default one chunk of padding; the library exposes neither, so Case.n below
restates them).  The padding holds zeros and takes part in every kernel.  The streaming block is RB = 256 and a launch has nb = min(ceil(n / 256), 8 * CUs)
workgroups (stream_grid), so the regimes are chosen by n:
  n < 256                  staggered EVEN / ODD on (6,2,2,2) without padding chunks: 192 (with the default padding no field is shorter than 384)
  ragged last block        the same FULL: 384; staggered EVEN / ODD on (6,2,2,2): 384; staggered FULL on (6,6,2,2): 1152 = 4.5 blocks
  whole blocks             staggered FULL (6,2,2,2) 768, Wilson FULL (6,2,2,2) 3072, staggered FULL (6,6,4,2) 1536, Wilson ODD (6,6,4,2) 3072
  5D on 4^4                n = 4608 * L5, 18 * L5 blocks: L5 = 2, 3 | 4, 5, 6 cross 64 blocks (one lane-loop pass of the final reduction), 56 | 57 is the last small
                           (1008) and the first large reduction (1026: only classes 0 and 1 hold two partials), 85, 86, floor(8 CUs 256 / 4608) (113 on 256 CUs, 2034
                           blocks) are large and uncapped, ceil((8 CUs 256 + 1) / 4608) (114: 2052 blocks capped to 2048, the second grid-stride pass covers four) and
                           170 are capped.
  5D on 4^4, no padding    n = 3072 * L5 = the number of complex numbers that carry data, the last device element included; 12 * L5 blocks: L5 = 2, 5, 6 cross 64 blocks,
                           85 is the last small reduction (1020), 86 the first large one (1032: only classes 0-7 hold two partials), 170 (2040) is still uncapped on
                           256 CUs, ceil((8 CUs 256 + 1) / 3072) (171) is the first capped one.  Further unpadded fields: Wilson FULL (6,2,2,2) 1536, staggered FULL
                           (6,6,4,2) 1152 (ragged), Wilson ODD (6,6,4,2) 2304, staggered EVEN (4,4,4,4) 384 (ragged), Wilson FULL (4,4,4,4) 3072.

The accuracy test (not exact): depth = 2 fmas per grid-stride trip + 6 shuffles + 4 wave sums + the final stage's depth for nb (tests/reduce_numpy.py depth), on a
256-CU device: L5 = 5, nb = 90: 2 + 6 + 4 + 7 = 19; L5 = 113, nb = 2034: 2 + 6 + 4 + 22 = 34; L5 = 114, nb = 2048, two trips: 4 + 6 + 4 + 22 = 36."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import reduce_numpy as rn

pytestmark = pytest.mark.gpu

RB = 256
SCALARS = (0.5 - 1.25j, -2 + 0.75j, 1j)
MARK = 99.0 + 0j          # what a download must leave at the sites of the other parity


@pytest.fixture(scope="module")
def gpu(lq):
    assert lq.lib.device_count() > 0, "no HIP device visible: the product has no CPU fallback"
    return lq


@pytest.fixture(scope="module")
def cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


_lattices = {}


def lattice(lq, L, pad=1, fresh=False):
    key = (tuple(L), pad)
    if fresh or key not in _lattices:
        old = os.environ.get("LQCD_PAD_CHUNKS")
        os.environ["LQCD_PAD_CHUNKS"] = str(pad)
        try:
            lat = lq.Lattice(L)
        finally:
            if old is None:
                del os.environ["LQCD_PAD_CHUNKS"]
            else:
                os.environ["LQCD_PAD_CHUNKS"] = old
        if fresh:
            return lat
        _lattices[key] = lat
    return _lattices[key]


class Case:
    def __init__(self, name, L, kind, subset="FULL", L5=None, pad=1):
        self.name, self.L, self.kind, self.subset, self.L5, self.pad = name, tuple(L), kind, subset, L5, pad

    def __repr__(self):
        return self.name

    @property
    def sites(self):
        return int(np.prod(self.L)) // (1 if self.subset == "FULL" else 2)

    @property
    def ncomp(self):
        return 3 if self.kind == "staggered" else 12

    @property
    def logical(self):          # complex numbers that carry data
        return self.sites * self.ncomp * (self.L5 or 1)

    @property
    def n(self):                # device_len: what the kernels stream, padding included
        Vh = int(np.prod(self.L)) // 2
        Vs = 64 * ((Vh + 63) // 64) + 64 * self.pad
        return self.ncomp * Vs * (2 if self.subset == "FULL" else 1) * (self.L5 or 1)

    def nb(self, cus):
        return min((self.n + RB - 1) // RB, 8 * cus)

    def trips(self, cus):
        return -(-self.n // (self.nb(cus) * RB))

    def new(self, lq, lat=None):
        lat = lat or lattice(lq, self.L, self.pad)
        if self.L5:
            return lq.Fermionfields(lat, lq.DOMAINWALL, L5=self.L5)
        return lq.Fermionfields(lat, lq.STAGGERED if self.kind == "staggered" else lq.WILSON, getattr(lq, self.subset))

    def shape(self, lq):
        s = lattice(lq, self.L, self.pad).fermion_shape(lq.STAGGERED if self.kind == "staggered" else lq.WILSON)
        return (self.L5,) + s if self.L5 else s

    def mask(self, lq):
        """True at the host entries that belong to the field"""
        shape = self.shape(lq)
        m = np.ones(shape, dtype=bool)
        if self.subset != "FULL":
            X, Y, Z, T = self.L
            t, z, y, x = np.meshgrid(np.arange(T), np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
            par = ((x + y + z + t) & 1) == (0 if self.subset == "EVEN" else 1)
            m = np.broadcast_to(par[..., None], shape).copy()
        return m

    def ints(self, lq, seed):
        """non-zero integers in [-15, 15] in both parts; the sites of the other parity hold NaN: they must never enter"""
        rng = np.random.default_rng(seed)
        shape = self.shape(lq)
        part = lambda: rng.integers(1, 16, size=shape) * rng.choice((-1, 1), size=shape)
        h = (part() + 1j * part()).astype(np.complex128)
        h[~self.mask(lq)] = complex(np.nan, np.nan)
        return h

    def get(self, lq, f):
        """the field's sites from the device; the sites of the other parity of the host array must come back untouched"""
        m = self.mask(lq)
        out = np.full(self.shape(lq), MARK)
        f.download(into=out)
        assert (out[~m] == MARK).all()
        return out[m]


def assert_exact(case):
    """every partial, every total and every intermediate of the checks below is an integer (or a multiple of 2^-8) below 2^53: fp64 computes it exactly"""
    worst = case.logical * 2 * 15 * 15
    assert worst < 2 ** 29 < 2 ** 53, (case, worst)
    return worst


def ref_dot(a, b):
    """sum conj(a) b in Python integers"""
    ar, ai, br, bi = (np.rint(v).astype(np.int64) for v in (a.real, a.imag, b.real, b.imag))
    assert (ar == a.real).all() and (bi == b.imag).all()
    return int((ar * br + ai * bi).sum()), int((ar * bi - ai * br).sum())


def dot(lq, a, b):
    re, im = C.c_double(4711.0), C.c_double(4711.0)
    lq.lib.check(lq.lib.lib().lqcd_dot(a._h, b._h, C.byref(re), C.byref(im)))
    return re.value, im.value


def norm2(lq, a):
    n2 = C.c_double(4711.0)
    lq.lib.check(lq.lib.lib().lqcd_norm2(a._h, C.byref(n2)))
    return n2.value


def axpy(lq, a, x, y):
    return lq.lib.lib().lqcd_axpy(C.c_double(a.real), C.c_double(a.imag), x._h, y._h)


def axpby(lq, a, x, b, y):
    return lq.lib.lib().lqcd_axpby(C.c_double(a.real), C.c_double(a.imag), x._h, C.c_double(b.real), C.c_double(b.imag), y._h)


def scale(lq, a, x):
    return lq.lib.lib().lqcd_scale(C.c_double(a.real), C.c_double(a.imag), x._h)


SMALL = [
    Case("stag-full-6222", (6, 2, 2, 2), "staggered"),
    Case("stag-even-6222", (6, 2, 2, 2), "staggered", "EVEN"),
    Case("stag-odd-6222", (6, 2, 2, 2), "staggered", "ODD"),
    Case("stag-full-6222-nopad", (6, 2, 2, 2), "staggered", pad=0),
    Case("stag-even-6222-nopad", (6, 2, 2, 2), "staggered", "EVEN", pad=0),
    Case("stag-odd-6222-nopad", (6, 2, 2, 2), "staggered", "ODD", pad=0),
    Case("wilson-full-6222", (6, 2, 2, 2), "wilson"),
    Case("stag-full-6642", (6, 6, 4, 2), "staggered"),
    Case("wilson-odd-6642", (6, 6, 4, 2), "wilson", "ODD"),
    Case("stag-full-6622", (6, 6, 2, 2), "staggered"),
    Case("wilson-full-6222-nopad", (6, 2, 2, 2), "wilson", pad=0),
    Case("stag-full-6642-nopad", (6, 6, 4, 2), "staggered", pad=0),
    Case("wilson-odd-6642-nopad", (6, 6, 4, 2), "wilson", "ODD", pad=0),
    Case("stag-even-4444-nopad", (4, 4, 4, 4), "staggered", "EVEN", pad=0),
    Case("wilson-full-4444-nopad", (4, 4, 4, 4), "wilson", pad=0),
]
SLICE = {1: 4608, 0: 3072}      # device length of one 4^4 Wilson slice, with and without the padding chunk


def five_d(L5, pad=1):
    return Case("dw-4444-L5=%d%s" % (L5, "" if pad else "-nopad"), (4, 4, 4, 4), "wilson", L5=L5, pad=pad)


# the 5D lengths depend on the device's CU count, which collection does not know: the fixed ones are parameters, the two computed ones resolve at run time
L5_PARAMS = [(k, 1) for k in (2, 3, 4, 5, 6, 56, 57, 85, 86, 170, "last-uncapped", "first-capped")] + [(k, 0) for k in (2, 5, 6, 85, 86, 170, "first-capped")]


def resolve(L5, cus, pad=1):
    cap = 8 * cus * RB
    return {"last-uncapped": cap // SLICE[pad], "first-capped": -(-(cap + 1) // SLICE[pad])}.get(L5, L5)


ALL = [pytest.param(c, id=c.name) for c in SMALL] + [pytest.param(k, id="dw-4444-L5=%s%s" % (k[0], "" if k[1] else "-nopad")) for k in L5_PARAMS]


def the_case(c, cus):
    return c if isinstance(c, Case) else five_d(resolve(c[0], cus, c[1]), c[1])


def test_the_cases_cover_the_regimes(cus):
    n = {c.name: c.n for c in SMALL}
    assert n["stag-even-6222-nopad"] == 192 and n["stag-odd-6222-nopad"] == 192 and n["stag-full-6222-nopad"] == 384                 # n < 256, and 1.5 blocks
    assert n["stag-even-6222"] == 384 and n["stag-full-6622"] == 1152 and n["stag-full-6222"] == 768 and n["wilson-full-6222"] == 3072
    assert n["stag-full-6642"] == 1536 and n["wilson-odd-6642"] == 3072
    assert n["wilson-full-6222-nopad"] == 1536 and n["stag-full-6642-nopad"] == 1152 and n["wilson-odd-6642-nopad"] == 2304
    assert n["stag-even-4444-nopad"] == 384 and n["wilson-full-4444-nopad"] == 3072          # no padding behind the last site: the last device element carries data
    assert sum(1 for c in SMALL if c.n % RB) >= 5 and sum(1 for c in SMALL if c.n < RB) == 2
    # without the padding chunk a 4^4 slice is 3072 long, 12 blocks: L5 = 85 is the last small reduction (1020), 86 the first large one (1032: classes 0-7 hold two
    # partials), 170 (2040) is uncapped on 256 CUs
    nopad = [the_case(k, cus) for k in L5_PARAMS if k[1] == 0]
    assert all(c.n == 3072 * c.L5 == c.logical for c in nopad)
    assert five_d(85, 0).nb(cus) == 1020 and five_d(86, 0).nb(cus) == 1032
    if cus == 256:
        assert five_d(170, 0).nb(cus) == 2040 and five_d(170, 0).trips(cus) == 1 and nopad[-1].L5 == 171 and nopad[-1].trips(cus) == 2
    assert any(1024 < c.nb(cus) and c.trips(cus) == 1 for c in nopad) and any(c.nb(cus) == 8 * cus and c.trips(cus) == 2 for c in nopad)
    cases = [the_case(k, cus) for k in L5_PARAMS if k[1] == 1]
    assert all(c.n == 4608 * c.L5 for c in cases)
    nbs = [c.nb(cus) for c in cases]
    assert any(b < 64 for b in nbs) and any(64 < b <= 1024 for b in nbs)
    assert five_d(56).nb(cus) == 1008 and five_d(57).nb(cus) == 1026          # the last small and the first large final reduction (cus >= 129)
    uncapped_large = [c for c in cases if 1024 < c.nb(cus) < 8 * cus and c.trips(cus) == 1]
    capped = [c for c in cases if c.nb(cus) == 8 * cus and c.trips(cus) == 2]
    assert uncapped_large and capped, (cus, nbs)
    first = five_d(resolve("first-capped", cus))
    assert first.n - 8 * cus * RB <= SLICE[1] and first.trips(cus) == 2      # its second grid-stride pass covers a few blocks only
    for c in SMALL + cases + nopad:
        assert_exact(c)


@pytest.mark.parametrize("c", ALL)
def test_dot_and_norm2_are_exact(gpu, cus, c):
    lq, case = gpu, the_case(c, cus)
    assert_exact(case)
    m = case.mask(lq)
    ah, bh = case.ints(lq, 11), case.ints(lq, 12)
    a, b = case.new(lq).upload(ah), case.new(lq).upload(bh)
    re, im = ref_dot(ah[m], bh[m])
    assert dot(lq, a, b) == (float(re), float(im))
    assert dot(lq, b, a) == (float(re), float(-im))
    aa = ref_dot(ah[m], ah[m])
    assert aa[1] == 0 and aa[0] >= 2 * case.logical
    d = dot(lq, a, a)
    assert d[1] == 0.0 and d[0] == float(aa[0]) and norm2(lq, a) == d[0]
    assert norm2(lq, b) == float(ref_dot(bh[m], bh[m])[0])
    assert dot(lq, a, b) == (float(re), float(im))           # the same bits again
    assert np.array_equal(case.get(lq, a), ah[m]) and np.array_equal(case.get(lq, b), bh[m])      # operands untouched


@pytest.mark.parametrize("c", ALL)
def test_axpy_axpby_scale_match_numpy_also_in_place(gpu, cus, c):
    lq, case = gpu, the_case(c, cus)
    assert_exact(case)
    m = case.mask(lq)
    xh, yh = case.ints(lq, 21), case.ints(lq, 22)
    xv, yv = xh[m], yh[m]
    x, y = case.new(lq), case.new(lq)
    x.upload(xh)
    a, b, s = SCALARS
    y.upload(yh)
    lq.lib.check(axpy(lq, a, x, y))
    assert np.array_equal(case.get(lq, y), yv + a * xv)
    y.upload(yh)
    lq.lib.check(axpby(lq, a, x, b, y))
    assert np.array_equal(case.get(lq, y), a * xv + b * yv)
    y.upload(yh)
    lq.lib.check(axpby(lq, s, x, a, y))
    assert np.array_equal(case.get(lq, y), s * xv + a * yv)
    y.upload(yh)
    for k in SCALARS:
        lq.lib.check(scale(lq, k, y))
        yv = k * yv
        assert np.array_equal(case.get(lq, y), yv)
    assert np.array_equal(case.get(lq, x), xv)
    # x and y the same field: same_shape admits it
    lq.lib.check(axpy(lq, a, x, x))
    assert np.array_equal(case.get(lq, x), (1 + a) * xv)
    x.upload(xh)
    lq.lib.check(axpby(lq, a, x, b, x))
    assert np.array_equal(case.get(lq, x), (a + b) * xv)
    # the norm of a result: every element was written once (the products are multiples of 1/16: still exact)
    want = (a + b) * xv
    assert norm2(lq, x) == float(np.sum(want.real ** 2 + want.imag ** 2))


@pytest.mark.parametrize("L,kind", [((6, 2, 2, 2), "staggered"), ((6, 6, 4, 2), "wilson"), ((6, 6, 2, 2), "staggered")])
def test_halves_of_a_full_field(gpu, L, kind):
    lq = gpu
    full, even, odd = Case("full", L, kind), Case("even", L, kind, "EVEN"), Case("odd", L, kind, "ODD")
    fh = full.ints(lq, 31)
    f, e, o = full.new(lq).upload(fh), even.new(lq), odd.new(lq)
    lq.extract_fermion_(e, f)
    lq.extract_fermion_(o, f)
    me, mo = even.mask(lq), odd.mask(lq)
    assert np.array_equal(even.get(lq, e), fh[me]) and np.array_equal(odd.get(lq, o), fh[mo])
    ne, no, nf = norm2(lq, e), norm2(lq, o), norm2(lq, f)
    assert ne == float(ref_dot(fh[me], fh[me])[0]) and no == float(ref_dot(fh[mo], fh[mo])[0])
    assert ne + no == nf == float(ref_dot(fh, fh)[0])
    # an upload of a FULL host array into a half field takes its own parity only (the other one holds NaN in ints())
    e2 = even.new(lq).upload(np.where(me, fh, complex(np.nan, np.nan)))
    assert norm2(lq, e2) == ne and dot(lq, e, e2) == (ne, 0.0)


@pytest.mark.parametrize("L5", [2, 6, "first-capped"])
def test_slices_of_a_5d_field(gpu, cus, L5):
    lq, case = gpu, five_d(resolve(L5, cus))
    L5 = case.L5
    xh, yh = case.ints(lq, 41), case.ints(lq, 42)
    x, y = case.new(lq).upload(xh), case.new(lq).upload(yh)
    xs, ys = x.w, y.w
    per_slice = [norm2(lq, v) for v in xs]
    assert per_slice == [float(ref_dot(xh[s], xh[s])[0]) for s in range(L5)]
    assert math.fsum(per_slice) == norm2(lq, x)
    for i, j in ((0, 0), (0, L5 - 1), (L5 - 1, 1), (L5 // 2, L5 // 2)):
        re, im = ref_dot(xh[i], yh[j])
        assert dot(lq, xs[i], ys[j]) == (float(re), float(im))
    a = SCALARS[0]
    k = L5 // 2
    lq.lib.check(axpy(lq, a, xs[0], ys[k]))                # into one slice: the others keep their bits
    want = yh.copy()
    want[k] = yh[k] + a * xh[0]
    assert np.array_equal(y.download(), want)
    lq.lib.check(axpy(lq, a, x, y))                        # on the parent: a view sees the new values
    want = want + a * xh
    for s in (0, k, L5 - 1):
        assert np.array_equal(ys[s].download(), want[s])
        assert np.array_equal(y.w[s].download(), want[s])
    assert np.array_equal(x.download(), xh)


def test_refusals_leave_the_output_untouched(gpu):
    lq = gpu
    L = (6, 2, 2, 2)
    lat, other = lattice(lq, L), lattice(lq, L, fresh=True)
    ws, st, ev, od = Case("w", L, "wilson"), Case("s", L, "staggered"), Case("e", L, "staggered", "EVEN"), Case("o", L, "staggered", "ODD")
    dw2, dw3 = Case("dw2", L, "wilson", L5=2), Case("dw3", L, "wilson", L5=3)
    sh = st.ints(lq, 51)
    y = st.new(lq).upload(sh)
    p2h = dw2.ints(lq, 52)
    p2 = dw2.new(lq).upload(p2h)
    elsewhere = st.new(lq, other)
    pairs = [(ws.new(lq), y), (ev.new(lq), y), (elsewhere, y), (ev.new(lq), od.new(lq)),       # kind, subset, context, subset
             (dw3.new(lq), p2), (p2.w[0], p2), (ws.new(lq), p2)]                                      # L5, a slice against its parent, a Wilson field against a 5D one
    for x, yy in pairs:
        for u, v in ((x, yy), (yy, x)):
            re, im = C.c_double(4711.0), C.c_double(4711.0)
            assert lq.lib.lib().lqcd_dot(u._h, v._h, C.byref(re), C.byref(im)) == lq.lib.ERR_ARG
            assert (re.value, im.value) == (4711.0, 4711.0)
            assert axpy(lq, 1j, u, v) == lq.lib.ERR_ARG and axpby(lq, 1j, u, 0.5 + 0j, v) == lq.lib.ERR_ARG
    assert np.array_equal(y.download(), sh) and np.array_equal(p2.download(), p2h)
    assert lq.lib.lib().lqcd_scale(C.c_double(2.0), C.c_double(0.0), None) == lq.lib.ERR_ARG
    n2 = C.c_double(4711.0)
    assert lq.lib.lib().lqcd_norm2(None, C.byref(n2)) == lq.lib.ERR_ARG and n2.value == 4711.0
    assert norm2(lq, y) == float(ref_dot(sh, sh)[0])          # the context still works
    del pairs
    elsewhere.close()
    other.close()


@pytest.mark.parametrize("c", [pytest.param(SMALL[4], id=SMALL[4].name), pytest.param(("first-capped", 1), id="dw-4444-first-capped"),
                               pytest.param(("first-capped", 0), id="dw-4444-first-capped-nopad")])
def test_a_non_finite_element_at_either_end_is_seen(gpu, cus, c):
    lq, case = gpu, the_case(c, cus)
    assert case.n < RB or case.trips(cus) == 2
    m = case.mask(lq)
    ah, bh = case.ints(lq, 61), case.ints(lq, 62)
    first, last = tuple(0 for _ in ah.shape), tuple(k - 1 for k in ah.shape)
    assert m[first] and m[last]
    a, b = case.new(lq), case.new(lq).upload(bh)
    for where in (first, last):
        for bad in (np.nan, np.inf):
            h = ah.copy()
            h[where] = complex(bad, 3.0)
            a.upload(h)
            n2 = norm2(lq, a)
            assert math.isnan(n2) if math.isnan(bad) else n2 == np.inf, (case, where, bad, n2)
            for d in (dot(lq, a, b), dot(lq, b, a), dot(lq, a, a)):
                assert not (math.isfinite(d[0]) and math.isfinite(d[1])), (case, where, bad, d)
    a.upload(ah)
    assert norm2(lq, a) == float(ref_dot(ah[m], ah[m])[0])


@pytest.mark.parametrize("L5", [5, "last-uncapped", "first-capped"])
def test_dot_of_nearly_orthogonal_fields_within_the_derived_bound(gpu, cus, L5):
    """a, b Gaussian and rounded to float32: every product is exact in fp64 and math.fsum of the products is the true sum; b is orthogonalised against a on the host
    before the rounding, so |sum conj(a) b| < 1e-8 sum |a||b| and a relative tolerance would say nothing.  |dot - fsum| <= (depth + 2) 2^-53 sum |a_i||b_i| with the depth
    of the module docstring, counted from the code for this device's nb; derived, no margin."""
    lq, case = gpu, five_d(resolve(L5, cus))
    rng = np.random.default_rng(70 + case.L5)
    shape = case.shape(lq)
    g = lambda: rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    ah = g().astype(np.complex64).astype(np.complex128)
    bh = g()
    bh = (bh - ah * (np.vdot(ah, bh) / np.vdot(ah, ah))).astype(np.complex64).astype(np.complex128)
    ar, ai, br, bi = ah.real.ravel(), ah.imag.ravel(), bh.real.ravel(), bh.imag.ravel()
    true_re, true_im = math.fsum(np.concatenate((ar * br, ai * bi))), math.fsum(np.concatenate((ar * bi, -(ai * br))))
    weight = math.fsum(np.abs(ah.ravel()) * np.abs(bh.ravel())) * (1 + 2.0 ** -50)          # (the moduli are rounded: an upper bound all the same)
    assert math.hypot(true_re, true_im) < 1e-8 * weight
    nb, trips = case.nb(cus), case.trips(cus)
    depth = 2 * trips + 6 + 4 + rn.depth(nb)
    if cus == 256:
        assert (nb, depth) == {5: (90, 19), 113: (2034, 34), 114: (2048, 36)}[case.L5]
    a, b = case.new(lq).upload(ah), case.new(lq).upload(bh)
    re, im = dot(lq, a, b)
    err, bound = math.hypot(re - true_re, im - true_im), (depth + 2) * 2.0 ** -53 * weight
    print("L5", case.L5, "nb", nb, "trips", trips, "depth", depth, "|dot - fsum| = %.3e, bound %.3e, |fsum| = %.3e, sum|a||b| = %.3e" % (err, bound, math.hypot(true_re, true_im), weight))
    assert err <= bound, (err, bound)
