"""Every stencil instance under the cache hints and the tile map of a full-size context.

lqcd_ctx_create turns nt_gauge and nt_store off and shrinks the XCD tile map on every lattice the rest of the suite uses (tests/fullsize_hints.py), so the NTB = true
half of every `if (ntb) ... else ...` pair of launch_stencil_interior, the streaming-store branches and the map 32^3 x 64 resolves to (16 sub-domains, split 4: ty 2, two
passes) are reached by the three full-size shapes of tests/test_gpu_fullsize.py alone.  Here a small context is put into that state by hand.

A cache hint changes no value.  Each row builds a context, asserts the adaptive defaults it was given, sets the full-size map, makes the call once with the two hints off and
once with them on, and asserts (i) the same bits, (ii) the oracle bound the project holds that call to, (iii) the read-only key nt_active -- bits 0-3 the hint word of the
last stencil launch, bit 4 set where the launched instance has the streamed backward-link loads compiled in -- and the form's own *_active keys, so that a row which lands in
another kernel than it names fails.  Shapes: 16.8.8.4, 32.8.8.4 (XH = 16: the x- and y-share), 16.16.16.8 (two passes), 32.32.8.4 (the smallest shape that resolves like
32^3 x 64: 512 workgroups, (nsub, ysplit, ty, tz, cpr, passes) = (16, 4, 2, 2, 4, 2)), and (8,4,6,2) / (6,6,4,2) / (8,4,6,4) for partially filled chunks.  No timing."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import f32_bound as fb
import fullsize_hints as fh
import test_gpu_tgauge8 as t8
from conftest import rel_err

pytestmark = pytest.mark.gpu

KAPPA = 0.141139
S16, W32, TWIN, MID = (16, 8, 8, 4), (32, 8, 8, 4), (32, 32, 8, 4), (16, 16, 16, 8)
CHUNKED = [S16, W32, TWIN, MID]                 # z-planes of whole chunks: the scalar-addressing kernel
PARTIAL = [(8, 4, 6, 2), (6, 6, 4, 2)]          # partially filled chunks: the direction-split and site-per-lane kernels
ANTI, YANTI = (1, 1, 1, -1), (1, -1, 1, 1)
TOL = 1e-13                                     # an operator application against the oracle
ON, ON_NTB = fh.FULL_WORD, fh.FULL_WORD | fh.NTB
IDS = lambda v: ".".join(map(str, v)) if isinstance(v, tuple) else str(v)
_memo = {}


@pytest.fixture(scope="module")
def gpu(lq):
    assert lq.lib.device_count() > 0, "no HIP device visible: the product has no CPU fallback"
    return lq


def memo(key, make):
    """host-side inputs and oracle results: made once, shared, never written"""
    if key not in _memo:
        v = make()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _memo[key] = v
    return _memo[key]


def links(orc, L, seed=611):
    return memo(("U", L, seed), lambda: orc.hot_gauge(L, seed))


def source(orc, L, seed=612):
    return memo(("b", L, seed), lambda: orc.gaussian_spinor(orc.wilson_shape(L), seed))


def context(lq, L, **tun):
    """a fresh context: the adaptive defaults it reports, then the full-size map (the hints are set per call by both())"""
    lat = lq.Lattice(L)
    got = {k: lat.get_param(k) for k in fh.FULLSIZE}
    assert got == fh.adaptive(L), (L, got)
    assert got["nt_gauge"] == 0 and got["nt_store"] == 0
    assert lat.get_param("nt_active") == -1
    for k, v in tun.items():
        lat.set_param(k, v)
    fh.on(lat)
    return lat


def both(lat, call):
    """call() with the hints off, then on, under the same map: ((result, nt_active) off, (result, nt_active) on)"""
    fh.off(lat)
    a = call()
    wa = lat.get_param("nt_active")
    fh.on(lat)
    b = call()
    return (a, wa), (b, lat.get_param("nt_active"))


def apply(lq, lat, op, x, hop_to=None):
    """y = op x (hop_to: the parity hop into a half field of that subset) into an output pre-filled with NaN"""
    def call():
        y = lq.Fermionfields(lat, lq.WILSON, hop_to) if hop_to is not None else x.similar()
        if hop_to is None:
            y.upload(np.full(lat.fermion_shape(lq.WILSON), np.nan + 1j * np.nan, dtype=np.complex128))
            lq.mul_(y, op, x)
        else:
            lq.hop_(y, op, x)
        return y.download()
    return call


def same_bits_and_oracle(pair, ref, words, what, tol=TOL):
    (off, woff), (on, won) = pair
    assert not np.isnan(on).any() and not np.isnan(off).any(), what
    assert np.array_equal(off, on), (what, "the hints changed a value", rel_err(on, off))
    err = rel_err(on, ref)
    assert err < tol, (what, err)
    assert (woff, won) == words, (what, "nt_active", (woff, won), "expected", words)


def wilson(lq, U, bc, **kw):
    p = {"Dirac_operator": "Wilson", "κ": KAPPA, "boundarycondition": bc, "eps_CG": 1e-16, "MaxCGstep": 3000}
    p.update(kw)
    return lq.Dirac_operator(U, None, p)


# ------------------------------------------------------------------ 1. Wilson applications: the scalar-addressing kernel
@pytest.mark.parametrize("recon", [12, 18])
@pytest.mark.parametrize("L", CHUNKED, ids=IDS)
def test_scalar_addressing_kernel_D_Ddag_DdagD_and_both_parity_hops(gpu, orc, L, recon):
    """wilson_dirsplit_s<D, R, NTB> plain instances, 12 and 18 reals, boundary conditions (1,1,1,-1) and (1,-1,1,1)"""
    lq = gpu
    lat = context(lq, L, gauge_recon=recon)
    assert lat.get_param("dslash_pipe") == 2 and lat.get_param("dslash_variant") == 1 and lat.get_param("dslash_s18") == 1
    assert fh.resolve(L, 16, 4)[5] == (2 if L in (TWIN, MID, W32) else 1)
    Uh, bh = links(orc, L), source(orc, L)
    U = lq.Gaugefields(lat).upload(Uh)
    x = lq.Fermionfields(lat, lq.WILSON).upload(bh)
    for bc in (ANTI, YANTI):
        D = wilson(lq, U, bc)
        refs = {dag: memo(("D", L, bc, dag), lambda: orc.wilson_D(Uh, bh, L, KAPPA, 1.0, bc, dag)) for dag in (False, True)}
        for dag in (False, True):
            same_bits_and_oracle(both(lat, apply(lq, lat, D.adjoint() if dag else D, x)), refs[dag], (0, ON_NTB), (L, recon, bc, "D", dag))
            assert lat.get_param("recon_active") == (1 if recon == 12 else 0)
        ref = memo(("DdD", L, bc), lambda: orc.wilson_D(Uh, np.ascontiguousarray(refs[False]), L, KAPPA, 1.0, bc, True))
        same_bits_and_oracle(both(lat, apply(lq, lat, lq.DdagD_operator(D), x)), ref, (0, ON_NTB), (L, recon, bc, "DdagD"))
        for dag in (False, True):
            for out_sub, in_sub, p in ((lq.EVEN, lq.ODD, 0), (lq.ODD, lq.EVEN, 1)):
                xin = lq.Fermionfields(lat, lq.WILSON, in_sub).upload(bh)
                ref = memo(("hop", L, bc, dag, p), lambda: orc.wilson_hop_parity(Uh, bh, L, 1.0, bc, dag, p))
                same_bits_and_oracle(both(lat, apply(lq, lat, D.adjoint() if dag else D, xin, hop_to=out_sub)), ref, (0, ON_NTB), (L, recon, bc, "hop", dag, p))
    assert np.array_equal(x.download(), bh)


@pytest.mark.parametrize("L", [W32, TWIN], ids=IDS)
def test_12_plus_delta_links_take_plain_loads_on_purpose(gpu, orc, L):
    """gauge_delta = 1 on links 1e-10 off the group: the DELTA instance has no NTB = true twin (stencil.hip: the streamed form measured slower), the stores stream"""
    lq = gpu
    lat = context(lq, L, gauge_delta=1)
    rng = np.random.default_rng(5)
    Uh = links(orc, L)
    Up = np.ascontiguousarray(Uh + 1e-10 * (rng.standard_normal(Uh.shape) + 1j * rng.standard_normal(Uh.shape)) / 3.0)
    bh = source(orc, L)
    U = lq.Gaugefields(lat).upload(Up)
    x = lq.Fermionfields(lat, lq.WILSON).upload(bh)
    D = wilson(lq, U, ANTI)
    for dag in (False, True):
        ref = orc.wilson_D(Up, bh, L, KAPPA, 1.0, ANTI, dag)
        same_bits_and_oracle(both(lat, apply(lq, lat, D.adjoint() if dag else D, x)), ref, (0, ON), (L, "delta", dag))
        assert lat.get_param("recon_active") == 2


@pytest.mark.parametrize("L,grid", [(S16, 8), (TWIN, 64), (MID, 24)], ids=IDS)
def test_persistent_forms_and_the_direction_split_kernel(gpu, orc, L, grid):
    """dslash_pipe = 1 / 3: wilson_dirsplit_pipe<D, R, NTB> reached through pipe_grid and pipe_min_chunks = 1 as in tests/test_gpu_pipe.py; dslash_pipe = 0: wilson_dirsplit,
    which reads the hint word at run time (no NTB instance: bit 4 clear)"""
    lq = gpu
    Uh, bh = links(orc, L), source(orc, L)
    for recon in (12, 18):
        lat = context(lq, L, gauge_recon=recon, pipe_grid=grid, pipe_min_chunks=1)
        U = lq.Gaugefields(lat).upload(Uh)
        x = lq.Fermionfields(lat, lq.WILSON).upload(bh)
        D = wilson(lq, U, ANTI)
        got = {}
        for pipe, word in ((1, ON_NTB), (3, ON_NTB), (0, ON), (2, ON_NTB)):
            lat.set_param("dslash_pipe", pipe)
            for dag in (False, True):
                ref = memo(("D", L, ANTI, dag), lambda: orc.wilson_D(Uh, bh, L, KAPPA, 1.0, ANTI, dag))
                pair = both(lat, apply(lq, lat, D.adjoint() if dag else D, x))
                same_bits_and_oracle(pair, ref, (0, word), (L, recon, "dslash_pipe", pipe, dag))
                got[(pipe, dag)] = pair[1][0]
        for pipe in (1, 3, 0):      # the forms are the same arithmetic per site (tests/test_gpu_pipe.py): under the hints as well
            for dag in (False, True):
                assert np.array_equal(got[(pipe, dag)], got[(2, dag)]), (L, recon, pipe, dag)


@pytest.mark.parametrize("L", PARTIAL + [S16], ids=IDS)
def test_site_per_lane_kernels_every_block_size_r_and_hint_word(gpu, orc, L):
    """dslash_variant = 0 (wilson_interior<TB, D, RGEN>): blocks 64 / 128 / 256, r = 1 and r = 0.6, nt_gauge in {1, 2, 3, 4, 7} -- bits 1 and 2 of nt_gauge are the
    forward-link loads (k.nt & 2) and the spinor loads (k.nt & 8) of these kernels -- against nt_gauge = nt_store = 0 of the same context"""
    lq = gpu
    lat = context(lq, L, dslash_variant=0)
    Uh, bh = links(orc, L), source(orc, L)
    U = lq.Gaugefields(lat).upload(Uh)
    x = lq.Fermionfields(lat, lq.WILSON).upload(bh)
    y = x.similar()
    for r in (1.0, 0.6):
        D = wilson(lq, U, ANTI, r=r)
        for dag in (False, True):
            op = D.adjoint() if dag else D
            ref = orc.wilson_D(Uh, bh, L, KAPPA, r, ANTI, dag)
            for block in (64, 128, 256):
                lat.set_param("dslash_block", block)
                fh.off(lat)
                lq.mul_(y, op, x)
                off = y.download()
                assert lat.get_param("nt_active") == 0
                assert rel_err(off, ref) < TOL, (L, r, dag, block)
                lat.set_param("nt_store", 1)
                for g in (1, 2, 3, 4, 7):
                    lat.set_param("nt_gauge", g)
                    y.upload(np.full(lat.fermion_shape(lq.WILSON), np.nan + 1j * np.nan, dtype=np.complex128))
                    lq.mul_(y, op, x)
                    word = (g & 3) | 4 | (8 if g & 4 else 0)
                    assert lat.get_param("nt_active") == word, (L, r, dag, block, g, lat.get_param("nt_active"))
                    assert np.array_equal(y.download(), off), (L, r, dag, block, g)


# ------------------------------------------------------------------ 2. clover epilogue, five-dimensional launch, multi-column hop
@pytest.mark.parametrize("L", [S16, TWIN] + PARTIAL, ids=IDS)
def test_clover_epilogue_with_streamed_stores(gpu, orc, L):
    """a call that carries the packed clover blocks keeps wilson_dirsplit<D, R12, CLOVER> (run-time hint word): D and D^+ to 1e-13 as tests/test_gpu_clover.py holds them"""
    lq = gpu
    CSW = 1.5612
    Uh, bh = links(orc, L), source(orc, L)
    A = memo(("A", L, CSW), lambda: orc.clover_build(Uh, L, KAPPA, CSW))
    for recon in (12, 18):
        lat = context(lq, L, gauge_recon=recon)
        assert lat.get_param("clover_fused") == 1
        U = lq.Gaugefields(lat).upload(Uh)
        x = lq.Fermionfields(lat, lq.WILSON).upload(bh)
        D = lq.Dirac_operator(U, None, {"Dirac_operator": "WilsonClover", "κ": KAPPA, "Clover_coefficient": CSW, "boundarycondition": ANTI})
        for dag in (False, True):
            ref = memo(("Dsw", L, dag), lambda: orc.wilson_clover_D(Uh, A, bh, L, KAPPA, 1.0, ANTI, dag))
            same_bits_and_oracle(both(lat, apply(lq, lat, D.adjoint() if dag else D, x)), ref, (0, ON), (L, recon, "clover", dag))


def test_domainwall_five_dimensional_launch_with_streamed_stores(gpu, orc):
    """the DW5 instance reads the backward link with plain loads on purpose (the next slice re-uses it): bit 4 clear, stores stream"""
    lq = gpu
    L, L5, M, mass = S16, 3, -1.4, 0.07
    lat = context(lq, L)
    Uh = links(orc, L)
    U = lq.Gaugefields(lat).upload(Uh)
    x = lq.Initialize_pseudofermion_fields(U[1], "Domainwall", L5=L5, nowing=True)
    D = lq.Dirac_operator(U, x, {"Dirac_operator": "Domainwall", "mass": mass, "L5": L5, "M": M, "boundarycondition": ANTI})
    rng = np.random.default_rng(3)
    ph = rng.standard_normal((L5,) + orc.wilson_shape(L)) + 1j * rng.standard_normal((L5,) + orc.wilson_shape(L))
    x.upload(ph)
    y = x.similar()

    def call(op):
        def f():
            lq.mul_(y, op, x)
            assert lat.get_param("dw_active") == 1
            return y.download()
        return f
    for dag in (False, True):
        ref = orc.domainwall_D(Uh, ph, L, M, mass, ANTI, dagger=dag)
        same_bits_and_oracle(both(lat, call(D.adjoint() if dag else D)), ref, (0, ON), ("domainwall", dag))


@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("L", [S16, TWIN], ids=IDS)
def test_multi_column_hop_with_streamed_stores(gpu, orc, L, n):
    """stencil_mrhs.hip, k.nt & 4: plain link loads (nt_active = 4), n = 2, 3, 4 columns in one launch"""
    lq = gpu
    lat = context(lq, L)
    Uh = links(orc, L)
    U = lq.Gaugefields(lat).upload(Uh)
    D = wilson(lq, U, ANTI)
    cols = [source(orc, L, 300 + j) for j in range(n)]
    for p, (sub_out, sub_in) in enumerate(((lq.EVEN, lq.ODD), (lq.ODD, lq.EVEN))):
        xs = [lq.Fermionfields(lat, lq.WILSON, sub_in).upload(c) for c in cols]
        ys = [lq.Fermionfields(lat, lq.WILSON, sub_out) for _ in range(n)]
        for dag in (False, True):
            def call():
                lq.hop_multi_(ys, D.adjoint() if dag else D, xs)
                assert lat.get_param("mrhs_active") == n and lat.get_param("recon_active") == 1
                return np.stack([y.download() for y in ys])
            ref = np.stack([memo(("hop", L, 300 + j, dag, p), lambda: orc.wilson_hop_parity(Uh, cols[j], L, 1.0, ANTI, dag, p)) for j in range(n)])
            same_bits_and_oracle(both(lat, call), ref, (0, 4), (L, n, p, dag))


# ------------------------------------------------------------------ 3. staggered
@pytest.mark.parametrize("recon", [12, 18])
@pytest.mark.parametrize("stag_both", [0, 1])
@pytest.mark.parametrize("L", [S16, (8, 4, 6, 4)], ids=IDS)
def test_staggered_direction_split_kernel(gpu, orc, L, stag_both, recon):
    """staggered_dirsplit<R12, BOTH, NTB>: the BOTH instances have the NTB pair, the one-hop instances read the hint word at run time"""
    lq = gpu
    mass = 0.1
    lat = context(lq, L, stag_both=stag_both, gauge_recon=recon, cg_persist=0)
    Uh = links(orc, L)
    ph = memo(("s", L), lambda: orc.gaussian_spinor(orc.staggered_shape(L), 613))
    U = lq.Gaugefields(lat).upload(Uh)
    D = lq.Dirac_operator(U, None, {"Dirac_operator": "Staggered", "mass": mass, "boundarycondition": ANTI})
    x = lq.Fermionfields(lat, lq.STAGGERED).upload(ph)
    y = x.similar()
    for dag in (False, True):
        def call():
            y.upload(np.full(lat.fermion_shape(lq.STAGGERED), np.nan + 1j * np.nan, dtype=np.complex128))
            lq.mul_(y, D.adjoint() if dag else D, x)
            assert lat.get_param("recon_active") == (1 if recon == 12 else 0)
            return y.download()
        ref = memo(("Ds", L, dag), lambda: orc.staggered_D(Uh, ph, L, mass, ANTI, dag))
        same_bits_and_oracle(both(lat, call), ref, (0, ON_NTB if stag_both else ON), (L, stag_both, recon, dag))


# ------------------------------------------------------------------ 4. the fp32 build
@pytest.mark.parametrize("pair32", [1, 0])
def test_fp32_pair_and_direction_split_kernels_with_streamed_stores(gpu, orc, pair32):
    """stx_nt of stencil_pair32.hip and k.nt & 4 of the fp32 build of wilson_dirsplit, through lqcd_op_apply_f32 as tests/test_gpu_f32_operators.py: the bits of
    nt_store = 0 and that module's site-wise bound against the fp64 oracle"""
    lq = gpu
    L = S16
    lat = context(lq, L, mixed_pair32=pair32)
    Uh, bh = links(orc, L), source(orc, L)
    U = lq.Gaugefields(lat).upload(Uh)
    D = wilson(lq, U, ANTI)
    x = lq.Fermionfields(lat, lq.WILSON).upload(bh)
    y = x.similar()
    for dag in (False, True):
        out = {}
        for store in (0, 1):
            lat.set_param("nt_store", store)
            lq.mul_f32_(y, D.adjoint() if dag else D, x)
            assert lat.get_param("f32_form_active") == (3 if pair32 else 1) and lat.get_param("pair32_active") == pair32
            # the pair kernel has the NTB template pair, the fp32 direction-split kernel reads the word at run time
            assert lat.get_param("nt_active") == ((fh.NTB | 1) if pair32 else 1) | (4 if store else 0), (pair32, dag, store, lat.get_param("nt_active"))
            out[store] = y.download()
        assert np.array_equal(out[0], out[1]), (pair32, dag)
        K = fb.wilson_K(out[1], orc.wilson_D(Uh, bh, L, KAPPA, 1.0, ANTI, dag), bh, KAPPA, 1.0)
        print("fp32 pair32", pair32, "dagger", dag, "K %.3f" % K)
        assert K <= fb.K_ASSERT["wilson"], (pair32, dag, K)


# ------------------------------------------------------------------ 5. even-odd BiCGStab: the DOT, CINV and CINV + DOT instances
@pytest.mark.parametrize("csw", [0.0, 1.3])
@pytest.mark.parametrize("L", [(16, 8, 8, 8), (8, 8, 8, 16)], ids=IDS)
def test_evenodd_bicgstab_is_the_same_solve_under_the_hints(gpu, orc, L, csw):
    lq = gpu
    Uh, bh = links(orc, L), source(orc, L)
    sdir = L[0] == 16      # z-planes of whole chunks: the scalar-addressing instances; (8,8,8,16): the direction-split kernels with the same epilogues
    for dag in (False, True):
        if csw:
            A = memo(("A", L, csw), lambda: orc.clover_build(Uh, L, KAPPA, csw))
            xo, ito, rro, st = memo(("eo", L, csw, dag), lambda: orc.wilson_clover_bicgstab_eo(Uh, A, bh, L, KAPPA, 1.0, ANTI, dag, eps=1e-19))
        else:
            xo, ito, rro, st = memo(("eo", L, csw, dag), lambda: orc.wilson_bicgstab_eo(Uh, bh, L, KAPPA, 1.0, ANTI, dag, eps=1e-19))
        assert st == 0
        for hop_s in ((1, 0) if csw else (1,)):
            lat = context(lq, L, clover_hop_s=hop_s)
            U = lq.Gaugefields(lat).upload(Uh)
            D = lq.Dirac_operator(U, None, {"Dirac_operator": "WilsonClover" if csw else "Wilson", "Clover_coefficient": csw, "κ": KAPPA, "boundarycondition": ANTI,
                                            "eps_CG": 1e-19, "MaxCGstep": 3000})
            Dd = D.adjoint() if dag else D
            Dd.method_CG = "bicgstab_evenodd"
            b = lq.Fermionfields(lat, lq.WILSON).upload(bh)

            def call():
                x = b.similar()
                it, rr = lq.solve_DinvX_(x, Dd, b, return_info=True)
                return x.download(), it, rr
            (off, woff), (on, won) = both(lat, call)
            print("eo bicgstab", L, "csw", csw, "dagger", dag, "clover_hop_s", hop_s, "iterations", on[1], "oracle", ito, "nt_active", woff, won)
            assert off[1] == on[1] and off[2] == on[2] and np.array_equal(off[0], on[0]), (L, csw, dag, hop_s, off[1:], on[1:])
            assert on[2] < 1e-19 and abs(on[1] - ito) <= 2 and rel_err(on[0], xo) < 1e-9, (L, csw, dag, hop_s, on[1], ito, rel_err(on[0], xo))
            # the last stencil launch of a solve rebuilds the other parity: a plain hop, of the scalar-addressing kernel (NTB pair) where z-planes are whole chunks, of the
            # direction-split kernel (run-time word) elsewhere.  The DOT / CINV launches before it are covered by the bits of x, not by the key
            assert (woff, won) == (0, ON_NTB if sdir else ON), (woff, won)


# ------------------------------------------------------------------ 6. CG on D^+ D
FORMS = ((2, 8, 1), (3, 8, 1), (3, 8, 4))      # (cg_fused, cg_rring, cg_rring_mult)
TGS = ((0, 12), (2, 12), (2, 8))               # (cg_tgauge, cg_tgauge_recon)


def cg_system(lq, orc, L, eps=1e-16):
    Uh, bh = t8.problem(orc, L)            # hot-start links and a Gaussian source: the systems of tests/test_gpu_tgauge8.py (its oracle rows are shared)
    lat = context(lq, L, cg_persist=0, cg_small=0)
    U = lq.Gaugefields(lat).upload(Uh)
    D = wilson(lq, U, ANTI, eps_CG=eps)
    b = lq.Fermionfields(lat, lq.WILSON).upload(bh)
    return Uh, bh, lat, U, D, b


def cg_call(lq, D, b, n):
    """x after n iterations from zero through lqcd_solve_cg_DdagD_fixed; n = None: the solve to eps -> (x, iterations, r.r)"""
    def call():
        x = b.similar()
        if n is None:
            it, rr = lq.solve_DinvX_(x, lq.DdagD_operator(D), b, return_info=True)
            return x.download(), it, rr
        lq.lib.check(lq.lib.lib().lqcd_solve_cg_DdagD_fixed(D._h, x._h, b._h, int(n)))
        return x.download(), n, 0.0
    return call


def keep_settings(L):
    """[(cg_store_keep_mb, slabs)] resolving to one slab and to all slabs of the full-size map on L (cg.hip cg_setup: 864 B of launch traffic per site)"""
    nslab = fh.resolve(L, 16, 4)[5] * L[3]
    slab_bytes = 864 * (L[0] * L[1] * L[2] * L[3] // nslab)
    mb = -(-slab_bytes // (1 << 20))
    assert min((mb << 20) // slab_bytes, nslab) == 1
    return [(mb, 1), (1 << 10, nslab)]


def cg_active(lat):
    return {k: lat.get_param(k) for k in ("tgauge_active", "tgauge_recon_active", "cg_rring_active", "cg_rring_depth_active", "cg_sweep_alt_active", "cg_store_keep_active")}


@pytest.mark.parametrize("tg", TGS, ids=["plain", "tgauge12", "tgauge8"])
@pytest.mark.parametrize("L", CHUNKED, ids=IDS)
def test_cg_windows_and_solves_are_the_same_bits(gpu, orc, L, tg):
    """cg_fused = 2 and the residual ring at depths 8 and 32; without temporal gauge (plain instances in update / recurrence mode), with it on 12 reals (TG) and on 8 (TG8);
    the store policy at one slab and at all slabs; the sweep forwards and alternating; graph 0 / 1; the x- and y-share where XH = 16.  Windows of 3 d + 5 iterations and one
    solve to eps 1e-16 each."""
    lq = gpu
    Uh, bh, lat, U, D, b = cg_system(lq, orc, L)
    tgauge, recon = tg
    lat.set_param("cg_tgauge", tgauge)
    lat.set_param("cg_tgauge_recon", recon)
    keeps = keep_settings(L)
    share = 1 if L[0] == 32 else 0
    assert lat.get_param("dslash_xshare") == 1 and lat.get_param("dslash_yshare") == 1
    for fused, K, M in FORMS:
        lat.set_param("cg_fused", fused)
        lat.set_param("cg_rring", K)
        lat.set_param("cg_rring_mult", M)
        d = K * M if fused == 3 else K
        n = 3 * d + 5
        rows = [(alt, kp, graph) for alt in (0, 1) for kp in keeps for graph in (0, 1)] if tgauge else [(1, keeps[0], 0), (1, keeps[0], 1)]
        first = None
        for alt, (mb, slabs), graph in rows:
            lat.set_param("cg_sweep_alt", alt)
            lat.set_param("cg_store_keep_mb", mb)
            lat.set_param("graph", graph)
            (off, woff), (on, won) = both(lat, cg_call(lq, D, b, n))
            what = (L, tg, fused, K, M, alt, mb, graph)
            assert np.array_equal(off[0], on[0]), (what, "the hints changed a window", rel_err(on[0], off[0]))
            assert (woff, won) == (0, ON_NTB), (what, woff, won)
            assert cg_active(lat) == {"tgauge_active": 1 if tgauge else 0, "tgauge_recon_active": recon if tgauge else 0, "cg_rring_active": K if fused == 3 else 0,
                                      "cg_rring_depth_active": K * M if fused == 3 else 0, "cg_sweep_alt_active": 1 if (alt and tgauge) else 0,
                                      "cg_store_keep_active": slabs if (alt and tgauge) else -1}, (what, cg_active(lat))
            assert (lat.get_param("xshare_active"), lat.get_param("yshare_active")) == (share, share), what
            # store policy, sweep direction and graph replay change no value either (tests/test_gpu_cg_store_keep.py, tests/test_gpu_sweep_order.py): under the hints as well
            first = on[0] if first is None else first
            assert np.array_equal(on[0], first), what
        lat.set_param("graph", 0)
        if share:      # the two-load path under the hints
            lat.set_param("dslash_xshare", 0)
            got = cg_call(lq, D, b, n)()[0]
            assert (lat.get_param("xshare_active"), lat.get_param("yshare_active")) == (0, 0)
            lat.set_param("dslash_xshare", 1)
            lat.set_param("dslash_yshare", 0)
            got2 = cg_call(lq, D, b, n)()[0]
            assert (lat.get_param("xshare_active"), lat.get_param("yshare_active")) == (1, 0)
            lat.set_param("dslash_yshare", 1)
            assert np.array_equal(got, first) and np.array_equal(got2, first), (L, tg, fused, K, M, "share")
        (off, woff), (on, won) = both(lat, cg_call(lq, D, b, None))
        print("cg", L, tg, (fused, K, M), "solve to 1e-16:", on[1], "iterations, r.r %.3e" % on[2], "nt_active", woff, won)
        assert off[1] == on[1] > 10 and off[2] == on[2] < 1e-16 and np.array_equal(off[0], on[0]), (L, tg, fused, K, M, off[1:], on[1:])
        assert (woff, won) == (0, ON_NTB)
    assert np.array_equal(b.download(), bh)


@pytest.mark.parametrize("L", [TWIN, W32], ids=IDS)
def test_cg_under_the_full_size_map_against_the_oracle(gpu, orc, L):
    """32.32.8.4 resolves like 32^3 x 64 and no other test runs it (32.8.8.4: the other shape with the shares): the hints-on solve stops within one iteration of the oracle's
    with x within 1e-9, in every link format; the 8-real window against the 12-real one within 10 x what decode(encode(.)) does to the oracle's own window
    (tests/test_gpu_tgauge8.py)"""
    lq = gpu
    Uh, bh, lat, U, D, b = cg_system(lq, orc, L)
    assert fh.resolve(L, 16, 4) == ((16, 4, 2, 2, 4, 2) if L == TWIN else (16, 2, 1, 1, 1, 2))
    before = orc.lib().orc_get_threads()
    orc.set_threads(8)      # the oracle's site loops are OpenMP-parallel (as tests/hard_systems.py runs them): the same arithmetic per site, its sums in thread order
    try:
        xo, ito, rro, st = memo(("cg", L), lambda: orc.cg_DdagD(orc.WILSON, Uh, bh, L, KAPPA, 1.0, ANTI, eps=1e-16))
        want = t8.oracle_pair(orc, L, ANTI, 29)
    finally:
        orc.set_threads(before)
    assert st == 0
    lat.set_param("cg_store_keep_mb", keep_settings(L)[0][0])
    wins = {}
    for fused, K, M in FORMS:
        lat.set_param("cg_fused", fused)
        lat.set_param("cg_rring", K)
        lat.set_param("cg_rring_mult", M)
        for tgauge, recon in TGS:
            lat.set_param("cg_tgauge", tgauge)
            lat.set_param("cg_tgauge_recon", recon)
            x, it, rr = cg_call(lq, D, b, None)()
            err = rel_err(x, xo)
            print("cg", L, (fused, K, M), (tgauge, recon), "iterations", it, "oracle", ito, "rel err %.3e" % err, "nt_active", lat.get_param("nt_active"))
            assert lat.get_param("nt_active") == ON_NTB and lat.get_param("tgauge_recon_active") == (recon if tgauge else 0)
            assert abs(it - ito) <= 1 and rr < 1e-16 and err < 1e-9, (L, fused, K, M, tgauge, recon, it, ito, rr, err)
            if (fused, K, M) == (3, 8, 1) and tgauge:
                wins[recon] = cg_call(lq, D, b, 29)()[0]
    assert lq.tgauge8_deviation(U) <= 1e-14
    got = t8.relmax(wins[8], wins[12])
    print("cg", L, "window 29: oracle 12 vs 8 %.3e, device 12 vs 8 %.3e" % (want, got))
    assert 0.0 < got <= 10.0 * want, (got, want)


# ------------------------------------------------------------------ 7. the update kernels' own hint
def test_nt_blas_is_a_hint(gpu, orc):
    """nt_blas = 0 against 1: the <false> instances of the fp64 update kernels (cg_fused = 2, the ring's batch kernel), ms_update_all (multi-shift, 3 shifts) and
    cg32_update_* (mixed-precision CG), under the full-size stencil hints"""
    lq = gpu
    L = MID
    Uh, bh, lat, U, D, b = cg_system(lq, orc, L)
    assert lat.get_param("nt_blas") == 1
    A = lq.DdagD_operator(D)

    def pair(call):
        out = []
        for v in (0, 1):
            lat.set_param("nt_blas", v)
            out.append(call())
        return out
    for tgauge in (0, 2):
        lat.set_param("cg_tgauge", tgauge)
        lat.set_param("cg_tgauge_recon", 12)
        for fused, K, M in FORMS:
            lat.set_param("cg_fused", fused)
            lat.set_param("cg_rring", K)
            lat.set_param("cg_rring_mult", M)
            n = 3 * (K * M if fused == 3 else K) + 5
            w0, w1 = pair(cg_call(lq, D, b, n))
            assert lat.get_param("cg_rring_depth_active") == (K * M if fused == 3 else 0) and lat.get_param("nt_active") == ON_NTB
            assert np.array_equal(w0[0], w1[0]), (tgauge, fused, K, M)
            s0, s1 = pair(cg_call(lq, D, b, None))
            assert s0[1] == s1[1] > 10 and s0[2] == s1[2] and np.array_equal(s0[0], s1[0]), (tgauge, fused, K, M)

    def multishift():
        xs = [b.similar() for _ in range(3)]
        x0 = b.similar()
        it, rr = lq.shiftedcg(xs, [0.01, 0.1, 1.0], x0, A, b, eps=1e-16, return_info=True)
        return [x0.download()] + [x.download() for x in xs], it, rr
    m0, m1 = pair(multishift)
    assert m0[1] == m1[1] > 10 and m0[2] == m1[2] and all(np.array_equal(a, c) for a, c in zip(m0[0], m1[0]))
    res = bh - orc.wilson_D(Uh, orc.wilson_D(Uh, np.ascontiguousarray(m1[0][2]), L, KAPPA, 1.0, ANTI), L, KAPPA, 1.0, ANTI, True) - 0.1 * m1[0][2]
    assert float(np.vdot(res, res).real) < 1e-15      # (a solve, not two equal failures)

    def mixed():
        x = b.similar()
        lq.clear_fermion_(x)
        info = lq.solve_mixed_DinvX_(x, A, b, return_info=True)
        return x.download(), info
    x0, x1 = pair(mixed)
    assert x0[1] == x1[1] and x1[1][2] < 1e-16 and np.array_equal(x0[0], x1[0]), (x0[1], x1[1])
    fb.no_handoff(lat, "mixed CG under the full-size hints")


# ------------------------------------------------------------------ 8. the folded halo schedule
FOLD_CODE = textwrap.dedent("""
    import os, sys, numpy as np
    sys.path.insert(0, os.getcwd())
    sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
    import latticeqcd_jl_amd as lq
    import fullsize_hints as fh
    from oracle import oracle as orc
    L, SDIR, K, BC = %s, %d, 0.141139, (1, 1, 1, -1)
    lat = lq.Lattice(L)
    assert {k: lat.get_param(k) for k in fh.FULLSIZE} == fh.adaptive(L)
    lat.comm_init(lq.comm_unique_id())
    assert lat.get_param("halo_stream_mode") == 3 and lat.get_param("halo_fold") == 1
    Uh = orc.hot_gauge(L, 111)
    U = lq.Gaugefields(lat).upload(Uh)
    D = lq.Dirac_operator(U, None, {"Dirac_operator": "Wilson", "κ": K, "boundarycondition": BC})
    psi = orc.gaussian_spinor(lat.fermion_shape(lq.WILSON), 112)
    x = lq.Fermionfields(lat, lq.WILSON).upload(psi)
    y = x.similar()
    fh.on(lat)
    for dag in (False, True):
        out, word = [], []
        for hints in (fh.off, fh.on):
            hints(lat)
            y.upload(np.full(psi.shape, np.nan + 1j * np.nan))
            lq.mul_(y, D.adjoint() if dag else D, x)
            assert lat.get_param("halo_fold_active") == 1 and lat.get_param("recon_active") == 1
            out.append(y.download())
            word.append(lat.get_param("nt_active"))
        ref = orc.wilson_D(Uh, psi, L, K, 1.0, BC, dag)
        err = np.abs(out[1] - ref).max() / np.abs(ref).max()
        print("fold", L, os.environ["LQCD_FORCE_PARTITION"], "dagger", dag, "rel err %%.3e" %% err, "nt_active", word)
        assert not np.isnan(out[1]).any() and np.array_equal(out[0], out[1]), ("the hints changed a value", dag)
        assert err < 1e-13, (dag, err)
        # the FOLD instances of the scalar-addressing kernel have the NTB pair; their folded direction-split twins read the word at run time
        assert word == [0, (fh.FULL_WORD | fh.NTB) if SDIR else fh.FULL_WORD], (dag, word)
    print("FOLD_HINTS_OK")
""")


@pytest.mark.parametrize("mask", ["8", "14"])
@pytest.mark.parametrize("L,sdir", [((8, 4, 6, 8), 0), (S16, 1)], ids=IDS)
def test_folded_halo_schedule_in_a_fresh_process_per_partition_mask(gpu, L, sdir, mask):
    """LQCD_FORCE_PARTITION in {8, 14} with LQCD_HALO_STREAM_MODE = 3: wilson_dirsplit_s<D, R, NTB, ..., FOLD> on 16.8.8.4, wilson_dirsplit_fold on (8,4,6,8)"""
    env = dict(os.environ, LQCD_FORCE_PARTITION=mask, LQCD_HALO_STREAM_MODE="3", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-c", FOLD_CODE % (L, sdir)], capture_output=True, text=True, env=env, timeout=300,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print(r.stdout[-1500:])
    assert r.returncode == 0 and "FOLD_HINTS_OK" in r.stdout, (L, mask, r.stdout[-1500:], r.stderr[-3000:])
