"""Every instance of the fp32 operators of the mixed-precision solvers, one application through lqcd_op_apply_f32, against the fp64 oracle on the unrounded
inputs at the site-wise bound K <= K_ASSERT of tests/f32_bound.py (fixed from the NumPy fp32 restatement, tests/test_cpu_f32_bound.py; never from a device
result).  Each case states which kernel form it must reach and reads it back from the read-only key f32_form_active -- a case that silently lands in another
kernel fails -- and runs D and D^+.  The mixed-precision solvers repair a wrong inner operator by themselves (extra correction steps, or the hand-off to the
fp64 solver), so their own tests cannot see one; the solves at the end of this file assert that no hand-off was taken (mixed_handoffs, mixed_fp64_iters) and
that the number of correction steps is the solver's own plan."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import f32_bound as fb

pytestmark = pytest.mark.gpu

KAPPA, CSW = 0.141139, 1.5612
INTERIOR, DIRSPLIT, PIPE, PAIR, FOLDED, EXTERIOR = 0, 1, 2, 3, 4, 8      # f32_form_active (+ EXTERIOR: an exterior launch followed)
SMALL = [(4, 4, 4, 4), (8, 4, 6, 2), (6, 6, 4, 2)]      # the last one: a partially filled chunk
BIG = (16, 8, 8, 4)                                      # z-planes of whole chunks: the pipe and pair kernels
BCS = [(1, 1, 1, -1), (-1, -1, 1, 1), (1, -1, -1, -1), (-1, 1, -1, 1)]      # every direction antiperiodic and periodic at least once
BASE = {"dslash_variant": 1, "gauge_recon": 12, "dslash_pipe": 2, "mixed_pair32": 1, "xcd_remap": 2, "dslash_block": 128, "stag_both": 0, "nt_gauge": 1}


@pytest.fixture(scope="module")
def gpu(lq):
    assert lq.lib.device_count() > 0, "no HIP device visible: the product has no CPU fallback"
    return lq


_cache = {}


def links(orc, L, seed=41, nonunitary=False):
    key = (L, seed, nonunitary)
    if key not in _cache:
        U = orc.hot_gauge(L, seed)
        if nonunitary:      # 1e-3 per element: far outside the 1e-14 of the 12-real rule, far inside the slack of ||U||_2 = 1 in S(n) (factor 6)
            U = U + 1e-3 * orc.gaussian_spinor(U.shape, seed + 1000)
        _cache[key] = np.ascontiguousarray(U)
    return _cache[key]


def setup(lq, L, tun):
    lat = lq.Lattice(L)
    for k, v in dict(BASE, **tun).items():
        lat.set_param(k, v)
    return lat


def check_both(lq, lat, D, x, y, ref_of, K_of, kind, form, label, pair=None):
    """D and D^+ through the fp32 operator: the form that ran, then the site-wise bound"""
    for dag in (False, True):
        lq.mul_f32_(y, D.adjoint() if dag else D, x)
        got = lat.get_param("f32_form_active")
        assert got == form, (label, dag, "f32_form_active", got, "expected", form)
        if pair is not None:
            assert lat.get_param("pair32_active") == pair, (label, dag)
        K = K_of(y.download(), ref_of(dag))
        print("K %-9s form %d %s dagger %d: %.3f" % (kind, form, label, dag, K))
        assert K <= fb.K_ASSERT[kind], (label, dag, K)


# ------------------------------------------------------------------------------------------------ Wilson r = 1
WILSON = [
    # (L, bc, tunables, non-unitary links, form, pair32_active)
    (BIG, BCS[0], {}, False, PAIR, 1),
    (BIG, BCS[1], {}, False, PAIR, 1),
    (BIG, BCS[2], {"mixed_pair32": 0}, False, DIRSPLIT, 0),
    (BIG, BCS[3], {"xcd_remap": 0}, False, DIRSPLIT, 0),                       # the pair kernel needs the XCD tile map: dropped
    (BIG, BCS[0], {"gauge_recon": 18}, False, DIRSPLIT, 0),                    # 18 reals: no pair kernel
    (BIG, BCS[1], {}, True, DIRSPLIT, 0),                                      # 18 forced by non-unitary links (use12 rule of mix_prepare)
    (BIG, BCS[2], {"dslash_pipe": 0, "mixed_pair32": 0}, False, DIRSPLIT, 0),
    (BIG, BCS[3], {"dslash_pipe": 1, "pipe_grid": 8, "pipe_min_chunks": 1, "mixed_pair32": 0}, False, PIPE, 0),
    (BIG, BCS[0], {"dslash_pipe": 3, "pipe_grid": 8, "pipe_min_chunks": 1, "mixed_pair32": 0}, False, PIPE, 0),
    (BIG, BCS[1], {"dslash_pipe": 1, "pipe_grid": 8, "pipe_min_chunks": 1, "mixed_pair32": 0, "gauge_recon": 18}, False, PIPE, 0),
    (BIG, BCS[2], {"dslash_pipe": 3, "pipe_grid": 8, "pipe_min_chunks": 1, "mixed_pair32": 0}, True, PIPE, 0),
    (BIG, BCS[3], {"dslash_variant": 0}, False, INTERIOR, 0),
    (SMALL[0], BCS[0], {}, False, DIRSPLIT, 0),                                # geometries the pair kernel does not take
    (SMALL[1], BCS[1], {}, False, DIRSPLIT, 0),
    (SMALL[2], BCS[2], {}, False, DIRSPLIT, 0),
    (SMALL[2], BCS[3], {"gauge_recon": 18}, False, DIRSPLIT, 0),
    (SMALL[0], BCS[3], {"dslash_variant": 0}, False, INTERIOR, 0),
    (SMALL[1], BCS[2], {"dslash_variant": 0, "dslash_block": 64}, False, INTERIOR, 0),
    (SMALL[2], BCS[1], {"dslash_variant": 0, "dslash_block": 256}, False, INTERIOR, 0),
]


@pytest.mark.parametrize("case", WILSON, ids=lambda c: "%s-%s-%s%s" % ("x".join(map(str, c[0])), "".join("a" if s < 0 else "p" for s in c[1]),
                                                                       ",".join("%s=%d" % kv for kv in c[2].items()) or "default", "-nonunitary" if c[3] else ""))
def test_wilson_r1_instances(gpu, orc, case):
    lq = gpu
    L, bc, tun, nonunit, form, pair = case
    lat = setup(lq, L, tun)
    Uh = links(orc, L, nonunitary=nonunit)
    U = lq.Gaugefields(lat).upload(Uh)
    D = lq.Dirac_operator(U, None, {"Dirac_operator": "Wilson", "κ": KAPPA, "boundarycondition": bc})
    psi = orc.gaussian_spinor(lat.fermion_shape(lq.WILSON), 42)
    x = lq.Fermionfields(lat, lq.WILSON).upload(psi)
    check_both(lq, lat, D, x, x.similar(), lambda dag: orc.wilson_D(Uh, psi, L, KAPPA, 1.0, bc, dag), lambda o, r: fb.wilson_K(o, r, psi, KAPPA, 1.0),
               "wilson", form, str(case[:4]), pair)


@pytest.mark.parametrize("L,bc", [(SMALL[2], BCS[0]), (BIG, BCS[3])])
@pytest.mark.parametrize("variant", [0, 1])
def test_wilson_general_r_reaches_the_interior_kernel_under_either_variant(gpu, orc, L, bc, variant):
    lq = gpu
    lat = setup(lq, L, {"dslash_variant": variant})
    Uh = links(orc, L)
    U = lq.Gaugefields(lat).upload(Uh)
    D = lq.Dirac_operator(U, None, {"Dirac_operator": "Wilson", "κ": KAPPA, "r": 0.7, "boundarycondition": bc})
    psi = orc.gaussian_spinor(lat.fermion_shape(lq.WILSON), 42)
    x = lq.Fermionfields(lat, lq.WILSON).upload(psi)
    check_both(lq, lat, D, x, x.similar(), lambda dag: orc.wilson_D(Uh, psi, L, KAPPA, 0.7, bc, dag), lambda o, r: fb.wilson_K(o, r, psi, KAPPA, 0.7),
               "wilson", INTERIOR, "r=0.7 %s variant %d" % (L, variant), 0)


# ------------------------------------------------------------------------------------------------ Wilson-clover
@pytest.mark.parametrize("L", SMALL + [BIG])
@pytest.mark.parametrize("recon", [12, 18])
def test_wilson_clover_instances_follow_links_and_coefficient(gpu, orc, L, recon):
    import ctypes as C
    lq = gpu
    bc = (1, 1, 1, -1)      # the boundary condition of test_gpu_clover.py
    lat = setup(lq, L, {"gauge_recon": recon})
    psi = orc.gaussian_spinor(lat.fermion_shape(lq.WILSON), 502)
    x = lq.Fermionfields(lat, lq.WILSON).upload(psi)
    y = x.similar()
    Uh = links(orc, L, 501)
    U = lq.Gaugefields(lat).upload(Uh)
    D = lq.Dirac_operator(U, None, {"Dirac_operator": "WilsonClover", "κ": KAPPA, "Clover_coefficient": CSW, "boundarycondition": bc})

    def run(Uh, csw, label):
        A = orc.clover_build(Uh, L, KAPPA, csw)
        check_both(lq, lat, D, x, y, lambda dag: orc.wilson_clover_D(Uh, A, psi, L, KAPPA, 1.0, bc, dag), lambda o, r: fb.wilson_K(o, r, psi, KAPPA, 1.0, A),
                   "clover", DIRSPLIT, "%s recon %d %s" % (L, recon, label), 0)

    run(Uh, CSW, "first links")
    Uh2 = links(orc, L, 503)
    U.upload(Uh2)                    # new links in the same handle: the fp32 copy of the blocks must follow them
    run(Uh2, CSW, "new links")
    lq.lib.check(lq.lib.lib().lqcd_op_set_clover(D._h, C.c_double(1.1)))      # same links, new coefficient
    run(Uh2, 1.1, "new csw")


def test_wilson_clover_refuses_the_site_per_lane_kernel(gpu, orc):
    lq = gpu
    L = SMALL[0]
    lat = setup(lq, L, {"dslash_variant": 0})
    U = lq.Gaugefields(lat).upload(links(orc, L, 501))
    D = lq.Dirac_operator(U, None, {"Dirac_operator": "WilsonClover", "κ": KAPPA, "Clover_coefficient": CSW})
    x = lq.Fermionfields(lat, lq.WILSON).upload(orc.gaussian_spinor(lat.fermion_shape(lq.WILSON), 502))
    with pytest.raises(lq.LQCDError, match="needs the direction-split kernel"):
        lq.mul_f32_(x.similar(), D, x)


# ------------------------------------------------------------------------------------------------ staggered
STAG = [
    # (L, bc, mass, tunables, form)
    (SMALL[0], BCS[0], 0.5, {}, DIRSPLIT),
    (SMALL[1], BCS[1], 0.01, {}, DIRSPLIT),
    (SMALL[2], BCS[2], 0.01, {"gauge_recon": 18}, DIRSPLIT),
    (BIG, BCS[3], 0.5, {"gauge_recon": 18}, DIRSPLIT),
    (BIG, BCS[0], 0.01, {"stag_both": 1, "nt_gauge": 1}, DIRSPLIT),                      # BOTH, NTB instance (odd nt)
    (BIG, BCS[1], 0.5, {"stag_both": 1, "nt_gauge": 0}, DIRSPLIT),                       # BOTH, even nt
    (SMALL[2], BCS[3], 0.01, {"stag_both": 1, "nt_gauge": 1, "gauge_recon": 18}, DIRSPLIT),
    (SMALL[2], BCS[0], 0.5, {"stag_both": 1, "nt_gauge": 0}, DIRSPLIT),
    (SMALL[1], BCS[2], 0.01, {"stag_both": 0, "nt_gauge": 0}, DIRSPLIT),
    (SMALL[2], BCS[1], 0.01, {"dslash_variant": 0, "dslash_block": 64}, INTERIOR),
    (SMALL[0], BCS[2], 0.5, {"dslash_variant": 0, "dslash_block": 128}, INTERIOR),
    (BIG, BCS[3], 0.01, {"dslash_variant": 0, "dslash_block": 256}, INTERIOR),
    (SMALL[2], BCS[0], 0.5, {"dslash_variant": 0, "dslash_block": 256}, INTERIOR),
]


@pytest.mark.parametrize("case", STAG, ids=lambda c: "%s-%s-m%g-%s" % ("x".join(map(str, c[0])), "".join("a" if s < 0 else "p" for s in c[1]), c[2],
                                                                     ",".join("%s=%d" % kv for kv in c[3].items()) or "default"))
def test_staggered_instances(gpu, orc, case):
    lq = gpu
    L, bc, mass, tun, form = case
    lat = setup(lq, L, tun)
    Uh = links(orc, L)
    U = lq.Gaugefields(lat).upload(Uh)
    D = lq.Dirac_operator(U, None, {"Dirac_operator": "Staggered", "mass": mass, "boundarycondition": bc})
    chi = orc.gaussian_spinor(lat.fermion_shape(lq.STAGGERED), 43)
    x = lq.Fermionfields(lat, lq.STAGGERED).upload(chi)
    check_both(lq, lat, D, x, x.similar(), lambda dag: orc.staggered_D(Uh, chi, L, mass, bc, dag), lambda o, r: fb.staggered_K(o, r, chi, mass),
               "staggered", form, str(case[:4]))


# ------------------------------------------------------------------------------------------------ the link-copy cache of mix_prepare
def test_link_copy_cache_follows_layout_reals_and_handle(gpu, orc):
    """mix_gauge18_valid / mix_gauge12_valid / mix_gauge12_layout: one context, two gauge handles, the pair and the one-site layouts of the 12-real copy and the
    18-real copy in alternation, new links in one handle in between.  Every application against the oracle for the links that handle holds NOW."""
    lq = gpu
    L, bc = BIG, (1, 1, 1, -1)
    lat = setup(lq, L, {})
    held = [links(orc, L, 61), links(orc, L, 62)]
    Us = [lq.Gaugefields(lat).upload(h) for h in held]
    Ds = [lq.Dirac_operator(u, None, {"Dirac_operator": "Wilson", "κ": KAPPA, "boundarycondition": bc}) for u in Us]
    psi = orc.gaussian_spinor(lat.fermion_shape(lq.WILSON), 42)
    x = lq.Fermionfields(lat, lq.WILSON).upload(psi)
    y = x.similar()
    # (handle, mixed_pair32, gauge_recon, upload new links with this seed first, form)
    seq = [(0, 1, 12, None, PAIR), (0, 0, 12, None, DIRSPLIT), (0, 0, 18, None, DIRSPLIT), (1, 1, 12, None, PAIR), (0, 0, 12, None, DIRSPLIT), (0, 1, 12, None, PAIR),
           (0, 1, 12, 63, PAIR), (1, 0, 18, None, DIRSPLIT), (0, 0, 18, None, DIRSPLIT), (1, 0, 12, 64, DIRSPLIT), (1, 1, 12, None, PAIR), (0, 0, 12, None, DIRSPLIT),
           (1, 1, 12, 65, PAIR), (1, 0, 18, None, DIRSPLIT)]
    for step, (h, pair, recon, seed, form) in enumerate(seq):
        if seed is not None:
            held[h] = links(orc, L, seed)
            Us[h].upload(held[h])
        lat.set_param("mixed_pair32", pair)
        lat.set_param("gauge_recon", recon)
        Uh = held[h]
        check_both(lq, lat, Ds[h], x, y, lambda dag: orc.wilson_D(Uh, psi, L, KAPPA, 1.0, bc, dag), lambda o, r: fb.wilson_K(o, r, psi, KAPPA, 1.0),
                   "wilson", form, "cache step %d %s" % (step, (h, pair, recon, seed)), pair)


# ------------------------------------------------------------------------------------------------ partitioned lattice (fp32 pack, exterior and folded kernels)
PART_CODE = """
    import os, sys, numpy as np
    sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
    import latticeqcd_jl_amd as lq
    from oracle import oracle as orc
    import f32_bound as fb
    L, K, CSW = (8, 4, 6, 8), 0.141139, 1.5612
    lat = lq.Lattice(L)
    lat.comm_init(lq.comm_unique_id())
    Uh = orc.hot_gauge(L, 111)
    U = lq.Gaugefields(lat).upload(Uh)
    A = orc.clover_build(Uh, L, K, CSW)
    psi = orc.gaussian_spinor(lat.fermion_shape(lq.WILSON), 112)
    chi = orc.gaussian_spinor(lat.fermion_shape(lq.STAGGERED), 113)
    xw = lq.Fermionfields(lat, lq.WILSON).upload(psi); yw = xw.similar()
    xs = lq.Fermionfields(lat, lq.STAGGERED).upload(chi); ys = xs.similar()
    BCS = [(1, 1, 1, -1), (-1, -1, 1, 1), (1, -1, -1, -1), (-1, 1, -1, 1)]
    n = 0
    for fold in (1, 0):
        lat.set_param("halo_fold", fold)
        form = 4 if fold else 1 + 8      # folded twin of the direction-split kernel / direction-split interior + exterior
        for bc in BCS[2 * fold:2 * fold + 2]:
            cases = [
                ("wilson", "wilson r=1", {"Dirac_operator": "Wilson", "κ": K}, xw, yw, lambda dag: orc.wilson_D(Uh, psi, L, K, 1.0, bc, dag), lambda o, r: fb.wilson_K(o, r, psi, K, 1.0)),
                ("wilson", "wilson r=0.7 (two r = 1 calls)", {"Dirac_operator": "Wilson", "κ": K, "r": 0.7}, xw, yw, lambda dag: orc.wilson_D(Uh, psi, L, K, 0.7, bc, dag), lambda o, r: fb.wilson_K(o, r, psi, K, 0.7)),
                ("clover", "clover", {"Dirac_operator": "WilsonClover", "κ": K, "Clover_coefficient": CSW}, xw, yw, lambda dag: orc.wilson_clover_D(Uh, A, psi, L, K, 1.0, bc, dag), lambda o, r: fb.wilson_K(o, r, psi, K, 1.0, A)),
                ("staggered", "staggered m=0.01", {"Dirac_operator": "Staggered", "mass": 0.01}, xs, ys, lambda dag: orc.staggered_D(Uh, chi, L, 0.01, bc, dag), lambda o, r: fb.staggered_K(o, r, chi, 0.01)),
            ]
            for kind, label, par, x, y, ref_of, K_of in cases:
                D = lq.Dirac_operator(U, None, dict(par, boundarycondition=bc))
                for dag in (False, True):
                    lq.mul_f32_(y, D.adjoint() if dag else D, x)
                    got, fa = lat.get_param("f32_form_active"), lat.get_param("halo_fold_active")
                    assert got == form and fa == fold, (label, fold, bc, dag, "f32_form_active", got, "halo_fold_active", fa)
                    Kv = K_of(y.download(), ref_of(dag))
                    print("K %-9s form %2d %s fold %d bc %s dagger %d: %.3f" % (kind, form, label, fold, bc, dag, Kv))
                    assert Kv <= fb.K_ASSERT[kind], (label, fold, bc, dag, Kv)
                    n += 1
    print("F32_PARTITIONED_OK", n)
"""


@pytest.mark.parametrize("mask", ["8", "15"])
def test_partitioned_fp32_pack_exterior_and_folded_kernels(gpu, mask):
    """LQCD_FORCE_PARTITION + a world-size-1 RCCL communicator (as test_rccl_self_partition_clover): t only, and every direction."""
    env = dict(os.environ, LQCD_FORCE_PARTITION=mask, HSA_ENABLE_IPC_MODE_LEGACY="0", LQCD_HALO_STREAM_MODE="3")
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(PART_CODE)], capture_output=True, text=True, env=env, timeout=300,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print(r.stdout[-6000:])
    assert r.returncode == 0 and "F32_PARTITIONED_OK 32" in r.stdout, (mask, r.stdout[-3000:], r.stderr[-3000:])


# ------------------------------------------------------------------------------------------------ the solves: no hand-off, the planned number of steps
SOLVES = [
    ("wilson-pair", BIG, {}, {"Dirac_operator": "Wilson", "κ": KAPPA}, PAIR),
    ("wilson-dirsplit", BIG, {"mixed_pair32": 0}, {"Dirac_operator": "Wilson", "κ": KAPPA}, DIRSPLIT),
    ("wilson-r0.7", SMALL[2], {}, {"Dirac_operator": "Wilson", "κ": KAPPA, "r": 0.7}, INTERIOR),
    ("clover", SMALL[2], {}, {"Dirac_operator": "WilsonClover", "κ": KAPPA, "Clover_coefficient": CSW}, DIRSPLIT),
    ("staggered", SMALL[2], {}, {"Dirac_operator": "Staggered", "mass": 0.5}, DIRSPLIT),
]


@pytest.mark.parametrize("case", SOLVES, ids=lambda c: c[0])
def test_mixed_cg_takes_no_handoff_and_the_planned_steps(gpu, orc, case):
    lq = gpu
    name, L, tun, par, form = case
    eps = 1e-18
    lat = setup(lq, L, tun)
    U = lq.Gaugefields(lat).upload(links(orc, L))
    D = lq.Dirac_operator(U, None, dict(par, boundarycondition=(1, 1, 1, -1), eps_CG=eps, MaxCGstep=3000))
    kind = lq.STAGGERED if par["Dirac_operator"] == "Staggered" else lq.WILSON
    bh = orc.gaussian_spinor(lat.fermion_shape(kind), 46)
    b = lq.Fermionfields(lat, kind).upload(bh)
    A = lq.DdagD_operator(D)
    sol = b.similar()
    lq.clear_fermion_(sol)
    it, outer, rr = lq.solve_mixed_DinvX_(sol, A, b, return_info=True)
    steps = fb.planned_steps(eps, float(np.vdot(bh, bh).real))
    print("mixed CG %s: %d fp32 iterations, %d steps (plan %d), |r|^2 %.2e" % (name, it, outer, steps, rr))
    assert lat.get_param("f32_form_active") == form
    assert lat.get_param("mixed_handoffs") == 0 and lat.get_param("mixed_fp64_iters") == 0, name
    assert rr < eps and steps <= outer <= steps + 1, (name, outer, steps)
    r = b.similar()
    lq.mul_(r, A, sol)
    lq.add_fermion_(r, -1.0, b)
    assert lq.dot(r, r).real < eps
    # the mixed multi-shift CG on the same operator: no correction handed to the fp64 solver
    sig = [0.01, 0.1, 1.0]
    xs = [b.similar() for _ in sig]
    lq.shiftedcg_mixed(xs, sig, None, A, b, eps=1e-16)
    assert lat.get_param("mixed_handoffs") == 0 and lat.get_param("mixed_fp64_iters") == 0, name
    for s, xj in zip(sig, xs):
        lq.mul_(r, A, xj)
        lq.add_fermion_(r, s, xj)
        lq.add_fermion_(r, -1.0, b)
        assert lq.dot(r, r).real < 1e-16, (name, s)


@pytest.mark.parametrize("clover", [False, True])
def test_mixed_evenodd_bicgstab_takes_no_handoff(gpu, orc, clover):
    lq = gpu
    L, bc = BIG, (1, 1, 1, -1)
    lat = setup(lq, L, {"bicg_mixed": 1})
    Uh = links(orc, L)
    U = lq.Gaugefields(lat).upload(Uh)
    par = {"Dirac_operator": "WilsonClover" if clover else "Wilson", "κ": KAPPA, "boundarycondition": bc, "eps_CG": 1e-18, "method_CG": "bicgstab_evenodd"}
    if clover:
        par["Clover_coefficient"] = CSW
    D = lq.Dirac_operator(U, None, par)
    b = lq.Fermionfields(lat, lq.WILSON).upload(orc.gaussian_spinor(lat.fermion_shape(lq.WILSON), 46))
    for dag in (False, True):
        Dd = D.adjoint() if dag else D
        sol = b.similar()
        lq.clear_fermion_(sol)
        lq.solve_DinvX_(sol, Dd, b)
        assert lat.get_param("f32_form_active") == (DIRSPLIT if clover else PAIR)
        assert lat.get_param("mixed_handoffs") == 0 and lat.get_param("mixed_fp64_iters") == 0, (clover, dag)
        r = b.similar()
        lq.mul_(r, Dd, sol)
        lq.add_fermion_(r, -1.0, b)
        assert lq.dot(r, r).real < 1e-16, (clover, dag)
