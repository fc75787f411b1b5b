"""The epilogues that steer the fp32 inner solvers, one launch each through lqcd_bench_stencil_f32 (the fp32 sibling of lqcd_bench_stencil_epilogue):

  mode 0  the first launch of an inner_cg32 iteration: dst = D in with the |D in|^2 partials
  mode 1  its update-mode second launch: dst = src - coef D^+ in with the |dst|^2 partials; a no-op once `done` is raised
  mode 2  one schur32 application of the mixed even-odd BiCGStab: both hops, the inverse clover blocks on the hop sums, <z, out>, |out|^2, <z2, out>

Fields: against the fp64 oracle at the site-wise bound of tests/f32_bound.py (K_ASSERT; S(n) extended as written at each check).
Sums: against the same sums formed on the host in fp64 from the DOWNLOADED device field (and the fp32-representable z the test uploads), so only the
summation is judged.  Bound: gamma_c = c u / (1 - c u), c = fp32 additions on the path of a partial before it becomes a double; counted from the kernels:

  site-pair kernel (stencil_pair32.hip pair_wave)       3 components x (re, im) fmas per lane slot, then doubles                      c = 6
  direction-split, folded twin (stencil.hip emit)       3 components x 2 fmas per thread, the wave's sum rounded back to float        c = 7
  persistent direction-split                            double accumulator                                                            c <= 7
  site-per-lane Wilson kernel                           12 components x 2 fmas per thread, then doubles                               c = 24
  staggered site-per-lane kernel                        3 components x 2 fmas per thread, then doubles                                c = 6
  staggered direction-split kernel, folded twin         1 component x 2 fmas per thread, the wave's sum rounded back to float         c = 3
  dot epilogue (both kernels)                           3 components x 2 fmas per thread for each of Re, Im and |.|^2, then doubles   c = 6

Positive sums: relative error <= gamma_c.  Signed sums: |error| <= gamma_c sum |z||out|.
Partitioned lattice without the folded launch: the interior kernel sums |old|^2 of its incomplete result (c = 7), the exterior kernel adds per site
sum_j (|new_j|^2 - |old_j|^2) in fp32: 12 accumulations, 6 roundings inside a term, 1 for the wave's sum (c = 19) on magnitudes |new|^2 + |old|^2, so
|error| <= u (26 sum |old|^2 + 19 sum |new|^2); old = the result without the hops across the partitioned faces (the oracle with boundary sign 0 there)."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import f32_bound as fb

pytestmark = pytest.mark.gpu

KAPPA, CSW = 0.141139, 1.5612
BC = (1, -1, 1, -1)
ODD_L, BIG = (6, 6, 4, 2), (16, 8, 8, 4)
INTERIOR, DIRSPLIT, PIPE, PAIR = 0, 1, 2, 3
C_ADDS = {("wilson", INTERIOR): 24, ("wilson", DIRSPLIT): 7, ("wilson", PIPE): 7, ("wilson", PAIR): 6, ("clover", DIRSPLIT): 7,
          ("staggered", INTERIOR): 6, ("staggered", DIRSPLIT): 3}      # (K_ASSERT key, form)
BASE = {"dslash_variant": 1, "gauge_recon": 12, "dslash_pipe": 2, "mixed_pair32": 1, "mixed_links16": 0}


def gamma(c):
    return c * fb.U_ROUND / (1.0 - c * fb.U_ROUND)


def f32(a):
    return a.astype(np.complex64).astype(np.complex128)


def stencil_f32(lq, D, dst, src, inp, z, z2, dagger, mode, coef=0.0, done=0, conj=0, soa=0):
    sums = (C.c_double * 5)()
    h = lambda f: f._h if f is not None else None
    lq.lib.check(lq.lib.lib().lqcd_bench_stencil_f32(D._h, dst._h, h(src), inp._h, h(z), h(z2), int(dagger), int(mode), C.c_double(coef), int(done), int(conj),
                                                     int(soa), sums))
    return list(sums)


@pytest.fixture(scope="module")
def gpu(lq):
    assert lq.lib.device_count() > 0, "no HIP device visible: the product has no CPU fallback"
    return lq


def make(lq, orc, L, kind, tun, comm=False):
    """(lattice, links, operator, oracle application(psi, dagger[, bc]), S(n) of one application, component axes, field kind)"""
    lat = lq.Lattice(L)
    if comm:
        lat.comm_init(lq.comm_unique_id())
    for k, v in dict(BASE, **tun).items():
        lat.set_param(k, v)
    Uh = orc.hot_gauge(L, 71)
    U = lq.Gaugefields(lat).upload(Uh)
    if kind == "staggered":
        D = lq.Dirac_operator(U, None, {"Dirac_operator": "Staggered", "mass": 0.01, "boundarycondition": BC})
        ref = lambda v, dag, bc=BC: orc.staggered_D(Uh, v, L, 0.01, bc, dag)
        scale = lambda v: fb.site_scale(v, 0.01, 0.5, 1.0, fb.S_AXES)
        return lat, U, D, ref, scale, fb.S_AXES, lq.STAGGERED
    r = 0.7 if kind == "wilson-r0.7" else 1.0
    if kind == "clover":
        A = orc.clover_build(Uh, L, KAPPA, CSW)
        D = lq.Dirac_operator(U, None, {"Dirac_operator": "WilsonClover", "κ": KAPPA, "Clover_coefficient": CSW, "boundarycondition": BC})
        ref = lambda v, dag, bc=BC: orc.wilson_clover_D(Uh, A, v, L, KAPPA, 1.0, bc, dag)
        d = np.sqrt((np.abs(A) ** 2).sum(axis=(-1, -2)))
        scale = lambda v: fb.site_scale(v, 1.0, KAPPA, 2.0, fb.W_AXES, d)
    else:
        D = lq.Dirac_operator(U, None, {"Dirac_operator": "Wilson", "κ": KAPPA, "r": r, "boundarycondition": BC})
        ref = lambda v, dag, bc=BC: orc.wilson_D(Uh, v, L, KAPPA, r, bc, dag)
        scale = lambda v: fb.site_scale(v, 1.0, KAPPA, 1.0 + r, fb.W_AXES)
    return lat, U, D, ref, scale, fb.W_AXES, lq.WILSON


CASES = [
    # (operator, lattice, tunables, form, K_ASSERT key)
    ("wilson", BIG, {}, PAIR, "wilson"),
    ("wilson", BIG, {"mixed_pair32": 0}, DIRSPLIT, "wilson"),
    ("wilson", BIG, {"mixed_pair32": 0, "dslash_pipe": 1, "pipe_grid": 8, "pipe_min_chunks": 1}, PIPE, "wilson"),
    ("wilson", ODD_L, {}, DIRSPLIT, "wilson"),
    ("wilson", ODD_L, {"dslash_variant": 0}, INTERIOR, "wilson"),
    ("wilson-r0.7", ODD_L, {}, INTERIOR, "wilson"),
    ("clover", ODD_L, {}, DIRSPLIT, "clover"),
    ("clover", BIG, {"gauge_recon": 18}, DIRSPLIT, "clover"),
    ("staggered", ODD_L, {}, DIRSPLIT, "staggered"),
    ("staggered", BIG, {"stag_both": 1}, DIRSPLIT, "staggered"),
    ("staggered", ODD_L, {"dslash_variant": 0}, INTERIOR, "staggered"),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s-%s" % (c[0], "x".join(map(str, c[1])), ",".join("%s=%d" % kv for kv in c[2].items()) or "default"))
def test_norm_partials_of_the_plain_and_the_update_launch(gpu, orc, case):
    lq = gpu
    kind, L, tun, form, kkey = case
    lat, U, D, ref, scale, axes, fk = make(lq, orc, L, kind, tun)
    shape = lat.fermion_shape(fk)
    ph, sh = orc.gaussian_spinor(shape, 72), orc.gaussian_spinor(shape, 73)
    new = lambda hst: lq.Fermionfields(lat, fk).upload(hst)
    p, s, dst = new(ph), new(sh), new(np.zeros_like(ph))
    c = C_ADDS[(kkey, form)]
    # mode 0: dst = D p, sum of the |dst|^2 partials
    n2 = stencil_f32(lq, D, dst, None, p, None, None, 0, 0)[0]
    assert lat.get_param("f32_form_active") == form
    out = dst.download()
    K = fb.site_K(out, ref(ph, False), scale(ph), axes)
    host = float((np.abs(out) ** 2).sum())
    print("%s %s mode 0: K %.3f, |sum - host| / host = %.2e (bound %.2e)" % (kind, L, K, abs(n2 - host) / host, gamma(c)))
    assert K <= fb.K_ASSERT[kkey]
    assert abs(n2 - host) <= gamma(c) * host
    # mode 1: dst = s - coef D^+ p.  S(n) = ||s(n)|| + |coef| S_D(n): the rounding of s, of the result, and coef times the error of D^+ p
    coef = 0.37
    n2 = stencil_f32(lq, D, dst, s, p, None, None, 1, 1, coef=coef)[0]
    assert lat.get_param("f32_form_active") == form
    out = dst.download()
    S1 = fb.site_norm(sh, axes) + coef * scale(ph)
    K = fb.site_K(out, sh - coef * ref(ph, True), S1, axes)
    host = float((np.abs(out) ** 2).sum())
    print("%s %s mode 1: K %.3f, |sum - host| / host = %.2e (bound %.2e)" % (kind, L, K, abs(n2 - host) / host, gamma(c)))
    assert K <= fb.K_ASSERT[kkey]
    assert abs(n2 - host) <= gamma(c) * host
    # done raised: the launch leaves the residual alone -- dst is s rounded to fp32, bit for bit
    stencil_f32(lq, D, dst, s, p, None, None, 1, 1, coef=coef, done=1)
    assert np.array_equal(dst.download(), f32(sh))
    assert lat.get_param("mixed_handoffs") == 0 and lat.get_param("mixed_fp64_iters") == 0      # (no solve ran: the keys are untouched)


def even_mask(L):
    t, z, y, x = np.meshgrid(np.arange(L[3]), np.arange(L[2]), np.arange(L[1]), np.arange(L[0]), indexing="ij")
    return ((x + y + z + t) & 1) == 0


def nb_sum(a):
    return sum(np.roll(a, 1, axis=ax) + np.roll(a, -1, axis=ax) for ax in range(4))


@pytest.mark.parametrize("kind,tun,form", [("wilson", {}, PAIR), ("wilson", {"mixed_pair32": 0}, DIRSPLIT), ("clover", {}, DIRSPLIT), ("clover", {"gauge_recon": 18}, DIRSPLIT)],
                         ids=["wilson-pair", "wilson-one-site", "clover-12", "clover-18"])
def test_schur_application_and_its_inner_products(gpu, orc, kind, tun, form):
    """out_e = in_e - k^2 [A^-1] H_eo [A^-1] H_oe in_e.  S(n) = ||in(n)|| + k^2 a(n) h sum_{+-mu} [ ||t(n+-mu)|| + S_t(n+-mu) ], t = [A^-1] H_oe in,
    S_t(m) = a(m) h sum_{+-nu} ||in(m+-nu)||, a = ||A^-1||_2 (1 without a clover term), h = 2: the second hop's own roundings, and the first hop's error
    (<= K u S_t) carried through the second."""
    lq = gpu
    L = BIG
    lat, U, D, _, _, axes, fk = make(lq, orc, L, kind, tun)
    Uh = orc.hot_gauge(L, 71)
    ev = even_mask(L)
    shape = lat.fermion_shape(fk)
    inh, zh, z2h = (f32(orc.gaussian_spinor(shape, sd)) for sd in (74, 75, 76))
    new = lambda hst: lq.Fermionfields(lat, fk).upload(hst)
    fin, fz, fz2, dst = new(inh), new(zh), new(z2h), new(np.zeros_like(inh))
    if kind == "clover":
        Ai = orc.clover_invert(orc.clover_build(Uh, L, KAPPA, CSW), L)
        a = np.linalg.norm(Ai, 2, axis=(-2, -1))
        def ainv(v):
            v12 = np.moveaxis(v, 0, -2).reshape(v.shape[1:5] + (12,))
            return np.ascontiguousarray(np.moveaxis(np.einsum("...ij,...j->...i", Ai, v12).reshape(v.shape[1:5] + (4, 3)), -2, 0))
    else:
        a = np.ones(ev.shape)
        ainv = lambda v: v
    ine = inh * ev[None, ..., None]
    worst = 0.0
    for dag in (0, 1):
        t = ainv(orc.wilson_hop_parity(Uh, np.ascontiguousarray(ine), L, 1.0, BC, bool(dag), 1))
        ref = ine - KAPPA ** 2 * ainv(orc.wilson_hop_parity(Uh, t, L, 1.0, BC, bool(dag), 0))
        St = a * 2.0 * nb_sum(fb.site_norm(ine, axes))
        S = fb.site_norm(ine, axes) + KAPPA ** 2 * a * 2.0 * nb_sum(fb.site_norm(t, axes) + St * (~ev))
        for soa in (0, 1):
            for conj in (0, 1):
                for fzz, zhh, z2 in ((fz, zh, None), (fin, inh, None), (fin, inh, fz2)):      # z2 rides only where z is the input: the <s, t>, |t|^2, <r0, t> launch
                    sums = stencil_f32(lq, D, dst, None, fin, fzz, z2, dag, 2, conj=conj, soa=soa)
                    assert lat.get_param("f32_form_active") == form and lat.get_param("pair32_active") == (1 if form == PAIR else 0)
                    out = dst.download() * ev[None, ..., None]
                    e = fb.site_norm(out - ref, axes)
                    K = float((e[ev] / (fb.U_ROUND * S[ev])).max())
                    worst = max(worst, K)
                    assert K <= fb.K_ASSERT[kind], (dag, soa, conj, K)
                    ze = zhh * ev[None, ..., None]
                    d1 = np.vdot(out, ze) if conj else np.vdot(ze, out)
                    mag = float((np.abs(ze) * np.abs(out)).sum())
                    host_n = float((np.abs(out) ** 2).sum())
                    assert abs(sums[0] - d1.real) <= gamma(6) * mag and abs(sums[1] - d1.imag) <= gamma(6) * mag, (dag, soa, conj, sums, d1)
                    assert abs(sums[2] - host_n) <= gamma(6) * host_n, (dag, soa, conj)
                    if z2 is not None:
                        z2e = z2h * ev[None, ..., None]
                        d2 = np.vdot(z2e, out)
                        mag2 = float((np.abs(z2e) * np.abs(out)).sum())
                        assert abs(sums[3] - d2.real) <= gamma(6) * mag2 and abs(sums[4] - d2.imag) <= gamma(6) * mag2, (dag, soa, conj, sums, d2)
    print("schur32 %s %s: worst K %.3f" % (kind, tun, worst))


def test_schur_mode_is_refused_where_the_fused_chain_does_not_run(gpu, orc):
    lq = gpu
    lat, U, D, _, _, axes, fk = make(lq, orc, ODD_L, "wilson", {})      # 144 sites per parity: not whole chunks
    f = [lq.Fermionfields(lat, fk).upload(orc.gaussian_spinor(lat.fermion_shape(fk), sd)) for sd in (74, 75, 76)]
    with pytest.raises(lq.LQCDError, match="mode 2 needs"):
        stencil_f32(lq, D, f[2], None, f[0], f[1], None, 0, 2)


PART_CODE = """
    import os, sys, ctypes as C, numpy as np
    sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
    import latticeqcd_jl_amd as lq
    from oracle import oracle as orc
    import f32_bound as fb
    import test_gpu_f32_epilogues as te
    L, mask = (8, 4, 6, 8), int(os.environ["LQCD_FORCE_PARTITION"])
    n = 0
    for kind, kkey in (("wilson", "wilson"), ("clover", "clover"), ("staggered", "staggered")):
        lat, U, D, ref, scale, axes, fk = te.make(lq, orc, L, kind, {}, comm=True)
        shape = lat.fermion_shape(fk)
        ph, sh = orc.gaussian_spinor(shape, 72), orc.gaussian_spinor(shape, 73)
        new = lambda hst: lq.Fermionfields(lat, fk).upload(hst)
        p, s, dst = new(ph), new(sh), new(np.zeros_like(ph))
        bc0 = tuple(0 if (mask >> mu) & 1 else te.BC[mu] for mu in range(4))      # no hop across a partitioned face: what the interior kernel leaves
        for fold in (1, 0):
            lat.set_param("halo_fold", fold)
            for mode, dag, coef in ((0, 0, 0.0), (1, 1, 0.37)):
                n2 = te.stencil_f32(lq, D, dst, s if mode else None, p, None, None, dag, mode, coef=coef)[0]
                form, fa = lat.get_param("f32_form_active"), lat.get_param("halo_fold_active")
                assert form == (4 if fold else 9) and fa == fold, (kind, fold, mode, form, fa)
                out = dst.download()
                if mode == 0:
                    want, old, S = ref(ph, False), ref(ph, False, bc0), scale(ph)
                else:
                    want, old, S = sh - coef * ref(ph, True), sh - coef * ref(ph, True, bc0), fb.site_norm(sh, axes) + coef * scale(ph)
                K = fb.site_K(out, want, S, axes)
                host = float((np.abs(out) ** 2).sum())
                bound = te.gamma(te.C_ADDS[(kkey, 1)]) * host if fold else fb.U_ROUND * (26.0 * float((np.abs(old) ** 2).sum()) + 19.0 * host)
                print("%s fold %d mode %d: K %.3f, |sum - host| = %.3e (bound %.3e)" % (kind, fold, mode, K, abs(n2 - host), bound))
                assert K <= fb.K_ASSERT[kkey], (kind, fold, mode, K)
                assert abs(n2 - host) <= bound, (kind, fold, mode, n2, host)
                n += 1
    print("F32_EPILOGUE_PARTITIONED_OK", n)
"""


def test_partitioned_launches_sum_interior_partials_and_exterior_corrections(gpu):
    """every direction partitioned on (8,4,6,8), a world-size-1 RCCL communicator: the folded launch (complete partials) and interior + exterior"""
    env = dict(os.environ, LQCD_FORCE_PARTITION="15", HSA_ENABLE_IPC_MODE_LEGACY="0", LQCD_HALO_STREAM_MODE="3")
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(PART_CODE)], capture_output=True, text=True, env=env, timeout=300,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print(r.stdout[-4000:])
    assert r.returncode == 0 and "F32_EPILOGUE_PARTITIONED_OK 12" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
