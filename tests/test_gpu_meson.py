"""Meson correlators on the device (include/lqcd_hip.h "meson correlators", csrc/meson.hip) against the numpy restatement (tests/meson_numpy.py, itself checked in
tests/test_cpu_meson_restatement.py) and the CPU solvers; the time-slice norm; reproducibility; argument errors and refusals; partitioned lattices; and the
chiral condensate measurement against a numpy loop over the same noise vectors.

Tolerances.  Contraction of uploaded columns: 144 terms per site and channel and a sum over V_3 sites, rounding about (144 + log2 V_3) eps ~ 2e-14 of
sum |terms| <= C_15(t) (Cauchy-Schwarz): 1e-13 C_15(t) per entry.  End to end: moving the CPU solver's eps from 1e-19 to 1e-26 shifts the table by at most
1.4e-10 C_15 at kappa = 0.125 on the golden configuration: 1e-8 C_15(t)."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import meson_numpy as mn
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
TOL_CONTRACT = 1e-13
TOL_SOLVE = 1e-8
KAPPA = 0.125
LATTICES = [(4, 4, 4, 4),      # half a 64-site chunk per time slice and parity
            (6, 4, 4, 8),      # 48 sites per slice: irregular straddling of the chunks
            (4, 6, 8, 10),     # four different extents, 96 sites per slice
            (8, 8, 8, 8)]      # whole chunks


@pytest.fixture(scope="module")
def gpu():
    import latticeqcd_jl_amd as lq
    if lq.lib.device_count() < 1:
        pytest.skip("no HIP device")
    return lq


_cache = {}


def _gauss(orc, L):
    """12 Gaussian Wilson columns of a lattice and their restatement table, computed once."""
    if ("g", L) not in _cache:
        cols = np.stack([orc.gaussian_spinor(orc.wilson_shape(L), 200 + j) for j in range(12)])
        _cache["g", L] = (cols, mn.contract(cols, L[3]))
    return _cache["g", L]


def _golden_links(lq):
    L = (4, 4, 4, 4)
    return L, lq.gauge_io.load_ildg(os.path.join(GOLDEN, "quenched_su3_4x4x4x4.ildg"), L)


def _point_columns(solve, L, src):
    cols = []
    for b in range(3):
        for be in range(4):
            rhs = np.zeros((4, L[3], L[2], L[1], L[0], 3), dtype=np.complex128)
            rhs[be, src[3], src[2], src[1], src[0], b] = 1.0
            x, _, _, st = solve(rhs)
            assert st == 0
            cols.append(x)
    return np.stack(cols)


def _wilson_ref(orc, key, U, L, kappa, src=(0, 0, 0, 0)):
    if key not in _cache:
        _cache[key] = mn.contract(_point_columns(lambda b: orc.wilson_bicgstab_eo(U, b, L, kappa, eps=1e-19), L, src), L[3])
    return _cache[key]


def _wilson(lq, U, kappa, **kw):
    p = {"Dirac_operator": "Wilson", "κ": kappa, "r": 1.0, "eps_CG": 1e-19, "MaxCGstep": 3000, "method_CG": "bicgstab_evenodd"}
    p.update(kw)
    return lq.Dirac_operator(U, None, p)


def _upload(lq, L, Uh):
    return lq.Gaugefields(lq.Lattice(L)).upload(Uh)


def _rel(tab, ref):
    """max over the entries of |tab - ref| / C_15(t)"""
    return float((np.abs(tab - ref) / ref[15]).max())


def _ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


# ---------------------------------------------------------------------------------- the contraction alone
@pytest.mark.parametrize("L", LATTICES, ids=lambda L: "x".join(map(str, L)))
def test_contract_equals_the_restatement(gpu, orc, L):
    lq = gpu
    cols, ref = _gauss(orc, L)
    lat = lq.Lattice(L)
    f = [lq.Fermionfields(lat, lq.WILSON).upload(c) for c in cols]
    tab = lq.meson_contract(f)
    err = _rel(tab, ref)
    print(L, "12 columns: max |device - restatement| / C_15 =", err)
    assert tab.shape == (16, L[3]) and err < TOL_CONTRACT
    parts = []
    for n in (4, 8):
        t = lq.meson_contract(f[:n])
        e = _rel(t, mn.contract(cols[:n], L[3]))
        print(L, n, "columns:", e)
        assert e < TOL_CONTRACT
    for b in range(3):
        parts.append(lq.meson_contract(f[4 * b:4 * b + 4]))
    e = _rel(parts[0] + parts[1] + parts[2], tab)
    print(L, "sum of three 4-column calls against the 12-column call:", e)
    assert e < TOL_CONTRACT
    # channel 15 is the squared modulus
    pion = sum(lq.norm2_timeslices(x) for x in f)
    assert np.abs(tab[15] - pion).max() < TOL_CONTRACT * pion.max()


@pytest.mark.parametrize("L", LATTICES, ids=lambda L: "x".join(map(str, L)))
def test_norm2_timeslices(gpu, orc, L):
    lq = gpu
    lat = lq.Lattice(L)
    for kind, shape in ((lq.WILSON, orc.wilson_shape(L)), (lq.STAGGERED, orc.staggered_shape(L))):
        psi = orc.gaussian_spinor(shape, 301)
        x = lq.Fermionfields(lat, kind).upload(psi)
        out, ref = lq.norm2_timeslices(x), mn.norm2_timeslices(psi)
        err = np.abs(out / ref - 1.0).max()
        n2 = C.c_double(0)
        lq.check(lq.lib.lib().lqcd_norm2(x._h, C.byref(n2)))
        print(L, kind, "max rel err =", err, " sum over t against lqcd_norm2:", abs(out.sum() / n2.value - 1.0))
        assert out.shape == (L[3],) and err < 1e-13
        assert abs(out.sum() / n2.value - 1.0) < 1e-13


# ---------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("src", [(0, 0, 0, 0), (1, 2, 3, 1)], ids=["origin", "src1231"])
def test_wilson_correlators_equal_the_cpu_solves(gpu, orc, src):
    lq = gpu
    L, Uh = _golden_links(lq)
    ref = _wilson_ref(orc, ("w", src), Uh, L, KAPPA, src)
    U = _upload(lq, L, Uh)
    D = _wilson(lq, U, KAPPA)
    tab, its = lq.meson_correlators(D, src, return_info=True)
    err = _rel(tab, ref)
    print("source", src, "max |device - cpu| / C_15 =", err, "iterations", its)
    assert err < TOL_SOLVE and len(its) == 12 and min(its) > 0
    pion = lq.pion_correlator(D, src)
    assert np.array_equal(pion, tab[15])


def test_clover_correlators_equal_the_cpu_solves(gpu, orc):
    lq = gpu
    L, Uh = _golden_links(lq)
    A = orc.clover_build(Uh, L, KAPPA, 1.0)
    ref = mn.contract(_point_columns(lambda b: orc.wilson_clover_bicgstab_eo(Uh, A, b, L, KAPPA, eps=1e-19), L, (0, 0, 0, 0)), L[3])
    U = _upload(lq, L, Uh)
    D = _wilson(lq, U, KAPPA, Dirac_operator="WilsonClover", Clover_coefficient=1.0)
    tab = lq.meson_correlators(D)
    err = _rel(tab, ref)
    print("clover: max |device - cpu| / C_15 =", err)
    assert err < TOL_SOLVE
    assert _rel(tab, _wilson_ref(orc, ("w", (0, 0, 0, 0)), Uh, L, KAPPA)) > 1e-3      # and the clover term is in it
    assert np.array_equal(lq.pion_correlator(D), tab[15])


def test_staggered_pion_equals_the_cpu_solves(gpu, orc):
    lq = gpu
    L = (4, 4, 4, 4)
    Uh = lq.gauge_io.load_ildg(os.path.join(GOLDEN, "staggered_4x4x4x4.ildg"), L)
    mass, src = 0.1, (1, 0, 2, 3)
    ref = np.zeros(L[3])
    for ic in range(3):
        b = np.zeros(orc.staggered_shape(L), dtype=np.complex128)
        b[src[3], src[2], src[1], src[0], ic] = 1.0
        y, _, _, st = orc.cg_DdagD(orc.STAGGERED, Uh, b, L, mass, eps=1e-19)
        assert st == 0
        ref += mn.norm2_timeslices(orc.staggered_D(Uh, y, L, mass, dagger=True))
    U = _upload(lq, L, Uh)
    D = lq.Dirac_operator(U, None, {"Dirac_operator": "staggered", "mass": mass, "eps_CG": 1e-19, "MaxCGstep": 3000})
    Cpi, its = lq.pion_correlator(D, src, return_info=True)
    err = np.abs(Cpi / ref - 1.0).max()
    print("staggered pion: max rel err =", err, "iterations", its)
    assert err < TOL_SOLVE and len(its) == 3
    m = lq.Pion_correlator_measurement(U, fermiontype="Staggered", mass=mass, eps_CG=1e-19, src=src)
    assert np.array_equal(m.measure(U), Cpi)


def test_free_field_pion_equals_the_momentum_space_formula(gpu):
    lq = gpu
    L, kappa = (4, 4, 6, 8), 0.11
    U = lq.Initialize_Gaugefields(3, 0, *L, condition="cold", lattice=lq.Lattice(L))
    tab = lq.meson_correlators(_wilson(lq, U, kappa))
    F = mn.free_pion(L, kappa)
    err = np.abs(tab[15] / F - 1.0).max()
    print("free field: max |C_15 / formula - 1| =", err)
    assert err < TOL_SOLVE
    m = lq.Pion_correlator_measurement(U, fermiontype="Wilson", κ=kappa, eps_CG=1e-19)
    assert np.abs(m.measure(U) / F - 1.0).max() < TOL_SOLVE


# ---------------------------------------------------------------------------------- reproducibility
def test_two_calls_give_the_same_bits_and_the_links_stay(gpu, orc):
    lq = gpu
    L = (6, 4, 4, 8)
    Uh = orc.hot_gauge(L, 31)
    U = _upload(lq, L, Uh)
    before = U.download()
    D = _wilson(lq, U, 0.1)
    a = lq.meson_correlators(D, (1, 0, 3, 5))
    # a smaller lattice's call in between
    Ls, Us = _golden_links(lq)
    small = lq.meson_correlators(_wilson(lq, _upload(lq, Ls, Us), KAPPA))
    b = lq.meson_correlators(D, (1, 0, 3, 5))
    assert np.array_equal(a, b) and np.isfinite(a).all() and (a[15] > 0).all()
    assert np.array_equal(U.download(), before)
    assert _rel(small, _wilson_ref(orc, ("w", (0, 0, 0, 0)), Us, Ls, KAPPA)) < TOL_SOLVE
    cols, _ = _gauss(orc, L)
    lat = lq.Lattice(L)
    f = [lq.Fermionfields(lat, lq.WILSON).upload(c) for c in cols]
    assert np.array_equal(lq.meson_contract(f), lq.meson_contract(f))
    assert np.array_equal(lq.norm2_timeslices(f[0]), lq.norm2_timeslices(f[0]))


# ---------------------------------------------------------------------------------- argument errors and refusals
def test_argument_errors_and_refusals_leave_the_outputs_untouched(gpu, orc):
    lq = gpu
    f = lq.lib.lib()
    L = (4, 4, 4, 4)
    _, Uh = _golden_links(lq)
    lat = lq.Lattice(L)
    U = lq.Gaugefields(lat).upload(Uh)
    D = _wilson(lq, U, KAPPA)
    tab = np.full((16, 4), np.nan)
    its = (C.c_int * 12)(*([-7] * 12))
    eps = C.c_double(1e-19)

    def untouched():
        return np.isnan(tab).all() and all(v == -7 for v in its)

    cols = [lq.Fermionfields(lat, lq.WILSON) for _ in range(12)]
    arr = (C.c_void_p * 12)(*[c._h for c in cols])
    # null pointers and a bad ncol
    assert f.lqcd_meson_contract(None, 12, _ptr(tab)) == 1
    assert f.lqcd_meson_contract(arr, 12, None) == 1
    for n in (0, 3, 5, 13, 16, -4):
        assert f.lqcd_meson_contract(arr, n, _ptr(tab)) == 1
    hole = (C.c_void_p * 4)(cols[0]._h, None, cols[2]._h, cols[3]._h)
    assert f.lqcd_meson_contract(hole, 4, _ptr(tab)) == 1
    # mixed contexts, kinds, subsets
    other = lq.Fermionfields(lq.Lattice(L), lq.WILSON)
    stag = lq.Fermionfields(lat, lq.STAGGERED)
    half = lq.Fermionfields(lat, lq.WILSON, lq.EVEN)
    for bad in (other, stag, half):
        mixed = (C.c_void_p * 4)(cols[0]._h, cols[1]._h, bad._h, cols[3]._h)
        assert f.lqcd_meson_contract(mixed, 4, _ptr(tab)) == 1
    assert f.lqcd_spinor_norm2_timeslices(None, _ptr(tab)) == 1
    assert f.lqcd_spinor_norm2_timeslices(cols[0]._h, None) == 1
    assert f.lqcd_spinor_norm2_timeslices(half._h, _ptr(tab)) == 1
    # the measurement: null pointers, a source outside the lattice
    for fn in (f.lqcd_meson_correlators, f.lqcd_pion_correlator):
        assert fn(None, lq.lib.i4((0, 0, 0, 0)), eps, 100, _ptr(tab), its) == 1
        assert fn(D._h, None, eps, 100, _ptr(tab), its) == 1
        assert fn(D._h, lq.lib.i4((0, 0, 0, 0)), eps, 100, None, its) == 1
        for src in ((4, 0, 0, 0), (0, -1, 0, 0), (0, 0, 0, 4)):
            assert fn(D._h, lq.lib.i4(src), eps, 100, _ptr(tab), its) == 1
    assert untouched()
    # a solve that does not converge
    for fn in (f.lqcd_meson_correlators, f.lqcd_pion_correlator):
        assert fn(D._h, lq.lib.i4((0, 0, 0, 0)), eps, 2, _ptr(tab), its) == 3
    assert untouched()
    # refusals: a staggered operator in the 16-channel entry, a Domainwall operator
    Ds = lq.Dirac_operator(U, None, {"Dirac_operator": "staggered", "mass": 0.1})
    assert f.lqcd_meson_correlators(Ds._h, lq.lib.i4((0, 0, 0, 0)), eps, 100, _ptr(tab), its) == 5
    assert "staggered" in f.lqcd_last_error().decode()
    Ddw = lq.Dirac_operator(U, None, {"Dirac_operator": "Domainwall", "mass": 0.25, "M": -1.0, "L5": 2})
    for fn in (f.lqcd_meson_correlators, f.lqcd_pion_correlator):
        assert fn(Ddw._h, lq.lib.i4((0, 0, 0, 0)), eps, 100, _ptr(tab), its) == 5
        assert "Domainwall" in f.lqcd_last_error().decode()
    assert untouched()
    with pytest.raises(lq.LQCDError) as e:
        lq.Pion_correlator_measurement(U, fermiontype="Domainwall")
    assert e.value.code == 5
    # an in-process PE grid
    gL, pe = (4, 4, 4, 8), (1, 1, 1, 2)
    lats = [lq.Lattice(gL, pe, r) for r in range(2)]
    lq.link_local(lats)
    Ug = lq.Gaugefields(lats[0])
    Dg = _wilson(lq, Ug, KAPPA)
    tab8 = np.full((16, 8), np.nan)
    assert f.lqcd_meson_correlators(Dg._h, lq.lib.i4((0, 0, 0, 0)), eps, 100, _ptr(tab8), its) == 5
    assert "PE grid" in f.lqcd_last_error().decode()
    xg = [lq.Fermionfields(lats[0], lq.WILSON) for _ in range(4)]
    assert f.lqcd_meson_contract((C.c_void_p * 4)(*[x._h for x in xg]), 4, _ptr(tab8)) == 5
    assert f.lqcd_spinor_norm2_timeslices(xg[0]._h, _ptr(tab8)) == 5
    assert np.isnan(tab8).all() and untouched()


# ---------------------------------------------------------------------------------- partitioned lattices
PART_L = (4, 4, 4, 8)


def _partition_reference(lq, orc, path):
    """The single-domain tables of the partitioned tests, saved for the worker processes."""
    Uh = orc.hot_gauge(PART_L, 111)
    U = _upload(lq, PART_L, Uh)
    tab = lq.meson_correlators(_wilson(lq, U, KAPPA), (1, 2, 3, 5))
    cols, ctab = _gauss(orc, PART_L)
    np.savez(path, tab=tab, ctab=ctab)


def test_partitioned_rccl_self_partition_matches_the_single_domain(gpu, orc, tmp_path):
    lq = gpu
    ref = os.path.join(str(tmp_path), "single.npz")
    _partition_reference(lq, orc, ref)
    code = textwrap.dedent(f"""
        import os, sys, numpy as np
        sys.path.insert(0, os.getcwd())
        import latticeqcd_jl_amd as lq
        from oracle import oracle as orc
        L = {PART_L!r}
        r = np.load({ref!r})
        lat = lq.Lattice(L)
        lat.comm_init(lq.comm_unique_id())
        U = lq.Gaugefields(lat).upload(orc.hot_gauge(L, 111))
        D = lq.Dirac_operator(U, None, {{"Dirac_operator": "Wilson", "κ": {KAPPA}, "eps_CG": 1e-19, "method_CG": "bicgstab_evenodd"}})
        tab = lq.meson_correlators(D, (1, 2, 3, 5))
        err = float((np.abs(tab - r["tab"]) / r["tab"][15]).max())
        f = [lq.Fermionfields(lat, lq.WILSON).upload(orc.gaussian_spinor(orc.wilson_shape(L), 200 + j)) for j in range(12)]
        cerr = float((np.abs(lq.meson_contract(f) - r["ctab"]) / r["ctab"][15]).max())
        assert err < {TOL_SOLVE} and cerr < {TOL_CONTRACT}, (err, cerr)
        print("RCCL_SELF_MESON_OK", err, cerr)
    """)
    env = dict(os.environ, LQCD_FORCE_PARTITION="15", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120, cwd=ROOT)
    assert r.returncode == 0 and "RCCL_SELF_MESON_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    print(r.stdout[-300:])


@pytest.mark.parametrize("pe,port", [((1, 1, 1, 2), 29812), ((1, 1, 2, 1), 29813)], ids=["t2", "z2"])
def test_partitioned_peer_two_processes_match_the_single_domain(gpu, orc, tmp_path, pe, port):
    lq = gpu
    ref = os.path.join(str(tmp_path), "single.npz")
    _partition_reference(lq, orc, ref)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2",
               MESON_TEST_LATTICE=",".join(map(str, PART_L)), MESON_TEST_PE=",".join(map(str, pe)), MESON_TEST_REF=ref)
    env.pop("LQCD_FORCE_PARTITION", None)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "tests", "meson_peer_worker.py")],
                       capture_output=True, text=True, env=env, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-5000:]
    for k in range(2):
        assert f"MESON_PEER_OK rank {k}" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ---------------------------------------------------------------------------------- the chiral condensate
def test_chiral_condensate_equals_a_numpy_loop_over_the_same_noise(gpu, orc):
    lq = gpu
    L = (4, 4, 4, 4)
    Uh = lq.gauge_io.load_ildg(os.path.join(GOLDEN, "staggered_4x4x4x4.ildg"), L)
    U = _upload(lq, L, Uh)
    mass, Nr, seed = 0.1, 3, 500
    m = lq.Chiral_condensate_measurement(U, fermiontype="Staggered", mass=mass, Nf=2, Nr=Nr, eps_CG=1e-19, randomseed=seed)
    val = m.measure(U)
    r = lq.Fermionfields(U.lattice, lq.STAGGERED)
    s = 0.0
    for ir in range(Nr):
        lq.Z4_distribution_fermi_(r, seed + ir)
        eta = r.download()
        assert np.abs(np.abs(eta) - 1.0).max() < 1e-15
        y, _, _, st = orc.cg_DdagD(orc.STAGGERED, Uh, eta, L, mass, eps=1e-19)
        assert st == 0
        s += np.vdot(eta, orc.staggered_D(Uh, y, L, mass, dagger=True))
    ref = (s / Nr).real / float(np.prod(L)) * (2 / 4.0)
    print("chiral condensate:", val, "numpy:", ref, "rel", abs(val / ref - 1.0))
    assert abs(val / ref - 1.0) < TOL_SOLVE
