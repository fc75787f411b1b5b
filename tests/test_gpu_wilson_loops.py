"""The R x T Wilson loops on the device (lqcd_gauge_wilson_loops; the reference's Wilson_loop measurement, src/measurements/measure_Wilsonloop.jl:71-126)
against the numpy restatement (tests/wilsonloop_numpy.py, itself checked in tests/test_cpu_wilsonloop_restatement.py), against an abelian field with a
known table, under a gauge rotation, behind the lazy link recorder and behind the gradient flow; argument errors and the refusal on a partitioned lattice.

Tolerance of device against restatement: a loop is a product of at most 2 (R + T) <= 28 links here, every product good to a few eps, the entries are
averages of O(1) traces -- absolute 1e-13 (the Polyakov loop test holds 1e-14 for products of 4-10 links)."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import flow_numpy as fn
import wilsonloop_numpy as wn
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
TOL = 1e-13


@pytest.fixture(scope="module")
def gpu():
    import latticeqcd_jl_amd as lq
    if lq.lib.device_count() < 1:
        pytest.skip("no HIP device")
    return lq


CASES = {        # name -> (L, Rmax, Tmax)
    "ildg": ((4, 4, 4, 4), 4, 4),               # every loop with R = 4 or T = 4 wraps the lattice
    "hot_tile": ((8, 16, 4, 4), 4, 4),          # the lattices of the flow test (chunks of whole x-rows / the generic form)
    "hot_generic": ((6, 4, 4, 4), 4, 4),
    "hot_all_differ": ((4, 6, 8, 10), 4, 10),   # four different extents: any mix-up of the axes shows
    "hot_8": ((8, 8, 8, 8), 7, 7),
}
_host = {}


def _field(lq, orc, case):
    """(L, host links, restatement table) of a case, computed once."""
    if case not in _host:
        L, Rmax, Tmax = CASES[case]
        Uh = lq.gauge_io.load_ildg(os.path.join(GOLDEN, "quenched_su3_4x4x4x4.ildg"), L) if case == "ildg" else orc.hot_gauge(L, 31)
        _host[case] = (L, Uh, wn.wilson_loops(Uh, L, Rmax, Tmax))
    return _host[case]


def _upload(lq, L, Uh):
    return lq.Gaugefields(lq.Lattice(L)).upload(Uh)


def _raw(lq, U, Rmax, Tmax, table):
    ptr = table.ctypes.data_as(C.POINTER(C.c_double)) if table is not None else None
    return lq.lib.lib().lqcd_gauge_wilson_loops(U._h, int(Rmax), int(Tmax), ptr)


@pytest.mark.parametrize("case", ["ildg", "hot_tile", "hot_generic", "hot_all_differ"])
def test_device_matches_the_restatement(gpu, orc, case):
    lq = gpu
    L, Uh, ref = _field(lq, orc, case)
    tab = lq.wilson_loops(_upload(lq, L, Uh), *CASES[case][1:])
    err = np.abs(tab - ref).max()
    print(case, "max |device - restatement| =", err)
    assert tab.shape == ref.shape and err < TOL
    if case == "ildg":
        assert abs(tab[0, 0] - 0.56878) < 1e-5


def test_cold_start_gives_one(gpu):
    lq = gpu
    U = lq.Initialize_Gaugefields(3, 0, 6, 4, 4, 8, condition="cold")
    tab = lq.wilson_loops(U, 4, 8)
    assert np.abs(tab - 1.0).max() <= 1e-15
    assert np.array_equal(lq.Wilson_loop_measurement(U).measure(U), tab[:4, :4])


def test_abelian_field_has_its_analytic_table(gpu, orc):
    lq = gpu
    tab = lq.wilson_loops(_upload(lq, wn.ABELIAN_L, wn.abelian_field()), 4, 5)
    err = np.abs(tab - wn.abelian_table(4, 5)).max()
    print("max |device - analytic| =", err)
    assert err < TOL


def test_gauge_rotation_on_the_host_changes_nothing(gpu, orc):
    lq = gpu
    L, Uh, ref = _field(lq, orc, "hot_all_differ")
    tab = lq.wilson_loops(_upload(lq, L, fn.gauge_transform(Uh, L, 77)), 4, 10)
    assert np.abs(tab - ref).max() < TOL


def test_hot_start_obeys_the_haar_bound(gpu, orc):
    """R, T <= 7 on 8^4: no loop wraps, sigma = 1 / sqrt(54 V); the bound is asserted on the restatement's numbers, then device = restatement."""
    lq = gpu
    L, Uh, ref = _field(lq, orc, "hot_8")
    assert np.abs(ref).max() < 5.0 * wn.haar_sigma(L)
    tab = lq.wilson_loops(_upload(lq, L, Uh), 7, 7)
    assert np.abs(tab - ref).max() < TOL


def test_two_calls_give_the_same_bits_and_leave_the_links_alone(gpu, orc):
    lq = gpu
    L, Uh, _ = _field(lq, orc, "hot_tile")
    U = _upload(lq, L, Uh)
    before = U.download()
    a = lq.wilson_loops(U, 4, 4)
    b = lq.wilson_loops(U, 4, 4)
    assert np.array_equal(a, b)
    small = lq.wilson_loops(U, 2, 3)                 # a smaller table in between reuses the context's buffers
    assert np.array_equal(small[:, :3], a[:2, :3]) and np.array_equal(lq.wilson_loops(U, 4, 4), a)
    assert np.array_equal(U.download(), before)


def test_calc_wilson_loop_takes_the_time_extent_first(gpu, orc):
    lq = gpu
    L, Uh, ref = _field(lq, orc, "hot_all_differ")
    U = _upload(lq, L, Uh)
    tab = lq.wilson_loops(U, 3, 3)
    w = lq.calc_Wilson_loop(U, 3, 2)                 # Lt = 3, Ls = 2
    assert w == lq.wilson_loops(U, 2, 3)[1, 2] and w == tab[1, 2]
    assert w != tab[2, 1] and abs(w - ref[1, 2]) < TOL


def test_recorded_link_update_is_flushed_first(gpu, orc):
    """One in-place per-direction link update waits in the recorder (exptU! -> mul! -> substitute_U! = one recorded lqcd_link_exp_mul); the loops are
    called before anything downloads the field and must see the updated links."""
    lq = gpu
    L, Uh, _ = _field(lq, orc, "hot_generic")
    U = _upload(lq, L, Uh)
    lat = U.lattice
    p = lq.initialize_TA_Gaugefields(U)
    lq.gauss_distribution_(p, 34)
    tmp = lq.Gaugefields(lat)
    lq.exptU_(tmp[1], 0.2, p[2])
    lq.mul_(tmp[2], tmp[1], U[2])
    lq.substitute_U_(U[2], tmp[2])
    assert len(lat._done) == 1
    tab = lq.wilson_loops(U, 4, 4)
    assert not lat._done
    after = U.download()
    assert np.abs(after[1] - Uh[1]).max() > 1e-3 and np.array_equal(after[0], Uh[0])
    assert np.abs(tab - wn.wilson_loops(after, L, 4, 4)).max() < TOL


def test_loops_behind_the_gradient_flow(gpu, orc):
    lq = gpu
    L, Uh, ref0 = _field(lq, orc, "ildg")
    U = _upload(lq, L, Uh)
    lq.flow_(U, lq.Gradientflow(U, Nflow=5, eps=0.02))
    tab = lq.wilson_loops(U, 4, 4)
    ref = wn.wilson_loops(fn.flow(Uh, L, 0.02, 5), L, 4, 4)
    assert np.abs(tab - ref).max() < 1e-12          # the flow test's own tolerance
    assert tab[0, 0] > ref0[0, 0]


def test_argument_errors_leave_the_table_untouched(gpu, orc):
    lq = gpu
    L, Uh, _ = _field(lq, orc, "hot_all_differ")      # (4, 6, 8, 10): min spatial extent 4, Lt = 10
    U = _upload(lq, L, Uh)
    for Rmax, Tmax in ((0, 2), (5, 2), (2, 11), (2, 0)):
        tab = np.full((max(Rmax, 1), max(Tmax, 1)), np.nan)
        assert _raw(lq, U, Rmax, Tmax, tab) == lq.lib.ERR_ARG
        assert np.isnan(tab).all()
    assert _raw(lq, U, 2, 2, None) == lq.lib.ERR_ARG
    tab = np.full((4, 10), np.nan)
    assert _raw(lq, U, 4, 10, tab) == lq.lib.OK and np.isfinite(tab).all()
    with pytest.raises(lq.LQCDError):
        lq.wilson_loops(U, 5, 2)


def test_partitioned_lattice_is_refused(gpu):
    code = textwrap.dedent("""
        import os, sys, ctypes as C, numpy as np
        sys.path.insert(0, os.getcwd())
        import latticeqcd_jl_amd as lq
        lat = lq.Lattice((8, 8, 8, 8))
        lat.comm_init(lq.comm_unique_id())
        U = lq.Initialize_Gaugefields(3, 0, 8, 8, 8, 8, condition="cold", lattice=lat)
        tab = np.full((2, 2), np.nan)
        st = lq.lib.lib().lqcd_gauge_wilson_loops(U._h, 2, 2, tab.ctypes.data_as(C.POINTER(C.c_double)))
        msg = lq.lib.lib().lqcd_last_error().decode()
        assert st == lq.lib.ERR_UNSUPPORTED and "partitioned" in msg, (st, msg)
        assert np.isnan(tab).all()
        print("WL_PARTITIONED_REFUSED")
    """)
    env = dict(os.environ, LQCD_FORCE_PARTITION="15", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120, cwd=ROOT)
    assert r.returncode == 0 and "WL_PARTITIONED_REFUSED" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
