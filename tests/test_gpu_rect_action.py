"""The plaquette + rectangle gauge action on the device (lqcd_gauge_rectangle, lqcd_gauge_action_improved, lqcd_gauge_force_improved,
lqcd_momentum_add_gauge_force_improved, lqcd_link_staple_improved and their Python mirror) against the numpy restatement (tests/rect_numpy.py, itself checked in
tests/test_cpu_rect_restatement.py): values, force, fused momentum update, the per-direction triple, the hand-over to the plaquette entries at beta_rect = 0,
finite differences, a quenched Luscher-Weisz trajectory, repeatability, argument errors, the refusal on a partitioned lattice and the extent-2 decision.

Tolerances.  Rectangle and action: averages / sums of O(1) traces of 6-link products, 1e-13 absolute on the mean and 1e-13 relative on the action (the Polyakov
and Wilson-loop tests hold 1e-14 / 1e-13 for comparable products).  Force: max |G_dev - G_ref| < 1e-13 max |G_ref|: 24 products of at most five links with
weights |beta_plaq| <= 21, |beta_rect| <= 1.9, each good to a few 2^-52.  An extent of 2 is computed, not refused (csrc/rectangle.hip header): (4,4,2,2) runs
through the same checks."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import rect_numpy as rn
from conftest import GOLDEN, ROOT, rel_err

pytestmark = pytest.mark.gpu

BETA = 5.7
LW = rn.lw(BETA)
IWASAKI = rn.c1_action(BETA, -0.331)
COEFS = {"lw": LW, "iwasaki": IWASAKI}
CASES = {
    "ildg": (4, 4, 4, 4),            # every 2-long side is half the extent
    "hot_generic": (6, 4, 4, 4),     # odd half-width, the generic chunk form
    "hot_tile": (8, 16, 4, 4),       # whole-row chunks and the tile map
    "hot_all_differ": (4, 6, 8, 10), # any axis mix-up shows
    "hot_extent2": (4, 4, 2, 2),     # a 2-long side closes on itself
}
ALL = list(CASES)
_host = {}


@pytest.fixture(scope="module")
def gpu(lq):
    assert lq.lib.device_count() > 0, "no HIP device visible: the product has no CPU fallback"
    return lq


class Ref:
    """host links of a case and the restatement's numbers, computed once and never changed"""

    def __init__(self, L, Uh):
        self.L, self.Uh = L, Uh
        self.rect, self.plaq = rn.rectangle(Uh, L), rn.plaquette(Uh, L)
        self.Gp, self.Gr = rn.force(Uh, L, 1.0, 0.0), rn.force(Uh, L, 0.0, 1.0)      # the force is linear in the two coefficients
        for a in (self.Uh, self.Gp, self.Gr):
            a.setflags(write=False)

    def action(self, bp, br):
        V = float(np.prod(self.L))
        return -bp * 6.0 * V * self.plaq - br * 12.0 * V * self.rect

    def force(self, bp, br):
        return bp * self.Gp + br * self.Gr


def _ref(lq, orc, case):
    if case not in _host:
        L = CASES[case]
        Uh = lq.gauge_io.load_ildg(os.path.join(GOLDEN, "quenched_su3_4x4x4x4.ildg"), L) if case == "ildg" else orc.hot_gauge(L, 31)
        _host[case] = Ref(L, np.ascontiguousarray(Uh))
    return _host[case]


def _upload(lq, L, Uh, lat=None):
    return lq.Gaugefields(lat if lat is not None else lq.Lattice(L)).upload(Uh)


def _d(x):
    return C.c_double(x)


def _action(lq, U, bp, br):
    s = C.c_double(float("nan"))
    st = lq.lib.lib().lqcd_gauge_action_improved(U._h, _d(bp), _d(br), C.byref(s))
    assert st == lq.lib.OK, lq.lib.lib().lqcd_last_error()
    return s.value


# ---------------------------------------------------------------- 1. rectangle, action
@pytest.mark.parametrize("case", ALL)
def test_rectangle_and_action_match_the_restatement(gpu, orc, case):
    lq = gpu
    ref = _ref(lq, orc, case)
    U = _upload(lq, ref.L, ref.Uh)
    r = lq.calculate_Rectangle(U)
    print(case, "rectangle", r, "restatement", ref.rect, "diff", abs(r - ref.rect))
    assert abs(r - ref.rect) < 1e-13
    assert abs(lq.calculate_Plaquette(U) - ref.plaq) < 1e-13
    for name, (bp, br) in COEFS.items():
        s, s_ref = _action(lq, U, bp, br), ref.action(bp, br)
        print(case, name, "S", s, "restatement", s_ref, "rel", abs(s - s_ref) / abs(s_ref))
        assert abs(s - s_ref) < 1e-13 * abs(s_ref)
        assert lq.evaluate_GaugeAction(U, bp, beta_rect=br) == s
        assert abs(s - rn.action(ref.Uh, ref.L, bp, br)) < 1e-13 * abs(s_ref)


def test_cold_start_gives_exactly_one(gpu):
    lq = gpu
    for L in ((6, 4, 4, 8), (4, 4, 2, 2)):
        U = lq.Initialize_Gaugefields(3, 0, *L, condition="cold")
        assert lq.calculate_Rectangle(U) == 1.0
        V = float(np.prod(L))
        assert abs(_action(lq, U, *LW) - (-6.0 * V * LW[0] - 12.0 * V * LW[1])) < 1e-13 * V
        G = lq.Gaugefields(U.lattice)
        lq.gauge_force_(G, U, *LW)
        Gh = rn.to_xyzt(G.download())
        assert np.abs(rn.ta(Gh)).max() < 1e-15 and abs(Gh[0, 0, 0, 0, 0, 0, 0] + (LW[0] * 6 + LW[1] * 18) / 6.0) < 1e-14


# ---------------------------------------------------------------- 2. force
@pytest.mark.parametrize("coef", list(COEFS))
@pytest.mark.parametrize("case", ALL)
def test_force_matches_the_restatement(gpu, orc, case, coef):
    lq = gpu
    ref = _ref(lq, orc, case)
    bp, br = COEFS[coef]
    U = _upload(lq, ref.L, ref.Uh)
    G = lq.Gaugefields(U.lattice)
    lq.gauge_force_(G, U, bp, beta_rect=br)
    Gref = ref.force(bp, br)
    err = np.abs(G.download() - Gref).max() / np.abs(Gref).max()
    print(case, coef, "max |G_dev - G_ref| / max |G_ref| =", err)
    assert err < 1e-13
    if case == "hot_generic":       # and the restatement's linearity shortcut is the enumerated force
        assert rel_err(rn.force(ref.Uh, ref.L, bp, br), Gref) < 1e-14


@pytest.mark.parametrize("case", ["hot_generic", "hot_tile", "hot_extent2"])
def test_force_on_two_row_and_on_eighteen_real_loads(gpu, orc, case):
    lq = gpu
    ref = _ref(lq, orc, case)
    L = ref.L
    lat = lq.Lattice(L)
    assert lat.get_param("staple_recon") == 1
    U = _upload(lq, L, ref.Uh, lat)
    lq.reunitarize_(U)                                   # every link projected: the field is tracked as unitary, the sweep loads two rows
    Uh = U.download()
    assert np.abs(Uh - ref.Uh).max() < 1e-14
    G = lq.Gaugefields(lat)
    lq.gauge_force_(G, U, *LW)
    Gref = rn.force(Uh, L, *LW)
    e2 = np.abs(G.download() - Gref).max() / np.abs(Gref).max()
    # one link off the group, reconstruction switched off: all 18 reals of every link are loaded
    Us = Uh.copy()
    Us[2, 1, 0, 1, 1] *= 1.01
    lat.set_param("staple_recon", 0)
    U.upload(Us)
    lq.gauge_force_(G, U, *LW)
    Gref18 = rn.force(Us, L, *LW)
    e18 = np.abs(G.download() - Gref18).max() / np.abs(Gref18).max()
    print(case, "two-row", e2, "18-real", e18)
    assert e2 < 1e-13 and e18 < 1e-13
    assert np.abs(Gref18 - Gref).max() > 1e-3


# ---------------------------------------------------------------- 3. fused momentum update, per-direction triple
@pytest.mark.parametrize("case", ["ildg", "hot_generic", "hot_tile", "hot_all_differ", "hot_extent2"])
def test_fused_momentum_update_and_the_triples(gpu, orc, case):
    lq = gpu
    ref = _ref(lq, orc, case)
    L = ref.L
    bp, br = LW
    lat = lq.Lattice(L)
    U = _upload(lq, L, ref.Uh, lat)
    Ph = orc.gaussian_momenta(L, 302)
    P1, P2, G = lq.Gaugefields(lat).upload(Ph), lq.Gaugefields(lat).upload(Ph), lq.Gaugefields(lat)
    lq.gauge_force_(G, U, bp, beta_rect=br)
    lq.Traceless_antihermitian_add_(P1, -0.37, G)
    lq.P_update_(U, P2, -0.37, bp, beta_rect=br)
    p1 = P1.download()
    assert rel_err(P2.download(), p1) < 1e-13
    assert np.abs(p1 - Ph).max() > 0.1
    # against the restatement as well: P + factor TA(G_ref)
    want = rn.to_host(rn.to_xyzt(Ph) - 0.37 * rn.ta(rn.to_xyzt(ref.force(bp, br))))
    assert rel_err(p1, want) < 1e-13
    # calc_dSdUmu! -> mul! -> Traceless_antihermitian_add!, the reference's P_update! (factor = -eps dtau / NC ... here: the same momenta)
    ga = lq.GaugeAction(U)
    ga.push_(bp / 2, lq.make_loops_fromname("plaquette") + lq.make_loops_fromname("plaquette", adjoint=True))
    ga.push_(br / 2, lq.make_loops_fromname("rectangular") + lq.make_loops_fromname("rectangular", adjoint=True))
    assert ga.beta == bp and ga.beta_rect == br
    for lazy in (0, 1):
        lat.set_param("lazy_links", lazy)
        P3 = lq.Gaugefields(lat).upload(Ph)
        tmp = lq.Gaugefields(lat)
        for mu in range(1, 5):
            lq.calc_dSdUmu_(tmp[1], ga, mu, U)
            lq.mul_(tmp[2], U[mu], tmp[1])
            lq.Traceless_antihermitian_add_(P3[mu], 0.37 / 3.0, tmp[2])      # (beta/2) staples against -(beta/6): factor -1/3
        assert rel_err(P3.download(), p1) < 1e-13, lazy
    St = tmp.download()[0]
    assert rel_err(St, rn.link_staple(ref.Uh, L, 3, bp, br)) < 1e-13


# ---------------------------------------------------------------- 4. beta_rect = 0 is today's plaquette path, bit for bit
@pytest.mark.parametrize("case", ["ildg", "hot_tile"])
def test_beta_rect_zero_hands_over_to_the_plaquette_entries(gpu, orc, case):
    lq = gpu
    lib = lq.lib.lib()
    ref = _ref(lq, orc, case)
    L = ref.L
    lat = lq.Lattice(L)
    U = _upload(lq, L, ref.Uh, lat)
    if case == "hot_tile":
        lq.reunitarize_(U)
    s = C.c_double(0)
    assert lib.lqcd_gauge_action(U._h, _d(BETA), C.byref(s)) == 0
    assert _action(lq, U, BETA, 0.0) == s.value
    Ga, Gb = lq.Gaugefields(lat), lq.Gaugefields(lat)
    assert lib.lqcd_gauge_force(Ga._h, U._h, _d(BETA)) == 0 and lib.lqcd_gauge_force_improved(Gb._h, U._h, _d(BETA), _d(0.0)) == 0
    assert np.array_equal(Ga.download(), Gb.download())
    Ph = orc.gaussian_momenta(L, 303)
    Pa, Pb = lq.Gaugefields(lat).upload(Ph), lq.Gaugefields(lat).upload(Ph)
    assert lib.lqcd_momentum_add_gauge_force(Pa._h, _d(0.21), U._h, _d(BETA)) == 0
    assert lib.lqcd_momentum_add_gauge_force_improved(Pb._h, _d(0.21), U._h, _d(BETA), _d(0.0)) == 0
    pa = Pa.download()
    assert np.array_equal(pa, Pb.download()) and np.abs(pa - Ph).max() > 0.01
    for mu in range(4):
        assert lib.lqcd_link_staple(Ga._h, 1, U._h, mu, _d(BETA)) == 0 and lib.lqcd_link_staple_improved(Gb._h, 1, U._h, mu, _d(BETA), _d(0.0)) == 0
        assert np.array_equal(Ga.download()[1], Gb.download()[1])


# ---------------------------------------------------------------- 5. finite differences on the device
@pytest.mark.parametrize("case,coef", [("ildg", "lw"), ("ildg", "iwasaki"), ("hot_extent2", "lw")])
def test_device_force_is_the_derivative_of_the_device_action(gpu, orc, case, coef):
    """The rotations and the bound of tests/test_cpu_rect_restatement.py: central difference at eps = 1e-4 against -2 Im tr(T G), 1e-6 max(1, |dS/d eps|)."""
    lq = gpu
    L = CASES[case]
    Uh = orc.hot_gauge(L, 811)
    bp, br = COEFS[coef]
    U = _upload(lq, L, Uh)
    G = lq.Gaugefields(U.lattice)
    lq.gauge_force_(G, U, bp, beta_rect=br)
    Gh = G.download()
    eps = 1e-4
    for site, mu, T in rn.fd_rotations(L):
        sp = _action(lq, U.upload(rn.rotate_link(Uh, site, mu, T, eps)), bp, br)
        sm = _action(lq, U.upload(rn.rotate_link(Uh, site, mu, T, -eps)), bp, br)
        d, pred = (sp - sm) / (2.0 * eps), rn.fd_prediction(Gh, site, mu, T)
        print(case, coef, site, mu, "dS/deps", d, "-2 Im tr(T G)", pred)
        assert abs(d - pred) < 1e-6 * max(1.0, abs(d))


# ---------------------------------------------------------------- 6. a quenched Luscher-Weisz trajectory
def test_luescher_weisz_trajectory_is_second_order_and_reversible(gpu, orc):
    """QPQ leapfrog of length 1 at beta = 5.7 on the reference's thermalised 4^4 configuration, through the Python mirror.  A wrong relative weight between the
    plaquette and the rectangle part of the force leaves a dH that does not fall like dtau^2 (bounds of tests/test_gpu_md.py)."""
    lq = gpu
    L = CASES["ildg"]
    Uh = _ref(lq, orc, "ildg").Uh
    lat = lq.Lattice(L)
    U, p = lq.Gaugefields(lat), lq.Gaugefields(lat)
    ga = lq.GaugeAction(U)
    ga.push_(LW[0] / 2, lq.make_loops_fromname("plaquette") + lq.make_loops_fromname("plaquette", adjoint=True))
    ga.push_(LW[1] / 2, lq.make_loops_fromname("rectangular") + lq.make_loops_fromname("rectangular", adjoint=True))

    def H():
        return lq.momentum_action(p) + lq.evaluate_GaugeAction(ga, U) / -3.0

    def run(nsteps):
        dt = 1.0 / nsteps
        for _ in range(nsteps):
            lq.U_update_(U, p, 0.5 * dt)
            lq.P_update_(U, p, dt, ga)
            lq.U_update_(U, p, 0.5 * dt)

    dH = []
    for nsteps in (20, 40):
        U.upload(Uh)
        lq.gauss_distribution_(p, 401)
        H0 = H()
        run(nsteps)
        dH.append(H() - H0)
    print("Luscher-Weisz leapfrog: H0 =", H0, "dH(20) =", dH[0], "dH(40) =", dH[1], "ratio", dH[0] / dH[1])
    assert abs(lq.evaluate_GaugeAction(ga, U) / -3.0 - _action(lq, U, *LW)) < 1e-14 * abs(H0)
    assert abs(dH[1]) < abs(dH[0]) and 3.0 < abs(dH[0] / dH[1]) < 5.0
    # reversibility: flip the momenta, integrate back (the 40-step trajectory)
    H1 = H()
    p.upload(-p.download())
    run(40)
    back = np.abs(U.download() - Uh).max()
    print("reversibility: max |U - U0| =", back, "|H - H0| / H0 =", abs(H() - H0) / abs(H0))
    assert back < 1e-10 and abs(H() - H0) < 1e-8 * abs(H0) and abs(H1 - H0) > 1e-8 * abs(H0)


# ---------------------------------------------------------------- 7. repeatability, the recorder
def _all_entries(lq, U, P0):
    """every entry once: (rectangle, action, force, momenta, staple slots)"""
    lat = U.lattice
    G, P, S = lq.Gaugefields(lat), lq.Gaugefields(lat).upload(P0), lq.Gaugefields(lat)
    r, s = lq.calculate_Rectangle(U), _action(lq, U, *LW)
    lq.gauge_force_(G, U, *LW)
    lq.P_update_(U, P, 0.3, *LW)
    for mu in range(4):
        assert lq.lib.lib().lqcd_link_staple_improved(S._h, mu, U._h, mu, _d(LW[0]), _d(LW[1])) == 0
    return r, s, G.download(), P.download(), S.download()


@pytest.mark.parametrize("case", ["hot_tile", "hot_generic"])
def test_two_calls_give_the_same_bits_and_leave_the_links_alone(gpu, orc, case):
    lq = gpu
    ref = _ref(lq, orc, case)
    U = _upload(lq, ref.L, ref.Uh)
    P0 = orc.gaussian_momenta(ref.L, 304)
    a, b = _all_entries(lq, U, P0), _all_entries(lq, U, P0)
    assert a[0] == b[0] and a[1] == b[1]
    for x, y in zip(a[2:], b[2:]):
        assert np.array_equal(x, y) and np.isfinite(x).all()
    assert np.array_equal(U.download(), ref.Uh)


def test_recorded_link_update_is_flushed_first(gpu, orc):
    """One in-place per-direction link update waits in the recorder (exptU! -> mul! -> substitute_U!); every entry is called before anything downloads the
    field and must see the updated links."""
    lq = gpu
    ref = _ref(lq, orc, "hot_generic")
    L = ref.L
    P0 = orc.gaussian_momenta(L, 305)

    def recorded():
        U = _upload(lq, L, ref.Uh)
        lat = U.lattice
        p = lq.initialize_TA_Gaugefields(U)
        lq.gauss_distribution_(p, 34)
        tmp = lq.Gaugefields(lat)
        out = lq.Gaugefields(lat).upload(np.zeros_like(P0))      # before the update is recorded: an upload runs what is recorded
        lq.exptU_(tmp[1], 0.2, p[2])
        lq.mul_(tmp[2], tmp[1], U[2])
        lq.substitute_U_(U[2], tmp[2])
        assert len(lat._done) == 1
        return U, lat, out, (tmp, p)      # the fields of the recorded update stay alive: destroying one would run it

    U, lat, out, _t = recorded()
    r = lq.calculate_Rectangle(U)
    assert not lat._done
    after = U.download()
    assert np.abs(after[1] - ref.Uh[1]).max() > 1e-3 and np.array_equal(after[0], ref.Uh[0])
    assert abs(r - rn.rectangle(after, L)) < 1e-13
    Gref = rn.force(after, L, *LW)
    lib = lq.lib.lib()
    calls = {
        "action": lambda U, o: lib.lqcd_gauge_action_improved(U._h, _d(LW[0]), _d(LW[1]), C.byref(C.c_double(0))),
        "force": lambda U, o: lib.lqcd_gauge_force_improved(o._h, U._h, _d(LW[0]), _d(LW[1])),
        "update": lambda U, o: lib.lqcd_momentum_add_gauge_force_improved(o._h, _d(1.0), U._h, _d(LW[0]), _d(LW[1])),
        "staple": lambda U, o: lib.lqcd_link_staple_improved(o._h, 0, U._h, 1, _d(LW[0]), _d(LW[1])),
    }
    for name, call in calls.items():
        U, lat, out, _t = recorded()
        assert call(U, out) == 0 and not lat._done, name
        assert np.array_equal(U.download(), after), name
        if name == "force":
            assert rel_err(out.download(), Gref) < 1e-13
        if name == "update":
            assert rel_err(out.download(), rn.to_host(rn.ta(rn.to_xyzt(Gref)))) < 1e-13
        if name == "staple":
            assert rel_err(out.download()[0], rn.link_staple(after, L, 1, *LW)) < 1e-13


# ---------------------------------------------------------------- 8. argument errors
def test_argument_errors_leave_the_outputs_untouched(gpu, orc):
    lq = gpu
    lib = lq.lib.lib()
    ref = _ref(lq, orc, "hot_generic")
    L = ref.L
    lat, lat2 = lq.Lattice(L), lq.Lattice(L)
    U, U2 = _upload(lq, L, ref.Uh, lat), _upload(lq, L, ref.Uh, lat2)
    nan = np.full(lat.gauge_shape, np.nan + 1j * np.nan)
    out, out2 = lq.Gaugefields(lat).upload(nan), lq.Gaugefields(lat2).upload(nan)
    ARG = lq.lib.ERR_ARG
    bp, br = _d(LW[0]), _d(LW[1])
    r = C.c_double(float("nan"))
    assert lib.lqcd_gauge_rectangle(None, C.byref(r)) == ARG and lib.lqcd_gauge_rectangle(U._h, None) == ARG
    assert lib.lqcd_gauge_action_improved(None, bp, br, C.byref(r)) == ARG and lib.lqcd_gauge_action_improved(U._h, bp, br, None) == ARG
    assert np.isnan(r.value)
    for zero in (br, _d(0.0)):        # the hand-over checks the same arguments
        assert lib.lqcd_gauge_force_improved(None, U._h, bp, zero) == ARG and lib.lqcd_gauge_force_improved(out._h, None, bp, zero) == ARG
        assert lib.lqcd_gauge_force_improved(out2._h, U._h, bp, zero) == ARG          # two contexts
        assert lib.lqcd_gauge_force_improved(U._h, U._h, bp, zero) == ARG             # out == U
        assert lib.lqcd_momentum_add_gauge_force_improved(None, _d(1.0), U._h, bp, zero) == ARG
        assert lib.lqcd_momentum_add_gauge_force_improved(out._h, _d(1.0), None, bp, zero) == ARG
        assert lib.lqcd_momentum_add_gauge_force_improved(out2._h, _d(1.0), U._h, bp, zero) == ARG
        assert lib.lqcd_momentum_add_gauge_force_improved(U._h, _d(1.0), U._h, bp, zero) == ARG
        assert lib.lqcd_link_staple_improved(None, 0, U._h, 0, bp, zero) == ARG and lib.lqcd_link_staple_improved(out._h, 0, None, 0, bp, zero) == ARG
        assert lib.lqcd_link_staple_improved(out2._h, 0, U._h, 0, bp, zero) == ARG
        assert lib.lqcd_link_staple_improved(U._h, 0, U._h, 1, bp, zero) == ARG
        for mo, mu in ((4, 0), (-1, 0), (0, 4), (0, -1)):
            assert lib.lqcd_link_staple_improved(out._h, mo, U._h, mu, bp, zero) == ARG
    assert np.isnan(out.download()).all() and np.isnan(out2.download()).all()
    assert np.array_equal(U.download(), ref.Uh) and np.array_equal(U2.download(), ref.Uh)
    with pytest.raises(lq.LQCDError):
        lq.gauge_force_(U, U, *LW)
    # and the Python mirror still refuses every other loop set
    ga = lq.GaugeAction(U)
    with pytest.raises(lq.LQCDError):
        lq.make_loops_fromname("chair")
    with pytest.raises(lq.LQCDError):
        ga.push_(1.0, lq.make_loops_fromname("plaquette"))
    with pytest.raises(lq.LQCDError):
        ga.push_(1.0, lq.make_loops_fromname("rectangular"))
    assert len(lq.make_loops_fromname("rectangular")) == 12 and ga.beta == 0.0 and ga.beta_rect == 0.0
    assert lib.lqcd_gauge_force_improved(out._h, U._h, bp, br) == 0 and np.isfinite(out.download()).all()


# ---------------------------------------------------------------- 9. refusal on a partitioned lattice
def test_partitioned_lattice_is_refused(gpu):
    code = textwrap.dedent("""
        import os, sys, ctypes as C, numpy as np
        sys.path.insert(0, os.getcwd())
        import latticeqcd_jl_amd as lq
        lat = lq.Lattice((8, 8, 8, 8))
        lat.comm_init(lq.comm_unique_id())
        U = lq.Initialize_Gaugefields(3, 0, 8, 8, 8, 8, condition="cold", lattice=lat)
        out = lq.Initialize_Gaugefields(3, 0, 8, 8, 8, 8, condition="cold", lattice=lat)
        before = out.download()
        lib = lq.lib.lib()
        d = C.c_double
        r = d(float("nan"))
        calls = [lambda br: lib.lqcd_gauge_rectangle(U._h, C.byref(r)),
                 lambda br: lib.lqcd_gauge_action_improved(U._h, d(9.5), d(br), C.byref(r)),
                 lambda br: lib.lqcd_gauge_force_improved(out._h, U._h, d(9.5), d(br)),
                 lambda br: lib.lqcd_momentum_add_gauge_force_improved(out._h, d(1.0), U._h, d(9.5), d(br)),
                 lambda br: lib.lqcd_link_staple_improved(out._h, 0, U._h, 1, d(9.5), d(br))]
        for call in calls:
            for br in (-0.475, 0.0):
                st = call(br)
                msg = lib.lqcd_last_error().decode()
                assert st == lq.lib.ERR_UNSUPPORTED and "partitioned" in msg, (st, msg)
        assert np.isnan(r.value) and np.array_equal(out.download(), before)
        print("RECT_PARTITIONED_REFUSED")
    """)
    env = dict(os.environ, LQCD_FORCE_PARTITION="15", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120, cwd=ROOT)
    assert r.returncode == 0 and "RECT_PARTITIONED_REFUSED" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
