"""The numpy restatement of the R x T Wilson loops (tests/wilsonloop_numpy.py), checked without reference to itself: against explicit path products,
against a constant abelian field with a known table, under gauge rotations and centre transformations, against the Haar variance of a hot start; and
the two host helpers of the Python layer (static_potential, creutz_ratios) on an exact area + perimeter law."""
import os

import numpy as np
import pytest

import flow_numpy as fn
import wilsonloop_numpy as wn
from conftest import GOLDEN


def _ildg(lq):
    L = (4, 4, 4, 4)
    return L, lq.gauge_io.load_ildg(os.path.join(GOLDEN, "quenched_su3_4x4x4x4.ildg"), L)


def test_restatement_equals_the_explicit_path_products(orc, lq):
    L, U = _ildg(lq)
    Um = orc._mat(U)
    tab = wn.wilson_loops(U, L, 4, 4)
    V = float(np.prod(L))
    worst = 0.0
    for R in range(1, 5):
        for T in range(1, 5):
            s = 0.0
            for mu in range(3):
                P = fn.loop(Um, [(mu, +1)] * R + [(3, +1)] * T + [(mu, -1)] * R + [(3, -1)] * T)
                s += float(np.trace(P, axis1=-2, axis2=-1).real.sum())
            worst = max(worst, abs(tab[R - 1, T - 1] - s / (9.0 * V)))
    print("max |restatement - explicit paths| =", worst)
    assert worst < 1e-14
    # W(1, 1) is the plaquette of the three space-time planes only
    assert abs(tab[0, 0] - 0.56878) < 1e-5 and abs(orc.plaquette(U, L) - 0.56822) < 1e-5


def test_abelian_constant_field_has_its_analytic_table(orc):
    tab = wn.wilson_loops(wn.abelian_field(), wn.ABELIAN_L, 4, 5)
    err = np.abs(tab - wn.abelian_table(4, 5)).max()
    print("max |restatement - analytic| =", err)
    assert err < 1e-14


def test_unit_gauge_gives_one(orc):
    L = (4, 6, 4, 6)
    assert np.abs(wn.wilson_loops(orc.unit_gauge(L), L, 4, 6) - 1.0).max() < 1e-15


def test_a_random_gauge_rotation_changes_nothing(orc):
    L = (4, 6, 4, 6)
    U = orc.hot_gauge(L, 41)
    a, b = wn.wilson_loops(U, L, 4, 6), wn.wilson_loops(fn.gauge_transform(U, L, 42), L, 4, 6)
    assert np.abs(a - b).max() < 1e-13


def test_a_centre_element_on_one_time_slice_changes_nothing_but_the_polyakov_loop(orc):
    L = (4, 4, 6, 6)
    U = orc.hot_gauge(L, 43)
    Uz = U.copy()
    Uz[3, 2] *= np.exp(2j * np.pi / 3.0)
    assert np.abs(wn.wilson_loops(U, L, 4, 6) - wn.wilson_loops(Uz, L, 4, 6)).max() < 1e-13
    p, pz = orc.polyakov_loop(U, L), orc.polyakov_loop(Uz, L)
    assert abs(pz - np.exp(2j * np.pi / 3.0) * p) < 1e-14 and abs(pz - p) > 1e-3 * abs(p)


@pytest.mark.parametrize("L", [(8, 8, 8, 8), (6, 4, 4, 4), (8, 16, 4, 4), (4, 6, 8, 10)])
def test_hot_start_entries_stay_inside_five_sigma(orc, L):
    """R < min spatial extent and T < Lt: distinct loops are distinct sets of links, Re tr / 3 has variance 1/18, sigma = 1 / sqrt(54 V).  (R = L or T = L is
    kept out: there the loops of neighbouring sites coincide and the entries are far larger.)"""
    Rmax, Tmax = min(L[:3]) - 1, L[3] - 1
    sig = wn.haar_sigma(L)
    for seed in (31, 32, 33):
        tab = wn.wilson_loops(orc.hot_gauge(L, seed), L, Rmax, Tmax)
        print(L, seed, "max |W| / sigma =", np.abs(tab).max() / sig, "rms / sigma =", np.sqrt((tab ** 2).mean()) / sig)
        assert np.abs(tab).max() < 5.0 * sig


def test_host_helpers_on_an_area_and_perimeter_law(lq):
    sigma, mu = 0.21, 0.13
    R, T = np.meshgrid(np.arange(1, 6), np.arange(1, 8), indexing="ij")
    W = np.exp(-sigma * R * T - 2.0 * mu * (R + T))
    chi = lq.creutz_ratios(W)
    pot = lq.static_potential(W)
    assert chi.shape == (4, 6) and pot.shape == (5, 6)
    assert np.abs(chi - sigma).max() < 1e-13
    assert np.abs(pot - (sigma * R[:, :-1] + 2.0 * mu)).max() < 1e-13
    # a ratio that is not positive gives NaN, and only there
    W2 = W.copy()
    W2[2, 3] = -W2[2, 3]
    chi2, pot2 = lq.creutz_ratios(W2), lq.static_potential(W2)
    assert np.isnan(pot2[2, 2]) and np.isnan(pot2[2, 3]) and np.isfinite(np.delete(pot2.ravel(), [2 * 6 + 2, 2 * 6 + 3])).all()
    bad = np.isnan(chi2)
    assert bad.sum() == 4 and bad[1, 2] and bad[1, 3] and bad[2, 2] and bad[2, 3]
    W3 = W.copy()
    W3[1, 1] = 0.0
    assert np.isnan(lq.static_potential(W3)[1, 0]) and np.isnan(lq.static_potential(W3)[1, 1])
