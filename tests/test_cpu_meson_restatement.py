"""The numpy restatement of the meson correlators (tests/meson_numpy.py), checked without reference to itself: channel 15 against sum |S|^2, the rho against
the expression of the literature test, the imaginary parts, the free-field pion against a momentum-space inverse, a gauge rotation and a translation of
the field together with its source.  Propagators come from the CPU even-odd BiCGStab (the plain BiCGStab breaks down on a point source on the golden
configuration)."""
import os

import numpy as np
import pytest

import flow_numpy as fn
import meson_numpy as mn
from conftest import GOLDEN

KAPPA = 0.125


def point_columns(orc, U, L, kappa, src=(0, 0, 0, 0), eps=1e-19):
    """The 12 columns cols[4 b + beta] for a point source at src = (x, y, z, t)."""
    cols = []
    for b in range(3):
        for be in range(4):
            rhs = np.zeros(orc.wilson_shape(L), dtype=np.complex128)
            rhs[be, src[3], src[2], src[1], src[0], b] = 1.0
            x, _, _, st = orc.wilson_bicgstab_eo(U, rhs, L, kappa, eps=eps)
            assert st == 0
            cols.append(x)
    return np.stack(cols)


@pytest.fixture(scope="module")
def golden(orc, lq):
    L = (4, 4, 4, 4)
    U = lq.gauge_io.load_ildg(os.path.join(GOLDEN, "quenched_su3_4x4x4x4.ildg"), L)
    cols = point_columns(orc, U, L, KAPPA)
    re, im = mn.contract(cols, L[3], imag=True)
    return L, U, cols, re, im


def test_gamma_15_is_gamma_5(orc):
    assert np.abs(mn.gamma_n(15) - orc.GAMMA[4]).max() == 0.0
    for n in range(16):     # every channel matrix is a phased permutation
        G = mn.gamma_n(n)
        assert (np.abs(G) > 0).sum() == 4 and np.abs(G @ G.conj().T - np.eye(4)).max() == 0.0


def test_channel_15_is_the_squared_modulus(golden):
    L, U, cols, re, im = golden
    pion = sum(mn.norm2_timeslices(c) for c in cols)
    err = np.abs(re[15] - pion).max() / pion.max()
    print("max |C_15 - sum |S|^2| / max =", err)
    assert err < 1e-14


def test_rho_equals_the_expression_of_the_literature_test(golden):
    L, U, cols, re, im = golden
    rho = re[1] + re[2] + re[4]
    err = np.abs(rho - mn.rho_literature(cols)).max() / re[15].max()
    print("max |C_1 + C_2 + C_4 - rho| / C_15 =", err)
    assert err < 1e-14


def test_imaginary_parts_vanish_and_channels_are_bounded_by_the_pion(golden):
    L, U, cols, re, im = golden
    print("max |Im| / C_15 =", (np.abs(im) / re[15]).max(), " min |C_n| / C_15 =", (np.abs(re) / re[15]).min())
    assert (np.abs(im) < 1e-15 * re[15]).all()
    assert (np.abs(re) <= re[15] * (1 + 1e-14)).all()       # Cauchy-Schwarz


def test_free_field_pion_equals_the_momentum_space_formula(orc):
    L, kappa = (4, 4, 6, 8), 0.11
    cols = point_columns(orc, orc.unit_gauge(L), L, kappa, eps=1e-26)
    C = mn.contract(cols, L[3])[15]
    F = mn.free_pion(L, kappa)
    err = np.abs(C - F).max() / F.max()
    print("free field: max |C_15 - formula| / max =", err)
    assert err < 1e-12


def test_a_gauge_rotation_changes_nothing(orc, golden):
    L, U, cols, re, im = golden
    re2 = mn.contract(point_columns(orc, fn.gauge_transform(U, L, 71), L, KAPPA, eps=1e-26), L[3])
    ref = mn.contract(point_columns(orc, U, L, KAPPA, eps=1e-26), L[3])
    err = (np.abs(re2 - ref) / ref[15]).max()
    print("gauge rotation: max |dC| / C_15 =", err)
    assert err < 1e-11


def test_moving_the_source_with_the_field_moves_the_table(orc, golden):
    """U'(x) = U(x - d) and the source at d: S'(x) = +-S(x - d) (the sign from the antiperiodic boundary drops out of S ... S^+), so C'_n(t) = C_n(t - d_t)."""
    L, U, cols, re, im = golden
    d = (1, 2, 3, 1)
    Ud = np.ascontiguousarray(np.roll(U, shift=(d[3], d[2], d[1], d[0]), axis=(1, 2, 3, 4)))
    re2 = mn.contract(point_columns(orc, Ud, L, KAPPA, src=d, eps=1e-26), L[3])
    ref = mn.contract(point_columns(orc, U, L, KAPPA, eps=1e-26), L[3])
    err = (np.abs(re2 - np.roll(ref, d[3], axis=1)) / np.roll(ref[15], d[3])).max()
    print("translation: max |dC| / C_15 =", err)
    assert err < 1e-11
    assert (np.abs(re2 - ref) / ref[15]).max() > 1e-3       # and it is not the unmoved table
