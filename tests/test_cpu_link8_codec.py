"""The 8-real SU(3) chart of the temporal-gauge CG (tests/link8_numpy.py, the numpy restatement of csrc/lqcd_internal.h link8_decode and csrc/fields.hip
tgauge8_encode): decode(encode(U)) against U and the unitarity of what comes back, both to the 1e-14 the device gates on, on random matrices and on the ones
built to be hard for a reduced format -- a1 = 0 and |a1| down to 1e-300 (the phase of the reflector), Im a3 and Im c2 up to 1 - 1e-12 (the poles of the two
stereographic projections) -- and an exact pole reported as a gate failure, not as a NaN.

Measured maximum of |decode(encode(U)) - U| (numpy, fp64, modulus of the complex difference): 1e5 Haar-random matrices 2.95e-15 (unitarity 1.33e-15);
unit / diagonal / permutation 9.9e-16; a1 = 0 1.65e-15; |a1| = 1e-1 .. 1e-300 and the smallest subnormal 2.39e-15; Im a3 = 1 - 1e-3 .. 1 - 1e-12 1.32e-15;
Im c2 = 1 - 1e-3 .. 1 - 1e-12 7.3e-16.  Unitarity of what comes back 1.3e-15 at most."""
import numpy as np
import pytest

import link8_numpy as l8

BOUND = 1e-14


def su3_from_rows(a, b):
    """Gram-Schmidt on (a, b), row 2 = conj(a x b)"""
    a = a / np.linalg.norm(a, axis=-1, keepdims=True)
    b = b - a * np.sum(np.conj(a) * b, axis=-1, keepdims=True)
    b = b / np.linalg.norm(b, axis=-1, keepdims=True)
    return np.stack([a, b, np.conj(np.cross(a, b))], axis=-2)


def rnd(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def haar(rng, n):
    return su3_from_rows(rnd(rng, n, 3), rnd(rng, n, 3))


def unitarity(M):
    return float(abs(M @ np.conj(np.swapaxes(M, -1, -2)) - np.eye(3)).max())


def check(M, what):
    back = l8.decode(l8.encode(M))
    dev, uni, g = float(abs(back - M).max()), unitarity(back), l8.gate(M)
    print("%-40s max |decode(encode(U)) - U| %.2e   unitarity %.2e   gate %.2e" % (what, dev, uni, g))
    assert np.isfinite(back).all()
    assert dev <= BOUND and uni <= BOUND, (what, dev, uni)
    assert g == dev
    return dev


def with_a1(rng, n, r):
    """row a with |a1| = r (a random phase), the rest random"""
    rest = rnd(rng, n, 2)
    rest *= np.sqrt(1.0 - r * r) / np.linalg.norm(rest, axis=-1, keepdims=True)
    a = np.concatenate([(r * np.exp(2j * np.pi * rng.random(n)))[:, None], rest], axis=-1)
    return su3_from_rows(a, rnd(rng, n, 3))


def test_haar_random_matrices():
    check(haar(np.random.default_rng(1), 100000), "1e5 Haar-random")


def test_unit_diagonal_and_permutation_matrices():
    rng = np.random.default_rng(2)
    eye = np.eye(3, dtype=complex)
    ph = 2 * np.pi * rng.random((64, 2))
    diag = np.zeros((64, 3, 3), dtype=complex)
    diag[:, 0, 0], diag[:, 1, 1], diag[:, 2, 2] = np.exp(1j * ph[:, 0]), np.exp(1j * ph[:, 1]), np.exp(-1j * (ph[:, 0] + ph[:, 1]))
    perms = []
    for p in ((0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0), (1, 0, 2)):
        P = eye[list(p)]
        perms.append(P * np.linalg.det(P).real)      # odd permutations with a sign: on the group, and real
    M = np.concatenate([eye[None], diag, np.array(perms)])
    assert unitarity(M) <= 1e-15
    check(M, "unit, diagonal, permutation")
    W = l8.encode(M)
    assert np.sum(W[:, :5] ** 2, axis=-1).max() <= 4.0 and np.sum(W[1 + 64:, 5:] ** 2, axis=-1).max() <= 4.0      # unit and real permutation matrices: far from both poles
    assert np.array_equal(l8.decode(l8.encode(eye)), eye)      # what the time-like links below the seam store


def test_a1_zero_and_small():
    rng = np.random.default_rng(3)
    check(with_a1(rng, 4096, 0.0), "a1 = 0")
    worst = 0.0
    for r in [10.0 ** -k for k in (1, 2, 4, 8, 16, 50, 100, 139, 140, 141, 150, 200, 300)] + [5e-324]:
        worst = max(worst, check(with_a1(rng, 1024, r), "|a1| = %.0e" % r))
    print("worst over |a1| = 1e-1 .. 1e-300: %.2e" % worst)


@pytest.mark.parametrize("row", ["a3", "c2"])
def test_near_the_poles(row):
    rng = np.random.default_rng(4)
    n, worst = 1024, 0.0
    for k in range(3, 13):
        x6 = 1.0 - 10.0 ** -k
        tail = rnd(rng, n, 3 if row == "a3" else 2)[..., :-1]      # the free components next to the one at the pole
        re = rng.standard_normal(n)
        free = np.sqrt(1.0 - x6 * x6)
        scale = free / np.sqrt(np.sum(abs(tail) ** 2, axis=-1) + re * re)
        v = np.concatenate([tail * scale[:, None], (re * scale + 1j * x6)[:, None]], axis=-1)      # a unit vector with Im (last) = 1 - 1e-k
        if row == "a3":
            M = su3_from_rows(v, rnd(rng, n, 3))
            assert abs(M[:, 0, 2].imag - x6).max() <= 1e-15
        else:
            a = haar(rng, n)[:, 0, :]
            X = l8.encode(su3_from_rows(a, rnd(rng, n, 3)))[:, :5]
            a1, phi, tau = l8.frame(X)
            s = np.conj(a1[:, 1]) * v[:, 0] + np.conj(a1[:, 2]) * v[:, 1]
            b = np.stack([-phi * s, v[:, 0] - tau * a1[:, 1] * s, v[:, 1] - tau * a1[:, 2] * s], axis=-1)
            M = np.stack([a1, b, np.conj(np.cross(a1, b))], axis=-2)
            assert unitarity(M) <= 4e-15
            assert abs(l8.encode(M)[:, 5:] ** 2).sum(axis=-1).min() >= 0.1 * 10.0 ** k      # (c1, c2) of these matrices does sit at the pole
        worst = max(worst, check(M, "Im %s = 1 - 1e-%d" % (row, k)))
    print("worst over Im %s = 1 - 1e-3 .. 1 - 1e-12: %.2e" % (row, worst))


def test_an_exact_pole_is_a_gate_failure_not_a_nan():
    rng = np.random.default_rng(5)
    good = haar(rng, 8)
    a_pole = np.array([0.0, 0.0, 1.0j])
    b = np.array([1.0 + 0.0j, 0.0, 0.0])
    Ma = np.stack([a_pole, b, np.conj(np.cross(a_pole, b))])      # a3 = i
    a = good[0, 0, :]
    X = l8.encode(good[:1])[0, :5]
    a1, phi, tau = l8.frame(X)
    c1, c2 = 0.0, 1.0j                                            # c2 = i
    s = np.conj(a1[1]) * c1 + np.conj(a1[2]) * c2
    bb = np.array([-phi * s, c1 - tau * a1[1] * s, c2 - tau * a1[2] * s])
    Mc = np.stack([a1, bb, np.conj(np.cross(a1, bb))])
    assert unitarity(Mc) <= 4e-15
    for M in (Ma, Mc):
        g = l8.gate(np.concatenate([good, M[None]]))
        assert g == l8.FAIL and not np.isnan(g)
    assert l8.gate(good) <= BOUND
