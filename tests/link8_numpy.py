"""numpy restatement of the 8-real SU(3) chart the temporal-gauge CG reads (csrc/lqcd_internal.h link8_decode, csrc/fields.hip tgauge8_encode).
A matrix M[..., 3, 3] has rows a = M[..., 0, :], b = M[..., 1, :] and row 2 = conj(a x b).
  a, a point of S^5 (Re a1, Re a2, Re a3, Im a1, Im a2 | Im a3), is its stereographic image X in R^5 from the pole Im a3 = 1;
  b = H (0, c1, c2)^T, H = 1 - tau v v^+ the Householder reflector of a (v = a + phi e1, phi = a1 / |a1|, tau = 1 / (1 + |a1|)), and (c1, c2), a point of
  S^3 (Re c1, Im c1, Re c2 | Im c2), is its stereographic image Y in R^3 from the pole Im c2 = 1.
encode returns W[..., 8] = (X1 .. X5, Y1 .. Y3).  The device takes one reciprocal of the product of its three denominators and a refined rsq where this file
divides and takes square roots: the two agree to rounding, not bit for bit."""
import numpy as np

TINY = 1e-280      # |(X1, X4)|^2 below it: the stored words of a1 leave no phase; phi = 1, |a1| = 0
BIG = 1e30         # |X|^2 or |Y|^2 above it: the link sits on a pole of the chart and fails the gate
FAIL = 1e300       # what the gate reports for such a link (and for anything that is not finite)


def _stereo(x, x6):
    """x[..., k], the pole coordinate x6 -> x / (1 - x6), with 1 - x6 = sum x_i^2 / (1 + x6) where x6 > 0 (relative precision near the pole)"""
    ss = np.sum(x * x, axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        om = np.where(x6 > 0.0, ss / (1.0 + x6), 1.0 - x6)
        return x / om[..., None]


def frame(X):
    """X[..., 5] -> a[..., 3], phi[...], tau[...]: the row the stencils see and the reflector both sides use"""
    n = np.sum(X * X, axis=-1)
    r2 = X[..., 0] ** 2 + X[..., 3] ** 2
    tiny = ~(r2 >= TINY)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        rho = np.where(tiny, 0.0, np.sqrt(np.where(tiny, 1.0, r2)))
        phi = np.where(tiny, 1.0 + 0.0j, (X[..., 0] + 1j * X[..., 3]) / np.where(tiny, 1.0, rho))
        d1 = n + 1.0
        a = np.stack([2.0 * X[..., 0] / d1 + 2.0j * X[..., 3] / d1, 2.0 * X[..., 1] / d1 + 2.0j * X[..., 4] / d1, 2.0 * X[..., 2] / d1 + 1j * (n - 1.0) / d1], axis=-1)
        tau = d1 / (d1 + 2.0 * rho)
    return a, phi, tau


def decode(W):
    """W[..., 8] -> M[..., 3, 3]"""
    X, Y = W[..., :5], W[..., 5:]
    a, phi, tau = frame(X)
    m = np.sum(Y * Y, axis=-1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d2 = m + 1.0
        c1 = 2.0 * Y[..., 0] / d2 + 2.0j * Y[..., 1] / d2
        c2 = 2.0 * Y[..., 2] / d2 + 1j * (m - 1.0) / d2
        s = np.conj(a[..., 1]) * c1 + np.conj(a[..., 2]) * c2
        b = np.stack([-phi * s, c1 - tau * a[..., 1] * s, c2 - tau * a[..., 2] * s], axis=-1)
        return np.stack([a, b, np.conj(np.cross(a, b))], axis=-2)


def encode(M):
    """M[..., 3, 3] -> W[..., 8]"""
    a, b = M[..., 0, :], M[..., 1, :]
    X = _stereo(np.stack([a[..., 0].real, a[..., 1].real, a[..., 2].real, a[..., 0].imag, a[..., 1].imag], axis=-1), a[..., 2].imag)
    a1, phi, tau = frame(X)      # a' decoded from X: b is projected with the reflector the decoder will build
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        q = np.conj(a1[..., 0] + phi) * b[..., 0] + np.conj(a1[..., 1]) * b[..., 1] + np.conj(a1[..., 2]) * b[..., 2]
        c1 = b[..., 1] - tau * a1[..., 1] * q
        c2 = b[..., 2] - tau * a1[..., 2] * q
        nrm = np.sqrt(abs(c1) ** 2 + abs(c2) ** 2)
        c1, c2 = c1 / nrm, c2 / nrm
    Y = _stereo(np.stack([c1.real, c1.imag, c2.real], axis=-1), c2.imag)
    return np.concatenate([X, Y], axis=-1)


def gate(M):
    """max |decode(encode(M)) - M| over all links and entries, the device's gate: FAIL where a link is on a pole of the chart (never a NaN)"""
    W = encode(M)
    with np.errstate(invalid="ignore", over="ignore"):
        d = abs(decode(W) - M).reshape(M.shape[:-2] + (9,)).max(axis=-1)
        big = np.maximum(np.sum(W[..., :5] ** 2, axis=-1), np.sum(W[..., 5:] ** 2, axis=-1))
        d = np.where(np.isfinite(d) & (big <= BIG), d, FAIL)
    return float(d.max())
