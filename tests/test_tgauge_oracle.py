"""Temporal gauge for the Wilson CG, stated with the CPU oracle: the convention the device kernels reproduce (fields.hip gauge_ensure_tgauge).
G(x, 0) = 1, G(x, t + 1) = G(x, t) U_t(x, t) put back on SU(3) at every step, U'_mu(n) = G(n) U_mu(n) G(n + mu)^+ with the time-like links below the seam
t = T - 1 replaced by exact unit matrices.  Then D[U'] (G psi) = G D[U] psi, the same for D^+, and the CG on (U', G b) produces G x_k.
The oracle's host link array holds the matrix that acts on colour transposed in its last two axes: the rotation is written for V = swapaxes(U)."""
import numpy as np

KAPPA = 0.141139
L = (4, 4, 4, 16)


def sw(A):
    return np.swapaxes(A, -1, -2)


def proj(M):
    """rows 0, 1 by Gram-Schmidt, row 2 = conj(row 0 x row 1)"""
    r0 = M[..., 0, :]
    r0 = r0 / np.linalg.norm(r0, axis=-1, keepdims=True)
    r1 = M[..., 1, :]
    r1 = r1 - r0 * np.sum(np.conj(r0) * r1, axis=-1, keepdims=True)
    r1 = r1 / np.linalg.norm(r1, axis=-1, keepdims=True)
    return np.stack([r0, r1, np.conj(np.cross(r0, r1))], axis=-2)


def gmul(G, psi):
    return np.ascontiguousarray(np.einsum("tzyxab,stzyxb->stzyxa", G, psi))


def rotate(U):
    """-> G [t,z,y,x,3,3], the rotated links in the oracle's layout, the 12-real gate of U', max |U'_t - 1| below the seam"""
    T = U.shape[1]
    V = sw(U)
    G = np.zeros((T,) + U.shape[2:], dtype=complex)
    G[0] = np.eye(3)
    for t in range(T - 1):
        G[t + 1] = proj(G[t] @ V[3, t])
    Vg = np.empty_like(V)
    for mu in range(4):                         # host axes are (t, z, y, x)
        Gs = np.roll(G, -1, axis=[3, 2, 1, 0][mu])
        Vg[mu] = G @ V[mu] @ np.conj(sw(Gs))
    gate = abs(Vg[..., 2, :] - np.conj(np.cross(Vg[..., 0, :], Vg[..., 1, :]))).max()
    unit = abs(Vg[3, : T - 1] - np.eye(3)).max()
    Vg[3, : T - 1] = np.eye(3)
    return G, np.ascontiguousarray(sw(Vg)), gate, unit


def test_rotated_links_pass_the_gates(orc):
    G, Ug, gate, unit = rotate(orc.hot_gauge(L, 111))
    assert gate <= 1e-14 and unit <= 1e-14, (gate, unit)


def test_operator_is_covariant(orc):
    for bc in ((1, 1, 1, -1), (1, 1, 1, 1)):
        U = orc.hot_gauge(L, 111)
        b = orc.gaussian_spinor(orc.wilson_shape(L), 112)
        G, Ug, _, _ = rotate(U)
        for dagger in (False, True):
            y = orc.wilson_D(U, b, L, KAPPA, 1.0, bc, dagger=dagger)
            yg = orc.wilson_D(Ug, gmul(G, b), L, KAPPA, 1.0, bc, dagger=dagger)
            err = abs(yg - gmul(G, y)).max() / abs(y).max()
            assert err <= 1e-13, (bc, dagger, err)      # the project's operator-parity bound


def test_cg_windows_equal_the_unrotated_run(orc):
    bc = (1, 1, 1, -1)
    U = orc.hot_gauge(L, 111)
    b = orc.gaussian_spinor(orc.wilson_shape(L), 112)
    G, Ug, _, _ = rotate(U)
    Gd = np.conj(sw(G))
    for n in (5, 40):
        x = orc.cg_DdagD_fixed(orc.WILSON, U, b, L, KAPPA, 1.0, bc, niter=n)
        xb = gmul(Gd, orc.cg_DdagD_fixed(orc.WILSON, Ug, gmul(G, b), L, KAPPA, 1.0, bc, niter=n))
        err = abs(xb - x).max() / abs(x).max()
        assert err <= 1e-12, (n, err)
