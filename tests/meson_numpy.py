"""Numpy restatement of the meson correlators (include/lqcd_hip.h "meson correlators"), written from the definition, independent of the device code.
Fields are in the host layout: a Wilson column is psi[s,t,z,y,x,c], a staggered one psi[t,z,y,x,c]; cols[4*b + beta] is the solution for source colour b,
source spin beta.

    Gamma_n = gamma_x^n0 gamma_y^n1 gamma_z^n2 gamma_t^n3,   n = n0 + 2 n1 + 4 n2 + 8 n3
    C_n(t)  = sum_{x: x_t = t} Re tr_{spin,colour}[ Gamma_n S(x) Gamma_n^+ gamma_5 S(x)^+ gamma_5 ],   S(x)[alpha a, beta b] = cols[4 b + beta][alpha, x, a]
"""
import numpy as np

from oracle import oracle as orc

NCHAN = 16


def gamma_n(n):
    G = np.eye(4, dtype=np.complex128)
    for mu in range(4):
        if (n >> mu) & 1:
            G = G @ orc.GAMMA[mu]
    return G


def propagator(cols):
    """S[t,z,y,x, alpha, a, beta, b] from ncol = 4 nb columns [s,t,z,y,x,c] in the order 4 b + beta."""
    cols = np.asarray(cols)
    nb = cols.shape[0] // 4
    assert cols.shape[0] == 4 * nb and cols.shape[1] == 4 and cols.shape[-1] == 3
    S = np.zeros(cols.shape[2:6] + (4, 3, 4, nb), dtype=np.complex128)
    for b in range(nb):
        for be in range(4):
            S[..., be, b] = np.moveaxis(cols[4 * b + be], 0, 4)        # [t,z,y,x,alpha,a]
    return S


def contract(cols, Lt=None, imag=False):
    """table[n, t] = C_n(t) summed over the colour blocks given; imag = True returns the imaginary parts of the traces as well."""
    S = propagator(cols)
    assert Lt is None or S.shape[0] == Lt
    g5 = orc.GAMMA[4]
    tab = np.zeros((NCHAN, S.shape[0]), dtype=np.complex128)
    for n in range(NCHAN):
        G = gamma_n(n)
        B = G.conj().T @ g5
        # tr[G S B S^+ g5] = G[i,j] S[j a, k b] B[k,l] conj(S[m a, l b]) g5[m,i]
        tab[n] = np.einsum("ij,tzyxjakb,kl,tzyxmalb,mi->t", G, S, B, np.conj(S), g5, optimize=True)
    return (tab.real, tab.imag) if imag else tab.real


def norm2_timeslices(psi):
    """sum |psi|^2 per time slice of a Wilson [s,t,z,y,x,c] or staggered [t,z,y,x,c] field."""
    a = np.abs(np.asarray(psi)) ** 2
    if a.ndim == 6:
        return a.sum(axis=(0, 2, 3, 4, 5))
    return a.sum(axis=(1, 2, 3, 4))


def rho_literature(cols):
    """The rho expression of tests/test_gpu_quenched_literature.py (_pion_correlator), signed: sum_i tr[g5 g_i S g_i g5 S^+]."""
    cols = np.asarray(cols)
    S = np.zeros(cols.shape[1:] + (4, 3), dtype=np.complex128)      # [sink spin, t, z, y, x, sink colour, source spin, source colour]
    for ic in range(3):
        for isp in range(4):
            S[..., isp, ic] = cols[4 * ic + isp]
    g5 = orc.GAMMA[4]
    Cv = np.zeros(S.shape[1])
    for i in range(3):
        T = np.einsum("pq,q...->p...", g5 @ orc.GAMMA[i], S)
        T = np.einsum("...Xd,XY->...Yd", T, orc.GAMMA[i] @ g5)
        Cv += np.real((T * np.conj(S)).sum(axis=(0, 2, 3, 4, 5, 6, 7)))
    return Cv


def free_pion(L, kappa, r=1.0, bc=(1, 1, 1, -1)):
    """C_15(t) of the free Wilson operator (unit links) for a point source at the origin, from the momentum-space inverse:
    D(p) = a(p) + i sum_mu b_mu(p) gamma_mu, a = 1 - 2 kappa r sum_mu cos p_mu, b_mu = 2 kappa sin p_mu (the sign of b does not enter |S|^2),
    D^-1 = (a - i b.gamma) / (a^2 + b^2); p_mu = 2 pi k / L_mu, and 2 pi (k + 1/2) / L_mu in an antiperiodic direction, whose extra phase
    e^{i pi x_mu / L_mu} has modulus one.  C(t) = 3 sum_x sum_{alpha beta} |S_{alpha beta}(x)|^2 (three colours)."""
    ks = [2.0 * np.pi * (np.arange(L[mu]) + (0.5 if bc[mu] < 0 else 0.0)) / L[mu] for mu in range(4)]
    pt, pz, py, px = np.meshgrid(ks[3], ks[2], ks[1], ks[0], indexing="ij")
    p = [px, py, pz, pt]
    a = 1.0 - 2.0 * kappa * r * sum(np.cos(q) for q in p)
    b = [2.0 * kappa * np.sin(q) for q in p]
    den = a * a + sum(q * q for q in b)
    Dinv = a[..., None, None] * np.eye(4) - 1j * sum(b[mu][..., None, None] * orc.GAMMA[mu] for mu in range(4))
    Dinv = Dinv / den[..., None, None]
    S = np.fft.ifftn(Dinv, axes=(0, 1, 2, 3))
    return 3.0 * (np.abs(S) ** 2).sum(axis=(1, 2, 3, 4, 5))
