"""Numpy restatement of the R x T Wilson loops of the three space-time planes (include/lqcd_hip.h "R x T Wilson loops"), written from the definition,
independent of the device code.  Fields are in the host layout U[mu,t,z,y,x,b,a]; matrices inside are [.., a, b] (oracle._mat), shifts by
flow_numpy._at (periodic).

    S_mu,R(x) = U_mu(x) U_mu(x + mu) ... U_mu(x + (R-1) mu)     mu = 0, 1, 2     (extended one link at a time)
    T_T(x)    = U_3(x) U_3(x + t) ... U_3(x + (T-1) t)
    W(R, T)   = 1/(9 V) sum_x sum_mu Re tr[ S_mu,R(x) T_T(x + R mu) S_mu,R(x + T t)^+ T_T(x)^+ ]
"""
import numpy as np

from flow_numpy import _at, _dag
from oracle import oracle as orc


def _unit(d, n):
    return [n if k == d else 0 for k in range(4)]


def wilson_loops(U, L, Rmax, Tmax):
    """The table W[R-1, T-1], R = 1..Rmax, T = 1..Tmax."""
    Um = orc._mat(U)
    V = float(np.prod(L))
    tab = np.zeros((Rmax, Tmax))
    tl = []
    for T in range(1, Tmax + 1):
        tl.append(Um[3] if T == 1 else tl[-1] @ _at(Um[3], _unit(3, T - 1)))
    for mu in range(3):
        S = None
        for R in range(1, Rmax + 1):
            S = Um[mu] if R == 1 else S @ _at(Um[mu], _unit(mu, R - 1))
            for T in range(1, Tmax + 1):
                A = tl[T - 1]
                P = S @ _at(A, _unit(mu, R)) @ _dag(_at(S, _unit(3, T))) @ _dag(A)
                tab[R - 1, T - 1] += float(np.trace(P, axis1=-2, axis2=-1).real.sum())
    return tab / (9.0 * V)


ABELIAN_L = (6, 4, 4, 8)


def abelian_field(L=ABELIAN_L):
    """U_3(x) = diag(e^{i a x}, e^{-i a x}, 1) with a = 2 pi / L[0] (x the first coordinate), every other link 1."""
    a = 2.0 * np.pi / L[0]
    x = np.arange(L[0])[None, None, None, :] * np.ones((L[3], L[2], L[1], 1))
    Um = np.zeros((4, L[3], L[2], L[1], L[0], 3, 3), dtype=np.complex128)
    for c in range(3):
        Um[..., c, c] = 1.0
    Um[3, ..., 0, 0] = np.exp(1j * a * x)
    Um[3, ..., 1, 1] = np.exp(-1j * a * x)
    return np.ascontiguousarray(orc._mat(Um))


def abelian_table(Rmax, Tmax, L=ABELIAN_L):
    """The loop in the (0, 3) plane is diag(e^{i a R T}, e^{-i a R T}, 1), the other two planes give the unit matrix:  W = [2 + (2 cos(a R T) + 1) / 3] / 3."""
    a = 2.0 * np.pi / L[0]
    R, T = np.meshgrid(np.arange(1, Rmax + 1), np.arange(1, Tmax + 1), indexing="ij")
    return (2.0 + (2.0 * np.cos(a * R * T) + 1.0) / 3.0) / 3.0


def haar_sigma(L):
    """Standard deviation of an entry of the table on Haar-random links while distinct loops are distinct sets of links (R < min spatial extent,
    T < Lt): the 3 V loops are uncorrelated and Re tr / 3 of a Haar matrix has variance 1/18, so sigma = sqrt(1 / (18 * 3 V)) = 1 / sqrt(54 V)."""
    return 1.0 / np.sqrt(54.0 * float(np.prod(L)))
