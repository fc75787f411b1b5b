"""Numpy restatement of the Wilson gradient flow and of the six observables measured along it (include/lqcd_hip.h "gradient flow"), written from the
textbook definitions on top of oracle.oracle's staple sum, independent of the device code.  Fields are in the host layout U[mu,t,z,y,x,b,a];
matrices inside are [.., a, b] (oracle._mat).

    Z_mu(x)  = TA(G) with G = -U_mu(x) A_mu(x), the staple force at beta = 6:  Z = -TA(U A)
    RK3      X1 = eps/4 Z(W0),                 W1 = exp(X1) W0
             X2 = 8 eps/9 Z(W1) - 17/9 X1,     W2 = exp(X2) W1
             X3 = 3 eps/4 Z(W2) - X2,          W3 = exp(X3) W2
    G_mu nu  = TA(sum of n loops through x in the (mu, nu) plane) / n, every loop run the way of +mu +nu -mu -nu
    p, E_plaq = 2 sum_{mu<nu} Re tr(1 - P), E_clov = -sum_{mu<nu} tr G G, Q[set] = -(1/4 pi^2) sum_x [tr G01 G23 - tr G02 G13 + tr G03 G12],
    Q_impr = 5/3 Q_clov - 1/12 Q_rect,  Q_rect = 2 Q[rect]
"""
import numpy as np

from oracle import oracle as orc

OBS = ("p", "E_plaq", "E_clov", "Q_plaq", "Q_clov", "Q_impr")


def _dag(A):
    return np.conj(np.swapaxes(A, -1, -2))


def ta(W):
    X = 0.5 * (W - _dag(W))
    return X - (np.trace(X, axis1=-2, axis2=-1) / 3.0)[..., None, None] * np.eye(3)


def expm_ah(X):
    """exp of anti-Hermitian matrices X = i H through the eigen-decomposition of H (batched)."""
    w, V = np.linalg.eigh(-1j * X)
    return (V * np.exp(1j * w)[..., None, :]) @ _dag(V)


def flow_Z(Um, L):
    return np.stack([-ta(Um[mu] @ orc._staple_sum(Um, L, mu)) for mu in range(4)])


def euler_step(U, L, eps):
    Um = orc._mat(U)
    return np.ascontiguousarray(orc._mat(expm_ah(eps * flow_Z(Um, L)) @ Um))


def rk3_step(U, L, eps):
    W = orc._mat(U)
    X = 0.25 * eps * flow_Z(W, L)
    W = expm_ah(X) @ W
    X = (8.0 / 9.0) * eps * flow_Z(W, L) - (17.0 / 9.0) * X
    W = expm_ah(X) @ W
    X = 0.75 * eps * flow_Z(W, L) - X
    W = expm_ah(X) @ W
    return np.ascontiguousarray(orc._mat(W))


def flow(U, L, eps, nsteps):
    for _ in range(nsteps):
        U = rk3_step(U, L, eps)
    return U


def _at(F, off):
    """F(x + off) for a field F[t,z,y,x,..] and an offset in (x, y, z, t) order."""
    return np.roll(F, shift=tuple(-o for o in off), axis=(3, 2, 1, 0))


def loop(Um, path):
    """Product of the links along a closed path from every x; path = sequence of (direction, +1 | -1)."""
    off = [0, 0, 0, 0]
    P = None
    for d, s in path:
        if s > 0:
            u = _at(Um[d], off)
            off[d] += 1
        else:
            off[d] -= 1
            u = _dag(_at(Um[d], off))
        P = u if P is None else P @ u
    return P


def leaves(mu, nu, kind):
    """The loop set of `kind` in the (mu, nu) plane as paths, all turning the way of +mu +nu -mu -nu."""
    out = []
    ext = [(1, 1)] if kind != "rect" else [(1, 2), (2, 1)]
    quads = [(1, 1)] if kind == "plaquette" else [(1, 1), (-1, 1), (-1, -1), (1, -1)]
    for sm, sn in quads:
        for a, b in ext:
            m, n = [(mu, sm)] * a, [(nu, sn)] * b
            mb, nb = [(mu, -sm)] * a, [(nu, -sn)] * b
            out.append(m + n + mb + nb if sm * sn > 0 else n + m + nb + mb)
    return out


def field(Um, mu, nu, kind):
    ps = leaves(mu, nu, kind)
    S = sum(loop(Um, p) for p in ps)
    return ta(S) / len(ps), S


def _trre(A, B):
    return np.einsum("...ab,...ba->...", A, B).real


def charge(Um, kind):
    G = {(mu, nu): field(Um, mu, nu, kind)[0] for mu in range(4) for nu in range(mu + 1, 4)}
    s = _trre(G[0, 1], G[2, 3]) - _trre(G[0, 2], G[1, 3]) + _trre(G[0, 3], G[1, 2])
    return -float(s.sum()) / (4.0 * np.pi ** 2)


def observables(U, L, rect=True):
    """(p, E_plaq, E_clov, Q_plaq, Q_clov, Q_impr) as a dict; rect=False: Q_impr = NaN (the partitioned device path)."""
    Um = orc._mat(U)
    V = float(np.prod(L))
    retr = 0.0
    eclov = 0.0
    for mu in range(4):
        for nu in range(mu + 1, 4):
            P = loop(Um, [(mu, 1), (nu, 1), (mu, -1), (nu, -1)])
            retr += float(np.trace(P, axis1=-2, axis2=-1).real.sum())
            Gc = field(Um, mu, nu, "clover")[0]
            eclov -= float(_trre(Gc, Gc).sum())
    p = retr / (18.0 * V)
    qc = charge(Um, "clover")
    out = {"p": p, "E_plaq": 2.0 * (18.0 * V - retr) / V, "E_clov": eclov / V, "Q_plaq": charge(Um, "plaquette"), "Q_clov": qc}
    out["Q_impr"] = (5.0 / 3.0) * qc - (2.0 * charge(Um, "rect")) / 12.0 if rect else float("nan")
    return out


def gauge_transform(U, L, seed):
    """U_mu(x) -> g(x) U_mu(x) g(x + mu)^+ with random SU(3) g."""
    rng = np.random.default_rng(seed)
    g = orc.random_su3(rng, int(np.prod(L))).reshape(L[3], L[2], L[1], L[0], 3, 3)
    Um = orc._mat(U)
    out = np.stack([g @ Um[mu] @ _dag(_at(g, [1 if k == mu else 0 for k in range(4)])) for mu in range(4)])
    return np.ascontiguousarray(orc._mat(out))


def reflect_x(U):
    """The reflection x -> -x (direction 0): U'_0(x) = U_0(Rx - 0)^+, U'_nu(x) = U_nu(Rx)."""
    Um = orc._mat(U)
    out = np.empty_like(Um)
    out[0] = _dag(np.flip(Um[0], axis=3))                      # index -x - 1
    for nu in range(1, 4):
        out[nu] = np.roll(np.flip(Um[nu], axis=3), 1, axis=3)  # index -x
    return np.ascontiguousarray(orc._mat(out))


def flux_gauge(L, n01, n23):
    """Constant abelian flux through the (0,1) and (2,3) planes, embedded as diag(e^{i phi}, e^{-i phi}, 1): plaquette angles 2 pi n01 / (L0 L1) and
    2 pi n23 / (L2 L3) everywhere, periodic through the last slice's links."""
    t, z, y, x = np.meshgrid(*(np.arange(n) for n in (L[3], L[2], L[1], L[0])), indexing="ij")
    th, th2 = 2 * np.pi * n01 / (L[0] * L[1]), 2 * np.pi * n23 / (L[2] * L[3])
    phi = np.zeros((4,) + x.shape)
    phi[1] = th * x
    phi[0] = np.where(x == L[0] - 1, -th * L[0] * y, 0.0)
    phi[3] = th2 * z
    phi[2] = np.where(z == L[2] - 1, -th2 * L[2] * t, 0.0)
    Um = np.zeros((4,) + x.shape + (3, 3), dtype=np.complex128)
    Um[..., 0, 0] = np.exp(1j * phi)
    Um[..., 1, 1] = np.exp(-1j * phi)
    Um[..., 2, 2] = 1.0
    return np.ascontiguousarray(orc._mat(Um))
