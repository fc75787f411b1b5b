"""Numpy restatement of the plaquette + rectangle gauge action (include/lqcd_hip.h "plaquette + rectangle action"), written from the definitions with every
staple enumerated as a path, independent of the device code.  Inside, fields are [4][X,Y,Z,T,3,3] arrays (matrices [a, b]) shifted with np.roll; the
entry points take and return the host layout U[mu,t,z,y,x,b,a].

    S_g = -(1/3) [ beta_plaq sum_plaq Re tr U_p + beta_rect sum_rect Re tr U_r ]          6 V plaquettes, 12 V rectangles (1x2 and 2x1, every plane, every corner)
    G_mu(n) = -(1/6) U_mu(n) [ beta_plaq (6 plaquette staples) + beta_rect (18 rectangle staples) ],   dS/d eps [U -> exp(i eps T) U] = -2 Im tr(T G)
"""
import numpy as np

GELLMANN = np.zeros((8, 3, 3), dtype=np.complex128)
GELLMANN[0][0, 1] = GELLMANN[0][1, 0] = 1
GELLMANN[1][0, 1] = -1j; GELLMANN[1][1, 0] = 1j
GELLMANN[2][0, 0] = 1; GELLMANN[2][1, 1] = -1
GELLMANN[3][0, 2] = GELLMANN[3][2, 0] = 1
GELLMANN[4][0, 2] = -1j; GELLMANN[4][2, 0] = 1j
GELLMANN[5][1, 2] = GELLMANN[5][2, 1] = 1
GELLMANN[6][1, 2] = -1j; GELLMANN[6][2, 1] = 1j
GELLMANN[7] = np.diag([1, 1, -2]) / np.sqrt(3)


def to_xyzt(U):
    """host layout [mu,t,z,y,x,b,a] -> [mu][x,y,z,t,a,b]"""
    return np.ascontiguousarray(np.transpose(U, (0, 4, 3, 2, 1, 6, 5)))


def to_host(W):
    return np.ascontiguousarray(np.transpose(W, (0, 4, 3, 2, 1, 6, 5)))


def dag(A):
    return np.conj(np.swapaxes(A, -1, -2))


def ta(W):
    X = 0.5 * (W - dag(W))
    return X - (np.trace(X, axis1=-2, axis2=-1) / 3.0)[..., None, None] * np.eye(3)


def at(F, off):
    """F(n + off) for F[x,y,z,t,..]"""
    return np.roll(F, shift=tuple(-o for o in off), axis=(0, 1, 2, 3))


def path(W, start, steps):
    """At every n: the ordered product of the links along `steps` = ((direction, +1 | -1), ...) from n + start."""
    off = list(start)
    P = None
    for d, s in steps:
        if s > 0:
            u = at(W[d], off)
            off[d] += 1
        else:
            off[d] -= 1
            u = dag(at(W[d], off))
        P = u if P is None else P @ u
    return P, off


def _retr_sum(P):
    return float(np.trace(P, axis1=-2, axis2=-1).real.sum())


def plaquette_sum(W):
    s = 0.0
    for mu in range(4):
        for nu in range(mu + 1, 4):
            P, off = path(W, (0, 0, 0, 0), ((mu, 1), (nu, 1), (mu, -1), (nu, -1)))
            assert off == [0, 0, 0, 0]
            s += _retr_sum(P)
    return s


def rectangle_sum(W):
    """sum of Re tr over the 12 V rectangles: long side along a, short side along b, every ordered pair a != b"""
    s = 0.0
    for a in range(4):
        for b in range(4):
            if a == b:
                continue
            P, off = path(W, (0, 0, 0, 0), ((a, 1), (a, 1), (b, 1), (a, -1), (a, -1), (b, -1)))
            assert off == [0, 0, 0, 0]
            s += _retr_sum(P)
    return s


def plaquette_staples(mu, nu):
    return [((nu, 1), (mu, -1), (nu, -1)), ((nu, -1), (mu, -1), (nu, 1))]


def rectangle_staples(mu, nu):
    """the six rectangle staples of the link (n, mu) in the plane (mu, nu): paths of five links from n + mu back to n"""
    return [
        ((mu, 1), (nu, 1), (mu, -1), (mu, -1), (nu, -1)),       # long side along mu, the link its first half, above
        ((mu, 1), (nu, -1), (mu, -1), (mu, -1), (nu, 1)),       #                                             below
        ((nu, 1), (mu, -1), (mu, -1), (nu, -1), (mu, 1)),       # long side along mu, the link its second half, above
        ((nu, -1), (mu, -1), (mu, -1), (nu, 1), (mu, 1)),       #                                              below
        ((nu, 1), (nu, 1), (mu, -1), (nu, -1), (nu, -1)),       # long side along nu, above
        ((nu, -1), (nu, -1), (mu, -1), (nu, 1), (nu, 1)),       #                     below
    ]


def staple_sum(W, mu, wp, wr):
    """wp (six plaquette staples) + wr (eighteen rectangle staples) of direction mu"""
    A = np.zeros_like(W[mu])
    start = [1 if k == mu else 0 for k in range(4)]
    for nu in range(4):
        if nu == mu:
            continue
        for w, paths in ((wp, plaquette_staples(mu, nu)), (wr, rectangle_staples(mu, nu))):
            if w == 0.0:
                continue
            for steps in paths:
                P, off = path(W, start, steps)
                assert off == [0, 0, 0, 0]
                A += w * P
    return A


# ---------------------------------------------------------------- entry points in the host layout
def rectangle(U, L):
    return rectangle_sum(to_xyzt(U)) / (36.0 * float(np.prod(L)))


def plaquette(U, L):
    return plaquette_sum(to_xyzt(U)) / (18.0 * float(np.prod(L)))


def action(U, L, beta_plaq, beta_rect):
    W = to_xyzt(U)
    return -(beta_plaq * plaquette_sum(W) + beta_rect * rectangle_sum(W)) / 3.0


def force(U, L, beta_plaq, beta_rect):
    W = to_xyzt(U)
    return to_host(np.stack([-(1.0 / 6.0) * W[mu] @ staple_sum(W, mu, beta_plaq, beta_rect) for mu in range(4)]))


def link_staple(U, L, mu, beta_plaq, beta_rect):
    """calc_dSdUmu! for this action: (beta_plaq/2) plaquette staples + (beta_rect/2) rectangle staples of direction mu, host layout [t,z,y,x,b,a]"""
    return to_host(staple_sum(to_xyzt(U), mu, 0.5 * beta_plaq, 0.5 * beta_rect)[None])[0]


def lw(beta):
    """Luscher-Weisz (tree-level Symanzik)"""
    return 5.0 * beta / 3.0, -beta / 12.0


def c1_action(beta, c1):
    """Iwasaki (c1 = -0.331), DBW2 (c1 = -1.4088)"""
    return (1.0 - 8.0 * c1) * beta, c1 * beta


def expm_ah(X):
    w, V = np.linalg.eigh(-1j * X)
    return (V * np.exp(1j * w)[..., None, :]) @ dag(V)


def fd_rotations(L, n=10, seed=4242):
    """n random (site (x, y, z, t), mu, generator T = sum_a c_a lambda_a / 2)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        site = tuple(int(rng.integers(0, L[k])) for k in range(4))
        mu = int(rng.integers(0, 4))
        T = np.einsum("a,aij->ij", rng.standard_normal(8), GELLMANN / 2)
        out.append((site, mu, T))
    return out


def rotate_link(U, site, mu, T, eps):
    """a copy of U (host layout) with U_mu(site) -> exp(i eps T) U_mu(site)"""
    x, y, z, t = site
    V = U.copy()
    m = V[mu, t, z, y, x].T                      # [a, b]
    V[mu, t, z, y, x] = (expm_ah(1j * eps * T) @ m).T
    return V


def fd_prediction(G, site, mu, T):
    """-2 Im tr(T G_mu(site)) for a force field in the host layout"""
    x, y, z, t = site
    return -2.0 * float(np.trace(T @ G[mu, t, z, y, x].T).imag)


def gauge_transform(U, L, seed):
    """U_mu(n) -> g(n) U_mu(n) g(n + mu)^+; returns (U', g) with g[x,y,z,t,a,b]"""
    rng = np.random.default_rng(seed)
    m = rng.standard_normal(tuple(L) + (3, 3)) + 1j * rng.standard_normal(tuple(L) + (3, 3))
    q, r = np.linalg.qr(m)
    d = np.diagonal(r, axis1=-2, axis2=-1)
    q = q * (d / np.abs(d))[..., None, :]
    g = q / (np.linalg.det(q) ** (1.0 / 3.0))[..., None, None]
    W = to_xyzt(U)
    out = np.stack([g @ W[mu] @ dag(at(g, [1 if k == mu else 0 for k in range(4)])) for mu in range(4)])
    return to_host(out), g


def flux_field(L, n01, n23):
    """constant abelian flux diag(e^{i phi}, e^{-i phi}, 1): every plaquette of the (0,1) plane has angle th = 2 pi n01 / (L0 L1), of the (2,3) plane
    th2 = 2 pi n23 / (L2 L3), periodic through the links of the last slice; host layout"""
    x, y, z, t = np.meshgrid(*(np.arange(n) for n in L), indexing="ij")
    th, th2 = 2 * np.pi * n01 / (L[0] * L[1]), 2 * np.pi * n23 / (L[2] * L[3])
    phi = np.zeros((4,) + x.shape)
    phi[1] = th * x
    phi[0] = np.where(x == L[0] - 1, -th * L[0] * y, 0.0)
    phi[3] = th2 * z
    phi[2] = np.where(z == L[2] - 1, -th2 * L[2] * t, 0.0)
    W = np.zeros((4,) + x.shape + (3, 3), dtype=np.complex128)
    W[..., 0, 0] = np.exp(1j * phi)
    W[..., 1, 1] = np.exp(-1j * phi)
    W[..., 2, 2] = 1.0
    return to_host(W), th, th2


def flux_rectangle(th, th2):
    """a rectangle of the (0,1) / (2,3) plane encloses 2 th / 2 th2, the other eight orientations give the unit matrix"""
    return (8.0 + 2.0 * (2.0 * np.cos(2.0 * th) + 1.0) / 3.0 + 2.0 * (2.0 * np.cos(2.0 * th2) + 1.0) / 3.0) / 12.0
