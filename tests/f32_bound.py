"""Site-wise error metric for one application of an fp32 operator, and a NumPy restatement of the operators in a chosen precision.

An application  out = a diag psi + b sum_{+-mu} hop_mu psi  is judged per site n:

    e(n) = || out_dev(n) - out_ref(n) ||_2                                   over the site's components
    S(n) = |a| d(n) ||psi(n)||_2 + |b| h sum_{+-mu} ||psi(n +- mu)||_2       h = 1 + r (Wilson: ||U||_2 = 1, ||r -+ gamma_mu||_2 = 1 + r), 1 (staggered)
                                                                             d(n) = 1, or ||A(n)||_F with a clover term
    K    = max_n e(n) / (u S(n)),   u = 2^-24

S(n) bounds the magnitude of everything that is summed into the site, so K counts roundings: the reference is the fp64 oracle on the UNROUNDED inputs,
i.e. the rounding of links and spinor to fp32 is part of what K bounds (0.25-0.27 of it on hot links and Gaussian spinors).  A single wrong hop, sign or
coefficient at a single site moves e(n) by O(S(n)) or O(1e-5 S(n)): K in the hundreds and above; a global max-norm ratio would hide it behind the largest site.

The restatement below is the plain evaluation (hop by hop, link times spinor, then the spin matrix) in `dtype` throughout: complex128 pins it to the oracle,
complex64 is the fp32 evaluation from which K_ASSERT is fixed (tests/test_cpu_f32_bound.py) -- never from a device result.

Fields are in the oracle's layout: U[mu,t,z,y,x,b,a] = U_mu^{ab}, Wilson psi[spin,t,z,y,x,c], staggered psi[t,z,y,x,c], clover A[t,z,y,x,12,12] (index spin*3+c)."""
import numpy as np

U_ROUND = 2.0 ** -24

# K_ASSERT = 6 x the largest K the complex64 restatement reaches over the lattices, boundary signs, couplings and D / D^+ of tests/test_gpu_f32_operators.py
# (measured values: DESIGN.md section 6, "The fp32 operators"; test_cpu_f32_bound.py asserts that the restatement stays a factor 5 below).  The factor 6 covers
# FMA contraction, another summation order and a third link row rebuilt from two rounded rows.
# measured maxima 0.6720 (Wilson, (16,8,8,4)), 0.7151 (clover, (8,4,6,8)), 1.4350 (staggered, (16,8,8,4)): 6 x those, rounded up in the third digit
K_ASSERT = {"wilson": 4.04, "clover": 4.30, "staggered": 8.62}

GAMMA = np.zeros((4, 4, 4), dtype=np.complex128)
GAMMA[0][0, 3] = -1j; GAMMA[0][1, 2] = -1j; GAMMA[0][2, 1] = 1j; GAMMA[0][3, 0] = 1j
GAMMA[1][0, 3] = -1; GAMMA[1][1, 2] = 1; GAMMA[1][2, 1] = 1; GAMMA[1][3, 0] = -1
GAMMA[2][0, 2] = -1j; GAMMA[2][1, 3] = 1j; GAMMA[2][2, 0] = 1j; GAMMA[2][3, 1] = -1j
GAMMA[3] = np.diag([1, 1, -1, -1])


def _real(dtype):
    return np.float32 if np.dtype(dtype) == np.complex64 else np.float64


def _face(arr, site_axis0, nu, idx, sign):
    """multiply the slice coordinate_nu = idx of a site array (site axes t,z,y,x starting at site_axis0) by a boundary sign"""
    if sign == 1:
        return
    sl = [slice(None)] * arr.ndim
    sl[site_axis0 + 3 - nu] = idx
    arr[tuple(sl)] *= sign


def _hops(U, psi, nu, bc, ax0, planted=None):
    """(U_nu(n) psi(n+nu), U_nu^+(n-nu) psi(n-nu)) with the boundary signs; psi has `ax0` leading non-site axes, colour last"""
    ax = ax0 + 3 - nu
    L = psi.shape[ax]
    Um = np.swapaxes(U[nu], -1, -2)                       # [t,z,y,x,a,b]
    pf = np.roll(psi, -1, axis=ax)
    sf = bc[nu]
    if planted and planted.get("flip_face") == nu:
        sf = -sf
    _face(pf, ax0, nu, L - 1, sf)
    fwd = np.einsum("...ab,...b->...a", Um, pf) if ax0 == 0 else np.einsum("...ab,s...b->s...a", Um, pf)
    loc = np.einsum("...ba,...b->...a", Um.conj(), psi) if ax0 == 0 else np.einsum("...ba,s...b->s...a", Um.conj(), psi)
    bwd = np.roll(loc, 1, axis=ax)
    _face(bwd, ax0, nu, 0, bc[nu])
    return fwd, bwd


def wilson_D_np(U, psi, kappa, r=1.0, bc=(1, 1, 1, -1), dagger=False, dtype=np.complex128, A=None, planted=None):
    """Wilson (A is None) or Wilson-clover D psi = diag psi - kappa sum_nu [(r - g_nu) U psi(n+nu) + (r + g_nu) U^+ psi(n-nu)], D^+: g -> -g.
    planted: dict of deliberate errors for the self-test of the metric (see test_cpu_f32_bound.py)."""
    planted = planted or {}
    R = _real(dtype)
    U = U.astype(dtype); psi = psi.astype(dtype)
    k = R(kappa * planted.get("kappa_factor", 1.0))
    rr = R(r)
    sg = -1.0 if dagger else 1.0
    if planted.get("swap_dagger"):
        sg = -sg
    G = (sg * GAMMA).astype(dtype)
    acc = np.zeros_like(psi)
    for nu in range(4):
        fwd, bwd = _hops(U, psi, nu, bc, 1, planted)
        if planted.get("hop_site") is not None and nu == 0:
            fwd[(slice(None),) + tuple(planted["hop_site"])] *= R(1.0 + planted["hop_rel"])
        acc += rr * fwd - np.einsum("st,t...->s...", G[nu], fwd)
        acc += rr * bwd + np.einsum("st,t...->s...", G[nu], bwd)
    if A is None:
        diag = psi
    else:
        A = A.astype(dtype)
        if planted.get("clover_conj_site") is not None:
            A = A.copy()
            s = tuple(planted["clover_conj_site"])
            A[s + (0, 4)] = np.conj(A[s + (0, 4)])
        p12 = np.moveaxis(psi, 0, -2).reshape(psi.shape[1:5] + (12,))
        diag = np.moveaxis(np.einsum("...ij,...j->...i", A, p12).reshape(psi.shape[1:5] + (4, 3)), -2, 0)
    return (diag - k * acc).astype(dtype)


def staggered_D_np(U, psi, mass, bc=(1, 1, 1, -1), dagger=False, dtype=np.complex128, planted=None):
    """m psi + (+-)1/2 sum_nu eta_nu [U psi(n+nu) - U^+ psi(n-nu)], eta_nu = (-1)^(x_0 + .. + x_{nu-1})"""
    planted = planted or {}
    R = _real(dtype)
    U = U.astype(dtype); psi = psi.astype(dtype)
    T, Z, Y, X = psi.shape[:4]
    c = [np.arange(X).reshape(1, 1, 1, X), np.arange(Y).reshape(1, 1, Y, 1), np.arange(Z).reshape(1, Z, 1, 1), np.arange(T).reshape(T, 1, 1, 1)]
    acc = np.zeros_like(psi)
    for nu in range(4):
        e = np.zeros((T, Z, Y, X), dtype=np.int64)
        for kk in range(nu):
            e = e + c[kk]
        eta = np.where(e & 1, -1.0, 1.0).astype(R)[..., None]
        if planted.get("flip_phase") == nu:
            eta = -eta
        fwd, bwd = _hops(U, psi, nu, bc, 0, planted)
        if planted.get("hop_site") is not None and nu == 0:
            fwd[tuple(planted["hop_site"])] *= R(1.0 + planted["hop_rel"])
        acc += eta * (fwd - bwd)
    hs = R(-0.5 if dagger else 0.5)
    if planted.get("swap_dagger"):
        hs = -hs
    return (R(mass * planted.get("kappa_factor", 1.0)) * psi + hs * acc).astype(dtype)


def site_norm(f, comp_axes):
    return np.sqrt((np.abs(f.astype(np.complex128)) ** 2).sum(axis=comp_axes))


def site_scale(psi, a, b, h, comp_axes, d=None):
    """S(n): psi in the oracle layout, comp_axes its non-site axes; d: per-site norm of the diagonal block (None: 1)"""
    nrm = site_norm(psi, comp_axes)                       # [t,z,y,x]
    nb = np.zeros_like(nrm)
    for ax in range(4):
        nb += np.roll(nrm, 1, axis=ax) + np.roll(nrm, -1, axis=ax)
    return abs(a) * (nrm if d is None else d * nrm) + abs(b) * h * nb


def site_K(out, ref, S, comp_axes):
    e = site_norm(np.asarray(out, dtype=np.complex128) - ref, comp_axes)
    return float((e / (U_ROUND * S)).max())


W_AXES, S_AXES = (0, 5), (4,)


def wilson_K(out, ref, psi, kappa, r=1.0, A=None):
    d = None if A is None else np.sqrt((np.abs(A) ** 2).sum(axis=(-1, -2)))
    return site_K(out, ref, site_scale(psi, 1.0, kappa, 1.0 + r, W_AXES, d), W_AXES)


def staggered_K(out, ref, psi, mass):
    return site_K(out, ref, site_scale(psi, mass, 0.5, 1.0, S_AXES), S_AXES)


# ---------------------------------------------------------------------------------------------- the hand-off of the mixed-precision solvers
def no_handoff(lat, what=""):
    """the last mixed-precision solve on this lattice reached eps by fp32 corrections alone (read-only keys mixed_handoffs, mixed_fp64_iters): a wrong or inaccurate
    inner operator ends in the fp64 solver with the right answer, and only these keys say so"""
    h, it = lat.get_param("mixed_handoffs"), lat.get_param("mixed_fp64_iters")
    print("mixed_handoffs %d mixed_fp64_iters %d %s" % (h, it, what))
    assert h == 0 and it == 0, ("a mixed-precision solve handed off to the fp64 solver", what, h, it)


def planned_steps(eps, rr0):
    """correction steps lqcd_solve_mixed_cg_DdagD plans at |r|^2 = rr0 (mixed.hip): one per 1e-12 of |r|^2 still to go"""
    import math
    return max(1, math.ceil(math.log(eps / rr0) / math.log(1e-12) - 1e-9))
