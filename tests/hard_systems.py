"""Ill-conditioned solver systems and the accuracy contract they are tested under (tests/test_cpu_hard_system_reference.py, tests/test_gpu_hard_solves.py).

Every other solver test of the suite runs on a hot gauge field far from kappa_c, where D^+D is so well conditioned that a CG stops after ~76 iterations.
The systems here are the ones light quarks on smooth configurations give: the links are one molecular-dynamics step of size 0.2 away from the unit field
(exactly SU(3), plaquette 0.8987 at 16.8.8.4), the boundary condition is periodic in all four directions (antiperiodic t at T = 4 lifts the spectrum),
kappa sits just below kappa_c (staggered: mass 0.005) and eps = 1e-16.  The solution is 10^3 .. 10^4 times the right-hand side in norm and a solve
takes several hundred to 1800 iterations, so the rounding of a solver's recurrences shows.

The contract.  For a solution x with reported residual rr_rep, t = |b - A x| formed by the oracle:

    t <= sqrt(rr_rep) + allowance      and      rr_rep < eps
    allowance = 8 max(C_ref, 0.25) u |A| |x|,      u = 2^-53
    |A| = (1 + 8 kappa)^2 for D^+D, 1 + 8 kappa for D and D^+, m^2 + 16 for staggered D^+D, + sigma for a shifted system
    C_ref = (t_ref - sqrt(rr_ref)) / (u |A| |x_ref|)  of the oracle's textbook solver on the same row (tests/golden/hard_systems.json)

which is the attainable-accuracy limit of a Krylov method with a recursive residual (the gap between the true and the recursive residual is the rounding
of the x and r updates, of order u |A| |x| times a modest constant); 8 is a margin for forms that carry several recurrences.  `t^2 < eps` is NOT the
contract: the oracle itself misses it on one of the 32.4.8.4 rows (at THREADS = 8 on wilson_cg_32: recursive 9.6e-17, true 1.03e-16).  A shifted system of a multi-shift solve reports no residual of its own -- it is
frozen once zeta^2 rr < eps -- so sqrt(eps) stands for sqrt(rr_rep) there.

The oracle's CG sums in thread order: its iterates are deterministic for a given thread count, THREADS, which the fixture and its test share.
"""
import json
import os

import numpy as np

U_ROUND = 2.0 ** -53
THREADS = 8
EPS = 1e-16
PERIODIC = (1, 1, 1, 1)
SHIFTS = (1e-4, 1e-3, 1e-2, 0.1)
GAUGE = {"momenta_seed": 5, "step": 0.2}
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hard_systems.json")

# solver: cg = CG on D^+D, multishift = multi-shift CG on D^+D + sigma, bicgstab_eo = even-odd BiCGStab on D (dagger: D^+)
# source: a Gaussian of the given seed, "point" = 1 in component 0, "even" = the Gaussian with its odd sites cleared; x0_seed: a Gaussian initial guess
SYSTEMS = {
    "wilson_cg_16": dict(kind="wilson", solver="cg", L=(16, 8, 8, 4), kappa=0.1285, bc=PERIODIC, source="gauss", seed=7, eps=EPS),
    "wilson_cg_16_x0": dict(kind="wilson", solver="cg", L=(16, 8, 8, 4), kappa=0.1285, bc=PERIODIC, source="gauss", seed=7, x0_seed=777, eps=EPS),
    "wilson_cg_32": dict(kind="wilson", solver="cg", L=(32, 4, 8, 4), kappa=0.1285, bc=PERIODIC, source="gauss", seed=7, eps=EPS),
    "wilson_cg_32_k0128": dict(kind="wilson", solver="cg", L=(32, 4, 8, 4), kappa=0.128, bc=PERIODIC, source="gauss", seed=7, eps=EPS),
    "wilson_multishift_16": dict(kind="wilson", solver="multishift", L=(16, 8, 8, 4), kappa=0.1285, bc=PERIODIC, source="gauss", seed=7, eps=EPS,
                                 sigmas=SHIFTS),
    "wilson_eo_D_gauss": dict(kind="wilson", solver="bicgstab_eo", dagger=False, L=(16, 8, 8, 4), kappa=0.128, bc=PERIODIC, source="gauss", seed=7,
                              eps=EPS),
    "wilson_eo_Ddag_gauss": dict(kind="wilson", solver="bicgstab_eo", dagger=True, L=(16, 8, 8, 4), kappa=0.128, bc=PERIODIC, source="gauss", seed=7,
                                 eps=EPS),
    "wilson_eo_D_point": dict(kind="wilson", solver="bicgstab_eo", dagger=False, L=(16, 8, 8, 4), kappa=0.128, bc=PERIODIC, source="point", seed=None,
                              eps=EPS),
    "staggered_cg_16": dict(kind="staggered", solver="cg", L=(16, 8, 8, 4), mass=0.005, bc=PERIODIC, source="gauss", seed=9, eps=EPS),
    "staggered_cg_16_even": dict(kind="staggered", solver="cg", L=(16, 8, 8, 4), mass=0.005, bc=PERIODIC, source="even", seed=9, eps=EPS),
}
for _name, _s in SYSTEMS.items():
    _s["name"] = _name

_memo = {}


def system(name):
    return SYSTEMS[name]


def _kind(orc, sys):
    return orc.WILSON if sys["kind"] == "wilson" else orc.STAGGERED


def _km(sys):
    return sys["kappa"] if sys["kind"] == "wilson" else sys["mass"]


def shape(orc, sys):
    return orc.wilson_shape(sys["L"]) if sys["kind"] == "wilson" else orc.staggered_shape(sys["L"])


def even_mask(L):
    """True on the even sites of a [t, z, y, x] grid."""
    t, z, y, x = np.meshgrid(range(L[3]), range(L[2]), range(L[1]), range(L[0]), indexing="ij")
    return ((x + y + z + t) & 1) == 0


def gauge(orc, sys):
    """The links of the row (shared by all rows of a shape): one exact-exponential link update of step 0.2 from the unit field.  Nobody writes them."""
    L = tuple(sys["L"])
    if ("U", L) not in _memo:
        Uh = orc.link_update(orc.unit_gauge(L), orc.gaussian_momenta(L, GAUGE["momenta_seed"]), GAUGE["step"], L)
        Uh.setflags(write=False)
        _memo["U", L] = Uh
    return _memo["U", L]


def rhs(orc, sys):
    k = ("b", sys["name"])
    if k not in _memo:
        shp = shape(orc, sys)
        if sys["source"] == "point":
            b = np.zeros(shp, dtype=np.complex128)
            b.reshape(-1)[0] = 1.0
        else:
            b = orc.gaussian_spinor(shp, sys["seed"])
            if sys["source"] == "even":
                b.reshape((-1,) + even_mask(sys["L"]).shape + (3,))[:, ~even_mask(sys["L"]), :] = 0.0
        b.setflags(write=False)
        _memo[k] = b
    return _memo[k]


def guess(orc, sys):
    """The initial guess of the row: None (zero) or the Gaussian of x0_seed."""
    if sys.get("x0_seed") is None:
        return None
    k = ("x0", sys["name"])
    if k not in _memo:
        x0 = orc.gaussian_spinor(shape(orc, sys), sys["x0_seed"])
        x0.setflags(write=False)
        _memo[k] = x0
    return _memo[k]


def apply_A(orc, sys, x, sigma=0.0, dagger=None):
    """dagger None: (D^+D + sigma) x; False / True: D x / D^+ x -- by the oracle."""
    Uh, L, kind, km, bc = gauge(orc, sys), tuple(sys["L"]), _kind(orc, sys), _km(sys), tuple(sys["bc"])
    x = np.ascontiguousarray(x)
    if dagger is None:
        y = orc.apply_D(kind, Uh, orc.apply_D(kind, Uh, x, L, km, 1.0, bc), L, km, 1.0, bc, dagger=True)
        return y + sigma * x if sigma else y
    return orc.apply_D(kind, Uh, x, L, km, 1.0, bc, dagger=bool(dagger))


def true_rr(orc, sys, x, sigma=0.0, dagger=None, b=None):
    """|b - A x|^2 of a downloaded solution, A as in apply_A; b: another right-hand side than the row's (a scaled or masked column)."""
    res = (rhs(orc, sys) if b is None else b) - apply_A(orc, sys, x, sigma, dagger)
    return float(np.vdot(res, res).real)


def norm_A(sys, sigma=0.0, dagger=None):
    if sys["kind"] == "staggered":
        return sys["mass"] ** 2 + 16.0 + sigma
    n = 1.0 + 8.0 * sys["kappa"]
    return n * n + sigma if dagger is None else n


def _dagger_of(sys):
    return sys.get("dagger") if sys["solver"] == "bicgstab_eo" else None


def ratio(sys, t, rr_rep, xnorm, sigma=0.0):
    """(t - sqrt(rr_rep)) / (u |A| |x|): the constant a solve shows in the contract (C_ref for the oracle's)."""
    return (t - np.sqrt(rr_rep)) / (U_ROUND * norm_A(sys, sigma, _dagger_of(sys)) * xnorm) if xnorm > 0.0 else 0.0


def fixture():
    if "fixture" not in _memo:
        with open(FIXTURE) as f:
            _memo["fixture"] = json.load(f)
    return _memo["fixture"]


def c_ref(sys, shift=None):
    row = fixture()[sys["name"]]
    return row["C_ref"] if shift is None else row["shift_C_ref"][shift]


def allowance(sys, xnorm, sigma=0.0, shift=None, factor=8.0):
    """factor max(C_ref, 0.25) u |A| |x|; shift: the index of sigma in the row's shifts (its own C_ref)."""
    return factor * max(c_ref(sys, shift), 0.25) * U_ROUND * norm_A(sys, sigma, _dagger_of(sys)) * xnorm


def meets(sys, t2, rr_rep, xnorm, sigma=0.0, shift=None, factor=8.0, label=""):
    """Prints the figures of one solve and returns whether it meets the contract; t2 = |b - A x|^2 from true_rr.  A shifted system (shift is not None)
    is held to sqrt(eps) in place of its unreported residual."""
    t = float(np.sqrt(t2))
    rep = sys["eps"] if shift is not None else rr_rep
    c = ratio(sys, t, rep, xnorm, sigma)
    ok = t <= np.sqrt(rep) + allowance(sys, xnorm, sigma, shift, factor) and rr_rep < sys["eps"]
    print("%s %s reported rr %.4e true rr %.4e |x| %.4e ratio %.3f (C_ref %.3f, allowed %.2f)%s"
          % (sys["name"], label, rr_rep, t2, xnorm, c, c_ref(sys, shift), factor * max(c_ref(sys, shift), 0.25), "" if ok else "   <-- MISSES"))
    return bool(ok), float(c)


def reference(orc, sys):
    """The oracle's textbook solver on the row, at THREADS threads: the scalars of tests/golden/hard_systems.json (C_ref included).  The thread count is restored."""
    Uh, L, kind, km, bc = gauge(orc, sys), tuple(sys["L"]), _kind(orc, sys), _km(sys), tuple(sys["bc"])
    b, eps = rhs(orc, sys), sys["eps"]
    bnorm = float(np.linalg.norm(b))
    before = orc.lib().orc_get_threads()
    orc.set_threads(THREADS)
    try:
        if sys["solver"] == "cg":
            x, it, rr, st = orc.cg_DdagD(kind, Uh, b, L, km, 1.0, bc, eps=eps, maxiter=6000, x0=guess(orc, sys))
            shifted = []
        elif sys["solver"] == "multishift":
            x, xs, it, rr, st = orc.multishift_cg(kind, Uh, b, L, km, list(sys["sigmas"]), 1.0, bc, eps=eps, maxiter=6000)
            shifted = list(zip(sys["sigmas"], xs))
        else:
            x, it, rr, st = orc.wilson_bicgstab_eo(Uh, b, L, km, 1.0, bc, bool(sys["dagger"]), eps=eps, maxiter=6000)
            shifted = []
        assert st == 0, (sys["name"], st)
        dag = _dagger_of(sys)
        t2 = true_rr(orc, sys, x, 0.0, dag)
        xnorm = float(np.linalg.norm(x))
        row = {"iterations": int(it), "rr": float(rr), "true_rr": t2, "xnorm": xnorm, "bnorm": bnorm,
               "C_ref": float(ratio(sys, np.sqrt(t2), rr, xnorm))}
        if shifted:
            row["shift_true_rr"] = [true_rr(orc, sys, xj, s) for s, xj in shifted]
            row["shift_xnorm"] = [float(np.linalg.norm(xj)) for _, xj in shifted]
            row["shift_C_ref"] = [float(ratio(sys, np.sqrt(t), eps, n, s)) for (s, _), t, n in zip(shifted, row["shift_true_rr"], row["shift_xnorm"])]
    finally:
        orc.set_threads(before)
    return row
