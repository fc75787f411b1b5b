"""How a solve ends: the case table and the oracle-side selection of the stopping thresholds (tests/test_cpu_solve_endings.py: the reference side;
tests/test_gpu_solve_endings.py: the device side).  No GPU here.

Every other solver test compares a solution with the oracle at eps = 1e-16 .. 1e-24 and accepts 1e-8 .. 1e-10: the update of the LAST iteration is
below the tolerance there, and a solve that lost it passes.  The rows here stop a solve at a chosen iteration k with an eps placed in the middle
(geometrically) of the two residuals it has to separate, loose enough that the last update and the truncation error are five decades above the
1e-10 the device solution is held to:

    rr_{k-1}, rr_k   the oracle's recursive residuals after k-1 and k iterations (eps = 1e-300, maxiter = k-1 and k)
    ss_k             BiCGStab cores: |s|^2 of iteration k, seen as the residual the oracle returns at eps = 0.999 rr_{k-1} when it stops at it == k
                     with a value other than rr_k -- the half-step exit of bicgstab_core
    mode "full"      eps = sqrt(rr_{k-1} rr_k), or sqrt(ss_k rr_k) where a half step exists: the solve ends behind the whole iteration k
    mode "half"      eps = sqrt(rr_{k-1} ss_k): the solve ends in the half step of iteration k (x += alpha p only)

The scalars are committed as tests/golden/solve_endings.json (tests/golden/make_solve_endings.py); the solutions are recomputed by the tests.
The oracle's CG sums in thread order, so the table is bound to hard_systems.THREADS like the hard-system fixture.
"""
import json
import os

import numpy as np

import hard_systems as hs

THREADS = hs.THREADS
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solve_endings.json")
BC = (1, 1, 1, -1)
KAPPA, MASS, CSW = 0.141139, 0.5, 1.5612
DW = {"L5": 2, "M": -1.0, "mass": 0.25}      # L5 = 2: the smallest fifth dimension the Domainwall tests use
GAUGE_SEED, SOURCE_SEED = 971, 972
SHIFTS = (0.01, 0.1, 1.0, 10.0)
COLUMN_SCALES = (1.0, 1e-2, 1e2, 0.0)
S, P, Q, B, F, T = (8, 8, 8, 8), (8, 4, 6, 4), (6, 6, 4, 2), (16, 16, 16, 12), (32, 16, 16, 18), (4, 4, 4, 8)
R = (16, 8, 8, 4)      # the volume of S with x-y planes of whole 64-site chunks: the smallest shape on which the residual ring, the temporal-gauge CG and the fp32 site-pair kernel run
MARGIN, VISIBLE, TIGHT = 1.2, 1e-5, 1e-22


def _row(op, solver, L, k, mode="full", dagger=False, mass=None):
    name = "%s_%s%s_%s_k%d_%s%s" % (op, solver, "_dag" if dagger else "", ".".join(str(v) for v in L), k, mode, "" if mass is None else "_m%g" % mass)
    return name, dict(name=name, op=op, solver=solver, L=tuple(L), k=k, mode=mode, dagger=dagger, mass=MASS if mass is None else mass)


def _table():
    """Where the k or mass first planned for a row does not qualify (tests/test_cpu_solve_endings.py: the conditions) the row stands at another, never
    exempted.  On 4.4.4.8 the staggered BiCG / BiCGStab residuals at mass 0.5 are not monotone (rr_1 > rr_0, rr_5 > rr_4: an eps between two of them is
    met earlier) and no iteration has a half step below rr_{k-1}: those rows stand at mass 2.  Wilson BiCG meets the eps of k = 5 at iteration 2
    (k = 6).  6.6.4.2 D half steps: k = 2 is 1.16 from its threshold, 4 has none, at 6 the truncation error (7.7e-6) is not visible: k = 3, 5.
    16.16.16.12 D^+: the residual RISES in iteration 2, which also hides the half step of iteration 3 from the selection: k = 4, whole and half.
    Clover D^+ k = 5 has no half step (k = 6)."""
    rows = []
    for k in (3, 5, 6, 9):      # below, no multiple of and above the polling burst of 8; every residue mod the ring of 4; odd and even
        rows += [_row("wilson", "cg", S, k), _row("staggered", "cg", S, k), _row("wilson", "cg", P, k), _row("wilson", "cg", R, k)]
    rows += [_row("clover", "cg", P, 5), _row("domainwall", "cg", P, 5)]
    for dagger in (False, True):
        for k in (2, 5):
            rows += [_row("wilson", "bicgstab", T, k, "full", dagger), _row("wilson", "bicgstab", T, k, "half", dagger)]
            rows += [_row("staggered", "bicg", T, k, "full", dagger, 2.0), _row("staggered", "bicgstab", T, k, "full", dagger, 2.0), _row("staggered", "bicgstab", T, k, "half", dagger, 2.0)]
        for k in (2, 6):
            rows += [_row("wilson", "bicg", T, k, "full", dagger)]
    eo = {(S, False): ((2, 3, 5), (2, 3, 5)), (S, True): ((2, 3, 5), (2, 3, 5)), (Q, False): ((2, 3, 5), (3, 5)), (Q, True): ((2, 3, 5), (2, 3, 5)),
          (B, False): ((2, 3), (2, 3)), (B, True): ((4,), (4,))}      # (lattice, dagger): (k of the full rows, k of the half rows); B: k <= 4 keeps the oracle short
    for (L, dagger), (full, half) in eo.items():
        rows += [_row("wilson", "bicgstab_eo", L, k, "full", dagger) for k in full] + [_row("wilson", "bicgstab_eo", L, k, "half", dagger) for k in half]
    for dagger, half in ((False, (2, 3, 5)), (True, (2, 3, 6))):
        rows += [_row("clover", "bicgstab_eo", S, k, "full", dagger) for k in (2, 3, 5)] + [_row("clover", "bicgstab_eo", S, k, "half", dagger) for k in half]
    rows += [_row("wilson", "bicgstab_eo", F, 3, "full")]      # 1152 dot partials > 1024: the merged launch with a.fold == 2
    for op in ("wilson", "staggered"):
        for k in (5, 9):
            rows += [_row(op, "multishift", S, k)]
    return dict(rows)


ROWS = _table()
_memo = {}


def row(name):
    return ROWS[name]


def names(solver=None, op=None, L=None):
    return [n for n, r in ROWS.items() if (solver is None or r["solver"] == solver) and (op is None or r["op"] == op) and (L is None or r["L"] == tuple(L))]


def fixture():
    if "fixture" not in _memo:
        with open(FIXTURE) as f:
            _memo["fixture"] = json.load(f)
    return _memo["fixture"]


def eps_of(name):
    return fixture()[name]["eps"]


# ------------------------------------------------------------------ the systems
def gauge(orc, L):
    L = tuple(L)
    if ("U", L) not in _memo:
        Uh = orc.hot_gauge(L, GAUGE_SEED)
        Uh.setflags(write=False)
        _memo["U", L] = Uh
    return _memo["U", L]


def clover(orc, L):
    L = tuple(L)
    if ("A", L) not in _memo:
        _memo["A", L] = orc.clover_build(gauge(orc, L), L, KAPPA, CSW)
    return _memo["A", L]


def shape(orc, r):
    if r["op"] == "staggered":
        return orc.staggered_shape(r["L"])
    if r["op"] == "domainwall":
        return (DW["L5"],) + orc.wilson_shape(r["L"])
    return orc.wilson_shape(r["L"])


def rhs(orc, r):
    key = ("b", r["op"] == "staggered", r["op"] == "domainwall", r["L"])
    if key not in _memo:
        b = orc.gaussian_spinor(shape(orc, r), SOURCE_SEED)
        b.setflags(write=False)
        _memo[key] = b
    return _memo[key]


def apply_A(orc, r, x):
    """The operator of the row's FULL system by the oracle: D^+D for the CG rows, D or D^+ for the others."""
    L, Uh = r["L"], gauge(orc, r["L"])
    x = np.ascontiguousarray(x)
    if r["op"] == "domainwall":
        return orc.domainwall_D(Uh, orc.domainwall_D(Uh, x, L, DW["M"], DW["mass"], BC), L, DW["M"], DW["mass"], BC, dagger=True)
    if r["op"] == "clover":
        D = lambda v, dg: orc.wilson_clover_D(Uh, clover(orc, L), v, L, KAPPA, 1.0, BC, dg)
    elif r["op"] == "wilson":
        D = lambda v, dg: orc.wilson_D(Uh, v, L, KAPPA, 1.0, BC, dg)
    else:
        D = lambda v, dg: orc.staggered_D(Uh, v, L, r["mass"], BC, dg)
    if r["solver"] in ("cg", "multishift"):
        return D(D(x, False), True)
    return D(x, bool(r["dagger"]))


def true_rr(orc, r, x, sigma=0.0, b=None):
    """|b - (A + sigma) x|^2 formed by the oracle."""
    x = np.ascontiguousarray(x)
    res = (rhs(orc, r) if b is None else b) - apply_A(orc, r, x)
    if sigma:
        res = res - sigma * x
    return float(np.vdot(res, res).real)


def solve(orc, r, eps, maxiter=3000, b=None):
    """The oracle's solver of the row from a zero guess at THREADS threads: (x, iterations, recursive residual, status); a multi-shift row returns
    (x, [x_sigma], iterations, residual, status)."""
    L, Uh = r["L"], gauge(orc, r["L"])
    b = rhs(orc, r) if b is None else b
    kind, km = (orc.STAGGERED, r["mass"]) if r["op"] == "staggered" else (orc.WILSON, KAPPA)
    before = orc.lib().orc_get_threads()
    orc.set_threads(THREADS)
    try:
        s, op, dg = r["solver"], r["op"], bool(r["dagger"])
        if s == "multishift":
            return orc.multishift_cg(kind, Uh, b, L, km, list(SHIFTS), 1.0, BC, eps=eps, maxiter=maxiter)
        if s == "cg" and op == "domainwall":
            x, it, rr = orc.domainwall_cg(Uh, b, L, DW["M"], DW["mass"], BC, eps=eps, maxiter=maxiter)
            return x, it, float(rr), 0 if rr < eps else 1
        if s == "cg" and op == "clover":
            return orc.cg_clover(Uh, clover(orc, L), b, L, KAPPA, 1.0, BC, eps=eps, maxiter=maxiter)
        if s == "cg":
            return orc.cg_DdagD(kind, Uh, b, L, km, 1.0, BC, eps=eps, maxiter=maxiter)
        if s == "bicg":
            return orc.bicg(kind, Uh, b, L, km, 1.0, BC, dg, eps=eps, maxiter=maxiter)
        if s == "bicgstab":
            return orc.bicgstab(kind, Uh, b, L, km, 1.0, BC, dg, eps=eps, maxiter=maxiter)
        if s == "bicgstab_eo" and op == "clover":
            return orc.wilson_clover_bicgstab_eo(Uh, clover(orc, L), b, L, KAPPA, 1.0, BC, dg, eps=eps, maxiter=maxiter)
        if s == "bicgstab_eo":
            return orc.wilson_bicgstab_eo(Uh, b, L, KAPPA, 1.0, BC, dg, eps=eps, maxiter=maxiter)
        raise KeyError(s)
    finally:
        orc.set_threads(before)


def capped(orc, r, k):
    """(x_k, rr_k): the oracle's iterate and recursive residual after exactly k iterations."""
    out = solve(orc, r, 1e-300, k)
    return out[0], float(out[-2])


def select(orc, r):
    """The scalars of the row from the oracle alone (what tests/golden/solve_endings.json holds)."""
    k = r["k"]
    rr_km1, rr_k = capped(orc, r, k - 1)[1], capped(orc, r, k)[1]
    ss_k = None
    if r["solver"] in ("bicgstab", "bicgstab_eo"):
        probe = solve(orc, r, 0.999 * rr_km1)
        if probe[-3] == k and float(probe[-2]) != rr_k:
            ss_k = float(probe[-2])
    if r["mode"] == "half":
        eps = float(np.sqrt(rr_km1 * ss_k)) if ss_k is not None else None
    else:
        eps = float(np.sqrt((rr_km1 if ss_k is None else ss_k) * rr_k))
    return {"k": k, "eps": eps, "rr_km1": rr_km1, "rr_k": rr_k, "ss_k": ss_k}


def separated(r, sc):
    """(upper, lower): the two residuals the row's eps separates."""
    if r["mode"] == "half":
        return sc["rr_km1"], sc["ss_k"]
    return (sc["rr_km1"] if sc["ss_k"] is None else sc["ss_k"]), sc["rr_k"]


def reference(orc, name):
    """The oracle's solve of the row at the fixture's eps: (x, iterations, residual) [multi-shift: (x, [x_sigma], iterations, residual)], memoised
    and read-only -- the tests share it."""
    if ("ref", name) not in _memo:
        out = solve(orc, ROWS[name], eps_of(name))
        assert out[-1] == 0, (name, out[-1])
        for a in ([out[0]] + list(out[1])) if ROWS[name]["solver"] == "multishift" else [out[0]]:
            a.setflags(write=False)
        _memo["ref", name] = out[:-1]
    return _memo["ref", name]


def rel_err(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


BATCHED_ROW = "wilson_bicgstab_eo_8.8.8.8_k3_full"      # its eps is the batched solve's: columns c_j b, c = COLUMN_SCALES
MIXED_ROWS = ("wilson_cg_8.8.8.8_k9_full", "wilson_cg_16.8.8.4_k9_full")      # their eps is the mixed-precision solves'
