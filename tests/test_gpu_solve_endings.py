"""How every solver ENDS, against the oracle (tests/solve_endings.py: the rows and how their eps is chosen; tests/test_cpu_solve_endings.py: the
reference side; tests/golden/solve_endings.json: the scalars).

The other solver tests run at eps = 1e-16 .. 1e-24 and accept 1e-8 .. 1e-10, where the last iteration's update of x is below the tolerance: a final
update that some workgroups skip, a deferred-x or residual ring flushed one term short, a half-step exit with the wrong update, launches behind the
converging one that are not quite no-ops, a shift or column frozen one step off, an exhausted solve whose x is not the iterate it claims -- none of
them shows.  Here every solve stops at a chosen iteration k of a LOOSE eps (the last update and the truncation error are >= 1e-5 of x), and

    1. it == k exactly; reported rr < eps and |rr - rr_oracle| <= 1e-8 rr_oracle
    2. rel_err(x, x_oracle) < 1e-10
    3. t^2 = |b - A x|^2 formed by the oracle, |t^2 - rr| <= 1e-6 rr.  A workgroup's share of the vector is >= 1/1024; missing the last update there
       moves t^2 by >= (rr_{k-1} / rr_k - 1) / 1024 >= 2e-4, rounding stays below 1e-10: two decades on either side.  The even-odd solves report the
       residual of the Schur system, which IS the full system's for plain Wilson (x_o is exact); Wilson-clover preconditions it with A_ee^-1, so
       t^2 is compared with the oracle's own t^2 there.

16.16.16.12 is the smallest lattice on which the streaming kernels of the even-odd BiCGStab reach their grid cap of 1024 workgroups -- more than one
residency round, where the merged update launch (bicg_fused = 4) used to test at entry the done flag its own lead workgroup raises.

8.8.8.8 and 8.4.6.4 cannot run the residual ring, the temporal-gauge CG or the fp32 site-pair kernel (their x-y planes are not whole 64-site chunks:
cg_rring_active, tgauge_active, pair32_active stay 0 there whatever is asked for), so the CG rows and the mixed-precision cases also stand on
16.8.8.4, the same volume, where all three run.  cg_tgauge = 1 does not take the temporal-gauge path on lattices of <= 1024 stencil workgroups;
2 does, and is what "on" means below.

Measured on the MI355X: 97 tests in 12 s; every row passes, the largest rel err of x against the oracle is below 1e-12 and |t^2 - rr| / rr below 1e-9.
The 16.16.16.12 rows also passed once with the library as it was before the merged launch got its own entry flag: whether a late workgroup sees the
lead's store is a matter of timing, and nothing here tries to force it -- the rows guard the ending, the entry test was fixed on the code.
"""

import numpy as np
import pytest

import solve_endings as se

pytestmark = pytest.mark.gpu

_NAMES = {"wilson": "Wilson", "clover": "WilsonClover", "staggered": "Staggered", "domainwall": "Domainwall"}


# ------------------------------------------------------------------ helpers
def device(lq, orc, r, eps, tunables=(), method=None, maxit=3000):
    """A fresh context with the row's links, operator and right-hand side: (lat, D, b)."""
    lat = lq.Lattice(r["L"])
    for k, v in tunables:
        lat.set_param(k, v)
    U = lq.Gaugefields(lat).upload(se.gauge(orc, r["L"]))
    p = {"Dirac_operator": _NAMES[r["op"]], "κ": se.KAPPA, "mass": r["mass"], "boundarycondition": se.BC, "eps_CG": eps, "MaxCGstep": maxit}
    if r["op"] == "clover":
        p["Clover_coefficient"] = se.CSW
    if method:
        p["method_CG"] = method
    if r["op"] == "domainwall":
        p.update({"mass": se.DW["mass"], "L5": se.DW["L5"], "M": se.DW["M"]})
        b = lq.Initialize_pseudofermion_fields(U[1], "Domainwall", L5=se.DW["L5"], nowing=True)
        D = lq.Dirac_operator(U, b, p)
    else:
        D = lq.Dirac_operator(U, None, p)
        b = lq.Fermionfields(lat, lq.STAGGERED if r["op"] == "staggered" else lq.WILSON)
    b.upload(np.array(se.rhs(orc, r)))
    return lat, D, b


def operator(lq, r, D):
    if r["solver"] in ("cg", "multishift"):
        return lq.DdagD_operator(D)
    Dd = D.adjoint() if r["dagger"] else D
    Dd.method_CG = {"bicg": "bicg", "bicgstab": "bicgstab", "bicgstab_eo": "bicgstab_evenodd"}[r["solver"]]
    return Dd


def run(lq, A, b):
    x = b.similar()
    lq.clear_fermion_(x)
    it, rr = lq.solve_DinvX_(x, A, b, return_info=True)
    return x.download(), it, rr


_t2_ref = {}


def held(orc, name, xh, it, rr, label, fails):
    """The three assertions for one device solve of the row; misses are appended to fails with their figures."""
    r, eps = se.row(name), se.eps_of(name)
    xo, ito, rro = se.reference(orc, name)[0], se.reference(orc, name)[-2], se.reference(orc, name)[-1]
    t2 = se.true_rr(orc, r, xh)
    if r["op"] == "clover" and r["solver"] == "bicgstab_eo":
        if name not in _t2_ref:
            _t2_ref[name] = se.true_rr(orc, r, xo)
        against = _t2_ref[name]
    else:
        against = rr
    err = se.rel_err(xh, xo)
    print("%s %s: it %d (oracle %d) rr %.10e (oracle %.10e, eps %.4e) rel err x %.3e true rr %.10e (against %.10e)" % (name, label, it, ito, rr, rro, eps, err, t2, against))
    ok = it == ito == r["k"] and rr < eps and abs(rr - rro) <= 1e-8 * rro and err < 1e-10 and abs(t2 - against) <= 1e-6 * against
    if not ok:
        fails.append("%s %s: it %d (k %d) rr %.10e (oracle %.10e, eps %.4e) rel err x %.3e true rr %.10e against %.10e" % (name, label, it, r["k"], rr, rro, eps, err, t2, against))


# ------------------------------------------------------------------ 1. CG on D^+D
# (id, tunables, cg_rring_active)
CG_FORMS = [
    ("reference", (("cg_small", 0), ("cg_fused", 0)), 0),
    ("norm_fused", (("cg_small", 0), ("cg_fused", 1)), 0),
    ("fused", (("cg_small", 0), ("cg_fused", 2), ("cg_defer_x", 0)), 0),
    ("defer_x1", (("cg_small", 0), ("cg_fused", 2), ("cg_defer_x", 1)), 0),
    ("defer_x4", (("cg_small", 0), ("cg_fused", 2), ("cg_defer_x", 4)), 0),
    ("small", (("cg_small", 1), ("cg_fused", 2), ("cg_defer_x", 4)), 0),
    ("rring4", (("cg_small", 0), ("cg_fused", 3), ("cg_rring", 4)), 4),
]


@pytest.mark.parametrize("name", se.names("cg", "wilson") + se.names("cg", "staggered"))
def test_cg_forms(lq, orc, name):
    r = se.row(name)
    lat, D, b = device(lq, orc, r, se.eps_of(name), (("cg_persist", 0),))
    A, fails = operator(lq, r, D), []
    special = r["op"] == "wilson" and r["L"] == se.R      # the ring and the temporal gauge run here
    for form, tun, K in CG_FORMS:
        for k, v in tun:
            lat.set_param(k, v)
        for tg in (0, 2) if special else (0,):
            lat.set_param("cg_tgauge", tg)
            for graph in (0, 1):
                lat.set_param("graph", graph)
                xh, it, rr = run(lq, A, b)
                assert lat.get_param("cg_rring_active") == (K if special else 0) and lat.get_param("tgauge_active") == (1 if tg and special else 0), (form, tg, graph)
                assert lat.get_param("cg_persist") == 0 and lat.get_param("graph") == graph
                held(orc, name, xh, it, rr, "%s tgauge %d graph %d" % (form, tg, graph), fails)
    lat.set_param("cg_tgauge", 0)
    lat.set_param("graph", 0)
    if r["op"] == "staggered":      # the one-launch form
        lat.set_param("cg_persist", 1)
        xh, it, rr = run(lq, A, b)
        assert lat.get_param("cg_persist") == 1      # (it switches itself off when it gives up)
        held(orc, name, xh, it, rr, "cg_persist 1", fails)
    assert np.array_equal(b.download(), se.rhs(orc, r))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("name", se.names("cg", "clover") + se.names("cg", "domainwall"))
def test_cg_clover_and_domainwall(lq, orc, name):
    r = se.row(name)
    lat, D, b = device(lq, orc, r, se.eps_of(name))
    fails = []
    xh, it, rr = run(lq, operator(lq, r, D), b)
    held(orc, name, xh, it, rr, "defaults", fails)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ 2. BiCG and BiCGStab on the full lattice
@pytest.mark.parametrize("name", se.names("bicg") + se.names("bicgstab"))
def test_bicg_and_bicgstab(lq, orc, name):
    r = se.row(name)
    lat, D, b = device(lq, orc, r, se.eps_of(name))
    fails = []
    xh, it, rr = run(lq, operator(lq, r, D), b)
    held(orc, name, xh, it, rr, r["mode"], fails)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ 3. even-odd BiCGStab
# (id, tunables, bicg_xrp_active on a lattice that takes the fused chain)
EO_FORMS = [
    ("generic", (("bicg_fused", 0),), 0),
    ("unfolded", (("bicg_fused", 1),), 0),
    ("fused2", (("bicg_fused", 2),), 0),
    ("merged_guard6", (("bicg_fused", 4), ("bicg_rec_guard", 6)), 2),
    ("merged_guard0", (("bicg_fused", 4), ("bicg_rec_guard", 0)), 2),      # the stopping test is deferred one kernel
]


@pytest.mark.parametrize("name", [n for n in se.names("bicgstab_eo") if se.row(n)["L"] != se.B])
def test_evenodd_bicgstab_forms(lq, orc, name):
    r = se.row(name)
    lat, D, b = device(lq, orc, r, se.eps_of(name))
    A, fails = operator(lq, r, D), []
    chain = (np.prod(r["L"]) // 2) % 64 == 0      # 6.6.4.2: the un-fused generic chain whatever bicg_fused says
    for form, tun, xrp in EO_FORMS if r["L"] != se.F else EO_FORMS[3:4]:
        for k, v in tun:
            lat.set_param(k, v)
        xh, it, rr = run(lq, A, b)
        if chain and tun[0][1]:
            assert lat.get_param("bicg_xrp_active") == xrp, form
        held(orc, name, xh, it, rr, form, fails)
    assert np.array_equal(b.download(), se.rhs(orc, r))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dagger", [False, True], ids=["D", "Ddag"])
def test_evenodd_bicgstab_where_the_streaming_grid_is_capped(lq, orc, dagger):
    """16.16.16.12: 1152 chunks of 256 elements on a grid capped at 1024 workgroups.  Every form on every row; then, for the merged update launch
    (bicg_fused = 4, the default), the loose solve again (i) after a tight solve with the same operator -- bicg_hint then enqueues some forty
    iterations behind the converging one, and they must change nothing -- and (ii) directly after that loose solve, the done flag of the last solve
    still raised at entry."""
    rows = [n for n in se.names("bicgstab_eo", "wilson", se.B) if se.row(n)["dagger"] == dagger]
    assert rows
    r = se.row(rows[0])
    lat, D, b = device(lq, orc, r, 1.0)
    A, fails = operator(lq, r, D), []
    for name in rows:
        A.eps_CG = se.eps_of(name)
        for form, tun, xrp in EO_FORMS:
            for k, v in tun:
                lat.set_param(k, v)
            xh, it, rr = run(lq, A, b)
            if tun[0][1]:
                assert lat.get_param("bicg_xrp_active") == xrp, form
            held(orc, name, xh, it, rr, form, fails)
    lat.set_param("bicg_fused", 4)
    lat.set_param("bicg_rec_guard", 6)
    for name in rows:
        A.eps_CG = 1e-19
        xh, it_tight, rr = run(lq, A, b)
        assert rr < 1e-19 and it_tight >= se.row(name)["k"] + 8      # (12 to 14 iterations here: the first burst of the next solve is that long)
        A.eps_CG = se.eps_of(name)
        for label in ("behind a tight solve of %d iterations" % it_tight, "behind a loose solve"):
            xh, it, rr = run(lq, A, b)
            assert lat.get_param("bicg_xrp_active") == 2
            held(orc, name, xh, it, rr, "merged_guard6 " + label, fails)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ 4. exhausted BiCGStab: x is the iterate of the last iteration
@pytest.mark.parametrize("k", [1, 3, 4, 5])
def test_an_exhausted_bicgstab_returns_the_iterate_it_stopped_at(lq, orc, k):
    """MaxCGstep = k, eps 1e-30: NotConverged, and x is the oracle's iterate after exactly k iterations -- all of it: the even-odd entry point
    reconstructs the odd half also on non-convergence."""
    cases = [("wilson", "bicgstab", se.T, ()), ("wilson", "bicgstab_eo", se.S, (("bicg_fused", 2),)), ("wilson", "bicgstab_eo", se.S, (("bicg_fused", 4),))]
    fails = []
    for op, solver, L, tun in cases:
        r = se._row(op, solver, L, k)[1]
        lat, D, b = device(lq, orc, r, 1e-30, tun, maxit=k)
        A = operator(lq, r, D)
        x = b.similar()
        lq.clear_fermion_(x)
        with pytest.raises(lq.NotConverged):
            lq.solve_DinvX_(x, A, b)
        xo, rro = se.capped(orc, r, k)
        err = se.rel_err(x.download(), xo)
        print("%s %s k %d: rel err of the exhausted iterate %.3e" % (solver, tun, k, err))
        if not err < 1e-10:
            fails.append("%s %s k %d: %.3e" % (solver, tun, k, err))
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ 5. multi-shift CG: the shifts freeze at different iterations
@pytest.mark.parametrize("name", se.names("multishift"))
def test_multishift(lq, orc, name):
    r, eps = se.row(name), se.eps_of(name)
    lat, D, b = device(lq, orc, r, eps)
    A = operator(lq, r, D)
    xs = [b.similar() for _ in se.SHIFTS]
    x = b.similar()
    it, rr = lq.shiftedcg(xs, list(se.SHIFTS), x, A, b, return_info=True)
    xo, xso, ito, rro = se.reference(orc, name)
    errs = [se.rel_err(x.download(), xo)] + [se.rel_err(xj.download(), xjo) for xj, xjo in zip(xs, xso)]
    print("%s: it %d (oracle %d) rr %.10e (oracle %.10e) rel err sigma 0 and %s: %s" % (name, it, ito, rr, rro, se.SHIFTS, ["%.3e" % e for e in errs]))
    assert it == ito == r["k"] and rr < eps and abs(rr - rro) <= 1e-8 * rro
    assert max(errs) < 1e-10, errs
    for j, sigma in enumerate(se.SHIFTS):      # a shifted system is frozen once zeta^2 rr < eps: its true residual obeys eps
        assert se.true_rr(orc, r, xs[j].download(), sigma) < eps * (1 + 1e-6), sigma


# ------------------------------------------------------------------ 6. the batched even-odd BiCGStab: columns that end at different iterations
def test_batched_bicgstab_columns_end_at_their_own_iteration(lq, orc):
    name = se.BATCHED_ROW
    r, eps = se.row(name), se.eps_of(name)
    lat, D, b = device(lq, orc, r, eps, method="bicgstab_evenodd")
    cols = [c * se.rhs(orc, r) for c in se.COLUMN_SCALES]
    bs = [lq.Fermionfields(lat, lq.WILSON).upload(c) for c in cols]
    xs = [c.similar() for c in bs]
    for x in xs:
        lq.clear_fermion_(x)
    its, rrs = lq.solve_DinvX_multi_(xs, D, bs, return_info=True)
    assert lat.get_param("mrhs_active") == 4
    fails = []
    for j, c in enumerate(se.COLUMN_SCALES):
        xh = xs[j].download()
        if c == 0.0:
            assert its[j] == 0 and rrs[j] == 0.0 and not xh.any()
            continue
        xo, ito, rro, st = se.solve(orc, r, eps, b=cols[j])
        err, t2 = se.rel_err(xh, xo), se.true_rr(orc, r, xh, b=cols[j])
        print("column %d (scale %g): it %d (oracle %d) rr %.10e (oracle %.10e) rel err %.3e true rr %.10e" % (j, c, its[j], ito, rrs[j], rro, err, t2))
        if not (st == 0 and its[j] == ito and rrs[j] < eps and abs(rrs[j] - rro) <= 1e-8 * rro and err < 1e-10 and abs(t2 - rrs[j]) <= 1e-6 * rrs[j]):
            fails.append("column %d: it %d (oracle %d) rr %.10e (oracle %.10e) rel err %.3e true rr %.10e" % (j, its[j], ito, rrs[j], rro, err, t2))
    assert len({its[j] for j in range(3)}) == 3, its
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ 7. mixed precision: other iterates, the same contract at the end
def _mixed_held(orc, r, xh, eps, label, xo_eps, x_tight):
    t2 = se.true_rr(orc, r, xh)
    err, ref = se.rel_err(xh, x_tight), se.rel_err(xo_eps, x_tight)
    print("%s: true rr %.6e (eps %.6e), error against the tight solution %.3e, the oracle's fp64 solve at this eps %.3e: ratio %.3f" % (label, t2, eps, err, ref, err / ref))
    assert t2 < eps * (1 + 1e-6), (label, t2, eps)
    assert err <= 4.0 * ref, (label, err, ref, err / ref)


@pytest.mark.parametrize("pair32", [0, 1])
@pytest.mark.parametrize("name", se.MIXED_ROWS)
def test_mixed_cg(lq, orc, name, pair32):
    r, eps = se.row(name), se.eps_of(name)
    lat, D, b = device(lq, orc, r, eps, (("mixed_pair32", pair32),))
    x = b.similar()
    lq.clear_fermion_(x)
    it, outer, rr = lq.solve_mixed_DinvX_(x, lq.DdagD_operator(D), b, return_info=True)
    assert lat.get_param("pair32_active") == (pair32 if r["L"] == se.R else 0) and rr < eps
    tight = se.solve(orc, r, se.TIGHT)
    assert tight[-1] == 0
    _mixed_held(orc, r, x.download(), eps, "mixed cg %s pair32 %d (%d inner, %d outer, reported %.4e)" % (r["L"], pair32, it, outer, rr), se.reference(orc, name)[0], tight[0])


@pytest.mark.parametrize("links16", [0, 1])
@pytest.mark.parametrize("name", se.MIXED_ROWS)
def test_mixed_evenodd_bicgstab(lq, orc, name, links16):
    eps = se.eps_of(name)
    r = se._row("wilson", "bicgstab_eo", se.row(name)["L"], 0)[1]
    lat, D, b = device(lq, orc, r, eps, (("bicg_mixed", 1), ("mixed_links16", links16)))
    xh, it, rr = run(lq, operator(lq, r, D), b)
    assert lat.get_param("pair32_active") == (1 if r["L"] == se.R else 0) and rr < eps
    xo, ito, rro, st = se.solve(orc, r, eps)
    tight = se.solve(orc, r, se.TIGHT)
    assert st == 0 and tight[-1] == 0
    _mixed_held(orc, r, xh, eps, "bicg_mixed %s links16 %d (%d iterations, reported %.4e)" % (r["L"], links16, it, rr), xo, tight[0])
