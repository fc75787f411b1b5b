"""Several right-hand sides (include/lqcd_hip.h "several right-hand sides"; csrc/stencil_mrhs.hip, csrc/bicgstab_eo_mrhs.hip): the multi-column parity hop and
operator against the CPU oracle, the independence of the columns bit for bit, the batched even-odd BiCGStab on columns that stop at different iterations against
the oracle and the single-column solver, non-convergence, the fall-backs (bitwise the single-column entries), the refusals, and the meson table with
meson_mrhs = 1 against meson_mrhs = 0.

Tolerances are the project's: 1e-13 for an operator application against the oracle (the Dslash tolerance), solutions 1e-9 to the oracle and 1e-10 to the
single-column solve, iteration counts +-1 (tests/test_gpu_solver_edges.py), true residual |D x - b|^2 < 1e-18 at eps = 1e-19, the meson table
1e-8 C_15(t) (tests/test_gpu_meson.py)."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from conftest import ROOT, rel_err

pytestmark = pytest.mark.gpu
KAPPA = 0.12
TOL = 1e-13
BCS = [(1, 1, 1, -1), (1, 1, 1, 1), (-1, 1, -1, 1)]
HOP_CASES = [((4, 4, 4, 8), n) for n in (1, 2, 3, 4, 5, 12)] + [(L, n) for L in ((8, 4, 4, 4), (16, 8, 4, 4)) for n in (4, 5)]


@pytest.fixture(scope="module")
def gpu():
    import latticeqcd_jl_amd as lq
    if lq.lib.device_count() < 1:
        pytest.skip("no HIP device")
    return lq


_cache = {}


def _links(orc, L, seed=111):
    if ("U", L, seed) not in _cache:
        _cache["U", L, seed] = orc.hot_gauge(L, seed)
    return _cache["U", L, seed]


def _col(orc, L, j):
    """Gaussian column j of lattice L (distinct seeds)."""
    if ("c", L, j) not in _cache:
        _cache["c", L, j] = orc.gaussian_spinor(orc.wilson_shape(L), 300 + j)
    return _cache["c", L, j]


def _ref_hop(orc, Uh, key, L, j, bc, dag, p):
    k = ("h", key, L, j, bc, dag, p)
    if k not in _cache:
        _cache[k] = orc.wilson_hop_parity(Uh, _col(orc, L, j), L, 1.0, bc, dag, p)
    return _cache[k]


def _ref_D(orc, Uh, L, j, bc, dag):
    k = ("D", L, j, bc, dag)
    if k not in _cache:
        _cache[k] = orc.wilson_D(Uh, _col(orc, L, j), L, KAPPA, 1.0, bc, dag)
    return _cache[k]


def _op(lq, U, bc=(1, 1, 1, -1), **kw):
    p = {"Dirac_operator": "Wilson", "κ": KAPPA, "r": 1.0, "boundarycondition": bc, "eps_CG": 1e-19, "MaxCGstep": 3000, "method_CG": "bicgstab_evenodd"}
    p.update(kw)
    return lq.Dirac_operator(U, None, p)


def _halves(lq, lat, orc, L, n, p):
    """n input columns of parity 1 - p and n output half-fields of parity p"""
    sub_out, sub_in = (lq.EVEN, lq.ODD) if p == 0 else (lq.ODD, lq.EVEN)
    xs = [lq.Fermionfields(lat, lq.WILSON, sub_in).upload(_col(orc, L, j)) for j in range(n)]
    ys = [lq.Fermionfields(lat, lq.WILSON, sub_out) for _ in range(n)]
    return xs, ys


# ---------------------------------------------------------------------------------- 1. hop and operator against the oracle
@pytest.mark.parametrize("L,n", HOP_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_hop_multi_against_the_oracle(gpu, orc, L, n):
    lq = gpu
    Uh = _links(orc, L)
    lat = lq.Lattice(L)
    U = lq.Gaugefields(lat).upload(Uh)
    worst = 0.0
    for bc in BCS:
        D = _op(lq, U, bc)
        for p in (0, 1):
            xs, ys = _halves(lq, lat, orc, L, n, p)
            for dag in (False, True):
                lq.hop_multi_(ys, D.adjoint() if dag else D, xs)
                assert lat.get_param("mrhs_active") >= 1 and lat.get_param("recon_active") == 1
                for j in range(n):
                    e = rel_err(ys[j].download(), _ref_hop(orc, Uh, "su3", L, j, bc, dag, p))
                    worst = max(worst, e)
                    assert e < TOL, (bc, p, dag, j, e)
    assert lat.get_param("mrhs_active") == min(n, 4)
    print(L, n, "hop_multi: worst rel_err to the oracle", worst)


@pytest.mark.parametrize("L", [(4, 4, 4, 8), (8, 4, 4, 4), (16, 8, 4, 4)], ids=lambda L: "x".join(map(str, L)))
def test_apply_multi_against_the_oracle(gpu, orc, L):
    lq = gpu
    Uh = _links(orc, L)
    lat = lq.Lattice(L)
    U = lq.Gaugefields(lat).upload(Uh)
    worst = 0.0
    for n in (4, 5):
        xs = [lq.Fermionfields(lat, lq.WILSON).upload(_col(orc, L, j)) for j in range(n)]
        ys = [x.similar() for x in xs]
        for bc in BCS:
            D = _op(lq, U, bc)
            for dag in (False, True):
                lq.mul_multi_(ys, D.adjoint() if dag else D, xs)
                assert lat.get_param("mrhs_active") == 4
                for j in range(n):
                    e = rel_err(ys[j].download(), _ref_D(orc, Uh, L, j, bc, dag))
                    worst = max(worst, e)
                    assert e < TOL, (n, bc, dag, j, e)
    print(L, "apply_multi: worst rel_err to the oracle", worst)


def test_hop_multi_reads_all_18_reals_off_the_group(gpu, orc):
    """One link scaled by 1.001: the 12-real gate fails and the 18-real instances run."""
    lq = gpu
    L, n, bc = (4, 4, 4, 8), 5, (1, 1, 1, -1)
    Uh = _links(orc, L).copy()
    Uh[2, 3, 1, 2, 1] *= 1.001
    lat = lq.Lattice(L)
    U = lq.Gaugefields(lat).upload(Uh)
    D = _op(lq, U, bc)
    for p in (0, 1):
        xs, ys = _halves(lq, lat, orc, L, n, p)
        for dag in (False, True):
            lq.hop_multi_(ys, D.adjoint() if dag else D, xs)
            assert lat.get_param("recon_active") == 0 and lat.get_param("mrhs_active") == 4
            for j in range(n):
                assert rel_err(ys[j].download(), _ref_hop(orc, Uh, "scaled", L, j, bc, dag, p)) < TOL, (p, dag, j)
    xs = [lq.Fermionfields(lat, lq.WILSON).upload(_col(orc, L, j)) for j in range(n)]
    ys = [x.similar() for x in xs]
    lq.mul_multi_(ys, D, xs)
    assert lat.get_param("recon_active") == 0
    for j in range(n):
        assert rel_err(ys[j].download(), orc.wilson_D(Uh, _col(orc, L, j), L, KAPPA, 1.0, bc)) < TOL


# ---------------------------------------------------------------------------------- 2. columns are independent
def test_columns_are_independent_bit_for_bit(gpu, orc):
    lq = gpu
    L = (16, 8, 4, 4)
    lat = lq.Lattice(L)
    U = lq.Gaugefields(lat).upload(_links(orc, L))
    D = _op(lq, U)
    xs, ys = _halves(lq, lat, orc, L, 12, 0)
    before = [x.download() for x in xs]
    lq.hop_multi_(ys, D, xs)
    ref = [y.download() for y in ys]
    for x, b in zip(xs, before):
        assert np.array_equal(x.download(), b)          # inputs are never written
    # a column's bits do not depend on the number of columns of the call or on its slot in a launch
    for j in (0, 5, 11):
        lq.hop_multi_([ys[0]], D, [xs[j]])
        assert np.array_equal(ys[0].download(), ref[j]), j
    # two columns given the same input produce identical bits
    lq.hop_multi_(ys[:4], D, [xs[0], xs[1], xs[0], xs[2]])
    o = [y.download() for y in ys[:4]]
    assert np.array_equal(o[0], o[2]) and np.array_equal(o[0], ref[0]) and np.array_equal(o[3], ref[2])
    # reversing the column order reverses the outputs
    lq.hop_multi_(ys[:4], D, xs[3::-1])
    for j in range(4):
        assert np.array_equal(ys[j].download(), ref[3 - j]), j
    # the same for the full operator
    fx = [lq.Fermionfields(lat, lq.WILSON).upload(_col(orc, L, j)) for j in range(4)]
    fy = [x.similar() for x in fx]
    lq.mul_multi_(fy, D, fx)
    fref = [y.download() for y in fy]
    lq.mul_multi_(fy, D, fx[::-1])
    for j in range(4):
        assert np.array_equal(fy[j].download(), fref[3 - j]), j
        assert np.array_equal(fx[j].download(), _col(orc, L, j))


# ---------------------------------------------------------------------------------- 3. / 4. the batched solver
def _solver_columns(orc, L):
    g = _col(orc, L, 0)
    pt = np.zeros_like(g)
    pt[0, 0, 0, 0, 0, 0] = 1.0
    return [g, 1e3 * g, 1e-13 * g, pt, np.zeros_like(g)]


def _oracle_solves(orc, Uh, L, dag):
    k = ("s", L, dag)
    if k not in _cache:
        _cache[k] = [orc.wilson_bicgstab_eo(Uh, np.ascontiguousarray(b), L, KAPPA, 1.0, (1, 1, 1, -1), dag, eps=1e-19) for b in _solver_columns(orc, L)]
    return _cache[k]


@pytest.mark.parametrize("dag", [False, True], ids=["D", "Ddag"])
@pytest.mark.parametrize("L", [(4, 4, 4, 8), (16, 8, 8, 8)], ids=lambda L: "x".join(map(str, L)))
def test_solver_with_columns_that_stop_at_different_iterations(gpu, orc, L, dag):
    lq = gpu
    Uh = _links(orc, L)
    lat = lq.Lattice(L)
    U = lq.Gaugefields(lat).upload(Uh)
    D0 = _op(lq, U)
    D = D0.adjoint() if dag else D0
    cols = _solver_columns(orc, L)
    bs = [lq.Fermionfields(lat, lq.WILSON).upload(b) for b in cols]
    xs = [b.similar() for b in bs]
    for x in xs:
        lq.clear_fermion_(x)
    its, rrs = lq.solve_DinvX_multi_(xs, D, bs, return_info=True)
    assert lat.get_param("mrhs_active") == 4
    sol = [x.download() for x in xs]
    ref = _oracle_solves(orc, Uh, L, dag)
    lat.set_param("bicg_fused", 2)
    single = []
    for b in bs:
        x1 = b.similar()
        lq.clear_fermion_(x1)
        single.append((x1, lq.solve_DinvX_(x1, D, b, return_info=True)[0]))
    lat.set_param("bicg_fused", 4)
    print(L, "dagger" if dag else "plain", "iterations: multi", its, "oracle", [r[1] for r in ref], "single", [s[1] for s in single])
    assert len(set(its)) >= 3          # the counts really differ
    r = bs[0].similar()
    for j in range(5):
        xo, ito, _, st = ref[j]
        assert st == 0 and abs(its[j] - ito) <= 1 and abs(its[j] - single[j][1]) <= 1, (j, its[j], ito, single[j][1])
        e_o, e_s = rel_err(sol[j], xo), rel_err(sol[j], single[j][0].download())
        lq.mul_(r, D, xs[j])
        lq.add_fermion_(r, -1.0, bs[j])
        res = lq.dot(r, r).real
        print("  column", j, "rel_err to the oracle", e_o, "to the single solve", e_s, "|Dx - b|^2", res, "recursive", rrs[j])
        assert e_o < 1e-9 and e_s < 1e-10 and res < 1e-18 and rrs[j] < 1e-19, (j, e_o, e_s, res)
    for j in (2, 4):          # below eps from the start: no iteration, x_e = 0, x_o = b_o
        assert its[j] == 0 and single[j][1] == 0 and np.array_equal(sol[j], single[j][0].download())
    # inputs are never written; two calls give identical bits
    for b, c in zip(bs, cols):
        assert np.array_equal(b.download(), c)
    for x in xs:
        lq.clear_fermion_(x)
    its2, _ = lq.solve_DinvX_multi_(xs, D, bs, return_info=True)
    assert its2 == its
    for j in range(5):
        assert np.array_equal(xs[j].download(), sol[j]), j
    # n = 4: a permuted column order gives bitwise the same per-column solutions and counts
    perm = [2, 0, 3, 1]
    for x in xs:
        lq.clear_fermion_(x)
    itp, _ = lq.solve_DinvX_multi_(xs[:4], D, [bs[q] for q in perm], return_info=True)
    for slot, q in enumerate(perm):
        assert itp[slot] == its[q] and np.array_equal(xs[slot].download(), sol[q]), (slot, q)


def test_solver_that_runs_out_of_iterations(gpu, orc):
    lq = gpu
    L = (4, 4, 4, 8)
    lat = lq.Lattice(L)
    U = lq.Gaugefields(lat).upload(_links(orc, L))
    D = _op(lq, U, MaxCGstep=3)
    bs = [lq.Fermionfields(lat, lq.WILSON).upload(b) for b in _solver_columns(orc, L)]
    xs = [b.similar() for b in bs]
    for x in xs:
        lq.clear_fermion_(x)
    with pytest.raises(lq.NotConverged) as ei:
        lq.solve_DinvX_multi_(xs, D, bs)
    assert ei.value.code == lq.lib.ERR_NOT_CONVERGED
    assert ei.value.iters == [3, 3, 0, 3, 0], ei.value.iters
    for x in xs:
        assert np.isfinite(x.download()).all()
    assert all(np.isfinite(v) for v in ei.value.final_rr)


# ---------------------------------------------------------------------------------- 5. fall-backs: bitwise the single-column entries
def _fallback_body(lq, orc, L, **opkw):
    lat = lq.Lattice(L)
    if os.environ.get("LQCD_FORCE_PARTITION"):
        lat.comm_init(lq.comm_unique_id())
    U = lq.Gaugefields(lat).upload(orc.hot_gauge(L, 111))
    D = _op(lq, U, **opkw)
    g = orc.gaussian_spinor(orc.wilson_shape(L), 300)
    pt = np.zeros_like(g)
    pt[0, 0, 0, 0, 0, 0] = 1.0
    cols = [g, pt, orc.gaussian_spinor(orc.wilson_shape(L), 301)]
    for p, (so, si) in enumerate(((lq.EVEN, lq.ODD), (lq.ODD, lq.EVEN))):
        xs = [lq.Fermionfields(lat, lq.WILSON, si).upload(c) for c in cols]
        ys = [lq.Fermionfields(lat, lq.WILSON, so) for _ in cols]
        lq.hop_multi_(ys, D, xs)
        assert lat.get_param("mrhs_active") == 0
        y1 = ys[0].similar()
        for x, y in zip(xs, ys):
            lq.hop_(y1, D, x)
            assert np.array_equal(y1.download(), y.download())
    bs = [lq.Fermionfields(lat, lq.WILSON).upload(c) for c in cols]
    ys = [b.similar() for b in bs]
    lq.mul_multi_(ys, D, bs)
    assert lat.get_param("mrhs_active") == 0
    y1 = bs[0].similar()
    for b, y in zip(bs, ys):
        lq.mul_(y1, D, b)
        assert np.array_equal(y1.download(), y.download())
    for x in ys:
        lq.clear_fermion_(x)
    its, _ = lq.solve_DinvX_multi_(ys, D, bs, return_info=True)
    assert lat.get_param("mrhs_active") == 0
    for j, b in enumerate(bs):
        lq.clear_fermion_(y1)
        it1, _ = lq.solve_DinvX_(y1, D, b, return_info=True)
        assert it1 == its[j] and np.array_equal(y1.download(), ys[j].download()), j


@pytest.mark.parametrize("case", ["Vh288", "r0.8", "clover"])
def test_fallbacks_are_the_single_column_entries(gpu, orc, case):
    if case == "Vh288":
        _fallback_body(gpu, orc, (6, 6, 4, 4))
    elif case == "r0.8":
        _fallback_body(gpu, orc, (4, 4, 4, 8), r=0.8)
    else:
        _fallback_body(gpu, orc, (4, 4, 4, 8), Dirac_operator="WilsonClover", Clover_coefficient=1.3)


def test_fallback_on_a_self_partitioned_lattice(gpu):
    """One RCCL self-partition (LQCD_FORCE_PARTITION = 8: the t direction) in a process of its own."""
    code = textwrap.dedent("""
        import os, sys
        sys.path.insert(0, os.getcwd())
        sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
        import latticeqcd_jl_amd as lq
        from oracle import oracle as orc
        import test_gpu_mrhs as t
        t._fallback_body(lq, orc, (4, 4, 4, 8))
        print("MRHS_SELF_PARTITION_OK")
    """)
    env = dict(os.environ, LQCD_FORCE_PARTITION="8", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "MRHS_SELF_PARTITION_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


# ---------------------------------------------------------------------------------- 6. refusals, outputs untouched
def _arr(fields):
    return (C.c_void_p * len(fields))(*[f._h for f in fields])


def test_refusals_leave_the_outputs_untouched(gpu, orc):
    lq = gpu
    lib = lq.lib.lib()
    L = (4, 4, 4, 8)
    lat, lat2 = lq.Lattice(L), lq.Lattice(L)
    U = lq.Gaugefields(lat).upload(_links(orc, L))
    D = _op(lq, U)
    mark = _col(orc, L, 7)
    full = lambda la=lat: lq.Fermionfields(la, lq.WILSON).upload(mark)
    ev = lambda: lq.Fermionfields(lat, lq.WILSON, lq.EVEN).upload(mark)
    od = lambda: lq.Fermionfields(lat, lq.WILSON, lq.ODD).upload(mark)
    fo, fi = [full(), full()], [full(), full()]
    eo, oi = [ev(), ev()], [od(), od()]
    it, rr = (C.c_int * 13)(), (C.c_double * 13)()
    entries = {
        "hop": lambda op, n, o, i: lib.lqcd_op_hop_multi(op, n, o, i, 0),
        "apply": lambda op, n, o, i: lib.lqcd_op_apply_multi(op, n, o, i, 0),
        "solve": lambda op, n, o, i: lib.lqcd_solve_bicgstab_eo_multi(op, n, o, i, 0, C.c_double(1e-19), 100, it, rr),
    }
    good = {"hop": (eo, oi), "apply": (fo, fi), "solve": (fo, fi)}
    touched = fo + eo

    def untouched():
        return all(np.array_equal(f.download(), ref) for f, ref in zip(touched, snapshot))

    snapshot = [f.download() for f in touched]
    ARG, UNS = lq.lib.ERR_ARG, lq.lib.ERR_UNSUPPORTED
    stag_lat = lat
    other = full(lat2)
    Ds = lq.Dirac_operator(U, None, {"Dirac_operator": "staggered", "mass": 0.1})
    Ddw = lq.Dirac_operator(U, None, {"Dirac_operator": "Domainwall", "mass": 0.25, "M": -1.0, "L5": 4})
    sf = [lq.Fermionfields(stag_lat, lq.STAGGERED), lq.Fermionfields(stag_lat, lq.STAGGERED)]
    for name, call in entries.items():
        o, i = good[name]
        assert call(None, 2, _arr(o), _arr(i)) == ARG, name                              # null operator
        assert call(D._h, 2, None, _arr(i)) == ARG and call(D._h, 2, _arr(o), None) == ARG, name
        assert call(D._h, 2, (C.c_void_p * 2)(o[0]._h, None), _arr(i)) == ARG, name      # null column
        assert call(D._h, 0, _arr(o), _arr(i)) == ARG and call(D._h, -1, _arr(o), _arr(i)) == ARG, name
        big_o, big_i = (C.c_void_p * 13)(*([o[0]._h] * 13)), (C.c_void_p * 13)(*([i[0]._h] * 13))
        assert call(D._h, 13, big_o, big_i) == ARG, name                                 # n > LQCD_MRHS_MAX
        assert call(D._h, 2, _arr([o[0], o[0]]), _arr(i)) == ARG, name                   # duplicate outputs
        assert b"distinct" in lib.lqcd_last_error()
        assert call(D._h, 2, _arr(o), _arr([i[0], other])) == ARG, name             # mixed contexts
        assert call(D._h, 2, _arr(o), _arr([i[0], sf[0]])) == ARG, name                  # wrong kind
        wrong = (fo, fi) if name == "hop" else (eo, oi)                                  # wrong subset
        assert call(D._h, 2, _arr(wrong[0]), _arr(wrong[1])) == ARG, name
        assert call(Ds._h, 2, _arr(o), _arr(i)) == UNS and b"staggered" in lib.lqcd_last_error(), name
        assert call(Ddw._h, 2, _arr(o), _arr(i)) == UNS and b"Domainwall" in lib.lqcd_last_error(), name
    # hop: the two subsets must be opposite, and the same for every column
    assert entries["hop"](D._h, 2, _arr(eo), _arr([oi[0], eo[1]])) == ARG
    assert entries["hop"](D._h, 2, _arr([eo[0], oi[1]]), _arr([oi[0], eo[1]])) == ARG
    # an output that is also an input of another column
    assert entries["apply"](D._h, 2, _arr(fo), _arr([fi[0], fo[0]])) == ARG
    # input columns may repeat
    assert entries["apply"](D._h, 2, _arr(fi), _arr([fo[0], fo[0]])) == lq.lib.OK
    assert untouched()
    # an in-process PE grid
    lats = [lq.Lattice((4, 4, 4, 16), (1, 1, 1, 2), rk) for rk in range(2)]
    lq.link_local(lats)
    Up = lq.Gaugefields(lats[0]).upload(orc.hot_gauge(lats[0].local_L, 5))
    Dp = _op(lq, Up)
    po = [lq.Fermionfields(lats[0], lq.WILSON), lq.Fermionfields(lats[0], lq.WILSON)]
    pi = [lq.Fermionfields(lats[0], lq.WILSON), lq.Fermionfields(lats[0], lq.WILSON)]
    for f in po:
        lq.gauss_distribution_fermion_(f, 9)
    snap = [f.download() for f in po]
    for name in ("apply", "solve"):
        assert entries[name](Dp._h, 2, _arr(po), _arr(pi)) == UNS and b"PE grid" in lib.lqcd_last_error(), name
    pe, pod = [lq.Fermionfields(lats[0], lq.WILSON, lq.EVEN)], [lq.Fermionfields(lats[0], lq.WILSON, lq.ODD)]
    assert entries["hop"](Dp._h, 1, _arr(pe), _arr(pod)) == UNS
    assert all(np.array_equal(f.download(), s) for f, s in zip(po, snap))


# ---------------------------------------------------------------------------------- 7. the meson table on the batched solver
@pytest.mark.parametrize("L,src", [((4, 4, 4, 8), (0, 0, 0, 0)), ((4, 4, 4, 8), (1, 2, 3, 5)), ((8, 8, 8, 16), (0, 0, 0, 0)), ((8, 8, 8, 16), (3, 0, 5, 9))],
                         ids=lambda v: "x".join(map(str, v)))
def test_meson_table_with_the_batched_solver(gpu, orc, L, src):
    lq = gpu
    lat = lq.Lattice(L)
    assert lat.get_param("meson_mrhs") == 0 and lat.get_param("mrhs_active") == 0          # fresh context: the default does not move
    U = lq.Gaugefields(lat).upload(_links(orc, L))
    D = _op(lq, U)
    tab0, it0 = lq.meson_correlators(D, src, return_info=True)
    assert lat.get_param("mrhs_active") == 0
    lat.set_param("meson_mrhs", 1)
    tab1, it1 = lq.meson_correlators(D, src, return_info=True)
    assert lat.get_param("mrhs_active") == 4
    pion1 = lq.pion_correlator(D, src)
    lat.set_param("meson_mrhs", 0)
    err = float((np.abs(tab1 - tab0) / tab0[15]).max())
    print(L, src, "max |C(mrhs) - C| / C_15 =", err, "iterations", it0, it1)
    assert err <= 1e-8
    assert all(abs(a - b) <= 1 for a, b in zip(it0, it1)), (it0, it1)
    assert np.array_equal(pion1, tab1[15])
    assert np.array_equal(lq.meson_correlators(D, src), tab0)                              # and back: the single solves' bits
