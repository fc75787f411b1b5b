"""Worker of tests/test_gpu_peer_solvers.py: one of N real PROCESSES that share cuda:0 and communicate through the peer-mapped backend (csrc/comm.hip).  Run under
torch.distributed.run; gloo carries the window descriptions and the cross-rank comparisons of this file.  Every rank rebuilds the seeded inputs (tests/peer_refs.py),
loads the references the parent computed once on the GLOBAL lattice, cuts its part with lq.pegrid.local_view and runs the cases of its world.  No oracle solve here.

After every case every rank all-gathers its returned scalars (iteration counts, residuals, actions, dH, dot) and its count of peer reductions (read-only key
peer_reductions): the scalars must be BIT-equal on all ranks (the promise of peer_allreduce_wave: every rank adds the same values in the same order) and the counts
equal -- a rank-local decision that issues one reduction more or fewer is named at the case that made it.  The first failed assertion, LQCDError or exception prints
the case and the rank and leaves with os._exit(1): nothing is retried, nothing further is launched by this rank."""
import ctypes as C
import datetime
import os
import sys
import traceback

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import latticeqcd_jl_amd as lq  # noqa: E402
import peer_refs as pr  # noqa: E402

KAPPA, MASS, CSW = pr.KAPPA, pr.MASS, pr.CSW


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def gather_blobs(blob):
    mine = torch.tensor(list(blob), dtype=torch.uint8)
    out = [torch.empty_like(mine) for _ in range(dist.get_world_size())]
    dist.all_gather(out, mine)
    return [bytes(t.tolist()) for t in out]


def check(cond, *what):
    """every figure is printed before it is asserted (the parent shows a world's output when it fails)"""
    print("  rank %s: %s" % (os.environ.get("RANK", "?"), " ".join(("%.3e" % v) if isinstance(v, float) else str(v) for v in what)), flush=True)
    if not cond:
        raise AssertionError(what)


class World:
    """one rank's context: the lattice, the hot links on the device, the references, the scalars of the running case"""

    def __init__(self, lat, gL, ref):
        self.lat, self.gL, self.ref = lat, gL, ref
        self.scalars = []
        self.tag = None
        self.Uh = pr.gauge(gL)
        self.U = lq.Gaugefields(lat).upload(self.loc(self.Uh, 1))

    def loc(self, a, lead):
        return lq.pegrid.local_view(a, self.lat.local_L, self.lat.origin, lead=lead)

    def r(self, key, lead=None):
        """reference `key` of the running boundary condition (or of the gauge side): a scalar, or this rank's part of a field"""
        v = self.ref[("g" if self.tag is None else self.tag) + "/" + key]
        return v[()] if lead is None else self.loc(v, lead)

    def rec(self, *vals):
        self.scalars += [float(v) for v in vals]

    def reductions(self):
        return self.lat.get_param("peer_reductions")

    def fermion(self, kind, host, lead):
        return lq.Fermionfields(self.lat, kind).upload(self.loc(host, lead))

    def residual(self, A, sol, b, y):
        """|b - A sol|^2 through the device's fp64 operator: mul_ + add_fermion_ + dot"""
        lq.mul_(y, A, sol)
        lq.add_fermion_(y, -1.0, b)
        d = lq.dot(y, y).real
        self.rec(d)
        return d

    def no_handoff(self, what):
        """tests/f32_bound.py::no_handoff"""
        h, it = self.lat.get_param("mixed_handoffs"), self.lat.get_param("mixed_fp64_iters")
        check(h == 0 and it == 0, "a mixed-precision solve handed off to the fp64 solver", what, h, it)


def op(w, name, bc, **kw):
    p = {"Dirac_operator": name, "κ": KAPPA, "mass": MASS, "Clover_coefficient": CSW, "boundarycondition": bc, "eps_CG": 1e-19}
    p.update(kw)
    return lq.Dirac_operator(w.U, None, p)


def eo_solves(w, D, b, refcase, what, tol):
    """even-odd BiCGStab on D and D^+ against the oracle's even-odd BiCGStab: the unfused partitioned chain (bicgstab_core: bicg_xrp_active stays 0, every
    inner product is a peer reduction)"""
    sol, y = b.similar(), b.similar()
    for dag in (0, 1):
        Dd = D.adjoint() if dag else D
        lq.clear_fermion_(sol)
        r0 = w.reductions()
        it, rr = lq.solve_DinvX_(sol, Dd, b, return_info=True)
        nred = w.reductions() - r0
        w.rec(it, rr)
        check(w.lat.get_param("bicg_xrp_active") == 0 and nred >= it > 0, what, dag, "not the unfused partitioned chain", nred, it)
        e, ito = rel(sol.download(), w.r("%s/x%d" % (refcase, dag), 1)), int(w.r("%s/it%d" % (refcase, dag)))
        res = w.residual(Dd, sol, b, y)
        check(rr < 1e-19 and e <= tol and abs(it - ito) <= 2 and res < 1e-17, what, dag, it, ito, rr, e, res)


def case1(w, bc):
    """Even-odd BiCGStab, Wilson, D and D^+, bicg_fused 4 and 2, halo_stream_mode 3 and -1.  Bounds: test_gpu_clover.py::test_wilson_clover_operator_cg_and_force
    (solution <= 1e-9, iterations +-2, device residual < 1e-17), the same call on the plain Wilson operator."""
    D = op(w, "Wilson", bc, method_CG="bicgstab_evenodd")
    b = w.fermion(lq.WILSON, pr.wilson_rhs(w.gL), 1)
    for mode in (3, -1):
        w.lat.set_param("halo_stream_mode", mode)
        for fused in (4, 2):
            w.lat.set_param("bicg_fused", fused)
            eo_solves(w, D, b, "c1", ("mode", mode, "bicg_fused", fused), 1e-9)
    w.lat.set_param("bicg_fused", 4)


def case2(w, bc):
    """Plain BiCGStab (cg_op 3..6 on the peer path), Wilson and staggered, D and D^+.  Bounds: test_gpu_parity.py::test_bicgstab_and_evenodd_match_oracle (r.r < 1e-19,
    solution < 1e-8, true residual < 1e-17).  The staggered BiCGStab has no strict-eps single-domain test (tests/solve_endings.py runs it at loose eps): the Wilson bounds."""
    for name, kind, host, lead, key in (("Wilson", lq.WILSON, pr.wilson_rhs(w.gL), 1, "w"), ("Staggered", lq.STAGGERED, pr.staggered_rhs(w.gL), 0, "s")):
        D = op(w, name, bc, method_CG="bicgstab")
        b = w.fermion(kind, host, lead)
        sol, y = b.similar(), b.similar()
        for dag in (0, 1):
            Dd = D.adjoint() if dag else D
            lq.clear_fermion_(sol)
            r0 = w.reductions()
            it, rr = lq.solve_DinvX_(sol, Dd, b, return_info=True)
            nred = w.reductions() - r0
            w.rec(it, rr)
            e, ito = rel(sol.download(), w.r("c2/%s_x%d" % (key, dag), lead)), int(w.r("c2/%s_it%d" % (key, dag)))
            res = w.residual(Dd, sol, b, y)
            check(nred >= it > 0 and rr < 1e-19 and e < 1e-8 and res < 1e-17, name, dag, it, ito, nred, rr, e, res)


def case3(w, bc):
    """Wilson-clover: even-odd BiCGStab on D and D^+, calc_UdSfdU_, fermion_force_ from uploaded X, Y.  Bounds: test_gpu_clover.py::test_wilson_clover_operator_cg_and_force
    (solution <= 1e-9, iterations +-2, residual < 1e-17; S <= 1e-10 relative, force <= 1e-9; the sweep alone <= 1e-13)."""
    D = op(w, "WilsonClover", bc, method_CG="bicgstab_evenodd")
    b = w.fermion(lq.WILSON, pr.wilson_rhs(w.gL), 1)
    eo_solves(w, D, b, "c3", "clover", 1e-9)
    D.eps_CG = 1e-22
    G = lq.Gaugefields(w.lat)
    r0 = w.reductions()
    Sf = lq.calc_UdSfdU_(G, lq.FermiAction(D), w.U, b)
    w.rec(Sf)
    So, Go = float(w.r("c3/S")), w.r("c3/G", 1)
    e = rel(G.download(), Go)
    check(w.reductions() > r0 and abs(Sf - So) < 1e-10 * So and e < 1e-9, "clover action force", Sf, So, e)
    X, Y = w.fermion(lq.WILSON, w.ref[w.tag + "/c3/X"], 1), w.fermion(lq.WILSON, w.ref[w.tag + "/c3/Y"], 1)
    lq.fermion_force_(G, D, X, Y)
    e = rel(G.download(), Go)
    check(e < 1e-13, "clover force sweep from uploaded X, Y", e)


def case4(w, bc):
    """Mixed precision: solve_mixed_DinvX_ on D^+D, Wilson and Wilson-clover, and the even-odd BiCGStab under bicg_mixed = 1; mixed_links16 0 and 1; halo_stream_mode 3 and -1.
    Bounds: test_gpu_clover.py::test_wilson_clover_operator_cg_and_force / test_gpu_mixed.py (true r.r < 1e-19, solution <= 1e-8, no hand-off).  A partitioned lattice has
    no site-pair kernel and therefore no int16 links (pair32_geometry_ok): pair32_active == 0 says so under both values of mixed_links16; and its even-odd solve is the
    fp64 chain whatever bicg_mixed says (csrc/bicgstab_eo.hip `fused`): the case holds it to the bounds of the mixed chain and to the hand-off keys all the same."""
    b = w.fermion(lq.WILSON, pr.wilson_rhs(w.gL), 1)
    sol, y = b.similar(), b.similar()
    ops = [(name, op(w, name, bc), key) for name, key in (("Wilson", "w"), ("WilsonClover", "c"))]
    for mode in (3, -1):
        w.lat.set_param("halo_stream_mode", mode)
        for l16 in (0, 1):
            w.lat.set_param("mixed_links16", l16)
            for name, D, key in ops:
                A = lq.DdagD_operator(D)
                lq.clear_fermion_(sol)
                r0 = w.reductions()
                it, outer, rr = lq.solve_mixed_DinvX_(sol, A, b, return_info=True)
                nred = w.reductions() - r0
                w.rec(it, outer, rr)
                w.no_handoff(("mixed CG", name, mode, l16))
                e = rel(sol.download(), w.r("c4/%s_x" % key, 1))
                res = w.residual(A, sol, b, y)
                check(w.lat.get_param("pair32_active") == 0 and nred > outer >= 1, name, mode, l16, "pair32_active / reductions", nred, outer)
                check(rr < 1e-19 and res < 1e-19 and e <= 1e-8, "mixed CG", name, mode, l16, it, outer, rr, res, e)
            w.lat.set_param("bicg_mixed", 1)
            for name, D, key in ops:
                D.method_CG = "bicgstab_evenodd"
                eo_solves(w, D, b, "c1" if key == "w" else "c3", ("bicg_mixed", name, mode, l16), 1e-8)
                w.no_handoff(("bicg_mixed", name, mode, l16))
                check(w.lat.get_param("pair32_active") == 0, "bicg_mixed", name, "pair32_active")
            w.lat.set_param("bicg_mixed", 0)
    w.lat.set_param("mixed_links16", 0)


def case5(w, bc):
    """Multi-shift CG: shiftedcg and shiftedcg_mixed with 3 shifts, Wilson and staggered (test_gpu_parity.py::test_multishift_cg_matches_oracle: residual < 1e-20, iterations
    +-1, every solution <= 1e-9; test_gpu_mixed.py::test_mixed_multishift_matches_oracle: worst true residual < 1e-20, no hand-off, <= 1e-9), and the staggered rational
    action with Nf = 2 (test_gpu_rhmc.py::test_rational_action_and_force_match_oracle: action and its image <= 1e-10, force <= 1e-10; the heat bath, there an identity at
    1e-9, here the field itself at 1e-9).  The partial fractions are the scipy fit of tests/peer_refs.py, handed to the library."""
    sig = list(pr.SHIFTS)
    for name, kind, host, lead, key in (("Wilson", lq.WILSON, pr.wilson_rhs(w.gL), 1, "w"), ("Staggered", lq.STAGGERED, pr.staggered_rhs(w.gL), 0, "s")):
        D = op(w, name, bc)
        A = lq.DdagD_operator(D)
        b = w.fermion(kind, host, lead)
        xs, x0 = [b.similar() for _ in sig], b.similar()
        o0, oxs, oit = w.r("c5/%s_x0" % key, lead), w.r("c5/%s_xs" % key, lead + 1), int(w.r("c5/%s_it" % key))
        r0 = w.reductions()
        it, resid = lq.shiftedcg(xs, sig, x0, A, b, eps=1e-20, return_info=True)
        nred = w.reductions() - r0
        w.rec(it, resid)
        errs = [rel(x0.download(), o0)] + [rel(x.download(), ox) for x, ox in zip(xs, oxs)]
        check(nred >= it > 0 and resid < 1e-20 and abs(it - oit) <= 1 and max(errs) < 1e-9, "shiftedcg", name, it, oit, nred, resid, errs)
        for x in xs + [x0]:
            lq.clear_fermion_(x)
        r0 = w.reductions()
        it, outer, worst = lq.shiftedcg_mixed(xs, sig, x0, A, b, eps=1e-20, return_info=True)
        nred = w.reductions() - r0
        w.rec(it, outer, worst)
        w.no_handoff(("shiftedcg_mixed", name))
        errs = [rel(x0.download(), o0)] + [rel(x.download(), ox) for x, ox in zip(xs, oxs)]
        check(nred >= it > 0 and worst < 1e-20 and outer >= len(sig) and max(errs) < 1e-9, "shiftedcg_mixed", name, it, outer, nred, worst, errs)
    D = op(w, "Staggered", bc, eps_CG=1e-22)
    fa = lq.FermiAction(D, {"Nf": pr.NF})
    check(fa.rational and abs(fa.alpha - pr.NF / 8.0) < 1e-15, "not the rational action", fa.alpha)
    for which, name in ((0, "action"), (1, "md"), (2, "sampling")):
        f = w.ref[w.tag + "/c5/fit_" + name]
        n = (len(f) - 1) // 2
        fa._set_coeffs(which, (float(f[0]), f[1:1 + n], f[1 + n:]))
        a0, res, poles = fa._coeffs(which)
        check(a0 == f[0] and np.array_equal(res, f[1:1 + n]) and np.array_equal(poles, f[1 + n:]), "coefficients not taken", name)
    phi = w.fermion(lq.STAGGERED, pr.staggered_rhs(w.gL), 0)
    r0 = w.reductions()
    S = lq.evaluate_FermiAction(fa, w.U, phi)
    w.rec(S)
    So = float(w.r("c5/r_S"))
    e = rel(fa._temporary_fermionfields[0].download(), w.r("c5/r_y", 0))
    check(w.reductions() > r0 and abs(S - So) < 1e-10 * abs(S) and e < 1e-10, "rational action", S, So, e)
    G = lq.Gaugefields(w.lat)
    lq.calc_UdSfdU_(G, fa, w.U, phi)
    e = rel(G.download(), w.r("c5/r_G", 1))
    check(e < 1e-10, "rational force", e)
    eta = phi.similar()
    lq.sample_pseudofermions_(eta, w.U, fa, phi)
    e = rel(eta.download(), w.r("c5/r_eta", 0))
    check(e < 1e-9, "rational heat bath", e)


def case6(w, bc):
    """Domainwall, L5 = 4: mul_ on D and D^+ (test_gpu_domainwall.py::test_mul_matches_the_oracle, <= 1e-13), CG (::test_cg_solution_matches_the_oracle: r.r < 1e-19,
    iterations +-2, <= 1e-9), action and force (::test_action_heat_bath_and_force: <= 1e-10 relative, <= 1e-8)."""
    x = lq.Initialize_pseudofermion_fields(w.U[1], "Domainwall", L5=pr.DW_L5, nowing=True)
    D = lq.Dirac_operator(w.U, x, {"Dirac_operator": "Domainwall", "mass": pr.DW_MASS, "L5": pr.DW_L5, "M": pr.DW_M, "eps_CG": 1e-19, "MaxCGstep": 3000,
                                   "boundarycondition": bc})
    x.upload(w.loc(pr.dw_rhs(w.gL), 2))
    y = x.similar()
    for dag in (0, 1):
        lq.mul_(y, D.adjoint() if dag else D, x)
        e = rel(y.download(), w.r("c6/D%d" % dag, 2))
        check(w.lat.get_param("dw_active") == 0 and e < 1e-13, "domainwall mul_", dag, e)
    sol = x.similar()
    r0 = w.reductions()
    it, rr = lq.solve_DinvX_(sol, lq.DdagD_operator(D), x, return_info=True)
    nred = w.reductions() - r0
    w.rec(it, rr)
    e, ito = rel(sol.download(), w.r("c6/x", 2)), int(w.r("c6/it"))
    check(nred >= it > 0 and rr < 1e-19 and abs(it - ito) <= 2 and e < 1e-9, "domainwall CG", it, ito, nred, rr, e)
    D.eps_CG = 1e-22
    fa = lq.FermiAction(D, {})
    S = lq.evaluate_FermiAction(fa, w.U, x)
    w.rec(S)
    So = float(w.r("c6/S"))
    G = lq.Gaugefields(w.lat)
    lq.calc_UdSfdU_(G, fa, w.U, x)
    e = rel(G.download(), w.r("c6/G", 1))
    check(abs(S - So) < 1e-10 * So and e < 1e-8, "domainwall action force", S, So, e)


def case7(w, bc):
    """Stout, rho = 0.11: calc_smearedU <= 1e-13, lqcd_stout_backprop out of place and in place <= 1e-12 (test_gpu_stout.py::test_smearing_and_backpropagation_match_the_oracle,
    ::test_rccl_self_partition_stout)."""
    nn = lq.CovNeuralnet(w.U)
    nn.push_(lq.STOUT_Layer(["plaquette"], [pr.RHO], w.U))
    Uout, _, _ = lq.calc_smearedU(w.U, nn)
    e = rel(Uout.download(), w.r("c7/U", 1))
    check(w.lat.get_param("staple_form_active") == 3 and e < 1e-13, "calc_smearedU", e)
    Gs = w.loc(pr.stout_force_in(w.gL), 1)
    Gd, G = lq.Gaugefields(w.lat).upload(Gs), lq.Gaugefields(w.lat)
    ref = w.r("c7/G", 1)
    lq.lib.check(lq.lib.lib().lqcd_stout_backprop(G._h, Gd._h, w.U._h, C.c_double(pr.RHO)))
    e = rel(G.download(), ref)
    check(e < 1e-12 and np.array_equal(Gd.download(), Gs), "stout back-propagation, out of place", e)
    lq.lib.check(lq.lib.lib().lqcd_stout_backprop(Gd._h, Gd._h, w.U._h, C.c_double(pr.RHO)))
    e = rel(Gd.download(), ref)
    check(e < 1e-12 and np.array_equal(Gd.download(), G.download()), "stout back-propagation, in place", e)


def case8(w, bc):
    """Gauge side against tests/rect_numpy.py at the bounds of test_gpu_rect_action.py (force, action, fused momentum update: 1e-13), through the partitioned sweep
    (staple_form_active == 3).  The library REFUSES beta_rect != 0 on a partitioned lattice (csrc/rectangle.hip: the rectangles need a halo of depth 2;
    test_gpu_rect_action.py::test_partitioned_lattice_is_refused), so the plaquette term is what runs here (beta_rect = 0 in the restatement) and the refusal is pinned
    on every rank: LQCD_ERR_UNSUPPORTED, outputs untouched, no reduction issued -- the ranks stay in step."""
    G = lq.Gaugefields(w.lat)
    lq.gauge_force_(G, w.U, pr.BETA)
    e = rel(G.download(), w.r("c8/G", 1))
    check(w.lat.get_param("staple_form_active") == 3 and e < 1e-13, "gauge_force_", e)
    r0 = w.reductions()
    S = lq.evaluate_GaugeAction(w.U, pr.BETA)
    w.rec(S)
    So = float(w.r("c8/S"))
    check(w.reductions() > r0 and abs(S - So) < 1e-13 * abs(So), "evaluate_GaugeAction", S, So)
    Ph = w.loc(pr.momenta(w.gL), 1)
    P = lq.Gaugefields(w.lat).upload(Ph)
    w.lat.set_param("staple_form_active", -1)
    lq.P_update_(w.U, P, pr.FACTOR, pr.BETA)
    e = rel(P.download(), w.r("c8/P", 1))
    check(w.lat.get_param("staple_form_active") == 3 and e < 1e-13, "P_update_", e)
    bp, br = pr.RECT_REFUSED
    before, r0 = G.download(), w.reductions()
    for call in (lambda: lq.gauge_force_(G, w.U, bp, beta_rect=br), lambda: lq.evaluate_GaugeAction(w.U, bp, beta_rect=br), lambda: lq.P_update_(w.U, G, pr.FACTOR, bp, beta_rect=br)):
        try:
            call()
            raise AssertionError("a rectangle entry point ran on a partitioned lattice")
        except lq.LQCDError as err:
            check(err.code == lq.lib.ERR_UNSUPPORTED and "partitioned" in str(err), "rectangle refusal", str(err))
    check(np.array_equal(G.download(), before) and w.reductions() == r0, "a refused call wrote or reduced")


def case9(w, bc):
    """Two leapfrog steps of the 2-flavour Wilson HMC through the plain API, the sequence of test_gpu_hmc_partitioned.py::_single with dtau = 0.05, against the same sequence
    on the oracle's primitives (tests/oracle_md.py); the momenta are the oracle's, uploaded.  Bounds of that test: links <= 1e-10, momenta <= 1e-9, dH <= 1e-7."""
    U0, P0, xih = pr.hmc_start(w.gL)
    U = lq.Gaugefields(w.lat).upload(w.loc(U0, 1))
    p, G = lq.Gaugefields(w.lat).upload(w.loc(P0, 1)), lq.Gaugefields(w.lat)
    D = lq.Dirac_operator(U, None, {"Dirac_operator": "Wilson", "κ": pr.HMC_KAPPA, "boundarycondition": bc, "eps_CG": 1e-22})
    fa = lq.FermiAction(D)
    xi = w.fermion(lq.WILSON, xih, 1)
    eta = xi.similar()
    lq.sample_pseudofermions_(eta, U, fa, xi)
    e = rel(eta.download(), w.r("c9/eta", 1))
    check(e < 1e-13, "eta = D^+ xi", e)
    r0 = w.reductions()
    K0, Sg0, Sf0 = lq.momentum_action(p), lq.evaluate_GaugeAction(U, pr.BETA), lq.dot(xi, xi).real
    w.rec(K0, Sg0, Sf0)
    for _ in range(pr.HMC_STEPS):
        lq.U_update_(U, p, 0.5 * pr.HMC_DTAU)
        lq.P_update_(U, p, pr.HMC_DTAU, pr.BETA)
        w.rec(lq.calc_UdSfdU_(G, fa, U, eta))
        lq.Traceless_antihermitian_add_(p, pr.HMC_DTAU, G)
        lq.U_update_(U, p, 0.5 * pr.HMC_DTAU)
    K1, Sg1, Sf1 = lq.momentum_action(p), lq.evaluate_GaugeAction(U, pr.BETA), lq.evaluate_FermiAction(fa, U, eta)
    w.rec(K1, Sg1, Sf1)
    dH = (K1 + Sg1 + Sf1) - (K0 + Sg0 + Sf0)
    eU, eP = rel(U.download(), w.r("c9/U", 1)), rel(p.download(), w.r("c9/P", 1))
    check(w.lat.get_param("staple_form_active") == 3 and w.reductions() > r0, "not the partitioned sweeps")
    check(eU < 1e-10 and eP < 1e-9 and abs(dH - float(w.r("c9/dH"))) < 1e-7, "trajectory", eU, eP, dH, float(w.r("c9/dH")))


CASES = {1: case1, 2: case2, 3: case3, 4: case4, 5: case5, 6: case6, 7: case7, 8: case8, 9: case9}
GAUGE_ONLY = (7, 8)


def same_on_all_ranks(w, what):
    """the scalars of the case, bit for bit, and the count of peer reductions, equal on every rank"""
    mine = torch.tensor([float(len(w.scalars))] + w.scalars + [float(w.reductions())], dtype=torch.float64)
    n = torch.tensor([mine.numel()], dtype=torch.int64)
    ns = [torch.empty_like(n) for _ in range(dist.get_world_size())]
    dist.all_gather(ns, n)
    check(all(int(t) == int(n) for t in ns), what, "ranks returned different numbers of scalars", [int(t) for t in ns])
    allv = [torch.empty_like(mine) for _ in range(dist.get_world_size())]
    dist.all_gather(allv, mine)
    reds = [int(t[-1]) for t in allv]
    check(len(set(reds)) == 1, what, "peer_reductions differ between the ranks", reds)
    bits = [t.view(torch.int64) for t in allv]
    bad = [k for k in range(mine.numel()) if any(int(b[k]) != int(bits[0][k]) for b in bits)]
    check(not bad, what, "scalars differ between the ranks at positions", bad, [[float(t[k]) for t in allv] for k in bad[:4]])
    w.scalars = []


def main():
    dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=120))
    rank, world = dist.get_rank(), dist.get_world_size()
    name = os.environ["PEER_SOLVERS_WORLD"]
    gL, pe, bcs, cases = pr.WORLDS[name]
    if os.environ.get("PEER_SOLVERS_CASES"):
        cases = tuple(int(v) for v in os.environ["PEER_SOLVERS_CASES"].split(","))
    what = "start"
    try:
        assert int(np.prod(pe)) == world
        ref = np.load(os.environ["PEER_SOLVERS_REF"])
        lat = lq.Lattice(gL, pe, rank, device=0)            # every rank on the ONE device
        lat.set_param("peer_timeout_ms", 20000)
        lat.comm_init_peer(gather_blobs)
        assert lat.comm_backend == "peer"
        mode0 = lat.get_param("halo_stream_mode")
        w = World(lat, gL, ref)
        for c in cases:
            for bc in ((None,) if c in GAUGE_ONLY else bcs):
                what = "case %d bc %s" % (c, bc)
                w.tag = None if bc is None else pr.bc_tag(bc)
                lat.set_param("halo_stream_mode", mode0)
                CASES[c](w, bc)
                lat.sync()
                same_on_all_ranks(w, what)
                print("PEER_SOLVERS_CASE_OK rank %d %s reductions %d" % (rank, what, w.reductions()), flush=True)
        what = "end"
        lat.sync()
        print(f"PEER_SOLVERS_OK rank {rank} world {name} pe {pe}", flush=True)
        dist.barrier()
        lat.close()
        dist.destroy_process_group()
    except BaseException as err:      # the first failure ends this rank: nothing is retried, nothing further is launched; the others meet peer_timeout_ms once
        print("PEER_SOLVERS_FAIL rank %d world %s at %s: %s: %s" % (rank, name, what, type(err).__name__, err), flush=True)
        traceback.print_exc()
        sys.stdout.flush(); sys.stderr.flush()
        os._exit(1)


if __name__ == "__main__":
    main()
