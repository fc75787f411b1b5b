"""TEST INFRASTRUCTURE: the CPU references of tests/test_gpu_peer_solvers.py, computed ONCE on the global lattice by the parent (the oracle, and
tests/rect_numpy.py for the gauge side) and written to one .npz.  The ranks of tests/peer_solvers_worker.py rebuild the seeded inputs with the functions
below, load the file and cut their part with lq.pegrid.local_view: no rank runs an oracle solve, and nothing here comes from the library under test (the
partial fractions of the rational action are the scipy fit of tests/rational_scipy.py; the worker hands the same numbers to the library).

Keys of the file: "<bc tag>/<case>/<name>", e.g. "ppp-/c1/x1" = the even-odd BiCGStab solution of D^+ x = b under bc (1,1,1,-1); the cases without
fermions (7, 8) sit under "g/"."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from oracle import oracle as orc  # noqa: E402

KAPPA, MASS, CSW = 0.125, 0.5, 1.5612                     # the operators of tests/peer_world_worker.py
BC_T = (1, 1, 1, -1)
SHIFTS = (0.004, 0.06, 0.9)                               # three of the shifts of test_gpu_parity.py::test_multishift_cg_matches_oracle
RHO = 0.11
DW_L5, DW_M, DW_MASS = 4, -1.0, 0.1                       # test_gpu_domainwall.py::test_cg_solution_matches_the_oracle
NF = 2
BETA, FACTOR = 5.7, -0.37                                 # gauge side: the plaquette coupling, the factor of test_gpu_rect_action.py's momentum update
RECT_REFUSED = (9.5, -0.475)                              # (beta_plaq, beta_rect) of test_gpu_rect_action.py::test_partitioned_lattice_is_refused
HMC_KAPPA, HMC_DTAU, HMC_STEPS = 0.141139, 0.05, 2        # test_gpu_hmc_partitioned.py::_single

# every world of tests/test_gpu_peer_solvers.py: name -> (global L, PE grid, boundary conditions, cases)
ALL = (1, 2, 3, 4, 5, 6, 7, 8, 9)
WORLDS = {
    "t2": ((4, 4, 4, 8), (1, 1, 1, 2), (BC_T,), ALL),
    # the issue's second boundary condition (1,-1,1,1), and (1,1,-1,1): the sign on the partitioned z face
    "z2": ((4, 4, 4, 8), (1, 1, 2, 1), (BC_T, (1, -1, 1, 1), (1, 1, -1, 1)), ALL),
    "zt4": ((4, 4, 4, 8), (1, 1, 2, 2), (BC_T,), ALL),
    "t4": ((4, 4, 4, 8), (1, 1, 1, 4), (BC_T,), (1, 2, 4, 5, 7, 8)),
    "x2": ((16, 4, 4, 4), (2, 1, 1, 1), (BC_T,), (1, 4, 5)),
}


def bc_tag(bc):
    return "".join("p" if s > 0 else "-" for s in bc)


# ---------------------------------------------------------------- seeded inputs (parent and ranks build the same arrays)
def gauge(L):
    return orc.hot_gauge(L, 111)


def wilson_rhs(L):
    return orc.gaussian_spinor(orc.wilson_shape(L), 112)


def staggered_rhs(L):
    return orc.gaussian_spinor(orc.staggered_shape(L), 112)


def dw_rhs(L):
    return orc.gaussian_spinor((DW_L5,) + orc.wilson_shape(L), 114)


def stout_force_in(L):
    rng = np.random.default_rng(8)
    return rng.standard_normal(orc.gauge_shape(L)) + 1j * rng.standard_normal(orc.gauge_shape(L))


def momenta(L):
    return orc.gaussian_momenta(L, 302)


def hmc_start(L):
    """(U, P, xi) of the trajectory: a mildly disordered start keeps the solves short (test_gpu_hmc_partitioned.py)"""
    U = orc.link_update(orc.unit_gauge(L), 0.3 * orc.gaussian_momenta(L, 899), 1.0, L)
    return U, orc.gaussian_momenta(L, 901), orc.gaussian_spinor(orc.wilson_shape(L), 902) * np.sqrt(0.5)


def rational_fits():
    """(a0, res, poles) of x^(-Nf/8) for the action and the MD force and of x^(Nf/16 - 1) for the heat bath on the staggered interval [m^2, m^2 + 16]:
    the tolerances of FermiAction's defaults (rhmc_tol_action 1e-12, rhmc_tol_MD 1e-8), fitted by scipy"""
    import rational_scipy as rs
    lo, hi = MASS ** 2, MASS ** 2 + 16.0
    out = {}
    for name, alpha, tol in (("action", NF / 8.0, 1e-12), ("md", NF / 8.0, 1e-8), ("sampling", 1.0 - NF / 16.0, 1e-12)):
        a0, res, poles, _ = rs.inverse_power_partial_fractions(alpha, lo, hi, tol)
        out[name] = (float(a0), np.asarray(res, dtype=np.float64), np.asarray(poles, dtype=np.float64))
    return out


# ---------------------------------------------------------------- the references
def _fermion_cases(L, bc, cases, U, put, status):
    def solved(what, st):
        status[what] = int(st)

    b = wilson_rhs(L)
    bs = staggered_rhs(L)
    if 1 in cases or 4 in cases:
        for dag in (0, 1):
            x, it, _, st = orc.wilson_bicgstab_eo(U, b, L, KAPPA, 1.0, bc, bool(dag), eps=1e-19)
            solved("c1 dag %d" % dag, st)
            put("c1/x%d" % dag, x); put("c1/it%d" % dag, it)
    if 2 in cases:
        for name, kind, km, rhs in (("w", orc.WILSON, KAPPA, b), ("s", orc.STAGGERED, MASS, bs)):
            for dag in (0, 1):
                x, it, _, st = orc.bicgstab(kind, U, rhs, L, km, 1.0, bc, bool(dag), eps=1e-19)
                solved("c2 %s dag %d" % (name, dag), st)
                put("c2/%s_x%d" % (name, dag), x); put("c2/%s_it%d" % (name, dag), it)
    A = orc.clover_build(U, L, KAPPA, CSW) if (3 in cases or 4 in cases) else None
    if 3 in cases or 4 in cases:
        for dag in (0, 1):
            x, it, _, st = orc.wilson_clover_bicgstab_eo(U, A, b, L, KAPPA, 1.0, bc, bool(dag), eps=1e-19)
            solved("c3 dag %d" % dag, st)
            put("c3/x%d" % dag, x); put("c3/it%d" % dag, it)
    if 3 in cases:
        S, G, X, Y = orc.clover_fermion_force(U, A, b, L, KAPPA, CSW, 1.0, bc, eps=1e-22)      # (asserts its own solve)
        put("c3/S", S); put("c3/G", G); put("c3/X", X); put("c3/Y", Y)
    if 4 in cases:
        x, it, _, st = orc.cg_DdagD(orc.WILSON, U, b, L, KAPPA, 1.0, bc, eps=1e-19)
        solved("c4 wilson", st)
        put("c4/w_x", x)
        x, it, _, st = orc.cg_clover(U, A, b, L, KAPPA, 1.0, bc, eps=1e-19)
        solved("c4 clover", st)
        put("c4/c_x", x)
    if 5 in cases:
        for name, kind, km, rhs in (("w", orc.WILSON, KAPPA, b), ("s", orc.STAGGERED, MASS, bs)):
            x0, xs, it, _, st = orc.multishift_cg(kind, U, rhs, L, km, SHIFTS, 1.0, bc, eps=1e-20)
            solved("c5 %s" % name, st)
            put("c5/%s_x0" % name, x0); put("c5/%s_xs" % name, np.stack(xs)); put("c5/%s_it" % name, it)
        fits = rational_fits()
        for name, (a0, res, poles) in fits.items():
            put("c5/fit_%s" % name, np.concatenate([[a0], res, poles]))
        a0, res, poles = fits["action"]
        y, _ = orc.rational_apply(orc.STAGGERED, U, bs, L, MASS, a0, res, poles, 1.0, bc)      # (asserts its own multi-shift solve)
        put("c5/r_y", y); put("c5/r_S", np.vdot(bs, y).real)
        put("c5/r_G", orc.rational_force(orc.STAGGERED, U, bs, L, MASS, fits["md"][1], fits["md"][2], 1.0, bc))
        a0, res, poles = fits["sampling"]           # eta = D^+D r(D^+D) xi  (csrc/rational.hip lqcd_action_sample_pseudofermions)
        t, _ = orc.rational_apply(orc.STAGGERED, U, bs, L, MASS, a0, res, poles, 1.0, bc)
        put("c5/r_eta", orc.staggered_D(U, orc.staggered_D(U, t, L, MASS, bc), L, MASS, bc, True))
    if 6 in cases:
        b5 = dw_rhs(L)
        for dag in (0, 1):
            put("c6/D%d" % dag, orc.domainwall_D(U, b5, L, DW_M, DW_MASS, bc, dagger=bool(dag)))
        x, it, rr = orc.domainwall_cg(U, b5, L, DW_M, DW_MASS, bc, eps=1e-19)
        solved("c6 cg", 0 if rr < 1e-19 else 1)
        put("c6/x", x); put("c6/it", it)
        S, _, _ = orc.domainwall_action(U, b5, L, DW_M, DW_MASS, bc, eps=1e-24)
        put("c6/S", S); put("c6/G", orc.domainwall_force(U, b5, L, DW_M, DW_MASS, bc, eps=1e-24))
    if 9 in cases:
        import oracle_md as omd
        U0, P0, xi = hmc_start(L)
        eta = orc.wilson_D(U0, xi, L, HMC_KAPPA, 1.0, bc, True)
        fermion = (orc.WILSON, HMC_KAPPA, bc, eta, 1e-22)
        H0 = orc.momentum_action(P0, L) + orc.gauge_action(U0, L, BETA) + np.vdot(xi, xi).real
        U1, P1 = omd.trajectory(orc, U0, P0, L, BETA, HMC_DTAU, HMC_STEPS, "QPQ", fermion=fermion)      # (asserts every solve)
        H1 = omd.hamiltonian(orc, U1, P1, L, BETA, fermion)
        put("c9/eta", eta); put("c9/U", U1); put("c9/P", P1); put("c9/dH", H1 - H0)


def _gauge_cases(L, cases, U, put):
    if 7 in cases:
        put("c7/U", orc.stout_smear(U, L, RHO))
        put("c7/G", orc.stout_backprop(stout_force_in(L), U, L, RHO))
    if 8 in cases:
        import rect_numpy as rn
        G = rn.force(U, L, BETA, 0.0)
        put("c8/S", rn.action(U, L, BETA, 0.0)); put("c8/G", G)
        put("c8/P", rn.to_host(rn.to_xyzt(momenta(L)) + FACTOR * rn.ta(rn.to_xyzt(G))))


def build(L, path, bcs=(BC_T,), cases=ALL):
    """Every reference of `cases` on the global lattice L under each boundary condition -> one .npz at `path`.  Returns {solve: status}: 0 = the oracle
    solve converged (the caller asserts it)."""
    L = tuple(int(v) for v in L)
    data, status = {}, {}
    U = gauge(L)
    _gauge_cases(L, cases, U, lambda k, v: data.__setitem__("g/" + k, np.asarray(v)))
    for bc in bcs:
        tag = bc_tag(bc)
        st = {}
        _fermion_cases(L, tuple(bc), cases, U, lambda k, v: data.__setitem__(tag + "/" + k, np.asarray(v)), st)
        status.update({tag + " " + k: v for k, v in st.items()})
    np.savez(path, **data)
    return status
