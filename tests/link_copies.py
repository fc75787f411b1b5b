"""Tables of tests/test_gpu_link_copies.py: the primed states of a gauge handle, the entry points that write links (WRITERS), the calls that read the cached
copies of them (CONSUMERS), and what each writer must leave of the handle's claim "every link is on SU(3) to rounding" (lqcd_gauge_s::unitary_version).

A Rig is one context with one link field, the operators built on it and fixed sources.  The consumers run on a rig and return, per consumer, the read-only keys
that say which copy was read and the arrays that came out; two rigs that hold the same link bits must return the same keys and the same bits.

Claim rules (column `claim` of WRITERS), written from the code's own rules (csrc/fields.hip, md.hip, links.hip, staple.hip, flow.hip, heatbath.hip, stout.hip):
    keep       the writer generates or projects every link: unit, hot start, reunitarize_, heatbath_, overrelaxation_
    if_group   a projected update (md_reunitarize = 1) or no write at all: kept when the field held the claim, never granted to a near / off field (their links
               fail the 1e-13 rule of the projection and are left alone)
    drop       uploads, md_reunitarize = 0, per-direction writes that are not the in-place projected update, the stout layer's output
A copy (substitute_U_) carries the claim of its source: keep from a group field, drop from a near / off one.
`recon` is the 12-real gate after the writer (recon_active of mul_): 1 on the group, "state" as primed (1 / 2 / 0), None: only held to the fresh handle."""
import ctypes as C

import numpy as np
import pytest

import staple_tile_map as tm
from conftest import rel_err

SMALL = (16, 8, 8, 4)         # scalar-addressing kernel, 12-real / 12 + delta links, temporal gauge under cg_tgauge = 2, the fp32 site-pair kernel, int16 links
ALT = (8, 8, 4, 8)            # the fp32 operator in its direction-split form (18-real and plain 12-real fp32 links): no pair kernel here
KAPPA, BC = 0.12, (1, 1, 1, -1)      # below the free critical hopping parameter: the solves also converge on unit links
CSW, CSW2 = 1.2, 1.7
MASS, DW_M, DW_MASS, L5 = 0.5, -1.0, 0.25, 2
BETA, BETA_RECT, FACTOR, DT = 5.7, -0.4, -0.37, 0.3
FLOW_EPS = 0.1
STATES = ("group", "near", "off")
RECON = {"group": 1, "near": 2, "off": 0}
NOISE = {"group": 0.0, "near": 1e-10, "off": 1e-3}
SEED_OLD, SEED_NEW, SEED_SRC, SEED_P = 5100, 5200, 5300, 5400
TOL = 1e-13
MOVED = 0.05                  # every writer that moves links moves some entry by more than this: a stale copy is an O(1) error in every consumer
SESSION_MESSAGE = "the gauge field changed under the open session"

_cache = {}


def kept_form(L):
    return 2 if tm.tile_ok(L) else 1


def _once(key, make):
    if key not in _cache:
        a = make()
        a.setflags(write=False)
        _cache[key] = a
    return _cache[key]


def hot(orc, L, seed):
    return _once(("hot", L, seed), lambda: orc.hot_gauge(L, seed))


def state_links(orc, L, seed, state):
    """the recipe of test_links_12_plus_delta_for_reference_format_configurations: hot links + NOISE[state] x complex Gaussian noise / 3"""
    def make():
        Uh = hot(orc, L, seed)
        if state == "group":
            return Uh.copy()
        rng = np.random.default_rng(seed + 1)
        return Uh + NOISE[state] * (rng.standard_normal(Uh.shape) + 1j * rng.standard_normal(Uh.shape)) / 3.0
    return _once(("links", L, seed, state), make)


def momenta(orc, L):
    return _once(("P", L), lambda: orc.gaussian_momenta(L, SEED_P + L[0]))


def source(orc, shape, seed):
    return _once(("src", shape, seed), lambda: orc.gaussian_spinor(shape, seed))


def make_field(lq, orc, lat, seed, state):
    """a link field in one of the three states: group = uploaded and projected (claim held), near / off = uploaded as they are (no claim)"""
    U = lq.Gaugefields(lat).upload(state_links(orc, lat.L, seed, state))
    if state == "group":
        lq.reunitarize_(U)
    return U


class Rig:
    def __init__(self, lq, orc, L, links, project=False, csw=CSW, share=None):
        self.lq, self.orc, self.L, self.csw = lq, orc, tuple(L), csw
        self.full = self.L == SMALL
        if share is None:
            self.lat = lq.Lattice(self.L)      # default tunables; a consumer or writer that sets one puts it back
        else:
            self.lat = share.lat
        self.U = lq.Gaugefields(self.lat).upload(links)
        if project:
            lq.reunitarize_(self.U)
        sh = self.lat.fermion_shape(lq.WILSON)
        self.b = lq.Fermionfields(self.lat, lq.WILSON).upload(source(orc, sh, 11))
        self.b2 = lq.Fermionfields(self.lat, lq.WILSON).upload(source(orc, sh, 12))
        if self.full:
            self.bs = lq.Fermionfields(self.lat, lq.STAGGERED).upload(source(orc, self.lat.fermion_shape(lq.STAGGERED), 13))
            self.b5 = lq.Fermionfields(self.lat, lq.DOMAINWALL, L5=L5).upload(source(orc, (L5,) + sh, 14))
        self.build_ops()

    def build_ops(self):
        lq, U = self.lq, self.U
        com = {"boundarycondition": BC, "eps_CG": 1e-19, "MaxCGstep": 3000}
        self.D = lq.Dirac_operator(U, None, dict(com, **{"Dirac_operator": "Wilson", "κ": KAPPA}))
        self.ops = [self.D]
        if self.full:
            self.Dc = lq.Dirac_operator(U, None, dict(com, **{"Dirac_operator": "WilsonClover", "κ": KAPPA, "Clover_coefficient": self.csw,
                                                              "method_CG": "bicgstab_evenodd"}))
            self.Ds = lq.Dirac_operator(U, None, dict(com, **{"Dirac_operator": "staggered", "mass": MASS}))
            self.Dw = lq.Dirac_operator(U, None, dict(com, **{"Dirac_operator": "Domainwall", "mass": DW_MASS, "M": DW_M, "L5": L5}))
            self.ops += [self.Dc, self.Ds, self.Dw]

    def fresh(self):
        """a handle with no history: a new context with the same tunables, the downloaded links uploaded, new operators"""
        return Rig(self.lq, self.orc, self.L, self.U.download(), csw=self.csw)

    def sibling(self, links, project=False):
        """a second field with its own operators on this rig's context"""
        return Rig(self.lq, self.orc, self.L, links, project=project, csw=self.csw, share=self)

    def momentum_field(self):
        return self.lq.Gaugefields(self.lat).upload(momenta(self.orc, self.L))

    def flush(self):
        self.U.download()      # every entry point that reads a field runs what the recorder holds (links.hip links_flush)


# ---------------------------------------------------------------------------------------------------------------------- consumers
# each returns (keys, arrays): the read-only keys that name the copy that was read, and the results
def c_force(r):
    """P_update_ into a zero momentum field; the form of the sweep is the handle's claim (0: 18 reals, 1 / 2: two rows)"""
    lq = r.lq
    P = lq.Gaugefields(r.lat)
    lq.P_update_(r.U, P, FACTOR, BETA)
    p = P.download()          # the recorder runs the sweep here
    form = r.lat.get_param("staple_form_active")
    P.close()
    return (form,), [p]


def c_wilson(r):
    lq = r.lq
    y, keys, out = r.b.similar(), [], []
    for D in (r.D, r.D.adjoint()):
        lq.mul_(y, D, r.b)
        keys.append(r.lat.get_param("recon_active"))
        out.append(y.download())
    return tuple(keys), out


def _cg(r, recon, small):
    lq, lat = r.lq, r.lat
    for k, v in (("cg_tgauge", 2), ("cg_small", small), ("cg_tgauge_recon", recon)):
        lat.set_param(k, v)
    x = r.b.similar()
    lq.lib.check(lq.lib.lib().lqcd_solve_cg_DdagD_fixed(r.D._h, x._h, r.b._h, 9))
    keys = (lat.get_param("tgauge_active"), lat.get_param("tgauge_recon_active"))
    for k, v in (("cg_tgauge", 1), ("cg_small", 1), ("cg_tgauge_recon", 8)):
        lat.set_param(k, v)
    return keys, [x.download()]


def c_cg12(r):
    return _cg(r, 12, 1)


def c_cg8(r):
    return _cg(r, 8, 0)       # the 8-real copy is read by the forms beyond cg_small only


def c_deviations(r):
    return (), [np.array([r.lq.unitarity_deviation(r.U), r.lq.tgauge8_deviation(r.U)])]


def c_f32(r):
    """the fp32 operator: fp32 links (mixed_links16 = 0), int16 links (2), and the direction-split form with the pair kernel switched off"""
    lq, lat = r.lq, r.lat
    y, keys, out = r.b.similar(), [], []
    for l16, pair in ((0, 1), (2, 1), (0, 0)):
        lat.set_param("mixed_links16", l16)
        lat.set_param("mixed_pair32", pair)
        for D in (r.D, r.D.adjoint()):
            lq.mul_f32_(y, D, r.b)
            keys.append((lat.get_param("f32_form_active"), lat.get_param("pair32_active")))
            out.append(y.download())
    lat.set_param("mixed_links16", 1)
    lat.set_param("mixed_pair32", 1)
    return tuple(keys), out


def c_mixed(r):
    lq = r.lq
    x = r.b.similar()
    lq.solve_mixed_DinvX_(x, lq.DdagD_operator(r.D), r.b)
    return (r.lat.get_param("mixed_handoffs"), r.lat.get_param("pair32_active")), [x.download()]


def c_clover(r):
    y = r.b.similar()
    r.lq.mul_(y, r.Dc, r.b)
    return (), [y.download()]


def c_clover_solves(r):
    """the even-odd BiCGStab in fp64 (clover term, its inverse), the mixed-precision CG on the clover operator (the fp32 copy of the clover term, mixed.hip mix_prepare), and
    the even-odd BiCGStab with the fp32 inner chain (bicg_mixed = 1, what mixed_action_solver = 1 switches on for the action solves: mix_prepare with eo_chain, the fp32 copy
    of A^-1, and on the plain Wilson operator the int16 links of the site-pair kernel)"""
    lq, lat = r.lq, r.lat
    x, z, xm, xw = (r.b.similar() for _ in range(4))
    lq.solve_DinvX_(x, r.Dc, r.b)
    lq.solve_mixed_DinvX_(z, lq.DdagD_operator(r.Dc), r.b)
    lat.set_param("bicg_mixed", 1)
    lq.solve_DinvX_(xm, r.Dc, r.b)
    keys = [(lat.get_param("pair32_active"), lat.get_param("mixed_handoffs"))]
    r.D.method_CG = "bicgstab_evenodd"
    lq.solve_DinvX_(xw, r.D, r.b)
    keys.append((lat.get_param("pair32_active"), lat.get_param("mixed_handoffs")))
    r.D.method_CG = "bicgstab"
    lat.set_param("bicg_mixed", 0)
    return tuple(keys), [x.download(), z.download(), xm.download(), xw.download()]


def c_others(r):
    """two columns at once, staggered, Domainwall"""
    lq = r.lq
    y1, y2, ys, y5 = r.b.similar(), r.b.similar(), r.bs.similar(), r.b5.similar()
    lq.mul_multi_([y1, y2], r.D, [r.b, r.b2])
    lq.mul_(ys, r.Ds, r.bs)
    lq.mul_(y5, r.Dw, r.b5)
    return (), [y1.download(), y2.download(), ys.download(), y5.download()]


CONSUMERS = {"wilson": c_wilson, "cg12": c_cg12, "cg8": c_cg8, "deviations": c_deviations, "f32": c_f32, "mixed": c_mixed, "clover": c_clover,
             "clover_solves": c_clover_solves, "others": c_others}
ON_ALT = ("wilson", "f32", "mixed")      # what the second lattice is for


def consumers_of(r):
    return {k: f for k, f in CONSUMERS.items() if r.full or k in ON_ALT}


def run_consumers(r):
    return {k: f(r) for k, f in consumers_of(r).items()}


def expected_keys(L, recon):
    """the keys a handle whose links pass the 12-real gate (recon = 1), the 12 + delta gate (2) or neither (0) must show.  cg8: no writer is exempt -- the 8-real chart
    takes every field here that passes the 12-real gate, unit links included (they decode exactly)"""
    if L == SMALL:
        tg = recon == 1
        pair = (3, 1) if recon == 1 else (1, 0)
        return {"wilson": (recon, recon), "cg12": (1, 12) if tg else (0, 0), "cg8": (1, 8) if tg else (0, 0),
                "f32": (pair, pair, pair, pair, (1, 0), (1, 0)), "mixed": (0, 1 if recon == 1 else 0)}
    return {"f32": ((1, 0),) * 6, "mixed": (0, 0)}


def check_keys(L, res, recon, what):
    want = expected_keys(L, recon)
    for k, v in want.items():
        assert res[k][0] == v, (what, k, res[k][0], v)


def compare(got, want, what):
    """keys first, then bits; returns the consumers that differ"""
    bad = []
    for k in want:
        if got[k][0] != want[k][0]:
            bad.append((k, "keys", got[k][0], want[k][0]))
            continue
        for i, (a, b) in enumerate(zip(got[k][1], want[k][1])):
            if not np.array_equal(a, b):
                bad.append((k, i, "max |diff| / max |ref| %.3e" % rel_err(a, b)))
    return bad


def check_oracle(r, Uh, res, force, what):
    """one application and the momentum update against the CPU oracle on the links the handle holds"""
    orc, L = r.orc, r.L
    bh = source(orc, r.lat.fermion_shape(r.lq.WILSON), 11)
    for dag, y in zip((False, True), res["wilson"][1]):
        err = rel_err(y, orc.wilson_D(Uh, bh, L, KAPPA, 1.0, BC, dagger=dag))
        assert err < TOL, (what, "mul_ against the oracle, dagger", dag, err)
    want = orc.momentum_add_ta(np.zeros(Uh.shape, dtype=np.complex128), FACTOR, orc.gauge_force(Uh, L, BETA), L)
    err = rel_err(force[1][0], want)
    assert err < TOL, (what, "P_update_ against the oracle", err, "form", force[0])


# ---------------------------------------------------------------------------------------------------------------------- writers
def _new(r):
    return hot(r.orc, r.L, SEED_NEW)


def w_upload(r, state):
    r.U.upload(_new(r))


def w_upload_disk(r, state):
    lq = r.lq
    tmp = lq.Gaugefields(r.lat).upload(_new(r))
    img = tmp.download(layout=lq.lib.LAYOUT_DISK)
    tmp.close()
    r.U.upload(img, layout=lq.lib.LAYOUT_DISK)
    assert np.array_equal(r.U.download(), _new(r))


def w_upload_wing(r, state):
    new, l = _new(r), r.lat.local_L
    W = np.zeros((4, l[3] + 2, l[2] + 2, l[1] + 2, l[0] + 2, 3, 3), dtype=np.complex128)
    W[:, 1:-1, 1:-1, 1:-1, 1:-1] = new
    r.U.upload(W, nwing=1)
    assert np.array_equal(r.U.download(), new)


def w_unit(r, state):
    r.lq.lib.check(r.lq.lib.lib().lqcd_gauge_unit(r.U._h))


def w_hot_start(r, state):
    r.lq.lib.check(r.lq.lib.lib().lqcd_gauge_hot_start(r.U._h, C.c_uint64(SEED_NEW)))


def _w_substitute(src_state):
    def w(r, state):
        V = make_field(r.lq, r.orc, r.lat, SEED_SRC, src_state)
        r.lq.substitute_U_(r.U, V)
        V.close()
    return w


def _w_U_update(reunit):
    def w(r, state):
        r.lat.set_param("md_reunitarize", reunit)
        P = r.momentum_field()
        r.lq.U_update_(r.U, P, DT)
        r.flush()
        r.lat.set_param("md_reunitarize", 1)
        P.close()
    return w


def w_merged_sweep(r, state):
    """P_update_ + U_update_ recorded and run as ONE sweep that writes the new links to the spare buffer and exchanges the two (staple.hip staple_force_expu)"""
    lq, orc, lat = r.lq, r.orc, r.lat
    assert lat.get_param("lazy_links") == 1 and lat.get_param("lazy_merge") == 2
    Uold, Ph = r.U.download(), momenta(orc, r.L)
    P = r.momentum_field()
    lq.P_update_(r.U, P, FACTOR, BETA)
    lq.U_update_(r.U, P, DT)
    assert lat.get_param("lazy_deferred") == 8, "the two updates did not wait for one another: the one-sweep form was not reached"
    p = P.download()
    form = lat.get_param("staple_form_active")
    assert form == (kept_form(r.L) if state == "group" else 0), (state, form)
    P1 = orc.momentum_add_ta(Ph.copy(), FACTOR, orc.gauge_force(Uold, r.L, BETA), r.L)
    U1 = orc.link_update(Uold.copy(), P1, DT, r.L)
    ep, eu = rel_err(p, P1), rel_err(r.U.download(), U1)
    assert ep < TOL and eu < TOL, ("merged sweep against the oracle", ep, eu)
    P.close()


def _w_triples(dirs, lazy):
    def w(r, state):
        lq, lat = r.lq, r.lat
        lat.lazy_links = bool(lazy)
        P, T = r.momentum_field(), lq.Gaugefields(lat)
        E, W = T[1], T[2]
        for mu in dirs:
            lq.exptU_(E, DT, P[mu])
            lq.mul_(W, E, r.U[mu])
            lq.substitute_U_(r.U[mu], W)
        r.flush()
        lat.lazy_links = True
        T.close()
        P.close()
    return w


def w_reunitarize(r, state):
    r.lq.reunitarize_(r.U)


def w_heatbath(r, state):
    lq = r.lq
    hb = lq.Heatbath(r.U, BETA, seed=SEED_NEW)
    lq.heatbath_(r.U, hb)
    hb.ITERATION_MAX = 1
    with pytest.raises(lq.LQCDError, match="ran out of itmax trials"):
        lq.heatbath_(r.U, hb)


def w_overrelaxation(r, state):
    r.lq.overrelaxation_(r.U)


def w_flow(r, state):
    r.lq.flow_(r.U, r.lq.Gradientflow(r.U, Nflow=1, eps=FLOW_EPS))


def w_flow_measure(r, state):
    tab = r.lq.gradient_flow_measure(r.U, eps=FLOW_EPS / 2, numflow=2, every=1)
    assert tab.shape == (2, 7) and np.isfinite(tab[:, :6]).all()


def w_improved(r, state):
    lq = r.lq
    P = r.momentum_field()
    lq.P_update_(r.U, P, FACTOR, BETA, BETA_RECT)
    lq.U_update_(r.U, P, DT)
    r.flush()
    P.close()


def w_smear(r, state):
    """calc_smearedU whose output handle is the field the operators were built on"""
    lq = r.lq
    V = make_field(lq, r.orc, r.lat, SEED_SRC, "group")
    nn = lq.CovNeuralnet(V)
    # push_ would give the layer a new output field of the net's own; the case needs the output to be the handle the operators were built on, which the binding offers no
    # call for: the layer and its output are entered by hand, in the two lists push_ fills
    nn.layers.append(lq.STOUT_Layer("plaquette", 0.1))
    nn._out.append(r.U)
    out, multi, _ = lq.calc_smearedU(V, nn)
    assert out is r.U
    err = rel_err(r.U.download(), r.orc.stout_smear(V.download(), r.L, 0.1))
    assert err < TOL, ("stout layer against the oracle", err)
    V.close()


def w_set_gauge(r, state):
    """every operator to a second field of the context, used there, and back: what it cached of the second field must not survive"""
    lq = r.lq
    V = make_field(lq, r.orc, r.lat, SEED_SRC, "group")
    for op in r.ops:
        op(V)
    keep = r.U
    r.U = V
    run_consumers(r)
    r.U = keep
    for op in r.ops:
        op(r.U)
    V.close()


def w_set_clover(r, state):
    r.lq.lib.check(r.lq.lib.lib().lqcd_op_set_clover(r.Dc._h, C.c_double(CSW2)))
    r.csw = CSW2


def w_recreate(r, state):
    """U.close(), a new field on the same context with other links, new operators: nothing of the context may still belong to the old handle"""
    for op in r.ops:
        op.close()
    r.U.close()
    r.U = r.lq.Gaugefields(r.lat).upload(_new(r))
    r.build_ops()


# name: (function, claim rule, recon after the writer, moves links, runs on the second lattice too: all but set_clover, which has no operator there)
WRITERS = {
    "upload": (w_upload, "drop", 1, True, True),
    "upload_disk": (w_upload_disk, "drop", 1, True, True),
    "upload_wing": (w_upload_wing, "drop", 1, True, True),
    "unit": (w_unit, "keep", 1, True, True),
    "hot_start": (w_hot_start, "keep", 1, True, True),
    "substitute_group": (_w_substitute("group"), "keep", 1, True, True),
    "substitute_near": (_w_substitute("near"), "drop", 2, True, True),
    "substitute_off": (_w_substitute("off"), "drop", 0, True, True),
    "U_update": (_w_U_update(1), "if_group", "state", True, True),
    "U_update_unprojected": (_w_U_update(0), "drop", "state", True, True),
    "merged_sweep": (w_merged_sweep, "if_group", "state", True, True),
    "triples_lazy": (_w_triples((1, 2, 3, 4), 1), "if_group", "state", True, True),
    "triples_eager": (_w_triples((1, 2, 3, 4), 0), "drop", "state", True, True),
    "triple_one_lazy": (_w_triples((3,), 1), "if_group", "state", True, True),
    "triple_one_eager": (_w_triples((3,), 0), "drop", "state", True, True),
    "reunitarize": (w_reunitarize, "keep", 1, False, True),
    "heatbath": (w_heatbath, "keep", 1, True, True),
    "overrelaxation": (w_overrelaxation, "keep", 1, True, True),
    "flow": (w_flow, "if_group", "state", True, True),
    "flow_measure": (w_flow_measure, "if_group", "state", True, True),
    "improved": (w_improved, "if_group", "state", True, True),
    "smear": (w_smear, "drop", None, True, True),
    "set_gauge": (w_set_gauge, "if_group", "state", False, True),
    "set_clover": (w_set_clover, "if_group", "state", False, False),
    "recreate": (w_recreate, "drop", 1, True, True),
}
SESSION_WRITERS = ("U_update", "merged_sweep", "flow", "upload")


def claim_kept(rule, state):
    return rule == "keep" or (rule == "if_group" and state == "group")
