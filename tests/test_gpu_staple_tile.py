"""The tile form of the staple sweep (csrc/staple.hip gauge_force_kernel_tile: the kernel of every production MD step; tunable staple_tile, read-only
staple_form_active) against the CPU oracle at every row width XH = Lx / 2 the form accepts -- 1, 2, 4, 8, 16, 32, 64 -- and, for the lattices it must refuse, the
generic two-row kernel.  The lane arithmetic behind it is checked without a GPU in tests/test_cpu_staple_tile_map.py; the shape table and the host gate's verdicts
come from tests/staple_tile_map.py.

Instances: gauge_force_ -> <0, false>; P_update_ -> <1, false>; P_update_ + U_update_ recorded and run as one sweep (lazy_links = 1, lazy_merge = 2) -> <1, true, false>;
flow_ -> <1, true, true>.  Every case asserts the form that ran (staple_form_active: 0 generic kernel on 18 reals, 1 generic kernel on two rows, 2 tile), so a
lattice that drops out of the gate fails instead of passing through another kernel; a fresh context reads -1, so a form 0 is one a sweep wrote.  No gate refuses Lx = 2 or Lx = 128: both run like the others.

Reference: orc.gauge_force, orc.momentum_add_ta, orc.link_update on the links the device holds (hot start of orc.hot_gauge, uploaded, reunitarize_d, downloaded),
momenta of orc.gaussian_momenta; computed once per lattice and never changed.  Bounds: those of tests/test_gpu_md.py and tests/test_gpu_reunit.py for the same
operations -- max |dev - ref| / max |ref| < 1e-13 on force, momenta and updated links, unitarity deviation < 1e-14 after an update; the flow cases keep the
bounds of tests/test_gpu_gradient_flow.py (1e-12 on links and observables after 10 steps).  The three forms of the force agree with one another to 1e-13 (their
products associate differently); md_remap changes the order of the workgroups only: equal bits.

Measured on an MI355X (max |dev - oracle| / max |oracle|; merged sweep with md_reunitarize = 1 / 0; unitarity deviation after the projected merged sweep; flow:
max |U - restatement| after 10 steps).  The tile and the generic two-row kernel do the same arithmetic in the same order and gave the same figure everywhere.

    lattice      XH  force tile  force 18   fused P   merged P  merged U (1 / 0)     unitarity  flow
    2x64x2x4      1  5.8e-16     3.6e-16    2.3e-16   2.3e-16   5.7e-16 / 3.5e-16    1.1e-15
    4x32x2x4      2  4.7e-16     3.5e-16    2.0e-16   2.0e-16   5.8e-16 / 4.6e-16    1.1e-15
    8x16x4x6      4  5.6e-16     4.8e-16    3.4e-16   3.4e-16   6.2e-16 / 5.0e-16    1.1e-15
    16x8x6x4      8  5.3e-16     3.8e-16    2.1e-16   2.1e-16   6.8e-16 / 4.6e-16    1.1e-15    8.7e-15
    16x16x4x2     8  5.3e-16     3.4e-16    2.2e-16   2.2e-16   6.0e-16 / 4.0e-16    1.1e-15    9.1e-15
    32x4x4x6     16  5.1e-16     3.4e-16    2.5e-16   2.5e-16   6.5e-16 / 5.0e-16    1.1e-15    1.2e-14
    32x8x2x4     16  5.7e-16     4.7e-16    2.6e-16   2.6e-16   6.0e-16 / 4.6e-16    8.9e-16    9.1e-15
    64x2x4x6     32  5.8e-16     3.7e-16    2.6e-16   2.6e-16   6.7e-16 / 4.4e-16    1.1e-15
    128x2x2x4    64  6.0e-16     4.1e-16    2.1e-16   2.1e-16   5.8e-16 / 4.7e-16    1.1e-15
    refused: 12x4x4x4 force 5.6e-16, P 2.6e-16, U 5.8e-16; 8x4x6x4 5.6e-16, 2.3e-16, 6.3e-16; 4x4x6x2 5.3e-16, 3.0e-16, 5.7e-16 (form 1 throughout)

Without projection (md_reunitarize = 0) the merged sweep left a unitarity deviation of at most 1.3e-15; the 1e-14 bound is asserted in both modes.  With the two LDS lane indices of staple_plane_tile swapped (an in-bounds mutation, not committed) the force came out wrong by
0.88 .. 1.10 of its maximum at every XH > 1, the momenta by 0.34 .. 0.44, the links of the merged sweep by 0.12 .. 0.14, the flow by 0.59 .. 0.67; XH = 1, where
n + x and n - x are one site, passed.
"""
import numpy as np
import pytest

import flow_numpy as fn
import staple_tile_map as tm
from conftest import rel_err

pytestmark = pytest.mark.gpu

BETA, FACTOR, DT = 5.7, -0.37, 0.11          # the step of tests/test_gpu_md.py
TOL, TOL_UNIT = 1e-13, 1e-14
TILE = [L for _, Ls in sorted(tm.ACCEPTED.items()) for L in Ls]
FLOW = tm.ACCEPTED[8] + tm.ACCEPTED[16]
FLOW_EPS, FLOW_STEPS = 0.02, 10               # tests/test_gpu_gradient_flow.py
_refs = {}


def _id(L):
    return "x".join(map(str, L))


@pytest.fixture(scope="module")
def gpu(lq):
    assert lq.lib.device_count() > 0, "no HIP device visible: the product has no CPU fallback"
    return lq


class Ref:
    """the host side of a lattice: start links as the device holds them, momenta, and the oracle's force, updated momenta and updated links"""

    def __init__(self, lq, orc, L):
        self.L = L
        self.U0 = orc.hot_gauge(L, 1000 + L[0])
        U = lq.Gaugefields(lq.Lattice(L)).upload(self.U0)
        lq.reunitarize_(U)
        self.Uh = U.download()
        assert np.abs(self.Uh - self.U0).max() < 1e-14           # an SU(3) field moves by rounding only
        self.Ph = orc.gaussian_momenta(L, 2000 + L[0])
        self.Gh = orc.gauge_force(self.Uh, L, BETA)
        self.P1 = orc.momentum_add_ta(self.Ph.copy(), FACTOR, self.Gh, L)
        self.U1 = orc.link_update(self.Uh.copy(), self.P1, DT, L)
        for a in (self.U0, self.Uh, self.Ph, self.Gh, self.P1, self.U1):
            a.setflags(write=False)


def _ref(lq, orc, L):
    if L not in _refs:
        _refs[L] = Ref(lq, orc, L)
    return _refs[L]


def _context(lq, ref, project=True, **params):
    """a fresh context with the given settings and the start links on it: projected (tracked as on the group, the same bits as ref.Uh) or as uploaded"""
    lat = lq.Lattice(ref.L)
    for k, v in params.items():
        lat.set_param(k, v)
    U = lq.Gaugefields(lat).upload(ref.U0 if project else ref.Uh)
    if project:
        lq.reunitarize_(U)
    assert lat.get_param("staple_form_active") == -1, "no sweep has run here: every form read below was written by the sweep before it"
    return lat, U


def _force(lq, lat, U):
    G = lq.Gaugefields(lat)
    lq.gauge_force_(G, U, BETA)
    return G.download(), lat.get_param("staple_form_active")


def _fused(lq, lat, U, ref):
    """P_update_ on its own: the recorder holds it until the download, which runs it as one momentum sweep"""
    P = lq.Gaugefields(lat).upload(ref.Ph)
    lq.P_update_(U, P, FACTOR, BETA)
    return P.download(), lat.get_param("staple_form_active")


def _pair(lq, lat, U, ref):
    """P_update_ then U_update_ on the same (U, P), as a Sexton-Weingarten block asks for them; returns (P, U, form, records that waited)"""
    P = lq.Gaugefields(lat).upload(ref.Ph)
    lq.P_update_(U, P, FACTOR, BETA)
    lq.U_update_(U, P, DT)
    waited = lat.get_param("lazy_deferred")
    p = P.download()
    return p, U.download(), lat.get_param("staple_form_active"), waited


def _entries(lq, ref, **params):
    """items 1 to 3 on one context: force, fused momentum update, merged momentum + link sweep"""
    lat, U = _context(lq, ref, **params)
    out = {}
    out["G"], f0 = _force(lq, lat, U)
    out["P"], f1 = _fused(lq, lat, U, ref)
    out["U_kept"] = U.download()
    out["Pm"], out["Um"], f2, waited = _pair(lq, lat, U, ref)
    return out, (f0, f1, f2), waited


def _against_oracle(out, ref, what):
    errs = {"G": rel_err(out["G"], ref.Gh), "P": rel_err(out["P"], ref.P1), "Pm": rel_err(out["Pm"], ref.P1), "Um": rel_err(out["Um"], ref.U1)}
    print(_id(ref.L), what, " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) < TOL, (what, errs)
    assert np.array_equal(out["U_kept"], ref.Uh), (what, "gauge_force_ / P_update_ changed the links")


# ---------------------------------------------------------------- 1. force: tile, generic two-row, generic 18-real
@pytest.mark.parametrize("L", TILE, ids=_id)
def test_force_matches_the_oracle_in_all_three_forms(gpu, orc, L):
    lq = gpu
    assert tm.tile_ok(L)
    ref = _ref(lq, orc, L)
    G = {}
    for form, params in ((2, {}), (1, {"staple_tile": 0}), (0, {"staple_recon": 0})):
        lat, U = _context(lq, ref, **params)
        assert np.array_equal(U.download(), ref.Uh)
        G[form], active = _force(lq, lat, U)
        err = rel_err(G[form], ref.Gh)
        print(_id(L), "force, form", form, "ran", active, "rel err", err)
        assert active == form, ("staple_form_active", active, form)
        assert err < TOL, (form, err)
        again, _ = _force(lq, lat, U)
        assert np.array_equal(again, G[form]), (form, "two calls differ")
        assert np.array_equal(U.download(), ref.Uh), (form, "gauge_force_ changed the links")
    for a, b in ((2, 1), (2, 0), (1, 0)):
        assert rel_err(G[a], G[b]) < TOL, (a, b, rel_err(G[a], G[b]))
    # links of unknown provenance: the 18-real kernel whatever staple_tile says
    lat, U = _context(lq, ref, project=False, staple_tile=1)
    G18, active = _force(lq, lat, U)
    assert active == 0 and rel_err(G18, ref.Gh) < TOL, (active, rel_err(G18, ref.Gh))


# ---------------------------------------------------------------- 2. fused momentum update
@pytest.mark.parametrize("L", TILE, ids=_id)
def test_fused_momentum_update_matches_the_oracle(gpu, orc, L):
    lq = gpu
    ref = _ref(lq, orc, L)
    lat, U = _context(lq, ref)
    p, active = _fused(lq, lat, U, ref)
    err, moved = rel_err(p, ref.P1), float(np.abs(p - ref.Ph).max())
    print(_id(L), "fused momentum update: form", active, "rel err", err, "max |P' - P|", moved)
    assert active == 2
    assert err < TOL
    assert moved > 0.01
    again, active = _fused(lq, lat, U, ref)
    assert active == 2 and np.array_equal(again, p)
    assert np.array_equal(U.download(), ref.Uh), "P_update_ changed the links"


# ---------------------------------------------------------------- 3. merged momentum + link sweep
@pytest.mark.parametrize("reunit", [1, 0])
@pytest.mark.parametrize("L", TILE, ids=_id)
def test_merged_sweep_matches_the_oracle_and_the_two_sweeps(gpu, orc, L, reunit):
    lq = gpu
    ref = _ref(lq, orc, L)
    lat, U = _context(lq, ref, lazy_links=1, lazy_merge=2, md_reunitarize=reunit)
    p, u, active, waited = _pair(lq, lat, U, ref)
    assert waited == 8, ("the two updates did not wait for one another", waited)
    dev = orc.unitarity_dev(u, L)
    ep, eu = rel_err(p, ref.P1), rel_err(u, ref.U1)
    print(_id(L), "merged sweep, md_reunitarize", reunit, ": form", active, "P", ep, "U", eu, "unitarity", dev)
    assert active == 2
    assert ep < TOL and eu < TOL
    assert float(np.abs(u - ref.Uh).max()) > 0.01 and float(np.abs(p - ref.Ph).max()) > 0.01
    assert dev < TOL_UNIT
    # the same pair as two sweeps
    lat2, U2 = _context(lq, ref, lazy_links=1, lazy_merge=0, md_reunitarize=reunit)
    p2, u2, active2, waited2 = _pair(lq, lat2, U2, ref)
    assert waited2 == 0 and active2 == 2
    assert rel_err(p2, ref.P1) < TOL and rel_err(u2, ref.U1) < TOL
    assert rel_err(p, p2) < TOL and rel_err(u, u2) < TOL
    # and once more from the start: equal bits
    lat3, U3 = _context(lq, ref, lazy_links=1, lazy_merge=2, md_reunitarize=reunit)
    p3, u3, _, _ = _pair(lq, lat3, U3, ref)
    assert np.array_equal(p3, p) and np.array_equal(u3, u)


# ---------------------------------------------------------------- 4. md_remap: another order of the workgroups, the same bits
@pytest.mark.parametrize("L", TILE, ids=_id)
def test_md_remap_changes_no_bit(gpu, orc, L):
    """md_remap = 1 reorders the workgroups on every lattice here (their block counts are multiples of 8): through block_map's plain interleave over the XCDs on all
    but (16,16,4,2), whose t-slice of 8 chunks takes the per-XCD tile map the benchmark's lattice takes (tests/test_cpu_staple_tile_map.py asserts which is which)"""
    lq = gpu
    ref = _ref(lq, orc, L)
    runs = {}
    for remap in (1, 0):
        out, forms, waited = _entries(lq, ref, md_remap=remap)
        assert forms == (2, 2, 2) and waited == 8, (remap, forms, waited)
        _against_oracle(out, ref, f"md_remap {remap}")
        runs[remap] = out
    for k in runs[1]:
        assert np.array_equal(runs[1][k], runs[0][k]), k


# ---------------------------------------------------------------- the lattices the tile form must refuse: the generic two-row kernel
@pytest.mark.parametrize("L", tm.REFUSED, ids=_id)
def test_refused_lattices_run_the_generic_two_row_kernel(gpu, orc, L):
    lq = gpu
    assert not tm.tile_ok(L)
    ref = _ref(lq, orc, L)
    out, forms, waited = _entries(lq, ref, staple_tile=1)
    assert forms == (1, 1, 1) and waited == 8, (forms, waited)
    _against_oracle(out, ref, "refused")
    assert float(np.abs(out["P"] - ref.Ph).max()) > 0.01
    assert orc.unitarity_dev(out["Um"], L) < TOL_UNIT


# ---------------------------------------------------------------- 6. the flow instance at XH = 8 and XH = 16
@pytest.mark.parametrize("L", FLOW, ids=_id)
def test_flow_matches_the_restatement_on_the_tile_form(gpu, orc, L):
    lq = gpu
    ref = _ref(lq, orc, L)
    lat, U = _context(lq, ref)
    lq.flow_(U, lq.Gradientflow(U, Nflow=FLOW_STEPS, eps=FLOW_EPS))
    active = lat.get_param("staple_form_active")
    want = fn.flow(ref.Uh, L, FLOW_EPS, FLOW_STEPS)
    err = float(np.abs(U.download() - want).max())
    print(_id(L), "flow: form", active, "max |U - restatement|", err)
    assert active == 2
    assert err < 1e-12
    o, r = lq.gauge_flow_observables(U), fn.observables(want, L)
    for k in fn.OBS:
        assert abs(o[k] - r[k]) <= 1e-12 * max(1.0, abs(r[k])), (k, o[k], r[k])
    assert float(np.abs(want - ref.Uh).max()) > 0.01
