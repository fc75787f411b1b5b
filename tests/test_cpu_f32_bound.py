"""CPU self-test of the site-wise fp32 error metric (tests/f32_bound.py) that the GPU tests of the fp32 operators assert.

1. The NumPy restatement in complex128 equals the oracle to 1e-13 (Wilson r = 1 and 0.7, Wilson-clover, staggered; D and D^+).
2. The same code in complex64 -- a plain fp32 evaluation, no FMA, NumPy's summation order -- stays a factor 6 below K_ASSERT on every lattice, boundary
   condition and coupling of tests/test_gpu_f32_operators.py: K_ASSERT is 6 x the largest K measured here, never a device's number.
3. Planted errors exceed K_ASSERT; the two smallest (kappa (1 + 1e-5), one hop of one site off by 1e-3) by a factor 5 and more.  If the metric could not
   separate those from the restatement with a factor 5 on each side it would be the wrong metric.

Setting F32_BOUND_PLANT to one of the names of PLANTS puts that error into the restatement of test 2, which then fails: the check of the check."""
import os

import numpy as np
import pytest

import f32_bound as fb

KAPPA, CSW = 0.141139, 1.5612
LATS = [(4, 4, 4, 4), (8, 4, 6, 2), (6, 6, 4, 2), (16, 8, 8, 4), (8, 4, 6, 8)]
BCS = [(1, 1, 1, -1), (-1, -1, 1, 1), (1, -1, -1, -1), (-1, 1, -1, 1)]      # every direction antiperiodic and periodic at least once
SITE = (1, 2, 3, 1)      # [t,z,y,x] of the planted single-site errors: inside every lattice above

PLANTS = {
    "kappa": {"kappa_factor": 1.0 + 1e-5},
    "hop": {"hop_site": SITE, "hop_rel": 1e-3},
    "face": {"flip_face": 2},
    "dagger": {"swap_dagger": True},
    "clover": {"clover_conj_site": SITE},
    "phase": {"flip_phase": 2},
}
_ENV_PLANT = PLANTS[os.environ["F32_BOUND_PLANT"]] if os.environ.get("F32_BOUND_PLANT") else None


@pytest.fixture(scope="module")
def fields(orc):
    out = {}
    for L in LATS:
        U = orc.hot_gauge(L, 41)
        out[L] = (U, orc.gaussian_spinor(orc.wilson_shape(L), 42), orc.gaussian_spinor(orc.staggered_shape(L), 43), orc.clover_build(U, L, KAPPA, CSW))
    return out


def _cases(orc, fields, L, bc, dg, planted=None):
    """(kind, label, K of the complex64 restatement, max |complex128 restatement - oracle|) for every operator on one lattice"""
    U, psi, chi, A = fields[L]
    for r in (1.0, 0.7):
        ref = orc.wilson_D(U, psi, L, KAPPA, r, bc, dg)
        d = np.abs(fb.wilson_D_np(U, psi, KAPPA, r, bc, dg) - ref).max()
        yield "wilson", "r=%g" % r, fb.wilson_K(fb.wilson_D_np(U, psi, KAPPA, r, bc, dg, np.complex64, planted=planted), ref, psi, KAPPA, r), d
    ref = orc.wilson_clover_D(U, A, psi, L, KAPPA, 1.0, bc, dg)
    d = np.abs(fb.wilson_D_np(U, psi, KAPPA, 1.0, bc, dg, A=A) - ref).max()
    yield "clover", "csw=%g" % CSW, fb.wilson_K(fb.wilson_D_np(U, psi, KAPPA, 1.0, bc, dg, np.complex64, A=A, planted=planted), ref, psi, KAPPA, 1.0, A), d
    for m in (0.5, 0.01):
        ref = orc.staggered_D(U, chi, L, m, bc, dg)
        d = np.abs(fb.staggered_D_np(U, chi, m, bc, dg) - ref).max()
        yield "staggered", "m=%g" % m, fb.staggered_K(fb.staggered_D_np(U, chi, m, bc, dg, np.complex64, planted=planted), ref, chi, m), d


@pytest.mark.parametrize("L", LATS)
def test_restatement_equals_the_oracle_in_fp64_and_stays_inside_the_bound_in_fp32(orc, fields, L):
    worst = {}
    for bc in BCS:
        for dg in (False, True):
            for kind, label, K, d in _cases(orc, fields, L, bc, dg, _ENV_PLANT):
                assert d < 1e-13, (kind, label, L, bc, dg, d)
                worst[kind] = max(worst.get(kind, 0.0), K)
                assert 6.0 * K <= fb.K_ASSERT[kind], (kind, label, L, bc, dg, K)
    print("restatement K on", L, {k: round(v, 4) for k, v in worst.items()})


def test_input_rounding_alone_is_a_part_of_the_bound(orc, fields):
    """the reference sees the unrounded inputs: rounding links and spinor to fp32 and evaluating in fp64 already gives K = 0.24-0.34"""
    L, bc = (6, 6, 4, 2), (1, -1, 1, -1)
    U, psi, chi, A = fields[L]
    ref = orc.wilson_D(U, psi, L, KAPPA, 1.0, bc, False)
    K = fb.wilson_K(fb.wilson_D_np(U.astype(np.complex64), psi.astype(np.complex64), KAPPA, 1.0, bc, False), ref, psi, KAPPA)
    assert 0.1 < K < 0.5, K


@pytest.mark.parametrize("L", [(6, 6, 4, 2), (16, 8, 8, 4)])
@pytest.mark.parametrize("name", sorted(PLANTS))
def test_planted_errors_exceed_the_bound(orc, fields, L, name):
    bc = (1, -1, 1, -1)
    U, psi, chi, A = fields[L]
    pl = PLANTS[name]
    got = []
    if name != "phase":
        ref = orc.wilson_D(U, psi, L, KAPPA, 1.0, bc, False)
        if name != "clover":
            got.append(("wilson", fb.wilson_K(fb.wilson_D_np(U, psi, KAPPA, 1.0, bc, False, np.complex64, planted=pl), ref, psi, KAPPA)))
        refc = orc.wilson_clover_D(U, A, psi, L, KAPPA, 1.0, bc, False)
        got.append(("clover", fb.wilson_K(fb.wilson_D_np(U, psi, KAPPA, 1.0, bc, False, np.complex64, A=A, planted=pl), refc, psi, KAPPA, 1.0, A)))
    if name in ("hop", "face", "dagger", "phase"):
        refs = orc.staggered_D(U, chi, L, 0.5, bc, False)
        got.append(("staggered", fb.staggered_K(fb.staggered_D_np(U, chi, 0.5, bc, False, np.complex64, planted=pl), refs, chi, 0.5)))
    print("planted", name, L, got)
    for kind, K in got:
        assert K > 5.0 * fb.K_ASSERT[kind], (name, kind, K)      # the smallest ones (kappa: K ~ 40, hop: K ~ 1000) with a factor 5 to spare; the rest by orders of magnitude
