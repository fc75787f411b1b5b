"""The reference side of the hard-system tests (tests/hard_systems.py; GPU side: tests/test_gpu_hard_solves.py).  No GPU: the oracle's textbook solvers
are rerun on every row of the table and held against tests/golden/hard_systems.json, against the accuracy contract with their own constant, and against
the hardness the rows are there for -- the guard against "fixing" a GPU failure by moving a row to an easier kappa.

Hardness.  Every row takes >= 300 iterations.  The rows solved through D^+D carry |x| / |b| >= 1e3.  The even-odd BiCGStab rows solve D x = b, whose
amplification at kappa = 0.128 is 5 to 6 (the oracle's figures are in the fixture): 1e3 is out of reach of the system itself, so these rows are pinned
by their iteration count and by the literal table below instead."""
import numpy as np
import pytest

import hard_systems as hs

# the rows as they were chosen: (shape, kappa or mass) -- an edit of tests/hard_systems.SYSTEMS has to be made here too, on purpose
PINNED = {
    "wilson_cg_16": ((16, 8, 8, 4), 0.1285), "wilson_cg_16_x0": ((16, 8, 8, 4), 0.1285), "wilson_cg_32": ((32, 4, 8, 4), 0.1285),
    "wilson_cg_32_k0128": ((32, 4, 8, 4), 0.128), "wilson_multishift_16": ((16, 8, 8, 4), 0.1285), "wilson_eo_D_gauss": ((16, 8, 8, 4), 0.128),
    "wilson_eo_Ddag_gauss": ((16, 8, 8, 4), 0.128), "wilson_eo_D_point": ((16, 8, 8, 4), 0.128), "staggered_cg_16": ((16, 8, 8, 4), 0.005),
    "staggered_cg_16_even": ((16, 8, 8, 4), 0.005),
}
_rows = {}


def rerun(orc, name):
    if name not in _rows:
        _rows[name] = hs.reference(orc, hs.system(name))
    return _rows[name]


def test_the_table_is_the_one_that_was_chosen():
    assert set(hs.SYSTEMS) == set(PINNED) == set(hs.fixture())
    for name, (L, km) in PINNED.items():
        s = hs.system(name)
        assert tuple(s["L"]) == L and s.get("kappa", s.get("mass")) == km and tuple(s["bc"]) == (1, 1, 1, 1) and s["eps"] == 1e-16, name
    assert tuple(hs.system("wilson_multishift_16")["sigmas"]) == (1e-4, 1e-3, 1e-2, 0.1)
    assert hs.GAUGE == {"momenta_seed": 5, "step": 0.2}


def test_the_links_are_smooth_and_exactly_su3(orc):
    s = hs.system("wilson_cg_16")
    Uh = np.array(hs.gauge(orc, s))
    assert abs(orc.plaquette(Uh, s["L"]) - 0.8987) < 5e-5
    assert orc.unitarity_dev(Uh, s["L"]) < 1e-14          # the gates of the 12-real and temporal-gauge paths hold


@pytest.mark.parametrize("name", sorted(hs.SYSTEMS))
def test_fixture_is_current_and_the_reference_meets_the_contract(orc, name):
    s, fix = hs.system(name), hs.fixture()[name]
    before = orc.lib().orc_get_threads()
    row = rerun(orc, name)
    assert orc.lib().orc_get_threads() == before
    print(name, row)
    assert row["iterations"] == fix["iterations"]
    for key in ("rr", "true_rr", "xnorm", "bnorm"):
        assert abs(row[key] - fix[key]) <= 1e-6 * abs(fix[key]), (name, key, row[key], fix[key])
    for key in ("shift_true_rr", "shift_xnorm"):
        for a, c in zip(row.get(key, ()), fix.get(key, ())):
            assert abs(a - c) <= 1e-6 * abs(c), (name, key, a, c)
    assert len(row.get("shift_true_rr", ())) == len(fix.get("shift_true_rr", ())) == len(s.get("sigmas", ()))
    # the contract of the GPU tests with the reference's own constant (from the fixture) in place of the margin of 8
    ok, c = hs.meets(s, row["true_rr"], row["rr"], row["xnorm"], factor=1.0, label="oracle")
    assert ok, (name, c)
    for j, sigma in enumerate(s.get("sigmas", ())):
        ok, c = hs.meets(s, row["shift_true_rr"][j], row["rr"], row["shift_xnorm"][j], sigma=sigma, shift=j, factor=1.0, label="oracle sigma %g" % sigma)
        assert ok, (name, sigma, c)
    # the row is hard
    assert row["iterations"] >= 300, (name, row["iterations"])
    if s["solver"] != "bicgstab_eo":
        assert row["xnorm"] / row["bnorm"] >= 1e3, (name, row["xnorm"] / row["bnorm"])


def test_t2_below_eps_is_not_the_contract(orc):
    """Why no test asserts `true residual < eps` here: a correct textbook CG misses it on one of the 32.4.8.4 rows (which one depends on the summation
    order of the inner products; at THREADS = 8 it is kappa = 0.1285) while it meets the contract on all of them."""
    rows = [rerun(orc, n) for n in ("wilson_cg_32", "wilson_cg_32_k0128")]
    assert all(r["rr"] < 1e-16 for r in rows)
    assert max(r["true_rr"] for r in rows) > 1e-16
