"""The reference side of the solve-ending tests (tests/solve_endings.py: the table and the selection; GPU side: tests/test_gpu_solve_endings.py).
No GPU: with the oracle alone, every row of the table is shown to be what the device tests need it to be --

  * the committed scalars are current;
  * the oracle at the row's eps converges at iteration k exactly (the residuals of the BiCG family are not monotone: an eps between rr_{k-1} and
    rr_k can be met earlier, and such a row is moved to another k in the table, not exempted here);
  * eps is at least a factor 1.2 from both residuals it separates (device and oracle residuals differ by about 1e-10 relative);
  * the last update and the truncation error are visible: rel_err(x_k, x_{k-1}) >= 1e-5 and rel_err(x_eps, x_tight) >= 1e-5, five decades above
    the 1e-10 the device solution is held to; per shift for a multi-shift row.

There is no skip list."""
import numpy as np
import pytest

import solve_endings as se


def test_the_table_covers_what_it_was_drawn_up_for():
    assert set(se.ROWS) == set(se.fixture())
    cg = [se.row(n) for n in se.names("cg")]
    for op, L in (("wilson", se.S), ("staggered", se.S), ("wilson", se.P), ("wilson", se.R)):
        assert sorted(r["k"] for r in cg if r["op"] == op and r["L"] == L) == [3, 5, 6, 9]
    assert {r["op"] for r in cg} == {"wilson", "staggered", "clover", "domainwall"}
    eo = [se.row(n) for n in se.names("bicgstab_eo")]
    for L in (se.S, se.Q, se.B):
        for dagger in (False, True):
            assert {r["mode"] for r in eo if r["L"] == L and r["dagger"] == dagger and r["op"] == "wilson"} == {"full", "half"}, (L, dagger)
    assert all(r["k"] <= 4 for r in eo if r["L"] in (se.B, se.F)) and any(r["L"] == se.F for r in eo)
    for s in ("bicg", "bicgstab"):
        assert {(r["op"], r["dagger"]) for r in (se.row(n) for n in se.names(s))} == {(o, d) for o in ("wilson", "staggered") for d in (False, True)}
    assert {(r["op"], r["dagger"], r["mode"]) for r in (se.row(n) for n in se.names("bicgstab"))} == \
        {(o, d, m) for o in ("wilson", "staggered") for d in (False, True) for m in ("full", "half")}
    # 16.16.16.12 is the smallest lattice at which the streaming grid of the even-odd solver reaches its cap of 1024 workgroups of 256
    assert (12 * np.prod(se.B) // 2 + 255) // 256 == 1152 and not any((12 * np.prod(L) // 2 + 255) // 256 >= 1024 for L in (se.S, se.P, se.Q, se.R, se.T))
    assert (np.prod(se.F) // 2 + 63) // 64 == 1152 and (np.prod(se.Q) // 2) % 64 != 0
    assert all((L[0] // 2 * L[1]) % 64 != 0 for L in (se.S, se.P)) and (se.R[0] // 2 * se.R[1]) % 64 == 0 and np.prod(se.R) == np.prod(se.S)


@pytest.mark.parametrize("name", sorted(se.ROWS))
def test_row_is_current_and_ends_where_it_says(orc, name):
    r, fix = se.row(name), se.fixture()[name]
    before = orc.lib().orc_get_threads()
    sc = se.select(orc, r)
    assert orc.lib().orc_get_threads() == before
    print(name, sc)
    assert sc["k"] == fix["k"] == r["k"] and (sc["ss_k"] is None) == (fix["ss_k"] is None)
    assert sc["eps"] is not None, "iteration k has no half step"
    for key in ("eps", "rr_km1", "rr_k", "ss_k"):
        if fix[key] is not None:
            assert abs(sc[key] - fix[key]) <= 1e-12 * abs(fix[key]), (key, sc[key], fix[key])
    eps = fix["eps"]
    hi, lo = se.separated(r, fix)
    print("  eps %.6e: %.3f below %.6e, %.3f above %.6e" % (eps, hi / eps, hi, eps / lo, lo))
    assert hi / eps >= se.MARGIN and eps / lo >= se.MARGIN
    ref = se.reference(orc, name)
    assert ref[-2] == r["k"], (ref[-2], r["k"])
    assert abs(ref[-1] - lo) <= 1e-12 * lo                    # it stops on the residual the row says: rr_k, or ss_k in the half step
    xkm1 = se.capped(orc, r, r["k"] - 1)[0]
    tight = se.solve(orc, r, se.TIGHT)
    assert tight[-1] == 0
    last, trunc = se.rel_err(ref[0], xkm1), se.rel_err(ref[0], tight[0])
    print("  last update %.3e, truncation error %.3e" % (last, trunc))
    assert last >= se.VISIBLE and trunc >= se.VISIBLE
    if r["solver"] == "multishift":
        for j, sigma in enumerate(se.SHIFTS):
            trunc = se.rel_err(ref[1][j], tight[1][j])
            print("  sigma %g: truncation error %.3e" % (sigma, trunc))
            assert trunc >= se.VISIBLE, sigma
    elif r["mode"] == "full":
        assert np.array_equal(ref[0], se.capped(orc, r, r["k"])[0])      # ... and returns the iterate of the whole iteration


def test_the_columns_of_the_batched_solve_end_at_different_iterations(orc):
    """The batched even-odd BiCGStab is run on c_j b, c = (1, 1e-2, 1e2, 0), at the eps of the k = 3 row of 8.8.8.8: the absolute stopping rule ends
    the columns at different iterations, none of them within a factor 1.2 of eps (its count is the same at eps 1.2 and eps / 1.2)."""
    name = se.BATCHED_ROW
    r, eps = se.row(name), se.eps_of(name)
    its = []
    for c in se.COLUMN_SCALES[:3]:
        b = c * se.rhs(orc, r)
        counts = [se.solve(orc, r, e, b=b)[1] for e in (eps, eps * se.MARGIN, eps / se.MARGIN)]
        print("column scale %g: iterations %s" % (c, counts))
        assert counts[0] == counts[1] == counts[2] > 0
        x, it, rr, st = se.solve(orc, r, eps, b=b)
        assert st == 0 and se.rel_err(x, se.solve(orc, r, se.TIGHT * c * c, b=b)[0]) >= se.VISIBLE
        its.append(counts[0])
    assert len(set(its)) == 3, its
    x, it, rr, st = se.solve(orc, r, eps, b=0.0 * se.rhs(orc, r))
    assert st == 0 and it == 0 and not x.any()
