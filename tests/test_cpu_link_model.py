"""tests/link_model.py against the C oracle, and the bookkeeping of the sequence generator that tests/test_gpu_lazy_links.py runs on the device:
determinism, no read of a slot the contract leaves unspecified, no exponential of a slot that is not traceless anti-Hermitian with |t| |A| <= 1,
magnitudes, and the share of (field, slot) pairs the comparison has to leave out.  No GPU."""
import numpy as np
import pytest

import link_model as lm
from conftest import rel_err

NSEEDS = 64


@pytest.fixture(scope="module")
def sequences():
    return [lm.generate(seed) for seed in range(NSEEDS)]


@pytest.fixture(scope="module")
def models(sequences):
    return [lm.Model(lm.SEQ_L, F0).replay(ops) for F0, ops in sequences]


def test_replayed_triples_match_the_oracle_on_a_hot_configuration(orc):
    """U_update! and P_update! as the reference writes them -- three generics per direction, four directions -- through the model, against the
    oracle's link_update, gauge_force and momentum_add_ta: 1e-14 relative (the same arithmetic, only the order inside the 3x3 products differs)."""
    L = (8, 4, 6, 2)
    F0 = lm.initial_fields(L, 5)
    dt, c, beta = 0.035, 0.015, 5.7
    m = lm.Model(L, F0)
    for mu in range(4):
        m.replay(lm.u_triple(mu, dt))
    Uo = orc.link_update(F0["U"].copy(), F0["P"], dt, L)
    assert rel_err(m.F["U"], Uo) < 1e-14
    Go = orc.gauge_force(Uo, L, beta)
    for mu in range(4):
        m.replay(lm.p_triple(mu, -c / 3.0, beta))       # factor TA(U (beta/2) staples) = (-3 factor) TA(-(beta/6) U staples)
    Po = orc.momentum_add_ta(F0["P"].copy(), c, Go, L)
    assert rel_err(m.F["P"], Po) < 1e-14
    assert not m.spec[("A", 0)] and not m.spec[("A", 1)] and all(m.spec[(n, s)] for n in ("U", "P", "B") for s in range(4))
    # the whole-field calls are the same loops
    w = lm.Model(L, F0).replay([("U_update", "U", "P", dt), ("P_update", "U", "P", c, beta), ("gauge_force", "A", "U", beta), ("ta_add", "P", c, "A")])
    assert rel_err(w.F["U"], Uo) < 1e-14 and rel_err(w.F["A"], Go) < 1e-14
    assert rel_err(w.F["P"], orc.momentum_add_ta(Po.copy(), c, Go, L)) < 1e-14
    # the fused generics are their two halves
    a = lm.Model(L, F0).replay([("exp_mul", ("B", 0), dt, ("P", 1), ("U", 2)), ("add_ta_staple", ("P", 3), 0.1, "U", 3, beta)])
    b = lm.Model(L, F0).replay([("exp", ("A", 0), dt, ("P", 1)), ("mul", ("B", 0), ("A", 0), ("U", 2)),
                                ("staple", ("A", 2), "U", 3, beta), ("mul", ("A", 3), ("U", 3), ("A", 2)), ("add_ta", ("P", 3), 0.1, ("A", 3))])
    assert rel_err(a.F["B"][0], b.F["B"][0]) < 1e-14 and rel_err(a.F["P"][3], b.F["P"][3]) < 1e-14


def test_contract_bookkeeping():
    """A completed triple leaves its temporaries unspecified, a read of one raises, a whole-slot write makes it specified again; a triple that is
    interrupted, or whose copy goes elsewhere than the mul's second factor, leaves everything specified."""
    F0 = lm.initial_fields(lm.SEQ_L, 9)
    m = lm.Model(lm.SEQ_L, F0).replay(lm.u_triple(2, 0.1))
    assert not m.spec[("A", 0)] and not m.spec[("A", 1)] and m.spec[("U", 2)]
    with pytest.raises(lm.UnspecifiedRead):
        m.apply(("copy", ("B", 0), ("A", 1)))
    m.apply(("copy", ("A", 1), ("B", 3)))
    assert m.spec[("A", 1)] and not m.spec[("A", 0)]
    m = lm.Model(lm.SEQ_L, F0).replay(lm.u_triple(2, 0.1, dst=("U", 1)))
    assert all(m.spec.values())
    ops = lm.p_triple(1, 0.02)
    m = lm.Model(lm.SEQ_L, F0).replay(ops[:2] + [("U_update", "U", "P", 0.1)] + ops[2:])
    assert all(m.spec.values())
    m = lm.Model(lm.SEQ_L, F0).replay(ops)
    assert not m.spec[("A", 0)] and not m.spec[("A", 1)] and m.spec[("P", 1)]


def test_generator_is_deterministic(sequences):
    for seed in (0, 17, 63):
        F0, ops = lm.generate(seed)
        assert ops == sequences[seed][1]
        assert all(np.array_equal(F0[k], sequences[seed][0][k]) for k in lm.FIELDS)
    assert len({repr(ops) for _, ops in sequences}) == NSEEDS


def test_sequences_have_6_to_12_generics_and_respect_the_refusals(sequences):
    for _, ops in sequences:
        assert lm.MIN_CALLS <= lm.n_calls(ops) <= lm.MAX_CALLS
        for op in ops:
            assert not (op[0] == "add_ta" and op[1] == op[3]) and not (op[0] == "staple" and op[1][0] == op[2])


def test_no_sequence_reads_an_unspecified_slot(models):
    assert len(models) == NSEEDS          # Model.apply raises UnspecifiedRead: the replay in the fixture is the check


def test_no_sequence_exponentiates_an_untyped_slot(models):
    n = 0
    for m in models:
        for defect, tnorm in m.exps:
            assert defect <= 1e-12 and tnorm <= 1.0
            n += 1
    assert n > NSEEDS


def test_magnitudes_stay_below_the_cap(models):
    assert max(m.peak for m in models) < lm.MAG_CAP
    assert max(float(np.abs(v).max()) for m in models for v in m.F.values()) < lm.MAG_CAP


def test_at_most_a_quarter_of_the_slots_is_left_out(models):
    left_out = sum(1 for m in models for ok in m.spec.values() if not ok)
    assert left_out <= 0.25 * 16 * NSEEDS, left_out
    assert sum(1 for m in models if not all(m.spec.values())) >= NSEEDS // 4      # and the contract does bite


def test_the_mutations_all_occur(sequences):
    """Every way of aliasing that section 3 of the GPU file relies on is present in the 64 sequences."""
    seen = set()
    for _, ops in sequences:
        for i, op in enumerate(ops):
            if op[0] in ("exp", "staple") and op[1][0] == "P":
                seen.add("first temporary in P")
            if op[0] == "mul" and op[1][0] in ("U", "P") and i and ops[i - 1][0] in ("exp", "staple"):
                seen.add("second temporary in " + op[1][0])
            if op[0] == "copy" and i and ops[i - 1][0] == "mul" and ops[i - 1][1] == op[2] and ops[i - 1][3] != op[1]:
                seen.add("dst is not the mul's B")
            if op[0] == "exp" and i + 1 < len(ops) and ops[i + 1][0] == "mul" and ops[i + 1][3][0] == "U" and ops[i + 1][3][1] != op[3][1]:
                seen.add("P slot differs from U slot")
            if op[0] in ("U_update", "P_update") and i and ops[i - 1][0] in ("exp", "staple", "mul") and i + 1 < len(ops) and ops[i + 1][0] in ("mul", "copy", "add_ta"):
                seen.add("interleaved whole-field update")
            if op[0] in ("exp", "staple") and op[1][0] in ("U", "P") and any(o[0] in ("U_update", "P_update") for o in ops[:i]):
                seen.add("temporary is a field of an earlier whole-field update")
    assert seen >= {"first temporary in P", "second temporary in U", "second temporary in P", "dst is not the mul's B", "P slot differs from U slot",
                    "interleaved whole-field update", "temporary is a field of an earlier whole-field update"}, seen
