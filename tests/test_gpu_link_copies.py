"""Every cached copy of the links against fresh links after every writer (tables: tests/link_copies.py).

A gauge handle carries derived copies of its links -- 12 reals, 12 + delta, the temporal-gauge copies on 12 and on 8 reals -- a context carries the fp32 and int16 copies
of the mixed-precision solvers, an operator its clover term and the inverse of it; each is rebuilt when the handle's version counter says that the links moved, and every
entry point that writes links has to move that counter.  The handle also carries the claim "every link is on SU(3) to rounding", which the staple sweep and the flow trust
(two rows per link are read).  Production alternates writes and solves on ONE handle; so does every case here:

    prime     a context with a field in one of three states (group: hot links uploaded and projected, claim held; near: + 1e-10 noise, the 12 + delta links; off: + 1e-3
              noise, 18 reals everywhere) runs every consumer once, and the read-only key of every copy is asserted: each copy exists and is current for the OLD links
    write     one entry point that writes links (or rebinds an operator), with links, seeds and steps that differ from the primed ones by O(0.1) and more
    consume   P_update_ first -- its form (staple_form_active) is the claim as the WRITER left it; the consumers after it measure the links and may grant it -- then every
              consumer again

Reference of the consumers: the same calls on a handle with no history -- a new context with the same tunables, upload(U.download()), new operators -- whose paths the
rest of the suite holds to the oracle.  Keys first, then np.array_equal: equal link bits build equal copies, kernels and reductions are deterministic.  The control case (no
writer) shows that for every consumer: on an MI355X all nine consumers were bit-equal between two contexts in all three states, so none is compared at a looser bound.
One application (mul_, D and D^+) and the momentum update are also held to the CPU oracle on the downloaded links at 1e-13, the bound of their own test files; the
momentum update only to the oracle, because a fresh handle holds no claim and takes the 18-real sweep.

The open CG session (consumer "the documented error") runs in the group state: the error of lqcd_cg_session_iterate belongs to a session in temporal gauge, which near / off
links do not enter.  The fp32 copies of the clover term and of its inverse are reached through the mixed-precision CG on the clover operator and through the even-odd
BiCGStab with the fp32 inner chain (bicg_mixed = 1, the switch mixed_action_solver = 1 throws for the action solves), which on the plain Wilson operator also reads the int16 links.

Found by the cases substitute_near / substitute_off on a group handle: lqcd_gauge_tgauge8_deviation went on reporting the deviation of the previous links' 8-real copy
for links that fail the 12-real gate and have no such copy, where a handle without history reports the documented 1e300 -- gauge_ensure_tgauge left before it
reset tgauge8_dev.  The reset moved up in fields.hip; the solver never read the stale figure (it asks tgauge_ok first).

Mutations tried in scratch builds, and the cases that failed (w-* = every state of writer w on both lattices): version++ out of lqcd_gauge_reunitarize: reunitarize-* (keys in the
near / off states, 1e-16 differences in the group state: the copies of the unprojected links); out of flow_stage's single-GPU branch: flow-*, flow_measure-*, the session
case of flow; out of hb_run: heatbath-*, overrelaxation-*, the self-partitioned case; out of link_op: triples_eager-*, triple_one_eager-*; the swap of staple_force_expu without
its version++: merged_sweep-*, its session case; lqcd_gauge_copy granting the claim unconditionally: substitute_near-*, substitute_off-* (two-row form 2 / 1 where the
18-real form 0 is expected); same_links of mix_prepare reduced to the handle: 67 of the first 126 cases (every writer that moves links in the group
state, the in-place updates in all three, and two of recreate: the recycled handle address matched); clover_inv_version kept in lqcd_op_set_clover: set_clover-*.

On an MI355X the module's 159 cases take 19 s: 7 s the child process of the self-partitioned case, 0.4 s the slowest other case, 0.1 s the typical one.
"""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import link_copies as lc
from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(lq):
    assert lq.lib.device_count() > 0, "no HIP device visible: the product has no CPU fallback"
    return lq


def _prime(lq, orc, L, state, what):
    """a rig in `state` on which every consumer has run on the old links, each with the key that says its copy was built and read"""
    r = lc.Rig(lq, orc, L, lc.state_links(orc, L, lc.SEED_OLD, state), project=state == "group")
    force = lc.c_force(r)
    assert force[0] == (lc.kept_form(L) if state == "group" else 0,), (what, "priming: claim", force[0])
    res = lc.run_consumers(r)
    lc.check_keys(L, res, lc.RECON[state], what + ": priming")
    return r, res


def _after(r, state, claim, recon, what):
    """the consumers on the written handle against a handle without history, the oracle and the expected claim"""
    force = lc.c_force(r)
    want_form = lc.kept_form(r.L) if claim else 0
    print(what, "staple_form_active", force[0][0], "expected", want_form)
    assert force[0] == (want_form,), (what, "claim after the writer: staple_form_active", force[0][0], "expected", want_form)
    Uh = r.U.download()
    got = lc.run_consumers(r)
    f = r.fresh()
    assert np.array_equal(f.U.download(), Uh)
    want = lc.run_consumers(f)
    bad = lc.compare(got, want, what)
    assert not bad, (what, "differs from a handle without history", bad)
    if recon is not None:
        lc.check_keys(r.L, got, recon, what)
    lc.check_oracle(r, Uh, got, force, what)
    return Uh


# ---------------------------------------------------------------- control: no writer
@pytest.mark.parametrize("L", [lc.SMALL, lc.ALT], ids=["16x8x8x4", "8x8x4x8"])
@pytest.mark.parametrize("state", lc.STATES)
def test_control_two_contexts_with_equal_links_give_equal_bits(gpu, orc, state, L):
    """No writer: every consumer on two contexts that hold the same links -- the premise of every other case.  Prints, per consumer, whether bit equality held."""
    r, res = _prime(gpu, orc, L, state, "control")
    f = r.fresh()
    want = lc.run_consumers(f)
    bad = lc.compare(res, want, "control")
    for k in want:
        print("control", state, L, k, "keys", res[k][0], "bit-equal between two contexts:", not [b for b in bad if b[0] == k])
    assert not bad, bad
    again = lc.run_consumers(r)
    assert not lc.compare(again, res, "control, second run"), "a second run on the same context differs"
    lc.check_oracle(r, r.U.download(), res, lc.c_force(r), "control")


# ---------------------------------------------------------------- every writer in every state
def _cases():
    for name, (_, _, _, _, alt) in lc.WRITERS.items():
        for state in lc.STATES:
            yield pytest.param(name, state, lc.SMALL, id=f"{name}-{state}-16x8x8x4")
            if alt:
                yield pytest.param(name, state, lc.ALT, id=f"{name}-{state}-8x8x4x8")


@pytest.mark.parametrize("name,state,L", list(_cases()))
def test_consumers_after_a_writer_equal_a_handle_without_history(gpu, orc, name, state, L):
    fn, rule, recon, moves, _ = lc.WRITERS[name]
    what = f"{name} / {state} / {L}"
    r, _ = _prime(gpu, orc, L, state, what)
    before = r.U.download()
    fn(r, state)
    Uh = _after(r, state, lc.claim_kept(rule, state), lc.RECON[state] if recon == "state" else recon, what)
    moved = float(np.abs(Uh - before).max())
    print(what, "max |U' - U|", moved)
    if moves:
        assert moved > lc.MOVED, (what, "the writer did not move the links", moved)


# ---------------------------------------------------------------- two fields that alternate on one context
def test_two_fields_alternate_on_the_fp32_copies_of_one_context(gpu, orc):
    """The fp32 and int16 link copies belong to the context: A and B take turns on them, A is written in between."""
    lq = gpu
    a = lc.Rig(lq, orc, lc.SMALL, lc.state_links(orc, lc.SMALL, lc.SEED_OLD, "group"), project=True)
    b = a.sibling(lc.state_links(orc, lc.SMALL, lc.SEED_SRC, "group"), project=True)
    use = ("mixed", "f32")

    def run(r):
        return {k: lc.CONSUMERS[k](r) for k in use}

    ra0, rb0 = run(a), run(b)
    P = a.momentum_field()
    lq.U_update_(a.U, P, lc.DT)
    rb1, ra1 = run(b), run(a)
    rb2 = run(b)
    for res in (ra0, rb0, ra1, rb1, rb2):
        assert res["mixed"][0] == (0, 1) and res["f32"][0][0] == (3, 1), (res["mixed"][0], res["f32"][0])
    fa, fb = a.fresh(), b.fresh()
    assert float(np.abs(fa.U.download() - lc.state_links(orc, lc.SMALL, lc.SEED_OLD, "group")).max()) > lc.MOVED
    wa, wb = run(fa), run(fb)
    assert not lc.compare(ra1, wa, "A after its update"), lc.compare(ra1, wa, "")
    for res, what in ((rb0, "B before"), (rb1, "B after A was written"), (rb2, "B after A was solved on")):
        bad = lc.compare(res, wb, what)
        assert not bad, (what, bad)
    assert lc.compare(ra0, wa, "A before"), "the update of A changed no result: the case proves nothing"
    P.close()


# ---------------------------------------------------------------- an open CG session across a write
@pytest.mark.parametrize("name", lc.SESSION_WRITERS)
def test_an_open_cg_session_refuses_to_iterate_after_a_write(gpu, orc, name):
    lq = gpu
    r, _ = _prime(lq, orc, lc.SMALL, "group", "session")
    r.lat.set_param("cg_tgauge", 2)
    x = r.b.similar()
    ses = lq.CGSession(r.D, x, r.b)
    assert r.lat.get_param("tgauge_active") == 1
    ses.iterate(2)
    lc.WRITERS[name][0](r, "group")
    with pytest.raises(lq.LQCDError, match=lc.SESSION_MESSAGE):
        ses.iterate(1)
    ses.close()
    assert np.isfinite(x.download()).all()
    r.lat.set_param("cg_tgauge", 1)
    got, want = lc.c_cg12(r), lc.c_cg12(r.fresh())
    assert got[0] == want[0] == (1, 12) and np.array_equal(got[1][0], want[1][0])


# ---------------------------------------------------------------- a self-partitioned context
def test_self_partitioned_context_after_update_flow_and_heatbath(gpu, orc):
    """LQCD_FORCE_PARTITION = 8 and a one-rank communicator: the partitioned forms of the link update, the flow and the heatbath, each followed by mul_ and P_update_
    against the oracle on the downloaded links at 1e-13; the staple sweep reports form 3 there."""
    code = textwrap.dedent("""
        import os, sys, numpy as np
        sys.path.insert(0, os.getcwd())
        sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
        import latticeqcd_jl_amd as lq
        from oracle import oracle as orc
        import link_copies as lc
        L = lc.SMALL
        lat = lq.Lattice(L)
        lat.comm_init(lq.comm_unique_id())
        U = lq.Gaugefields(lat).upload(orc.hot_gauge(L, lc.SEED_OLD))
        lq.reunitarize_(U)
        D = lq.Dirac_operator(U, None, {"Dirac_operator": "Wilson", "κ": lc.KAPPA, "boundarycondition": lc.BC, "eps_CG": 1e-19})
        bh = orc.gaussian_spinor(lat.fermion_shape(lq.WILSON), 11)
        b = lq.Fermionfields(lat, lq.WILSON).upload(bh)
        y = b.similar()
        Pm = lq.Gaugefields(lat).upload(orc.gaussian_momenta(L, lc.SEED_P))

        def consume(what, before):
            Uh = U.download()
            lq.mul_(y, D, b)
            ref = orc.wilson_D(Uh, bh, L, lc.KAPPA, 1.0, lc.BC)
            e1 = np.abs(y.download() - ref).max() / np.abs(ref).max()
            P = lq.Gaugefields(lat)
            lq.P_update_(U, P, lc.FACTOR, lc.BETA)
            p = P.download()
            form = lat.get_param("staple_form_active")
            want = orc.momentum_add_ta(np.zeros(Uh.shape, dtype=np.complex128), lc.FACTOR, orc.gauge_force(Uh, L, lc.BETA), L)
            e2 = np.abs(p - want).max() / np.abs(want).max()
            moved = 1.0 if before is None else np.abs(Uh - before).max()
            print(what, "mul_", e1, "P_update_", e2, "form", form, "moved", moved)
            assert e1 < lc.TOL and e2 < lc.TOL and form == 3 and moved > lc.MOVED, (what, e1, e2, form, moved)
            P.close()
            return Uh

        Uh = consume("primed", None)
        lq.U_update_(U, Pm, lc.DT)
        Uh = consume("U_update_", Uh)
        lq.flow_(U, lq.Gradientflow(U, Nflow=1, eps=lc.FLOW_EPS))
        Uh = consume("flow_", Uh)
        lq.heatbath_(U, lq.Heatbath(U, lc.BETA, seed=lc.SEED_NEW))
        Uh = consume("heatbath_", Uh)
        print("LINK_COPIES_SELF_OK")
    """)
    env = dict(os.environ, LQCD_FORCE_PARTITION="8", HSA_ENABLE_IPC_MODE_LEGACY="0", LQCD_HALO_STREAM_MODE="3")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "LINK_COPIES_SELF_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
