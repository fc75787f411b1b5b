"""The quenched heatbath and overrelaxation sweeps on the device (lqcd_gauge_heatbath, lqcd_gauge_overrelax, lqcd_gauge_heatbath_measure; the
reference's "Heatbath" update method, src/updates/heatbath.jl) against the numpy restatement (tests/heatbath_numpy.py, itself checked in
tests/test_cpu_heatbath_restatement.py), against the literature and the library's own quenched HMC, against the reference's Heatbath / SU(3) run, and on
partitioned lattices (world-size-1 RCCL with LQCD_FORCE_PARTITION; two processes on the one GPU through the peer backend) against the single-domain run."""
import ctypes as C
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import heatbath_numpy as hn
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import latticeqcd_jl_amd as lq
    if lq.lib.device_count() < 1:
        pytest.skip("no HIP device")
    return lq


def _hot(lq, L, seed):
    return lq.Initialize_Gaugefields(3, 0, *L, condition="hot", randomseed=seed)


def _fixture(lq):
    L = (4, 4, 4, 4)
    return L, lq.Gaugefields(lq.Lattice(L)).upload(lq.gauge_io.load_ildg(os.path.join(GOLDEN, "heatbath_su3_4x4x4x4.ildg"), L))


def _heatbath(lq, U, beta, nsweeps=1, nor=0, itmax=10**5, seed=111, first=0):
    lq.check(lq.lib.lib().lqcd_gauge_heatbath(U._h, C.c_double(beta), int(nsweeps), int(nor), int(itmax), C.c_uint64(seed), C.c_uint64(first)))


@pytest.mark.parametrize("case,beta", [("hot", 5.7), ("hot", 0.0), ("hot", 0.6), ("fixture", 5.7)])
def test_one_hb_and_one_or_sweep_match_the_restatement(gpu, case, beta):
    lq = gpu
    if case == "fixture":
        L, U = _fixture(lq)
    else:
        L = (4, 4, 4, 4)
        U = _hot(lq, L, 21)
    U0 = U.download()
    counts = {}
    ref, capped = hn.sweep(U0, L, False, beta, 10**5, 77, 5, counts)
    _heatbath(lq, U, beta, seed=77, first=5)
    assert capped == 0 and np.abs(U.download() - ref).max() <= 1e-12
    want = {0.0: ("haar",), 0.6: ("creutz",), 5.7: ("kp",)}[beta]
    for b in want:
        assert counts.get(b, 0) > 0, counts          # the branch ran
    ref, _ = hn.sweep(U.download(), L, True)
    lq.overrelaxation_(U)
    # the reflection divides by k = |quaternion part of W|: on the disordered links of beta <= 0.6 some k are small and the rounding of W is
    # amplified by 1/k (device and restatement differ there by a few 1e-12 at most, 1e-13 typically)
    assert np.abs(U.download() - ref).max() <= (1e-12 if beta > 1.0 else 1e-11)


def test_or_sweep_is_microcanonical(gpu):
    lq = gpu
    U = _hot(lq, (16, 16, 16, 16), 31)
    _heatbath(lq, U, 6.0, nsweeps=20)
    S0 = lq.evaluate_GaugeAction(U, 6.0)
    lq.overrelaxation_(U)
    S1 = lq.evaluate_GaugeAction(U, 6.0)
    assert abs(S1 - S0) <= 1e-12 * abs(S0), (S0, S1)


def test_links_stay_on_the_group_and_operators_see_them(gpu, orc):
    lq = gpu
    L, kappa, bc = (8, 8, 8, 8), 0.141139, (1, 1, 1, -1)
    U = _hot(lq, L, 41)
    D = lq.Dirac_operator(U, None, {"Dirac_operator": "Wilson", "κ": kappa, "boundarycondition": bc})
    b = lq.Fermionfields(U.lattice, lq.WILSON)
    lq.gauss_distribution_fermion_(b, 42)
    y = b.similar()
    lq.mul_(y, D, b)                               # cached link copies made from the hot start
    _heatbath(lq, U, 5.7, nsweeps=200, nor=3)
    assert lq.unitarity_deviation(U) <= 1e-13
    lq.mul_(y, D, b)
    ref = orc.wilson_D(U.download(), b.download(), L, kappa, 1.0, bc)
    assert np.abs(y.download() - ref).max() <= 1e-13 * max(1.0, np.abs(ref).max())


def test_runs_are_reproducible_and_split_runs_equal_one_run(gpu):
    lq = gpu
    L = (8, 8, 4, 4)
    A = _hot(lq, L, 51)
    _heatbath(lq, A, 5.7, nsweeps=10, nor=1, seed=3)
    B = _hot(lq, L, 51)
    for s in range(10):
        _heatbath(lq, B, 5.7, nor=1, seed=3, first=s)
    assert np.array_equal(A.download(), B.download())
    Cc = _hot(lq, L, 51)
    _heatbath(lq, Cc, 5.7, nsweeps=10, nor=1, seed=4)
    assert not np.array_equal(A.download(), Cc.download())
    # heatbath_measure = the step-by-step schedule with calculate_Plaquette after every block, bit for bit
    M = _hot(lq, L, 52)
    tab = lq.heatbath_measure(M, lq.Heatbath(M, 5.7, seed=9), 6, numOR=2)
    S = _hot(lq, L, 52)
    hb = lq.Heatbath(S, 5.7, seed=9)
    rows = []
    for _ in range(6):
        lq.heatbath_(S, hb)
        lq.overrelaxation_(S, hb)
        lq.overrelaxation_(S, hb)
        rows.append(lq.calculate_Plaquette(S))
    assert np.array_equal(np.array(rows), tab) and np.array_equal(S.download(), M.download())
    assert hb.sweep == 6
    # update_(Heatbathupdate(useOR, numOR = 3)) = heatbath_ + 3 x overrelaxation_
    P = _hot(lq, L, 53)
    Q = _hot(lq, L, 53)
    m = lq.Heatbathupdate(P, None, True, useOR=True, numOR=3, beta=5.7)
    assert lq.update_(m, P)
    hb = lq.Heatbath(Q, 5.7)
    lq.heatbath_(Q, hb)
    for _ in range(3):
        lq.overrelaxation_(Q, hb)
    assert np.array_equal(P.download(), Q.download())


def test_beta_zero_is_the_haar_measure(gpu):
    lq = gpu
    L = (8, 8, 8, 8)
    U = _hot(lq, L, 61)
    plaq = lq.heatbath_measure(U, lq.Heatbath(U, 0.0, seed=5), 20)
    Um = np.swapaxes(U.download(), -1, -2)
    tr = np.trace(Um, axis1=-2, axis2=-1).ravel()
    n = tr.size                                   # Haar: <tr U> = 0, <|tr U|^2> = 1, Var Re tr = Var Im tr = 1/2, Var |tr U|^2 = 1
    assert abs(tr.real.mean() / 3.0) < 4.0 * np.sqrt(0.5 / n) / 3.0
    assert abs(tr.imag.mean() / 3.0) < 4.0 * np.sqrt(0.5 / n) / 3.0
    assert abs(np.mean(np.abs(tr) ** 2) - 1.0) < 4.0 * np.sqrt(1.0 / n)
    nplaq = 6 * L[0] * L[1] * L[2] * L[3]          # Re tr U_p / 3 of a Haar plaquette: variance 1/18
    assert abs(plaq[-1]) < 4.0 * np.sqrt(1.0 / 18.0 / nplaq)


def _binned(x, nb=20):
    bins = x[: len(x) // nb * nb].reshape(nb, -1).mean(axis=1)
    return float(x.mean()), float(bins.std(ddof=1) / np.sqrt(nb))


@pytest.mark.parametrize("beta,lit", [(5.7, 0.5492), (6.0, 0.5937)])
def test_plaquette_lands_on_the_literature_value(gpu, beta, lit):
    lq = gpu
    L = (12, 12, 12, 12)
    U = lq.Initialize_Gaugefields(3, 0, *L, condition="cold")
    hb = lq.Heatbath(U, beta, seed=int(100 * beta))
    lq.heatbath_measure(U, hb, 200, numOR=3)
    mean, err = _binned(lq.heatbath_measure(U, hb, 2000, numOR=3))
    print("beta %.1f: <P> = %.5f +- %.5f (literature %.4f)" % (beta, mean, err, lit))
    assert abs(mean - lit) < 8e-4 + 3 * err, (mean, err, lit)


def test_heatbath_and_hmc_sample_the_same_ensemble(gpu):
    from test_gpu_quenched_literature import _run
    lq = gpu
    L, beta = (6, 6, 6, 6), 5.7
    U = lq.Initialize_Gaugefields(3, 0, *L, condition="cold")
    hb = lq.Heatbath(U, beta, seed=71)
    lq.heatbath_measure(U, hb, 200, numOR=3)
    mh, eh = _binned(lq.heatbath_measure(U, hb, 2000, numOR=3))
    mm, em, acc, _ = _run(lq, L, beta, 0.05, 20, 100, 1000, seed=72)
    print("6^4 beta 5.7: heatbath %.5f +- %.5f, HMC %.5f +- %.5f (acceptance %.2f)" % (mh, eh, mm, em, acc))
    assert abs(mh - mm) < 4.0 * np.hypot(eh, em), (mh, eh, mm, em)


def test_reference_heatbath_su3_run(gpu):
    lq = gpu
    ref = json.load(open(os.path.join(GOLDEN, "heatbath_reference.json")))
    start = json.load(open(os.path.join(GOLDEN, "golden.json")))
    p0 = start["plaquette"][ref["start_plaquette_golden_json_key"]]          # 0.5714781743564799
    L, U = _fixture(lq)
    assert abs(lq.calculate_Plaquette(U) - p0) <= 1e-13
    m = lq.Heatbathupdate(U, None, True, useOR=False, beta=5.7)
    for _ in range(10):
        lq.update_(m, U)
    p = lq.calculate_Plaquette(U)
    assert abs(p - ref["end_of_run_plaquette"]) <= ref["tolerance_relative"] * ref["end_of_run_plaquette"], p


def test_error_paths(gpu):
    lq = gpu
    U = _hot(lq, (4, 4, 4, 4), 81)
    with pytest.raises(lq.LQCDError) as e:
        _heatbath(lq, U, 5.7, itmax=1)
    assert e.value.code == 3
    assert lq.unitarity_deviation(U) <= 1e-13
    before = U.download()
    f = lq.lib.lib()
    plaq = (C.c_double * 4)()
    for args in ((-1.0, 1, 0, 10), (5.7, -1, 0, 10), (5.7, 1, -1, 10), (5.7, 1, 0, 0)):
        assert f.lqcd_gauge_heatbath(U._h, C.c_double(args[0]), args[1], args[2], args[3], C.c_uint64(1), C.c_uint64(0)) == 1
        assert f.lqcd_gauge_heatbath_measure(U._h, C.c_double(args[0]), args[1], args[2], args[3], C.c_uint64(1), C.c_uint64(0), plaq) == 1
    assert f.lqcd_gauge_heatbath_measure(U._h, C.c_double(5.7), 1, 0, 10, C.c_uint64(1), C.c_uint64(0), None) == 1
    assert f.lqcd_gauge_overrelax(U._h, -1) == 1
    assert np.array_equal(U.download(), before)


def test_partitioned_rccl_self_partition_matches_the_single_domain(gpu, orc, tmp_path):
    lq = gpu
    L = (8, 8, 8, 8)
    U = lq.Gaugefields(lq.Lattice(L)).upload(orc.hot_gauge(L, 111))
    tab = lq.heatbath_measure(U, lq.Heatbath(U, 5.7, seed=5), 2, numOR=3)
    ref = os.path.join(str(tmp_path), "single.npz")
    np.savez(ref, U=U.download(), tab=tab)
    code = textwrap.dedent(f"""
        import os, sys, numpy as np
        sys.path.insert(0, os.getcwd())
        import latticeqcd_jl_amd as lq
        from oracle import oracle as orc
        L = {L!r}
        r = np.load({ref!r})
        lat = lq.Lattice(L)
        lat.comm_init(lq.comm_unique_id())
        U = lq.Gaugefields(lat).upload(orc.hot_gauge(L, 111))
        tab = lq.heatbath_measure(U, lq.Heatbath(U, 5.7, seed=5), 2, numOR=3)
        err = float(np.abs(U.download() - r["U"]).max())
        assert err <= 1e-12 and np.abs(tab - r["tab"]).max() <= 1e-12, (err, tab, r["tab"])
        print("RCCL_SELF_HB_OK", err)
    """)
    env = dict(os.environ, LQCD_FORCE_PARTITION="15", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120, cwd=ROOT)
    assert r.returncode == 0 and "RCCL_SELF_HB_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_partitioned_peer_two_processes_match_the_single_domain(gpu):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29790", HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2",
               HB_TEST_LATTICE="8,8,8,8", HB_TEST_PE="1,1,1,2")
    env.pop("LQCD_FORCE_PARTITION", None)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", "29790", os.path.join(ROOT, "tests", "heatbath_peer_worker.py")],
                       capture_output=True, text=True, env=env, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-5000:]
    for k in range(2):
        assert f"HB_PEER_OK rank {k}" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
