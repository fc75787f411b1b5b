"""The gradient flow and its observables on the device (lqcd_gradient_flow, lqcd_gauge_flow_observables, lqcd_gradient_flow_measure; the driver's
flow block, the reference's src/system/lqcd.jl:95-100,149-164) against the numpy restatement (tests/flow_numpy.py, itself checked in
tests/test_cpu_flow_restatement.py), against the same stages composed from the MD exports, and on partitioned lattices (world-size-1 RCCL with
LQCD_FORCE_PARTITION; two processes on the one GPU through the peer backend) against the single-domain run."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import flow_numpy as fn
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
EPS = 0.02


@pytest.fixture(scope="module")
def gpu():
    import latticeqcd_jl_amd as lq
    if lq.lib.device_count() < 1:
        pytest.skip("no HIP device")
    return lq


def _start(lq, case):
    if case == "ildg":
        L = (4, 4, 4, 4)
        U = lq.Gaugefields(lq.Lattice(L)).upload(lq.gauge_io.load_ildg(os.path.join(GOLDEN, "quenched_su3_4x4x4x4.ildg"), L))
    else:       # hot starts: (8,16,4,4) takes the tile form of the sweep (x-rows of 4, chunks of 16 whole rows), (6,4,4,4) the generic two-row form
        L = (8, 16, 4, 4) if case == "hot_tile" else (6, 4, 4, 4)
        U = gpu_hot(lq, L, 31)
    return L, U


def gpu_hot(lq, L, seed):
    return lq.Initialize_Gaugefields(3, 0, *L, condition="hot", randomseed=seed)


def _close(a, b, tol):
    return abs(a - b) <= tol * max(1.0, abs(b))


@pytest.mark.parametrize("case", ["ildg", "hot_tile", "hot_generic"])
def test_flow_and_observables_match_the_restatement(gpu, orc, case):
    lq = gpu
    L, U = _start(lq, case)
    U0 = U.download()
    lq.flow_(U, lq.Gradientflow(U, Nflow=10, eps=EPS))
    ref = fn.flow(U0, L, EPS, 10)
    assert np.abs(U.download() - ref).max() < 1e-12
    o, r = lq.gauge_flow_observables(U), fn.observables(ref, L)
    for k in fn.OBS:
        assert _close(o[k], r[k], 1e-12), (k, o[k], r[k])
    assert lq.calculate_energy_density(U, "plaquette") == o["E_plaq"] and lq.calculate_energy_density(U, "clover") == o["E_clov"]
    assert lq.calculate_topological_charge(U, "improved") == o["Q_impr"] and lq.calculate_topological_charge(U, "plaquette") == o["Q_plaq"]
    assert abs(o["p"] - lq.calculate_Plaquette(U)) < 1e-14


def test_flow_equals_the_composition_of_the_md_exports(gpu):
    """X <- a X + f TA(G), U <- exp(X) U as lqcd_link_scaled_copy + lqcd_momentum_add_gauge_force (beta = 6) + lqcd_gauge_exp_update, 20 steps at 16^3x32."""
    lq = gpu
    L = (16, 16, 16, 32)
    U = gpu_hot(lq, L, 41)
    W = lq.Gaugefields(U.lattice)
    lq.substitute_U_(W, U)
    X = lq.Gaugefields(U.lattice)
    f = lq.lib.lib()
    for _ in range(20):
        for a, c in ((0.0, 0.25), (-17.0 / 9.0, 8.0 / 9.0), (-1.0, 0.75)):
            for mu in range(4):
                lq.check(f.lqcd_link_scaled_copy(X._h, mu, C.c_double(a), X._h, mu))
            lq.check(f.lqcd_momentum_add_gauge_force(X._h, C.c_double(c * EPS), W._h, C.c_double(6.0)))
            lq.check(f.lqcd_gauge_exp_update(W._h, C.c_double(1.0), X._h))
    lq.check(f.lqcd_gradient_flow(U._h, C.c_double(EPS), 20))
    assert np.abs(U.download() - W.download()).max() < 1e-12


def test_measure_is_the_step_by_step_schedule_bit_for_bit_and_reproducible(gpu):
    lq = gpu
    L = (8, 16, 4, 4)
    runs = []
    for _ in range(2):
        U = gpu_hot(lq, L, 51)
        runs.append((lq.gradient_flow_measure(U, EPS, 12, 3), U.download()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    tab = runs[0][0]
    assert tab.shape == (4, 7) and np.allclose(tab[:, 0], EPS * np.arange(3, 13, 3), rtol=0, atol=1e-15)
    U = gpu_hot(lq, L, 51)
    rows = []
    for s in range(1, 13):
        lq.flow_(U, lq.Gradientflow(U, Nflow=1, eps=EPS))
        if s % 3 == 0:
            o = lq.gauge_flow_observables(U)
            rows.append([tab[len(rows), 0]] + [o[k] for k in fn.OBS])
    assert np.array_equal(np.array(rows), tab)
    assert np.array_equal(U.download(), runs[0][1])
    assert np.all(np.diff(tab[:, 2]) < 0)                        # E_plaq falls along the flow (dE_plaq/dt = (2/V) sum tr Z^2)
    t0, w0 = lq.flow_scales(tab)
    assert np.isnan(t0) or 0 < t0 <= tab[-1, 0]


def test_links_stay_unitary_over_100_steps(gpu):
    lq = gpu
    U = gpu_hot(lq, (8, 16, 4, 4), 61)
    lq.flow_(U, lq.Gradientflow(U, Nflow=100, eps=0.01))
    assert lq.unitarity_deviation(U) <= 1e-13
    Um = np.swapaxes(U.download(), -1, -2)
    assert np.abs(Um @ np.conj(np.swapaxes(Um, -1, -2)) - np.eye(3)).max() <= 1e-13


def test_dslash_on_the_flowed_handle_sees_the_flowed_links(gpu, orc):
    """An operator built before the flow (its cached 12-real / fp32 link copies made from the old links) applied after it: the version bump rebuilds them."""
    lq = gpu
    L, kappa, bc = (8, 16, 4, 4), 0.141139, (1, 1, 1, -1)
    U = gpu_hot(lq, L, 71)
    D = lq.Dirac_operator(U, None, {"Dirac_operator": "Wilson", "κ": kappa, "boundarycondition": bc})
    b = lq.Fermionfields(U.lattice, lq.WILSON)
    lq.gauss_distribution_fermion_(b, 72)
    y = b.similar()
    lq.mul_(y, D, b)
    lq.flow_(U, lq.Gradientflow(U, Nflow=3, eps=EPS))
    lq.mul_(y, D, b)
    ref = orc.wilson_D(U.download(), b.download(), L, kappa, 1.0, bc)
    assert np.abs(y.download() - ref).max() / np.abs(ref).max() < 1e-13


def test_rccl_self_partition_equals_the_single_domain_run(gpu, orc, tmp_path):
    lq = gpu
    L = (8, 4, 6, 8)
    Uh = orc.hot_gauge(L, 111)
    U = lq.Gaugefields(lq.Lattice(L)).upload(Uh)
    tab = lq.gradient_flow_measure(U, EPS, 6, 3)
    lq.flow_(U, lq.Gradientflow(U, Nflow=4, eps=EPS))
    o = lq.gauge_flow_observables(U)
    ref = os.path.join(str(tmp_path), "single.npz")
    np.savez(ref, U=U.download(), tab=tab, obs=np.array([o[k] for k in fn.OBS]))
    code = textwrap.dedent(f"""
        import os, sys, numpy as np
        sys.path.insert(0, os.getcwd())
        import latticeqcd_jl_amd as lq
        from oracle import oracle as orc
        L, EPS = {L!r}, {EPS!r}
        r = np.load({ref!r})
        lat = lq.Lattice(L)
        lat.comm_init(lq.comm_unique_id())
        U = lq.Gaugefields(lat).upload(orc.hot_gauge(L, 111))
        assert lat.get_param("staple_form_active") == -1
        tab = lq.gradient_flow_measure(U, EPS, 6, 3)
        lq.flow_(U, lq.Gradientflow(U, Nflow=4, eps=EPS))
        assert lat.get_param("staple_form_active") == 3      # the partitioned instance of the flow stage
        o = lq.gauge_flow_observables(U)
        close = lambda a, b: abs(a - b) <= 1e-13 * max(1.0, abs(b))
        assert np.abs(U.download() - r["U"]).max() < 1e-13
        for j, k in enumerate(("p", "E_plaq", "E_clov", "Q_plaq", "Q_clov")):
            assert close(o[k], r["obs"][j]), (k, o[k], r["obs"][j])
            assert all(close(tab[i, j + 1], r["tab"][i, j + 1]) for i in range(tab.shape[0])), (k, tab, r["tab"])
        assert np.isnan(o["Q_impr"]) and np.all(np.isnan(tab[:, 6]))
        print("RCCL_SELF_FLOW_OK")
    """)
    for mask in ("8", "15"):
        env = dict(os.environ, LQCD_FORCE_PARTITION=mask, HSA_ENABLE_IPC_MODE_LEGACY="0")
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120, cwd=ROOT)
        assert r.returncode == 0 and "RCCL_SELF_FLOW_OK" in r.stdout, (mask, r.stdout[-2000:], r.stderr[-3000:])


_port = [29740]


@pytest.mark.parametrize("pe", [(1, 1, 1, 2), (1, 1, 2, 1)])
def test_two_processes_peer_backend_equal_the_single_domain_run(gpu, pe):
    _port[0] += 1
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_port[0]), HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2",
               FLOW_TEST_LATTICE="8,4,8,8", FLOW_TEST_PE=",".join(map(str, pe)))
    env.pop("LQCD_FORCE_PARTITION", None)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", str(_port[0]), os.path.join(ROOT, "tests", "flow_peer_worker.py")],
                       capture_output=True, text=True, env=env, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-5000:]
    for k in range(2):
        assert f"FLOW_PEER_OK rank {k}" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
