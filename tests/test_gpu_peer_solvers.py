"""Every rank-coupled solver and force between REAL processes: N ranks that share the one GPU of the test box and communicate through the peer-mapped backend
(csrc/comm.hip), each case against the CPU oracle's result on the global lattice.  What tests/test_gpu_peer_world2.py left to the self-mapped runs (one rank whose
window points at itself, where a reduction counter can never disagree and a corner is the rank's own memory): the even-odd and the plain BiCGStab, Wilson-clover with
its force, the mixed-precision solvers, the multi-shift CG and the rational action, Domainwall, stout with its back-propagation, the gauge side and two leapfrog
steps of the Wilson HMC -- tests/peer_solvers_worker.py holds the cases and cites the single-domain test each bound comes from.

Worlds (tests/peer_refs.py WORLDS): global 4.4.4.8 on (1,1,1,2), (1,1,2,1), (1,1,2,2) [the diagonal rank: corners of a third process] and (1,1,1,4) [a ring: the
forward and the backward neighbour differ]; 16.4.4.4 on (2,1,1,1) [the per-lane ghost selects of the x fold].  One torch.distributed.run launch per world runs all
its cases; the references are computed once per global shape, in this process, before the first launch.

Two departures from the issue this file answers, both because of what the library is:
  * case 8 runs the plaquette action only.  The rectangle entry points REFUSE a partitioned lattice (csrc/rectangle.hip: they need a halo of depth 2;
    test_gpu_rect_action.py::test_partitioned_lattice_is_refused pins that), so beta_rect != 0 cannot be compared with tests/rect_numpy.py between ranks; the case pins
    the refusal on every rank instead (no reduction issued, outputs untouched) and compares the plaquette term with rect_numpy at beta_rect = 0.
  * world z2 runs (1,-1,1,1), the boundary condition the issue names, and (1,1,-1,1), the one that puts the sign on the partitioned z face as the issue intends.

Safety on the shared GPU: a rank that fails prints PEER_SOLVERS_FAIL and leaves at once (the others meet peer_timeout_ms once); a world that ends by signal or
time-out, or whose output speaks of an illegal memory access, makes every later world of this file fail without launching."""
import os
import re
import signal
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import peer_refs  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_port = [29840]
_faulted = []          # the world that faulted, hung or died by a signal: nothing of this file is launched after it

# seconds: about five times the duration measured on an MI355X (t2 10.3 s, z2 14.0 s, zt4 15.8 s, t4 6.1 s, x2 4.9 s), rounded up to 30 s
TIMEOUT = {"t2": 60, "z2": 90, "zt4": 90, "t4": 60, "x2": 30}


@pytest.fixture(scope="module")
def refs(tmp_path_factory, orc):
    """one .npz per global shape with every boundary condition and case its worlds need; every oracle solve behind it converged"""
    d = tmp_path_factory.mktemp("peer_refs")
    need = {}
    for L, pe, bcs, cases in peer_refs.WORLDS.values():
        b, c = need.setdefault(L, ([], set()))
        b += [bc for bc in bcs if bc not in b]
        c.update(cases)
    out = {}
    for L, (bcs, cases) in need.items():
        out[L] = str(d / ("refs_" + "x".join(map(str, L)) + ".npz"))
        status = peer_refs.build(L, out[L], bcs=bcs, cases=tuple(sorted(cases)))
        assert all(st == 0 for st in status.values()), status
    return out


@pytest.fixture(scope="module")
def gpu():
    import latticeqcd_jl_amd as lq
    if lq.lib.device_count() < 1:
        pytest.skip("no HIP device")
    return lq


@pytest.mark.parametrize("world", ["t2", "z2", "zt4", "t4", "x2"])
def test_solvers_and_forces_between_processes_equal_the_oracle(gpu, refs, world):
    if _faulted:
        pytest.fail("earlier world faulted: " + _faulted[0])
    L, pe, _, _ = peer_refs.WORLDS[world]
    n = 1
    for v in pe:
        n *= v
    _port[0] += 1
    # the environment of tests/test_gpu_peer_world2.py, plus the world's name and the reference file
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_port[0]), HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2",
               PEER_SOLVERS_WORLD=world, PEER_SOLVERS_REF=refs[L])
    env.pop("LQCD_FORCE_PARTITION", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1", "--master-port", str(_port[0]),
           os.path.join(ROOT, "tests", "peer_solvers_worker.py")]
    # a session of its own: at the time limit the launcher AND its ranks are killed, nothing is left running on the GPU
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, cwd=ROOT, start_new_session=True)
    try:
        out, err = proc.communicate(timeout=TIMEOUT[world])
    except subprocess.TimeoutExpired:
        os.killpg(proc.pid, signal.SIGKILL)
        out, err = proc.communicate()
        _faulted.append(world + " (timed out)")
        pytest.fail("world %s ran into its time limit of %d s\n%s" % (world, TIMEOUT[world], out[-6000:] + err[-3000:]))
    r = subprocess.CompletedProcess(cmd, proc.returncode, out, err)
    tail = r.stdout[-6000:] + r.stderr[-6000:]
    # (a rank killed by a signal: the launcher itself returns 1 and reports "exitcode  : -11 (pid: ...)")
    if r.returncode < 0 or re.search(r"illegal memory access|Memory access fault|exitcode\s*:\s*-\d+", r.stdout + r.stderr):
        _faulted.append("%s (exit status %d)" % (world, r.returncode))
    print(r.stdout)          # every figure of every rank (shown when the test fails, or with -rP)
    assert r.returncode == 0, tail
    for k in range(n):
        assert f"PEER_SOLVERS_OK rank {k} " in r.stdout, tail
    assert "PEER_SOLVERS_FAIL" not in r.stdout
