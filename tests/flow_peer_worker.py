"""Worker of tests/test_gpu_gradient_flow.py: one of two real processes that share cuda:0 and run the gradient flow and its observables through the
peer-mapped backend (csrc/comm.hip), against a single-domain run of the same global lattice in the same process.  Run under torch.distributed.run."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import latticeqcd_jl_amd as lq  # noqa: E402
from oracle import oracle as orc  # noqa: E402

EPS, NSTEPS, EVERY = 0.02, 6, 3


def gather_blobs(blob):
    mine = torch.tensor(list(blob), dtype=torch.uint8)
    out = [torch.empty_like(mine) for _ in range(dist.get_world_size())]
    dist.all_gather(out, mine)
    return [bytes(t.tolist()) for t in out]


def close(a, b, tol=1e-13):
    return abs(a - b) <= tol * max(1.0, abs(b))


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    gL = tuple(int(v) for v in os.environ["FLOW_TEST_LATTICE"].split(","))
    pe = tuple(int(v) for v in os.environ["FLOW_TEST_PE"].split(","))
    assert int(np.prod(pe)) == world
    Uh = orc.hot_gauge(gL, 111)
    # the single-domain run of the global lattice
    lat1 = lq.Lattice(gL)
    U1 = lq.Gaugefields(lat1).upload(Uh)
    tab1 = lq.gradient_flow_measure(U1, EPS, NSTEPS, EVERY)
    lq.flow_(U1, lq.Gradientflow(U1, Nflow=2, eps=EPS))
    o1 = lq.gauge_flow_observables(U1)
    ref = U1.download()
    # the same on the PE grid
    lat = lq.Lattice(gL, pe, rank, device=0)
    lat.set_param("peer_timeout_ms", 20000)
    lat.comm_init_peer(gather_blobs)
    assert lat.comm_backend == "peer"
    U = lq.Gaugefields(lat).upload(lq.pegrid.local_view(Uh, lat.local_L, lat.origin, lead=1))
    tab = lq.gradient_flow_measure(U, EPS, NSTEPS, EVERY)
    lq.flow_(U, lq.Gradientflow(U, Nflow=2, eps=EPS))
    o = lq.gauge_flow_observables(U)
    loc = lq.pegrid.local_view(ref, lat.local_L, lat.origin, lead=1)
    err = float(np.abs(U.download() - loc).max())
    assert err < 1e-13, err
    for k in ("p", "E_plaq", "E_clov", "Q_plaq", "Q_clov"):
        assert close(o[k], o1[k]), (k, o[k], o1[k])
    assert np.isnan(o["Q_impr"]) and not np.isnan(o1["Q_impr"])
    assert tab.shape == tab1.shape
    for r in range(tab.shape[0]):
        assert tab[r, 0] == tab1[r, 0]
        for j in range(1, 6):
            assert close(tab[r, j], tab1[r, j]), (r, j, tab[r, j], tab1[r, j])
        assert np.isnan(tab[r, 6])
    vals = torch.tensor([o[k] for k in ("p", "E_plaq", "E_clov", "Q_clov")], dtype=torch.float64)
    allv = [torch.empty_like(vals) for _ in range(world)]
    dist.all_gather(allv, vals)
    assert all(torch.equal(v, allv[0]) for v in allv), "ranks disagree"
    print(f"FLOW_PEER_OK rank {rank} pe {pe} err {err:.2e}", flush=True)
    dist.barrier()
    lat.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
