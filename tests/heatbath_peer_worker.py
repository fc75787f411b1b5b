"""Worker of tests/test_gpu_heatbath.py: one of two real processes that share cuda:0 and run heatbath + overrelaxation updates through the peer-mapped
backend (csrc/comm.hip), against a single-domain run of the same global lattice in the same process.  Run under torch.distributed.run."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import latticeqcd_jl_amd as lq  # noqa: E402
from oracle import oracle as orc  # noqa: E402

BETA, NUPD, NOR = 5.7, 2, 3


def gather_blobs(blob):
    mine = torch.tensor(list(blob), dtype=torch.uint8)
    out = [torch.empty_like(mine) for _ in range(dist.get_world_size())]
    dist.all_gather(out, mine)
    return [bytes(t.tolist()) for t in out]


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    gL = tuple(int(v) for v in os.environ["HB_TEST_LATTICE"].split(","))
    pe = tuple(int(v) for v in os.environ["HB_TEST_PE"].split(","))
    assert int(np.prod(pe)) == world
    Uh = orc.hot_gauge(gL, 111)
    # the single-domain run of the global lattice
    U1 = lq.Gaugefields(lq.Lattice(gL)).upload(Uh)
    tab1 = lq.heatbath_measure(U1, lq.Heatbath(U1, BETA, seed=5), NUPD, numOR=NOR)
    ref = U1.download()
    # the same on the PE grid
    lat = lq.Lattice(gL, pe, rank, device=0)
    lat.set_param("peer_timeout_ms", 20000)
    lat.comm_init_peer(gather_blobs)
    assert lat.comm_backend == "peer"
    U = lq.Gaugefields(lat).upload(lq.pegrid.local_view(Uh, lat.local_L, lat.origin, lead=1))
    tab = lq.heatbath_measure(U, lq.Heatbath(U, BETA, seed=5), NUPD, numOR=NOR)
    loc = lq.pegrid.local_view(ref, lat.local_L, lat.origin, lead=1)
    err = float(np.abs(U.download() - loc).max())
    assert err <= 1e-12, err
    assert np.abs(tab - tab1).max() <= 1e-12, (tab, tab1)
    vals = torch.tensor(tab, dtype=torch.float64)
    allv = [torch.empty_like(vals) for _ in range(world)]
    dist.all_gather(allv, vals)
    assert all(torch.equal(v, allv[0]) for v in allv), "ranks disagree"
    print(f"HB_PEER_OK rank {rank} pe {pe} err {err:.2e}", flush=True)
    dist.barrier()
    lat.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
