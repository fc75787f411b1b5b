"""Worker of tests/test_gpu_meson.py: one of two real processes that share cuda:0 and measure the meson correlators through the peer-mapped backend
(csrc/comm.hip), against the single-domain tables of the same global lattice saved by the test.  Run under torch.distributed.run."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import latticeqcd_jl_amd as lq  # noqa: E402
from oracle import oracle as orc  # noqa: E402

KAPPA, SRC = 0.125, (1, 2, 3, 5)
TOL_CONTRACT, TOL_SOLVE = 1e-13, 1e-8


def gather_blobs(blob):
    mine = torch.tensor(list(blob), dtype=torch.uint8)
    out = [torch.empty_like(mine) for _ in range(dist.get_world_size())]
    dist.all_gather(out, mine)
    return [bytes(t.tolist()) for t in out]


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    gL = tuple(int(v) for v in os.environ["MESON_TEST_LATTICE"].split(","))
    pe = tuple(int(v) for v in os.environ["MESON_TEST_PE"].split(","))
    ref = np.load(os.environ["MESON_TEST_REF"])
    assert int(np.prod(pe)) == world
    lat = lq.Lattice(gL, pe, rank, device=0)
    lat.set_param("peer_timeout_ms", 20000)
    lat.comm_init_peer(gather_blobs)
    assert lat.comm_backend == "peer"
    U = lq.Gaugefields(lat).upload(lq.pegrid.local_view(orc.hot_gauge(gL, 111), lat.local_L, lat.origin, lead=1))
    D = lq.Dirac_operator(U, None, {"Dirac_operator": "Wilson", "κ": KAPPA, "eps_CG": 1e-19, "method_CG": "bicgstab_evenodd"})
    tab = lq.meson_correlators(D, SRC)
    err = float((np.abs(tab - ref["tab"]) / ref["tab"][15]).max())
    assert err < TOL_SOLVE, err
    f = [lq.Fermionfields(lat, lq.WILSON).upload(lq.pegrid.local_view(orc.gaussian_spinor(orc.wilson_shape(gL), 200 + j), lat.local_L, lat.origin, lead=1))
         for j in range(12)]
    ctab = lq.meson_contract(f)
    cerr = float((np.abs(ctab - ref["ctab"]) / ref["ctab"][15]).max())
    assert cerr < TOL_CONTRACT, cerr
    n2 = lq.norm2_timeslices(f[0])
    full = (np.abs(orc.gaussian_spinor(orc.wilson_shape(gL), 200)) ** 2).sum(axis=(0, 2, 3, 4, 5))
    assert np.abs(n2 / full - 1.0).max() < TOL_CONTRACT
    for v in (tab, ctab):
        vals = torch.tensor(v, dtype=torch.float64)
        allv = [torch.empty_like(vals) for _ in range(world)]
        dist.all_gather(allv, vals)
        assert all(torch.equal(x, allv[0]) for x in allv), "ranks disagree"
    print(f"MESON_PEER_OK rank {rank} pe {pe} origin {lat.origin} err {err:.2e} contract {cerr:.2e}", flush=True)
    dist.barrier()
    lat.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
