"""The reference builder of tests/test_gpu_peer_solvers.py, without a GPU: every oracle solve behind the file converges at each global shape, and the
ranks' local views of every PE grid used tile the global array exactly once."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import peer_refs  # noqa: E402


def _shapes():
    """global shape -> (union of the boundary conditions, union of the cases) over the worlds that use it"""
    out = {}
    for L, pe, bcs, cases in peer_refs.WORLDS.values():
        b, c = out.setdefault(L, (set(), set()))
        b.update(bcs); c.update(cases)
    return out


@pytest.mark.parametrize("L", sorted(_shapes()), ids=lambda L: "x".join(map(str, L)))
def test_every_oracle_solve_converges(orc, tmp_path, L):
    bcs, cases = _shapes()[L]
    path = str(tmp_path / "refs.npz")
    status = peer_refs.build(L, path, bcs=sorted(bcs, reverse=True), cases=tuple(sorted(cases)))
    assert status and all(st == 0 for st in status.values()), status
    ref = np.load(path)
    assert all(np.isfinite(ref[k]).all() for k in ref.files)
    for bc in bcs:                    # every case asked for left its keys under every boundary condition
        for c in cases - {7, 8}:
            assert any(k.startswith("%s/c%d/" % (peer_refs.bc_tag(bc), c)) for k in ref.files), (bc, c)
    for c in cases & {7, 8}:
        assert any(k.startswith("g/c%d/" % c) for k in ref.files), c


@pytest.mark.parametrize("world", sorted(peer_refs.WORLDS))
def test_local_views_tile_the_global_array_exactly_once(lq, world):
    pegrid = lq.pegrid
    L, pe, _, _ = peer_refs.WORLDS[world]
    n = int(np.prod(pe))
    for lead, shape in ((1, (4, L[3], L[2], L[1], L[0], 3, 3)), (0, (L[3], L[2], L[1], L[0], 3)), (2, (2, 4, L[3], L[2], L[1], L[0], 3))):
        ident = np.arange(int(np.prod(shape)), dtype=np.int64).reshape(shape)      # every element names itself
        seen = np.zeros(ident.size, dtype=np.int64)
        for rank in range(n):
            local, origin, _, _ = pegrid.decompose(L, pe, rank)
            v = pegrid.local_view(ident, local, origin, lead=lead)
            want = list(shape)
            for k, mu in enumerate((3, 2, 1, 0)):
                want[lead + k] = local[mu]
            assert v.shape == tuple(want)
            np.add.at(seen, v.ravel(), 1)
            # the view is the block at the rank's origin: its first element is the global element at the origin
            idx = [0] * len(shape)
            for k, mu in enumerate((3, 2, 1, 0)):
                idx[lead + k] = origin[mu]
            assert v.ravel()[0] == ident[tuple(idx)]
        assert (seen == 1).all(), (world, lead)
