"""The store policy by slab of the CG's stencil launches (tunable cg_store_keep_mb, StencilCall::keep_slabs, PipeArgs::keep_from; stencil.hip sdir_wave's epilogue): where
the sweep alternates, the workgroups of the last K_s slabs a launch runs store plain and every other one streams its store.  A store hint changes no value, so every
setting is compared bit for bit with the policy off (-1) in the same library: the settings that resolve to 0, 1, nslab - 1 and nslab slabs on 16.8.8.4 (4 slabs of
884736 B of launch traffic) and 16.16.16.8 (8 slabs of 3538944 B), both in temporal gauge with cg_small = 0, on the smooth-link systems of tests/rring_deep.py."""
import numpy as np
import pytest

import hard_systems as hs
import rring_deep as rd
from test_gpu_cg_rring_deep import form, smooth, window

pytestmark = pytest.mark.gpu

K, M = 8, 2
DEPTH = K * M
N = 3 * DEPTH + 5                 # crosses three batch boundaries and ends inside the fourth batch
NSLAB = {rd.SMALL: 4, rd.BIG: 8}
BYTES_PER_SITE = 864              # what a stencil launch of the iteration moves per site (cg.hip CG_STENCIL_BYTES)


def slab_bytes(L):
    return BYTES_PER_SITE * (int(np.prod(L)) // NSLAB[L])


def settings(L):
    """[(cg_store_keep_mb, slabs it resolves to)] for 0, 1, nslab - 1, nslab slabs: the smallest number of MB that reaches each"""
    out = []
    for k in (0, 1, NSLAB[L] - 1, NSLAB[L]):
        mb = -(-k * slab_bytes(L) // (1 << 20))
        assert min((mb << 20) // slab_bytes(L), NSLAB[L]) == k
        out.append((mb, k))
    return out + [(1 << 10, NSLAB[L])]      # far beyond the launch: clamped


def system(lq, orc, L, eps=None):
    s, lat, U, D, b = smooth(lq, orc, L, K, M, eps=eps)
    lat.set_param("cg_tgauge", 2)            # (both shapes: the sweep alternates in temporal gauge only)
    assert lat.get_param("cg_sweep_alt") == 1
    return s, lat, U, D, b


def reference(lq, lat, D, b, n):
    lat.set_param("cg_store_keep_mb", -1)
    ref = window(lq, D, b, n)
    assert lat.get_param("cg_store_keep_active") == -1
    return ref


def check_window(lq, lat, D, b, n, ref, mb, want):
    lat.set_param("cg_store_keep_mb", mb)
    got = window(lq, D, b, n)
    assert lat.get_param("tgauge_active") == 1
    assert lat.get_param("cg_store_keep_active") == want, (mb, want)
    assert np.array_equal(got, ref), (mb, want)


@pytest.mark.parametrize("L", rd.LATTICES, ids=lambda L: ".".join(map(str, L)))
def test_residual_ring_windows_and_a_converging_solve_are_the_same_bits(lq, orc, L):
    bh = hs.rhs(orc, rd.smooth(L))
    s, lat, U, D, b = system(lq, orc, L, eps=1e-6 * float(np.vdot(bh, bh).real))
    ref = reference(lq, lat, D, b, N)
    assert (lat.get_param("cg_rring_active"), lat.get_param("cg_rring_depth_active")) == (K, DEPTH)
    assert lat.get_param("cg_sweep_alt_active") == 1
    xs = b.similar()
    it0, rr0 = lq.solve_DinvX_(xs, lq.DdagD_operator(D), b, return_info=True)      # converges inside a batch: the flush behind the converging iteration
    print("L", L, "solve to 1e-6 |b|^2:", it0, "iterations, k mod depth", it0 % DEPTH)
    assert it0 > DEPTH
    xs = xs.download()
    for mb, want in settings(L):
        check_window(lq, lat, D, b, N, ref, mb, want)
        x = b.similar()
        it, rr = lq.solve_DinvX_(x, lq.DdagD_operator(D), b, return_info=True)
        assert lat.get_param("cg_store_keep_active") == want
        assert (it, rr) == (it0, rr0) and np.array_equal(x.download(), xs), (mb, want)
    # a captured burst replays the policy it was captured with
    lat.set_param("graph", 1)
    for mb, want in [(-1, -1)] + settings(L)[:3]:
        check_window(lq, lat, D, b, N, ref, mb, want)
    lat.set_param("graph", 0)
    # without the alternating sweep the policy stays off
    lat.set_param("cg_sweep_alt", 0)
    check_window(lq, lat, D, b, N, ref, settings(L)[1][0], -1)
    assert np.array_equal(b.download(), bh)


def test_the_deferred_x_form_is_the_same_bits_forwards_and_backwards(lq, orc):
    L = rd.BIG
    s, lat, U, D, b = system(lq, orc, L)
    form(lat, 2)
    for graph in (0, 1):
        lat.set_param("graph", graph)
        lat.set_param("cg_sweep_alt", 1)
        ref = reference(lq, lat, D, b, N)
        assert lat.get_param("cg_rring_active") == 0 and lat.get_param("cg_sweep_alt_active") == 1
        for mb, want in settings(L):
            check_window(lq, lat, D, b, N, ref, mb, want)
            assert lat.get_param("sweep_rev_active") == 1
        lat.set_param("cg_sweep_alt", 0)          # D^+ forwards: today's policy whatever the key says
        for mb, want in settings(L)[:2]:
            check_window(lq, lat, D, b, N, ref, mb, -1)
            assert lat.get_param("sweep_rev_active") == 0
        lat.set_param("cg_store_keep_mb", -1)


@pytest.mark.parametrize("L", rd.LATTICES, ids=lambda L: ".".join(map(str, L)))
def test_plain_applications_ignore_the_key(lq, orc, L):
    s, lat, U, D, b = system(lq, orc, L)
    out = []
    for mb in (-1, settings(L)[1][0], 0):
        lat.set_param("cg_store_keep_mb", mb)
        row = []
        for op in (D, D.adjoint()):
            y = b.similar()
            lq.mul_(y, op, b)
            row.append(y.download())
        out.append(row)
    for row in out[1:]:
        assert np.array_equal(row[0], out[0][0]) and np.array_equal(row[1], out[0][1])


def test_the_key_refuses_values_below_minus_one_and_a_launch_bound_context_keeps_it_off(lq, orc):
    s, lat, U, D, b = system(lq, orc, rd.SMALL)
    default = lat.get_param("cg_store_keep_mb")
    with pytest.raises(lq.LQCDError):
        lat.set_param("cg_store_keep_mb", -2)
    assert lat.get_param("cg_store_keep_mb") == default
    window(lq, D, b, 3)
    assert lat.get_param("cg_store_keep_active") == -1      # 64 stencil workgroups and the key never set
