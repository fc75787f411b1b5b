"""The numpy restatement of the heatbath (tests/heatbath_numpy.py) against what it must be, on the CPU: the y0 samplers draw the SU(2) heatbath
density, the overrelaxation sweep is microcanonical, the sweeps keep the links on the group, and the sweep counter keys the draws so that a run split
into calls is the run in one call.  tests/test_gpu_heatbath.py holds the device to this restatement."""
import math

import numpy as np
import pytest

import heatbath_numpy as hn
from oracle import oracle as orc

L = (2, 2, 2, 4)


def _density_cdf(alpha, edges):
    """CDF of ~ sqrt(1 - y^2) exp(alpha y) on [-1, 1] at the bin edges (fine trapezoid rule)."""
    y = np.linspace(-1.0, 1.0, 400001)
    f = np.sqrt(np.clip(1.0 - y * y, 0.0, None)) * np.exp(alpha * (y - 1.0))
    F = np.concatenate([[0.0], np.cumsum(0.5 * (f[1:] + f[:-1]) * np.diff(y))])
    return np.interp(edges, y, F / F[-1])


@pytest.mark.parametrize("alpha", [0.0, 0.5, 2.0, 12.0])
@pytest.mark.parametrize("branch", ["creutz", "kp"])
def test_y0_sampler_draws_the_su2_heatbath_density(alpha, branch):
    if branch == "kp" and alpha == 0.0:
        branch = "haar"          # Kennedy-Pendleton needs alpha > 0: the alpha = 0 branch is the exact Haar one
    n, nbins = 20000, 20
    ys = np.array([hn.sample_y0(alpha, hn.hb_key(2024, s, 0, 0, 0), 10**5, branch=branch) for s in range(n)])
    # equal-probability bins of the exact density
    grid = np.linspace(-1.0, 1.0, 200001)
    cdf = _density_cdf(alpha, grid)
    edges = np.interp(np.linspace(0.0, 1.0, nbins + 1), cdf, grid)
    edges[0], edges[-1] = -1.0, 1.0
    obs, _ = np.histogram(ys, bins=edges)
    exp = n * np.diff(_density_cdf(alpha, edges))
    chi2 = float(np.sum((obs - exp) ** 2 / exp))
    # 19 degrees of freedom: P(chi2 > 43.8) = 0.001
    assert chi2 < 43.8, (alpha, branch, chi2)
    assert np.all(np.abs(ys) <= 1.0)


def test_or_sweep_keeps_every_local_action_and_the_total():
    U = orc.hot_gauge(L, 5)
    U = hn.run(U, L, 5.7, 1)
    before = hn.local_action(U, L)
    # each link's Re tr(U A) with A as the sweep saw it: the reflection keeps it link by link, so the total is kept too
    Um = orc._mat(U).copy()
    for mu in range(4):
        for p in range(2):
            A = orc._staple_sum(Um, L, mu)
            for idx in np.ndindex(*Um.shape[1:5]):
                t, z, y, x = idx
                if (x + y + z + t) % 2 != p:
                    continue
                u = Um[(mu,) + idx]
                new, _ = hn.link_update(u, A[idx], True)
                assert abs(np.trace(new @ A[idx]).real - np.trace(u @ A[idx]).real) <= 1e-13 * max(1.0, abs(np.trace(u @ A[idx]).real))
                Um[(mu,) + idx] = new
    after = hn.local_action(np.ascontiguousarray(orc._mat(Um)), L)
    assert abs(after.sum() - before.sum()) <= 1e-13 * abs(before.sum())
    U2, capped = hn.sweep(U, L, True)
    assert capped == 0 and np.abs(U2 - np.ascontiguousarray(orc._mat(Um))).max() == 0.0


@pytest.mark.parametrize("beta", [0.0, 6.0])
def test_hb_sweeps_keep_the_links_on_the_group(beta):
    counts = {}
    U = hn.run(orc.hot_gauge(L, 7), L, beta, 2, counts=counts)
    dev, ddet = hn.unitarity(U)
    assert dev <= 1e-14 and ddet <= 1e-14, (dev, ddet)
    assert counts.get("haar" if beta == 0.0 else "kp", 0) > 0, counts


def test_chunked_sweeps_equal_the_unchunked_run():
    U0 = orc.hot_gauge(L, 9)
    one = hn.run(U0, L, 5.7, 3, nor=1, seed=42)
    U = U0
    for s in range(3):
        U = hn.run(U, L, 5.7, 1, nor=1, seed=42, first_sweep=s)
    assert np.array_equal(U, one)
    other = hn.run(U0, L, 5.7, 3, nor=1, seed=43)
    assert not np.array_equal(other, one)


def test_itmax_one_runs_out_and_leaves_the_links_on_the_group():
    U, capped = hn.sweep(orc.hot_gauge(L, 11), L, False, 5.7, itmax=1, seed=1)
    assert capped > 0
    assert max(hn.unitarity(U)) <= 1e-14


def test_heatbath_raises_the_plaquette_towards_equilibrium():
    U = orc.hot_gauge(L, 13)
    p0 = hn.plaquette(U, L)
    assert abs(p0 - orc.plaquette(U, L)) < 1e-13
    U = hn.run(U, L, 6.0, 3)
    assert hn.plaquette(U, L) > p0 + 0.2
    assert not math.isnan(hn.plaquette(U, L))
