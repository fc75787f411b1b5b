"""The numpy restatement of the gradient flow and of its observables (tests/flow_numpy.py), checked without reference to itself: the Euler step is a stout
step, the flow decreases E at the rate its generator gives, the integrator is of third order, the observables are gauge invariant, the charges are odd
under a reflection, and a constant abelian flux has the charge its flux quanta give and does not flow."""
import numpy as np
import pytest

import flow_numpy as fn

L = (4, 4, 2, 4)


def test_euler_step_is_a_stout_step(orc):
    U = orc.hot_gauge(L, 21)
    for eps in (0.01, 0.05):
        assert np.abs(fn.euler_step(U, L, eps) - orc.stout_smear(U, L, eps)).max() < 1e-13


def test_plaquette_energy_decreases_at_the_rate_of_the_generator(orc):
    """S = 2 sum_plaq Re tr(1 - P) is the Wilson action at beta = 6, so E_plaq = S / V.  With dU/dtau = P U the HMC conserves H = -sum tr P^2 + S and
    dP/dtau = TA(G) = Z, so dS/dtau = 2 sum tr(P Z) for any P; along the flow P = Z:  dE_plaq/dt = (2/V) sum_{x,mu} tr Z_mu(x)^2  (<= 0: Z is anti-Hermitian)."""
    U = fn.flow(orc.hot_gauge(L, 22), L, 0.02, 5)
    V = float(np.prod(L))
    Z = fn.flow_Z(orc._mat(U), L)
    rate = 2.0 / V * float(np.einsum("...ab,...ba->...", Z, Z).real.sum())
    h = 1e-3
    dE = (fn.observables(fn.rk3_step(U, L, h), L)["E_plaq"] - fn.observables(fn.rk3_step(U, L, -h), L)["E_plaq"]) / (2 * h)
    assert rate < 0
    assert abs(dE - rate) < 1e-5 * abs(rate), (dE, rate)


def test_the_integrator_is_third_order(orc):
    U0 = fn.flow(orc.hot_gauge(L, 23), L, 0.01, 3)
    t = 0.2
    ref = fn.flow(U0, L, t / 160, 160)
    errs = [np.abs(fn.flow(U0, L, t / n, n) - ref).max() for n in (4, 8, 16)]
    for a, b in zip(errs, errs[1:]):
        assert 6.0 < a / b < 10.0, errs


def test_plaquette_energy_is_36_times_one_minus_p(orc):
    U = fn.flow(orc.hot_gauge(L, 24), L, 0.02, 2)
    o = fn.observables(U, L)
    assert abs(o["p"] - orc.plaquette(U, L)) < 1e-14
    assert abs(o["E_plaq"] - 36.0 * (1.0 - o["p"])) < 1e-12


def test_observables_are_gauge_invariant(orc):
    U = fn.flow(orc.hot_gauge(L, 25), L, 0.03, 3)
    a, b = fn.observables(U, L), fn.observables(fn.gauge_transform(U, L, 26), L)
    for k in fn.OBS:
        assert abs(a[k] - b[k]) < 1e-12 * max(1.0, abs(a[k])), (k, a[k], b[k])


def test_charges_flip_under_a_reflection_and_energy_does_not(orc):
    U = fn.flow(orc.hot_gauge(L, 27), L, 0.03, 3)
    a, b = fn.observables(U, L), fn.observables(fn.reflect_x(U), L)
    assert abs(a["Q_clov"]) > 1e-4
    for k in ("Q_clov", "Q_impr"):          # (the single plaquette leaf at x is no symmetric loop set: Q_plaq is odd only up to lattice artefacts)
        assert abs(a[k] + b[k]) < 1e-12, (k, a[k], b[k])
    for k in ("p", "E_plaq", "E_clov"):
        assert abs(a[k] - b[k]) < 1e-12, (k, a[k], b[k])


@pytest.mark.parametrize("n01,n23", [(1, 1), (1, 2), (1, -1)])
def test_abelian_flux_has_its_charge_and_does_not_flow(orc, n01, n23):
    """Only the (0,1) and (2,3) planes carry flux; every leaf of those planes is diag(e^{i th}, e^{-i th}, 1), so G_01 = diag(i sin th, -i sin th, 0)
    (likewise G_23 with th'), tr G01 G23 = -2 sin th sin th' and Q_clov = V sin th sin th' / (2 pi^2) -> 2 n01 n23 as th = 2 pi n01 / (L0 L1),
    th' = 2 pi n23 / (L2 L3) -> 0.  The staple sum of every link is e^{i th} + e^{-i th} times the link: Hermitian, so Z = 0."""
    L8 = (8, 8, 8, 8)
    U = fn.flux_gauge(L8, n01, n23)
    o = fn.observables(U, L8)
    q = 2.0 * n01 * n23
    assert abs(o["Q_clov"] - q) < 0.01 * abs(q), o
    assert abs(o["Q_impr"] - q) < 0.01 * abs(q), o
    assert np.abs(fn.rk3_step(U, L8, 0.05) - U).max() < 1e-13
