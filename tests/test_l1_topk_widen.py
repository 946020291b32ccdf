"""The threshold search of K23 (l2t_widen<false> in csrc/topk_filter_tile.h, on l2f_thresholds<false> of
csrc/l2_filter_tile.h) in a Python port, IEEE double like the device code: no GPU needed.

Distance space is the L1 distance itself -- no square, no square root.  DESIGN s4 "K23" quotes two facts from this
port: the first guess of the slack is accepted over the whole range of witness bounds under the four (alpha, beta) of
the GPU tests, and the threshold it yields lies within 7 rho + 300u (relative) of the witnesses' bound.  Exactness does
not rest on either -- the device CHECKS the deciding inequality and leaves the query unresolved when it fails -- but a
slack that stopped being accepted would send queries to the fp64 route for nothing.  The port is kept line for line
with the device functions."""
import math

import numpy as np
import pytest

U = 2.0 ** -53
INF = math.inf
TINY = 2.0 ** -1074


def thresholds(t, alpha, beta, rho):
    """l2f_thresholds<false> for a finite t: (tb, tn)"""
    pos = alpha > 0.0
    x = (t - beta) / alpha
    sig = 16.0 * U * ((abs(t) + abs(beta)) / abs(alpha)) + 1e-290
    sig += TINY / abs(alpha)
    xlo, xhi = x - sig, x + sig
    lo, hi = xlo * (1.0 - rho), xhi * (1.0 + 2.0 * rho)
    lo_t = lo * (1.0 - 4.0 * U) if xlo > 0.0 else -INF
    hi_t = hi * (1.0 + 4.0 * U) if xhi > 0.0 else 0.0
    return (lo_t, hi_t) if pos else (hi_t, lo_t)


def widen(tau, alpha, beta, rho):
    """l2t_widen<false>: (iterations used, t, threshold) or None when there is no threshold"""
    pos = alpha > 0.0
    if not abs(tau) < INF:
        return None
    dt = max(tau, 0.0) if pos else -tau
    if not pos and not dt > 0.0:
        return None
    y = dt
    slack = 4.0 * rho * y + 64.0 * U * (y + 2.0 * abs(beta) / abs(alpha)) + 1e-280
    slack += 4.0 * (TINY / abs(alpha))
    for it in range(12):
        yy = y + slack if pos else y - slack
        t = alpha * yy + beta
        tb, tn = thresholds(t, alpha, beta, rho)
        if (tb > dt) if pos else (tb < dt):
            return it, t, tn
        slack *= 4.0
    return None


def _cases(d):
    return [(1.0, 0.0), (-1.0 / d, -1.0), (1.0, -1.0), (-1.0 / d, 0.0)]


@pytest.mark.parametrize("d", [67, 1024])
def test_first_guess_is_accepted_and_tight(d):
    rho = 2.0 * (d + 16.0) * U
    worst = 0.0
    for alpha, beta in _cases(d):
        for dt in 10.0 ** np.arange(-30.0, 31.0):
            tau = dt if alpha > 0 else -dt
            got = widen(float(tau), alpha, beta, rho)
            assert got is not None and got[0] == 0, (alpha, beta, dt, got)
            tn = got[2]
            # the threshold is on the far side of the witnesses' bound ...
            assert tn > dt if alpha > 0 else tn < dt
            # ... and close to it.  From the formulas: the slack moves y by 4 rho + 64u (1 + 2 |beta| / (|alpha| y)),
            # l2f_thresholds<false> by 2 rho + 4u + its sigma <= 16u (2 + |beta| / (|alpha| y)); nothing is squared:
            # where beta does not swamp the distance term, |tn - dt| <= (6 rho + 276u) dt (plus rho^2 terms: 7 rho)
            if abs(alpha) * dt >= abs(beta):
                rel = abs(tn - dt) / dt
                worst = max(worst, rel)
                assert rel <= 7.0 * rho + 300.0 * U, (alpha, beta, dt, tn)
    print("d %d: tn(t) lies within %.3g (relative) of D_tau; 7 rho + 300u = %.3g" % (d, worst, 7.0 * rho + 300.0 * U))


def test_no_threshold_where_there_is_none():
    rho = 2.0 * (1024 + 16.0) * U
    assert widen(INF, 1.0, 0.0, rho) is None and widen(float("nan"), 1.0, 0.0, rho) is None
    # alpha < 0 and witnesses whose distances have no positive lower bound
    assert widen(0.0, -1.0 / 1024, -1.0, rho) is None and widen(5.0, -1.0 / 1024, -1.0, rho) is None
    # a bound of exactly zero under alpha > 0 has a threshold in L1 space (nothing is squared, so the guess does not
    # underflow): an all-duplicates witness set still excludes the rest of the gallery
    got = widen(0.0, 1.0, 0.0, rho)
    assert got is not None and 0.0 < got[2] < 1e-270


@pytest.mark.parametrize("d", [67, 1024])
def test_threshold_separates_the_words(d):
    """What launch B relies on, on words formed as the canonical chain forms them from an exactly known S:
    a witness (L on the near side of the bound) has a word < t, a column beyond the threshold a word >= t."""
    rho = 2.0 * (d + 16.0) * U
    rng = np.random.default_rng(d)
    for alpha, beta in _cases(d):
        for dt in (1e-3, 1.0, 0.25 * d, 2.0 * d, 1e6):
            tau = dt if alpha > 0 else -dt
            _, t, tn = widen(float(tau), alpha, beta, rho)
            # S = L (1 + eta), |eta| <= (d + 4) 2u: the chain's own roundings of the differences and of the sum
            # (DESIGN s4, K22 step 3)
            eta = (d + 4.0) * 2.0 * U * rng.uniform(-1.0, 1.0, 2000)
            near = dt * (1.0 - rng.uniform(0.0, 1e-9, 2000)) if alpha > 0 else dt * (1.0 + rng.uniform(0.0, 1e-9, 2000))
            far = tn * (1.0 + rng.uniform(1e-16, 1e-9, 2000)) if alpha > 0 else tn * (1.0 - rng.uniform(1e-16, 1e-9, 2000))
            near[0], far[0] = dt, np.nextafter(tn, INF if alpha > 0 else -INF)
            word = lambda L: alpha * (L * (1.0 + eta)) + beta
            assert (word(near) < t).all(), (alpha, beta, dt)
            assert (word(far) >= t).all(), (alpha, beta, dt)
