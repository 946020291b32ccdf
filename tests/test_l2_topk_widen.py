"""The threshold search of K20 (l2t_widen in csrc/l2_topk.hip, on l2f_thresholds of csrc/l2_filter_tile.h) in a
Python port, IEEE double like the device code: no GPU needed.

DESIGN s4 "K20" step 3 quotes two facts from this port: the first guess of the slack is accepted over the whole
range of witness bounds under the four (alpha, beta) of the GPU tests, and the threshold it yields lies within
14 rho + 600u (relative; 3.3e-12 at d = 1024) of the witnesses' bound.  Exactness does not rest on either -- the
device CHECKS the deciding inequality and leaves the query unresolved when it fails -- but a slack that stopped
being accepted would send queries to the fp64 route for nothing.  The port is kept line for line with the device functions."""
import math

import numpy as np
import pytest

U = 2.0 ** -53
INF = math.inf


def thresholds(t, alpha, beta, rho):
    """l2f_thresholds for a finite t: (tb, tn)"""
    pos = alpha > 0.0
    x = (t - beta) / alpha
    sig = 16.0 * U * ((abs(t) + abs(beta)) / abs(alpha)) + 1e-290
    xlo, xhi = x - sig, x + sig
    lo, hi = xlo * (1.0 - rho), xhi * (1.0 + 2.0 * rho)
    lo_t = (lo * lo) * (1.0 - 4.0 * U) if xlo > 0.0 else -INF
    hi_t = (hi * hi) * (1.0 + 4.0 * U) if xhi > 0.0 else 0.0
    return (lo_t, hi_t) if pos else (hi_t, lo_t)


def widen(tau, alpha, beta, rho):
    """l2t_widen: (iterations used, t, threshold) or None when there is no threshold"""
    pos = alpha > 0.0
    if not abs(tau) < INF:
        return None
    dt = max(tau, 0.0) if pos else -tau
    if not pos and not dt > 0.0:
        return None
    y = math.sqrt(dt)
    slack = 4.0 * rho * y + 64.0 * U * (y + 2.0 * abs(beta) / abs(alpha)) + 1e-280
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
    for alpha, beta in _cases(d):
        for dt in 10.0 ** np.arange(-30.0, 31.0):
            tau = dt if alpha > 0 else -dt
            got = widen(float(tau), alpha, beta, rho)
            assert got is not None and got[0] == 0, (alpha, beta, dt, got)
            tn = got[2]
            # the threshold is on the far side of the witnesses' bound ...
            assert tn > dt if alpha > 0 else tn < dt
            # ... and close to it.  From the formulas: the slack moves y by 4 rho + 64u (1 + 2 |beta| / (|alpha| y)),
            # l2f_thresholds by 2 rho + its sigma <= 16u (2 + |beta| / (|alpha| y)), squaring doubles the sum: where
            # beta does not swamp the distance term, |tn - dt| <= (12 rho + 600u) dt (plus rho^2 terms: 14 rho)
            if abs(alpha) * math.sqrt(dt) >= abs(beta):
                assert abs(tn - dt) <= (14.0 * rho + 600.0 * U) * dt, (alpha, beta, dt, tn)


def test_no_threshold_where_there_is_none():
    rho = 2.0 * (1024 + 16.0) * U
    assert widen(INF, 1.0, 0.0, rho) is None and widen(float("nan"), 1.0, 0.0, rho) is None
    # alpha < 0 and witnesses whose distances have no positive lower bound
    assert widen(0.0, -1.0 / 1024, -1.0, rho) is None and widen(5.0, -1.0 / 1024, -1.0, rho) is None
    # a bound of exactly zero under alpha > 0: every guess underflows, the query stays unresolved
    assert widen(0.0, 1.0, 0.0, rho) is None


@pytest.mark.parametrize("d", [67, 1024])
def test_threshold_separates_the_words(d):
    """What launch B relies on, on words formed as the canonical chain forms them from an exactly known S:
    a witness (D on the near side of the bound) has a word < t, a column beyond the threshold a word >= t."""
    rho = 2.0 * (d + 16.0) * U
    rng = np.random.default_rng(d)
    for alpha, beta in _cases(d):
        for dt in (1e-3, 1.0, 0.25 * d, 2.0 * d, 1e6):
            tau = dt if alpha > 0 else -dt
            _, t, tn = widen(float(tau), alpha, beta, rho)
            # S = D (1 + eta), |eta| <= (d + 4) 2u: the chain's own rounding of the sum (DESIGN s4, K19 step 3)
            eta = (d + 4.0) * 2.0 * U * rng.uniform(-1.0, 1.0, 2000)
            near = dt * (1.0 - rng.uniform(0.0, 1e-9, 2000)) if alpha > 0 else dt * (1.0 + rng.uniform(0.0, 1e-9, 2000))
            far = tn * (1.0 + rng.uniform(1e-16, 1e-9, 2000)) if alpha > 0 else tn * (1.0 - rng.uniform(1e-16, 1e-9, 2000))
            near[0], far[0] = dt, np.nextafter(tn, INF if alpha > 0 else -INF)
            word = lambda D: alpha * np.sqrt(D * (1.0 + eta)) + beta
            assert (word(near) < t).all(), (alpha, beta, dt)
            assert (word(far) >= t).all(), (alpha, beta, dt)
