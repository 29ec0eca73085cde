"""nano_check<WF = true> takes t = min(x, y) where the reference's cases select x (k starts first) or y, with
x = k_chi - l_clo and y = l_chi - k_clo (msgpu_kernels.hip).  t is read only where the vertex has an orientation: pos
(k_clo < l_clo and k_chi < l_chi) or neg (both reversed).  There the minimum must be the selected difference bit for bit:
over seeded random and hand-made well-formed range pairs (lo <= hi, no NaN) -- equal endpoints, nested ranges, one-ulp
neighbours, magnitudes from 1e-300 to 1e300, infinite ends.  No GPU: the arithmetic is IEEE fp64 on both sides."""
import itertools

import numpy as np


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def _check(k_lo, k_hi, l_lo, l_hi):
    """arrays of well-formed pairs -> (lanes with an orientation, lanes in all)"""
    k_lo, k_hi, l_lo, l_hi = (np.asarray(v, dtype=np.float64) for v in (k_lo, k_hi, l_lo, l_hi))
    assert (k_lo <= k_hi).all() and (l_lo <= l_hi).all(), "well formed"
    with np.errstate(invalid="ignore", over="ignore"):
        x = k_hi - l_lo
        y = l_hi - k_lo
    pos = (k_lo < l_lo) & (k_hi < l_hi)
    neg = (k_lo > l_lo) & (k_hi > l_hi)
    sel = np.where(k_lo < l_lo, x, y)
    use = pos | neg
    assert not np.isnan(x[use]).any() and not np.isnan(y[use]).any(), "no NaN under an orientation"
    # v_min_f64 and fmin agree with np.fmin where neither operand is a NaN, except on +0 against -0 -- shown not to occur:
    zero_pair = (x == 0) & (y == 0) & (np.signbit(x) != np.signbit(y))
    assert not (zero_pair & use).any()
    m = np.fmin(x, y)
    bad = use & (_bits(m) != _bits(sel))
    assert not bad.any(), (k_lo[bad][:4], k_hi[bad][:4], l_lo[bad][:4], l_hi[bad][:4])
    # and the orientation fixes which one: x under pos, y under neg
    assert (_bits(m)[pos] == _bits(x)[pos]).all() and (_bits(m)[neg] == _bits(y)[neg]).all()
    return int(use.sum()), len(use)


def _ranges(rng, n, scale):
    a = rng.uniform(-1, 1, n) * scale
    w = rng.uniform(0, 1, n) * scale * rng.choice([0.0, 1e-12, 1e-3, 1.0], n)
    lo = a
    with np.errstate(over="ignore"):
        hi = a + np.abs(w)
    hi = np.where(np.isfinite(hi), hi, lo)
    return lo, np.maximum(lo, hi)


def test_random_pairs():
    rng = np.random.default_rng(20)
    seen = 0
    for scale in (1e-300, 1e-150, 1e-9, 1.0, 600.0, 3e4, 2.0 ** 31, 1e15, 1e150, 1e300):
        k_lo, k_hi = _ranges(rng, 20000, scale)
        l_lo, l_hi = _ranges(rng, 20000, scale)
        used, _ = _check(k_lo, k_hi, l_lo, l_hi)
        seen += used
        # nanopore coordinates with a correction: integers plus a quotient, close together
        base = np.floor(rng.uniform(0, 50, 20000)) * scale
        k = (base, base + np.floor(rng.uniform(0, 5, 20000)) * scale)
        l_base = base + np.floor(rng.uniform(-3, 4, 20000)) * scale
        l = (l_base, l_base + np.floor(rng.uniform(0, 5, 20000)) * scale)
        seen += _check(k[0], k[1], l[0], l[1])[0]
    assert seen > 100000


def test_hand_made_pairs():
    inf = np.inf
    vals = [-inf, -1e300, -1e9, -600.0, np.nextafter(-600.0, 0.0), -1e-300, -5e-324, -0.0, 0.0, 5e-324, 1e-300, 1.0,
            np.nextafter(1.0, 2.0), 599.0, 600.0, np.nextafter(600.0, inf), 1e9, np.nextafter(1e9, inf), 1e300, inf]
    quads = [q for q in itertools.product(vals, repeat=4) if q[0] <= q[1] and q[2] <= q[3]]
    k_lo, k_hi, l_lo, l_hi = (np.array(c) for c in zip(*quads))
    used, total = _check(k_lo, k_hi, l_lo, l_hi)
    assert used > 1000 and total - used > 1000  # equal endpoints, nested ranges and equal starts have no orientation
    # what the argument leaves out on purpose: without an orientation the two may differ (nested: x and y are unrelated)
    nested = (k_lo < l_lo) & (l_hi < k_hi)
    with np.errstate(invalid="ignore", over="ignore"):
        x, y = k_hi - l_lo, l_hi - k_lo
    assert (np.fmin(x, y)[nested] != np.where(k_lo < l_lo, x, y)[nested]).any()


def test_one_ulp_neighbours():
    rng = np.random.default_rng(21)
    a = rng.uniform(0, 1e6, 5000)
    up = np.nextafter(a, np.inf)
    w = rng.uniform(0, 1e3, 5000)
    # k and l one ulp apart at both ends, in both orders; and one end equal (no orientation)
    for k_lo, k_hi, l_lo, l_hi in ((a, a + w, up, np.nextafter(a + w, np.inf)), (up, np.nextafter(a + w, np.inf), a, a + w),
                                   (a, a + w, up, a + w), (a, a + w, a, np.nextafter(a + w, np.inf))):
        _check(k_lo, np.maximum(k_lo, k_hi), l_lo, np.maximum(l_lo, l_hi))
