"""What the exact cost-volume tests share (test_costvol_cpu.py states the precondition, test_gpu_costvol.py uses it).

With small integer pixels every raw cost, every window sum and every intermediate of the kernel's running sums is an
integer below 2^24, which fp32 holds exactly in any summation order: csrc/phl_costvol.hip must then equal the float64
oracle bit for bit, whatever order it adds in, and any indexing error (reflect, tile seam, disparity offset, zero padding,
channel padding) shows as a difference."""
import numpy as np

CRITS = ("AD", "SD", "nprod")                       # the order of phl.CRITERIA: the kernel's CRIT template argument
WINDOWS = tuple(range(1, 18, 2))                    # R = 0..8: every instance the host dispatch builds
PIXEL_RANGE = {"AD": 255, "SD": 31, "nprod": 63}    # integer pixels are drawn from [-r, r]
CRIT_MAX = {"AD": 2 * 255, "SD": (2 * 31) ** 2, "nprod": 63 * 63}      # largest |criterion| of one channel on that range
SHAPE, MAX_DISP = (19, 37), 41                      # ragged in y, x and disparity; disparities beyond the image width
EDGE_INSTANCES = ((9, "AD", 3), (17, "SD", 4), (3, "nprod", 1))     # (window, criterion, channels) of the tile/reflect sweep
EDGE_SIZES = (1, 2, 15, 16, 17, 33)                 # h and w around the 16-pixel tile; 1 and 2 fold a window of 17 many times


def channels_of(ws, crit):
    """1..4, chosen so that each criterion meets every channel count over the nine windows."""
    return 1 + (ws // 2 + CRITS.index(crit)) % 4


def running_sum_bound(ws, c, crit):
    """Bound on every intermediate: a running sum adds the entering element before it subtracts the leaving one, so the
    horizontal sum holds at most ws + 1 raw costs and the vertical one ws + 1 rows of ws: no more than ws^2 + ws + 1
    raw costs at once, each at most c * max|crit|."""
    return (ws * ws + ws + 1) * c * CRIT_MAX[crit]


def int_images(h, w, c, crit, seed):
    """Two float64 [h, w, c] images of signed integers, uniform on the criterion's range."""
    rng = np.random.default_rng(seed)
    r = PIXEL_RANGE[crit]
    return (rng.integers(-r, r + 1, size=(h, w, c)).astype(np.float64),
            rng.integers(-r, r + 1, size=(h, w, c)).astype(np.float64))


def first_difference(got, want):
    """None if equal, else a message naming the first differing (y, x, k) of two [h, w, L] arrays."""
    bad = np.argwhere(got != want)
    if not len(bad):
        return None
    y, x, k = (int(v) for v in bad[0])
    return f"{len(bad)} of {want.size} differ, first at (y, x, k) = ({y}, {x}, {k}): got {got[y, x, k]!r}, want {want[y, x, k]!r}"



def scipy_reflect_defined(h, w, ws):
    """False where scipy.ndimage's 'reflect' border -- the oracle's and the reference's aggregate -- is not a function of
    its input: at an axis of length 2 under a window of 17 (radius 8 = four image lengths) it returns other memory
    (NaN, 1e277, different from call to call; scipy 1.15, no other (length, odd window <= 17) pair).  There the kernel is
    held to the rule itself, ``box_reflect``."""
    return not (ws == 17 and 2 in (h, w))


def box_reflect(cost, ws):
    """ws x ws window sums of cost [h, w, L] under the border rule scipy documents for 'reflect' (d c b a | a b c d | d c b a,
    period 2n): numpy's 'symmetric' padding, summed explicitly in float64."""
    r = ws // 2
    h, w = cost.shape[:2]
    p = np.pad(cost, ((r, r), (r, r), (0, 0)), mode="symmetric")
    out = np.zeros_like(cost)
    for dy in range(ws):
        for dx in range(ws):
            out += p[dy:dy + h, dx:dx + w]
    return out


def reference_volume(a, b, ws, crit, L):
    """The float64 oracle; where scipy's border is undefined, the oracle's raw costs (its window-1 volume) aggregated by
    ``box_reflect``.  test_costvol_cpu.py holds the two forms equal everywhere else."""
    from oracle import costvol_oracle as co

    if scipy_reflect_defined(a.shape[0], a.shape[1], ws):
        return co.disparity_badness(a, b, ws, crit, max_disp=L)
    return box_reflect(co.disparity_badness(a, b, 1, crit, max_disp=L), ws)
