"""The argument checks of the eight guided-filter entry points against one list of cases, without a GPU: every check
below returns before the first HIP call.  A case is asked of every entry point it applies to and has one expected status
there, which pins the precedence the entry points share: bad arguments, then zero elements (or no gradient asked for),
then the shared size and channel bounds, then flags, then the full covariance's channel bound, then "more than half" (the
bilinear backwards), then aliasing.  Every message starts with the entry point's own name and a colon.  (The tests of each
entry point's own arguments stay in test_guided*_cpu.py and test_gpu_guided_args.py.)"""
import ctypes

import pytest

OK, INVALID, TOO_LARGE, UNSUPPORTED = 0, 1, 6, 7
FULL_COV = 1        # PHL_GUIDED_BILINEAR_FULL_COV

# entry -> (function, backward, takes the four index maps, takes a flags word, the full covariance); the bilinear forward
# is one function for both models and is asked in both forms
BILINEAR_FULL = "phl_guided_filter_bilinear+FULL_COV"
ENTRIES = {
    "phl_guided_filter": ("phl_guided_filter", False, True, False, False),
    "phl_guided_filter_full": ("phl_guided_filter_full", False, True, False, True),
    "phl_guided_filter_bilinear": ("phl_guided_filter_bilinear", False, False, True, False),
    BILINEAR_FULL: ("phl_guided_filter_bilinear", False, False, True, True),
    "phl_guided_filter_grad": ("phl_guided_filter_grad", True, True, False, False),
    "phl_guided_filter_full_grad": ("phl_guided_filter_full_grad", True, True, False, True),
    "phl_guided_filter_bilinear_grad": ("phl_guided_filter_bilinear_grad", True, False, True, False),
    "phl_guided_filter_bilinear_full_grad": ("phl_guided_filter_bilinear_full_grad", True, False, False, True),
}
MAPS = ("row_of_low", "col_of_low", "low_of_row", "low_of_col")
# fake device addresses, never dereferenced; p3 / p4 / p5 / p6 are src, out or g, grad_y, grad_x, grad_eps
DEFAULTS = dict(y=0x1000, x=0x2000, p3=0x3000, p4=0x4000, p5=0x5000, p6=0x6000, B=1, cy=4, cx=3, H=48, W=64, h=24, w=32, r=4,
                row_of_low=0x7000, col_of_low=0x8000, low_of_row=0x9000, low_of_col=0xa000, eps=0xb000, scale=1.0, sub=1, flags=0)


def _call(lib, entry, **over):
    name, backward, maps, flags, full = ENTRIES[entry]
    a = dict(DEFAULTS, **over)
    if entry == BILINEAR_FULL:
        a["flags"] |= FULL_COV
    args = [a["y"], a["x"], a["p3"], a["p4"]] + ([a["p5"], a["p6"]] if backward else [])
    args += [a[k] for k in ("B", "cy", "cx", "H", "W", "h", "w", "r")] + ([a[k] for k in MAPS] if maps else [])
    args += [a["eps"], ctypes.c_float(a["scale"])] + ([a["sub"]] if backward else []) + ([ctypes.c_uint(a["flags"])] if flags else [])
    return getattr(lib, name)(*args, None)


def everyone(e):
    return True


def backward(e):
    return ENTRIES[e][1]


def forward(e):
    return not ENTRIES[e][1]


def with_maps(e):
    return ENTRIES[e][2]


def with_flags(e):
    return ENTRIES[e][3]


def full(e):
    return ENTRIES[e][4]


def bilinear_backward(e):
    return backward(e) and not with_maps(e)


def both(f, g):
    return lambda e: f(e) and g(e)


NOTHING_ASKED = dict(p4=None, p5=None, p6=None)
# (id, the entry points it is asked of, the arguments that differ from DEFAULTS, status, a substring of the message)
CASES = [
    ("null_y", everyone, dict(y=None), INVALID, None),
    ("null_x", everyone, dict(x=None), INVALID, None),
    ("null_out", forward, dict(p4=None), INVALID, None),
    ("null_g", backward, dict(p3=None), INVALID, None),
    ("null_eps", everyone, dict(eps=None), INVALID, None),
    ("null_src_is_allowed_but_y_is_not", forward, dict(p3=None, y=None), INVALID, None),
    *[("null_" + m, with_maps, {m: None}, INVALID, None) for m in MAPS],
    ("h_above_H", everyone, dict(h=49), INVALID, None),
    ("w_above_W", everyone, dict(w=65), INVALID, None),
    ("h_zero", everyone, dict(h=0), INVALID, None),
    ("w_zero", everyone, dict(w=0), INVALID, None),
    ("scale_nan", everyone, dict(scale=float("nan")), INVALID, None),
    ("scale_inf", everyone, dict(scale=float("inf")), INVALID, None),
    ("cx_zero", everyone, dict(cx=0), INVALID, None),
    ("r_negative", everyone, dict(r=-1), INVALID, None),
    ("too_large", everyone, dict(H=1 << 16, W=1 << 16, h=8, w=8), TOO_LARGE, None),
    ("cx_17", everyone, dict(cx=17), UNSUPPORTED, "guide channels"),
    ("cx_5_full", full, dict(cx=5), UNSUPPORTED, "at most 4"),
    ("unknown_flags", both(with_flags, forward), dict(flags=2), UNSUPPORTED, "flags"),
    ("flags_of_the_diagonal_backward", both(with_flags, backward), dict(flags=FULL_COV), UNSUPPORTED, "flags"),
    ("h_more_than_half", bilinear_backward, dict(h=25), UNSUPPORTED, "more than half"),
    ("w_more_than_half", bilinear_backward, dict(w=33), UNSUPPORTED, "more than half"),
    ("out_is_y", forward, dict(p4=DEFAULTS["y"]), INVALID, None),
    ("out_is_x", forward, dict(p4=DEFAULTS["x"]), INVALID, None),
    ("out_is_src", forward, dict(p4=DEFAULTS["p3"]), INVALID, None),
    ("grad_y_is_y", backward, dict(p4=DEFAULTS["y"]), INVALID, None),
    ("grad_x_is_g", backward, dict(p5=DEFAULTS["p3"]), INVALID, None),
    ("grad_eps_is_eps", backward, dict(p6=DEFAULTS["eps"]), INVALID, None),
    ("grad_x_is_grad_y", backward, dict(p5=DEFAULTS["p4"]), INVALID, None),
    ("no_images", everyone, dict(B=0, y=None, x=None, p3=None, p4=None), OK, None),
    ("no_labels", everyone, dict(cy=0, y=None, p3=None, p4=None), OK, None),
    ("no_pixels", everyone, dict(H=0, h=0, y=None, x=None, p3=None, p4=None), OK, None),
    ("nothing_asked", backward, NOTHING_ASKED, OK, None),
    # two faults at once: the earlier check answers
    ("bad_arguments_before_zero_elements", everyone, dict(cy=0, h=49), INVALID, None),
    ("cx_zero_before_zero_elements", everyone, dict(B=0, cx=0), INVALID, None),
    ("zero_elements_before_null", everyone, dict(B=0, eps=None), OK, None),
    ("zero_elements_before_cx_17", everyone, dict(B=0, cx=17), OK, None),
    ("zero_elements_before_cx_5", full, dict(B=0, cx=5), OK, None),
    ("zero_elements_before_flags", with_flags, dict(B=0, flags=6), OK, None),
    ("zero_elements_before_aliasing", everyone, dict(cy=0, p4=DEFAULTS["y"]), OK, None),
    ("cx_17_before_nothing_asked", backward, dict(NOTHING_ASKED, cx=17), UNSUPPORTED, "guide channels"),
    ("nothing_asked_before_cx_5", both(backward, full), dict(NOTHING_ASKED, cx=5), OK, None),
    ("nothing_asked_before_flags", both(backward, with_flags), dict(NOTHING_ASKED, flags=FULL_COV), OK, None),
    ("nothing_asked_before_more_than_half", bilinear_backward, dict(NOTHING_ASKED, h=25), OK, None),
    ("nothing_asked_after_null", backward, dict(NOTHING_ASKED, p3=None), INVALID, None),
    ("null_before_cx_17", everyone, dict(y=None, cx=17), INVALID, None),
    ("null_before_cx_5", full, dict(x=None, cx=5), INVALID, None),
    ("too_large_before_cx_17", everyone, dict(H=1 << 16, W=1 << 16, h=8, w=8, cx=17), TOO_LARGE, None),
    ("cx_17_before_flags", with_flags, dict(cx=17, flags=2), UNSUPPORTED, "guide channels"),
    ("flags_before_cx_5", both(with_flags, full), dict(cx=5, flags=2), UNSUPPORTED, "flags"),
    ("flags_before_more_than_half", both(with_flags, backward), dict(flags=FULL_COV, h=25), UNSUPPORTED, "flags"),
    ("cx_5_before_more_than_half", both(bilinear_backward, full), dict(cx=5, h=25), UNSUPPORTED, "guide channels"),
    ("cx_5_before_aliasing", full, dict(cx=5, p4=DEFAULTS["y"]), UNSUPPORTED, "guide channels"),
    ("flags_before_aliasing", with_flags, dict(flags=4, p4=DEFAULTS["y"]), UNSUPPORTED, "flags"),
    ("more_than_half_before_aliasing", bilinear_backward, dict(h=25, p4=DEFAULTS["y"]), UNSUPPORTED, "more than half"),
]
MATRIX = [(e, c) for c in CASES for e in ENTRIES if c[1](e)]


def test_the_matrix_asks_every_entry_point():
    import phl

    assert {v[0] for v in ENTRIES.values()} == {r[0] for r in phl._ABI if r[0].startswith("phl_guided_filter") and len(r[2]) > 7}
    for e in ENTRIES:
        assert sum(1 for n, _ in MATRIX if n == e) >= 30, e


@pytest.mark.parametrize("entry,case", MATRIX, ids=[f"{e}-{c[0]}" for e, c in MATRIX])
def test_entry_matrix(entry, case):
    import phl

    lib = phl.load_library()
    _, _, over, status, part = case
    assert _call(lib, entry, **over) == status
    if status != OK:
        msg = lib.phl_last_error().decode()
        assert msg.startswith(ENTRIES[entry][0] + ":"), msg
        assert part is None or part in msg, msg
