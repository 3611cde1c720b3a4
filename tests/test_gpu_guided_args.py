"""phl_guided_filter and phl_guided_filter_grad check the arguments they share in one place: for a bad set both return
the same status, one of PHL_ERR_INVALID / PHL_ERR_TOO_LARGE / PHL_ERR_UNSUPPORTED, and each names itself in the message.
Every case is rejected before the first launch: the pointers are fake addresses that nothing dereferences."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu
INVALID, TOO_LARGE, UNSUPPORTED = 1, 6, 7
Y, X, T, O1, O2, O3, M1, M2, M3, M4, E = (0x1000 * k for k in range(1, 12))


def _shared(B=1, cy=4, cx=3, H=48, W=64, h=24, w=32, r=4, m1=M1, m2=M2, m3=M3, m4=M4, eps=E, scale=1.0):
    return [B, cy, cx, H, W, h, w, r, m1, m2, m3, m4, eps, ctypes.c_float(scale)]


BAD = {
    "negative_size": _shared(W=-64),
    "h_above_H": _shared(h=49),
    "cx_0": _shared(cx=0),
    "cx_17": _shared(cx=17),
    "HW_above_int32": _shared(H=1 << 16, W=1 << 16, h=8, w=8),
    "null_index_map": _shared(m3=None),
    "scale_not_finite": _shared(scale=float("nan")),
}


@pytest.mark.parametrize("case", list(BAD))
def test_both_entry_points_reject_alike(case):
    import phl

    lib = phl.load_library()
    got = {}
    for name, args in (("phl_guided_filter", [Y, X, T, O1] + BAD[case] + [None]),
                       ("phl_guided_filter_grad", [Y, X, T, O1, O2, O3] + BAD[case] + [1, None])):
        got[name] = getattr(lib, name)(*args)
        msg = lib.phl_last_error().decode()
        assert msg.startswith(name + ":"), (name, msg)
    assert got["phl_guided_filter"] == got["phl_guided_filter_grad"], got
    assert got["phl_guided_filter"] in (INVALID, TOO_LARGE, UNSUPPORTED), got
