"""Argument checks of phl_nchw_softmax_compat_wide (include/phl.h): the product step for up to 512 labels.  Sizes, null
pointers, aliasing, the label range and the size limits, with the status each returns.  Every case returns before the
first HIP call, so no GPU is needed; the pointers are never dereferenced."""
import ctypes

import pytest

OK, INVALID, TOO_LARGE, UNSUPPORTED = 0, 1, 6, 7
PRODUCT = 0
E, G, M, O, MIS = 0x1000, 0x2000, 0x3000, 0x4000, 0x5004      # fake device addresses; MIS is off the 16-byte grid

# (E0, G, mu, out, B, L, n) -> status
CASES = [
    # the label range
    ((E, G, M, O, 2, 513, 64), UNSUPPORTED),
    ((E, G, M, O, 1, 1 << 20, 63), UNSUPPORTED),
    ((E, None, M, O, 1, 513, 1), UNSUPPORTED),
    # negative sizes, L < 1
    ((E, G, M, O, 2, 0, 64), INVALID),
    ((E, G, M, O, 2, -3, 64), INVALID),
    ((E, G, M, O, -1, 341, 64), INVALID),
    ((E, G, M, O, 2, 341, -1), INVALID),
    ((E, G, M, O, 2, 0, 0), INVALID),                    # L is checked before the element count
    # null pointers with elements present (G alone may be null)
    ((None, G, M, O, 2, 341, 64), INVALID),
    ((E, G, M, None, 2, 341, 64), INVALID),
    ((E, G, None, O, 2, 341, 64), INVALID),
    ((E, None, None, O, 1, 8, 63), INVALID),
    # out aliasing an input
    ((E, G, M, E, 2, 341, 64), INVALID),
    ((E, G, M, G, 2, 341, 64), INVALID),
    ((E, None, M, E, 2, 64, 64), INVALID),
    # zero elements: PHL_OK whatever the pointers
    ((E, G, M, O, 0, 257, 64), OK),
    ((E, G, M, O, 2, 257, 0), OK),
    ((E, G, M, O, 0, 512, 64), OK),
    ((E, G, M, O, 2, 512, 0), OK),
    ((None, None, None, None, 0, 512, 64), OK),
    ((MIS, MIS, MIS, MIS, 3, 341, 0), OK),
    ((E, G, M, E, 0, 5000, 64), OK),                     # the label range is looked at after the element count
    # too many elements: the byte count leaves int64, or the tiles (32 pixels above 256 labels, 64 up to there) leave the grid
    ((E, G, M, O, 1 << 20, 341, 1 << 40), TOO_LARGE),
    ((E, G, M, O, 1 << 20, 512, 1 << 40), TOO_LARGE),
    ((E, G, M, O, 1 << 20, 64, 1 << 40), TOO_LARGE),
    ((E, G, M, O, 1 << 16, 300, 1 << 21), TOO_LARGE),    # 2^16 tiles per image, 2^32 workgroups
    ((E, G, M, O, 1 << 16, 8, 1 << 22), TOO_LARGE),
    ((E, G, M, O, 1 << 20, 1 << 20, 1 << 40), TOO_LARGE),
]


@pytest.mark.parametrize("args,status", CASES, ids=[f"{i}-L{c[0][5]}" for i, c in enumerate(CASES)])
def test_nchw_softmax_compat_wide_argument_checks(args, status):
    import phl

    lib = phl.load_library()
    assert lib.phl_nchw_softmax_compat_wide(*args, None) == status
    if status != OK:
        assert lib.phl_last_error().decode().startswith("phl_nchw_softmax_compat_wide:"), lib.phl_last_error()
    if status == UNSUPPORTED:
        assert "512" in lib.phl_last_error().decode(), lib.phl_last_error()


def test_the_old_entry_keeps_its_range():
    """phl_nchw_softmax_compat is not widened: PRODUCT above 256 labels is still PHL_ERR_UNSUPPORTED there."""
    import phl

    lib = phl.load_library()
    for L in (257, 341, 512):
        assert lib.phl_nchw_softmax_compat(E, G, M, ctypes.c_float(0.0), ctypes.c_float(0.0), O, 2, L, 64, PRODUCT, None) == UNSUPPORTED
        assert lib.phl_last_error().decode().startswith("phl_nchw_softmax_compat:"), lib.phl_last_error()
    assert lib.phl_nchw_softmax_compat(E, G, M, ctypes.c_float(0.0), ctypes.c_float(0.0), O, 0, 257, 64, PRODUCT, None) == OK


def test_binding_constants_and_checks_need_no_gpu():
    import phl
    import torch

    assert phl.NCHW_WIDE_MAX_L == 512 and phl.NCHW_PRODUCT_MAX_L == 256
    with pytest.raises(TypeError):
        phl.nchw_softmax_compat_wide(torch.zeros(1, 300, 3, 3), None, torch.zeros(300, 300))      # CPU tensors
