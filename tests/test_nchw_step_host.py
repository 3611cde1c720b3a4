"""Argument checks of phl_nchw_softmax_compat (include/phl.h): sizes, modes, null pointers, aliasing, the label range of
each mode and the size limits, with the status each returns.  Every case returns before the first HIP call, so no GPU is
needed; the pointers are never dereferenced."""
import ctypes

import pytest

OK, INVALID, TOO_LARGE, UNSUPPORTED = 0, 1, 6, 7
PRODUCT, UNIFORM, SOFTMAX, LOGITS = 0, 1, 2, 3
E, G, M, O, MIS = 0x1000, 0x2000, 0x3000, 0x4000, 0x5004      # fake device addresses; MIS is off the 16-byte grid
INF, NAN = float("inf"), float("nan")

# (E0, G, mu, alpha, beta, out, B, L, n, mode) -> status
CASES = [
    # negative sizes, L < 1, unknown modes
    ((E, G, M, 0.0, 0.0, O, -1, 8, 64, PRODUCT), INVALID),
    ((E, G, M, 0.0, 0.0, O, 2, 8, -64, PRODUCT), INVALID),
    ((E, G, M, 0.0, 0.0, O, 2, 0, 64, SOFTMAX), INVALID),
    ((E, G, M, 0.0, 0.0, O, 2, -3, 64, LOGITS), INVALID),
    ((E, G, M, 0.0, 0.0, O, 2, 8, 64, 4), INVALID),
    ((E, G, M, 0.0, 0.0, O, 2, 8, 64, -1), INVALID),
    ((E, G, M, 0.0, 0.0, O, 2, 0, 0, SOFTMAX), INVALID),              # L is checked before the element count
    # null pointers with elements present
    ((None, G, M, 0.0, 0.0, O, 2, 8, 64, PRODUCT), INVALID),
    ((E, G, M, 0.0, 0.0, None, 2, 8, 64, PRODUCT), INVALID),
    ((E, G, None, 0.0, 0.0, O, 2, 8, 64, PRODUCT), INVALID),
    ((E, None, M, 0.0, 0.0, O, 2, 8, 64, LOGITS), INVALID),
    ((None, None, None, 1.0, -1.0, O, 1, 8, 63, UNIFORM), INVALID),
    ((E, None, None, 0.0, 0.0, None, 1, 8, 63, SOFTMAX), INVALID),
    # out aliasing an input
    ((E, G, M, 0.0, 0.0, E, 2, 8, 64, PRODUCT), INVALID),
    ((E, G, M, 0.0, 0.0, G, 2, 8, 64, PRODUCT), INVALID),
    ((E, G, None, 0.0, 0.0, G, 2, 8, 64, LOGITS), INVALID),
    ((E, None, None, 0.0, 0.0, E, 2, 8, 64, SOFTMAX), INVALID),
    # alpha / beta must be finite where they are read
    ((E, G, None, INF, -1.0, O, 2, 8, 64, UNIFORM), INVALID),
    ((E, G, None, 1.0, NAN, O, 2, 8, 64, UNIFORM), INVALID),
    ((E, G, None, 1.0, -INF, O, 2, 8, 0, UNIFORM), INVALID),          # also with nothing to do
    ((None, None, None, NAN, INF, None, 2, 8, 0, SOFTMAX), OK),       # not read in the other modes
    # the label range of each mode
    ((E, G, M, 0.0, 0.0, O, 2, 257, 64, PRODUCT), UNSUPPORTED),
    ((E, G, M, 0.0, 0.0, O, 1, 1 << 20, 63, PRODUCT), UNSUPPORTED),
    ((E, G, None, 1.0, -1.0, O, 2, 1025, 64, UNIFORM), UNSUPPORTED),
    # too many elements: the byte count leaves int64, or the tiles leave the grid
    ((E, G, M, 0.0, 0.0, O, 1 << 20, 1 << 20, 1 << 40, SOFTMAX), TOO_LARGE),
    ((E, G, M, 0.0, 0.0, O, 1 << 20, 256, 1 << 40, PRODUCT), TOO_LARGE),
    ((E, G, M, 0.0, 0.0, O, (1 << 31) - 1, (1 << 31) - 1, 2, LOGITS), TOO_LARGE),
    ((E, G, M, 0.0, 0.0, O, 1, 1, 1 << 40, SOFTMAX), TOO_LARGE),
    ((E, G, M, 0.0, 0.0, O, 1 << 16, 8, 1 << 22, PRODUCT), TOO_LARGE),
    ((E, G, None, 1.0, -1.0, O, 1, 300, 1 << 40, UNIFORM), TOO_LARGE),
    # zero elements: PHL_OK whatever the pointers and the label count
    ((MIS, MIS, MIS, 0.0, 0.0, MIS, 2, 8, 0, PRODUCT), OK),
    ((None, None, None, 0.0, 0.0, None, 0, 8, 64, PRODUCT), OK),
    ((MIS, None, None, 0.0, 0.0, MIS, 3, 5000, 0, LOGITS), OK),
    ((E, G, M, 0.0, 0.0, E, 0, 257, 64, PRODUCT), OK),
    ((None, None, None, 1.0, -1.0, None, 2, 1025, 0, UNIFORM), OK),
]


@pytest.mark.parametrize("args,status", CASES, ids=[f"{i}-mode{c[0][9]}" for i, c in enumerate(CASES)])
def test_nchw_softmax_compat_argument_checks(args, status):
    import phl

    lib = phl.load_library()
    e0, g, mu, alpha, beta, out, *rest = args
    assert lib.phl_nchw_softmax_compat(e0, g, mu, ctypes.c_float(alpha), ctypes.c_float(beta), out, *rest, None) == status
    if status != OK:
        assert lib.phl_last_error().decode().startswith("phl_nchw_softmax_compat"), lib.phl_last_error()


def test_binding_checks_need_no_gpu():
    """What phl.nchw_softmax_compat refuses before it reaches the library."""
    import phl
    import torch

    with pytest.raises(TypeError):
        phl.nchw_softmax_compat(torch.zeros(1, 4, 3, 3))                    # a CPU tensor
    assert (phl.NCHW_PRODUCT, phl.NCHW_UNIFORM, phl.NCHW_SOFTMAX, phl.NCHW_LOGITS) == (PRODUCT, UNIFORM, SOFTMAX, LOGITS)
