"""Argument checks of the compat entry points of the C ABI (include/phl.h): null pointers, negative n, L out of range,
row strides that are not a multiple of 4 and misaligned base addresses, with the status each returns.  Every case returns
before the first HIP call, so no GPU is needed; the pointers are never dereferenced."""
import pytest

OK, INVALID, UNSUPPORTED = 0, 1, 7
A, B, C, D, MIS = 0x1000, 0x2000, 0x3000, 0x4000, 0x5004      # fake device addresses; MIS is off the 16-byte grid

# (entry point, arguments before the stream, status, text the error message starts with)
CASES = [
    # phl_softmax_neg_add(E0, e_rs, G, g_rs, out, o_rs, n, L)
    ("phl_softmax_neg_add", (None, 8, None, 0, B, 8, 5, 8), INVALID, "phl_softmax_neg_add"),
    ("phl_softmax_neg_add", (A, 8, None, 0, None, 8, 5, 8), INVALID, "phl_softmax_neg_add"),
    ("phl_softmax_neg_add", (A, 8, None, 0, B, 8, -1, 8), INVALID, "phl_softmax_neg_add"),
    ("phl_softmax_neg_add", (A, 8, None, 0, B, 8, 5, 0), INVALID, "phl_softmax_neg_add"),
    ("phl_softmax_neg_add", (None, 3, None, 0, None, 3, 0, 7), OK, None),
    # phl_uniform_compat_softmax(E0, e_rs, X, x_rs, alpha, beta, out, o_rs, n, L, flags)
    ("phl_uniform_compat_softmax", (A, 8, None, 8, 1.0, -1.0, C, 8, 5, 8, 0), INVALID, "phl_uniform_compat_softmax"),
    ("phl_uniform_compat_softmax", (A, 8, B, 8, 1.0, -1.0, C, 8, -1, 8, 0), INVALID, "phl_uniform_compat_softmax"),
    ("phl_uniform_compat_softmax", (A, 8, B, 8, 1.0, -1.0, C, 8, 5, 0, 0), INVALID, "phl_uniform_compat_softmax"),
    ("phl_uniform_compat_softmax", (A, 6, B, 6, 1.0, -1.0, C, 6, 5, 6, 0), UNSUPPORTED, "phl_uniform_compat_softmax"),
    ("phl_uniform_compat_softmax", (A, 1028, B, 1028, 1.0, -1.0, C, 1028, 5, 1028, 0), UNSUPPORTED, "phl_uniform_compat_softmax"),
    ("phl_uniform_compat_softmax", (A, 8, B, 10, 1.0, -1.0, C, 8, 5, 8, 0), UNSUPPORTED, "phl_uniform_compat_softmax"),
    ("phl_uniform_compat_softmax", (A, 8, MIS, 8, 1.0, -1.0, C, 8, 5, 8, 0), UNSUPPORTED, "phl_uniform_compat_softmax"),
    ("phl_uniform_compat_softmax", (MIS, 8, B, 8, 1.0, -1.0, C, 8, 5, 8, 0), UNSUPPORTED, "phl_uniform_compat_softmax"),
    ("phl_uniform_compat_softmax", (A, 8, B, 8, 1.0, -1.0, MIS, 8, 5, 8, 0), UNSUPPORTED, "phl_uniform_compat_softmax"),
    ("phl_uniform_compat_softmax", (A, 6, B, 8, 1.0, -1.0, C, 8, 5, 8, 0), UNSUPPORTED, "phl_uniform_compat_softmax"),
    ("phl_uniform_compat_softmax", (A, 8, B, 8, 1.0, -1.0, C, 2, 5, 8, 0), UNSUPPORTED, "phl_uniform_compat_softmax"),
    ("phl_uniform_compat_softmax", (MIS, 6, MIS, 6, 1.0, -1.0, MIS, 6, 0, 6, 0), OK, None),
    # phl_compat_softmax(E0, e_rs, X, x_rs, MuT, out, o_rs, n, L, flags)
    ("phl_compat_softmax", (A, 64, B, 64, None, D, 64, 5, 64, 0), INVALID, "phl_compat_softmax"),
    ("phl_compat_softmax", (A, 64, B, 64, C, D, 64, -3, 64, 0), INVALID, "phl_compat_softmax"),
    ("phl_compat_softmax", (A, 260, B, 260, C, D, 260, 5, 260, 0), UNSUPPORTED, "phl_compat_softmax"),
    ("phl_compat_softmax", (A, 64, B, 64, C, D, 64, 5, 62, 0), UNSUPPORTED, "phl_compat_softmax"),
    ("phl_compat_softmax", (A, 66, B, 64, C, D, 64, 5, 64, 0), UNSUPPORTED, "phl_compat_softmax"),
    ("phl_compat_softmax", (A, 64, B, 1 << 24, C, D, 64, 5, 64, 0), UNSUPPORTED, "phl_compat_softmax"),
    ("phl_compat_softmax", (A, 64, B, 64, MIS, D, 64, 5, 64, 0), UNSUPPORTED, "phl_compat_softmax"),
    ("phl_compat_softmax", (A, 64, B, 64, C, MIS, 64, 5, 64, 0), UNSUPPORTED, "phl_compat_softmax"),
    ("phl_compat_softmax", (A, 64, MIS, 64, C, D, 64, 5, 64, 0), UNSUPPORTED, "phl_compat_softmax"),
    ("phl_compat_softmax", (MIS, 64, B, 64, C, D, 64, 5, 64, 0), UNSUPPORTED, "phl_compat_softmax"),
    ("phl_compat_softmax", (A, 64, B, 66, C, D, 64, 5, 64, 0), UNSUPPORTED, "phl_compat_softmax"),
    ("phl_compat_softmax", (A, 64, B, 64, C, D, 70, 5, 64, 0), UNSUPPORTED, "phl_compat_softmax"),
    ("phl_compat_softmax", (A, 1 << 24, B, 64, C, D, 64, 5, 64, 0), UNSUPPORTED, "phl_compat_softmax"),
    ("phl_compat_softmax", (A, 64, B, 64, C, D, 1 << 24, 5, 64, 0), UNSUPPORTED, "phl_compat_softmax"),
    ("phl_compat_softmax", (None, 3, None, 3, None, None, 3, 0, 300, 0), OK, None),
    # phl_compat_softmax_split(E0, e_rs, X, x_rs, MuT, planes, out, o_rs, n, L, flags)
    ("phl_compat_softmax_split", (A, 256, B, 256, C, None, D, 256, 5, 256, 0), INVALID, "phl_compat_softmax_split"),
    ("phl_compat_softmax_split", (A, 256, B, 256, C, A, D, 256, 5, -4, 0), INVALID, "phl_compat_softmax_split"),
    ("phl_compat_softmax_split", (A, 128, B, 128, C, A, D, 128, 5, 128, 0), UNSUPPORTED, "phl_compat_softmax_split"),
    ("phl_compat_softmax_split", (A, 516, B, 516, C, A, D, 516, 5, 516, 0), UNSUPPORTED, "phl_compat_softmax_split"),
    ("phl_compat_softmax_split", (A, 344, B, 344, C, A, D, 344, 5, 342, 0), UNSUPPORTED, "phl_compat_softmax_split"),
    ("phl_compat_softmax_split", (A, 344, B, 344, C, A, D, 346, 5, 344, 0), UNSUPPORTED, "phl_compat_softmax_split"),
    ("phl_compat_softmax_split", (A, 256, B, 256, C, MIS, D, 256, 5, 256, 0), UNSUPPORTED, "phl_compat_softmax_split"),
    ("phl_compat_softmax_split", (MIS, 256, B, 256, C, A, D, 256, 5, 256, 0), UNSUPPORTED, "phl_compat_softmax_split"),
    ("phl_compat_softmax_split", (A, 256, MIS, 256, C, A, D, 256, 5, 256, 0), UNSUPPORTED, "phl_compat_softmax_split"),
    ("phl_compat_softmax_split", (A, 256, B, 256, MIS, A, D, 256, 5, 256, 0), UNSUPPORTED, "phl_compat_softmax_split"),
    ("phl_compat_softmax_split", (A, 256, B, 256, C, A, MIS, 256, 5, 256, 0), UNSUPPORTED, "phl_compat_softmax_split"),
    ("phl_compat_softmax_split", (A, 258, B, 256, C, A, D, 256, 5, 256, 0), UNSUPPORTED, "phl_compat_softmax_split"),
    ("phl_compat_softmax_split", (A, 256, B, 254, C, A, D, 256, 5, 256, 0), UNSUPPORTED, "phl_compat_softmax_split"),
    ("phl_compat_softmax_split", (A, 256, B, 256, C, A, D, 1 << 24, 5, 256, 0), UNSUPPORTED, "phl_compat_softmax_split"),
    ("phl_compat_softmax_split", (None, 1, None, 1, None, None, None, 1, 0, 100, 0), OK, None),
    # phl_compat_prepare(MuT, L, planes): the label range first, then the pointers
    ("phl_compat_prepare", (None, 128, None), UNSUPPORTED, "phl_compat_prepare"),
    ("phl_compat_prepare", (A, 514, B), UNSUPPORTED, "phl_compat_prepare"),
    ("phl_compat_prepare", (None, 256, B), INVALID, "phl_compat_prepare"),
    ("phl_compat_prepare", (A, 344, None), INVALID, "phl_compat_prepare"),
    ("phl_compat_prepare", (MIS, 256, B), INVALID, "phl_compat_prepare"),
    ("phl_compat_prepare", (A, 344, MIS), INVALID, "phl_compat_prepare"),
    # phl_uniform_compat_grad(Q, q_rs, gQ, g_rs, alpha, beta, dE, d_rs, gX, x_rs, n, L): shapes before n == 0
    ("phl_uniform_compat_grad", (A, 8, None, 8, 1.0, -1.0, C, 8, D, 8, 5, 8), INVALID, "phl_uniform_compat_grad"),
    ("phl_uniform_compat_grad", (A, 8, B, 8, 1.0, -1.0, None, 8, D, 8, 5, 8), INVALID, "phl_uniform_compat_grad"),
    ("phl_uniform_compat_grad", (A, 8, B, 8, 1.0, -1.0, C, 8, D, 8, -1, 8), INVALID, "phl_uniform_compat_grad"),
    ("phl_uniform_compat_grad", (A, 8, B, 8, 1.0, -1.0, C, 8, D, 8, 5, 0), INVALID, "phl_uniform_compat_grad"),
    ("phl_uniform_compat_grad", (A, 8, B, 8, 1.0, -1.0, C, 8, D, 8, 0, 2), UNSUPPORTED, "phl_uniform_compat_grad"),
    ("phl_uniform_compat_grad", (A, 8, B, 8, 1.0, -1.0, C, 8, D, 8, 0, 6), UNSUPPORTED, "phl_uniform_compat_grad"),
    ("phl_uniform_compat_grad", (A, 8, B, 8, 1.0, -1.0, C, 8, D, 8, 0, 516), UNSUPPORTED, "phl_uniform_compat_grad"),
    ("phl_uniform_compat_grad", (A, 6, B, 8, 1.0, -1.0, C, 8, D, 8, 0, 8), UNSUPPORTED, "phl_uniform_compat_grad"),
    ("phl_uniform_compat_grad", (A, 8, B, 8, 1.0, -1.0, C, 8, D, 2, 0, 8), UNSUPPORTED, "phl_uniform_compat_grad"),
    ("phl_uniform_compat_grad", (A, 8, B, 8, 1.0, -1.0, C, 8, MIS, 8, 0, 8), UNSUPPORTED, "phl_uniform_compat_grad"),
    ("phl_uniform_compat_grad", (MIS, 8, B, 8, 1.0, -1.0, C, 8, D, 8, 0, 8), UNSUPPORTED, "phl_uniform_compat_grad"),
    ("phl_uniform_compat_grad", (A, 8, MIS, 8, 1.0, -1.0, C, 8, D, 8, 0, 8), UNSUPPORTED, "phl_uniform_compat_grad"),
    ("phl_uniform_compat_grad", (A, 8, B, 8, 1.0, -1.0, MIS, 8, D, 8, 0, 8), UNSUPPORTED, "phl_uniform_compat_grad"),
    ("phl_uniform_compat_grad", (A, 8, B, 10, 1.0, -1.0, C, 8, D, 8, 0, 8), UNSUPPORTED, "phl_uniform_compat_grad"),
    ("phl_uniform_compat_grad", (A, 8, B, 8, 1.0, -1.0, C, 6, D, 8, 0, 8), UNSUPPORTED, "phl_uniform_compat_grad"),
    ("phl_uniform_compat_grad", (None, 3, B, 8, 1.0, -1.0, C, 8, None, 1, 0, 8), OK, None),
    ("phl_uniform_compat_grad", (A, 8, B, 8, 1.0, -1.0, C, 8, D, 8, 0, 512), OK, None),
    # phl_softmax_neg_grad(Q, q_rs, gQ, g_rs, dE, d_rs, n, L)
    ("phl_softmax_neg_grad", (A, 8, B, 8, None, 8, 5, 8), INVALID, "phl_uniform_compat_grad"),
    ("phl_softmax_neg_grad", (A, 8, B, 8, C, 8, 0, 10), UNSUPPORTED, "phl_uniform_compat_grad / phl_softmax_neg_grad"),
    ("phl_softmax_neg_grad", (A, 8, B, 9, C, 8, 0, 8), UNSUPPORTED, "phl_uniform_compat_grad / phl_softmax_neg_grad"),
    ("phl_softmax_neg_grad", (A, 8, B, 8, MIS, 8, 0, 8), UNSUPPORTED, "phl_uniform_compat_grad / phl_softmax_neg_grad"),
    ("phl_softmax_neg_grad", (A, 8, B, 8, C, 8, 0, 8), OK, None),
    # phl_compat_grad_x(dE, de_rs, Mu, scale, gX, gx_rs, n, L)
    ("phl_compat_grad_x", (A, 8, None, 1.0, C, 8, 5, 8), INVALID, "phl_compat_grad_x"),
    ("phl_compat_grad_x", (A, 8, B, 1.0, C, 8, -2, 8), INVALID, "phl_compat_grad_x"),
    ("phl_compat_grad_x", (A, 8, B, 1.0, C, 8, 0, 514), UNSUPPORTED, "phl_compat_grad_x"),
    ("phl_compat_grad_x", (A, 8, B, 1.0, C, 8, 0, 6), UNSUPPORTED, "phl_compat_grad_x"),
    ("phl_compat_grad_x", (None, 3, None, 1.0, None, 8, 0, 8), UNSUPPORTED, "phl_compat_grad_x"),
    ("phl_compat_grad_x", (A, 8, B, 1.0, C, 6, 0, 8), UNSUPPORTED, "phl_compat_grad_x"),
    ("phl_compat_grad_x", (A, 8, MIS, 1.0, C, 8, 0, 8), UNSUPPORTED, "phl_compat_grad_x"),
    ("phl_compat_grad_x", (MIS, 8, B, 1.0, C, 8, 0, 8), UNSUPPORTED, "phl_compat_grad_x"),
    ("phl_compat_grad_x", (A, 8, B, 1.0, MIS, 8, 0, 8), UNSUPPORTED, "phl_compat_grad_x"),
    ("phl_compat_grad_x", (A, 10, B, 1.0, C, 8, 0, 8), UNSUPPORTED, "phl_compat_grad_x"),
    ("phl_compat_grad_x", (None, 8, None, 1.0, None, 8, 0, 8), OK, None),
    # phl_compat_mu_grad(X, x_rs, dE, de_rs, scale, n, L, workspace, gMu, accumulate): every valid call launches
    ("phl_compat_mu_grad", (A, 8, B, 8, 1.0, 0, 8, C, None, 0), INVALID, "phl_compat_mu_grad"),
    ("phl_compat_mu_grad", (A, 8, B, 8, 1.0, 0, 8, None, D, 0), INVALID, "phl_compat_mu_grad"),
    ("phl_compat_mu_grad", (None, 8, B, 8, 1.0, 5, 8, C, D, 0), INVALID, "phl_compat_mu_grad"),
    ("phl_compat_mu_grad", (A, 8, B, 8, 1.0, -1, 8, C, D, 0), INVALID, "phl_compat_mu_grad"),
    ("phl_compat_mu_grad", (A, 8, B, 8, 1.0, 5, 6, C, D, 0), UNSUPPORTED, "phl_compat_mu_grad"),
    ("phl_compat_mu_grad", (A, 8, B, 8, 1.0, 5, 520, C, D, 0), UNSUPPORTED, "phl_compat_mu_grad"),
    ("phl_compat_mu_grad", (A, 2, B, 8, 1.0, 5, 8, C, D, 0), UNSUPPORTED, "phl_compat_mu_grad"),
    ("phl_compat_mu_grad", (A, 8, B, 8, 1.0, 5, 8, MIS, D, 0), UNSUPPORTED, "phl_compat_mu_grad"),
    ("phl_compat_mu_grad", (A, 8, MIS, 8, 1.0, 5, 8, C, D, 0), UNSUPPORTED, "phl_compat_mu_grad"),
    ("phl_compat_mu_grad", (MIS, 8, B, 8, 1.0, 5, 8, C, D, 0), UNSUPPORTED, "phl_compat_mu_grad"),
    ("phl_compat_mu_grad", (A, 8, B, 6, 1.0, 5, 8, C, D, 0), UNSUPPORTED, "phl_compat_mu_grad"),
]


@pytest.mark.parametrize("name,args,status,message", CASES, ids=[f"{c[0]}-{i}" for i, c in enumerate(CASES)])
def test_compat_entry_point_argument_checks(name, args, status, message):
    import phl

    lib = phl.load_library()
    assert getattr(lib, name)(*args, None) == status
    if message is not None:
        assert lib.phl_last_error().decode().startswith(message), lib.phl_last_error()
