"""CPU: the training step's entry points (include/phl.h: phl_nchw_step_train, phl_nchw_step_train_grad,
phl_nchw_step_train_partials) and the ``fused_step`` keyword where no GPU is involved.  The argument checks return before
the first HIP call, so the pointers are never dereferenced."""
import pytest
import torch

OK, INVALID, TOO_LARGE, UNSUPPORTED = 0, 1, 6, 7
E, G, M, Y, O, GM, MIS = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7004      # fake device addresses

# (E0, G, mu, out, B, L, n) -> status, in the header's order: sizes, zero elements, pointers, size limits, label range
FORWARD = [
    ((E, G, M, O, 2, 0, 64), INVALID),
    ((E, G, M, O, 2, -3, 64), INVALID),
    ((E, G, M, O, -1, 18, 64), INVALID),
    ((E, G, M, O, 2, 18, -1), INVALID),
    ((E, G, M, O, 2, 0, 0), INVALID),                    # L is checked before the element count
    ((E, G, M, O, 0, 18, 64), OK),
    ((E, G, M, O, 2, 18, 0), OK),
    ((None, None, None, None, 0, 64, 64), OK),
    ((MIS, MIS, MIS, MIS, 3, 60, 0), OK),
    ((E, G, M, E, 0, 5000, 64), OK),                     # ... and the label range after it
    ((None, G, M, O, 2, 18, 64), INVALID),
    ((E, G, None, O, 2, 18, 64), INVALID),
    ((E, G, M, None, 2, 18, 64), INVALID),
    ((None, G, M, O, 2, 65, 64), INVALID),               # a null pointer before the label range
    ((E, G, M, E, 2, 18, 64), INVALID),
    ((E, G, M, G, 2, 18, 64), INVALID),
    ((E, None, M, M, 1, 18, 64), INVALID),
    ((E, G, M, E, 2, 65, 64), INVALID),                  # aliasing before the label range
    ((E, G, M, O, 1 << 20, 64, 1 << 40), TOO_LARGE),
    ((E, G, M, O, 1 << 16, 8, 1 << 22), TOO_LARGE),      # 2^16 tiles per image, 2^32 tiles
    ((E, G, M, O, 1 << 20, 1 << 20, 1 << 40), TOO_LARGE),    # the size before the label range
    ((E, G, M, O, 2, 65, 64), UNSUPPORTED),
    ((E, None, M, O, 1, 65, 1), UNSUPPORTED),
    ((E, G, M, O, 1, 1 << 20, 63), UNSUPPORTED),
]

# (E0, G, mu, gY, dE, gmu, B, L, n) -> status
BACKWARD = [
    ((E, G, M, Y, O, GM, 2, 0, 64), INVALID),
    ((E, G, M, Y, O, GM, -1, 18, 64), INVALID),
    ((E, G, M, Y, O, GM, 2, 18, -1), INVALID),
    ((E, G, M, Y, None, None, 2, 0, 0), INVALID),
    ((E, G, M, Y, O, GM, 0, 18, 64), OK),
    ((E, G, M, Y, O, GM, 2, 18, 0), OK),
    ((None, None, None, None, None, None, 0, 64, 64), OK),
    ((E, G, M, Y, E, E, 0, 5000, 64), OK),
    ((None, G, M, Y, O, GM, 2, 18, 64), INVALID),
    ((E, G, None, Y, O, GM, 2, 18, 64), INVALID),
    ((E, G, M, None, O, GM, 2, 18, 64), INVALID),
    ((E, G, M, Y, None, None, 2, 18, 64), INVALID),      # both outputs null
    ((E, None, M, Y, None, None, 1, 65, 64), INVALID),   # ... before the label range
    ((E, G, M, Y, E, GM, 2, 18, 64), INVALID),
    ((E, G, M, Y, Y, None, 2, 18, 64), INVALID),
    ((E, G, M, Y, O, M, 2, 18, 64), INVALID),
    ((E, G, M, Y, O, O, 2, 18, 64), INVALID),            # the two outputs on each other
    ((E, G, M, Y, None, Y, 2, 18, 64), INVALID),
    ((E, G, M, Y, O, G, 2, 65, 64), INVALID),
    ((E, G, M, Y, O, GM, 1 << 20, 64, 1 << 40), TOO_LARGE),
    ((E, G, M, Y, None, GM, 1 << 16, 8, 1 << 22), TOO_LARGE),
    ((E, G, M, Y, O, GM, 1 << 20, 1 << 20, 1 << 40), TOO_LARGE),
    ((E, G, M, Y, O, GM, 2, 65, 64), UNSUPPORTED),
    ((E, None, M, Y, None, GM, 1, 65, 1), UNSUPPORTED),
    ((E, None, M, Y, O, None, 1, 1 << 20, 63), UNSUPPORTED),
]


@pytest.mark.parametrize("args,status", FORWARD, ids=[f"{i}-L{c[0][5]}" for i, c in enumerate(FORWARD)])
def test_step_train_argument_checks(args, status):
    import phl

    lib = phl.load_library()
    assert lib.phl_nchw_step_train(*args, None) == status
    if status != OK:
        assert lib.phl_last_error().decode().startswith("phl_nchw_step_train:"), lib.phl_last_error()
    if status == UNSUPPORTED:
        assert "64" in lib.phl_last_error().decode(), lib.phl_last_error()


@pytest.mark.parametrize("args,status", BACKWARD, ids=[f"{i}-L{c[0][7]}" for i, c in enumerate(BACKWARD)])
def test_step_train_grad_argument_checks(args, status):
    import phl

    lib = phl.load_library()
    assert lib.phl_nchw_step_train_grad(*args, None) == status
    if status != OK:
        assert lib.phl_last_error().decode().startswith("phl_nchw_step_train_grad:"), lib.phl_last_error()
    if status == UNSUPPORTED:
        assert "64" in lib.phl_last_error().decode(), lib.phl_last_error()


def test_partials():
    import phl

    assert phl.NCHW_TRAIN_MAX_L == 64
    for B, L, n in ((1, 1, 1), (1, 18, 63), (1, 18, 64), (1, 18, 65), (3, 64, 130), (2, 4, 64 * 511), (1, 4, 64 * 1024),
                    (1, 4, 64 * 1024 + 1), (3, 60, 1110 * 1390), (1 << 20, 64, 1 << 40), (7, 2, (1 << 62) + 5)):
        tiles = B * ((n + 63) // 64)
        R = phl.nchw_step_train_partials(B, L, n)
        assert 1 <= R <= 1024 and R == min(tiles, 1024), (B, L, n, R)
        assert all(phl.nchw_step_train_partials(B, L, n) == R for _ in range(3))
    for B, L, n in ((0, 18, 64), (2, 18, 0), (-1, 18, 64), (2, 0, 64), (2, 18, -5)):
        assert phl.nchw_step_train_partials(B, L, n) == 0


def test_binding_checks_need_no_gpu():
    import phl

    with pytest.raises(TypeError):
        phl.nchw_step_train(torch.zeros(1, 18, 3, 3), None, torch.zeros(18, 18))                  # CPU tensors
    with pytest.raises(TypeError):
        phl.nchw_step_train_grad(torch.zeros(1, 18, 3, 3), None, torch.zeros(18, 18), torch.zeros(1, 18, 3, 3))


def test_fused_step_changes_nothing_on_cpu_float64():
    """fused_step=True where the kernels do not run (CPU, float64, under autograd): the plain loop's bits."""
    from crf.crf_module import CRFasRNN, charb

    gen = torch.Generator().manual_seed(3)
    L, H, W = 6, 9, 11
    logits0 = torch.randn((2, L, H, W), generator=gen, dtype=torch.float64)
    guide0 = torch.rand((2, 1, H, W), generator=gen, dtype=torch.float64)
    up = torch.randn((2, L, H, W), generator=gen, dtype=torch.float64)
    res = []
    for flag in (False, True):
        net = CRFasRNN(charb(3.0), niters=2, r=2, eps=1e-2, fused_step=flag).double()
        assert net.fused_step is flag
        logits, guide = logits0.clone().requires_grad_(True), guide0.clone().requires_grad_(True)
        out = net(guide, logits, labels=torch.arange(L, dtype=torch.float64))
        (out * up).sum().backward()
        res.append([out.detach(), logits.grad, guide.grad, net.Mu.gamma.grad, net.Mu.s.grad])
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_the_heads_forward_the_keyword():
    from crf.mb_stereo_crf import CRFdepthRefiner, CRFdepthUpsampler, CRFwUncertainty

    for head in (CRFdepthRefiner, CRFwUncertainty, CRFdepthUpsampler):
        assert head(fused_step=True).CRF.fused_step is True
        assert head().CRF.fused_step is False
        assert head(fused_grad=True).CRF.fused_step is False and head(fused_grad=True).CRF.fused_grad is True
