"""What needs no GPU of the expected-label head (include/phl.h: phl_nchw_expected_value, phl_nchw_expected_value_grad):
the argument checks of both entry points with the status each returns -- every case returns before the first HIP call,
the pointers are never dereferenced --, what the binding refuses, and the CPU side of the surface:
logits2average_depth and CRFasRNN.expected_depth compute the present torch lines bit for bit."""
import pytest
import torch
import torch.nn.functional as F

OK, INVALID, TOO_LARGE = 0, 1, 6
X, G, LAB, O, GO, MIS = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6004   # fake device addresses; MIS is off the 16-byte grid
WG = 1024                                                                # PHL_NCHW_EXPECT_PIXELS
I31 = (1 << 31) - 1

# (X, G, labels, out, B, L, n, negate) -> status
FORWARD = [
    # negative sizes, L < 1 (checked before the element count)
    ((X, G, LAB, O, -1, 8, 64, 0), INVALID),
    ((X, G, LAB, O, 2, 8, -64, 1), INVALID),
    ((X, G, LAB, O, 2, 0, 64, 0), INVALID),
    ((X, G, LAB, O, 2, -3, 64, 1), INVALID),
    ((X, G, LAB, O, 2, 0, 0, 0), INVALID),
    ((None, None, None, None, 0, 0, 64, 0), INVALID),
    # zero elements: PHL_OK whatever the pointers and the label count
    ((MIS, MIS, MIS, MIS, 2, 8, 0, 0), OK),
    ((None, None, None, None, 0, 8, 64, 1), OK),
    ((None, None, None, None, 3, 5000, 0, 0), OK),
    ((X, G, LAB, X, 0, 257, 64, 1), OK),
    ((MIS, None, None, None, I31, I31, 0, 0), OK),
    # null pointers with elements present; NULL G and NULL labels are legal (they fail later: too large)
    ((None, G, LAB, O, 2, 8, 64, 0), INVALID),
    ((X, G, LAB, None, 2, 8, 64, 1), INVALID),
    ((None, None, None, None, 1, 1, 1, 0), INVALID),
    ((X, None, None, O, 1, 1, 1 << 62, 0), TOO_LARGE),
    # out aliasing an input
    ((X, G, LAB, X, 2, 8, 64, 0), INVALID),
    ((X, G, LAB, G, 2, 8, 64, 1), INVALID),
    ((X, G, LAB, LAB, 2, 8, 64, 0), INVALID),
    ((X, None, None, X, 1, 1, 1, 1), INVALID),
    # too many elements: the byte count leaves int64, or the workgroups leave the grid
    ((X, G, LAB, O, 1 << 20, 1 << 20, 1 << 40, 0), TOO_LARGE),
    ((X, G, LAB, O, I31, I31, 2, 1), TOO_LARGE),
    ((X, G, LAB, O, 1, 1, 1 << 61, 0), TOO_LARGE),
    ((X, G, LAB, O, 1, 1, WG * I31 + 1, 0), TOO_LARGE),                  # 2^31 workgroups, 8 TiB: the grid alone
    ((MIS, G, None, O, 1 << 16, 1, WG << 15, 1), TOO_LARGE),             # 2^16 images of 2^15 workgroups
]
# (X, G, labels, gout, gZ, B, L, n, negate) -> status
GRAD = [
    ((X, G, LAB, GO, O, -1, 8, 64, 0), INVALID),
    ((X, G, LAB, GO, O, 2, 8, -64, 1), INVALID),
    ((X, G, LAB, GO, O, 2, 0, 64, 0), INVALID),
    ((X, G, LAB, GO, O, 2, -1, 0, 0), INVALID),
    ((MIS, MIS, MIS, MIS, MIS, 2, 8, 0, 0), OK),
    ((None, None, None, None, None, 0, 8, 64, 1), OK),
    ((X, G, LAB, X, X, 3, 1030, 0, 0), OK),
    ((None, G, LAB, GO, O, 2, 8, 64, 0), INVALID),
    ((X, G, LAB, None, O, 2, 8, 64, 0), INVALID),
    ((X, G, LAB, GO, None, 2, 8, 64, 1), INVALID),
    ((X, None, None, GO, O, 1, 1, 1 << 62, 0), TOO_LARGE),               # NULL G and NULL labels are legal
    ((X, G, LAB, GO, X, 2, 8, 64, 0), INVALID),
    ((X, G, LAB, GO, G, 2, 8, 64, 0), INVALID),
    ((X, G, LAB, GO, LAB, 2, 8, 64, 1), INVALID),
    ((X, G, LAB, GO, GO, 2, 8, 64, 0), INVALID),
    ((X, G, LAB, GO, O, 1 << 20, 1 << 20, 1 << 40, 0), TOO_LARGE),
    ((X, G, LAB, GO, O, I31, I31, 2, 1), TOO_LARGE),
    ((X, G, LAB, GO, O, 1, 1, WG * I31 + 1, 0), TOO_LARGE),
    ((X, MIS, None, GO, O, 1 << 16, 1, WG << 15, 1), TOO_LARGE),
]


def _check(name, args, status):
    import phl

    lib = phl.load_library()
    assert getattr(lib, name)(*args, None) == status
    if status != OK:
        text = lib.phl_last_error().decode()
        assert text.startswith(name + ":"), text


@pytest.mark.parametrize("args,status", FORWARD, ids=[f"{i}-{c[1]}" for i, c in enumerate(FORWARD)])
def test_expected_value_argument_checks(args, status):
    _check("phl_nchw_expected_value", args, status)


@pytest.mark.parametrize("args,status", GRAD, ids=[f"{i}-{c[1]}" for i, c in enumerate(GRAD)])
def test_expected_value_grad_argument_checks(args, status):
    _check("phl_nchw_expected_value_grad", args, status)


def test_binding_checks_need_no_gpu():
    """What the binding refuses before it reaches the library."""
    import phl

    x = torch.zeros(1, 4, 3, 3)
    with pytest.raises(TypeError):
        phl.nchw_expected_value(x)                                          # a CPU tensor
    with pytest.raises(TypeError):
        phl.nchw_expected_value(x, x, negate=True)
    with pytest.raises(TypeError):
        phl.nchw_expected_value_grad(x, None, None, torch.zeros(1, 1, 3, 3))
    with pytest.raises(TypeError):
        phl.nchw_expected_value_fn(x.requires_grad_())
    assert phl.NCHW_EXPECT_PIXELS == WG
    assert issubclass(phl.NchwExpectedValue, torch.autograd.Function)


def _present_formula(logits, labels=None):
    """logits2average_depth as it stood before the kernel (crf/mb_stereo_crf.py of the reference, :62-66)."""
    probs = F.softmax(logits, dim=1)
    if labels is None:
        labels = torch.arange(probs.shape[1], dtype=torch.float32, device=probs.device)[None, :, None, None]
    return (probs * labels).sum(1, keepdim=True)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_logits2average_depth_on_cpu_is_the_present_formula(dtype):
    from crf.mb_stereo_crf import logits2average_depth

    g = torch.Generator().manual_seed(3)
    logits = (torch.rand((2, 7, 5, 6), generator=g) * 60 - 30).to(dtype)
    per_channel = (torch.rand((1, 7, 1, 1), generator=g) * 9 - 4).to(dtype)
    per_pixel = (torch.rand((2, 7, 5, 6), generator=g) * 9).to(dtype)
    for labels in (None, per_channel, per_pixel):
        got = logits2average_depth(logits, labels)
        want = _present_formula(logits, labels)
        assert got.dtype == want.dtype and got.shape == (2, 1, 5, 6) and torch.equal(got, want)
    grad_in = logits.clone().requires_grad_()
    out = logits2average_depth(grad_in, per_channel)
    assert torch.equal(out.detach(), _present_formula(logits, per_channel))
    out.sum().backward()
    assert grad_in.grad is not None and grad_in.grad.shape == logits.shape


@pytest.mark.parametrize("lattice_free_kwargs", [dict(niters=2, r=2), dict(niters=0, r=2), dict(niters=1, r=3, gchannels=3)])
def test_expected_depth_on_cpu_is_forward_then_the_average(lattice_free_kwargs):
    from crf.crf_module import CRFasRNN, charb
    from crf.mb_stereo_crf import logits2average_depth

    g = torch.Generator().manual_seed(5)
    L, H, W = 6, 9, 11
    net = CRFasRNN(charb(3.0), **lattice_free_kwargs)
    refs = torch.rand((2, lattice_free_kwargs.get("gchannels", 1), H, W), generator=g)
    logits = torch.randn((2, L, H, W), generator=g) * 3
    confidence = torch.rand((2, 1, H, W), generator=g)
    labels = torch.linspace(0, 7.5, L)
    values = torch.rand((L,), generator=g) * 5 - 1
    with torch.no_grad():
        for conf in (None, confidence):
            for lab in (None, labels):
                logit_out = net(refs, logits, conf, lab)
                assert torch.equal(net.expected_depth(refs, logits, conf, lab), logits2average_depth(logit_out))
                want = logits2average_depth(logit_out, values[None, :, None, None])
                assert torch.equal(net.expected_depth(refs, logits, conf, lab, values), want)                        # [L]
                assert torch.equal(net.expected_depth(refs, logits, conf, lab, values[None, :, None, None]), want)
                assert want.shape == (2, 1, H, W)
    # under autograd as well: the same numbers, and a gradient for the logits
    leaf = logits.clone().requires_grad_()
    out = net.expected_depth(refs, leaf, confidence, labels, labels)
    assert torch.equal(out.detach(), logits2average_depth(net(refs, logits, confidence, labels), labels[None, :, None, None]).detach())
    out.sum().backward()
    assert leaf.grad is not None and torch.isfinite(leaf.grad).all()


def test_heads_on_cpu_compute_what_they_computed():
    """The three heads end with CRFasRNN.expected_depth: on the CPU that is logits2average_depth of forward's logits."""
    from crf.mb_stereo_crf import CRFdepthRefiner, CRFdepthUpsampler, CRFwUncertainty, logits2average_depth

    g = torch.Generator().manual_seed(7)
    logits = torch.randn((1, 5, 12, 14), generator=g)
    rgb, feats = torch.rand((1, 3, 12, 14), generator=g), torch.rand((1, 8, 12, 14), generator=g)
    with torch.no_grad():
        ref = CRFdepthRefiner(d_in=8, d_guide=6, r=2, niters=1)
        want = logits2average_depth(ref.CRF(ref._guide(rgb, feats), logits))
        assert torch.equal(ref((logits, rgb, feats)), want)
        unc = CRFwUncertainty(d_in=8, d_guide=6, r=2, niters=1)
        depth, conf = unc((logits, rgb, feats))
        assert torch.equal(depth, logits2average_depth(unc.CRF(unc._guide(rgb, feats), logits, conf)))
        ups = CRFdepthUpsampler(r=2, niters=1)
        low = torch.rand((1, 1, 6, 7), generator=g) * 5
        up = F.interpolate(low, size=(12, 14), mode="bilinear", align_corners=False)
        labels = torch.linspace(0, float(up.max()), 18)
        lg = -10 * ups.CRF.Mu.get_energies_from_scalar(up, labels[None, :, None, None])
        want = logits2average_depth(ups.CRF(rgb, lg, confidence=(up > 1e-2).float(), labels=labels), labels[None, :, None, None])
        assert torch.equal(ups((low, rgb, None)), want)
