"""What needs no GPU of the confidence-weighted unaries (include/phl.h: phl_nchw_confidence_unaries,
phl_nchw_confidence_unaries_grad): the argument checks of both entry points with the status each returns -- every case
returns before the first HIP call, the pointers are never dereferenced --, what the binding refuses, the routing predicate
of CRFasRNN's E0 line, the keyword ``fused_unaries`` on the three heads, and the CPU side: with the keyword a net computes
on CPU tensors the bits it computes without."""
import inspect

import pytest
import torch

OK, INVALID, TOO_LARGE = 0, 1, 6
X, C, E, GE, GC, GL, MIS = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7004   # fake device addresses; MIS is off the 16-byte grid
WG = 1024                                                                           # PHL_NCHW_CONF_PIXELS
I31 = (1 << 31) - 1

# (logits, conf, E0, B, L, n) -> status
FORWARD = [
    # negative sizes, L < 1 (checked before the element count)
    ((X, C, E, -1, 8, 64), INVALID),
    ((X, C, E, 2, 8, -64), INVALID),
    ((X, C, E, 2, 0, 64), INVALID),
    ((X, C, E, 2, -3, 64), INVALID),
    ((X, C, E, 2, 0, 0), INVALID),
    ((None, None, None, 0, 0, 64), INVALID),
    # zero elements: PHL_OK whatever the pointers and the label count
    ((MIS, MIS, MIS, 2, 8, 0), OK),
    ((None, None, None, 0, 8, 64), OK),
    ((None, None, None, 3, 5000, 0), OK),
    ((X, C, X, 0, 257, 64), OK),
    ((MIS, None, None, I31, I31, 0), OK),
    # each null pointer with elements present
    ((None, C, E, 2, 8, 64), INVALID),
    ((X, None, E, 2, 8, 64), INVALID),
    ((X, C, None, 2, 8, 64), INVALID),
    ((None, None, None, 1, 1, 1), INVALID),
    # E0 aliasing an input (the inputs may be one another)
    ((X, C, X, 2, 8, 64), INVALID),
    ((X, C, C, 2, 8, 64), INVALID),
    ((X, X, X, 1, 1, 1), INVALID),
    ((X, X, E, 1, 1, 1 << 62), TOO_LARGE),
    # too many elements: the byte count leaves int64, or the workgroups leave the grid
    ((X, C, E, 1 << 20, 1 << 20, 1 << 40), TOO_LARGE),
    ((X, C, E, I31, I31, 2), TOO_LARGE),
    ((X, C, E, 1, 1, 1 << 61), TOO_LARGE),
    ((X, C, E, 1, 1, WG * I31 + 1), TOO_LARGE),                           # 2^31 workgroups, 8 TiB: the grid alone
    ((MIS, C, E, 1 << 16, 1, WG << 15), TOO_LARGE),                       # 2^16 images of 2^15 workgroups
]
# (logits, conf, gE0, grad_conf, grad_logits, B, L, n) -> status
GRAD = [
    ((X, C, GE, GC, GL, -1, 8, 64), INVALID),
    ((X, C, GE, GC, GL, 2, 8, -64), INVALID),
    ((X, C, GE, GC, GL, 2, 0, 64), INVALID),
    ((X, C, GE, GC, GL, 2, -1, 0), INVALID),
    ((None, None, None, None, None, 0, 0, 64), INVALID),
    # zero elements
    ((MIS, MIS, MIS, MIS, MIS, 2, 8, 0), OK),
    ((None, None, None, None, None, 0, 8, 64), OK),
    ((X, C, GE, X, X, 3, 1030, 0), OK),
    ((X, C, GE, None, None, 0, 8, 64), OK),
    # each null input; either output alone is legal (they fail later: too large), both missing is not
    ((None, C, GE, GC, GL, 2, 8, 64), INVALID),
    ((X, None, GE, GC, GL, 2, 8, 64), INVALID),
    ((X, C, None, GC, GL, 2, 8, 64), INVALID),
    ((None, C, GE, None, GL, 2, 8, 64), INVALID),
    ((X, None, GE, GC, None, 2, 8, 64), INVALID),
    ((X, C, GE, None, None, 2, 8, 64), INVALID),
    ((X, C, GE, GC, None, 1, 1, 1 << 62), TOO_LARGE),
    ((X, C, GE, None, GL, 1, 1, 1 << 62), TOO_LARGE),
    # an output that is one of the inputs, or the other output -- with and without the other output
    ((X, C, GE, X, GL, 2, 8, 64), INVALID),
    ((X, C, GE, C, GL, 2, 8, 64), INVALID),
    ((X, C, GE, GE, GL, 2, 8, 64), INVALID),
    ((X, C, GE, GC, X, 2, 8, 64), INVALID),
    ((X, C, GE, GC, C, 2, 8, 64), INVALID),
    ((X, C, GE, GC, GE, 2, 8, 64), INVALID),
    ((X, C, GE, GC, GC, 2, 8, 64), INVALID),
    ((X, C, GE, X, None, 2, 8, 64), INVALID),
    ((X, C, GE, C, None, 2, 8, 64), INVALID),
    ((X, C, GE, GE, None, 2, 8, 64), INVALID),
    ((X, C, GE, None, X, 2, 8, 64), INVALID),
    ((X, C, GE, None, C, 2, 8, 64), INVALID),
    ((X, C, GE, None, GE, 2, 8, 64), INVALID),
    ((X, C, GE, GC, GE, 1, 1, 1 << 62), INVALID),                         # aliasing is seen before the element count
    # too many elements
    ((X, C, GE, GC, GL, 1 << 20, 1 << 20, 1 << 40), TOO_LARGE),
    ((X, C, GE, GC, GL, I31, I31, 2), TOO_LARGE),
    ((X, C, GE, GC, GL, 1, 1, 1 << 61), TOO_LARGE),
    ((X, C, GE, GC, GL, 1, 1, WG * I31 + 1), TOO_LARGE),
    ((X, MIS, GE, GC, None, 1 << 16, 1, WG << 15), TOO_LARGE),
]


def _check(name, args, status):
    import phl

    lib = phl.load_library()
    assert getattr(lib, name)(*args, None) == status
    if status != OK:
        text = lib.phl_last_error().decode()
        assert text.startswith(name + ":"), text


@pytest.mark.parametrize("args,status", FORWARD, ids=[f"{i}-{c[1]}" for i, c in enumerate(FORWARD)])
def test_confidence_unaries_argument_checks(args, status):
    _check("phl_nchw_confidence_unaries", args, status)


@pytest.mark.parametrize("args,status", GRAD, ids=[f"{i}-{c[1]}" for i, c in enumerate(GRAD)])
def test_confidence_unaries_grad_argument_checks(args, status):
    _check("phl_nchw_confidence_unaries_grad", args, status)


def test_binding_checks_need_no_gpu():
    """What the binding refuses before it reaches the library: CPU tensors are a TypeError, whatever else is wrong."""
    import phl

    x, c = torch.zeros(1, 4, 3, 3), torch.ones(1, 1, 3, 3)
    with pytest.raises(TypeError):
        phl.nchw_confidence_unaries(x, c)
    with pytest.raises(TypeError):
        phl.nchw_confidence_unaries(x.double(), c.double())
    with pytest.raises(TypeError):
        phl.nchw_confidence_unaries_grad(x, c, x)
    with pytest.raises(TypeError):
        phl.nchw_confidence_unaries_grad(x, c, x, need_conf=False, need_logits=False)
    with pytest.raises(TypeError):
        phl.nchw_confidence_unaries_fn(x, c.clone().requires_grad_())
    assert phl.NCHW_CONF_PIXELS == WG
    assert issubclass(phl.NchwConfidenceUnaries, torch.autograd.Function)
    grad = inspect.signature(phl.nchw_confidence_unaries_grad).parameters
    assert grad["need_conf"].default is True and grad["need_logits"].default is False
    assert all(grad[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("need_conf", "need_logits"))
    assert inspect.signature(phl.nchw_confidence_unaries).parameters["out"].kind is inspect.Parameter.KEYWORD_ONLY


def test_the_routing_predicate_off_the_gpu(monkeypatch):
    """False for everything that is not a pair of fp32 CUDA logits [B, L, H, W] and a fp32 [B, 1, H, W] confidence on
    their device.  Without a GPU a stand-in carries what the predicate reads of a CUDA tensor, so that the routed case is
    seen too, and the dtype, the shape and the device are seen to be what turns it down."""
    from crf import crf_module as cm

    route = cm._confidence_routable
    logits, conf = torch.zeros(2, 5, 3, 4), torch.ones(2, 1, 3, 4)
    assert not route(logits, conf)                                            # CPU
    assert not route(logits.double(), conf.double())
    assert not route(logits, None) and not route(None, conf) and not route(logits, 0.5)

    class OnDevice:
        """What the predicate reads of a tensor, with is_cuda set."""
        def __init__(self, shape, dtype=torch.float32, device="cuda:0", is_cuda=True):
            self.shape, self.dtype, self.device, self.is_cuda = shape, dtype, device, is_cuda

        def dim(self):
            return len(self.shape)

    monkeypatch.setattr(torch, "is_tensor", lambda t: isinstance(t, (torch.Tensor, OnDevice)))
    lg = OnDevice((2, 5, 3, 4))
    assert route(lg, OnDevice((2, 1, 3, 4)))                                  # the case that is routed
    assert route(OnDevice((2, 1, 3, 4)), OnDevice((2, 1, 3, 4)))              # one label
    assert route(OnDevice((0, 5, 3, 4)), OnDevice((0, 1, 3, 4)))              # nothing to do is the kernel's PHL_OK
    assert not route(lg, OnDevice((2, 5, 3, 4)))                              # a confidence per label
    assert not route(lg, OnDevice((1, 1, 3, 4)))                              # broadcast over the batch
    assert not route(lg, OnDevice((2, 1, 1, 1))) and not route(lg, OnDevice((2, 1, 3, 1)))
    assert not route(lg, OnDevice((1, 3, 4))) and not route(lg, OnDevice((3, 4))) and not route(lg, OnDevice(()))
    assert not route(lg, OnDevice((2, 1, 3, 4), dtype=torch.float64))
    assert not route(OnDevice((2, 5, 3, 4), dtype=torch.float64), OnDevice((2, 1, 3, 4)))
    assert not route(OnDevice((2, 5, 3, 4), dtype=torch.float16), OnDevice((2, 1, 3, 4), dtype=torch.float16))
    assert not route(lg, OnDevice((2, 1, 3, 4), device="cuda:1"))
    assert not route(lg, OnDevice((2, 1, 3, 4), device="cpu", is_cuda=False))
    assert not route(OnDevice((2, 5, 3, 4), device="cpu", is_cuda=False), OnDevice((2, 1, 3, 4), device="cpu", is_cuda=False))
    assert not route(OnDevice((2, 5, 12)), OnDevice((2, 1, 12)))              # [B, L, n]: the binding's, not CRFasRNN's
    assert not route(lg, 0.5) and not route(lg, None)


def test_the_heads_forward_the_keyword():
    from crf.crf_module import CRFasRNN, charb
    from crf.mb_stereo_crf import CRFdepthRefiner, CRFdepthUpsampler, CRFwUncertainty

    params = inspect.signature(CRFasRNN.__init__).parameters
    names = list(params)
    assert params["fused_unaries"].kind is inspect.Parameter.KEYWORD_ONLY and params["fused_unaries"].default is False
    assert names.index("fused_unaries") == names.index("bilinear_full_grad") + 1
    assert CRFasRNN(charb(.05)).fused_unaries is False and CRFasRNN(charb(.05), fused_unaries=True).fused_unaries is True
    assert CRFasRNN(charb(.05), lattice=True, fused_unaries=True).fused_unaries is True
    for head, kw in ((CRFdepthRefiner, dict(d_in=8, d_guide=6)), (CRFwUncertainty, dict(d_in=8, d_guide=6)), (CRFdepthUpsampler, {})):
        p = inspect.signature(head.__init__).parameters
        if "fused_unaries" in p:                                              # (CRFwUncertainty takes *args, **kwargs)
            assert p["fused_unaries"].kind is inspect.Parameter.KEYWORD_ONLY and p["fused_unaries"].default is False
        assert head(**kw).CRF.fused_unaries is False
        assert head(fused_unaries=True, **kw).CRF.fused_unaries is True


@pytest.mark.parametrize("kwargs", [dict(niters=2, r=2), dict(niters=0, r=2), dict(niters=1, r=3, gchannels=3)])
def test_on_cpu_tensors_the_keyword_changes_no_bit(kwargs):
    from crf.crf_module import CRFasRNN, charb

    g = torch.Generator().manual_seed(13)
    L, H, W = 6, 9, 11
    old, new = CRFasRNN(charb(3.0), **kwargs), CRFasRNN(charb(3.0), fused_unaries=True, **kwargs)
    new.load_state_dict(old.state_dict())
    refs = torch.rand((2, kwargs.get("gchannels", 1), H, W), generator=g)
    logits = torch.randn((2, L, H, W), generator=g) * 3
    energies = torch.rand((2, L, H, W), generator=g) * 8
    labels, values = torch.linspace(0, 7.5, L), torch.rand((L,), generator=g) * 5 - 1
    per_pixel, per_label = torch.rand((2, 1, H, W), generator=g), torch.rand((2, L, H, W), generator=g)
    with torch.no_grad():
        for conf in (None, per_pixel, per_label, 0.5, per_pixel.double()):
            lg = logits.double() if torch.is_tensor(conf) and conf.dtype == torch.float64 else logits
            rf = refs.to(lg.dtype)
            a, b = (old if lg is logits else old.double()), (new if lg is logits else new.double())
            assert torch.equal(a(rf, lg, conf, labels.to(lg.dtype)), b(rf, lg, conf, labels.to(lg.dtype)))
            assert torch.equal(a.expected_depth(rf, lg, conf, labels.to(lg.dtype), values.to(lg.dtype)),
                               b.expected_depth(rf, lg, conf, labels.to(lg.dtype), values.to(lg.dtype)))
        old.float(), new.float()
        assert torch.equal(old(refs, None, energies=energies), new(refs, None, energies=energies))
    # recorded: the same bits, and the same gradients for the logits and the confidence
    grads = []
    for net in (old, new):
        lg, cf = logits.clone().requires_grad_(), per_pixel.clone().requires_grad_()
        out = net.expected_depth(refs, lg, cf, labels, values)
        out.sum().backward()
        grads.append((out.detach(), lg.grad, cf.grad))
    for x, y in zip(*grads):
        assert x is not None and torch.equal(x, y)


def test_the_heads_on_cpu_compute_what_they_computed():
    from crf.mb_stereo_crf import CRFdepthRefiner, CRFdepthUpsampler, CRFwUncertainty

    g = torch.Generator().manual_seed(17)
    logits = torch.randn((1, 5, 12, 14), generator=g)
    rgb, feats = torch.rand((1, 3, 12, 14), generator=g), torch.rand((1, 8, 12, 14), generator=g)
    low = torch.rand((1, 1, 6, 7), generator=g) * 5
    low[0, 0, :2, :2] = 0
    with torch.no_grad():
        for head, kw, inputs in ((CRFdepthRefiner, dict(d_in=8, d_guide=6), (logits, rgb, feats)),
                                 (CRFwUncertainty, dict(d_in=8, d_guide=6), (logits, rgb, feats)),
                                 (CRFdepthUpsampler, {}, (low, rgb, None))):
            torch.manual_seed(19)
            old = head(r=2, niters=1, **kw)
            new = head(r=2, niters=1, fused_unaries=True, **kw)
            new.load_state_dict(old.state_dict())
            a, b = old(inputs), new(inputs)
            for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
                assert torch.equal(x, y)
