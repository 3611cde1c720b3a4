"""What needs no GPU of the upsampler head's scalar unaries (include/phl.h: phl_nchw_scalar_unaries,
phl_nchw_scalar_unaries_grad): the argument checks of both entry points with the status each returns -- every case returns
before the first HIP call, the pointers are never dereferenced --, what the binding refuses, the head's routing predicate,
and CRFasRNN's ``energies=`` keyword on the CPU: E0 handed over as it is computes what ``-logits`` computed, bit for bit."""
import pytest
import torch

OK, INVALID, TOO_LARGE = 0, 1, 6
D, GA, S, E, LAB, GE, GR = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000     # fake device addresses
WG = 1024                                                                             # PHL_NCHW_SCALAR_PIXELS
I31 = (1 << 31) - 1

# (disp, gamma, s, E0, labels, B, h, w, H, W, L) -> status
FORWARD = [
    # L < 2, a size below 1, a negative B (checked before anything else)
    ((D, GA, S, E, LAB, 1, 3, 4, 7, 13, 1), INVALID),
    ((D, GA, S, E, LAB, 1, 3, 4, 7, 13, 0), INVALID),
    ((D, GA, S, E, LAB, 1, 3, 4, 7, 13, -5), INVALID),
    ((D, GA, S, E, LAB, 1, 0, 4, 7, 13, 18), INVALID),
    ((D, GA, S, E, LAB, 1, 3, 0, 7, 13, 18), INVALID),
    ((D, GA, S, E, LAB, 1, 3, 4, 0, 13, 18), INVALID),
    ((D, GA, S, E, LAB, 1, 3, 4, 7, 0, 18), INVALID),
    ((D, GA, S, E, LAB, 1, 3, 4, 7, -13, 18), INVALID),
    ((D, GA, S, E, LAB, -1, 3, 4, 7, 13, 18), INVALID),
    ((None, None, None, None, None, 0, 3, 4, 7, 13, 1), INVALID),
    # an empty batch: PHL_OK whatever the pointers
    ((None, None, None, None, None, 0, 3, 4, 7, 13, 18), OK),
    ((D, GA, S, D, D, 0, I31, I31, I31, I31, I31), OK),
    # null pointers
    ((None, GA, S, E, LAB, 1, 3, 4, 7, 13, 18), INVALID),
    ((D, None, S, E, LAB, 1, 3, 4, 7, 13, 18), INVALID),
    ((D, GA, None, E, LAB, 1, 3, 4, 7, 13, 18), INVALID),
    ((D, GA, S, None, LAB, 1, 3, 4, 7, 13, 18), INVALID),
    ((D, GA, S, E, None, 1, 3, 4, 7, 13, 18), INVALID),
    # an output that is one of the inputs, or the other output
    ((D, GA, S, D, LAB, 1, 3, 4, 7, 13, 18), INVALID),
    ((D, GA, S, GA, LAB, 1, 3, 4, 7, 13, 18), INVALID),
    ((D, GA, S, S, LAB, 1, 3, 4, 7, 13, 18), INVALID),
    ((D, GA, S, E, E, 1, 3, 4, 7, 13, 18), INVALID),
    ((D, GA, S, E, D, 1, 3, 4, 7, 13, 18), INVALID),
    ((D, GA, S, E, GA, 1, 3, 4, 7, 13, 18), INVALID),
    ((D, GA, S, E, S, 1, 3, 4, 7, 13, 18), INVALID),
    # too many elements: the byte counts leave int64, or the workgroups leave the grid
    ((D, GA, S, E, LAB, I31, 1, 1, I31, I31, I31), TOO_LARGE),
    ((D, GA, S, E, LAB, 1, 1, 1, I31, I31, 2), TOO_LARGE),
    ((D, GA, S, E, LAB, I31, I31, I31, 1, 1, 2), TOO_LARGE),                   # the disparity alone
    ((D, GA, S, E, LAB, 1, 1, 1, 1 << 21, 1 << 20, 2), TOO_LARGE),              # 2^41 pixels: 2^31 workgroups
    ((D, GA, S, E, LAB, 1 << 16, 1, 1, WG, 1 << 15, 2), TOO_LARGE),             # 2^16 images of 2^15 workgroups
]
# (disp, labels, gamma, s, gE0, grad, B, h, w, H, W, L) -> status
GRAD = [
    ((D, LAB, GA, S, GE, GR, 1, 3, 4, 7, 13, 1), INVALID),
    ((D, LAB, GA, S, GE, GR, 1, 3, 4, 7, 13, -1), INVALID),
    ((D, LAB, GA, S, GE, GR, 1, 0, 4, 7, 13, 18), INVALID),
    ((D, LAB, GA, S, GE, GR, 1, 3, -4, 7, 13, 18), INVALID),
    ((D, LAB, GA, S, GE, GR, 1, 3, 4, 0, 13, 18), INVALID),
    ((D, LAB, GA, S, GE, GR, 1, 3, 4, 7, 0, 18), INVALID),
    ((D, LAB, GA, S, GE, GR, -2, 3, 4, 7, 13, 18), INVALID),
    ((None, None, None, None, None, None, 0, 3, 4, 7, 13, 18), OK),
    ((D, LAB, GA, S, GE, D, 0, 3, 4, 7, 13, 2), OK),
    ((None, LAB, GA, S, GE, GR, 1, 3, 4, 7, 13, 18), INVALID),
    ((D, None, GA, S, GE, GR, 1, 3, 4, 7, 13, 18), INVALID),
    ((D, LAB, None, S, GE, GR, 1, 3, 4, 7, 13, 18), INVALID),
    ((D, LAB, GA, None, GE, GR, 1, 3, 4, 7, 13, 18), INVALID),
    ((D, LAB, GA, S, None, GR, 1, 3, 4, 7, 13, 18), INVALID),
    ((D, LAB, GA, S, GE, None, 1, 3, 4, 7, 13, 18), INVALID),
    ((D, LAB, GA, S, GE, D, 1, 3, 4, 7, 13, 18), INVALID),
    ((D, LAB, GA, S, GE, LAB, 1, 3, 4, 7, 13, 18), INVALID),
    ((D, LAB, GA, S, GE, GA, 1, 3, 4, 7, 13, 18), INVALID),
    ((D, LAB, GA, S, GE, S, 1, 3, 4, 7, 13, 18), INVALID),
    ((D, LAB, GA, S, GE, GE, 1, 3, 4, 7, 13, 18), INVALID),
    ((D, LAB, GA, S, GE, GR, I31, 1, 1, I31, I31, I31), TOO_LARGE),
    ((D, LAB, GA, S, GE, GR, I31, I31, I31, 1, 1, 2), TOO_LARGE),
    ((D, LAB, GA, S, GE, GR, 1, 1, 1, 1 << 21, 1 << 20, 2), TOO_LARGE),
    ((D, LAB, GA, S, GE, GR, 1 << 16, 1, 1, WG, 1 << 15, 2), TOO_LARGE),
]


def _check(name, args, status):
    import phl

    lib = phl.load_library()
    assert getattr(lib, name)(*args, 10.0, 1e-2, None) == status
    if status != OK:
        text = lib.phl_last_error().decode()
        assert text.startswith(name + ":"), text


@pytest.mark.parametrize("args,status", FORWARD, ids=[f"{i}-{c[1]}" for i, c in enumerate(FORWARD)])
def test_scalar_unaries_argument_checks(args, status):
    _check("phl_nchw_scalar_unaries", args, status)


@pytest.mark.parametrize("args,status", GRAD, ids=[f"{i}-{c[1]}" for i, c in enumerate(GRAD)])
def test_scalar_unaries_grad_argument_checks(args, status):
    _check("phl_nchw_scalar_unaries_grad", args, status)


def test_binding_checks_need_no_gpu():
    """What the binding refuses before it reaches the library."""
    import phl

    disp, one = torch.zeros(1, 1, 3, 4), torch.zeros(())
    with pytest.raises(TypeError):
        phl.nchw_scalar_unaries(disp, (7, 13), 18, one, one)                 # CPU tensors
    with pytest.raises(TypeError):
        phl.nchw_scalar_unaries_fn(disp, (7, 13), 18, one.clone().requires_grad_(), one)
    with pytest.raises(TypeError):
        phl.nchw_scalar_unaries_grad(disp, (7, 13), torch.zeros(18), one, one, torch.zeros(1, 18, 7, 13))
    assert phl.NCHW_SCALAR_PIXELS == WG
    assert issubclass(phl.NchwScalarUnaries, torch.autograd.Function)


def test_the_heads_routing_predicate_off_the_gpu(monkeypatch):
    """False for everything that is not a fp32 CUDA disparity without a gradient in front of a charb -- and for that too
    with the switch off.  Without a GPU a stand-in carries what the predicate reads of a CUDA tensor, so that the one
    routed case is seen too, and the switch, the dtype, the gradient and the Mu are seen to be what turns it down."""
    from crf import mb_stereo_crf as heads
    from crf.crf_module import charb, potts

    route, mu = heads._scalar_unaries_routable, charb(.05)
    disp = torch.rand(1, 1, 3, 4)
    assert heads._SCALAR_UNARIES is True                                      # the default: on
    assert not route(disp, mu)                                                # CPU
    assert not route(disp.double(), mu)
    assert not route(disp.clone().requires_grad_(), mu)
    assert not route(disp, potts(18))
    assert not route(disp[0], mu) and not route(disp.expand(1, 2, 3, 4), mu) and not route(None, mu)

    class OnDevice:
        """What the predicate reads of a tensor, with is_cuda set."""
        def __init__(self, dtype=torch.float32, shape=(1, 1, 3, 4), requires_grad=False, device="cuda:0"):
            self.dtype, self.shape, self.requires_grad, self.device, self.is_cuda = dtype, shape, requires_grad, device, True

        def dim(self):
            return len(self.shape)

        def numel(self):
            n = 1
            for v in self.shape:
                n *= v
            return n

    monkeypatch.setattr(torch, "is_tensor", lambda t: isinstance(t, (torch.Tensor, OnDevice)))
    monkeypatch.setattr(mu, "_parameters", {"gamma": OnDevice(shape=()), "s": OnDevice(shape=())})
    assert route(OnDevice(), mu)                                              # the one case that is routed
    assert not route(OnDevice(dtype=torch.float64), mu)
    assert not route(OnDevice(requires_grad=True), mu)
    assert not route(OnDevice(shape=(0, 1, 3, 4)), mu)
    assert not route(OnDevice(shape=(1, 2, 3, 4)), mu)
    assert not route(OnDevice(), potts(18))
    assert not route(OnDevice(device="cuda:1"), mu)                           # Mu lives elsewhere
    monkeypatch.setattr(heads, "_SCALAR_UNARIES", False)
    assert not route(OnDevice(), mu)                                          # the switch


@pytest.mark.parametrize("kwargs", [dict(niters=2, r=2), dict(niters=0, r=2), dict(niters=1, r=3, gchannels=3)])
def test_energies_are_the_negated_logits_on_the_cpu(kwargs):
    from crf.crf_module import CRFasRNN, charb

    g = torch.Generator().manual_seed(11)
    L, H, W = 6, 9, 11
    net = CRFasRNN(charb(3.0), **kwargs)
    refs = torch.rand((2, kwargs.get("gchannels", 1), H, W), generator=g)
    E = torch.rand((2, L, H, W), generator=g) * 8
    labels, values = torch.linspace(0, 7.5, L), torch.rand((L,), generator=g) * 5 - 1
    with torch.no_grad():
        for lab in (None, labels):
            assert torch.equal(net(refs, None, energies=E, labels=lab), net(refs, -E, labels=lab))
            assert torch.equal(net(refs, None, None, lab, E), net(refs, -E, None, lab))
            for val in (None, values, values[None, :, None, None]):
                got = net.expected_depth(refs, None, energies=E, labels=lab, values=val)
                assert got.shape == (2, 1, H, W) and torch.equal(got, net.expected_depth(refs, -E, labels=lab, values=val))
    # under autograd: the gradient arrives at the energies
    leaf = E.clone().requires_grad_()
    net.expected_depth(refs, None, energies=leaf, labels=labels, values=labels).sum().backward()
    assert leaf.grad is not None and torch.isfinite(leaf.grad).all()
    # E0 itself leaves no room for logits or a confidence
    conf = torch.ones((2, 1, H, W))
    for call in (net, net.expected_depth):
        with pytest.raises(ValueError):
            call(refs, -E, energies=E)
        with pytest.raises(ValueError):
            call(refs, None, conf, energies=E)
        with pytest.raises(ValueError):
            call(refs, -E, conf, energies=E)
