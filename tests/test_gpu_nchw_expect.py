"""The expected-label head on the GPU: phl.nchw_expected_value / phl.nchw_expected_value_grad (phl_nchw_expect.hip),
phl.NchwExpectedValue, and the surface built on them (logits2average_depth, CRFasRNN.expected_depth, the three heads).

Accuracy rule, forward and backward alike: the yardstick is the float64 torch transcription
``(softmax(sign * (X + G), 1) * labels).sum(1)`` on the same inputs (its autograd for the backward); with
err_hip = max|hip - f64| and err_t32 = max|the same transcription in fp32 on the GPU - f64| over all elements,
err_hip <= 2 * err_t32, and err_hip == 0 where err_t32 == 0.  No absolute tolerance.  Every pair of errors is printed; the
largest of each per test is printed last."""
import pytest
import torch
import torch.nn.functional as F

import _guided_util
from _nchw_util import binding_spy, old_loop

DEV = _guided_util.DEV
pytestmark = pytest.mark.gpu

LS = [1, 2, 7, 8, 9, 18, 33, 257, 1030]      # below, at and above the eight-plane block; above every limit of the step kernels
BS = [1, 3]


def _sizes():
    """5x7: dwords, less than a workgroup; 6x6: float4; one float4 above a workgroup's pixels (float4, two workgroups),
    three pixels above (dwords, two workgroups) and one pixel below (dwords, every pixel slot of a thread used)."""
    import phl

    wg = phl.NCHW_EXPECT_PIXELS
    return [(5, 7), (6, 6), (1, wg + 4), (1, wg + 3), (1, wg - 1)]


def _label_sets(L, gen):
    return {"none": None,
            "linspace": torch.linspace(0, 40, L, device=DEV),
            "unsorted": torch.randn((L,), device=DEV, generator=gen) * 50}


def _lab4(labels, L, dtype):
    if labels is None:
        labels = torch.arange(L, dtype=torch.float32, device=DEV)
    return labels.to(dtype)[None, :, None, None]


def _transcription(X, G, labels, negate, dtype):
    """(softmax(sign * (X + G), 1) * labels).sum(1) in ``dtype``, [B, 1, H, W]."""
    z = X.to(dtype) if G is None else X.to(dtype) + G.to(dtype)
    return (F.softmax(-z if negate else z, 1) * _lab4(labels, X.shape[1], dtype)).sum(1, keepdim=True)


class _Worst:
    def __init__(self):
        self.hip = self.t32 = 0.0

    def judge(self, name, hip, t32, want):
        e_hip, e_t32 = float((hip.double() - want).abs().max()), float((t32.double() - want).abs().max())
        print(f"{name}: err_hip = {e_hip:.3e}  err_t32 = {e_t32:.3e}  |want| <= {float(want.abs().max()):.4g}")
        self.hip, self.t32 = max(self.hip, e_hip), max(self.t32, e_t32)
        assert hip.shape == want.shape and torch.isfinite(hip).all(), name
        if e_t32 == 0:
            assert e_hip == 0, (name, e_hip)
        else:
            assert e_hip <= 2 * e_t32, (name, e_hip, e_t32)

    def report(self, what):
        print(f"largest {what}: err_hip = {self.hip:.3e}  err_t32 = {self.t32:.3e}")


def _uniform(shape, gen):
    return torch.rand(shape, device=DEV, generator=gen) * 60 - 30


def _forward_case(worst, name, X, G, labels, negate):
    import phl

    hip = phl.nchw_expected_value(X, G, labels, negate=negate)
    worst.judge(name, hip, _transcription(X, G, labels, negate, torch.float32), _transcription(X, G, labels, negate, torch.float64))
    return hip


@pytest.mark.parametrize("L", LS)
def test_forward_against_float64(L):
    worst = _Worst()
    for H, W in _sizes():
        for B in BS:
            gen = torch.Generator(device=DEV).manual_seed(1000 * L + 10 * H + B)
            X, G0 = _uniform((B, L, H, W), gen), torch.randn((B, L, H, W), device=DEV, generator=gen) * 5
            for lname, labels in _label_sets(L, gen).items():
                for G in (None, G0):
                    for negate in (False, True):
                        name = f"L{L} B{B} {H}x{W} labels={lname} G={'yes' if G is not None else 'no'} negate={negate}"
                        _forward_case(worst, name, X, G, labels, negate)
    worst.report(f"forward L={L}")


@pytest.mark.parametrize("L", LS)
def test_forward_column_patterns(L):
    """Sorted columns (the maximum arrives last / first: the rescale runs in every block or never), constant columns
    (mean(labels)), one entry 200 above the rest (that label), a single label (labels[0] exactly)."""
    import phl

    worst = _Worst()
    for H, W in _sizes()[:3]:
        gen = torch.Generator(device=DEV).manual_seed(77 * L + W)
        X = _uniform((2, L, H, W), gen)
        up, down = X.sort(dim=1).values, X.sort(dim=1, descending=True).values
        for lname, labels in _label_sets(L, gen).items():
            lab = _lab4(labels, L, torch.float32).reshape(L)
            for negate in (False, True):
                tag = f"L{L} {H}x{W} labels={lname} negate={negate}"
                _forward_case(worst, tag + " ascending", up, None, labels, negate)
                _forward_case(worst, tag + " descending", down, None, labels, negate)
                const = torch.full((2, L, H, W), 12.5, device=DEV) * torch.tensor([1.0, -3.0], device=DEV)[:, None, None, None]
                hip = _forward_case(worst, tag + " constant", const, None, labels, negate)
                mean = float(lab.double().mean())
                assert float((hip.double() - mean).abs().max()) <= 4e-7 * max(1.0, float(lab.abs().max())), tag   # fp32 spacing
                k = torch.randint(0, L, (2, 1, H, W), device=DEV, generator=gen)
                peak = (torch.rand((2, L, H, W), device=DEV, generator=gen) * 10).scatter_add_(
                    1, k, torch.full((2, 1, H, W), 210.0, device=DEV))
                hip = _forward_case(worst, tag + " peaked", -peak if negate else peak, None, labels, negate)
                assert torch.equal(hip, lab[k.reshape(2, H, W)][:, None]), tag
        if L == 1:
            for labels in (None, torch.tensor([-7.25], device=DEV)):
                hip = phl.nchw_expected_value(X, None, labels)
                assert torch.equal(hip, torch.full_like(hip, 0.0 if labels is None else -7.25))
    worst.report(f"patterns L={L}")


def test_forward_off_the_16_byte_grid_and_other_layouts():
    """A base pointer one element off the 16-byte grid with n % 4 == 0 takes the dword path: the same arithmetic in the
    same order, so the same bits as the aligned call.  3-D input, ``out``, permuted views, label shapes."""
    import phl

    B, L, H, W = 3, 18, 6, 6
    gen = torch.Generator(device=DEV).manual_seed(5)
    X, G = _uniform((B, L, H, W), gen), torch.randn((B, L, H, W), device=DEV, generator=gen) * 5
    labels = torch.linspace(0, 40, L, device=DEV)
    want = phl.nchw_expected_value(X, G, labels, negate=True)

    def shifted(t):
        buf = torch.zeros((t.numel() + 5,), device=DEV)
        v = buf[1:1 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        return v

    assert torch.equal(phl.nchw_expected_value(shifted(X), G, labels, negate=True), want)
    assert torch.equal(phl.nchw_expected_value(X, shifted(G), labels, negate=True), want)
    out = shifted(torch.full((B, 1, H, W), float("nan"), device=DEV))
    assert phl.nchw_expected_value(X, G, labels, negate=True, out=out) is out and torch.equal(out, want)
    g = torch.randn((B, 1, H, W), device=DEV, generator=gen)
    gz = phl.nchw_expected_value_grad(X, G, labels, g, negate=True)
    assert torch.equal(phl.nchw_expected_value_grad(shifted(X), shifted(G), labels, shifted(g), negate=True), gz)
    # [B, L, n]; [1, L, 1, 1] labels and labels of another dtype; inputs that are not contiguous
    flat = phl.nchw_expected_value(X.reshape(B, L, H * W), G.reshape(B, L, H * W), labels[None, :, None, None], negate=True)
    assert flat.shape == (B, 1, H * W) and torch.equal(flat.reshape(B, 1, H, W), want)
    assert torch.equal(phl.nchw_expected_value(X, G, labels.double().cpu(), negate=True), want)
    Xp = X.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not Xp.is_contiguous() and torch.equal(phl.nchw_expected_value(Xp, G, labels, negate=True), want)
    assert phl.nchw_expected_value(torch.zeros((2, 5, 0, 3), device=DEV)).shape == (2, 1, 0, 3)
    with pytest.raises(ValueError):
        phl.nchw_expected_value(X, G, torch.rand((1, L, H, W), device=DEV))          # labels per pixel
    with pytest.raises(ValueError):
        phl.nchw_expected_value(X, G[:, :, :3])
    with pytest.raises(TypeError):
        phl.nchw_expected_value(X.double())
    with pytest.raises(TypeError):
        phl.nchw_expected_value(X, out=out[..., ::2])
    with pytest.raises(phl.PhlError) as e:
        phl.nchw_expected_value(X.reshape(B * L, 1, H, W), out=X.reshape(B * L, 1, H, W))
    assert e.value.status == 1


def _autograd(X, G, labels, negate, g, dtype):
    x = X.detach().to(dtype).requires_grad_()
    gg = None if G is None else G.detach().to(dtype)
    (_transcription(x, gg, labels, negate, dtype) * g.to(dtype)).sum().backward()
    return x.grad


@pytest.mark.parametrize("L", LS)
def test_backward_against_float64(L):
    import phl

    worst = _Worst()
    for H, W in _sizes():
        for B in (BS if L < 1030 else [1]):
            gen = torch.Generator(device=DEV).manual_seed(2000 * L + 10 * H + B)
            X, G0 = _uniform((B, L, H, W), gen), torch.randn((B, L, H, W), device=DEV, generator=gen) * 5
            g = torch.randn((B, 1, H, W), device=DEV, generator=gen)
            for lname, labels in _label_sets(L, gen).items():
                for G in (None, G0):
                    for negate in (False, True):
                        name = f"grad L{L} B{B} {H}x{W} labels={lname} G={'yes' if G is not None else 'no'} negate={negate}"
                        hip = phl.nchw_expected_value_grad(X, G, labels, g, negate=negate)
                        worst.judge(name, hip, _autograd(X, G, labels, negate, g, torch.float32),
                                    _autograd(X, G, labels, negate, g, torch.float64))
                        if L == 1:
                            assert torch.equal(hip, torch.zeros_like(hip)), name
    worst.report(f"backward L={L}")


def test_both_entry_points_repeat_their_bits():
    import phl

    for L, (H, W) in ((18, (5, 7)), (33, (6, 6)), (257, (1, phl.NCHW_EXPECT_PIXELS + 4))):
        gen = torch.Generator(device=DEV).manual_seed(L)
        X, G = _uniform((3, L, H, W), gen), torch.randn((3, L, H, W), device=DEV, generator=gen) * 5
        g = torch.randn((3, 1, H, W), device=DEV, generator=gen)
        labels = torch.randn((L,), device=DEV, generator=gen) * 50
        assert torch.equal(phl.nchw_expected_value(X, G, labels, negate=True), phl.nchw_expected_value(X, G, labels, negate=True))
        assert torch.equal(phl.nchw_expected_value_grad(X, G, labels, g, negate=True),
                           phl.nchw_expected_value_grad(X, G, labels, g, negate=True))


def _binding_spy():
    """Calls of the binding: (name, negate) of nchw_expected_value / _fn / _grad, and of nchw_softmax_compat(logits=True)."""
    def negate(name, at=None):
        return lambda a, kw: (name, bool(a[at]) if at is not None and len(a) > at else bool(kw.get("negate", False)))

    return binding_spy({"nchw_expected_value": negate("nchw_expected_value"),
                        "nchw_expected_value_fn": negate("nchw_expected_value_fn", at=3),
                        "nchw_expected_value_grad": negate("nchw_expected_value_grad"),
                        "nchw_softmax_compat": lambda a, kw: ("logits", None) if kw.get("logits") else None})


def test_autograd_function():
    import phl

    B, L, H, W = 2, 9, 5, 7
    gen = torch.Generator(device=DEV).manual_seed(9)
    X, G = _uniform((B, L, H, W), gen), torch.randn((B, L, H, W), device=DEV, generator=gen) * 5
    labels, g = torch.linspace(0, 40, L, device=DEV), torch.randn((B, 1, H, W), device=DEV, generator=gen)
    want = phl.nchw_expected_value_grad(X, G, labels, g, negate=True)
    x, gg = X.clone().requires_grad_(), G.clone().requires_grad_()
    with _binding_spy() as seen:
        out = phl.nchw_expected_value_fn(x, gg, labels, True)
        assert torch.equal(out.detach(), phl.nchw_expected_value(X, G, labels, negate=True))
        out.backward(g)
    assert [k for k, _ in seen].count("nchw_expected_value_grad") == 1
    assert torch.equal(x.grad, want) and torch.equal(gg.grad, want)                 # X and G: the same gradient
    x2 = X.clone().requires_grad_()
    phl.NchwExpectedValue.apply(x2, G, labels, True).backward(g)                     # only X asks
    assert torch.equal(x2.grad, want)
    g2 = G.clone().requires_grad_()
    phl.NchwExpectedValue.apply(X, g2, labels[None, :, None, None], True).backward(g)
    assert torch.equal(g2.grad, want)
    with _binding_spy() as seen:                                                     # neither asks: nothing is computed
        out = phl.nchw_expected_value_fn(X, G, labels, True)
        assert not out.requires_grad
        (out * x.detach().requires_grad_().sum()).sum().backward()
    assert "nchw_expected_value_grad" not in [k for k, _ in seen]


# ---- the surface ------------------------------------------------------------------------------------------------------
def _head(kind, gen):
    """(head, inputs) of a small call of each head of crf/mb_stereo_crf.py.  The modules draw their parameters from the
    global generator: it is seeded here, so that a test computes the same numbers whatever ran before it."""
    from crf import mb_stereo_crf as heads

    torch.manual_seed(31)
    if kind == "upsampler":
        net = heads.CRFdepthUpsampler(r=4, niters=2).to(DEV)
        low = torch.rand((1, 1, 24, 20), device=DEV, generator=gen) * 30 + 1
        low[:, :, 5:11, 3:9] = 0                                                  # a hole: confidence 0 there
        return net, (low, torch.rand((1, 3, 48, 40), device=DEV, generator=gen), None)
    cls = heads.CRFdepthRefiner if kind == "refiner" else heads.CRFwUncertainty
    net = cls(d_in=8, d_guide=6, r=4, niters=2).to(DEV)
    logits = torch.randn((2, 12, 30, 37), device=DEV, generator=gen) * 3
    return net, (logits, torch.rand((2, 3, 30, 37), device=DEV, generator=gen), torch.rand((2, 8, 30, 37), device=DEV, generator=gen))


def _head_call(net, inputs):
    """(what the head returns, the operands it handed CRFasRNN.expected_depth) of one call."""
    got, real = [], net.CRF.expected_depth

    def capture(*a, **kw):
        got.append((a, kw))
        return real(*a, **kw)

    net.CRF.expected_depth = capture
    try:
        out = net(inputs)
    finally:
        del net.CRF.expected_depth
    (a, kw), = got
    return out, a, kw


def _expected_depth_f64(net, a, kw):
    """CRFasRNN.expected_depth in float64 on the operands the head's fp32 prologue made (charb's own default labels are
    fp32: the same values are handed over in float64)."""
    dbl = lambda t: t.detach().double() if torch.is_tensor(t) else t      # noqa: E731
    kw = {k: dbl(t) for k, t in kw.items()}
    if len(a) < 4 and kw.get("labels") is None:
        kw["labels"] = torch.arange(a[1].shape[1], dtype=torch.float64, device=a[1].device)
    net.CRF.double()
    try:
        return net.CRF.expected_depth(*[dbl(t) for t in a], **kw)
    finally:
        net.CRF.float()


@pytest.mark.parametrize("kind", ["upsampler", "refiner", "uncertainty"])
def test_heads_end_in_the_kernel(kind):
    gen = torch.Generator(device=DEV).manual_seed(31)
    net, inputs = _head(kind, gen)
    first = (lambda r: r[0]) if kind == "uncertainty" else (lambda r: r)
    with torch.no_grad():
        with _binding_spy() as seen:
            out, a, kw = _head_call(net, inputs)
        new = first(out)
        assert seen == [("nchw_expected_value", True)], seen                      # once, on E0 and G; the logits never written
        values = kw.get("values")
        mid = _transcription(net.CRF(*a, **{k: v for k, v in kw.items() if k != "values"}), None, values, False, torch.float32)
        with old_loop(), _binding_spy() as seen:                                  # the same operands on the torch form
            old = net.CRF.expected_depth(*a, **kw)
            want = _expected_depth_f64(net, a, kw)
            assert torch.equal(first(net(inputs)), old)                           # ... which is what the head then gives
        assert seen == [], seen
    assert new.shape == old.shape == (inputs[1].shape[0], 1) + tuple(inputs[1].shape[2:])
    if kind == "upsampler":
        conf = F.interpolate(inputs[0], size=inputs[1].shape[2:], mode="bilinear", align_corners=False) > 1e-2
        assert 0 < float(conf.float().mean()) < 1
    e_new, e_old = float((new.double() - want).abs().max()), float((old.double() - want).abs().max())
    e_mid = float((mid.double() - want).abs().max())          # the fused loop's logits, then the torch lines: the loop's share
    print(f"{kind}: e_new = {e_new:.3e}  e_old = {e_old:.3e}  (fused loop + torch lines: {e_mid:.3e})  "
          f"|depth| <= {float(want.abs().max()):.4g}")
    assert torch.isfinite(new).all() and e_new <= 2 * e_old, (kind, e_new, e_old)


def test_head_under_autograd():
    """Logits that ask for a gradient: forward's plain loop, then phl.NchwExpectedValue, and a gradient for the logits."""
    gen = torch.Generator(device=DEV).manual_seed(33)
    net, (logits, rgb, feats) = _head("refiner", gen)
    g = torch.randn((2, 1, 30, 37), device=DEV, generator=gen)

    def grad_of(dtype):
        leaf = logits.detach().to(dtype).requires_grad_()
        if dtype == torch.float64:
            with torch.no_grad():
                guide = net._guide(rgb, feats).double()
            net.CRF.double()
            try:
                out = net.CRF.expected_depth(guide, leaf, labels=torch.arange(12, dtype=torch.float64, device=DEV))
            finally:
                net.CRF.float()
        else:
            out = net((leaf, rgb, feats))
        out.backward(g.to(dtype))
        return out.detach(), leaf.grad

    with _binding_spy() as seen:
        out_new, new = grad_of(torch.float32)
    assert seen == [("nchw_expected_value_fn", False), ("nchw_expected_value", False), ("nchw_expected_value_grad", False)], seen
    with old_loop(), _binding_spy() as seen:
        out_old, old = grad_of(torch.float32)
        out_want, want = grad_of(torch.float64)
    assert seen == [], seen
    for what, a, b, c in (("depth", out_new, out_old, out_want), ("grad", new, old, want)):
        e_new, e_old = float((a.double() - c).abs().max()), float((b.double() - c).abs().max())
        print(f"refiner under autograd, {what}: e_new = {e_new:.3e}  e_old = {e_old:.3e}  |{what}| <= {float(c.abs().max()):.4g}")
        assert torch.isfinite(a).all() and e_new <= 2 * e_old, (what, e_new, e_old)


def test_what_never_reaches_the_binding():
    from crf.mb_stereo_crf import logits2average_depth

    def formula(logits, labels=None):
        probs = F.softmax(logits, dim=1)
        if labels is None:
            labels = torch.arange(probs.shape[1], dtype=torch.float32, device=probs.device)[None, :, None, None]
        return (probs * labels).sum(1, keepdim=True)

    gen = torch.Generator(device=DEV).manual_seed(35)
    logits = _uniform((2, 7, 5, 6), gen)
    per_channel = torch.rand((1, 7, 1, 1), device=DEV, generator=gen) * 9
    per_pixel = torch.rand((2, 7, 5, 6), device=DEV, generator=gen) * 9
    with _binding_spy() as seen:
        for lg, lab in ((logits.cpu(), None), (logits.cpu(), per_channel.cpu()), (logits.double(), None),
                        (logits.double(), per_channel.double()), (logits, per_pixel), (logits, per_channel.double()),
                        (logits, per_channel.clone().requires_grad_())):
            got = logits2average_depth(lg, lab)
            assert torch.equal(got.detach(), formula(lg, lab).detach()), (lg.dtype, lg.device)
        with old_loop():
            assert torch.equal(logits2average_depth(logits, per_channel), formula(logits, per_channel))
    assert seen == [], seen
    with _binding_spy() as seen:                                                    # ... and what does
        a = logits2average_depth(logits)
        b = logits2average_depth(logits, per_channel)
        c = logits2average_depth(logits.clone().requires_grad_(), per_channel.reshape(7, 1, 1))
    assert [k for k, _ in seen] == ["nchw_expected_value", "nchw_expected_value", "nchw_expected_value_fn", "nchw_expected_value"]
    assert a.shape == b.shape == c.shape == (2, 1, 5, 6) and c.requires_grad and torch.equal(b, c.detach())
