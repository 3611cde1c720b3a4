"""The channel-major mean-field step for training (phl.nchw_step_train, phl.nchw_step_train_grad, phl.NchwStepTrain) and
the ``fused_step`` keyword of CRFasRNN and its heads, at most 64 labels.

The kernels compute in float64 between the fp32 loads and the fp32 stores, so the step is judged per element against
float64 torch autograd of ``conv2d(softmax(-(E0 + G), 1), M.t()[..., None, None])`` on the device by a rounding bound, not
against another fp32 evaluation.  With T the sum of the absolute values of the terms of an element's sums:

    |Y  - ref| <= ulp32(ref) + L        * 2^-50 * T + 2^-126        T = sum_a |M[a,c]| Q_a
    |dE - ref| <= ulp32(ref) + (2L + 4) * 2^-50 * T + 2^-126        T = Q_a (sum_b Q_b T_b + T_a), T_a = sum_c |M[a,c]| |gY_c|
    |gM - ref| <= ulp32(ref) + B n      * 2^-50 * T + 2^-126        T = sum over b, p of Q_a |gY_c|

-- the one fp32 rounding of the store with a factor 2 of slack, the N * 2^-53 bound of a double sum with a factor 8, and
flushed subnormals.  The largest error / bound ratio of each group is printed with e_hip and the error of fp32 torch
autograd.  The end-to-end runs follow the loop rule of tests/test_gpu_guided_grad.py: e_new <= 2 e_old against the
float64 run, e_old the plain fp32 autograd loop on the same device."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

from _guided_util import DEV, report
from _nchw_util import binding_spy

pytestmark = pytest.mark.gpu


def _ulp32(ref):
    a = ref.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))).double() - a.double())


def _reference(E0, G, M, gY, dtype=torch.float64):
    """(Y, dE, gM, Q) of the transcription, by torch autograd in ``dtype``; volumes [B, L, n]."""
    e, m = E0.detach().to(dtype).requires_grad_(True), M.detach().to(dtype).requires_grad_(True)
    z = -(e if G is None else e + G.detach().to(dtype))
    Q = F.softmax(z[:, :, None], dim=1)
    Y = F.conv2d(Q, m.t()[..., None, None])[:, :, 0]
    Y.backward(gY.detach().to(dtype))
    return Y.detach(), e.grad, m.grad, Q.detach()[:, :, 0]


def _judge(name, E0, G, M, gY, Y, dE, gM):
    """The three bounds of the header; prints the figures, then asserts."""
    B, L, n = E0.shape
    rY, rE, rM, Q = _reference(E0, G, M, gY)
    tY, tE, tM, _ = _reference(E0, G, M, gY, torch.float32)
    aM, aY = M.double().abs(), gY.double().abs()
    T_Y = torch.einsum("ac,bap->bcp", aM, Q)
    T_t = torch.einsum("ac,bcp->bap", aM, aY)
    T_E = Q * ((Q * T_t).sum(1, keepdim=True) + T_t)
    T_M = torch.einsum("bap,bcp->ac", Q, aY)
    worst = 0.0
    for what, got, ref, t32, T, N in (("Y", Y, rY, tY, T_Y, L), ("dE", dE, rE, tE, T_E, 2 * L + 4), ("gM", gM, rM, tM, T_M, B * n)):
        if got is None:
            continue
        assert got.dtype == torch.float32 and got.shape == ref.shape and torch.isfinite(got).all(), (name, what)
        err = (got.double() - ref).abs()
        bound = _ulp32(ref) + N * 2.0 ** -50 * T + 2.0 ** -126
        ratio = float((err / bound).max())
        u = 2.0 ** -24 * max(float(ref.abs().max()), 1e-300)
        print(f"{name} {what}: e_hip = {float(err.max()):.3e} ({float(err.max()) / u:.2f} u)  e_torch = "
              f"{float((t32.double() - ref).abs().max()) / u:.2f} u  worst error / bound = {ratio:.3f}")
        assert ratio <= 1.0, (name, what, ratio)
        worst = max(worst, ratio)
    return worst


def _case(B, L, n, seed, with_g, offset=False):
    gen = torch.Generator(device=DEV).manual_seed(seed)

    def vol(make):
        if not offset:
            return make(B * L * n).view(B, L, n)
        buf = torch.empty(B * L * n + 1, device=DEV)             # one element into a larger buffer: the dword form
        buf[1:] = make(B * L * n)
        return buf[1:].view(B, L, n)

    E0 = vol(lambda k: torch.rand(k, device=DEV, generator=gen) * 60 - 30)
    G = vol(lambda k: torch.randn(k, device=DEV, generator=gen) * 5) if with_g else None
    gY = vol(lambda k: torch.randn(k, device=DEV, generator=gen))
    M = torch.randn((L, L), device=DEV, generator=gen)            # not symmetric: a transposed product shows
    return E0, G, M, gY


def _run(E0, G, M, gY, **kw):
    import phl

    Y = phl.nchw_step_train(E0, G, M)
    dE, gM = phl.nchw_step_train_grad(E0, G, M, gY, **kw)
    return Y, dE, gM


@pytest.mark.parametrize("L", [1, 2, 3, 17, 18, 32, 33, 63, 64])
def test_step_against_float64(L):
    for n in (1, 63, 64, 65, 130, 256):
        for B in (1, 3):
            for with_g in (True, False):
                args = _case(B, L, n, 100 * L + n + B, with_g)
                res = _run(*args)
                _judge(f"L={L} n={n} B={B} G={with_g}", *args, *res)
                if n % 4 == 0:
                    assert all(t.data_ptr() % 16 == 0 for t in args if t is not None)
                    off = _case(B, L, n, 100 * L + n + B, with_g, offset=True)
                    assert off[0].data_ptr() % 16 == 4 and torch.equal(off[0], args[0])
                    res_off = _run(*off)
                    _judge(f"L={L} n={n} B={B} G={with_g} dwords", *off, *res_off)
                    for a, b in zip(res, res_off):               # the access width is all that differs
                        assert torch.equal(a, b)


def test_more_tiles_than_workgroups():
    import phl

    L = 4
    for tiles in (1024, 1025, 2 * 1024 + 3):
        n = 64 * tiles - (8 if tiles == 1025 else 7)                  # a short last tile, float4 and dwords
        R = phl.nchw_step_train_partials(1, L, n)
        assert R == 1024 and tiles in (R, R + 1, 2 * R + 3)
        args = _case(1, L, n, tiles, True)
        _judge(f"tiles={tiles} R={R}", *args, *_run(*args))


def test_extremes():
    import phl

    B, L, n = 2, 18, 130
    gen = torch.Generator(device=DEV).manual_seed(5)
    _, _, M, gY = _case(B, L, n, 6, False)
    E0 = (torch.randint(0, 2, (B, L, n), device=DEV, generator=gen).float() * 200 - 100)
    E0[:, :, 7] = 100.0
    E0[:, 5, 7] = -100.0                                         # one label 200 below the rest
    G = torch.zeros_like(E0)
    G[0, 3, 9] = -100.0                                          # ... and through G: -200 in all
    for g in (None, G):
        Y, dE, gM = _run(E0, g, M, gY)
        _judge(f"extremes G={g is not None}", E0, g, M, gY, Y, dE, gM)
    assert torch.equal(Y[:, :, 7], M[5][None].expand(B, L))       # Q is one-hot there: Y is row 5 of M
    dE, gM = phl.nchw_step_train_grad(E0, G, M, torch.zeros_like(gY))
    assert torch.equal(dE, torch.zeros_like(dE)) and torch.equal(gM, torch.zeros_like(gM))


def test_deterministic_and_partial_requests():
    import phl

    args = _case(3, 33, 1000, 7, True)
    Y, dE, gM = _run(*args)
    Y2, dE2, gM2 = _run(*args)
    assert torch.equal(Y, Y2) and torch.equal(dE, dE2) and torch.equal(gM, gM2)
    e_only = phl.nchw_step_train_grad(*args, need_mu=False)
    m_only = phl.nchw_step_train_grad(*args, need_e=False)
    assert e_only[1] is None and torch.equal(e_only[0], dE)
    assert m_only[0] is None and torch.equal(m_only[1], gM)
    out = torch.empty_like(Y)
    assert phl.nchw_step_train(*args[:3], out=out) is out and torch.equal(out, Y)
    nc = args[3].transpose(0, 1).contiguous().transpose(0, 1)      # gY that is not contiguous
    assert not nc.is_contiguous() and torch.equal(phl.nchw_step_train_grad(*args[:3], nc)[0], dE)
    big = _case(1, 65, 64, 8, True)
    for call in (lambda: phl.nchw_step_train(*big[:3]), lambda: phl.nchw_step_train_grad(*big)):
        with pytest.raises(phl.PhlError) as err:
            call()
        assert err.value.status == 7


@contextlib.contextmanager
def _spy():
    """Counts of phl.nchw_step_train ("step"), phl.nchw_step_train_grad ("grad", with its (need_e, need_mu) in "parts"),
    charb.forward ("charb") and F.softmax ("softmax")."""
    from crf import crf_module

    calls = {"step": 0, "grad": 0, "charb": 0, "softmax": 0, "parts": []}
    real = {"charb": crf_module.charb.forward, "softmax": F.softmax}

    def grad(a, k):
        calls["grad"] += 1
        calls["parts"].append((k["need_e"], k["need_mu"]))

    def charb_forward(*a, **k):
        calls["charb"] += 1
        return real["charb"](*a, **k)

    def softmax(*a, **k):
        calls["softmax"] += 1
        return real["softmax"](*a, **k)

    crf_module.charb.forward, F.softmax = charb_forward, softmax
    try:
        with binding_spy({"nchw_step_train": lambda a, k: calls.update(step=calls["step"] + 1), "nchw_step_train_grad": grad}):
            yield calls
    finally:
        crf_module.charb.forward, F.softmax = real["charb"], real["softmax"]


def test_function_saves_its_inputs_and_honours_needs_input_grad():
    import phl
    from crf.crf_module import CRFasRNN, charb

    E0, G, M, gY = (t.view(2, 18, 5, 26) if t.dim() == 3 else t for t in _case(2, 18, 130, 9, True))
    rY, rE, rM, _ = _reference(E0.view(2, 18, 130), G.view(2, 18, 130), M, gY.view(2, 18, 130))
    with _spy() as calls:
        for ne, ng, nm in ((True, False, False), (False, None, True), (False, True, True), (True, True, True)):
            e, m = E0.clone().requires_grad_(ne), M.clone().requires_grad_(nm)
            g = None if ng is None else G.clone().requires_grad_(ng)
            out = phl.nchw_step_train_fn(e, g, m)
            assert len(out.grad_fn.saved_tensors) == 3
            saved = out.grad_fn.saved_tensors
            assert saved[0].data_ptr() == e.data_ptr() and saved[2].data_ptr() == m.data_ptr()
            (out * gY).sum().backward()
            assert calls["parts"][-1] == (ne or bool(ng), nm)
            assert (e.grad is not None) == ne and (m.grad is not None) == nm and (g is None or (g.grad is not None) == ng)
            if ne and ng:
                assert torch.equal(e.grad, g.grad)
                assert float((e.grad.double().view(2, 18, 130) - rE).abs().max()) <= 2.0 ** -22 * float(rE.abs().max())
                assert float((m.grad.double() - rM).abs().max()) <= 2.0 ** -22 * float(rM.abs().max())
        assert calls["grad"] == 4 and calls["step"] == 4
        # notrain_mu: nothing is asked for M
        net = CRFasRNN(charb(3.0), niters=2, r=2, eps=1e-2, notrain_mu=True, fused_step=True).to(DEV)
        logits = (-E0[:1]).clone().requires_grad_(True)
        net(torch.rand((1, 1, 5, 26), device=DEV), logits).sum().backward()
        assert calls["parts"][4:] == [(True, False)] * 2 and logits.grad is not None and net.Mu.gamma.grad is None


def _train_inputs(L, H, W, seed=10, gchannels=1):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    logits0 = torch.randn((1, L, H, W), device=DEV, generator=gen) * 2
    guide0 = torch.rand((1, gchannels, H, W), device=DEV, generator=gen)
    up = torch.rand((1, L, H, W), device=DEV, generator=gen) * 2 - 1
    return logits0, guide0, up


def _train_step(net, params, inputs, dtype, labels=True):
    """The gradients of logits, guide and ``params(net)`` of one step of sum(net(guide, logits) * up), and the output."""
    logits0, guide0, up = inputs
    L = logits0.shape[1]
    logits, guide = logits0.clone().to(dtype).requires_grad_(True), guide0.clone().to(dtype).requires_grad_(True)
    net.zero_grad(set_to_none=True)
    out = net(guide, logits, labels=torch.arange(L, dtype=dtype, device=DEV) if labels else None)
    (out * up.to(dtype)).sum().backward()
    res = {"logits": logits.grad, "guide": guide.grad}
    res.update({k: p.grad.clone() for k, p in params(net).items() if p.grad is not None})
    return res, out.detach()


def test_route_charb():
    """The inputs of test_gpu_guided_grad.py::test_crfasrnn_trains_on_the_kernels on the new route."""
    from crf.crf_module import CRFasRNN, charb

    niters, L = 3, 16
    inputs = _train_inputs(L, 96, 128)
    params = lambda net: {"gamma": net.Mu.gamma, "s": net.Mu.s, "omega": net.W.omega}       # noqa: E731
    net = CRFasRNN(charb(3.0), niters=niters, fused_grad=True, fused_step=True).to(DEV)
    with _spy() as calls:
        hip, _ = _train_step(net, params, inputs, torch.float32)
    assert (calls["step"], calls["grad"], calls["charb"], calls["softmax"]) == (niters, niters, 0, 0)
    assert calls["parts"] == [(True, True)] * niters
    net.fused_step, net.W.fused_grad = False, False
    with _spy() as calls:
        t32, _ = _train_step(net, params, inputs, torch.float32)
    assert calls["step"] == 0 and calls["grad"] == 0 and calls["charb"] == niters and calls["softmax"] == niters + 1
    want, _ = _train_step(net.double(), params, inputs, torch.float64)
    for k in hip:
        report(f"fused_step charb grad_{k}", hip[k], t32[k], want[k], factor=2, what="grad")


def test_route_potts():
    """A bias-free 1x1 conv as Mu: its weight trains through the step's gM."""
    from crf.crf_module import CRFasRNN, potts

    niters, L = 3, 8
    inputs = _train_inputs(L, 96, 128, seed=11)
    params = lambda net: {"weight": net.Mu.weight, "omega": net.W.omega}                      # noqa: E731
    net = CRFasRNN(potts(L), niters=niters, fused_grad=True, fused_step=True).to(DEV)
    with _spy() as calls:
        hip, _ = _train_step(net, params, inputs, torch.float32, labels=False)
    assert (calls["step"], calls["grad"], calls["softmax"]) == (niters, niters, 0)
    assert hip["weight"].shape == (L, L, 1, 1)
    net.fused_step, net.W.fused_grad = False, False
    with _spy() as calls:
        t32, _ = _train_step(net, params, inputs, torch.float32, labels=False)
    assert calls["step"] == 0 and calls["grad"] == 0 and calls["softmax"] == niters + 1
    want, _ = _train_step(net.double(), params, inputs, torch.float64, labels=False)
    for k in hip:
        report(f"fused_step potts grad_{k}", hip[k], t32[k], want[k], factor=2, what="grad")


def test_route_upsampler():
    """CRFdepthUpsampler(fused_grad=True, fused_step=True), one L1 step: the depth and the gradients of gamma and s.  The
    target lies below every depth, so the L1 loss has no kink between the runs."""
    from crf.mb_stereo_crf import CRFdepthUpsampler

    gen = torch.Generator(device=DEV).manual_seed(12)
    disp = torch.rand((1, 1, 6, 8), device=DEV, generator=gen) * 20 + 1
    img = torch.rand((1, 3, 96, 128), device=DEV, generator=gen)

    def step(net, dtype):
        net.zero_grad(set_to_none=True)
        if dtype == torch.float64:                               # the head's torch lines with every operand float64, the labels too
            up = F.interpolate(disp.double(), size=img.shape[2:], mode="bilinear", align_corners=False)
            labels = torch.linspace(0, float(up.max()), 18, dtype=dtype, device=DEV)
            logits = -10 * net.CRF.Mu.get_energies_from_scalar(up, labels[None, :, None, None])
            depth = net.CRF.expected_depth(img.double(), logits, confidence=(up > 1e-2).double(), labels=labels, values=labels)
        else:
            depth = net((disp, img, None))
        (depth - (-1.0)).abs().mean().backward()
        return {"depth": depth.detach(), "gamma": net.CRF.Mu.gamma.grad.clone(), "s": net.CRF.Mu.s.grad.clone()}

    torch.manual_seed(0)
    net = CRFdepthUpsampler(fused_grad=True, fused_step=True).to(DEV)
    with _spy() as calls:
        hip = step(net, torch.float32)
    assert (calls["step"], calls["grad"], calls["charb"], calls["softmax"]) == (2, 2, 0, 0)
    net.CRF.fused_step, net.CRF.W.fused_grad = False, False
    with _spy() as calls:
        t32 = step(net, torch.float32)
    assert calls["step"] == 0 and calls["grad"] == 0 and calls["charb"] == 2
    want = step(net.double(), torch.float64)
    for k in hip:
        report(f"fused_step upsampler {k}", hip[k], t32[k], want[k], factor=2, what=k)


def test_route_uncertainty():
    """CRFwUncertainty(fused_step=True), 12 labels: the confidence net trains through E0 = -logits * confidence, that is
    through the step's dE.  The rule judges the maximum over all elements, so the net's gradients are taken as one vector
    (a bias of one element alone would compare two single roundings)."""
    from crf.mb_stereo_crf import CRFwUncertainty

    L, H, W = 12, 48, 64
    gen = torch.Generator(device=DEV).manual_seed(13)
    logits = torch.randn((1, L, H, W), device=DEV, generator=gen) * 2
    img = torch.rand((1, 3, H, W), device=DEV, generator=gen)
    feats = torch.randn((1, 64, H, W), device=DEV, generator=gen)
    up = torch.rand((1, 1, H, W), device=DEV, generator=gen) * 2 - 1

    def step(net, dtype):
        net.zero_grad(set_to_none=True)
        if dtype == torch.float64:                               # the head's lines; charb's own default labels are fp32
            confidence = torch.exp(-net.uncertainty_net(img.double()))
            depth = net.CRF.expected_depth(net._guide(img.double(), feats.double()), logits.double(), confidence,
                                           labels=torch.arange(L, dtype=dtype, device=DEV))
        else:
            depth, _ = net((logits, img, feats))
        (depth * up.to(dtype)).sum().backward()
        ps = list(net.uncertainty_net.parameters())
        assert all(p.grad is not None for p in ps)
        return {"depth": depth.detach(), "confidence net": torch.cat([p.grad.reshape(-1) for p in ps]),
                "gamma": net.CRF.Mu.gamma.grad.clone()}

    torch.manual_seed(0)
    net = CRFwUncertainty(fused_step=True).to(DEV)
    with _spy() as calls:
        hip = step(net, torch.float32)
    assert (calls["step"], calls["grad"], calls["charb"], calls["softmax"]) == (2, 2, 0, 0)
    net.CRF.fused_step = False
    with _spy() as calls:
        t32 = step(net, torch.float32)
    assert calls["step"] == 0 and calls["grad"] == 0 and calls["charb"] == 2
    want = step(net.double(), torch.float64)
    assert float(want["confidence net"].abs().max()) > 0
    for k in ("depth", "confidence net"):
        report(f"fused_step uncertainty {k}", hip[k], t32[k], want[k], factor=2, what=k)


def test_declines_keep_their_routes_and_bits():
    from crf.crf_module import CRFasRNN, charb

    def both(make, inputs, grad=True, labels=True):
        res = []
        for flag in (True, False):
            net = make(flag).to(DEV)
            params = lambda net: {"gamma": net.Mu.gamma, "s": net.Mu.s}                      # noqa: E731
            with _spy() as calls:
                if grad:
                    g, out = _train_step(net, params, inputs, torch.float32, labels=labels)
                    assert all(torch.isfinite(v).all() for v in g.values())
                    res.append([out])                            # (torch's own backward does not repeat its bits)
                else:
                    with torch.no_grad():
                        res.append([net(inputs[1], inputs[0])])
            assert calls["step"] == 0 and calls["grad"] == 0
        for a, b in zip(*res):
            assert torch.equal(a, b)

    both(lambda f: CRFasRNN(charb(3.0), niters=2, r=2, eps=1e-2, fused_step=f), _train_inputs(65, 12, 20))       # 65 labels
    both(lambda f: CRFasRNN(charb(3.0), niters=2, lattice=True, fused_step=f), _train_inputs(4, 16, 24, gchannels=3))     # the lattice W
    both(lambda f: CRFasRNN(charb(3.0), niters=2, r=2, eps=1e-2, fused_step=f), _train_inputs(16, 12, 20), grad=False)
