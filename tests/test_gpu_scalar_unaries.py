"""The upsampler head's scalar unaries on the GPU: phl.nchw_scalar_unaries / phl.nchw_scalar_unaries_grad
(phl_nchw_scalar.hip), phl.NchwScalarUnaries, and CRFdepthUpsampler on top of them.

The yardstick is the float64 torch transcription of the head's prologue on the fp32 inputs widened: ``up`` from
F.interpolate in float64, the mask ``up.float() > 1e-2``, ``E0 = scale * exp(s) * (sqrt(g^2 + (labels - up)^2) - g) * mask``
with g = gamma * lmax -- evaluated on the library's own labels, which are checked against a float64 linspace first.  Every
bound is derived (fp32 spacing, the float64 cancellation in r - g, the float64 sums), none is measured; the figures are
printed before they are judged.  Shapes: the smallest that reach each branch of the kernels (see SHAPES)."""
import contextlib
import copy
import math

import pytest
import torch
import torch.nn.functional as F

import _guided_util

DEV = _guided_util.DEV
pytestmark = pytest.mark.gpu

SCALE, THRESHOLD = 10.0, 1e-2
# (B, h, w) -> (H, W), L
SHAPES = [
    ((1, 3, 4), (7, 13), 18),        # n = 91: dwords, one partial tile, non-integer ratios
    ((2, 5, 7), (20, 28), 18),       # n = 560: float4, ratio 4, the maximum placed in image 1
    ((1, 1, 3), (4, 9), 2),          # one source row, the i1 clamp, the smallest L
    ((1, 4, 1), (9, 5), 9),          # one source column, L not a multiple of 8
    ((1, 9, 11), (4, 5), 33),        # shrinking
    ((1, 6, 8), (6, 8), 18),         # identity
    ((2, 6, 5), (33, 37), 18),       # n = 1221: two workgroup tiles, odd n
]
CASES = [(shape, size, L, 0.05) for shape, size, L in SHAPES] + [((2, 5, 7), (20, 28), 18, 1e-3)]   # strong cancellation
IDS = [f"{b}x{h}x{w}-{H}x{W}-L{L}-g{gamma}" for (b, h, w), (H, W), L, gamma in CASES]


def _ulp32(x):
    """The spacing of the fp32 numbers at |x| (float64 tensor in, float64 out)."""
    _, e = torch.frexp(x.abs())
    ulp = torch.ldexp(torch.ones_like(x), (e - 24).clamp(min=-149))
    return torch.where(x == 0, torch.full_like(x, 2.0 ** -149), ulp)


def _inputs(shape, seed, max_in_image=None):
    """Disparities uniform in [0.5, 60] with about 30 % of the pixels exactly 0 (no measurement) -- the first image's
    top-left 2 x 2 among them, so that also the smallest shapes have a pixel whose every source is 0."""
    gen = torch.Generator().manual_seed(seed)
    disp = torch.rand((shape[0], 1) + shape[1:], generator=gen) * 59.5 + 0.5
    disp[torch.rand(disp.shape, generator=gen) < 0.3] = 0
    disp[0, 0, :2, :2] = 0
    if max_in_image is not None:
        disp[max_in_image, 0, 0, 0] = 60.0      # a corner: an enlarging resize samples it with weight 1
    return disp.to(DEV), gen


def _param(v):
    return torch.tensor(v, dtype=torch.float32, device=DEV)


def _up64(disp, size):
    return F.interpolate(disp.double(), size=size, mode="bilinear", align_corners=False)


def _energies64(up, labels, gamma, s):
    """(E0, mask) in float64 from up [B, 1, H, W], labels [L], gamma, s: float64 tensors (gamma and s may be leaves)."""
    c = up.float() > THRESHOLD                                       # torch's own fp32 comparison
    g = gamma * labels[-1]
    r = torch.sqrt(g ** 2 + (labels[None, :, None, None] - up) ** 2)
    return SCALE * torch.exp(s) * (r - g) * c, c


def _torch_prologue32(disp, size, L, gamma, s):
    """The head's torch lines in fp32 (crf/mb_stereo_crf.py): the E0 CRFasRNN forms from them."""
    from crf.crf_module import charbonneir

    up = F.interpolate(disp, size=size, mode="bilinear", align_corners=False)
    labels = torch.linspace(0, float(up.max()), L, device=up.device)
    lab4 = labels[None, :, None, None]
    logits = -10 * (charbonneir(lab4, up, gamma * lab4.max()) * torch.exp(s))
    return -logits * (up > 1e-2).float()


@pytest.fixture(scope="module", params=CASES, ids=IDS)
def case(request):
    """One call of the binding per case and its float64 reference, shared by the tests below and left unchanged."""
    import phl

    shape, size, L, gamma = request.param
    disp, gen = _inputs(shape, 100 + CASES.index(request.param), max_in_image=1 if size == (20, 28) else None)
    gm, s = _param(gamma), _param(0.3)
    E0, labels = phl.nchw_scalar_unaries(disp, size, L, gm, s)
    up = _up64(disp, size)
    # the conditions the bounds below rest on: no sample near the threshold, and both sides of the mask present
    assert float((up - THRESHOLD).abs().min()) >= 1e-4
    want, c = _energies64(up, labels.double(), gm.double(), s.double())
    assert 0 < float(c.float().mean()) < 1
    gE0 = torch.randn(E0.shape, generator=gen).to(DEV)
    return dict(disp=disp, size=size, L=L, gamma=gm, s=s, E0=E0, labels=labels, up=up, want=want, c=c, gE0=gE0)


def test_labels_are_the_linspace_to_the_maximum(case):
    up, labels, L = case["up"], case["labels"], case["L"]
    assert labels.shape == (L,) and labels.dtype == torch.float32
    lmax64 = up.max()
    err = float((labels[-1].double() - lmax64).abs())
    print(f"lmax = {float(labels[-1])!r}  float64 max = {float(lmax64)!r}  |diff| = {err:.3e}  ulp32 = {float(_ulp32(lmax64)):.3e}")
    assert err <= float(_ulp32(lmax64))
    assert float(labels[0]) == 0.0 and math.copysign(1.0, float(labels[0])) == 1.0
    # ... and the others divide [0, lmax] -- the fp32 lmax just checked, as the kernel defines them -- evenly
    lin = torch.linspace(0, float(labels[-1]), L, dtype=torch.float64, device=DEV)
    d = (labels.double() - lin).abs()
    print(f"labels: max |diff to the float64 linspace| / ulp32 = {float((d / _ulp32(lin)).max()):.3f}")
    assert bool((d <= _ulp32(lin)).all())
    if case["size"] == (20, 28):
        assert int(up.flatten(1).max(1).values.argmax()) == 1           # the maximum lies in image 1


def test_energies(case):
    E0, want, c = case["E0"], case["want"], case["c"]
    assert E0.shape == want.shape and E0.dtype == torch.float32 and torch.isfinite(E0).all()
    off = ~c.expand_as(E0)
    assert bool((E0[off].view(torch.int32) == 0).all())                 # +0.0, bit for bit
    k = SCALE * math.exp(float(case["s"].double()))
    floor = 1e-10 * k * float(case["gamma"].double()) * float(case["labels"][-1].double())
    err = (E0.double() - want).abs()
    t32 = _torch_prologue32(case["disp"], case["size"], case["L"], case["gamma"], case["s"])
    worst = float((err / (_ulp32(want) + floor))[~off].max())
    print(f"E0: max err = {float(err.max()):.3e} (fp32 torch form: {float((t32.double() - want).abs().max()):.3e})  "
          f"max err / bound = {worst:.3f}  floor = {floor:.3e}  |E0| <= {float(want.abs().max()):.4g}")
    assert bool((err <= _ulp32(want) + floor)[~off].all())


def test_backward(case):
    import phl

    disp, size, labels, gm, s, gE0 = (case[k] for k in ("disp", "size", "labels", "gamma", "s", "gE0"))
    g64, s64 = gm.double().requires_grad_(), s.double().requires_grad_()
    E, c = _energies64(case["up"], labels.double(), g64, s64)
    (E * gE0.double()).sum().backward()
    with torch.no_grad():                                               # T = sum |terms| of each gradient
        lab, lmax = labels.double()[None, :, None, None], labels[-1].double()
        g = g64 * lmax
        r = torch.sqrt(g ** 2 + (lab - case["up"]) ** 2)
        T_s = float((gE0.double() * E).abs().sum())
        T_g = float((gE0.double() * c * SCALE * torch.exp(s64) * lmax * (g / r - 1)).abs().sum())
    gg, gs = phl.nchw_scalar_unaries_grad(disp, size, labels, gm, s, gE0)
    assert gg.shape == gs.shape == () and gg.dtype == gs.dtype == torch.float32
    for name, got, want, T in (("grad_gamma", gg, g64.grad, T_g), ("grad_s", gs, s64.grad, T_s)):
        err, bound = float((got.double() - want).abs()), float(_ulp32(want)) + 1e-12 * T
        print(f"{name}: got {float(got)!r}  want {float(want)!r}  err = {err:.3e}  bound = {bound:.3e}  T = {T:.4g}")
        assert math.isfinite(float(got)) and err <= bound, (name, err, bound)
    again = phl.nchw_scalar_unaries_grad(disp, size, labels, gm, s, gE0)
    assert torch.equal(torch.stack(again).view(torch.int32), torch.stack((gg, gs)).view(torch.int32))   # the same bits


def test_autograd_function(case):
    import phl

    disp, size, L, gE0 = case["disp"], case["size"], case["L"], case["gE0"]
    gm, s = case["gamma"].clone().requires_grad_(), case["s"].clone().requires_grad_()
    leaf = disp.clone().requires_grad_()
    E0, labels = phl.nchw_scalar_unaries_fn(leaf, size, L, gm, s)
    assert torch.equal(E0.detach().view(torch.int32), case["E0"].view(torch.int32))
    assert torch.equal(labels, case["labels"]) and E0.requires_grad and not labels.requires_grad
    (E0 * gE0).sum().backward()
    gg, gs = phl.nchw_scalar_unaries_grad(disp, size, case["labels"], case["gamma"], case["s"], gE0)
    assert torch.equal(gm.grad, gg) and torch.equal(s.grad, gs) and leaf.grad is None


# ---- the head --------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _switch(on):
    from crf import mb_stereo_crf as heads

    was, heads._SCALAR_UNARIES = heads._SCALAR_UNARIES, on
    try:
        yield
    finally:
        heads._SCALAR_UNARIES = was


@contextlib.contextmanager
def _spy():
    """Names of the scalar-unary calls that reach the binding, in order (the _fn's forward calls the plain one)."""
    import phl

    seen, real = [], {k: getattr(phl, k) for k in ("nchw_scalar_unaries", "nchw_scalar_unaries_fn")}

    def wrap(k):
        def f(*a, **kw):
            seen.append(k)
            return real[k](*a, **kw)
        return f

    for k in real:
        setattr(phl, k, wrap(k))
    try:
        yield seen
    finally:
        for k, v in real.items():
            setattr(phl, k, v)


def _head():
    """The upsampler call of tests/test_gpu_nchw_expect.py (_head("upsampler")): 24 x 20 -> 48 x 40, a hole set to 0."""
    from crf import mb_stereo_crf as heads

    gen = torch.Generator(device=DEV).manual_seed(31)
    torch.manual_seed(31)
    net = heads.CRFdepthUpsampler(r=4, niters=2).to(DEV)
    low = torch.rand((1, 1, 24, 20), device=DEV, generator=gen) * 30 + 1
    low[:, :, 5:11, 3:9] = 0
    return net, (low, torch.rand((1, 3, 48, 40), device=DEV, generator=gen), None)


def _head64(net, inputs):
    """(a float64 copy of the head, its output): the head's torch lines with every operand float64, the labels too."""
    low, img = inputs[0].double(), inputs[1].double()
    net64 = copy.deepcopy(net).double()
    up = F.interpolate(low, size=img.shape[2:], mode="bilinear", align_corners=False)
    labels = torch.linspace(0, float(up.max()), 18, dtype=torch.float64, device=DEV)
    logits = -10 * net64.CRF.Mu.get_energies_from_scalar(up, labels[None, :, None, None])
    return net64, net64.CRF.expected_depth(img, logits, confidence=(up > 1e-2).double(), labels=labels, values=labels)


def _judge(name, new, old, want):
    e_new, e_old = float((new.double() - want).abs().max()), float((old.double() - want).abs().max())
    print(f"{name}: e_new = {e_new:.3e}  e_old = {e_old:.3e}  |{name}| <= {float(want.abs().max()):.4g}")
    assert torch.isfinite(new).all() and e_new <= 2 * e_old, (name, e_new, e_old)


def test_head_without_grad():
    net, inputs = _head()
    with torch.no_grad():
        with _spy() as seen:
            new = net(inputs)
        assert seen == ["nchw_scalar_unaries"], seen
        with _switch(False), _spy() as seen:
            old = net(inputs)
        assert seen == [], seen
        _, want = _head64(net, inputs)
    assert new.shape == old.shape == want.shape == (1, 1, 48, 40)
    _judge("depth", new, old, want)


def test_head_training():
    net, inputs = _head()
    names = [n for n, _ in net.named_parameters()]
    assert "CRF.Mu.gamma" in names and "CRF.Mu.s" in names
    target = torch.rand((1, 1, 48, 40), device=DEV, generator=torch.Generator(device=DEV).manual_seed(37)) * 30

    def grads(module, out):
        (out - target.to(out.dtype)).abs().mean().backward()
        return out.detach(), {n: p.grad.detach().clone() for n, p in module.named_parameters() if p.grad is not None}

    def run():
        net.zero_grad(set_to_none=True)
        return grads(net, net(inputs))

    with _spy() as seen:
        out_new, new = run()
    assert seen == ["nchw_scalar_unaries_fn", "nchw_scalar_unaries"], seen
    with _switch(False), _spy() as seen:
        out_old, old = run()
    assert seen == [], seen
    out_want, want = grads(*_head64(net, inputs))
    assert set(new) == set(old) == set(want) and {"CRF.Mu.gamma", "CRF.Mu.s"} <= set(new)
    _judge("depth", out_new, out_old, out_want)
    for n in sorted(new):
        _judge(n, new[n], old[n], want[n])
    # a disparity that asks for a gradient stays on the torch lines
    low = inputs[0].clone().requires_grad_()
    with _spy() as seen:
        out = net((low, inputs[1], None))
    assert seen == [], seen
    with _switch(False):
        assert torch.equal(out, net((inputs[0].clone().requires_grad_(), inputs[1], None)))
