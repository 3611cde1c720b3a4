"""The confidence-weighted unaries on the GPU: phl.nchw_confidence_unaries / phl.nchw_confidence_unaries_grad
(phl_nchw_conf.hip), phl.NchwConfidenceUnaries, and the ``fused_unaries`` keyword of CRFasRNN under CRFwUncertainty and
CRFdepthUpsampler.

E0 = -logits * confidence and grad_logits = -(confidence * gE0) are one fp32 product each: they are held to the bits of
the torch line and of fp32 autograd.  grad_conf = -sum_a logits_a gE0_a is a float64 sum of exact products in label order,
rounded once, so it is judged per element against float64 by the bound of tests/test_gpu_nchw_train.py with N = L,

    |grad_conf - ref| <= ulp32(ref) + L * 2^-50 * T + 2^-126,        T = sum_a |logits_a gE0_a|

-- derived, not measured; the worst error / bound is printed with fp32 autograd's beside it.  The heads follow the loop
rule (_nchw_util.report_loop): e_new <= 2 e_old against the float64 run."""
import contextlib
import copy

import pytest
import torch
import torch.nn.functional as F

from _guided_util import DEV
from _nchw_util import binding_spy, on_float4_path, report_loop, shifted

pytestmark = pytest.mark.gpu

# (B, L, H, W): n = H * W
SHAPES = [
    (1, 1, 1, 1),
    (2, 3, 1, 3),
    (1, 9, 5, 51),       # n = 255
    (3, 8, 32, 32),      # n = 1024: one full tile, float4
    (1, 17, 25, 41),     # n = 1025: dwords, one pixel in a second tile
    (2, 7, 4, 257),      # n = 1028: float4, the second tile nearly empty
    (1, 64, 3, 347),     # n = 1041
    (1, 231, 2, 6),      # n = 12
]
CASES = [(s, kind, False) for s in SHAPES for kind in ("real", "mask")] + [((2, 7, 4, 257), kind, True) for kind in ("real", "mask")]
IDS = [f"{b}x{l}x{h}x{w}-{kind}{'-shifted' if off else ''}" for (b, l, h, w), kind, off in CASES]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _ulp32(ref):
    a = ref.abs().float()
    return torch.nextafter(a, torch.full_like(a, float("inf"))).double() - a.double()


def _inputs(shape, kind, seed):
    """Logits in [-100, 100] with about a tenth exact zeros of either sign, a confidence in (0, 3] or a 0/1 mask with
    both values present, and a normal upstream gradient with a few zeros."""
    B, L, H, W = shape
    gen = torch.Generator().manual_seed(seed)
    logits = torch.rand(shape, generator=gen) * 200 - 100
    z = torch.rand(shape, generator=gen)
    logits[z < 0.05] = 0.0
    logits[(z >= 0.05) & (z < 0.1)] = -0.0
    if kind == "real":
        conf = 3 - torch.rand((B, 1, H, W), generator=gen) * 2.999
        assert float(conf.min()) > 0 and float(conf.max()) <= 3
    else:
        conf = (torch.rand((B, 1, H, W), generator=gen) < 0.5).float()
        flat = conf.view(-1)
        if flat.numel() > 1:
            flat[0], flat[-1] = 0.0, 1.0                          # both values present
    gE0 = torch.randn(shape, generator=gen)
    gE0[torch.rand(shape, generator=gen) < 0.03] = 0.0
    return logits.to(DEV), conf.to(DEV), gE0.to(DEV)


@pytest.fixture(scope="module", params=CASES, ids=IDS)
def case(request):
    """The inputs of one case and its references, computed once, shared by the tests below and left unchanged: the torch
    line, fp32 autograd, and grad_conf in float64 with its T."""
    shape, kind, off = request.param
    logits, conf, gE0 = _inputs(shape, kind, 300 + CASES.index(request.param))
    if off:
        logits, conf, gE0 = shifted(logits), shifted(conf), shifted(gE0)
        assert not on_float4_path(logits, conf, gE0) and shape[2] * shape[3] % 4 == 0
    lg, cf = logits.clone().requires_grad_(), conf.clone().requires_grad_()
    E0 = -lg * cf
    gl32, gc32 = torch.autograd.grad(E0, (lg, cf), gE0)
    terms = logits.double() * gE0.double()
    return dict(shape=shape, kind=kind, logits=logits, conf=conf, gE0=gE0, E0=E0.detach(), gl32=gl32, gc32=gc32,
                gc64=-terms.sum(1, keepdim=True), T=terms.abs().sum(1, keepdim=True))


def test_forward_is_the_torch_line_bit_for_bit(case):
    import phl

    logits, conf, want = case["logits"], case["conf"], case["E0"]
    B, L, H, W = case["shape"]
    got = phl.nchw_confidence_unaries(logits, conf)
    assert got.shape == want.shape and got.dtype == torch.float32 and got.is_contiguous()
    assert torch.equal(_bits(got), _bits(want))
    if logits.numel() >= 1000:                                       # zeros of either sign came through
        assert bool((_bits(got) == 0).any()) and bool((_bits(got) == -2 ** 31).any())
    out = torch.full_like(want, float("nan"))
    assert phl.nchw_confidence_unaries(logits, conf, out=out) is out and torch.equal(_bits(out), _bits(want))
    flat = phl.nchw_confidence_unaries(logits.reshape(B, L, H * W), conf.reshape(B, 1, H * W))          # [B, L, n]
    assert flat.shape == (B, L, H * W) and torch.equal(_bits(flat), _bits(want.reshape(B, L, H * W)))
    assert torch.equal(_bits(phl.nchw_confidence_unaries(logits, conf)), _bits(got))                    # the same bits again


def test_backward(case):
    import phl

    logits, conf, gE0, L = case["logits"], case["conf"], case["gE0"], case["shape"][1]
    gc, gl = phl.nchw_confidence_unaries_grad(logits, conf, gE0, need_conf=True, need_logits=True)
    assert gc.shape == conf.shape and gl.shape == logits.shape and gc.dtype == gl.dtype == torch.float32
    # grad_logits: the bits of fp32 autograd
    assert torch.equal(_bits(gl), _bits(case["gl32"]))
    # grad_conf: one float64 sum rounded once
    ref, T = case["gc64"], case["T"]
    bound = _ulp32(ref) + L * 2.0 ** -50 * T + 2.0 ** -126
    err, err32 = (gc.double() - ref).abs(), (case["gc32"].double() - ref).abs()
    ratio, ratio32 = float((err / bound).max()), float((err32 / bound).max())
    print(f"grad_conf {case['shape']} {case['kind']}: worst error / bound = {ratio:.3f} (fp32 autograd: {ratio32:.3f})  "
          f"max err = {float(err.max()):.3e} (fp32 autograd: {float(err32.max()):.3e})  |grad_conf| <= {float(ref.abs().max()):.4g}")
    assert torch.isfinite(gc).all() and ratio <= 1.0, ratio
    # a part alone: the default is the confidence's; the shared bits do not depend on the other part
    only_c = phl.nchw_confidence_unaries_grad(logits, conf, gE0)
    assert only_c[1] is None and torch.equal(_bits(only_c[0]), _bits(gc))
    only_l = phl.nchw_confidence_unaries_grad(logits, conf, gE0, need_conf=False, need_logits=True)
    assert only_l[0] is None and torch.equal(_bits(only_l[1]), _bits(gl))
    # two calls: the same bits
    again = phl.nchw_confidence_unaries_grad(logits, conf, gE0, need_conf=True, need_logits=True)
    assert torch.equal(_bits(again[0]), _bits(gc)) and torch.equal(_bits(again[1]), _bits(gl))


def _saved_volumes(make, inputs, numel):
    """The number of tensors of ``numel`` elements autograd saves while ``make()`` runs that are none of ``inputs``."""
    own, seen = {t.data_ptr() for t in inputs}, []

    def pack(t):
        if t.numel() == numel and t.data_ptr() not in own:
            seen.append(tuple(t.shape))
        return t

    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        out = make()
    return out, len(seen)


def test_autograd_function(case):
    import phl

    logits, conf, gE0 = case["logits"], case["conf"], case["gE0"]
    gc, gl = phl.nchw_confidence_unaries_grad(logits, conf, gE0, need_conf=True, need_logits=True)
    for need_l, need_c in ((True, True), (False, True), (True, False)):
        lg, cf = logits.clone().requires_grad_(need_l), conf.clone().requires_grad_(need_c)
        with binding_spy({"nchw_confidence_unaries_grad": lambda a, k: (k["need_conf"], k["need_logits"])}) as parts:
            E0, extra = _saved_volumes(lambda: phl.nchw_confidence_unaries_fn(lg, cf), (lg, cf), logits.numel())
            assert E0.requires_grad and torch.equal(_bits(E0.detach()), _bits(case["E0"]))
            assert extra == 0, extra                                  # the logits and the confidence, nothing else
            got = torch.autograd.grad(E0, [t for t in (lg, cf) if t.requires_grad], gE0)
        assert parts == [(need_c, need_l)], parts                     # one call, for what is asked
        want = [t for t, need in ((gl, need_l), (gc, need_c)) if need]
        assert len(got) == len(want) and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, want))
    # the torch line keeps one volume that is not an input: -logits
    lg, cf = logits.clone().requires_grad_(), conf.clone().requires_grad_()
    _, extra = _saved_volumes(lambda: -lg * cf, (lg, cf), logits.numel())
    assert extra == 1, extra


def test_what_the_binding_refuses_and_accepts():
    import phl

    logits, conf, gE0 = _inputs((2, 5, 4, 6), "real", 7)
    want = -logits * conf
    # operands that are not contiguous are made so
    lt, ct, gt = (t.transpose(2, 3).contiguous().transpose(2, 3) for t in (logits, conf, gE0))
    assert not lt.is_contiguous() and not ct.is_contiguous() and not gt.is_contiguous()
    assert torch.equal(_bits(phl.nchw_confidence_unaries(lt, ct)), _bits(want))
    gc, gl = phl.nchw_confidence_unaries_grad(logits, conf, gE0, need_logits=True)
    got = phl.nchw_confidence_unaries_grad(lt, ct, gt, need_logits=True)
    assert torch.equal(_bits(got[0]), _bits(gc)) and torch.equal(_bits(got[1]), _bits(gl))
    # an empty batch, an empty image
    assert phl.nchw_confidence_unaries(logits[:0], conf[:0]).shape == (0, 5, 4, 6)
    assert phl.nchw_confidence_unaries(logits[..., :0], conf[..., :0]).shape == (2, 5, 4, 0)
    with pytest.raises(TypeError):
        phl.nchw_confidence_unaries(logits.double(), conf.double())
    with pytest.raises(TypeError):
        phl.nchw_confidence_unaries(logits, conf.cpu())
    with pytest.raises(TypeError):
        phl.nchw_confidence_unaries(logits, conf, out=torch.empty((2, 5, 4, 6), device=DEV, dtype=torch.float64))
    with pytest.raises(TypeError):
        phl.nchw_confidence_unaries_grad(logits, conf, gE0.double())
    for bad in (logits, conf[:1], conf[0], conf[..., :1], conf.reshape(2, 1, 24)):
        with pytest.raises(ValueError):
            phl.nchw_confidence_unaries(logits, bad)
    with pytest.raises(ValueError):
        phl.nchw_confidence_unaries(logits[0, 0], conf[0, 0])
    with pytest.raises(ValueError):
        phl.nchw_confidence_unaries_grad(logits, conf, gE0[:, :4])
    with pytest.raises(ValueError):
        phl.nchw_confidence_unaries_grad(logits, conf, gE0, need_conf=False, need_logits=False)
    with pytest.raises(phl.PhlError) as e:
        phl.nchw_confidence_unaries(logits, conf, out=logits)
    assert e.value.status == 1


# ---- the heads ---------------------------------------------------------------------------------------------------------
def _groups(net, prefixes):
    """The gradients of the parameters under each prefix as one vector (a single element would compare two roundings)."""
    out = {}
    for prefix in prefixes:
        gs = [p.grad.reshape(-1) for n, p in net.named_parameters() if n.startswith(prefix)]
        assert gs and all(g is not None for g in gs), prefix
        out[prefix] = torch.cat(gs).detach().clone()
    return out


def _spy():
    return binding_spy({"nchw_confidence_unaries": lambda a, k: "unaries", "nchw_confidence_unaries_fn": lambda a, k: "fn",
                        "nchw_confidence_unaries_grad": lambda a, k: ("grad", k["need_conf"], k["need_logits"])})


def _pair(make):
    """(the head with fused_unaries=True, the same head without it), the other keywords and every parameter equal."""
    torch.manual_seed(0)
    new = make(fused_unaries=True).to(DEV)
    old = make().to(DEV)
    old.load_state_dict(new.state_dict())
    assert new.CRF.fused_unaries is True and old.CRF.fused_unaries is False
    return new, old


def test_head_uncertainty():
    """CRFwUncertainty at 12 labels, [1, 12, 48, 64], one L1 step (the target lies below every depth: no kink between the
    runs), fused_grad and fused_step on in both nets."""
    from crf.mb_stereo_crf import CRFwUncertainty

    L, H, W = 12, 48, 64
    gen = torch.Generator(device=DEV).manual_seed(13)
    logits = torch.randn((1, L, H, W), device=DEV, generator=gen) * 2
    img = torch.rand((1, 3, H, W), device=DEV, generator=gen)
    feats = torch.randn((1, 64, H, W), device=DEV, generator=gen)
    prefixes = ("uncertainty_net.", "projection.", "CRF.Mu.gamma", "CRF.Mu.s")

    def step(net, dtype):
        net.zero_grad(set_to_none=True)
        if dtype == torch.float64:                               # the head's lines; charb's own default labels are fp32
            confidence = torch.exp(-net.uncertainty_net(img.double()))
            depth = net.CRF.expected_depth(net._guide(img.double(), feats.double()), logits.double(), confidence,
                                           labels=torch.arange(L, dtype=dtype, device=DEV))
        else:
            depth, confidence = net((logits, img, feats))
        (depth - (-1.0)).abs().mean().backward()
        return dict(_groups(net, prefixes), depth=depth.detach(), confidence=confidence.detach())

    new, old = _pair(lambda **kw: CRFwUncertainty(fused_grad=True, fused_step=True, **kw))
    with torch.no_grad():
        with _spy() as seen:
            d_new, c_new = new((logits, img, feats))
        assert seen == ["unaries"], seen                             # one call per forward
        with _spy() as seen:
            d_old, c_old = old((logits, img, feats))
        assert seen == [], seen
    assert d_new.shape == (1, 1, H, W) and torch.equal(_bits(d_new), _bits(d_old)) and torch.equal(_bits(c_new), _bits(c_old))
    with _spy() as seen:
        g_new = step(new, torch.float32)
    assert seen == ["fn", "unaries", ("grad", True, False)], seen    # the Function's forward is the one binding call
    with _spy() as seen:
        g_old = step(old, torch.float32)
    assert seen == [], seen
    assert torch.equal(_bits(g_new["depth"]), _bits(g_old["depth"])) and torch.equal(_bits(g_new["confidence"]), _bits(g_old["confidence"]))
    want = step(copy.deepcopy(old).double(), torch.float64)
    assert float(want["uncertainty_net."].abs().max()) > 0
    for k in prefixes:
        report_loop(f"uncertainty grad {k}", g_new[k], g_old[k], want[k])
    report_loop("uncertainty depth", g_new["depth"], g_old["depth"], want["depth"])


@contextlib.contextmanager
def _torch_prologue():
    """The module switch behind PHL_SCALAR_UNARIES=0: the upsampler's torch lines, which hand logits and the 0/1 mask to
    CRFasRNN."""
    from crf import mb_stereo_crf as heads

    was, heads._SCALAR_UNARIES = heads._SCALAR_UNARIES, False
    try:
        yield
    finally:
        heads._SCALAR_UNARIES = was


def test_head_upsampler_on_its_torch_lines():
    """CRFdepthUpsampler with its fused prologue switched off: the keyword covers -logits * mask, and the logits (a
    function of gamma and s) get their gradient from the kernel: need_logits=True, nothing for the mask."""
    from crf.mb_stereo_crf import CRFdepthUpsampler

    gen = torch.Generator(device=DEV).manual_seed(12)
    disp = torch.rand((1, 1, 6, 8), device=DEV, generator=gen) * 20 + 1
    disp[:, :, :2, :2] = 0                                           # no measurement: the mask is 0 there
    img = torch.rand((1, 3, 96, 128), device=DEV, generator=gen)
    prefixes = ("CRF.Mu.gamma", "CRF.Mu.s")

    def step(net, dtype):
        net.zero_grad(set_to_none=True)
        if dtype == torch.float64:                               # the head's torch lines with every operand float64, the labels too
            up = F.interpolate(disp.double(), size=img.shape[2:], mode="bilinear", align_corners=False)
            labels = torch.linspace(0, float(up.max()), 18, dtype=dtype, device=DEV)
            lg = -10 * net.CRF.Mu.get_energies_from_scalar(up, labels[None, :, None, None])
            mask = (up > 1e-2).double()
            assert 0 < float(mask.mean()) < 1
            depth = net.CRF.expected_depth(img.double(), lg, confidence=mask, labels=labels, values=labels)
        else:
            depth = net((disp, img, None))
        (depth - (-1.0)).abs().mean().backward()
        return dict(_groups(net, prefixes), depth=depth.detach())

    new, old = _pair(lambda **kw: CRFdepthUpsampler(fused_grad=True, fused_step=True, **kw))
    with _torch_prologue():
        with torch.no_grad():
            with _spy() as seen:
                d_new = new((disp, img, None))
            assert seen == ["unaries"], seen
            with _spy() as seen:
                d_old = old((disp, img, None))
            assert seen == [], seen
        assert d_new.shape == (1, 1, 96, 128) and torch.equal(_bits(d_new), _bits(d_old))
        with _spy() as seen:
            g_new = step(new, torch.float32)
        assert seen == ["fn", "unaries", ("grad", False, True)], seen
        with _spy() as seen:
            g_old = step(old, torch.float32)
        assert seen == [], seen
    assert torch.equal(_bits(g_new["depth"]), _bits(g_old["depth"]))
    want = step(copy.deepcopy(old).double(), torch.float64)
    for k in prefixes:
        report_loop(f"upsampler grad {k}", g_new[k], g_old[k], want[k])
    report_loop("upsampler depth", g_new["depth"], g_old["depth"], want["depth"])
    # with the fused prologue the head hands E0 over as energies: the keyword has nothing to do
    with torch.no_grad(), _spy() as seen:
        new((disp, img, None))
    assert seen == [], seen
