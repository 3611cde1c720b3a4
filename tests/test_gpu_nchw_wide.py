"""The channel-major mean-field step for a general Mu at 256 < L <= 512 labels (phl.nchw_softmax_compat_wide,
k_nchw_tile on its 32-pixel tile, phl_nchw.hip) and the CRFasRNN loop routed onto it.

Rule of the step's accuracy checks (the project's own, test_gpu_nchw_step.py): with Y64 the float64 result on the device,
e_hip = max|hip - Y64| and e_torch = max|fp32 torch ops - Y64| over ALL elements, and
e_hip <= max(2e-6 * max(1, |Y64|.max()), 2 * e_torch).  The loop is held to e_new <= 2 * e_old against the float64 module,
e_old being the plain loop in the same tree.  Every pair of errors is printed."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

from _guided_util import DEV, spy

pytestmark = pytest.mark.gpu

# 257: one label into the range, odd, a label tile of one row; 288: whole 32-label tiles; 341 / 344: the reference's count at
# 2048 columns and its padded form; 511: odd at the top; 512: full
LS = [257, 288, 341, 344, 511, 512]
SIZES = [(7, 9), (13, 17), (16, 24)]         # n = 63 (a short single tile pair, planes off the 16-byte grid), 221, 384 (aligned)
# the float4 path (n % 4 == 0, 16-byte aligned bases) with a short last tile: n = 100, 12, 4, 260
VEC_SIZES = [(5, 20), (2, 6), (1, 4), (4, 65)]
B = 2
WIDE_TP = 32                                 # pixels of a tile above 256 labels
WIDE = "phl_nchw_softmax_compat_wide"
PRODUCT, UNIFORM, SOFTMAX, LOGITS = 0, 1, 2, 3


def _inputs(L, H, W, seed, B=B):
    g = torch.Generator(device=DEV).manual_seed(seed)
    E0 = torch.rand((B, L, H, W), device=DEV, generator=g) * 30 - 5
    G = torch.randn((B, L, H, W), device=DEV, generator=g) * 5
    Mu = torch.rand((L, L), device=DEV, generator=g) * 4 + torch.arange(L, device=DEV, dtype=torch.float32)[:, None] * 0.05
    return E0, G, Mu


def _energy(E0, G):
    return E0 if G is None else E0 + G


def _truth(E0, G, Mu64):
    return torch.einsum("ac,bahw->bchw", Mu64, F.softmax(-_energy(E0.double(), None if G is None else G.double()), 1))


def _torch32(E0, G, Mu):
    return F.conv2d(F.softmax(-_energy(E0, G), 1), Mu.t()[..., None, None])


def _check_product(name, hip, E0, G, Mu):
    want = _truth(E0, G, Mu.double())
    e_hip = float((hip.double() - want).abs().max())
    e_torch = float((_torch32(E0, G, Mu).double() - want).abs().max())
    bound = max(2e-6 * max(1.0, float(want.abs().max())), 2 * e_torch)
    print(f"{name}: e_hip = {e_hip:.3e}  e_torch = {e_torch:.3e}  |Y| <= {float(want.abs().max()):.4g}")
    assert torch.isfinite(hip).all(), name
    assert e_hip <= bound, (name, e_hip, e_torch)


@contextlib.contextmanager
def _launch_spy():
    """(entry point, its mode -- None for the wide entry, which has none) of every library launch made through phl._launch."""
    import phl

    real, seen = phl._launch, []

    def launch(device, name, *args):
        seen.append((name, None if name == WIDE else args[-1]))
        return real(device, name, *args)

    phl._launch = launch
    try:
        yield seen
    finally:
        phl._launch = real


def _on_float4_path(*tensors):
    return all(t is None or (t.is_contiguous() and t.data_ptr() % 16 == 0 and t[0, 0].numel() % 4 == 0) for t in tensors)


@pytest.mark.parametrize("L", LS)
def test_product_parity(L):
    import phl

    for H, W in SIZES:
        E0, G, Mu = _inputs(L, H, W, seed=L + H)
        assert not torch.equal(Mu, Mu.t())                     # a transposed operand cannot pass
        for g in (G, None):
            with _launch_spy() as seen:
                hip = phl.nchw_softmax_compat_wide(E0, g, Mu)
            assert seen == [(WIDE, None)], seen
            assert hip.shape == E0.shape
            _check_product(f"wide product L{L} {H}x{W} G={'yes' if g is not None else 'none'}", hip, E0, g, Mu)


def test_product_needs_the_max_subtraction():
    """Energies near +80 and -80 in one column: exp(80) ** 2 leaves fp32 without the subtraction of the column maximum."""
    import phl

    L = 341
    E0, G, Mu = _inputs(L, 13, 17, seed=3)
    E0 = torch.where(torch.arange(L, device=DEV)[None, :, None, None] % 2 == 0, E0 * 0.1 + 80, E0 * 0.1 - 80)
    hip = phl.nchw_softmax_compat_wide(E0, G * 0.1, Mu)
    _check_product(f"wide product L{L} energies +-80", hip, E0, G * 0.1, Mu)


@pytest.mark.parametrize("L", [257, 512])
def test_product_parity_short_float4_tiles(L):
    import phl

    for H, W in VEC_SIZES:
        E0, G, Mu = _inputs(L, H, W, seed=L + W)
        assert _on_float4_path(E0, G) and (H * W) % WIDE_TP != 0
        for g in (G, None):
            with _launch_spy() as seen:
                hip = phl.nchw_softmax_compat_wide(E0, g, Mu)
            assert seen == [(WIDE, None)] and _on_float4_path(hip)
            _check_product(f"wide product L{L} {H}x{W} G={'yes' if g is not None else 'none'}", hip, E0, g, Mu)


def _shifted(t):
    """A contiguous copy of t whose base lies 4 bytes past the 16-byte grid."""
    buf = torch.zeros((t.numel() + 5,), device=DEV)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("L", [257, 512])
def test_dword_fallback_for_a_base_off_the_16_byte_grid(L):
    """n % 4 == 0 with one of E0, G, out off the 16-byte grid takes the dword loads and stores; nothing else differs
    between the two forms, so the bits are those of the aligned call."""
    import phl

    H, W = VEC_SIZES[0]
    E0, G, Mu = _inputs(L, H, W, seed=L + 40)
    want = phl.nchw_softmax_compat_wide(E0, G, Mu)
    assert _on_float4_path(E0, G, want)
    assert torch.equal(phl.nchw_softmax_compat_wide(_shifted(E0), G, Mu), want)
    assert torch.equal(phl.nchw_softmax_compat_wide(E0, _shifted(G), Mu), want)
    out = _shifted(torch.full(E0.shape, float("nan"), device=DEV))
    assert phl.nchw_softmax_compat_wide(E0, G, Mu, out=out) is out and torch.equal(out, want)
    _check_product(f"wide product L{L} {H}x{W}, out off the 16-byte grid", out, E0, G, Mu)


@pytest.mark.parametrize("L", [257, 512])
@pytest.mark.parametrize("H,W", VEC_SIZES[:2] + SIZES[:1])
def test_nothing_written_behind_out(H, W, L):
    """``out`` as a view at the front of a larger buffer: a short last tile leaves the 4096 floats behind it alone (on the
    float4 path and, at n = 63, on the dword path)."""
    import phl

    E0, G, Mu = _inputs(L, H, W, seed=L + 50)
    want = phl.nchw_softmax_compat_wide(E0, G, Mu)
    sentinel, pad = -12345.5, 4096
    buf = torch.full((E0.numel() + pad,), sentinel, device=DEV)
    out = buf[:E0.numel()].view(E0.shape)
    assert _on_float4_path(E0, G, out) == ((H * W) % 4 == 0)
    assert phl.nchw_softmax_compat_wide(E0, G, Mu, out=out) is out
    assert torch.equal(out, want)
    assert torch.equal(buf[E0.numel():], torch.full((pad,), sentinel, device=DEV))


@pytest.mark.parametrize("L", [341, 512])
def test_two_calls_give_the_same_bits(L):
    import phl

    for H, W in SIZES[1:]:
        E0, G, Mu = _inputs(L, H, W, seed=L + 60)
        first = phl.nchw_softmax_compat_wide(E0, G, Mu)
        out = torch.full(E0.shape, float("nan"), device=DEV)
        assert phl.nchw_softmax_compat_wide(E0, G, Mu, out=out) is out and torch.equal(out, first)


@pytest.mark.parametrize("L", [18, 64, 256])                     # VALU, matrix cores, the full 64-pixel tile
def test_up_to_256_labels_it_is_the_old_kernel(L):
    import phl

    for H, W in SIZES[1:]:
        E0, G, Mu = _inputs(L, H, W, seed=L + 70)
        for g in (G, None):
            with _launch_spy() as seen:
                wide = phl.nchw_softmax_compat_wide(E0, g, Mu)
                old = phl.nchw_softmax_compat(E0, g, Mu, uniform=False)
            assert seen == [(WIDE, None), ("phl_nchw_softmax_compat", PRODUCT)], seen
            assert torch.equal(wide, old)


def test_arguments():
    import phl

    L, H, W = 257, 13, 18
    g = torch.Generator(device=DEV).manual_seed(11)
    E0 = (torch.rand((B, H, W, L), device=DEV, generator=g) * 30 - 5).permute(0, 3, 1, 2)       # a permuted view
    G = (torch.randn((B, L, H, 2 * W), device=DEV, generator=g) * 5)[..., ::2]                  # a strided slice
    Mu = _inputs(L, 1, 1, seed=5)[2]
    assert not E0.is_contiguous() and not G.is_contiguous()
    hip = phl.nchw_softmax_compat_wide(E0, G, Mu)
    _check_product("wide product, non-contiguous inputs", hip, E0, G, Mu)
    flat = phl.nchw_softmax_compat_wide(E0.reshape(B, L, H * W), G.reshape(B, L, H * W), Mu)      # [B, L, n]
    assert flat.shape == (B, L, H * W) and torch.equal(flat.reshape(B, L, H, W), hip)
    Gc = G.contiguous()
    with pytest.raises(phl.PhlError) as e:
        phl.nchw_softmax_compat_wide(E0, Gc, Mu, out=Gc)
    assert e.value.status == 1
    with pytest.raises(TypeError):
        phl.nchw_softmax_compat_wide(E0, G, Mu, out=torch.empty((B, L, H, 2 * W), device=DEV)[:, :, :, ::2])
    with pytest.raises(TypeError):
        phl.nchw_softmax_compat_wide(E0.double(), None, Mu)
    with pytest.raises(ValueError):
        phl.nchw_softmax_compat_wide(E0, G)                                  # Mu=None
    with pytest.raises(ValueError):
        phl.nchw_softmax_compat_wide(E0, G, Mu[:, :-1])
    E1, G1, Mu1 = _inputs(513, 2, 3, seed=1)
    with pytest.raises(phl.PhlError) as e:
        phl.nchw_softmax_compat_wide(E1, G1, Mu1)
    assert e.value.status == phl.ERR_UNSUPPORTED == 7
    assert phl.nchw_softmax_compat_wide(torch.zeros((2, 300, 0, 3), device=DEV), None, Mu1[:300, :300]).shape == (2, 300, 0, 3)


# ---- the loop ---------------------------------------------------------------------------------------------------------
class _CountingF:
    """torch.nn.functional as crf.crf_module sees it, with softmax and conv2d counted."""

    def __init__(self, calls):
        self._calls = calls

    def __getattr__(self, name):
        return getattr(F, name)

    def softmax(self, *a, **k):
        self._calls["softmax"] += 1
        return F.softmax(*a, **k)

    def conv2d(self, *a, **k):
        self._calls["conv2d"] += 1
        return F.conv2d(*a, **k)


@contextlib.contextmanager
def _loop_spy():
    """Counts of F.softmax / F.conv2d calls made from crf.crf_module, and in ``calls["phl"]`` the order of the loop's calls
    into the binding: "wide" (nchw_softmax_compat_wide), "step" / "logits" (nchw_softmax_compat without / with
    logits=True), "expect" (nchw_expected_value)."""
    import phl
    from crf import crf_module as cm

    calls = {"softmax": 0, "conv2d": 0, "phl": []}
    real = {k: getattr(phl, k) for k in ("nchw_softmax_compat", "nchw_softmax_compat_wide", "nchw_expected_value")}
    real_f = cm.F

    def step(*a, **k):
        calls["phl"].append("logits" if k.get("logits") else "step")
        return real["nchw_softmax_compat"](*a, **k)

    def wide(*a, **k):
        calls["phl"].append("wide")
        return real["nchw_softmax_compat_wide"](*a, **k)

    def expect(*a, **k):
        calls["phl"].append("expect")
        return real["nchw_expected_value"](*a, **k)

    cm.F = _CountingF(calls)
    phl.nchw_softmax_compat, phl.nchw_softmax_compat_wide, phl.nchw_expected_value = step, wide, expect
    try:
        yield calls
    finally:
        cm.F = real_f
        for k, f in real.items():
            setattr(phl, k, f)


@contextlib.contextmanager
def _old_loop():
    """The module switch behind PHL_NCHW_STEP=0."""
    from crf import crf_module as cm

    was, cm._NCHW_STEP = cm._NCHW_STEP, False
    try:
        yield
    finally:
        cm._NCHW_STEP = was


def _both_loops(call, niters, end):
    """(new loop, old loop) outputs of one no-grad call, with the call counts of both checked.  end: the new loop's last
    call, "logits" or "expect"."""
    with torch.no_grad():
        with _loop_spy() as calls, spy() as wcalls:
            new = call()
        assert calls == {"softmax": 0, "conv2d": 0, "phl": ["wide"] * niters + [end]}, calls
        assert wcalls == {"hip": niters, "box_sum": 0}, wcalls
        with _old_loop(), _loop_spy() as calls:
            old = call()
        assert calls["phl"] == [] and calls["softmax"] == niters + 1 and calls["conv2d"] == niters, calls
    return new, old


def _report_loop(name, new, old, want):
    e_new, e_old = float((new.double() - want).abs().max()), float((old.double() - want).abs().max())
    print(f"{name}: e_new = {e_new:.3e}  e_old = {e_old:.3e}  |out| <= {float(want.abs().max()):.4g}")
    assert torch.isfinite(new).all()
    assert e_new <= 2 * e_old, (name, e_new, e_old)


L_REF = 341                                  # the reference's label count at 2048 columns (max_disp = w // 6)


def _crf_case():
    from crf.crf_module import CRFasRNN, charb

    g = torch.Generator(device=DEV).manual_seed(41)
    net = CRFasRNN(charb(.05), niters=2, r=4, eps=1e-2).to(DEV)
    refs = torch.rand((1, 1, 24, 40), device=DEV, generator=g)
    logits = torch.randn((1, L_REF, 24, 40), device=DEV, generator=g) * 3
    labels = torch.arange(L_REF, dtype=torch.float32, device=DEV)
    return net, refs, logits, labels


def test_loop_at_341_labels():
    net, refs, logits, labels = _crf_case()
    new, old = _both_loops(lambda: net(refs, logits, labels=labels), net.niters, "logits")
    assert new.shape == logits.shape
    with torch.no_grad():
        want = net.double()(refs.double(), logits.double(), labels=labels.double())
    net.float()
    _report_loop("CRFasRNN charb L341", new, old, want)


def test_expected_depth_at_341_labels():
    """The loop ends in one phl.nchw_expected_value call on E0 and G; the logits are never written."""
    net, refs, logits, labels = _crf_case()
    new, old = _both_loops(lambda: net.expected_depth(refs, logits, labels=labels), net.niters, "expect")
    assert new.shape == (1, 1, 24, 40)
    with torch.no_grad():
        want = net.double().expected_depth(refs.double(), logits.double(), labels=labels.double())
    net.float()
    _report_loop("CRFasRNN.expected_depth charb L341", new, old, want)


def test_refiner_head_at_341_labels():
    from crf.mb_stereo_crf import CRFdepthRefiner

    torch.manual_seed(31)                    # the module draws its parameters from the global generator
    g = torch.Generator(device=DEV).manual_seed(42)
    net = CRFdepthRefiner(d_in=8, d_guide=6, r=4, niters=2).to(DEV)
    logits = torch.randn((1, L_REF, 24, 40), device=DEV, generator=g) * 3
    rgb, feats = torch.rand((1, 3, 24, 40), device=DEV, generator=g), torch.rand((1, 8, 24, 40), device=DEV, generator=g)
    new, old = _both_loops(lambda: net((logits, rgb, feats)), 2, "expect")
    assert new.shape == (1, 1, 24, 40)
    with torch.no_grad():
        guide = net._guide(rgb, feats)       # the head's fp32 prologue; charb's own default labels are fp32: 0 .. L-1
        net.CRF.double()
        want = net.CRF.expected_depth(guide.double(), logits.double(), labels=torch.arange(L_REF, dtype=torch.float64, device=DEV))
        net.CRF.float()
    _report_loop("CRFdepthRefiner L341", new, old, want)


def test_routing_stays_where_it_must():
    from crf.crf_module import CRFasRNN, charb, potts

    g = torch.Generator(device=DEV).manual_seed(43)
    refs = torch.rand((1, 1, 12, 20), device=DEV, generator=g)

    # a general Mu above 512 labels keeps the plain loop
    net = CRFasRNN(charb(.05), niters=2, r=4, eps=1e-2).to(DEV)
    logits = torch.randn((1, 513, 12, 20), device=DEV, generator=g) * 3
    with torch.no_grad(), _loop_spy() as calls:
        net(refs, logits, labels=torch.arange(513, dtype=torch.float32, device=DEV))
    assert calls["phl"] == [] and calls["softmax"] == net.niters + 1, calls

    # the Potts family above 256 labels is still the UNIFORM mode of the old entry
    pnet = CRFasRNN(potts(300), niters=2, r=4, eps=1e-2, notrain_mu=True).to(DEV)
    plogits = torch.randn((1, 300, 12, 20), device=DEV, generator=g) * 3
    with torch.no_grad(), _launch_spy() as seen, _loop_spy() as calls:
        pnet(refs, plogits)
    assert calls["phl"] == ["step", "step", "logits"] and calls["softmax"] == 0, calls
    assert [m for name, m in seen if name.startswith("phl_nchw_softmax_compat")] == [UNIFORM, UNIFORM, LOGITS], seen

    # autograd, float64 and CPU tensors at 341 labels never reach the kernel, and compute exactly what the plain loop computes
    logits = torch.randn((1, L_REF, 12, 20), device=DEV, generator=g) * 3

    def run(net, refs, logits):
        labels = torch.arange(L_REF, dtype=logits.dtype, device=logits.device)
        with _loop_spy() as calls:
            out = net(refs, logits, labels=labels)
        assert calls["phl"] == [] and calls["softmax"] == net.niters + 1, calls
        with _old_loop():
            assert torch.equal(out.detach(), net(refs, logits, labels=labels).detach())

    run(net, refs, logits.clone().requires_grad_())           # a gradient of the logits
    run(net, refs, logits)                                    # grad mode on: Mu's and W's parameters ask for one
    with torch.no_grad():
        run(net.double(), refs.double(), logits.double())
        run(net.float().cpu(), refs.cpu(), logits.cpu())
