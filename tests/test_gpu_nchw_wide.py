"""The channel-major mean-field step for a general Mu at 256 < L <= 512 labels (phl.nchw_softmax_compat_wide,
k_nchw_tile on its 32-pixel tile, phl_nchw.hip) and the CRFasRNN loop routed onto it.

Rule of the step's accuracy checks (the project's own, test_gpu_nchw_step.py): with Y64 the float64 result on the device,
e_hip = max|hip - Y64| and e_torch = max|fp32 torch ops - Y64| over ALL elements, and
e_hip <= max(2e-6 * max(1, |Y64|.max()), 2 * e_torch).  The loop is held to e_new <= 2 * e_old against the float64 module,
e_old being the plain loop in the same tree.  Every pair of errors is printed."""
import pytest
import torch

from _guided_util import DEV
from _nchw_util import (B, LOGITS, PRODUCT, UNIFORM, WIDE, both_loops, check_product, inputs, launch_spy, loop_spy, old_loop,
                        on_float4_path, report_loop, shifted)

pytestmark = pytest.mark.gpu

# 257: one label into the range, odd, a label tile of one row; 288: whole 32-label tiles; 341 / 344: the reference's count at
# 2048 columns and its padded form; 511: odd at the top; 512: full
LS = [257, 288, 341, 344, 511, 512]
SIZES = [(7, 9), (13, 17), (16, 24)]         # n = 63 (a short single tile pair, planes off the 16-byte grid), 221, 384 (aligned)
# the float4 path (n % 4 == 0, 16-byte aligned bases) with a short last tile: n = 100, 12, 4, 260
VEC_SIZES = [(5, 20), (2, 6), (1, 4), (4, 65)]
WIDE_TP = 32                                 # pixels of a tile above 256 labels


@pytest.mark.parametrize("L", LS)
def test_product_parity(L):
    import phl

    for H, W in SIZES:
        E0, G, Mu = inputs(L, H, W, seed=L + H)
        assert not torch.equal(Mu, Mu.t())                     # a transposed operand cannot pass
        for g in (G, None):
            with launch_spy() as seen:
                hip = phl.nchw_softmax_compat_wide(E0, g, Mu)
            assert seen == [(WIDE, None)], seen
            assert hip.shape == E0.shape
            check_product(f"wide product L{L} {H}x{W} G={'yes' if g is not None else 'none'}", hip, E0, g, Mu)


def test_product_needs_the_max_subtraction():
    """Energies near +80 and -80 in one column: exp(80) ** 2 leaves fp32 without the subtraction of the column maximum."""
    import phl

    L = 341
    E0, G, Mu = inputs(L, 13, 17, seed=3)
    E0 = torch.where(torch.arange(L, device=DEV)[None, :, None, None] % 2 == 0, E0 * 0.1 + 80, E0 * 0.1 - 80)
    hip = phl.nchw_softmax_compat_wide(E0, G * 0.1, Mu)
    check_product(f"wide product L{L} energies +-80", hip, E0, G * 0.1, Mu)


@pytest.mark.parametrize("L", [257, 512])
def test_product_parity_short_float4_tiles(L):
    import phl

    for H, W in VEC_SIZES:
        E0, G, Mu = inputs(L, H, W, seed=L + W)
        assert on_float4_path(E0, G) and (H * W) % WIDE_TP != 0
        for g in (G, None):
            with launch_spy() as seen:
                hip = phl.nchw_softmax_compat_wide(E0, g, Mu)
            assert seen == [(WIDE, None)] and on_float4_path(hip)
            check_product(f"wide product L{L} {H}x{W} G={'yes' if g is not None else 'none'}", hip, E0, g, Mu)


@pytest.mark.parametrize("L", [257, 512])
def test_dword_fallback_for_a_base_off_the_16_byte_grid(L):
    """n % 4 == 0 with one of E0, G, out off the 16-byte grid takes the dword loads and stores; nothing else differs
    between the two forms, so the bits are those of the aligned call."""
    import phl

    H, W = VEC_SIZES[0]
    E0, G, Mu = inputs(L, H, W, seed=L + 40)
    want = phl.nchw_softmax_compat_wide(E0, G, Mu)
    assert on_float4_path(E0, G, want)
    assert torch.equal(phl.nchw_softmax_compat_wide(shifted(E0), G, Mu), want)
    assert torch.equal(phl.nchw_softmax_compat_wide(E0, shifted(G), Mu), want)
    out = shifted(torch.full(E0.shape, float("nan"), device=DEV))
    assert phl.nchw_softmax_compat_wide(E0, G, Mu, out=out) is out and torch.equal(out, want)
    check_product(f"wide product L{L} {H}x{W}, out off the 16-byte grid", out, E0, G, Mu)


@pytest.mark.parametrize("L", [257, 512])
@pytest.mark.parametrize("H,W", VEC_SIZES[:2] + SIZES[:1])
def test_nothing_written_behind_out(H, W, L):
    """``out`` as a view at the front of a larger buffer: a short last tile leaves the 4096 floats behind it alone (on the
    float4 path and, at n = 63, on the dword path)."""
    import phl

    E0, G, Mu = inputs(L, H, W, seed=L + 50)
    want = phl.nchw_softmax_compat_wide(E0, G, Mu)
    sentinel, pad = -12345.5, 4096
    buf = torch.full((E0.numel() + pad,), sentinel, device=DEV)
    out = buf[:E0.numel()].view(E0.shape)
    assert on_float4_path(E0, G, out) == ((H * W) % 4 == 0)
    assert phl.nchw_softmax_compat_wide(E0, G, Mu, out=out) is out
    assert torch.equal(out, want)
    assert torch.equal(buf[E0.numel():], torch.full((pad,), sentinel, device=DEV))


@pytest.mark.parametrize("L", [341, 512])
def test_two_calls_give_the_same_bits(L):
    import phl

    for H, W in SIZES[1:]:
        E0, G, Mu = inputs(L, H, W, seed=L + 60)
        first = phl.nchw_softmax_compat_wide(E0, G, Mu)
        out = torch.full(E0.shape, float("nan"), device=DEV)
        assert phl.nchw_softmax_compat_wide(E0, G, Mu, out=out) is out and torch.equal(out, first)


@pytest.mark.parametrize("L", [18, 64, 256])                     # VALU, matrix cores, the full 64-pixel tile
def test_up_to_256_labels_it_is_the_old_kernel(L):
    import phl

    for H, W in SIZES[1:]:
        E0, G, Mu = inputs(L, H, W, seed=L + 70)
        for g in (G, None):
            with launch_spy() as seen:
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
    Mu = inputs(L, 1, 1, seed=5)[2]
    assert not E0.is_contiguous() and not G.is_contiguous()
    hip = phl.nchw_softmax_compat_wide(E0, G, Mu)
    check_product("wide product, non-contiguous inputs", hip, E0, G, Mu)
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
    E1, G1, Mu1 = inputs(513, 2, 3, seed=1)
    with pytest.raises(phl.PhlError) as e:
        phl.nchw_softmax_compat_wide(E1, G1, Mu1)
    assert e.value.status == phl.ERR_UNSUPPORTED == 7
    assert phl.nchw_softmax_compat_wide(torch.zeros((2, 300, 0, 3), device=DEV), None, Mu1[:300, :300]).shape == (2, 300, 0, 3)


# ---- the loop ---------------------------------------------------------------------------------------------------------
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
    new, old = both_loops(lambda: net(refs, logits, labels=labels), net.niters, "logits")
    assert new.shape == logits.shape
    with torch.no_grad():
        want = net.double()(refs.double(), logits.double(), labels=labels.double())
    net.float()
    report_loop("CRFasRNN charb L341", new, old, want)


def test_expected_depth_at_341_labels():
    """The loop ends in one phl.nchw_expected_value call on E0 and G; the logits are never written."""
    net, refs, logits, labels = _crf_case()
    new, old = both_loops(lambda: net.expected_depth(refs, logits, labels=labels), net.niters, "expect")
    assert new.shape == (1, 1, 24, 40)
    with torch.no_grad():
        want = net.double().expected_depth(refs.double(), logits.double(), labels=labels.double())
    net.float()
    report_loop("CRFasRNN.expected_depth charb L341", new, old, want)


def test_refiner_head_at_341_labels():
    from crf.mb_stereo_crf import CRFdepthRefiner

    torch.manual_seed(31)                    # the module draws its parameters from the global generator
    g = torch.Generator(device=DEV).manual_seed(42)
    net = CRFdepthRefiner(d_in=8, d_guide=6, r=4, niters=2).to(DEV)
    logits = torch.randn((1, L_REF, 24, 40), device=DEV, generator=g) * 3
    rgb, feats = torch.rand((1, 3, 24, 40), device=DEV, generator=g), torch.rand((1, 8, 24, 40), device=DEV, generator=g)
    new, old = both_loops(lambda: net((logits, rgb, feats)), 2, "expect")
    assert new.shape == (1, 1, 24, 40)
    with torch.no_grad():
        guide = net._guide(rgb, feats)       # the head's fp32 prologue; charb's own default labels are fp32: 0 .. L-1
        net.CRF.double()
        want = net.CRF.expected_depth(guide.double(), logits.double(), labels=torch.arange(L_REF, dtype=torch.float64, device=DEV))
        net.CRF.float()
    report_loop("CRFdepthRefiner L341", new, old, want)


def test_routing_stays_where_it_must():
    from crf.crf_module import CRFasRNN, charb, potts

    g = torch.Generator(device=DEV).manual_seed(43)
    refs = torch.rand((1, 1, 12, 20), device=DEV, generator=g)

    # a general Mu above 512 labels keeps the plain loop
    net = CRFasRNN(charb(.05), niters=2, r=4, eps=1e-2).to(DEV)
    logits = torch.randn((1, 513, 12, 20), device=DEV, generator=g) * 3
    with torch.no_grad(), loop_spy(order=True) as calls:
        net(refs, logits, labels=torch.arange(513, dtype=torch.float32, device=DEV))
    assert calls["phl"] == [] and calls["softmax"] == net.niters + 1, calls

    # the Potts family above 256 labels is still the UNIFORM mode of the old entry
    pnet = CRFasRNN(potts(300), niters=2, r=4, eps=1e-2, notrain_mu=True).to(DEV)
    plogits = torch.randn((1, 300, 12, 20), device=DEV, generator=g) * 3
    with torch.no_grad(), launch_spy() as seen, loop_spy(order=True) as calls:
        pnet(refs, plogits)
    assert calls["phl"] == ["step", "step", "logits"] and calls["softmax"] == 0, calls
    assert [m for name, m in seen if name.startswith("phl_nchw_softmax_compat")] == [UNIFORM, UNIFORM, LOGITS], seen

    # autograd, float64 and CPU tensors at 341 labels never reach the kernel, and compute exactly what the plain loop computes
    logits = torch.randn((1, L_REF, 12, 20), device=DEV, generator=g) * 3

    def run(net, refs, logits):
        labels = torch.arange(L_REF, dtype=logits.dtype, device=logits.device)
        with loop_spy(order=True) as calls:
            out = net(refs, logits, labels=labels)
        assert calls["phl"] == [] and calls["softmax"] == net.niters + 1, calls
        with old_loop():
            assert torch.equal(out.detach(), net(refs, logits, labels=labels).detach())

    run(net, refs, logits.clone().requires_grad_())           # a gradient of the logits
    run(net, refs, logits)                                    # grad mode on: Mu's and W's parameters ask for one
    with torch.no_grad():
        run(net.double(), refs.double(), logits.double())
        run(net.float().cpu(), refs.cpu(), logits.cpu())
