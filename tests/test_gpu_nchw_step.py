"""The channel-major fused mean-field step (phl.nchw_softmax_compat, phl_nchw.hip) and the CRFasRNN loop built on it.

Rule of the step's accuracy checks (the project's own, test_gpu_crf_api.py): with Y64 the float64 result on the device,
e_hip = max|hip - Y64| and e_torch = max|fp32 torch ops - Y64| over ALL elements, and
e_hip <= max(2e-6 * max(1, |Y64|.max()), 2 * e_torch).  Softmax mode: <= 2e-6 and columns summing to 1 within 1e-5, logits
mode: <= 1e-4 * |E|.max() (the bounds of phl.softmax_neg_add's test).  The loop is held to e_new <= 2 * e_old against the
float64 fixture / the float64 module, e_old being the plain loop in the same tree (the factor test_golden_crfasrnn_default_w
grants the multi-iteration fixtures).  Every pair of errors is printed."""
import pytest
import torch
import torch.nn.functional as F

from _guided_fixtures import load_case
from _guided_util import DEV
from _nchw_util import (B, LOGITS, PRODUCT, SOFTMAX, UNIFORM, both_loops, check_product, energy, inputs, launch_spy, loop_spy,
                        old_loop, on_float4_path, report_loop, shifted)

pytestmark = pytest.mark.gpu

LS = [1, 5, 16, 18, 33, 64, 231, 256]         # VALU product up to 32 labels, matrix cores above; odd and full tiles
SIZES = [(7, 9), (13, 17), (16, 24)]         # n = 63 (one short tile, planes off the 16-byte grid), 221, 384 (aligned)
# the float4 path (n % 4 == 0, 16-byte aligned bases) with a short last tile: n = 100 (a full tile + 36 pixels), 12 (one
# short tile), 4 (one float4), 260 (four pixels past the streaming kernel's 256-pixel workgroup as well)
VEC_SIZES = [(5, 20), (2, 6), (1, 4), (4, 65)]
TP = 64                                      # pixels of a tile of k_nchw_tile


@pytest.mark.parametrize("L", LS)
def test_product_parity(L):
    import phl

    for H, W in SIZES:
        E0, G, Mu = inputs(L, H, W, seed=L + H)
        if L > 1:
            assert not torch.equal(Mu, Mu.t())                 # a transposed operand cannot pass
        for g in (G, None):
            with launch_spy() as seen:
                hip = phl.nchw_softmax_compat(E0, g, Mu)
            assert seen == [("phl_nchw_softmax_compat", PRODUCT)]
            assert hip.shape == E0.shape
            check_product(f"product L{L} {H}x{W} G={'yes' if g is not None else 'none'}", hip, E0, g, Mu)


@pytest.mark.parametrize("L", [18, 64])
def test_product_needs_the_max_subtraction(L):
    """Energies near +80 and -80 in one column: exp(80) ** 2 leaves fp32 without the subtraction of the column maximum."""
    import phl

    E0, G, Mu = inputs(L, 13, 17, seed=3)
    E0 = torch.where(torch.arange(L, device=DEV)[None, :, None, None] % 2 == 0, E0 * 0.1 + 80, E0 * 0.1 - 80)
    hip = phl.nchw_softmax_compat(E0, G * 0.1, Mu)
    check_product(f"product L{L} energies +-80", hip, E0, G * 0.1, Mu)


@pytest.mark.parametrize("L", [1, 5, 18, 64, 256, 300])         # 300: columns longer than an LDS tile
def test_softmax_and_logits_modes(L):
    import phl

    for H, W in SIZES:
        E0, G, _ = inputs(L, H, W, seed=2 * L + W)
        for g in (G, None):
            with launch_spy() as seen:
                q = phl.nchw_softmax_compat(E0, g)
            assert seen == [("phl_nchw_softmax_compat", SOFTMAX)]
            want = F.softmax(-energy(E0.double(), None if g is None else g.double()), 1)
            err, colsum = float((q.double() - want).abs().max()), float((q.sum(1) - 1).abs().max())
            print(f"softmax L{L} {H}x{W} G={'yes' if g is not None else 'none'}: err = {err:.3e}  |colsum - 1| = {colsum:.3e}")
            assert err <= 2e-6 and colsum <= 1e-5
        with launch_spy() as seen:
            lg = phl.nchw_softmax_compat(E0, G, logits=True)
        assert seen == [("phl_nchw_softmax_compat", LOGITS)]
        want = -(E0.double() + G.double())
        err = float((lg.double() - want).abs().max())
        print(f"logits L{L} {H}x{W}: err = {err:.3e} of {float(want.abs().max()):.4g}")
        assert err <= 1e-4 * float(want.abs().max())
    with pytest.raises(ValueError):
        phl.nchw_softmax_compat(E0, None, logits=True)


@pytest.mark.parametrize("L", [2, 5, 18, 64, 256, 300, 1024])
def test_uniform_mode(L):
    import phl
    from crf.crf_module import _compat_matrix, potts

    for H, W in SIZES[::2]:
        E0, G, _ = inputs(L, H, W, seed=L + 7)
        Mp = _compat_matrix(potts(L).to(DEV), L, None, DEV)
        with launch_spy() as seen:
            hip = phl.nchw_softmax_compat(E0, G, Mp)                     # detected
        assert seen == [("phl_nchw_softmax_compat", UNIFORM)]
        check_product(f"uniform potts L{L} {H}x{W}", hip, E0, G, Mp)
        M64 = 0.3 * torch.ones((L, L), dtype=torch.float64, device=DEV) - 1.7 * torch.eye(L, dtype=torch.float64, device=DEV)
        with launch_spy() as seen:
            hip = phl.nchw_softmax_compat(E0, None, uniform=(0.3, -1.7))
        assert seen == [("phl_nchw_softmax_compat", UNIFORM)]
        check_product(f"uniform (0.3, -1.7) L{L} {H}x{W}", hip, E0, None, M64.float(), M64)
        if L <= 256:                                                      # the same matrix through the product
            with launch_spy() as seen:
                prod = phl.nchw_softmax_compat(E0, G, Mp, uniform=False)
            assert seen == [("phl_nchw_softmax_compat", PRODUCT)]
            check_product(f"potts as a product L{L} {H}x{W}", prod, E0, G, Mp)


@pytest.mark.parametrize("batch", [1, 2, 3])
@pytest.mark.parametrize("L", [5, 18, 32, 33, 64, 231, 256])
def test_product_parity_short_float4_tiles(L, batch):
    import phl

    for H, W in VEC_SIZES:
        E0, G, Mu = inputs(L, H, W, seed=L + W + batch, B=batch)
        assert on_float4_path(E0, G) and (H * W) % TP != 0
        for g in (G, None):
            with launch_spy() as seen:
                hip = phl.nchw_softmax_compat(E0, g, Mu)
            assert seen == [("phl_nchw_softmax_compat", PRODUCT)] and on_float4_path(hip)
            check_product(f"product L{L} B{batch} {H}x{W} G={'yes' if g is not None else 'none'}", hip, E0, g, Mu)


@pytest.mark.parametrize("L", [5, 64, 300])                      # 300: the streaming kernel, a thread per pixel
def test_uniform_and_softmax_short_float4_tiles(L):
    import phl

    for H, W in VEC_SIZES:
        E0, G, _ = inputs(L, H, W, seed=3 * L + W)
        assert on_float4_path(E0, G)
        M64 = 0.3 * torch.ones((L, L), dtype=torch.float64, device=DEV) - 1.7 * torch.eye(L, dtype=torch.float64, device=DEV)
        for g in (G, None):
            name = f"L{L} {H}x{W} G={'yes' if g is not None else 'none'}"
            with launch_spy() as seen:
                hip = phl.nchw_softmax_compat(E0, g, uniform=(0.3, -1.7))
            assert seen == [("phl_nchw_softmax_compat", UNIFORM)]
            check_product("uniform (0.3, -1.7) " + name, hip, E0, g, M64.float(), M64)
            with launch_spy() as seen:
                q = phl.nchw_softmax_compat(E0, g)
            assert seen == [("phl_nchw_softmax_compat", SOFTMAX)]
            want = F.softmax(-energy(E0.double(), None if g is None else g.double()), 1)
            err, colsum = float((q.double() - want).abs().max()), float((q.sum(1) - 1).abs().max())
            print(f"softmax {name}: err = {err:.3e}  |colsum - 1| = {colsum:.3e}")
            assert torch.isfinite(q).all() and err <= 2e-6 and colsum <= 1e-5


@pytest.mark.parametrize("L", [18, 64])                          # VALU, matrix cores
def test_dword_fallback_for_a_base_off_the_16_byte_grid(L):
    """n % 4 == 0 with one of E0, G, out off the 16-byte grid takes the dword loads and stores; nothing else differs
    between the two forms, so the bits are those of the aligned call."""
    import phl

    H, W = VEC_SIZES[0]
    E0, G, Mu = inputs(L, H, W, seed=L + 40)
    want = phl.nchw_softmax_compat(E0, G, Mu)
    assert on_float4_path(E0, G, want)
    assert torch.equal(phl.nchw_softmax_compat(shifted(E0), G, Mu), want)
    assert torch.equal(phl.nchw_softmax_compat(E0, shifted(G), Mu), want)
    out = shifted(torch.full(E0.shape, float("nan"), device=DEV))
    assert phl.nchw_softmax_compat(E0, G, Mu, out=out) is out and torch.equal(out, want)
    check_product(f"product L{L} {H}x{W}, out off the 16-byte grid", out, E0, G, Mu)


@pytest.mark.parametrize("L", [18, 64])
@pytest.mark.parametrize("H,W", VEC_SIZES[:2])
def test_nothing_written_behind_out(H, W, L):
    """``out`` as a view at the front of a larger buffer: a short last tile leaves the 4096 floats behind it alone."""
    import phl

    E0, G, Mu = inputs(L, H, W, seed=L + 50)
    want = phl.nchw_softmax_compat(E0, G, Mu)
    sentinel, pad = -12345.5, 4096
    buf = torch.full((E0.numel() + pad,), sentinel, device=DEV)
    out = buf[:E0.numel()].view(E0.shape)
    assert on_float4_path(E0, G, out)
    assert phl.nchw_softmax_compat(E0, G, Mu, out=out) is out
    assert torch.equal(out, want)
    assert torch.equal(buf[E0.numel():], torch.full((pad,), sentinel, device=DEV))


def test_label_ranges():
    import phl

    E0, G, Mu = inputs(257, 7, 9, seed=1)
    with pytest.raises(phl.PhlError) as e:
        phl.nchw_softmax_compat(E0, G, Mu)
    assert e.value.status == phl.ERR_UNSUPPORTED
    E0 = torch.zeros((1, 1025, 7, 9), device=DEV)
    with pytest.raises(phl.PhlError) as e:
        phl.nchw_softmax_compat(E0, None, uniform=(1.0, -1.0))
    assert e.value.status == phl.ERR_UNSUPPORTED
    assert phl.nchw_softmax_compat(torch.zeros((2, 5, 0, 3), device=DEV), None, Mu[:5, :5]).shape == (2, 5, 0, 3)


def test_arguments():
    import phl

    L, H, W = 18, 13, 18
    g = torch.Generator(device=DEV).manual_seed(11)
    E0 = (torch.rand((B, H, W, L), device=DEV, generator=g) * 30 - 5).permute(0, 3, 1, 2)       # a permuted view
    G = (torch.randn((B, L, H, 2 * W), device=DEV, generator=g) * 5)[..., ::2]                  # a strided slice
    Mu = inputs(L, 1, 1, seed=5)[2]
    assert not E0.is_contiguous() and not G.is_contiguous()
    hip = phl.nchw_softmax_compat(E0, G, Mu)
    check_product("non-contiguous inputs", hip, E0, G, Mu)
    out = torch.full((B, L, H, W), float("nan"), device=DEV)
    again = phl.nchw_softmax_compat(E0, G, Mu, out=out)
    assert again is out and torch.equal(out, hip)                           # two calls, the same bits
    flat = phl.nchw_softmax_compat(E0.reshape(B, L, H * W), G.reshape(B, L, H * W), Mu)      # [B, L, n]
    assert flat.shape == (B, L, H * W) and torch.equal(flat.reshape(B, L, H, W), hip)
    for L2 in (64, 256):                                                    # ... on the matrix cores as well
        E2, G2, Mu2 = inputs(L2, 16, 24, seed=L2)
        assert torch.equal(phl.nchw_softmax_compat(E2, G2, Mu2), phl.nchw_softmax_compat(E2, G2, Mu2))
    Gc = G.contiguous()
    with pytest.raises(phl.PhlError) as e:
        phl.nchw_softmax_compat(E0, Gc, Mu, out=Gc)
    assert e.value.status == 1
    with pytest.raises(TypeError):
        phl.nchw_softmax_compat(E0, G, Mu, out=out[:, :, :, ::2])
    with pytest.raises(TypeError):
        phl.nchw_softmax_compat(E0.double(), None, Mu)


# ---- the loop ---------------------------------------------------------------------------------------------------------
def test_loop_on_the_crfasrnn_fixture():
    from crf.crf_module import CRFasRNN, charb

    z = load_case("crfasrnn_guided")
    assert float(z["gamma"]) == 3.0 and int(z["niters"]) == 3 and z["logits"].shape[1] == 16
    net = CRFasRNN(charb(3.0), niters=3)
    with torch.no_grad():
        net.W.omega.copy_(torch.from_numpy(z["omega"]))
    net = net.to(DEV)
    refs, logits, labels = (torch.from_numpy(z[k]).to(DEV) for k in ("x", "logits", "labels"))
    new, old = both_loops(lambda: net(refs, logits, labels=labels), net.niters)
    report_loop("crfasrnn_guided", new, old, torch.from_numpy(z["out"]).to(DEV))


def test_loop_on_the_upsampler_call_shape():
    """CRFdepthUpsampler's call (crf/mb_stereo_crf.py): 18 labels on a linspace, a 0/1 confidence, an rgb guide."""
    from crf.crf_module import CRFasRNN, charb

    g = torch.Generator(device=DEV).manual_seed(21)
    net = CRFasRNN(charb(.05), niters=2, r=15, eps=1e-2, gchannels=3).to(DEV)
    img = torch.rand((1, 3, 45, 83), device=DEV, generator=g)
    up = torch.rand((1, 1, 45, 83), device=DEV, generator=g) * 40
    up = torch.where(torch.rand((1, 1, 45, 83), device=DEV, generator=g) < 0.2, torch.zeros_like(up), up)
    labels = torch.linspace(0, float(up.max()), 18, device=DEV)
    with torch.no_grad():
        logits = -10 * net.Mu.get_energies_from_scalar(up, labels[None, :, None, None])
    confidence = (up > 1e-2).float()
    assert tuple(logits.shape) == (1, 18, 45, 83) and 0 < float(confidence.mean()) < 1
    new, old = both_loops(lambda: net(img, logits, confidence=confidence, labels=labels), net.niters)
    with torch.no_grad():
        want = net.double()(img.double(), logits.double(), confidence=confidence.double(), labels=labels.double())
    net.float()
    report_loop("upsampler shape L18", new, old, want)


def test_loop_with_potts():
    from crf.crf_module import CRFasRNN, potts

    g = torch.Generator(device=DEV).manual_seed(22)
    net = CRFasRNN(potts(8), niters=3, notrain_mu=True).to(DEV)
    refs = torch.rand((2, 1, 40, 50), device=DEV, generator=g)
    logits = torch.randn((2, 8, 40, 50), device=DEV, generator=g) * 3
    with launch_spy() as seen:
        new, old = both_loops(lambda: net(refs, logits), net.niters)
    modes = [m for name, m in seen if name == "phl_nchw_softmax_compat"]
    assert modes == [UNIFORM] * 3 + [LOGITS], modes
    with torch.no_grad():
        want = net.double()(refs.double(), logits.double())
    net.float()
    report_loop("potts(8)", new, old, want)


def test_routing_keeps_the_plain_loop():
    """Autograd, float64 and CPU tensors never reach the new kernel, and compute exactly what the plain loop computes."""
    from crf.crf_module import CRFasRNN, charb

    g = torch.Generator(device=DEV).manual_seed(23)
    refs = torch.rand((1, 1, 20, 30), device=DEV, generator=g)
    logits = torch.randn((1, 5, 20, 30), device=DEV, generator=g) * 3
    net = CRFasRNN(charb(3.0), niters=2, r=4).to(DEV)

    def run(net, refs, logits):
        labels = torch.arange(5, dtype=logits.dtype, device=logits.device)    # charb's own default labels are fp32
        with loop_spy() as calls:
            out = net(refs, logits, labels=labels)
        assert calls["step"] == 0 and calls["softmax"] == 3, calls
        with old_loop():
            assert torch.equal(out.detach(), net(refs, logits, labels=labels).detach())

    run(net, refs, logits.clone().requires_grad_())           # a gradient of the logits
    run(net, refs, logits)                                    # grad mode on: Mu's and W's parameters ask for one
    with torch.no_grad():
        run(net.double(), refs.double(), logits.double())
        run(net.float().cpu(), refs.cpu(), logits.cpu())
