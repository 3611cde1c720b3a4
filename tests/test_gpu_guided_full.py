"""The full-covariance guided filter on the HIP kernels (phl.guided_filter(full_cov=True), phl_guided.hip:
k_guide_stats_full, k_guide_coef_full).

Rule of every accuracy check, the one of tests/test_gpu_guided.py through _guided_util.report: with the float64 torch form
on the device as the target, e_hip <= e_torch with no margin, e_torch the fp32 full-covariance torch form on the same
device; every case under the precondition e_torch >= 8 u, u = 2^-24 max|want|, so that the rule has something to judge.
Every sweep runs on two guides: independent uniform channels, and the correlated guide base + 0.25 noise_c.  On the
correlated guide the kernels' result must also differ from the diagonal kernels' by at least 1000 e_hip -- kernels that
dropped the off-diagonal terms cannot pass that.  (Not where the model has no off-diagonal term to use: one guide channel,
or a window of one pixel, r // s == 0, where cov and S vanish identically and both models give A = 0.)  e_hip is printed
in u for every case."""
import pytest
import torch

import _guided_util as util
from _guided_fixtures import load_case
from _guided_util import DEV, GUIDES, NEAREST_FULL, affine_inputs, correlated_guide, full_case, report, route, spy, torch_form

pytestmark = pytest.mark.gpu


def _max_r():
    import phl

    return phl.load_library().phl_guided_filter_max_r()


@pytest.mark.parametrize("guide", GUIDES)
@pytest.mark.parametrize("s", [1, 2, 3])
@pytest.mark.parametrize("r", [1, 4, 20, 100])
def test_radius_and_subsample(r, s, guide):
    full_case("gf" if s == 1 else "bga", 3, 5, 3, 61, 75, r, s, 1e-2, guide, seed=r + s)


@pytest.mark.parametrize("guide", GUIDES)
@pytest.mark.parametrize("dr", [0, 1, 25])
def test_both_sides_of_the_tiled_radius(dr, guide):
    r = _max_r() + dr
    full_case("gf", 1, 2, 3, 203, 171, r, 1, 1e-2, guide, seed=dr)
    full_case("bga", 2, 3, 4, 203, 171, 2 * r, 2, 1e-5, guide, seed=dr + 1)


@pytest.mark.parametrize("guide", GUIDES)
@pytest.mark.parametrize("cx", [1, 2, 3, 4])
@pytest.mark.parametrize("cy", [1, 5, 64])
def test_channels(cy, cx, guide):
    full_case("fast", 3, cy, cx, 45, 83, 4, 2, 1e-2, guide, seed=cy + cx)


def test_five_channels_fall_back_to_the_torch_form():
    import phl
    from crf import guided

    g = torch.Generator(device=DEV).manual_seed(5)
    y = torch.rand((1, 2, 30, 40), device=DEV, generator=g)
    x = correlated_guide(1, phl.GUIDED_FULL_MAX_CX + 1, 30, 40, g, DEV)
    with pytest.raises(phl.PhlError) as e:
        phl.guided_filter(y, x, 2, 1e-2, full_cov=True)
    assert e.value.status == 7 and "phl_guided_filter_full" in str(e.value)
    for m in (guided.GuidedFilter(5, 2, 1e-2, full_cov=True).to(DEV), guided.BatchedGuidedAdjacency(5, 2, 1e-2, full_cov=True).to(DEV)):
        with torch.no_grad(), spy() as calls:
            out = m(y, x)
        assert calls == route(nearest=1, box_sum=calls["box_sum"]) and calls["box_sum"] > 0          # one attempt, then the torch form
        with torch.no_grad(), torch_form():
            assert torch.equal(out, m(y, x))


@pytest.mark.parametrize("guide", GUIDES)
def test_window_of_one_pixel(guide):
    full_case("fast", 1, 5, 3, 33, 70, 1, 2, 1e-2, guide)                  # r // s == 0


@pytest.mark.parametrize("guide", GUIDES)
def test_noncontiguous_and_out(guide):
    full_case("bga", 3, 5, 3, 61, 75, 4, 2, 1e-2, guide, noncontiguous=True)
    full_case("bga", 2, 5, 3, 61, 75, 4, 2, 1e-2, guide, use_out=True)
    full_case("gf", 2, 5, 2, 40, 130, 4, 1, 1e-2, guide, use_out=True)


def test_chunk_boundary_inside_an_image():
    """B * cy above the labels of one chunk (the chunks are those of the diagonal form: cx + 1 fp32 planes a label), the
    boundary inside the second image; the labels around it, filtered in a call of their own, give the same bits."""
    import phl

    B, cy, cx, H, W, r = 2, 75, 3, 256, 192, 8
    per = phl.guided_filter_labels_per_chunk(B, cy, cx, H, W, full=True)
    nchunks = -(-B * cy // per)
    print(f"{per} labels per chunk of {B} x {cy}: {nchunks} chunks")
    assert nchunks >= 2 and per % cy != 0
    res = full_case("bga", B, cy, cx, H, W, r, 1, 1e-5, "correlated", seed=1)
    l = per % cy
    ys = res["y"][:, l - 4:l + 4].contiguous()
    alone = phl.guided_filter(ys, res["x"], r, res["m"].eps.detach(), scale=0.5 * (2 * r + 1) ** 2, subtract=ys, full_cov=True)
    assert torch.equal(alone, res["hip"][:, l - 4:l + 4])


@pytest.mark.parametrize("eps", [1e-2, 1e-4])
@pytest.mark.parametrize("name", ["gf_tsukuba", "gf_r4"])
def test_natural_images(name, eps):
    from crf import guided

    z = load_case(name)
    y, x = torch.from_numpy(z["y"]).to(DEV), torch.from_numpy(z["x"]).to(DEV)
    m = guided.GuidedFilter(int(z["cx"]), int(z["r"]), eps, full_cov=True).to(DEV)
    util.check_forward(NEAREST_FULL, f"full {name} eps{eps:g}", m, y, x, off_diagonal=name == "gf_tsukuba")        # (gf_r4: a random guide)


def test_affine_reproduction_on_the_kernels():
    """fp32, eps = 1e-6: the float64 model's own error is 2.3e-5 (eps against the smallest eigenvalue of S); the bound is
    1e-4, four times that for the fp32 roundings of the coefficient planes.  The diagonal kernels are off by 0.14."""
    import phl

    y, x = affine_inputs(DEV, torch.float32)
    full = phl.guided_filter(y, x, 3, 1e-6, full_cov=True)
    diag = phl.guided_filter(y, x, 3, 1e-6)
    e_full, e_diag = float((full - y).abs().max()), float((diag - y).abs().max())
    print(f"affine y on the kernels: |full - y| = {e_full:.3e}  |diagonal - y| = {e_diag:.3e}")
    assert e_full <= 1e-4
    assert e_diag >= 1e-2


def test_deterministic():
    g = torch.Generator(device=DEV).manual_seed(4)
    y = torch.rand((2, 7, 131, 257), device=DEV, generator=g)
    x = correlated_guide(2, 3, 131, 257, g, DEV)
    util.check_deterministic(NEAREST_FULL, y, x)


def test_crfasrnn_full_cov_without_grad():
    """CRFasRNN's loop with the full-covariance W: one kernel call per iteration, and the end-to-end rule of
    tests/test_gpu_guided.py (e_hip <= 2 e_torch against the float64 loop; the fp32 compatibility and softmax steps are
    common to both paths)."""
    from crf.crf_module import CRFasRNN, charb

    z = load_case("crfasrnn_guided")
    g = torch.Generator(device=DEV).manual_seed(8)
    x1 = torch.from_numpy(z["x"]).to(DEV)
    refs = torch.cat([x1, x1 + 0.1 * torch.rand(x1.shape, device=DEV, generator=g), x1 + 0.1 * torch.rand(x1.shape, device=DEV, generator=g)], 1)
    logits, labels = torch.from_numpy(z["logits"]).to(DEV), torch.from_numpy(z["labels"]).to(DEV)
    net = CRFasRNN(charb(3.), niters=3, gchannels=3, full_cov=True).to(DEV)
    with torch.no_grad(), spy() as calls:
        hip = net(refs, logits, labels=labels)
    assert calls == route(nearest=3)
    with torch.no_grad(), torch_form():
        t32 = net(refs, logits, labels=labels)
        want = net.double()(refs.double(), logits.double(), labels=labels.double())
    report("crfasrnn full_cov", hip, t32, want, factor=2)


def test_autograd_keeps_the_torch_form():
    """With autograd recording the torch form runs -- also with fused_grad=True: this model has no backward kernel -- and
    its fp32 gradients are those of the float64 torch form within 1e-3 of each gradient's largest magnitude (the bound and
    the reasoning of tests/test_gpu_guided.py::test_autograd_keeps_the_torch_form)."""
    g = torch.Generator(device=DEV).manual_seed(6)
    y = torch.rand((1, 3, 40, 50), device=DEV, generator=g, requires_grad=True)
    x = correlated_guide(1, 3, 40, 50, g, DEV)
    util.check_autograd_keeps_the_torch_form(NEAREST_FULL, y, x, "full_cov grad", fused_grad=True)
