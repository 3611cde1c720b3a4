"""The box-window guided filter on the HIP kernels (phl.guided_filter, phl_guided.hip).

Rule of every accuracy check: with g the float64 result (the reference's fixture, or the torch form in float64 on the
device), e_hip = max|hip - g| and e_torch = max|fp32 torch form - g| over ALL elements, measured on the same device, and
e_hip <= e_torch with no margin -- fp64 window sums must beat fp32 prefix sums.  The two multi-iteration fixtures
(CRFasRNN, mean_field_infer) are held to e_hip <= 2 e_torch: the fp32 compatibility and softmax steps are common to both
paths.  Both numbers are printed."""
import pytest
import torch

import _guided_util as util
from _guided_fixtures import CASES, END_TO_END, build_module, load_case
from _guided_util import DEV, NEAREST, route, spy, torch_form
from _guided_util import report as _report
from _guided_util import sweep_case as _sweep_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", [c for c in CASES if c not in END_TO_END])
def test_goldens(name):
    from crf import guided

    z = load_case(name)
    m = build_module(guided, z, torch.float32, DEV)
    y, x = torch.from_numpy(z["y"]).to(DEV), torch.from_numpy(z["x"]).to(DEV)
    with torch.no_grad(), spy() as calls:
        hip = m(y, x)
    assert calls == route(nearest=1)
    with torch.no_grad(), torch_form():
        t32 = m(y, x)
    _report(name, hip, t32, torch.from_numpy(z["out"]).to(DEV))


def test_golden_crfasrnn_default_w():
    from crf.crf_module import CRFasRNN, charb

    z = load_case("crfasrnn_guided")
    net = CRFasRNN(charb(float(z["gamma"])), niters=int(z["niters"]))
    with torch.no_grad():
        net.W.omega.copy_(torch.from_numpy(z["omega"]))
    net = net.to(DEV)
    refs, logits, labels = (torch.from_numpy(z[k]).to(DEV) for k in ("x", "logits", "labels"))
    with torch.no_grad(), spy() as calls:
        hip = net(refs, logits, labels=labels)
    assert calls == route(nearest=int(z["niters"]))
    with torch.no_grad(), torch_form():
        t32 = net(refs, logits, labels=labels)
    _report("crfasrnn_guided", hip, t32, torch.from_numpy(z["out"]).to(DEV), factor=2)


def test_golden_mean_field_guided_adjacency():
    from crf.crf_module import mean_field_infer
    from crf.guided import GuidedAdjacency

    z = load_case("meanfield_guided")
    W = GuidedAdjacency(torch.from_numpy(z["x"]).to(DEV), int(z["r"]), float(z["eps"]))
    with torch.no_grad():
        W.omega.copy_(torch.from_numpy(z["omega"]))
    W = W.to(DEV)
    E0, Mu = torch.from_numpy(z["E0"]).to(DEV), torch.from_numpy(z["Mu"]).to(DEV)
    with torch.no_grad(), spy() as calls:
        hip = mean_field_infer(E0, W, Mu, int(z["niters"]))
    assert calls == route(nearest=int(z["niters"]))
    with torch.no_grad(), torch_form():
        t32 = mean_field_infer(E0, W, Mu, int(z["niters"]))
    _report("meanfield_guided", hip, t32, torch.from_numpy(z["out"]).to(DEV), factor=2)


@pytest.mark.parametrize("s", [1, 2, 3])
@pytest.mark.parametrize("r", [1, 4, 20, 100])
def test_sweep_radius_and_subsample(r, s):
    kind = "gf" if s == 1 else "bga"
    _sweep_case(kind, 3, 5, 3, 61, 75, r, s, 1e-2, seed=r + s)          # odd H / W, B = 3; r = 100: larger than the image


@pytest.mark.parametrize("dr", [0, 1, 25])
def test_sweep_both_sides_of_the_tiled_radius(dr):
    """The largest radius of the LDS-tiled form (its LDS is within a few hundred bytes of a CU's 160 KiB), the first of
    the streamed form, and one well above, on an image larger than the window and several strips high."""
    import phl

    r = phl.load_library().phl_guided_filter_max_r() + dr
    _sweep_case("gf", 1, 2, 3, 203, 171, r, 1, 1e-2, seed=dr)
    _sweep_case("bga", 2, 3, 1, 203, 171, 2 * r, 2, 1e-5, seed=dr + 1)


@pytest.mark.parametrize("cx", [1, 3, 16])
@pytest.mark.parametrize("cy", [1, 5, 64])
def test_sweep_channels(cy, cx):
    _sweep_case("fast", 3, cy, cx, 45, 83, 4, 2, 1e-2, seed=cy + cx)


def test_sweep_window_of_one_pixel():
    _sweep_case("fast", 1, 5, 3, 33, 70, 1, 2, 1e-2)                      # r // s == 0
    _sweep_case("bga", 2, 2, 1, 33, 70, 2, 3, 1e-2)


def test_sweep_noncontiguous_and_out():
    _sweep_case("bga", 3, 5, 3, 61, 75, 4, 2, 1e-2, noncontiguous=True)
    _sweep_case("bga", 2, 5, 3, 61, 75, 4, 2, 1e-2, use_out=True)
    _sweep_case("gf", 2, 5, 1, 40, 130, 4, 1, 1e-2, use_out=True)


def test_sweep_large_image():
    _sweep_case("bga", 1, 8, 1, 1110, 1390, 20, 2, 1e-5)


def test_deterministic():
    g = torch.Generator(device=DEV).manual_seed(4)
    y = torch.rand((2, 7, 131, 257), device=DEV, generator=g)
    x = torch.rand((2, 16, 131, 257), device=DEV, generator=g)
    util.check_deterministic(NEAREST, y, x)


def test_unsupported_shapes_fall_back_to_torch():
    import phl
    from crf import guided

    g = torch.Generator(device=DEV).manual_seed(5)
    y = torch.rand((1, 2, 30, 40), device=DEV, generator=g)
    x = torch.rand((1, 17, 30, 40), device=DEV, generator=g)
    with pytest.raises(phl.PhlError) as e:
        phl.guided_filter(y, x, 2, 1e-2)
    assert e.value.status == 7
    for m in (guided.GuidedFilter(17, 2, 1e-2).to(DEV), guided.BatchedGuidedAdjacency(17, 2, 1e-2).to(DEV)):
        with torch.no_grad(), spy() as calls:
            out = m(y, x)
        assert calls == route(nearest=1, box_sum=calls["box_sum"]) and calls["box_sum"] > 0          # one attempt, then the torch form
        with torch.no_grad(), torch_form():
            assert torch.equal(out, m(y, x))


def test_autograd_keeps_the_torch_form():
    """With autograd recording the torch form runs (no kernel call), and its fp32 gradients are those of the float64
    torch form.  Bound: 1e-3 of each gradient's largest magnitude.  The fp32 forward at this size is 2e-5 relative from
    float64 (prefix sums, measured for the 48 x 64 fixture); the backward passes through the same box sums once more
    and through 1 / (var + eps) twice, and 1e-3 leaves a factor of 50 over the forward's error for that."""
    g = torch.Generator(device=DEV).manual_seed(6)
    y = torch.rand((1, 3, 40, 50), device=DEV, generator=g, requires_grad=True)
    x = torch.rand((1, 3, 40, 50), device=DEV, generator=g)
    util.check_autograd_keeps_the_torch_form(NEAREST, y, x, "grad")


def test_gaussian_and_bilinear_never_reach_the_kernels():
    from crf import guided

    g = torch.Generator(device=DEV).manual_seed(7)
    y = torch.rand((1, 2, 40, 50), device=DEV, generator=g)
    x = torch.rand((1, 1, 40, 50), device=DEV, generator=g)
    with torch.no_grad(), spy() as calls:
        guided.GuidedFilter(1, 2, 1e-2, gaussian=True).to(DEV)(y, x)
        guided.FastGuidedFilter(1, 4, 1e-2, mode="bilinear").to(DEV)(y, x)
        guided.BatchedGuidedAdjacency(1, 4, 1e-2, mode="bilinear").to(DEV)(y, x)
        guided.GuidedFilter(1, 2, 1e-2).double().to(DEV)(y.double(), x.double())
        guided.GuidedFilter(1, 2, 1e-2)(y.cpu(), x.cpu())
    assert calls == route(box_sum=calls["box_sum"])
