"""The label-chunk loop of the box-window guided filter (phl_guided.hip: forward(), backward()) with chunk boundaries inside
an image.

The labels B * cy of a call are processed in chunks that keep the per-label temporaries within a fixed budget.  Every
case here first asks the library how many labels a chunk of that very call holds (phl.guided_filter_labels_per_chunk,
the function forward() and backward() size their chunks with) and asserts that there is more than one chunk, that a chunk
boundary lies inside an image, that some chunk holds labels of two images and that some chunk starts inside an image: the
`n0 > 0`, `b = n / cy`, `na` / `nb` arithmetic and the accumulate-or-overwrite branch of k_grad_reduce / k_grad_direct.

Rule of every accuracy check, the one of tests/test_gpu_guided.py unchanged: e_hip <= e_torch with no margin, both
against the float64 torch form on the device.  The rule judges only where the fp32 torch form errs, so each case also
asserts a precondition on its input: e_torch >= 8 u, u = 2^-24 * max|want| (8 = four times the forward kernels' largest
recorded error).  A label's output and its grad_y depend on its own plane and on per-image statistics only:
those are compared bit for bit between calls that chunk differently.  Every figure is printed."""
import functools

import pytest
import torch

from _guided_util import DEV, report, sweep_case, sweep_case_grad, torch_form

pytestmark = pytest.mark.gpu

MIN_U = 8

#           kind  B  cy   cx  H    W    r  s  eps
FORWARD = [("bga", 2, 150, 1, 256, 192, 8, 1, 1e-5),        # chunks of 256 + 44 labels
           ("bga", 2, 50, 16, 256, 256, 8, 2, 1e-2)]        # 90 + 10, five passes of k_guide_apply's plane groups
BACKWARD = [("gf", 2, 7, 16, 128, 128, 4, 1, 1e-2),         # 9 + 5, full resolution: ys = y + n0 * HWf
            ("bga", 3, 20, 3, 256, 256, 8, 2, 1e-2)]        # 46 + 14: the first chunk ends inside the third image
ALL = dict(need_y=True, need_x=True, need_eps=True)


def _boundary(B, cy, per):
    """The checks of the chunk layout named in the header; (image, label in it) of the first chunk boundary."""
    nimg = B * cy
    print(f"{per} labels per chunk of {B} x {cy}")
    assert 0 < per < nimg
    assert per % cy != 0
    chunks = [(n0, min(nimg, n0 + per)) for n0 in range(0, nimg, per)]
    assert any(n0 // cy != (n1 - 1) // cy for n0, n1 in chunks), chunks         # labels of two images in one launch
    assert any(n0 % cy != 0 for n0, _ in chunks), chunks                        # a chunk that starts inside an image
    return per // cy, per % cy


def _per_chunk(case, **needs):
    import phl

    kind, B, cy, cx, H, W, r, s, eps = case
    return phl.guided_filter_labels_per_chunk(B, cy, cx, H // s, W // s, full=s == 1, **needs)


def _label_ranges(cy, l):
    """Labels of the boundary's image on both sides of the boundary, and labels wholly behind it."""
    return [(max(0, l - 6), min(cy, l + 6)), (l + 1, min(cy, l + 7))]


def _call_args(case, m):
    kind, B, cy, cx, H, W, r, s, eps = case
    return dict(subsample=s, scale=0.5 * (2 * r + 1) ** 2 if kind == "bga" else 1.0), kind == "bga", r, m.eps.detach()


def _forward_labels_alone(case, res):
    """Bit for bit: the labels around the chunk boundary filtered in a call of their own (one chunk)."""
    import phl

    kind, B, cy, cx, H, W, r, s, eps = case
    b, l = _boundary(B, cy, _per_chunk(case))
    kw, sub, r, e = _call_args(case, res["m"])
    for l0, l1 in _label_ranges(cy, l):
        ys = res["y"][:, l0:l1].contiguous()
        assert phl.guided_filter_labels_per_chunk(B, l1 - l0, cx, H // s, W // s) == B * (l1 - l0)
        alone = phl.guided_filter(ys, res["x"], r, e, subtract=ys if sub else None, **kw)
        assert torch.equal(alone, res["hip"][:, l0:l1]), (res["name"], l0, l1)


@pytest.mark.parametrize("case", FORWARD, ids=["cx1", "cx16"])
def test_forward_tiled(case):
    _boundary(case[1], case[2], _per_chunk(case))
    res = sweep_case(*case, seed=1, min_torch_u=MIN_U)
    _forward_labels_alone(case, res)


def test_forward_streamed():
    import phl

    kind, B, cy, cx, H, W, _, s, eps = FORWARD[0]
    case = ("gf", B, cy, cx, H, W, phl.load_library().phl_guided_filter_max_r() + 1, s, eps)
    _boundary(B, cy, _per_chunk(case))
    res = sweep_case(*case, seed=2, min_torch_u=MIN_U)
    _forward_labels_alone(case, res)


def _eps_grad_torch(m, y, x, g, dtype):
    """d sum(m(y, x) g) / d eps in the torch form, with eps = softplus(omega) itself as the leaf, in ``dtype``."""
    from crf import guided

    eps = m.eps.detach().to(dtype).requires_grad_(True)
    real = guided.GuidedFilter.eps
    guided.GuidedFilter.eps = property(lambda self: eps)
    try:
        with torch_form():
            (m(y.to(dtype), x.to(dtype)) * g.to(dtype)).sum().backward()
    finally:
        guided.GuidedFilter.eps = real
    return eps.grad


@functools.lru_cache(maxsize=None)
def _backward(i):
    """A backward case under the rule (all three gradients in one kernel call); its tensors, shared by the tests below."""
    case = BACKWARD[i]
    _boundary(case[1], case[2], _per_chunk(case, **ALL))
    return sweep_case_grad(*case, seed=3 + i, min_torch_u=MIN_U)


@pytest.mark.parametrize("i", range(len(BACKWARD)), ids=["gf_full", "bga_s2"])
def test_backward(i):
    _backward(i)


@pytest.mark.parametrize("i", range(len(BACKWARD)), ids=["gf_full", "bga_s2"])
def test_backward_labels_alone(i):
    """grad_y, bit for bit: the labels around the chunk boundary in a call of their own."""
    import phl

    case, res = BACKWARD[i], _backward(i)
    kind, B, cy, cx, H, W, r, s, eps = case
    b, l = _boundary(B, cy, _per_chunk(case, **ALL))
    kw, sub, r, e = _call_args(case, res["m"])
    for l0, l1 in _label_ranges(cy, l):
        ys, gs = res["y"][:, l0:l1].contiguous(), res["g"][:, l0:l1].contiguous()
        assert phl.guided_filter_labels_per_chunk(B, l1 - l0, cx, H // s, W // s, full=s == 1, need_y=True) == B * (l1 - l0)
        gy, _, _ = phl.guided_filter_grad(ys, res["x"], gs, r, e, subtract_is_y=sub, **kw)
        assert torch.equal(gy, res["hip"][0][:, l0:l1]), (res["name"], l0, l1)


def test_backward_need_flags():
    """The need flags change the bytes of a label and with them the chunking of the same tensors.  grad_y is per label:
    the same bits whatever the flags.  grad_eps is summed over the labels chunk by chunk, so its bits may differ with
    the chunking: each is held to the accuracy rule against float64 autograd."""
    import phl

    case, res = BACKWARD[0], _backward(0)
    kind, B, cy, cx, H, W, r, s, eps = case
    m, y, x, g = res["m"], res["y"], res["x"], res["g"]
    kw, sub, r, e = _call_args(case, m)
    per_all = _per_chunk(case, **ALL)
    per_ye = _per_chunk(case, need_y=True, need_eps=True)
    _boundary(B, cy, per_ye)                                    # nsel = 2: no A, no mA, more labels per chunk
    assert per_ye != per_all
    _boundary(B, cy, _per_chunk(case, need_eps=True))
    full = phl.guided_filter_grad(y, x, g, r, e, subtract_is_y=sub, **ALL, **kw)
    assert torch.equal(full[0], res["hip"][0]) and torch.equal(full[1], res["hip"][1])       # the module made this call
    ge32, ge64 = _eps_grad_torch(m, y, x, g, torch.float32), _eps_grad_torch(m, y, x, g, torch.float64)
    report(f"{res['name']} grad_eps, all needs", full[2], ge32, ge64, what="grad", min_torch_u=MIN_U)
    for needs in (dict(need_y=True), dict(need_y=False, need_eps=True), dict(need_y=True, need_eps=True)):
        gy, gx, ge = phl.guided_filter_grad(y, x, g, r, e, subtract_is_y=sub, **needs, **kw)
        assert gx is None and (gy is None) == (not needs["need_y"]) and (ge is None) == ("need_eps" not in needs)
        if gy is not None:
            assert torch.equal(gy, full[0]), needs
        if ge is not None:
            report(f"{res['name']} grad_eps, {needs}", ge, ge32, ge64, what="grad", min_torch_u=MIN_U)
