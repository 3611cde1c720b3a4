"""Edge shapes of the box-window guided filter's tile routine (phl_guided.hip), forward and backward: a solving resolution
one pixel high or wide, exactly one 32 x 64 tile and one pixel past it in both axes, and the streamed form (radius above
phl_guided_filter_max_r) on images a few rows or columns thick, where a 64-row strip is almost empty.

Rule of every accuracy check, the one of tests/test_gpu_guided.py unchanged: e_hip <= e_torch with no margin, both
against the float64 torch form on the device.  The rule judges only where the fp32 torch form errs, so each case also
asserts a precondition on its input: e_torch >= 8 u, u = 2^-24 * max|want| (8 = four times the forward kernels' largest
recorded error).  Shapes at which fp32 prefix sums are exact or nearly so (a 1 x 1 image, 2 x 3 at subsample 2,
3 x 3) cannot be judged by the rule and get no accuracy case; the 1 x 1 image is checked exactly instead.  Every figure is
printed."""
import pytest
import torch

from _guided_util import DEV, sweep_case, sweep_case_grad

pytestmark = pytest.mark.gpu

MIN_U = 8
B, CY, EPS = 2, 3, 1e-2
STREAMED = None          # r: the first radius of the streamed form


#        kind   cx  H     W    r         s
CASES = [("gf", 3, 1, 130, 4, 1),              # h = 1, three tile columns
         ("gf", 3, 130, 1, 4, 1),              # w = 1, five tile rows
         ("bga", 3, 2, 131, 4, 2),             # low resolution 1 x 65
         ("bga", 1, 67, 3, 6, 3),              # low resolution 22 x 1
         ("gf", 3, 32, 64, 4, 1),              # exactly one tile
         ("bga", 3, 64, 128, 4, 2),            # low resolution exactly one tile
         ("gf", 3, 33, 65, 4, 1),              # one past the tile in both axes
         ("bga", 2, 66, 130, 9, 2),            # low resolution 33 x 65
         ("gf", 3, 1, 2000, STREAMED, 1),      # streamed, h = 1
         ("gf", 3, 1500, 2, 40, 1),            # streamed, w = 2
         ("bga", 1, 4, 1500, 80, 2)]           # streamed, low resolution 2 x 750
IDS = [f"{c[0]}_cx{c[1]}_{c[2]}x{c[3]}_r{c[4] or 'stream'}_s{c[5]}" for c in CASES]


def _args(case, i):
    import phl

    kind, cx, H, W, r, s = case
    max_r = phl.load_library().phl_guided_filter_max_r()
    if r is STREAMED:
        r = max_r + 1
    assert (min(r // s, max(H // s, W // s)) > max_r) == (i >= 8)          # the form the table of cases says
    return (kind, B, CY, cx, H, W, r, s, EPS), dict(seed=20 + i, min_torch_u=MIN_U)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_forward(i):
    args, kw = _args(CASES[i], i)
    sweep_case(*args, **kw)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_backward(i):
    args, kw = _args(CASES[i], i)
    sweep_case_grad(*args, **kw)


@pytest.mark.parametrize("r", [0, 4, 100])
def test_image_of_one_pixel_is_exact(r):
    """The window holds one pixel: mean(y x) - mean(y) mean(x) is exactly 0 in fp64 (a product of two fp32 values is exact
    there), so A = 0, b = y and the filter returns y itself; with scale and subtract, one rounding of y k - y."""
    import phl

    gen = torch.Generator(device=DEV).manual_seed(30 + r)
    y = torch.rand((2, 3, 1, 1), device=DEV, generator=gen) * 7 - 2
    x = torch.rand((2, 3, 1, 1), device=DEV, generator=gen)
    assert torch.equal(phl.guided_filter(y, x, r, EPS), y)
    k = 0.5 * (2 * r + 1) ** 2
    assert float(torch.tensor(k, dtype=torch.float32)) == k                 # the kernel takes the scale as fp32
    got = phl.guided_filter(y, x, r, EPS, scale=k, subtract=y)
    assert torch.equal(got, (y.double() * k - y.double()).float())


@pytest.mark.parametrize("H,W", [(33, 65), (1, 130)])
def test_nothing_written_behind_out(H, W):
    """``out`` as a view at the front of a larger buffer: the 4096 floats behind it keep their value.  (grad_y has no such
    check: phl.guided_filter_grad allocates its gradients itself.)"""
    import phl

    gen = torch.Generator(device=DEV).manual_seed(H + W)
    y = torch.rand((B, CY, H, W), device=DEV, generator=gen)
    x = torch.rand((B, 3, H, W), device=DEV, generator=gen)
    want = phl.guided_filter(y, x, 4, EPS)
    sentinel, pad = -12345.5, 4096
    buf = torch.full((y.numel() + pad,), sentinel, device=DEV)
    out = buf[:y.numel()].view(y.shape)
    assert out.is_contiguous() and out.data_ptr() == buf.data_ptr()
    assert phl.guided_filter(y, x, 4, EPS, out=out) is out
    assert torch.equal(out, want)
    assert torch.equal(buf[y.numel():], torch.full((pad,), sentinel, device=DEV))
