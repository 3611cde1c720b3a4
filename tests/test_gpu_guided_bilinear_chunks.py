"""The label-chunk loop of phl_guided_filter_bilinear (phl_guided.hip: forward(), BL) with a chunk boundary inside an
image, in the manner of test_gpu_guided_chunks.py: the case asks the library how many labels a chunk of that very call
holds (phl.guided_filter_bilinear_labels_per_chunk, the function forward() sizes its chunks with; the window-mean
planes count beside the coefficient planes) and asserts more than one chunk and a boundary inside an image.  The accuracy
rule is that of tests/test_gpu_guided.py, e_hip <= e_torch with no margin under the precondition e_torch >= 8 u; a
label's output depends on its own plane and on per-image statistics only, so the labels on both sides of the boundary,
filtered in a call of their own, must match bit for bit.  Every figure is printed."""
import pytest
import torch

from _guided_util import BILINEAR, DEV, check_forward, module

pytestmark = pytest.mark.gpu

KIND, B, CY, CX, H, W, R, S, EPS = "bga", 2, 50, 16, 256, 256, 8, 2, 1e-2


def test_chunk_boundary_inside_an_image():
    import phl

    cy = CY
    while True:                                         # (50 labels an image do split with the formula as it stands)
        per = phl.guided_filter_bilinear_labels_per_chunk(B, cy, CX, H // S, W // S)
        if 0 < per < B * cy and per % cy != 0:
            break
        cy += 7
    nimg = B * cy
    print(f"{per} labels per chunk of {B} x {cy}")
    chunks = [(n0, min(nimg, n0 + per)) for n0 in range(0, nimg, per)]
    assert len(chunks) > 1
    assert any(n0 % cy != 0 for n0, _ in chunks), chunks                        # a chunk that starts inside an image
    gen = torch.Generator(device=DEV).manual_seed(1)
    y = torch.rand((B, cy, H, W), device=DEV, generator=gen)
    x = torch.rand((B, CX, H, W), device=DEV, generator=gen)
    m = module(KIND, CX, R, S, EPS, BILINEAR).to(DEV)
    hip, _ = check_forward(BILINEAR, f"bilinear {KIND} B{B} cy{cy} cx{CX} {H}x{W} r{R} s{S}", m, y, x)
    # the labels around the first boundary (of image 0) and labels wholly behind it, each range one chunk of its own
    b, l = per // cy, per % cy
    with torch.no_grad():
        for l0, l1 in ((max(0, l - 6), min(cy, l + 6)), (l + 1, min(cy, l + 7))):
            ys = y[:, l0:l1].contiguous()
            assert phl.guided_filter_bilinear_labels_per_chunk(B, l1 - l0, CX, H // S, W // S) == B * (l1 - l0)
            alone = phl.guided_filter_bilinear(ys, x, R, m.eps, subsample=S, scale=0.5 * (2 * R + 1) ** 2, subtract=ys)
            assert torch.equal(alone, hip[:, l0:l1]), (l0, l1)
