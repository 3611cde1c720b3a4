"""FastGuidedFilter(mode='bilinear') without a GPU: the repository's torch form in float64 against the reference's classes
run in float64 with that mode (tests/golden/guided_bil_*.npz, written by tests/golden/generate_guided_bilinear.py), the
``fused_bilinear`` keyword through the classes that take it, and the argument checks and the chunk query of
phl_guided_filter_bilinear, which return before the first HIP call.

Bound of the fixtures: that of test_guided_cpu.py, 1e-12 of the output's largest magnitude."""
import ctypes

import numpy as np
import pytest
import torch

from _guided_fixtures import BIL_CASES, build_module, load_case

BOUND = 1e-12


@pytest.mark.parametrize("name", BIL_CASES)
def test_bilinear_classes_match_reference_float64(name):
    from crf import guided

    z = load_case(name)
    assert str(z["mode"]) == "bilinear"
    y, x = torch.from_numpy(z["y"]).double(), torch.from_numpy(z["x"]).double()
    with torch.no_grad():
        out = build_module(guided, z, torch.float64, "cpu", "bilinear")(y, x)
        flagged = build_module(guided, z, torch.float64, "cpu", "bilinear", fused_bilinear=True)(y, x)
    err = float(np.abs(out.numpy() - z["out"]).max())
    print(f"{name}: max |torch float64 - reference float64| = {err:.3e}, |out| <= {np.abs(z['out']).max():.4g}")
    assert err <= BOUND * np.abs(z["out"]).max(), (name, err)
    assert torch.equal(out, flagged)                    # CPU, float64: the flag changes nothing


def test_flag_changes_nothing_on_cpu_fp32():
    from crf import guided

    g = torch.Generator().manual_seed(3)
    y, x = torch.rand((2, 3, 41, 67), generator=g), torch.rand((2, 3, 41, 67), generator=g)
    for cls in (guided.FastGuidedFilter, guided.BatchedGuidedAdjacency):
        with torch.no_grad():
            a = cls(3, 4, 1e-2, subsample_ratio=2, mode="bilinear")(y, x)
            b = cls(3, 4, 1e-2, subsample_ratio=2, mode="bilinear", fused_bilinear=True)(y, x)
        assert torch.equal(a, b)


def test_keyword_checks():
    from crf import guided
    from crf.crf_module import CRFasRNN, charb
    from crf.mb_stereo_crf import CRFdepthRefiner, CRFdepthUpsampler, CRFwUncertainty

    for cls in (guided.FastGuidedFilter, guided.BatchedGuidedAdjacency):
        with pytest.raises(ValueError):
            cls(1, 4, 1e-2, fused_bilinear=True)                         # mode defaults to 'nearest'
        with pytest.raises(ValueError):
            cls(1, 4, 1e-2, mode="bicubic", fused_bilinear=True)
        m = cls(1, 4, 1e-2, mode="bilinear", fused_bilinear=True)
        assert m.fused_bilinear and m.mode == "bilinear" and not cls(1, 4, 1e-2, mode="bilinear").fused_bilinear
    with pytest.raises(ValueError):
        CRFasRNN(charb(.05), fused_bilinear=True)
    with pytest.raises(ValueError):
        CRFasRNN(charb(.05), lattice=True, mode="bilinear")
    with pytest.raises(ValueError):
        CRFasRNN(charb(.05), lattice=True, mode="bilinear", fused_bilinear=True)
    net = CRFasRNN(charb(.05), gchannels=3, mode="bilinear", fused_bilinear=True)
    assert net.W.mode == "bilinear" and net.W.fused_bilinear
    assert CRFasRNN(charb(.05)).W.mode == "nearest" and not CRFasRNN(charb(.05)).W.fused_bilinear
    for head in (CRFdepthRefiner, CRFwUncertainty, CRFdepthUpsampler):
        W = head(mode="bilinear", fused_bilinear=True).CRF.W
        assert W.mode == "bilinear" and W.fused_bilinear
        with pytest.raises(ValueError):
            head(lattice=True, fused_bilinear=True)


def test_binding_checks():
    import phl

    t = torch.zeros(1, 1, 4, 4)
    with pytest.raises(ValueError):
        phl.guided_filter_bilinear(t, t, 1, 1e-2, subsample=1)
    with pytest.raises(TypeError):
        phl.guided_filter_bilinear(t, t, 1, 1e-2, subsample=2)                # not a CUDA tensor
    with pytest.raises(TypeError):
        phl.guided_filter_bilinear(t.double(), t.double(), 1, 1e-2, subsample=2)
    assert phl.GUIDED_BILINEAR_FULL_COV == 1


OK, INVALID, TOO_LARGE, UNSUPPORTED = 0, 1, 6, 7
Y, X, S, O, E = (0x1000 * k for k in range(1, 6))       # fake device addresses, never dereferenced


def _args(y=Y, x=X, src=S, out=O, B=1, cy=4, cx=3, H=48, W=64, h=24, w=32, r=4, eps=E, scale=1.0, flags=0):
    return (y, x, src, out, B, cy, cx, H, W, h, w, r, eps, scale, flags)


ARG_CASES = [
    (_args(B=-1), INVALID), (_args(cy=-1), INVALID), (_args(cx=0), INVALID), (_args(H=-3), INVALID), (_args(r=-1), INVALID),
    (_args(h=49), INVALID), (_args(w=65), INVALID), (_args(h=0), INVALID), (_args(scale=float("inf")), INVALID),
    (_args(y=None), INVALID), (_args(x=None), INVALID), (_args(out=None), INVALID), (_args(eps=None), INVALID),
    (_args(out=Y), INVALID), (_args(out=X), INVALID), (_args(out=S), INVALID),
    (_args(H=1 << 16, W=1 << 16, h=8, w=8), TOO_LARGE), (_args(B=1 << 20, cy=1 << 20), TOO_LARGE),
    (_args(H=(1 << 30) + 1, W=1, h=8, w=1), TOO_LARGE), (_args(cx=17), UNSUPPORTED),
    (_args(cx=5, flags=1), UNSUPPORTED), (_args(flags=2), UNSUPPORTED), (_args(cx=17, flags=1), UNSUPPORTED),
    (_args(B=0, y=None, x=None, out=None), OK), (_args(cy=0, y=None, out=None), OK), (_args(H=0, h=0, y=None, out=None), OK),
    (_args(B=0, y=None, x=None, out=None, flags=2), OK),                      # empty calls return before the flags are read
]


@pytest.mark.parametrize("args,status", ARG_CASES, ids=[str(i) for i in range(len(ARG_CASES))])
def test_guided_filter_bilinear_argument_checks(args, status):
    import phl

    lib = phl.load_library()
    a = list(args)
    a[13] = ctypes.c_float(a[13])
    assert lib.phl_guided_filter_bilinear(*a, None) == status
    if status != OK:
        assert lib.phl_last_error().decode().startswith("phl_guided_filter_bilinear"), lib.phl_last_error()


def test_labels_per_chunk_query():
    """phl_guided_filter_bilinear_labels_per_chunk against the formula of phl_guided.hip worked by hand:
    min(B * cy, 65535, 96 MiB / per) and at least 1, per = 2 * 4 (cx + 1) hw bytes a label -- the window-mean planes beside
    the coefficient planes."""
    import phl

    q = phl.guided_filter_bilinear_labels_per_chunk
    budget = 96 << 20
    assert budget == 100663296
    assert q(2, 50, 16, 128, 128) == 45 == budget // (2 * 17 * 4 * 16384)
    assert q(2, 50, 16, 128, 128) == phl.guided_filter_labels_per_chunk(2, 50, 16, 128, 128) // 2
    assert q(1, 8, 1, 555, 695) == 8 and q(1, 100, 1, 555, 695) == 16 == budget // (2 * 3085800)
    assert q(1, 64, 3, 555, 695) == 8 == budget // (32 * 385725)
    assert q(1, 3, 16, 8192, 8192) == 1 and q(1, 70000, 1, 1, 1) == 65535
    lib = phl.load_library()
    for bad in ((0, 5, 1, 8, 8), (1, 0, 1, 8, 8), (1, 5, 0, 8, 8), (1, 5, 1, 0, 8), (1, 5, 1, 8, 0)):
        assert lib.phl_guided_filter_bilinear_labels_per_chunk(*bad) == 0
