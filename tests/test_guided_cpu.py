"""The box-window guided-filter family without a GPU: the repository's torch form (crf/guided.py) in float64 against the
reference's classes run in float64 (tests/golden/guided_*.npz, written by tests/golden/generate_guided.py with the
reference's own mBoxFilter as the box sum), and the argument checks of phl_guided_filter, which return before the first
HIP call.

Bound: 1e-12 of the output's largest magnitude -- float64 rounding (2.2e-16) times a few thousand operations.  Where the
fixtures were written the difference is exactly 0; the bound leaves room for another torch build's cumsum grouping and
none for a changed formula.  ``omega`` is loaded from the fixture: the reference initialises it as fp32
log(exp(eps) - 1), the repository's box-window constructor with expm1."""
import numpy as np
import pytest
import torch

from _guided_fixtures import CASES, END_TO_END, build_module, load_case

BOUND = 1e-12


def _check(got, want, name):
    err = float(np.abs(got - want).max())
    print(f"{name}: max |torch float64 - reference float64| = {err:.3e}, |out| <= {np.abs(want).max():.4g}")
    assert err <= BOUND * np.abs(want).max(), (name, err)


@pytest.mark.parametrize("name", [c for c in CASES if c not in END_TO_END])
def test_filter_classes_match_reference_float64(name):
    from crf import guided

    z = load_case(name)
    m = build_module(guided, z, torch.float64, "cpu")
    with torch.no_grad():
        out = m(torch.from_numpy(z["y"]).double(), torch.from_numpy(z["x"]).double())
    _check(out.numpy(), z["out"], name)


def test_crfasrnn_default_w_matches_reference_float64():
    from crf.crf_module import CRFasRNN, charb

    z = load_case("crfasrnn_guided")
    net = CRFasRNN(charb(float(z["gamma"])), niters=int(z["niters"]))
    with torch.no_grad():
        net.W.omega.copy_(torch.from_numpy(z["omega"]))
    net = net.double()
    with torch.no_grad():
        out = net(torch.from_numpy(z["x"]).double(), torch.from_numpy(z["logits"]).double(), labels=torch.from_numpy(z["labels"]).double())
    _check(out.numpy(), z["out"], "crfasrnn_guided")


def test_mean_field_over_guided_adjacency_matches_reference_float64():
    from crf.crf_module import mean_field_infer
    from crf.guided import GuidedAdjacency

    z = load_case("meanfield_guided")
    W = GuidedAdjacency(torch.from_numpy(z["x"]), int(z["r"]), float(z["eps"]))
    with torch.no_grad():
        W.omega.copy_(torch.from_numpy(z["omega"]))
    W = W.double()
    W.guide_img = W.guide_img.double()
    with torch.no_grad():
        Q = mean_field_infer(torch.from_numpy(z["E0"]).double(), W, torch.from_numpy(z["Mu"]).double(), int(z["niters"]))
    _check(Q.numpy(), z["out"], "meanfield_guided")


OK, INVALID, TOO_LARGE, UNSUPPORTED = 0, 1, 6, 7
Y, X, S, O, M1, M2, M3, M4, E = (0x1000 * k for k in range(1, 10))       # fake device addresses, never dereferenced


def _args(y=Y, x=X, src=S, out=O, B=1, cy=4, cx=3, H=48, W=64, h=24, w=32, r=4, m1=M1, m2=M2, m3=M3, m4=M4, eps=E, scale=1.0):
    return (y, x, src, out, B, cy, cx, H, W, h, w, r, m1, m2, m3, m4, eps, scale)


ARG_CASES = [
    (_args(B=-1), INVALID), (_args(cy=-1), INVALID), (_args(cx=0), INVALID), (_args(H=-3), INVALID), (_args(r=-1), INVALID),
    (_args(h=49), INVALID), (_args(w=65), INVALID), (_args(h=0), INVALID), (_args(scale=float("inf")), INVALID),
    (_args(y=None), INVALID), (_args(x=None), INVALID), (_args(out=None), INVALID), (_args(eps=None), INVALID),
    (_args(m1=None), INVALID), (_args(m4=None), INVALID), (_args(out=Y), INVALID), (_args(out=X), INVALID), (_args(out=S), INVALID),
    (_args(H=1 << 16, W=1 << 16, h=8, w=8), TOO_LARGE), (_args(B=1 << 20, cy=1 << 20), TOO_LARGE),
    (_args(H=(1 << 30) + 1, W=1, h=8, w=1), TOO_LARGE), (_args(cx=17), UNSUPPORTED),
    (_args(B=0, y=None, x=None, out=None), OK), (_args(cy=0, y=None, out=None), OK), (_args(H=0, h=0, y=None, out=None), OK),
]


@pytest.mark.parametrize("args,status", ARG_CASES, ids=[str(i) for i in range(len(ARG_CASES))])
def test_guided_filter_argument_checks(args, status):
    import ctypes

    import phl

    lib = phl.load_library()
    a = list(args)
    a[17] = ctypes.c_float(a[17])
    assert lib.phl_guided_filter(*a, None) == status
    if status != OK:
        assert lib.phl_last_error().decode().startswith("phl_guided_filter"), lib.phl_last_error()


def test_tiled_form_takes_the_default_radius():
    """The reference's default r = 20 at full resolution stays on the LDS-tiled form (above phl_guided_filter_max_r the
    kernels run their streamed form; no radius is refused)."""
    import phl

    assert phl.load_library().phl_guided_filter_max_r() >= 20


def test_labels_per_chunk_query():
    """phl_guided_filter_labels_per_chunk against the formula of phl_guided.hip worked by hand: min(B * cy, 96 MiB / per),
    per = 4 (cx + 1) hw bytes a label in the forward, hw (4 unless full + 8 (cx + 1) + 8 cx for grad_x + 24 cx for grad_x
    or grad_eps) in the backward.  The GPU tests of the chunk loop ask this query, not a copy of the constant."""
    import phl

    q = phl.guided_filter_labels_per_chunk
    budget = 96 << 20
    assert budget == 100663296
    assert q(1, 8, 1, 555, 695) == 8 == min(8, budget // 3085800)                     # the suite's large image: one chunk
    assert q(1, 100, 1, 555, 695) == 32 and q(4, 25, 1, 555, 695) == 32
    assert q(1, 8, 1, 555, 695, need_y=True, need_x=True, need_eps=True) == 5 == budget // (52 * 385725)
    assert q(2, 50, 16, 128, 128) == 90 == budget // (17 * 4 * 16384)
    assert q(2, 50, 16, 128, 128, full=True) == 90                                     # the forward ignores full
    assert q(2, 50, 16, 128, 128, full=True, need_y=True, need_x=True, need_eps=True) == 9 == budget // (648 * 16384)
    assert q(2, 50, 3, 128, 128, need_y=True, need_x=True, need_eps=True) == 46 == budget // (132 * 16384)
    # the need flags change the bytes of a label: grad_y alone keeps P and Q only, grad_eps adds the fp64 terms
    assert q(2, 50, 16, 128, 128, full=True, need_y=True) == 45 == budget // (136 * 16384)
    assert q(2, 50, 16, 128, 128, full=True, need_eps=True) == 11 == budget // (520 * 16384)
    assert q(2, 50, 16, 128, 128, full=True, need_y=True, need_eps=True) == 11
    assert q(2, 50, 16, 128, 128, full=True, need_x=True) == 9
    assert q(2, 50, 16, 128, 128, full=True, grad=True) == 45                          # a backward that is asked for nothing
    # never fewer than one label, never more than a grid dimension; nothing for sizes below 1 or another mask
    assert q(1, 3, 16, 8192, 8192) == 1 and q(1, 70000, 1, 1, 1) == 65535
    lib = phl.load_library()
    assert lib.phl_guided_filter_labels_per_chunk(0, 5, 1, 8, 8, 0, -1) == 0
    assert lib.phl_guided_filter_labels_per_chunk(1, 5, 1, 8, 8, 0, 8) == 0 == lib.phl_guided_filter_labels_per_chunk(1, 5, 1, 8, 8, 0, -2)


def test_guided_adjacency_keeps_fp32_for_an_fp32_guide():
    """GuidedAdjacency.__matmul__ casts U to its guide's dtype.  The constructor makes the guide fp32, so a float64 U is
    still filtered in fp32, as it was when the cast was a fixed .float(): same bits as the product of U.float()."""
    from crf.guided import GuidedAdjacency

    g = torch.Generator().manual_seed(0)
    guide = torch.rand((1, 3, 20, 24), generator=g, dtype=torch.float64)
    U = torch.rand((480, 5), generator=g, dtype=torch.float64)
    W = GuidedAdjacency(guide, 2, 1e-2)
    assert W.guide_img.dtype == torch.float32
    out = W @ U
    assert out.dtype == torch.float32 and torch.equal(out, W @ U.float())
    img = U.t().reshape(1, 5, 20, 24).float()
    with torch.no_grad():
        want = W._torch_forward(img, W.guide_img) * 0.5 * 25 - img
    assert torch.equal(out, want[0].reshape(5, -1).t())


def test_binding_rejects_other_tensors():
    import phl

    t = torch.zeros(1, 1, 4, 4)
    with pytest.raises(TypeError):
        phl.guided_filter(t, t, 1, 1e-2)
    with pytest.raises(TypeError):
        phl.guided_filter(t.double(), t.double(), 1, 1e-2)
