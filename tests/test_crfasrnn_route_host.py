"""The route table of CRFasRNN (crf.crf_module._nchw_route), pinned row by row from plain values: every row, every
precondition of a row flipped on its own, what is no precondition of a row left without effect, and the label limits of
each route at both sides.  Then CRFasRNN._run itself on CPU tensors and on float64: "plain", and the bits of
_mean_field_nchw.  No GPU."""
import pytest
import torch

# a call that meets every precondition of the "lattice" row; the other rows are this one with their differences
BASE = dict(lattice=True, niters=5, e0_fp32_cuda=True, e0_4d=True, refs_fp32_cuda=True, grad=False, grad_w=False,
            fused_grad=False, fused_step=False, L=16, mu_matrix=True, mu_potts=False, step=True)
RECORDING = dict(grad=True, grad_w=True)
ROWS = {
    "lattice": {},
    "lattice_grad": dict(RECORDING, fused_grad=True),
    "step": dict(lattice=False),
    "step_grad": dict(RECORDING, lattice=False, fused_step=True),
}
# row -> (one value changed -> the route the table then gives); a precondition missed is "plain" unless said otherwise
FLIPS = {
    "lattice": [(dict(niters=0), "plain"), (dict(e0_fp32_cuda=False), "plain"), (dict(mu_matrix=False), "plain"),
                (RECORDING, "plain"), (dict(grad=True), "plain"), (dict(lattice=False), "step"),
                # no preconditions of this row
                (dict(e0_4d=False), "lattice"), (dict(refs_fp32_cuda=False), "lattice"), (dict(step=False), "lattice"),
                (dict(fused_grad=True), "lattice"), (dict(fused_step=True), "lattice"), (dict(grad_w=True), "lattice"),
                (dict(L=4096), "lattice"), (dict(mu_potts=True), "lattice")],
    "lattice_grad": [(dict(niters=0), "plain"), (dict(e0_fp32_cuda=False), "plain"), (dict(mu_matrix=False), "plain"),
                     (dict(fused_grad=False), "plain"), (dict(refs_fp32_cuda=False), "plain"), (dict(L=513), "plain"),
                     (dict(grad=False), "lattice"), (dict(lattice=False), "plain"),
                     (dict(fused_grad=False, fused_step=True), "plain"),      # a lattice W never enters the step branch
                     (dict(e0_4d=False), "lattice_grad"), (dict(step=False), "lattice_grad"),
                     (dict(fused_step=True), "lattice_grad"), (dict(mu_potts=True), "lattice_grad")],
    "step": [(dict(niters=0), "plain"), (dict(e0_fp32_cuda=False), "plain"), (dict(e0_4d=False), "plain"),
             (dict(mu_matrix=False), "plain"), (dict(step=False), "plain"), (dict(L=513), "plain"),
             (RECORDING, "plain"), (dict(grad_w=True), "plain"),              # W's parameters alone record as well
             (dict(grad_w=True, fused_step=True), "step_grad"), (dict(lattice=True), "lattice"),
             (dict(refs_fp32_cuda=False), "step"), (dict(fused_grad=True), "step"), (dict(fused_step=True), "step"),
             (dict(mu_potts=True), "step")],
    "step_grad": [(dict(niters=0), "plain"), (dict(e0_fp32_cuda=False), "plain"), (dict(e0_4d=False), "plain"),
                  (dict(mu_matrix=False), "plain"), (dict(step=False), "plain"), (dict(fused_step=False), "plain"),
                  (dict(L=65), "plain"), (dict(L=65, mu_potts=True), "plain"),
                  (dict(grad=False, grad_w=False), "step"), (dict(lattice=True), "plain"),
                  (dict(lattice=True, fused_grad=True), "lattice_grad"),
                  (dict(grad=False), "step_grad"),                            # only W's parameters ask
                  (dict(refs_fp32_cuda=False), "step_grad"), (dict(fused_grad=True), "step_grad"),
                  (dict(mu_potts=True), "step_grad")],
}
# (row, L, Potts family) -> route: both sides of every label limit
LIMITS = [
    ("step_grad", 1, False, "step_grad"), ("step_grad", 64, False, "step_grad"), ("step_grad", 65, False, "plain"),
    ("step_grad", 64, True, "step_grad"), ("step_grad", 65, True, "plain"),
    ("step", 1, False, "step"), ("step", 256, False, "step"), ("step", 257, False, "step"),
    ("step", 512, False, "step"), ("step", 513, False, "plain"), ("step", 1024, False, "plain"),
    ("step", 512, True, "step"), ("step", 513, True, "step"), ("step", 1024, True, "step"),
    ("step", 1025, True, "plain"), ("step", 1025, False, "plain"),
    # _label_pad(L) <= 512: 509 .. 512 pad to 512, 513 to 516
    ("lattice_grad", 231, False, "lattice_grad"), ("lattice_grad", 509, False, "lattice_grad"),
    ("lattice_grad", 510, False, "lattice_grad"), ("lattice_grad", 511, False, "lattice_grad"),
    ("lattice_grad", 512, False, "lattice_grad"), ("lattice_grad", 513, False, "plain"), ("lattice_grad", 513, True, "plain"),
    ("lattice", 513, False, "lattice"), ("lattice", 1025, False, "lattice"),
]


def _route(row, **changed):
    from crf.crf_module import _nchw_route

    return _nchw_route(**{**BASE, **ROWS[row], **changed})


@pytest.mark.parametrize("row", list(ROWS))
def test_every_row_and_every_precondition_on_its_own(row):
    assert _route(row) == row
    for changed, want in FLIPS[row]:
        assert _route(row, **changed) == want, (row, changed)


@pytest.mark.parametrize("row,L,potts,want", LIMITS)
def test_label_limits(row, L, potts, want):
    assert _route(row, L=L, mu_potts=potts) == want


def test_the_limits_are_the_kernels_own():
    import phl
    from crf import crf_module as cm

    assert (cm._STEP_GRAD_MAX_L, cm._STEP_MAX_L, cm._STEP_POTTS_MAX_L) == (64, 512, 1024)
    assert (cm._STEP_GRAD_MAX_L, cm._STEP_MAX_L, cm._STEP_POTTS_MAX_L) == (phl.NCHW_TRAIN_MAX_L, phl.NCHW_WIDE_MAX_L,
                                                                          phl.NCHW_UNIFORM_MAX_L)
    assert [cm._label_pad(L) for L in (509, 510, 511, 512, 513)] == [512, 512, 512, 512, 516]


def test_nothing_but_plain_without_its_head():
    """No keyword and no Mu reaches a kernel route from CPU tensors, another dtype or niters = 0."""
    for row in ROWS:
        for keywords in ({}, dict(fused_grad=True, fused_step=True)):
            for missed in (dict(e0_fp32_cuda=False), dict(niters=0), dict(mu_matrix=False)):
                assert _route(row, **{**keywords, **missed}) == "plain", (row, keywords, missed)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("lattice", [False, True])
def test_run_on_the_cpu_is_the_plain_loop(dtype, lattice, monkeypatch):
    from crf import crf_module as cm

    seen = []
    real = cm._nchw_route
    monkeypatch.setattr(cm, "_nchw_route", lambda *a, **k: seen.append(real(*a, **k)) or seen[-1])
    g = torch.Generator().manual_seed(3)
    refs = torch.rand((2, 1, 9, 11), generator=g).to(dtype)
    logits = (torch.randn((2, 5, 9, 11), generator=g) * 3).to(dtype)
    labels = torch.arange(5, dtype=dtype)
    net = cm.CRFasRNN(cm.charb(3.0), niters=2, r=2, eps=1e-2, fused_grad=True, fused_step=True).to(dtype)
    if lattice:                                           # the route is taken before W runs: a W that only marks the class
        net.W = cm.BatchedAdjacency()
        monkeypatch.setattr(cm.BatchedAdjacency, "forward", lambda self, Y, refs: Y * 0.5)
    for grad in (False, True):
        with torch.set_grad_enabled(grad):
            out = net(refs, logits, labels=labels)
            want = -cm._mean_field_nchw(-logits, lambda Q: net.W(net.Mu(Q, labels), refs), net.niters)
        assert seen and set(seen) == {"plain"}, seen
        assert out.dtype == dtype and torch.equal(out.detach(), want.detach())
        depth, done = net._run(refs, logits, None, labels, expect=True)
        assert done is False and torch.equal(depth.detach(), want.detach())
