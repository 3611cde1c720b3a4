"""The energy regimes of tests/_energy_util.py are usable references (no GPU): for L in {4, 32, 256} and n = 293 the float64
and the fp32 torch forms of softmax(-(E0 + X Mu)), forward and autograd, are finite at every regime, and ``masked`` leaves
every pixel a finite label.  And the reason the GPU tests exist, as arithmetic: an fp32 accumulation started at E0
(chain_model) errs at least three times as much as the same accumulation with E0 added last, at L = 256 and an offset of
1e4."""
import pytest
import torch

from _energy_util import INF, REGIMES, chain_model, regimes, winners

N = 293


def _operands(L, seed):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    regs = regimes(N, L, gen)
    X = torch.rand((N, L), generator=gen) * 1.5 - 0.3
    Mu = (torch.rand((L, L), generator=gen) - 0.3) * (4.0 / L ** 0.5)
    gout = torch.randn((N, L), generator=gen)
    return regs, X, Mu, gout


@pytest.mark.parametrize("L", [4, 32, 256])
def test_references_are_finite_at_every_regime(L):
    regs, X, Mu, gout = _operands(L, L)
    assert tuple(regs) == REGIMES
    for name, E in regs.items():
        assert E.dtype == torch.float32 and E.shape == (N, L) and not bool(torch.isnan(E).any()) and not bool((E == -INF).any()), name
        assert bool(torch.isfinite(E).any(1).all()), f"{name}: a pixel without a finite label"
        if name != "masked":
            assert bool(torch.isfinite(E).all()), name
        for dtype in (torch.float64, torch.float32):
            e, x, m = (t.detach().clone().to(dtype).requires_grad_(True) for t in (E, X, Mu))
            Q = torch.softmax(-(e + x @ m), dim=1)
            Q.backward(gout.to(dtype))
            Q = Q.detach()
            for what, t in (("Q", Q), ("gE0", e.grad), ("gX", x.grad), ("gMu", m.grad)):
                assert bool(torch.isfinite(t).all()), (name, dtype, what)
            assert float((Q.sum(1) - 1).abs().max()) <= 1e-5, (name, dtype)
            if name == "masked":
                assert bool((Q[torch.isinf(E)] == 0).all()) and bool((e.grad[torch.isinf(E)] == 0).all()), (name, dtype)


@pytest.mark.parametrize("L", [4, 32, 256])
def test_regimes_are_what_their_names_say(L):
    regs, _, _, _ = _operands(L, 7 * L)
    a, b = N // 3, 2 * N // 3
    m = torch.isinf(regs["masked"])
    assert bool(m[:a, 0].all()) and bool(m[a:b, L - 1].all()) and 0.15 < float(m.float().mean()) < 0.6
    assert bool((regs["ties"] == 7.65e4).all())
    rows = (regs["row_offsets"].min(1).values / 50).round() * 50             # base < 8: the offset to the nearest 50
    assert len(set(rows.tolist())) == 6
    win = winners(N, L, "cpu")
    assert set(win.tolist()) == set(range(L)) and int(win[0]) == 0 and int(win[-1]) == L - 1
    Q = torch.softmax(-regs["dominated"], dim=1)
    assert torch.equal(Q, torch.zeros_like(Q).scatter_(1, win[:, None], 1.0))  # the others underflow to exactly 0
    q = torch.softmax(-regs["spread_120"].double(), dim=1)
    if L >= 32:
        assert bool(((q > 0) & (q < 2.0 ** -126)).any())                      # fp32's denormal range is reached


def test_chain_on_e0_loses_what_e0_last_keeps():
    """L = 256, n = 512, E0 = 1e4 + 8 rand: the Q error of an fmaf chain started at E0 is at least 3x that of the same
    chain started at 0 with E0 added at the end (the softmax itself in float64: only the rounding of E is seen)."""
    L, n = 256, 512
    gen = torch.Generator(device="cpu").manual_seed(256)
    E0 = 1e4 + 8 * torch.rand((n, L), generator=gen)
    X = torch.rand((n, L), generator=gen) * 1.5 - 0.3
    Mu = (torch.rand((L, L), generator=gen) - 0.3) * (4.0 / L ** 0.5)
    want = torch.softmax(-(E0.double() + X.double() @ Mu.double()), dim=1)
    for group in (1, 4):
        chain = chain_model(E0, X, Mu, group)
        last = E0 + chain_model(torch.zeros_like(E0), X, Mu, group)
        e_chain = float((torch.softmax(-chain.double(), 1) - want).abs().max())
        e_last = float((torch.softmax(-last.double(), 1) - want).abs().max())
        e_torch = float((torch.softmax(-(E0 + X @ Mu), 1).double() - want).abs().max())
        print(f"[measured] L={L} off=1e4 group={group}: chain {e_chain:.2e}  E0 last {e_last:.2e}  torch fp32 {e_torch:.2e}")
        assert e_chain >= 3 * e_last, (group, e_chain, e_last)
    # the split form of the model is the same product: without an offset it is as good as the plain chain
    E0s = 8 * torch.rand((n, L), generator=gen)
    w = E0s.double() + X.double() @ Mu.double()
    e_split = float((chain_model(E0s, X, Mu, 32, split=True).double() - w).abs().max())
    e_plain = float((chain_model(E0s, X, Mu, 1).double() - w).abs().max())
    print(f"[measured] L={L} off=0: |E - E64| split model {e_split:.2e}  fmaf chain {e_plain:.2e}")
    assert e_split <= 2 * e_plain
