"""Every kernel that ends in a softmax over labels, at the energies the workload feeds it (tests/_energy_util.py): offsets of
3e2 and +-7.65e4, per-pixel offsets, ties, one dominating label, a spread that runs Q through the denormal range, and +inf
(masked) energies -- against the float64 torch form on the device, by the rules the suite already applies to the same
quantities (no figure changed; see _energy_util.py).  Shapes are the smallest that reach every code path: pixel-major
n = 293 = 2 * 128 + 37 (both wave groups of the tile kernels plus the tail kernel) and n = 37 (the tail alone), rows as
row-padded views; channel-major B = 2 with (5, 13) on the dword path and (8, 16) on the float4 path.  Every case asserts
the route it means to test and prints its errors as ``[measured]`` lines; a test asserts after all its cases have printed.

The contract of the one kernel that accumulates on top of E0.  k_compat_softmax and k_compat_tail start their fp32
accumulators at E0 - s_p (s_p the row minimum) and meet the project's rule at every regime.  k_compat_split (the split
route up to 256 labels, whole 128-pixel tiles) still starts them at E0, so each of its accumulations rounds at the magnitude
of E0 where torch's fp32 form rounds once, and at the offset regimes it misses the project's rule e_hip <= max(2e-6, 2
e_torch) (figures in the reasons of the strict xfail twins below and in DESIGN.md 7.14).  There, and only there, its Q is
held to e_hip <= 2 e_chain, e_chain being the error of _energy_util.chain_model -- the same accumulation in plain torch --
against float64 (measured: e_hip / e_chain = 0.96 .. 1.03); every other regime, the logits and every other kernel are held
to the project's rule.  The backward and the mean_field_infer loop at 200 labels run that kernel and follow it.  The twins
assert the project's rule on the same cases and are marked xfail(strict=True, raises=AssertionError): the suite reports the
day it is met.  The model's error is printed for every regime of that kernel, held to or not."""
import functools

import pytest
import torch
import torch.nn.functional as F

from _energy_util import (INF, LOOP_REGIMES, OFFSET_REGIMES, REGIMES, Report, chain_model, grad_bound, loop_judge, nchw,
                          padded_rows, regimes, winners)
from _guided_util import DEV
from _nchw_util import (B, LOGITS, PRODUCT, SOFTMAX, UNIFORM, WIDE, both_loops, energy, launch_spy, on_float4_path, torch32,
                        truth)

pytestmark = pytest.mark.gpu

NS = (293, 37)
SHAPES = ((5, 13), (8, 16))
COMPAT_ENTRIES = {"phl_compat_softmax", "phl_compat_softmax_split", "phl_uniform_compat_softmax", "phl_softmax_neg_add"}
ENTRY = {"f32": "phl_compat_softmax", "split": "phl_compat_softmax_split", "wide": "phl_compat_softmax_split",
         "uniform": "phl_uniform_compat_softmax", "gemm": "phl_softmax_neg_add"}
# (route, L, arith): "wide" is the split route above 256 labels (k_compat_wide)
COMPAT_CASES = ([("f32", L, "f32") for L in (4, 32, 100, 176, 256)] + [("split", L, "split") for L in (132, 252, 256)] +
                [("wide", L, "split") for L in (260, 384, 512)] + [("uniform", L, None) for L in (64, 300, 1000)] +
                [("gemm", 6, None), ("gemm", 516, "f32")])


@pytest.fixture(autouse=True)
def _default_arith(monkeypatch):
    monkeypatch.delenv("PHL_COMPAT_ARITH", raising=False)       # the routes asserted below are the binding's defaults


def _names(seen):
    return [name for name, _ in seen]


@functools.lru_cache(maxsize=None)
def _operands(L, n, potts=False):
    """(regimes, X, Mu, G, gout) of one (L, n): X and Mu as in test_compat_grad_parity, or the Potts-family Mu."""
    gen = torch.Generator(device=DEV).manual_seed(1000 * L + n)
    regs = regimes(n, L, gen)
    X = padded_rows(torch.rand((n, L), device=DEV, generator=gen) * 1.5 - 0.3, pad=8)
    if potts:
        Mu = 0.7 * torch.ones((L, L), device=DEV) - 1.3 * torch.eye(L, device=DEV)
    else:
        Mu = (torch.rand((L, L), device=DEV, generator=gen) - 0.3) * (4.0 / L ** 0.5)
        Mu[: L // 2] *= 0.5
    G = torch.randn((n, L), device=DEV, generator=gen) * 5
    gout = torch.randn((n, L), device=DEV, generator=gen)
    return regs, X, Mu, G, gout


# ---- pixel-major: softmax_neg_add --------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [4, 256, 260, 516, 1028, 7])
def test_softmax_neg_add(L):
    """One L per kernel of phl_softmax_neg_add's dispatch: k_softmax_neg_add<1> (4, 256), <2> (260), <4> (516), the generic
    kernel (1028: above the register forms; 7: rows off the 16-byte grid)."""
    import phl

    rep = Report()
    for n in NS:
        regs, _, _, G, _ = _operands(L, n)
        for regime in REGIMES:
            E0 = padded_rows(regs[regime])
            assert (L % 4 != 0) or phl._aligned(E0)
            for g in (G, None):
                name = f"softmax_neg_add L={L} n={n} {regime} G={'yes' if g is not None else 'no'}"
                with launch_spy(modeless=()) as seen:
                    got = phl.softmax_neg_add(E0, g)
                assert _names(seen) == ["phl_softmax_neg_add"]
                # the float4 kernels need 16-byte rows of every operand, the result included: else the generic kernel runs
                assert (L % 4 != 0) or (phl._aligned(got) and (g is None or phl._aligned(g))), name
                E64 = energy(E0.double(), None if g is None else g.double())
                want, ref32 = torch.softmax(-E64, 1), torch.softmax(-energy(E0, g), 1)
                _, e_torch = rep.judge(name, got, ref32, want)
                _q_checks(rep, name, got, want, e_torch, regime, E0, g)
    rep.done()


def _q_checks(rep, name, q, want, e_torch, regime, E0, g):
    if float((q.sum(1) - 1).abs().max()) > 1e-5:
        rep.fail(name, "rows do not sum to 1")
    if regime == "masked":
        rep.exact(name, q, torch.isinf(E0), 0.0)
    if regime == "dominated" and g is None:
        rep.one_hot(name, q, winners(q.shape[0], q.shape[1], DEV), want, e_torch)


# ---- pixel-major: compat_softmax ---------------------------------------------------------------------------------------
_chain_cache = {}


def _split_chain(E0, X, Mu):
    """chain_model on the rows as the split route deals them: whole 128-pixel tiles to k_compat_split (six bf16 partial
    products per chunk of 32, started at E0, the accumulator rounded every 8 products: measured, see chain_model), the
    last n % 128 to k_compat_tail (an fmaf chain started at E0 - s_p, s_p the
    row minimum over the finite entries, added back at the end)."""
    nm = E0.shape[0] // 128 * 128
    parts = [chain_model(E0[:nm], X[:nm], Mu, 32, split=True, inner=8)] if nm else []
    if E0.shape[0] > nm:
        e = E0[nm:]
        s = e.min(1, keepdim=True).values
        s = torch.where(torch.isfinite(s), s, torch.zeros_like(s))
        parts.append(chain_model(e - s, X[nm:], Mu, 1) + s)
    return torch.cat(parts)


def _chain_energy(route, L, n, regime, E0, X, Mu):
    key = (route, L, n, regime)
    if key not in _chain_cache:
        _chain_cache[key] = _split_chain(E0, X, Mu)
    return _chain_cache[key]


def _on_e0(route, n):
    """The cases that run k_compat_split, the one kernel that accumulates on top of E0: the split route up to 256 labels
    with at least one whole tile.  They print the model's error as well."""
    return route == "split" and n >= 128


def _compat_contract(route, L, n, regime, logits):
    """Which cases of compat_softmax are held to the chain contract: Q of k_compat_split at the offset regimes, nothing
    else.  The logits are held to the project's rule everywhere (its floor scales with |want|)."""
    return _on_e0(route, n) and regime in OFFSET_REGIMES and not logits


XFAIL_ON_E0 = ("k_compat_split starts its fp32 accumulators at E0, so every accumulation rounds at ulp(|E0|); torch's fp32 "
               "form rounds there once.  Measured on an MI355X (e_hip / e_torch against float64): ")


def _compat_case(rep, route, L, arith, n, regime, logits, contract):
    import phl

    regs, X, Mu, _, _ = _operands(L, n, route == "uniform")
    E0 = padded_rows(regs[regime])
    out = torch.full((n, L + 12), -7.0, device=DEV)
    name = f"compat_softmax {route} L={L} n={n} {regime} logits={logits}"
    found, _ = phl._compat_route(L, (X, E0, out[:, :L]), Mu, None, True, arith or ("split" if L > 176 else "f32"))
    assert found == {"wide": "split"}.get(route, route), (name, found)
    assert route not in ("split", "wide") or (L > 256) == (route == "wide")
    with launch_spy(modeless=()) as seen:
        got = phl.compat_softmax(E0, X, Mu, out=out[:, :L], logits=logits, arith=arith)
    took = set(_names(seen)) & COMPAT_ENTRIES
    assert took == (set() if route == "gemm" and logits else {ENTRY[route]}), (name, _names(seen))
    assert bool((out[:, L:] == -7.0).all()), name + ": wrote into the row padding"
    E64, E32 = E0.double() + X.double() @ Mu.double(), E0 + X @ Mu
    want, ref32 = (-E64, -E32) if logits else (torch.softmax(-E64, 1), torch.softmax(-E32, 1))
    chain = None
    if _on_e0(route, n):
        Ec = _chain_energy(route, L, n, regime, E0, X, Mu)
        chain = -Ec if logits else torch.softmax(-Ec.double(), 1)
    _, e_torch = rep.judge(name, got, ref32, want, chain=chain, contract=contract)
    if regime == "masked":
        rep.exact(name, got, torch.isinf(E0), -INF if logits else 0.0)
    if not logits:
        if float((got.sum(1) - 1).abs().max()) > 1e-5:
            rep.fail(name, "rows do not sum to 1")
        if regime == "dominated":
            rep.one_hot(name, got, (-E64).argmax(1), want, e_torch)
            if route != "uniform" and not torch.equal((-E64).argmax(1), winners(n, L, DEV)):
                rep.fail(name, "X @ Mu moved the winner: the regime is not what its name says")


@pytest.mark.parametrize("route,L,arith", COMPAT_CASES)
def test_compat_softmax(route, L, arith):
    rep = Report()
    for n in NS:
        for regime in REGIMES:
            for logits in (False, True):
                _compat_case(rep, route, L, arith, n, regime, logits, contract=_compat_contract(route, L, n, regime, logits))
    rep.done()


@pytest.mark.xfail(strict=True, raises=AssertionError,
                   reason=XFAIL_ON_E0 + "Q at offset 3e2: 4.0e-5 / 2.0e-6 (L = 132), 4.1e-5 / 1.4e-6 (L = 256); at offset 7.65e4: "
                   "8.4e-3 / 6.5e-4 (L = 132), 5.5e-3 / 3.6e-4 (L = 252), 5.7e-3 / 3.3e-4 (L = 256); ties: 1.5e-3 / 1.0e-4 (L = 256)")
@pytest.mark.parametrize("route,L,arith,n,regime", [
    (route, L, arith, n, regime) for route, L, arith in COMPAT_CASES for n in NS for regime in OFFSET_REGIMES
    if _compat_contract(route, L, n, regime, False)])
def test_compat_softmax_project_rule_where_the_chain_starts_at_e0(route, L, arith, n, regime):
    """The cases test_compat_softmax holds to the chain contract, against the project's rule: expected to fail until
    k_compat_split's accumulators start from E0 - s_p as k_compat_softmax's do (Next)."""
    rep = Report()
    _compat_case(rep, route, L, arith, n, regime, False, contract=False)
    rep.done()


# ---- pixel-major: the CompatSoftmax backward ---------------------------------------------------------------------------
# (L, arith through PHL_COMPAT_ARITH, Potts-family Mu, route)
GRAD_CASES = [(32, None, False, "f32"), (256, "f32", False, "f32"), (256, "split", False, "split"), (384, None, False, "wide"),
              (64, None, True, "uniform")]


def _grad_contract(route, L, n, regime, logits):
    """The backward reuses the Q the forward kernel saved, so in softmax mode it misses the gradients' rule where the
    forward misses its own: k_compat_split at the offset regimes.  (This reading of the contract for the gradients -- their
    own rule with e_chain in place of e_torch, e_chain from float64 gradients evaluated at the model's Q -- is this file's;
    the issue spells the contract out for Q only.)"""
    return _on_e0(route, n) and regime in OFFSET_REGIMES and not logits


def _chain_grads(Ec, X, Mu, gout):
    """float64 gradients of softmax(-E) evaluated at the model's E: (gE0, gX, gMu)."""
    Q, g = torch.softmax(-Ec.double(), 1), gout.double()
    dE = Q * ((g * Q).sum(1, keepdim=True) - g)
    return dE, dE @ Mu.double().t(), X.double().t() @ dE


def _grad_case(rep, route, L, n, regime, logits, contract):
    import phl
    from test_gpu_compat_grad import _grads

    regs, X, Mu, _, gout = _operands(L, n, route == "uniform")
    E0 = padded_rows(regs[regime])
    name = f"compat grad {route} L={L} n={n} {regime} logits={logits}"
    f_ours = lambda e, x, m: phl.compat_softmax_fn(e, x, m, logits=logits)                          # noqa: E731
    f_torch = lambda e, x, m: (-(e + x @ m)) if logits else torch.softmax(-(e + x @ m), dim=1)     # noqa: E731
    with launch_spy(modeless=()) as seen:
        got = _grads(f_ours, E0, X, Mu, gout)
    assert set(_names(seen)) & COMPAT_ENTRIES == {ENTRY[route]}, (name, _names(seen))
    again = _grads(f_ours, E0, X, Mu, gout)
    if not all(torch.equal(a, b) for a, b in zip(got, again)):
        rep.fail(name, "two calls differ in their bits")
    ref32 = _grads(f_torch, E0, X, Mu, gout)
    want = _grads(f_torch, E0.double(), X.double(), Mu.double(), gout.double())
    chain = None
    if _on_e0(route, n) and not logits:
        chain = _chain_grads(_chain_energy(route, L, n, regime, E0, X, Mu), X, Mu, gout)
    bound = grad_bound
    if regime == "dominated" and not logits:     # the reference gradients are ~1e-83: an absolute bound, not the relative rule
        bound = lambda w, e_torch: 1e-6 * float(gout.abs().max())                                   # noqa: E731
    for k, what in ((1, "gE0"), (2, "gX"), (3, "gMu")):
        rep.judge(f"{name} {what}", got[k], ref32[k], want[k], bound=bound, chain=None if chain is None else chain[k - 1],
                  contract=contract)
    if regime == "masked" and not logits:
        rep.exact(name + " gE0", got[1], torch.isinf(E0), 0.0)


@pytest.mark.parametrize("L,arith,potts,route", GRAD_CASES)
def test_compat_softmax_backward(L, arith, potts, route, monkeypatch):
    if arith:
        monkeypatch.setenv("PHL_COMPAT_ARITH", arith)
    else:
        monkeypatch.delenv("PHL_COMPAT_ARITH", raising=False)
    rep = Report()
    for n in NS:
        for regime in REGIMES:
            for logits in (False, True):
                _grad_case(rep, route, L, n, regime, logits, contract=_grad_contract(route, L, n, regime, logits))
    rep.done()


@pytest.mark.xfail(strict=True, raises=AssertionError,
                   reason=XFAIL_ON_E0 + "L = 256, n = 293: gE0 4.5e-5 / 2.0e-6 at offset 3e2, 1.2e-2 / 5.1e-4 at offset 7.65e4, "
                   "4.9e-3 / 3.9e-4 at row_offsets, 3.0e-3 / 1.6e-4 at ties; gMu 1.9e-2 / 1.4e-3 at offset 7.65e4")
@pytest.mark.parametrize("L,arith,route,n,regime", [
    (L, arith, route, n, regime) for L, arith, _, route in GRAD_CASES for n in NS for regime in OFFSET_REGIMES
    if _grad_contract(route, L, n, regime, False)])
def test_compat_softmax_backward_project_rule_where_the_chain_starts_at_e0(L, arith, route, n, regime, monkeypatch):
    """The cases test_compat_softmax_backward holds to the chain contract, against the gradients' rule: expected to fail until
    k_compat_split's accumulators start from E0 - s_p."""
    if arith:
        monkeypatch.setenv("PHL_COMPAT_ARITH", arith)
    rep = Report()
    _grad_case(rep, route, L, n, regime, False, contract=False)
    rep.done()


# ---- channel-major -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cm_operands(L, H, W):
    gen = torch.Generator(device=DEV).manual_seed(77 * L + H)
    regs = {k: nchw(v, B, H, W) for k, v in regimes(B * H * W, L, gen).items()}
    G = torch.randn((B, L, H, W), device=DEV, generator=gen) * 5
    Mu = torch.rand((L, L), device=DEV, generator=gen) * 4 + torch.arange(L, device=DEV, dtype=torch.float32)[:, None] * 0.05
    gY = torch.randn((B, L, H, W), device=DEV, generator=gen)
    return regs, G, Mu, gY


def _rows(t):
    """[B, L, H, W] -> [B * H * W, L], the layout of the regimes."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _nchw_cases(L):
    for H, W in SHAPES:
        regs, G, Mu, gY = _cm_operands(L, H, W)
        for regime in REGIMES:
            E0 = regs[regime]
            assert on_float4_path(E0, G) == ((H * W) % 4 == 0)
            for g in (G, None):
                yield f"L={L} {H}x{W} {regime} G={'yes' if g is not None else 'no'}", regime, E0, g, Mu, gY


def _product_mode(rep, what, L, call, mode_seen, Mu_of):
    for name, regime, E0, g, Mu, _ in _nchw_cases(L):
        M = Mu_of(Mu)
        with launch_spy() as seen:
            hip = call(E0, g, M)
        assert seen == mode_seen, (name, seen)
        rep.judge(f"{what} {name}", hip, torch32(E0, g, M), truth(E0, g, M.double()))


@pytest.mark.parametrize("L", [3, 18, 64, 65, 256])
def test_nchw_product(L):
    import phl

    rep = Report()
    _product_mode(rep, "nchw product", L, lambda E0, g, M: phl.nchw_softmax_compat(E0, g, M),
                  [("phl_nchw_softmax_compat", PRODUCT)], lambda Mu: Mu)
    rep.done()


@pytest.mark.parametrize("L", [18, 300, 1024])
def test_nchw_uniform(L):
    import phl

    rep = Report()
    potts = 0.7 * torch.ones((L, L), device=DEV) - 1.3 * torch.eye(L, device=DEV)
    _product_mode(rep, "nchw uniform", L, lambda E0, g, M: phl.nchw_softmax_compat(E0, g, M),
                  [("phl_nchw_softmax_compat", UNIFORM)], lambda Mu: potts)
    rep.done()


@pytest.mark.parametrize("L", [257, 300, 512])
def test_nchw_wide(L):
    import phl

    rep = Report()
    _product_mode(rep, "nchw wide", L, lambda E0, g, M: phl.nchw_softmax_compat_wide(E0, g, M), [(WIDE, None)], lambda Mu: Mu)
    rep.done()


@pytest.mark.parametrize("L", [18, 300])
def test_nchw_softmax_and_logits(L):
    import phl

    rep = Report()
    for name, regime, E0, g, _, _ in _nchw_cases(L):
        with launch_spy() as seen:
            q = phl.nchw_softmax_compat(E0, g)
        assert seen == [("phl_nchw_softmax_compat", SOFTMAX)], (name, seen)
        want = F.softmax(-energy(E0.double(), None if g is None else g.double()), 1)
        _, e_torch = rep.judge(f"nchw softmax {name}", q, F.softmax(-energy(E0, g), 1), want)
        _q_checks(rep, f"nchw softmax {name}", _rows(q), _rows(want), e_torch, regime, _rows(E0), g)
        if g is None:
            continue
        with launch_spy() as seen:
            lg = phl.nchw_softmax_compat(E0, g, logits=True)
        assert seen == [("phl_nchw_softmax_compat", LOGITS)], (name, seen)
        rep.judge(f"nchw logits {name}", lg, -(E0 + g), -(E0.double() + g.double()))
        if regime == "masked":
            rep.exact(f"nchw logits {name}", lg, torch.isinf(E0), -INF)
    rep.done()


@pytest.mark.parametrize("L", [3, 18, 64])
def test_nchw_step_train_and_grad(L):
    """phl.nchw_step_train and phl.nchw_step_train_grad by the per-element rounding bounds of test_gpu_nchw_train.py."""
    import phl
    from test_gpu_nchw_train import _judge

    rep = Report()
    gen = torch.Generator(device=DEV).manual_seed(L)
    M = torch.randn((L, L), device=DEV, generator=gen)
    for name, regime, E0, g, _, gY in _nchw_cases(L):
        e, gg, gy = (None if t is None else t.reshape(B, L, -1) for t in (E0, g, gY))
        with launch_spy(modeless=("phl_nchw_step_train", "phl_nchw_step_train_grad")) as seen:
            Y = phl.nchw_step_train(e, gg, M)
            dE, gM = phl.nchw_step_train_grad(e, gg, M, gy)
        assert _names(seen) == ["phl_nchw_step_train", "phl_nchw_step_train_grad"], (name, seen)
        try:
            _judge(f"[measured] nchw train {name}", e, gg, M, gy, Y, dE, gM)
        except AssertionError as err:
            rep.fail(name, f"test_gpu_nchw_train._judge: {err}")
        if regime == "masked":
            rep.exact(name + " dE", dE, torch.isinf(e), 0.0)
    rep.done()


@pytest.mark.parametrize("L", [18, 300])
def test_nchw_expected_value_and_grad(L):
    """phl.nchw_expected_value and its gradient by the rule of test_gpu_nchw_expect.py (err_hip <= 2 err_t32, no absolute
    tolerance).  The regime is the ENERGY: X itself with ``negate``, -X without (softmax(+X) of a +inf is a NaN in torch)."""
    import phl
    from test_gpu_nchw_expect import _Worst, _autograd, _transcription

    rep, worst = Report(), _Worst()
    labels = torch.linspace(0, 40, L, device=DEV)
    for name, regime, E0, g, _, gY in _nchw_cases(L):
        gout = gY[:, :1].contiguous()
        for negate in (True, False):
            X, tag = (E0 if negate else -E0), f"{name} negate={negate}"
            with launch_spy(modeless=("phl_nchw_expected_value", "phl_nchw_expected_value_grad")) as seen:
                hip = phl.nchw_expected_value(X, g, labels, negate=negate)
                gz = phl.nchw_expected_value_grad(X, g, labels, gout, negate=negate)
            assert _names(seen) == ["phl_nchw_expected_value", "phl_nchw_expected_value_grad"], (tag, seen)
            try:
                worst.judge(f"[measured] nchw expect {tag}", hip, _transcription(X, g, labels, negate, torch.float32),
                            _transcription(X, g, labels, negate, torch.float64))
                worst.judge(f"[measured] nchw expect grad {tag}", gz, _autograd(X, g, labels, negate, gout, torch.float32),
                            _autograd(X, g, labels, negate, gout, torch.float64))
            except AssertionError as err:
                rep.fail(tag, f"test_gpu_nchw_expect._Worst.judge: {err}")
            if regime == "masked":
                rep.exact(tag + " gradient", gz, torch.isinf(X), 0.0)
    rep.done()


# ---- loops ---------------------------------------------------------------------------------------------------------------
class _W64(torch.autograd.Function):
    """The float64 twin of ``W @ U`` for a LatticeGaussian W: the fp32 filter applied to the fp32 head and tail of U, summed
    in float64; its backward is the same operator on the gradient (LatticeFilter's own backward)."""

    @staticmethod
    def forward(ctx, U, W):
        ctx.W = W
        hi = U.float()
        lo = (U - hi.double()).float()
        return (W @ hi).double() + (W @ lo).double()

    @staticmethod
    def backward(ctx, g):
        return _W64.apply(g, ctx.W), None


def _twin_loop(E0, W, Mu, niters, chain_route=None):
    """The plain loop in float64 on W's twin.  chain_route "split": every step's E carries the rounding of the accumulation
    model of the split route (as a constant, so that autograd gives the gradients of that perturbed forward)."""
    Q = torch.softmax(-E0, 1)
    for _ in range(niters):
        X = _W64.apply(Q, W)
        E = E0 + X @ Mu
        if chain_route == "split":
            Ec = _split_chain(E0.detach().float(), X.detach().float(), Mu.detach().float()).double()
            E = E + torch.where(torch.isfinite(Ec), Ec - E.detach(), torch.zeros_like(Ec))
        Q = torch.softmax(-E, 1)
    return Q


def _plain_loop(E0, W, Mu, niters):
    Q = F.softmax(-E0, dim=1)
    for _ in range(niters):
        Q = F.softmax(-(E0 + (W @ Q) @ Mu), dim=1)
    return Q


@functools.lru_cache(maxsize=None)
def _lattice_case(L):
    """A 40 x 56 image lattice (n = 2240 = 17 tiles + 64), the loop regimes, a Charbonnier Mu and an upstream gradient.
    Mu is scaled so that the regime stays what its name says, as X and G do in the single steps: Q's rows sum to 1, so the
    rows of |W Q| sum to at most gain = max(W 1) + 1 and |(W Q) Mu| <= gain * max|Mu|, which the scale sets to 8 -- the range
    of the regimes' ``base``."""
    from crf.crf_module import charbonneir, compatibility_matrix
    from crf.gaussian_matrix import LatticeGaussian

    h, w = 40, 56
    gen = torch.Generator(device=DEV).manual_seed(L)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32, device=DEV), torch.arange(w, dtype=torch.float32, device=DEV), indexing="ij")
    ref = torch.stack([yy / 6, xx / 6, torch.rand((h, w), device=DEV, generator=gen) * 3], dim=-1).reshape(h * w, 3).contiguous()
    regs = regimes(h * w, L, gen)
    Mu = compatibility_matrix(lambda a, b: charbonneir(a, b, 3.0), torch.arange(L, dtype=torch.float32, device=DEV))
    gain = float((LatticeGaussian(ref) @ torch.ones((h * w, 1), device=DEV)).abs().max()) + 1
    Mu = Mu * (8 / (gain * float(Mu.abs().max())))
    gout = torch.randn((h * w, L), device=DEV, generator=gen)
    return ref, regs, Mu.contiguous(), gout


# mean_field_infer at L = 200 runs k_compat_split every iteration: at the offset regimes the loop misses with it.  (The
# contract for a loop, e_new <= 2 max(e_old, e_chain) with e_chain from the loop run on the model, and for its gradients, their
# rule on e_chain, is this file's reading: the issue spells the contract out for the kernels' Q only.)
LOOP_ON_E0 = tuple(r for r in LOOP_REGIMES if r in OFFSET_REGIMES)


def _loop_contract(L, regime):
    return L > 176 and regime in LOOP_ON_E0


def _mean_field_case(rep, L, regime, fused_grad, contract):
    from crf.crf_module import mean_field_infer
    from crf.gaussian_matrix import LatticeGaussian
    from test_gpu_compat_grad import _check_graph

    ref, regs, Mu, gout = _lattice_case(L)
    E0, niters, route = regs[regime], 3, "split" if L > 176 else "f32"
    W = LatticeGaussian(ref)
    name = f"mean_field_infer L={L} {regime} fused_grad={fused_grad}"
    if not fused_grad:
        with torch.no_grad(), launch_spy(modeless=()) as seen:
            new = mean_field_infer(E0, W, Mu, niters)
            names = _names(seen)
            old = _plain_loop(E0, W, Mu, niters)
            want = _twin_loop(E0.double(), W, Mu.double(), niters)
            chain = _twin_loop(E0.double(), W, Mu.double(), niters, route) if route == "split" else None
            print(f"{name}: |(W Q) Mu| <= {float(((W @ new) @ Mu).abs().max()):.3g}")
        assert names.count(ENTRY[route]) == niters and names.count("phl_softmax_neg_add") == 1, names
        loop_judge(rep, name, new, old, want, chain, contract)
        if regime == "masked":
            rep.exact(name, new, torch.isinf(E0), 0.0)
        return
    res = {}
    for kind in ("new", "old", "want") + (("chain",) if route == "split" else ()):
        dtype = torch.float32 if kind in ("new", "old") else torch.float64
        e, m = (t.detach().clone().to(dtype).requires_grad_(True) for t in (E0, Mu))
        if kind == "new":
            Q = mean_field_infer(e, W, m, niters, fused_grad=True)
            _check_graph(Q, niters)
        elif kind == "old":
            Q = _plain_loop(e, W, m, niters)
        else:
            Q = _twin_loop(e, W, m, niters, route if kind == "chain" else None)
        Q.backward(gout.to(dtype))
        res[kind] = (Q.detach(), e.grad, m.grad)
    for k, what in ((0, "Q"), (1, "gE0"), (2, "gMu")):
        if k == 0:
            loop_judge(rep, f"{name} {what}", res["new"][k], res["old"][k], res["want"][k], res["chain"][k] if "chain" in res else None, contract)
        else:
            rep.judge(f"{name} {what}", res["new"][k], res["old"][k], res["want"][k], bound=grad_bound,
                      chain=res["chain"][k] if "chain" in res else None, contract=contract)
    if regime == "masked":
        rep.exact(name + " Q", res["new"][0], torch.isinf(E0), 0.0)
        rep.exact(name + " gE0", res["new"][1], torch.isinf(E0), 0.0)


@pytest.mark.parametrize("fused_grad", [False, True])
@pytest.mark.parametrize("L", [16, 200])
def test_mean_field_infer_loops(L, fused_grad):
    """mean_field_infer on a 40 x 56 image lattice, niters = 3, against the plain fp32 loop and its float64 twin (_W64: the
    lattice filter has no float64 form); with fused_grad=True the gradients of E_0 and Mu by the gradients' rule."""
    rep = Report()
    for regime in LOOP_REGIMES:
        _mean_field_case(rep, L, regime, fused_grad, contract=_loop_contract(L, regime))
    rep.done()


@pytest.mark.xfail(strict=True, raises=AssertionError,
                   reason=XFAIL_ON_E0 + "L = 200, Q after 3 iterations: 1.9e-2 / 3.1e-4 at offset 7.65e4, 1.9e-2 / 2.8e-4 at row_offsets; "
                   "gE0 4.1e-2 / 5.7e-4 and 1.6e-2 / 5.4e-4")
@pytest.mark.parametrize("regime", LOOP_ON_E0)
@pytest.mark.parametrize("fused_grad", [False, True])
@pytest.mark.parametrize("L", [200])
def test_mean_field_infer_loops_project_rule_where_the_chain_starts_at_e0(L, fused_grad, regime):
    rep = Report()
    _mean_field_case(rep, L, regime, fused_grad, contract=False)
    rep.done()


def _crf_inputs(regime):
    H, W, L = 24, 32, 18
    gen = torch.Generator(device=DEV).manual_seed(18)
    E0 = nchw(regimes(B * H * W, L, gen)[regime], B, H, W)
    img = torch.rand((B, 3, H, W), device=DEV, generator=gen)
    return -E0, img, torch.arange(L, dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("regime", LOOP_REGIMES)
def test_crfasrnn_channel_major_loop(regime):
    """CRFasRNN (logits = -E0) on the channel-major step kernels, 24 x 32, L = 18, niters = 3: through both_loops, against
    the float64 module."""
    from crf.crf_module import CRFasRNN, charb

    logits, img, labels = _crf_inputs(regime)
    refs = img[:, :1].contiguous()
    net = CRFasRNN(charb(3.0), niters=3, r=4).to(DEV)
    new, old = both_loops(lambda: net(refs, logits, labels=labels), net.niters)
    with torch.no_grad():
        want = net.double()(refs.double(), logits.double(), labels=labels.double())
    net.float()
    rep = Report()
    loop_judge(rep, f"CRFasRNN channel-major {regime}", new, old, want)
    if regime == "masked":
        rep.exact("CRFasRNN channel-major masked", new, torch.isinf(logits), -INF)
    rep.done()


def _crf_lattice_case(rep, regime):
    from crf import crf_module as cm
    from crf.gaussian_matrix import LatticeGaussian

    logits, img, labels = _crf_inputs(regime)
    Bn, L, H, W = logits.shape
    n, niters = H * W, 3
    refs = cm.ijrgbGuide(trainable=False).to(DEV)(img)
    net = cm.CRFasRNN(cm.charb(3.0), niters=niters, lattice=True).to(DEV)
    with torch.no_grad(), launch_spy(modeless=()) as seen:
        new = net(refs, logits, labels=labels)
    assert _names(seen).count("phl_compat_softmax") == niters * Bn, _names(seen)          # 18 labels run as 20 on the f32 kernel
    old = net(refs, logits.clone().requires_grad_(True), labels=labels).detach()          # autograd: the plain modules
    with torch.no_grad():
        M = cm._compat_matrix(net.Mu, L, labels, DEV)
        outs = []
        for b in range(Bn):
            Wb = LatticeGaussian(refs[b].reshape(-1, n).t().contiguous())
            e0 = (-logits[b]).reshape(L, n).t().contiguous()
            Q = torch.softmax(-e0.double(), 1)
            for _ in range(niters):                  # the reference's order: E = E0 + W(Mu(Q))
                E = e0.double() + _W64.apply(Q @ M.double(), Wb)
                Q = torch.softmax(-E, 1)
            outs.append((-E).t().reshape(L, H, W))
    loop_judge(rep, f"CRFasRNN lattice {regime}", new, old, torch.stack(outs))
    if regime == "masked":
        rep.exact("CRFasRNN lattice masked", new, torch.isinf(logits), -INF)


@pytest.mark.parametrize("regime", LOOP_REGIMES)
def test_crfasrnn_lattice_loop(regime):
    """CRFasRNN(lattice=True) without autograd (pixel-major inside, phl.compat_softmax per iteration) against the plain
    modules under autograd and the float64 twin of the reference's loop."""
    rep = Report()
    _crf_lattice_case(rep, regime)
    rep.done()
