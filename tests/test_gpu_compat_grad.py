"""The backward of the fused compatibility + softmax step (phl_compat_grad.hip through phl.CompatSoftmax /
phl.SoftmaxNegAdd): parity of the raw gradients against float64, only the gradients autograd asks for, determinism,
mean_field_infer(fused_grad=True), CRFasRNN(fused_grad=True) against reference-generated gradients and the plain path,
and a short notebook-shaped training run."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _leaf(t):
    """A leaf copy of t with t's own strides (clone() would make a row-padded view dense)."""
    u = torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device=t.device)
    return u.copy_(t.detach()).requires_grad_(True)


def _grads(fn, E0, X, Mu, gout):
    E0, X, Mu = (_leaf(t) for t in (E0, X, Mu))
    out = fn(E0, X, Mu)
    out.backward(gout)
    return out.detach(), E0.grad, X.grad, Mu.grad


def _graph_nodes(t):
    seen, stack, names = set(), [t.grad_fn], []
    while stack:
        f = stack.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        names.append(type(f).__name__)
        stack.extend(nf for nf, _ in f.next_functions)
    return names


def _check_graph(out, ncompat, node="CompatSoftmaxBackward"):
    names = _graph_nodes(out)
    for bad in ("MmBackward0", "SoftmaxBackward0", "ConvolutionBackward0", "AddmmBackward0", "BmmBackward0"):
        assert bad not in names, bad
    assert names.count(node) == ncompat, names.count(node)
    assert names.count("SoftmaxNegAddBackward") >= 1


@pytest.mark.parametrize("L", [4, 16, 32, 64, 100, 224, 256, 344, 512])
def test_compat_grad_parity(L):
    """gE0, gX, gMu of softmax(-(E0 + X Mu)) and of its logits against float64 autograd, for ragged n (1, 37, several
    128-pixel tiles plus every tail class of 4, ~140 k), an asymmetric Mu (a row-padded view of it in logits mode) and
    row-padded views of E0 and X.  Bound: twice
    the error of torch's fp32 autograd on the same operands plus 2.5e-7 of the largest magnitude (the Q the forward
    kernels save carries about two ulp of their hardware exp2 / reciprocal: a single row can show it)."""
    import phl

    g = torch.Generator(device="cuda").manual_seed(1000 + L)
    Mu = (torch.rand((L, L), device="cuda", generator=g) - 0.3) * (4.0 / L ** 0.5)
    Mu[: L // 2] *= 0.5
    if L > 4:
        assert not torch.equal(Mu, Mu.t())
    Mu_view = torch.full((L, L + 4), 1e3, device="cuda")[:, :L].copy_(Mu)       # row stride L + 4: the padding is poison
    assert Mu_view.stride(0) == L + 4
    for n in (1, 37, 128 * 3 + 1, 128 * 4 + 2, 128 * 5 + 3, 128 * 6, 140_003):
        for logits in (False, True):
            M = Mu_view if logits else Mu
            E0 = (torch.rand((n, L + 4), device="cuda", generator=g) * 8)[:, :L]
            X = (torch.rand((n, L + 8), device="cuda", generator=g) * 1.5 - 0.3)[:, :L]
            gout = torch.randn((n, L), device="cuda", generator=g)
            f_ours = lambda e, x, m: phl.compat_softmax_fn(e, x, m, logits=logits)               # noqa: E731
            f_torch = lambda e, x, m: (-(e + x @ m)) if logits else torch.softmax(-(e + x @ m), dim=1)   # noqa: E731
            got = _grads(f_ours, E0, X, M, gout)
            ref32 = _grads(f_torch, E0, X, M, gout)
            want = _grads(f_torch, E0.double(), X.double(), Mu.double(), gout.double())
            for k, name in ((1, "gE0"), (2, "gX"), (3, "gMu")):
                w = want[k]
                e_ours = float((got[k].double() - w).abs().max())
                e_torch = float((ref32[k].double() - w).abs().max())
                tol = 2 * e_torch + 2.5e-7 * float(w.abs().max())
                print(f"[measured] compat grad L={L} n={n} logits={logits} {name}: ours {e_ours:.2e} torch fp32 {e_torch:.2e} tol {tol:.2e}")
                assert e_ours <= tol, (L, n, logits, name, e_ours, tol)


def test_only_what_is_asked_and_potts_route(monkeypatch):
    """No phl_compat_mu_grad launch when Mu is fixed, no phl_compat_grad_x when X needs no gradient; the Potts family
    takes phl_uniform_compat_grad (dE and gX in one pass) and matches the dense route."""
    import phl

    lib = phl.load_library()
    calls = []
    for name in ("phl_compat_mu_grad", "phl_compat_grad_x", "phl_uniform_compat_grad", "phl_softmax_neg_grad"):
        real = getattr(lib, name)

        def spy(*a, _real=real, _name=name):
            calls.append(_name)
            return _real(*a)
        monkeypatch.setattr(lib, name, spy)
    L, n = 64, 128 * 7 + 3
    g = torch.Generator(device="cuda").manual_seed(5)
    E0 = (torch.rand((n, L), device="cuda", generator=g) * 5).requires_grad_(True)
    X = torch.rand((n, L), device="cuda", generator=g)
    Mu = torch.rand((L, L), device="cuda", generator=g)
    phl.compat_softmax_fn(E0, X, Mu).sum().backward()
    assert "phl_compat_mu_grad" not in calls and "phl_compat_grad_x" not in calls, calls
    assert calls.count("phl_softmax_neg_grad") == 1, calls
    calls.clear()
    X.requires_grad_(True)
    phl.compat_softmax_fn(E0, X, Mu, logits=True).sum().backward()
    assert calls == ["phl_compat_grad_x"], calls
    calls.clear()
    Mu.requires_grad_(True)
    gout = torch.randn((n, L), device="cuda", generator=g)
    phl.compat_softmax_fn(E0, X, Mu).backward(gout)
    assert sorted(calls) == ["phl_compat_grad_x", "phl_compat_mu_grad", "phl_softmax_neg_grad"], calls

    P = (0.7 * torch.ones((L, L), device="cuda") - 1.3 * torch.eye(L, device="cuda"))
    for logits in (False, True):
        calls.clear()
        r = _grads(lambda e, x, m: phl.compat_softmax_fn(e, x, m, logits=logits), E0, X, P, gout)
        assert "phl_uniform_compat_grad" in calls and "phl_compat_grad_x" not in calls, calls
        calls.clear()
        d = _grads(lambda e, x, m: phl.compat_softmax_fn(e, x, m, logits=logits, uniform=False), E0, X, P, gout)
        assert "phl_uniform_compat_grad" not in calls and "phl_compat_grad_x" in calls, calls
        for k in (0, 1, 2, 3):
            err = float((r[k] - d[k]).abs().max() / d[k].abs().max())
            assert err <= 1e-5, (logits, k, err)


def test_backward_is_deterministic():
    """Two backward passes at ~140 k pixels and 256 labels give the same gMu and gX bit for bit."""
    import phl

    L, n = 256, 140_003
    g = torch.Generator(device="cuda").manual_seed(9)
    E0 = torch.rand((n, L), device="cuda", generator=g) * 8
    X = torch.rand((n, L), device="cuda", generator=g)
    Mu = (torch.rand((L, L), device="cuda", generator=g) - 0.5) * 0.2
    gout = torch.randn((n, L), device="cuda", generator=g)
    a = _grads(phl.compat_softmax_fn, E0, X, Mu, gout)
    b = _grads(phl.compat_softmax_fn, E0, X, Mu, gout)
    assert torch.equal(a[3], b[3]) and torch.equal(a[2], b[2]) and torch.equal(a[1], b[1])


def _plain_loop(E0, W, Mu, niters):
    import torch.nn.functional as F

    Q = F.softmax(-E0, dim=1)
    for _ in range(niters):
        Q = F.softmax(-(E0 + (W @ Q) @ Mu), dim=1)
    return Q


@pytest.mark.parametrize("L", [32, 231])
def test_mean_field_infer_fused_grad(L):
    """mean_field_infer(fused_grad=True) with E_0, Mu and a LatticeGaussian(ref) all requiring grad: Q within 1e-5 of
    the plain torch loop, the gradients of E_0, Mu and ref within 1e-4 of their largest magnitude, and a graph with no
    torch matrix product, softmax or convolution, and exactly niters CompatSoftmax nodes.  Then with only ref requiring
    grad: the loop finds W's graph at its first ``W @ Q`` and continues on the Functions from there."""
    from crf.crf_module import charbonneir, compatibility_matrix, mean_field_infer
    from crf.gaussian_matrix import LatticeGaussian

    z = np.load(os.path.join(GOLDEN, "meanfield_tsukuba_L32.npz"))
    n = z["E0"].shape[0]
    g = torch.Generator(device="cuda").manual_seed(L)
    if L == 32:
        E0 = torch.from_numpy(z["E0"]).cuda()
    else:
        E0 = torch.rand((n, L), device="cuda", generator=g) * 3
    # (energies of the same size at both label counts: a sharper softmax would only measure its own conditioning)
    Mu = compatibility_matrix(lambda a, b: charbonneir(a, b, 3.0), torch.arange(L, dtype=torch.float32, device="cuda")) * (9.6 / L if L == 32 else 4.8 / L)
    ref = torch.from_numpy(z["ref"]).cuda()
    gout = torch.randn((n, L), device="cuda", generator=g)
    niters = 4
    res = {}
    for fused in (True, False):
        e, m, r = (t.clone().requires_grad_(True) for t in (E0, Mu, ref))
        Q = mean_field_infer(e, LatticeGaussian(r), m, niters, fused_grad=True) if fused else _plain_loop(e, LatticeGaussian(r), m, niters)
        if fused:
            _check_graph(Q, niters)
        Q.backward(gout)
        res[fused] = (Q.detach(), e.grad, m.grad, r.grad)
    dq = float((res[True][0] - res[False][0]).abs().max())
    print(f"[measured] mean_field_infer fused_grad L={L}: |dQ| {dq:.2e}")
    assert dq <= 1e-5, dq
    for k, name in ((1, "E_0"), (2, "Mu"), (3, "ref")):
        err = float((res[True][k] - res[False][k]).abs().max() / res[False][k].abs().max())
        print(f"[measured] mean_field_infer fused_grad L={L} grad {name}: rel {err:.2e}")
        assert err <= 1e-4, (name, err)

    # only W's features require grad
    res = {}
    for fused in (True, False):
        r = ref.clone().requires_grad_(True)
        Q = mean_field_infer(E0, LatticeGaussian(r), Mu, niters, fused_grad=True) if fused else _plain_loop(E0, LatticeGaussian(r), Mu, niters)
        if fused:
            names = _graph_nodes(Q)
            assert names.count("CompatSoftmaxBackward") == niters, names.count("CompatSoftmaxBackward")
            assert "MmBackward0" not in names and "SoftmaxBackward0" not in names
        Q.backward(gout)
        res[fused] = (Q.detach(), r.grad)
    dq = float((res[True][0] - res[False][0]).abs().max())
    err = float((res[True][1] - res[False][1]).abs().max() / res[False][1].abs().max())
    print(f"[measured] mean_field_infer fused_grad L={L}, ref only: |dQ| {dq:.2e}, grad ref rel {err:.2e}")
    assert dq <= 1e-5 and err <= 1e-4, (dq, err)


def _crf_case(mu, fused, z, trainable=True, labels=True):
    from crf.crf_module import CRFasRNN, ijrgbGuide

    net = CRFasRNN(mu, niters=int(z["niters"]), lattice=True, fused_grad=fused).cuda()
    guide = ijrgbGuide(float(z["s_ij"]), float(z["s_rgb"]), trainable=trainable).cuda()
    logits = torch.from_numpy(z["logits"]).cuda().requires_grad_(True)
    lab = torch.from_numpy(z["labels"]).cuda() if labels else None     # (a conv Mu takes no labels)
    out = net(guide(torch.from_numpy(z["img"]).cuda()), logits, labels=lab)
    return net, guide, logits, out


def test_crfasrnn_fused_grad_matches_reference_and_plain():
    """CRFasRNN(charb(3.0), lattice=True, fused_grad=True) with a trainable guide: the gradients of the logits, gamma, s,
    s_ij and s_rgb within 1e-4 relative of the reference's own backward (crfasrnn_train.npz) and of the plain path; the
    graph has no torch matrix product, softmax or convolution, and one CompatProduct per image and iteration."""
    from crf.crf_module import charb

    z = np.load(os.path.join(GOLDEN, "crfasrnn_train.npz"))
    g_out = torch.from_numpy(z["g_out"]).cuda()
    got = {}
    for fused in (True, False):
        net, guide, logits, out = _crf_case(charb(float(z["gamma"])), fused, z)
        if fused:
            _check_graph(out, int(z["niters"]) * out.shape[0], node="CompatProductBackward")
        (out * g_out).sum().backward()
        got[fused] = dict(out=out.detach().cpu().numpy(), logits=logits.grad.cpu().numpy(), gamma=net.Mu.gamma.grad.cpu().numpy(),
                          s=net.Mu.s.grad.cpu().numpy(), s_ij=guide.s_ij.grad.cpu().numpy(), s_rgb=guide.s_rgb.grad.cpu().numpy())
    errs = {}
    for key in ("out", "logits", "gamma", "s", "s_ij", "s_rgb"):
        want = z["grad_" + key] if key != "out" else z["out"]
        for fused, tag in ((True, "fused"), (False, "plain")):
            errs[(tag, key)] = e = float(np.abs(got[fused][key] - want).max() / np.abs(want).max())
            print(f"[measured] CRFasRNN {tag} {key}: rel err vs reference {e:.2e}")
        errs[("fused-plain", key)] = e = float(np.abs(got[True][key] - got[False][key]).max() / np.abs(got[False][key]).max())
        print(f"[measured] CRFasRNN fused vs plain {key}: rel {e:.2e}")
    bad = {k: v for k, v in errs.items() if k[0] != "plain" and v > 1e-4}
    assert not bad, bad


def test_crfasrnn_fused_grad_potts_conv():
    """CRFasRNN(potts(L), lattice=True, fused_grad=True): the 1x1 conv weight's gradient matches the plain path."""
    from crf.crf_module import potts

    z = np.load(os.path.join(GOLDEN, "crfasrnn_train.npz"))
    g_out = torch.from_numpy(z["g_out"]).cuda()
    L = z["logits"].shape[1]
    res = {}
    for fused in (True, False):
        torch.manual_seed(0)
        net, guide, logits, out = _crf_case(potts(L), fused, z, labels=False)
        if fused:
            _check_graph(out, int(z["niters"]) * out.shape[0], node="CompatProductBackward")
        (out * g_out).sum().backward()
        res[fused] = (net.Mu.weight.grad.clone(), logits.grad.clone(), guide.s_ij.grad.clone())
    for k in range(3):
        e = float((res[True][k] - res[False][k]).abs().max() / res[False][k].abs().max())
        print(f"[measured] CRFasRNN potts fused vs plain grad {k}: rel {e:.2e}")
        assert e <= 1e-4, (k, e)


def test_notebook_shaped_training():
    """10 Adam steps of CRFasRNN(charb(.05)) with a trainable ijrgbGuide on a 48x64 Tsukuba crop (L = 16), fused against
    plain: per-step losses within 1e-4 relative, and so are the parameters afterwards."""
    import torch.nn.functional as F

    from crf.crf_module import CRFasRNN, charb, ijrgbGuide

    z = np.load(os.path.join(GOLDEN, "meanfield_tsukuba_crop.npz"))
    h, w = int(z["h"]), int(z["w"])
    L = z["E0"].shape[1]
    img = torch.from_numpy((z["ref"][:, :3] * 0.1).reshape(1, h, w, 3).transpose(0, 3, 1, 2).copy()).cuda()
    E0 = torch.from_numpy(z["E0"].reshape(1, h, w, L).transpose(0, 3, 1, 2).copy()).cuda()
    logits0 = -E0 / E0.std()
    target = E0.argmin(1)
    runs = {}
    for fused in (True, False):
        net = CRFasRNN(charb(0.05), niters=5, lattice=True, fused_grad=fused).cuda()
        guide = ijrgbGuide(trainable=True).cuda()
        opt = torch.optim.Adam(list(net.parameters()) + list(guide.parameters()), lr=2e-3)
        losses = []
        for _ in range(10):
            opt.zero_grad()
            out = net(guide(img), logits0, labels=torch.arange(L, dtype=torch.float32, device="cuda"))
            loss = F.cross_entropy(out, target)
            loss.backward()
            opt.step()
            losses.append(float(loss))
        params = [float(p) for p in (net.Mu.gamma, net.Mu.s, guide.s_ij, guide.s_rgb)]
        runs[fused] = (losses, params)
    print(f"[measured] training losses fused {runs[True][0]} plain {runs[False][0]}; params fused {runs[True][1]} plain {runs[False][1]}")
    for a, b in zip(runs[True][0], runs[False][0]):
        assert abs(a - b) <= 1e-4 * abs(b), (a, b)
    for a, b in zip(runs[True][1], runs[False][1]):
        assert abs(a - b) <= 1e-4 * max(abs(b), 1e-3), (a, b)
