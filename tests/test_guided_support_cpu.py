"""The judge of the guided-filter GPU tests, judged without a GPU: _guided_util's accuracy rule (``report``), its spy with
``route``, and its table of the four variants.  CPU tensors only; ``import phl`` does not load the library."""
import inspect

import pytest
import torch

import _guided_util as util
from _guided_util import SPIED, VARIANTS, kernel_route, report, route, spy

U = 2.0 ** -24


def _case(e_hip, e_torch):
    """want with max|want| = 1 (so u = 2^-24), and two results off by e_hip and e_torch in one element each."""
    want = torch.tensor([1.0, 0.5, 0.25], dtype=torch.float64)
    hip, t32 = want.clone(), want.clone()
    hip[1] += e_hip
    t32[2] -= e_torch
    return hip, t32, want


def test_report_passes_a_case_that_meets_all_three():
    hip, t32, want = _case(9 * U, 10 * U)
    e_hip, e_torch, mag = report("ok", hip, t32, want, min_torch_u=8)
    assert (e_hip, e_torch, mag) == (9 * U, 10 * U, 1.0)
    report("ok, factor 2", *_case(20 * U, 10 * U), factor=2)
    report("ok, no precondition", *_case(0.0, U))


def test_report_raises_above_the_factor():
    with pytest.raises(AssertionError):
        report("worse", *_case(11 * U, 10 * U), min_torch_u=8)
    with pytest.raises(AssertionError):
        report("worse, factor 2", *_case(21 * U, 10 * U), factor=2)


def test_report_raises_on_an_unmet_precondition():
    hip, t32, want = _case(0.0, 7 * U)
    report("no precondition", hip, t32, want)
    with pytest.raises(AssertionError, match="precondition"):
        report("too exact", hip, t32, want, min_torch_u=8)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_report_raises_on_a_non_finite_result(bad):
    hip, t32, want = _case(0.0, 10 * U)
    hip[0] = bad
    with pytest.raises(AssertionError):
        report("non-finite", hip, t32, want)
    t32[0] = bad                                    # ... whatever the torch form gives
    with pytest.raises(AssertionError):
        report("both non-finite", hip, t32, want)


@pytest.fixture
def stubs(monkeypatch):
    """The seven spied names replaced by stubs that return their own name: nothing of the library is called."""
    import phl
    from crf import guided

    where = {key: (phl, name) for key, name in SPIED.items()}
    where["box_sum"] = (guided, "_box_sum")
    for key, (mod, name) in where.items():
        monkeypatch.setattr(mod, name, lambda *a, _key=key, **k: (_key, a, k))
    return where


def test_spy_counts_each_of_its_seven_names(stubs):
    assert len(stubs) == 7 and set(stubs) == set(route())
    with spy() as calls:
        assert calls == route()
        for n, (key, (mod, name)) in enumerate(stubs.items(), 1):
            for _ in range(n):
                assert getattr(mod, name)(1, two=2) == (key, (1,), {"two": 2})        # arguments and result pass through
            assert calls[key] == n and sum(calls.values()) == n * (n + 1) // 2
    assert calls == route(**{key: n for n, key in enumerate(stubs, 1)})


def test_spy_restores_every_attribute_when_the_body_raises(stubs):
    before = {key: getattr(mod, name) for key, (mod, name) in stubs.items()}
    with pytest.raises(RuntimeError):
        with spy():
            assert all(getattr(mod, name) is not before[key] for key, (mod, name) in stubs.items())
            raise RuntimeError
    assert all(getattr(mod, name) is before[key] for key, (mod, name) in stubs.items())


def test_route_equality_distinguishes_each_key():
    keys = list(route())
    assert keys == list(SPIED) + ["box_sum"] and all(v == 0 for v in route().values())
    for key in keys:
        assert route(**{key: 1}) != route() and route(**{key: 1}) != route(**{key: 2})
        for other in keys:
            assert (route(**{key: 1}) == route(**{other: 1})) == (key == other)
    with pytest.raises(AssertionError):
        util.torch_route(route(nearest=1))
    assert util.torch_route(route(nearest=1, box_sum=3)) == route(box_sum=3) != route(nearest=1, box_sum=3)


@pytest.mark.parametrize("variant", list(VARIANTS), ids=["-".join(k) for k in VARIANTS])
def test_variant_table_names_what_exists(variant):
    import phl

    v = VARIANTS[variant]
    assert variant[0] in ("nearest", "bilinear") and variant[1] in ("diagonal", "full")
    forward, backward, function = (getattr(phl, name) for name in (v.forward, v.backward, v.function))
    assert callable(forward) and callable(backward) and issubclass(function, torch.autograd.Function)
    assert v.forward in SPIED.values() and v.backward in SPIED.values()
    assert set(v.call) <= set(inspect.signature(forward).parameters)
    assert kernel_route(variant, 2) == route(**{k: 2 for k, name in SPIED.items() if name in (v.forward, v.backward)})
    assert sum(kernel_route(variant, grad=False).values()) == 1
    # the constructors take the keywords, and the gradient keyword passes their checks with the route's keywords alone
    for kind in ("fast", "bga") + (("gf",) if variant[0] == "nearest" else ()):
        assert getattr(util.module(kind, 3, 4, 2, 1e-2, variant), v.grad_kw) is False
        m = util.module(kind, 3, 4, 2, 1e-2, variant, **{v.grad_kw: True})
        assert getattr(m, v.grad_kw) is True and all(getattr(m, k) == val for k, val in v.ctor.items())
    # the diagonal counterpart: the same interpolation, the diagonal model, the same direct call but for ``call``
    assert (v.diagonal is None) == (variant[1] == "diagonal") and v.call == ({} if v.diagonal is None else {"full_cov": True})
    if v.diagonal is not None:
        d = VARIANTS[v.diagonal]
        assert v.diagonal == (variant[0], "diagonal") and d.forward == v.forward and d.backward != v.backward
