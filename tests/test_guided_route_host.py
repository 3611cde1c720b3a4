"""The route table of the guided-filter W (crf.guided._guided_route) and the keyword rules (_check_guided_keywords),
pinned from plain values.  The table: the full product of the function's inputs against the docstring's rows written out
here.  The dispatch: every class with every keyword combination its constructor admits, the kernels replaced by stubs
that return a tag, GuidedFilter._fused driven with small CPU tensors -- the tag is the one the table names.  The
constructors: success or the exception type of every combination of the boolean keywords and ``mode``, for the four
guided classes, CRFasRNN and the two heads, as the package gave them before the rules moved into one function.  No GPU."""
import itertools

import pytest
import torch

MODES = ("nearest", "bilinear", "bicubic")
FILTER_KW = ("gaussian", "fused_grad", "full_cov", "full_cov_grad")
FAST_KW = FILTER_KW + ("fused_bilinear", "bilinear_grad", "bilinear_full_grad")
HEAD_KW = FAST_KW[1:]
R, EPS, CX = 4, 1e-2, 2
ADJACENCY_SCALE = 0.5 * (2 * R + 1) ** 2


def combinations(names, modes=MODES):
    """Every value of the boolean keywords ``names``, the first one slowest, under every mode (None: the class has none)."""
    for mode in modes:
        for values in itertools.product((False, True), repeat=len(names)):
            yield dict(zip(names, values), **({} if mode is None else {"mode": mode}))


# ---- the constructors ---------------------------------------------------------------------------------------------------
def _guided(name):
    def build(kw):
        from crf import guided

        return getattr(guided, name)(CX, R, EPS, **kw)
    return build


def _adjacency(kw):
    from crf import guided

    return guided.GuidedAdjacency(torch.zeros(1, CX, 6, 8), R, EPS, **kw)


def _engine(lattice):
    def build(kw):
        from crf.crf_module import CRFasRNN, charb

        return CRFasRNN(charb(3.0), niters=1, r=R, eps=EPS, gchannels=CX, lattice=lattice, **kw)
    return build


def _head(name, lattice):
    def build(kw):
        from crf import mb_stereo_crf

        return getattr(mb_stereo_crf, name)(d_in=4, d_guide=5, r=R, niters=1, lattice=lattice, **kw)
    return build


# case -> (its keywords in the order of ``combinations``, its modes, the constructor call)
CONSTRUCTORS = {
    "GuidedFilter": (FILTER_KW, (None,), _guided("GuidedFilter")),
    "FastGuidedFilter": (FAST_KW, MODES, _guided("FastGuidedFilter")),
    "BatchedGuidedAdjacency": (FAST_KW, MODES, _guided("BatchedGuidedAdjacency")),
    "CRFasRNN": (FAST_KW, MODES, _engine(False)),
    "CRFasRNN lattice": (FAST_KW, MODES, _engine(True)),
    "CRFdepthRefiner": (HEAD_KW, MODES, _head("CRFdepthRefiner", False)),
    "CRFdepthRefiner lattice": (HEAD_KW, MODES, _head("CRFdepthRefiner", True)),
    "CRFdepthUpsampler": (HEAD_KW, MODES, _head("CRFdepthUpsampler", False)),
    "CRFdepthUpsampler lattice": (HEAD_KW, MODES, _head("CRFdepthUpsampler", True)),
}
_LETTER = {None: ".", ValueError: "V", NotImplementedError: "N"}


def constructor_outcomes(case):
    """One letter per combination, in the order of ``combinations``: '.' constructs, 'V' ValueError, 'N' NotImplementedError
    (the exact type), '?' anything else."""
    names, modes, build = CONSTRUCTORS[case]
    out = []
    for kw in combinations(names, modes):
        try:
            build(kw)
            out.append(_LETTER[None])
        except Exception as e:  # noqa: BLE001
            out.append(_LETTER.get(type(e), "?"))
    return "".join(out)


# The outcomes before the rules moved into _check_guided_keywords, one string per mode.  Within a string the keywords
# count in binary, the first of the case's keywords (CONSTRUCTORS) being the highest bit.
_FAST = (".VVVVVVVVVVVVVVV.VVVVVVV.VVVVVVV.VVVVVVVVVVVVVVV.VVVVVVV.VVVVVVV"
         "NNNNNNNNVVVVVVVVNNNNNNNNNNNNNNNNNNNNNNNNVVVVVVVVNNNNNNNNNNNNNNNN",
         ".VVV.V.VVVVVVVVV.VVV..NN.VVV..NN.VVV.V.VVVVVVVVV.VVV..NN.VVV..NN"
         "NNNNNNNNVVVVVVVVNNNNNNNNNNNNNNNNNNNNNNNNVVVVVVVVNNNNNNNNNNNNNNNN",
         ".VVVVVVVVVVVVVVV.VVVVVVV.VVVVVVV.VVVVVVVVVVVVVVV.VVVVVVV.VVVVVVV"
         "NNNNNNNNVVVVVVVVNNNNNNNNNNNNNNNNNNNNNNNNVVVVVVVVNNNNNNNNNNNNNNNN")
_ENGINE = (".VVVVVVVVVVVVVVV.VVVVVVV.VVVVVVV.VVVVVVVVVVVVVVV.VVVVVVV.VVVVVVV"
           "NVVVNVNVVVVVVVVVNVVVNNNNNVVVNNNNNVVVNVNVVVVVVVVVNVVVNNNNNVVVNNNN",
           ".VVV.V.VVVVVVVVV.VVV..NN.VVV..NN.VVV.V.VVVVVVVVV.VVV..NN.VVV..NN"
           "NVVVNVNVVVVVVVVVNVVVNNNNNVVVNNNNNVVVNVNVVVVVVVVVNVVVNNNNNVVVNNNN",
           ".VVVVVVVVVVVVVVV.VVVVVVV.VVVVVVV.VVVVVVVVVVVVVVV.VVVVVVV.VVVVVVV"
           "NVVVNVNVVVVVVVVVNVVVNNNNNVVVNNNNNVVVNVNVVVVVVVVVNVVVNNNNNVVVNNNN")
_ENGINE_LATTICE = (".VVVVVVVVVVVVVVVVVVVVVVVVVVVVVVV.VVVVVVVVVVVVVVVVVVVVVVVVVVVVVVV"
                   ".VVVVVVVVVVVVVVVVVVVVVVVVVVVVVVV.VVVVVVVVVVVVVVVVVVVVVVVVVVVVVVV",
                   "VVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVV"
                   "VVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVV",
                   "VVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVV"
                   "VVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVVV")
_HEADS = tuple(s[:64] for s in _ENGINE)                         # the heads have no ``gaussian``: CRFasRNN's without it
_HEADS_LATTICE = tuple(s[:64] for s in _ENGINE_LATTICE)
OUTCOMES = {
    "GuidedFilter": (".V...V...VNN.VNN",),
    "FastGuidedFilter": _FAST,
    "BatchedGuidedAdjacency": _FAST,
    "CRFasRNN": _ENGINE,
    "CRFasRNN lattice": _ENGINE_LATTICE,
    "CRFdepthRefiner": _HEADS,
    "CRFdepthRefiner lattice": _HEADS_LATTICE,
    "CRFdepthUpsampler": _HEADS,
    "CRFdepthUpsampler lattice": _HEADS_LATTICE,
}


@pytest.mark.parametrize("case", list(CONSTRUCTORS))
def test_every_keyword_combination_constructs_or_raises_as_before(case):
    names, modes, _ = CONSTRUCTORS[case]
    got, want = constructor_outcomes(case), "".join(OUTCOMES[case])
    assert len(want) == len(modes) * 2 ** len(names) and "?" not in got
    wrong = [(kw, a, b) for kw, a, b in zip(combinations(names, modes), got, want) if a != b]
    assert not wrong, wrong[:5]


def test_two_broken_rules_raise_the_first():
    """The example of the order: bilinear_grad and bilinear_full_grad together, with full_cov, is the diagonal keyword on the
    full model (NotImplementedError), from every constructor that takes them."""
    kw = dict(mode="bilinear", fused_bilinear=True, full_cov=True, bilinear_grad=True, bilinear_full_grad=True)
    for case in ("FastGuidedFilter", "BatchedGuidedAdjacency", "CRFasRNN", "CRFdepthRefiner", "CRFdepthUpsampler"):
        with pytest.raises(NotImplementedError):
            CONSTRUCTORS[case][2](kw)


# ---- the table ------------------------------------------------------------------------------------------------------------
ROUTE_INPUTS = ("gaussian", "mode", "fused_bilinear", "full_cov", "subsample", "operands_ok", "recording", "fused_grad",
                "full_cov_grad", "bilinear_grad", "bilinear_full_grad")
_BILINEAR_KEYWORDS = ("bilinear_grad", "bilinear_full_grad")
# The rows of _guided_route's docstring: (mode, needs fused_bilinear, full_cov, subsample >= 2 or None for any, the
# keywords of which one admits a recorded forward) -> (bilinear_kernels, full_cov).  All rows: a box window, operands_ok.
TABLE_ROWS = [
    (("nearest", False, False, None, ("fused_grad",)), (False, False)),
    (("nearest", False, True, None, ("full_cov_grad",)), (False, True)),
    (("bilinear", True, False, True, _BILINEAR_KEYWORDS), (True, False)),
    (("bilinear", True, True, True, _BILINEAR_KEYWORDS), (True, True)),
    (("bilinear", True, False, False, _BILINEAR_KEYWORDS), (False, False)),       # subsample 1: the nearest kernels
    (("bilinear", True, True, False, _BILINEAR_KEYWORDS), (False, True)),
]


def table_route(**v):
    """The docstring's table as rules: the one row whose preconditions hold, or "torch"."""
    if v["gaussian"] or not v["operands_ok"]:
        return "torch"
    found = []
    for (mode, needs_fused, full_cov, coarse, keywords), kernels in TABLE_ROWS:
        if v["mode"] != mode or (needs_fused and not v["fused_bilinear"]) or bool(v["full_cov"]) != full_cov:
            continue
        if coarse is not None and (v["subsample"] >= 2) != coarse:
            continue
        if v["recording"] and not any(v[k] for k in keywords):
            continue
        found.append(kernels + (bool(v["recording"]),))
    assert len(found) <= 1, (v, found)
    return found[0] if found else "torch"


def test_the_table_over_the_full_product_of_its_inputs():
    from crf.guided import _guided_route

    values = {k: (False, True) for k in ROUTE_INPUTS}
    values.update(mode=MODES, subsample=(1, 2, 3))
    seen = set()
    for combo in itertools.product(*(values[k] for k in ROUTE_INPUTS)):
        v = dict(zip(ROUTE_INPUTS, combo))
        got = _guided_route(**v)
        assert got == table_route(**v), v
        assert got == "torch" or (type(got) is tuple and all(type(t) is bool for t in got)), (v, got)
        seen.add(got)
    assert seen == {"torch"} | set(itertools.product((False, True), repeat=3))       # every route is reached


def test_the_two_asymmetries_of_the_table():
    from crf.guided import _guided_route

    base = dict(gaussian=False, mode="bilinear", fused_bilinear=True, full_cov=False, subsample=2, operands_ok=True,
                recording=True, fused_grad=False, full_cov_grad=False, bilinear_grad=False, bilinear_full_grad=False)
    # either bilinear keyword admits a recorded bilinear forward, whatever full_cov says; the nearest keywords do not
    for full_cov in (False, True):
        for keyword in _BILINEAR_KEYWORDS:
            assert _guided_route(**{**base, "full_cov": full_cov, keyword: True}) == (True, full_cov, True)
        assert _guided_route(**{**base, "full_cov": full_cov, "fused_grad": True, "full_cov_grad": True}) == "torch"
    # at subsample 1 a recorded forward lands on the nearest Function of its model
    for full_cov in (False, True):
        assert _guided_route(**{**base, "full_cov": full_cov, "subsample": 1, "bilinear_grad": True}) == (False, full_cov, True)


# ---- the dispatch ---------------------------------------------------------------------------------------------------------
FORWARDS = ("guided_filter", "guided_filter_bilinear")
FUNCTIONS = ("GuidedFilterFn", "GuidedFilterFullFn", "GuidedFilterBilinearFn", "GuidedFilterBilinearFullFn")
# (bilinear_kernels, full_cov) -> the names in phl of the forward and of the Function of a recorded one
KERNELS = {(False, False): ("guided_filter", "GuidedFilterFn"), (False, True): ("guided_filter", "GuidedFilterFullFn"),
           (True, False): ("guided_filter_bilinear", "GuidedFilterBilinearFn"),
           (True, True): ("guided_filter_bilinear", "GuidedFilterBilinearFullFn")}
RECORDINGS = {"no_grad": False, "frozen": False, "omega": True, "y": True}     # how a call is made -> autograd records it
OPERANDS = ("ok", "y3d", "x3d", "not_hip", "omega_not_hip")


def install_stubs(monkeypatch, status=None):
    """crf.guided._hip_ok says yes; the two forwards of phl and ``apply`` of the four Functions return a tag of their
    name and arguments (the forwards: full_cov last; the Functions: None there) -- or raise PhlError(status)."""
    import phl
    from crf import guided

    monkeypatch.setattr(guided, "_hip_ok", lambda t: True)

    def forward(name):
        def f(y, x, r, eps, *, subsample=1, scale=1.0, subtract=None, full_cov=False):
            if status is not None:
                raise phl.PhlError(status, "stub")
            assert subtract is None or subtract is y
            return (name, int(r), int(subsample), float(scale), subtract is not None, bool(full_cov))
        return f

    def apply(name):
        def f(y, x, eps, r, subsample, scale, subtract_is_y):
            if status is not None:
                raise phl.PhlError(status, "stub")
            assert eps.requires_grad or not torch.is_grad_enabled()        # eps = softplus(omega) keeps its graph
            return (name, int(r), int(subsample), float(scale), bool(subtract_is_y), None)
        return staticmethod(f)

    for name in FORWARDS:
        monkeypatch.setattr(phl, name, forward(name))
    for name in FUNCTIONS:
        monkeypatch.setattr(getattr(phl, name), "apply", apply(name))


def dispatch_cases():
    """(key, module, keywords, subsample): each of the four classes with every keyword combination its constructor
    admits, FastGuidedFilter and BatchedGuidedAdjacency at subsample_ratio 1 and 2, the other two (which have no ratio)
    driven at both."""
    for name, (names, modes, build) in list(CONSTRUCTORS.items())[:3]:
        for kw in combinations(names, modes):
            for s in (1, 2):
                try:
                    m = build(kw if name == "GuidedFilter" else dict(kw, subsample_ratio=s))
                except (ValueError, NotImplementedError):
                    continue
                yield f"{name} {sorted(kw.items())} s{s}", m, kw, s
    for full_cov in (False, True):
        for s in (1, 2):
            yield f"GuidedAdjacency full_cov={full_cov} s{s}", _adjacency(dict(full_cov=full_cov)), dict(full_cov=full_cov), s


def drive(monkeypatch, m, s, how, operands):
    """What m._fused returns at subsample s, the call made as RECORDINGS and OPERANDS name it, with the scale and the
    subtrahend of m's class; and, where it returns a tag and the class has a forward, what m(y, x) returns."""
    from crf import guided

    adjacency = type(m).__name__ in ("BatchedGuidedAdjacency", "GuidedAdjacency")
    y, x = torch.zeros(1, 3, 6, 8), torch.zeros(1, CX, 6, 8)
    y.requires_grad_(how == "y")
    m.omega.requires_grad_(how != "frozen")
    if operands == "y3d":
        y = y[0]
    if operands == "x3d":
        x = x[0]
    if operands == "not_hip":
        monkeypatch.setattr(guided, "_hip_ok", lambda t: False)
    if operands == "omega_not_hip":
        monkeypatch.setattr(guided, "_hip_ok", lambda t: t is not m.omega)
    with torch.set_grad_enabled(how != "no_grad"):
        if adjacency:
            tag = m._fused(y, x, subsample=s, scale=ADJACENCY_SCALE, subtract=y)
        else:
            tag = m._fused(y, x, subsample=s)
        called = None
        if tag is not None and type(m).__name__ != "GuidedAdjacency" and getattr(m, "subsample_ratio", 1) == s:
            called = m(y, x)
    monkeypatch.setattr(guided, "_hip_ok", lambda t: True)
    return tag, called


def dispatch_tags(monkeypatch):
    """key -> [the tag of _fused or None, the tag of the module's own call or None], over every case, way of recording
    and kind of operands."""
    install_stubs(monkeypatch)
    out = {}
    for key, m, _, s in dispatch_cases():
        for how in RECORDINGS:
            for operands in OPERANDS:
                out[f"{key} {how} {operands}"] = list(drive(monkeypatch, m, s, how, operands))
    return out


def test_fused_dispatches_what_the_table_names(monkeypatch):
    from crf.guided import _guided_route

    install_stubs(monkeypatch)
    n = tagged = 0
    for key, m, kw, s in dispatch_cases():
        adjacency = type(m).__name__ in ("BatchedGuidedAdjacency", "GuidedAdjacency")
        for how, recording in RECORDINGS.items():
            for operands in OPERANDS:
                route = _guided_route(gaussian=kw.get("gaussian", False), mode=kw.get("mode", "nearest"),
                                      fused_bilinear=kw.get("fused_bilinear", False), full_cov=kw["full_cov"], subsample=s,
                                      operands_ok=operands == "ok", recording=recording, fused_grad=kw.get("fused_grad", False),
                                      full_cov_grad=kw.get("full_cov_grad", False), bilinear_grad=kw.get("bilinear_grad", False),
                                      bilinear_full_grad=kw.get("bilinear_full_grad", False))
                want = None
                if route != "torch":
                    bilinear_kernels, full_cov, recorded = route
                    name = KERNELS[bilinear_kernels, full_cov][recorded]
                    want = (name, R, s, ADJACENCY_SCALE if adjacency else 1.0, adjacency, None if recorded else full_cov)
                tag, called = drive(monkeypatch, m, s, how, operands)
                assert tag == want, (key, how, operands, route)
                assert called is None or called == want, (key, how, operands)
                n, tagged = n + 1, tagged + (tag is not None)
    assert n > 2000 and tagged > 200, (n, tagged)


def test_unsupported_is_the_torch_form_and_any_other_error_is_raised(monkeypatch):
    import phl

    install_stubs(monkeypatch)
    cases = [(m, s, how) for _, m, _, s in dispatch_cases() for how in RECORDINGS if drive(monkeypatch, m, s, how, "ok")[0] is not None]
    assert len(cases) > 100
    install_stubs(monkeypatch, status=phl.ERR_UNSUPPORTED)
    assert phl.ERR_UNSUPPORTED == 7
    for m, s, how in cases:
        assert drive(monkeypatch, m, s, how, "ok") == (None, None)
    install_stubs(monkeypatch, status=3)
    for m, s, how in cases:
        with pytest.raises(phl.PhlError):
            drive(monkeypatch, m, s, how, "ok")
