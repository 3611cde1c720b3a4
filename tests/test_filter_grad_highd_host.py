"""CPU preconditions of tests/test_gpu_filter_grad_highd.py: every input it names is fit to be judged by K (its
e_ref_T is at most cap / K = 5e-5, and the reference's own fp32 formulation is itself inside the caps), the feature
groups are the even split phl_filter_grad documents (include/phl.h), and the binding's limit is the header's."""
import os
import re

import pytest

from _filter_grad_highd import CAP_REF, CAP_SRC, E_REF_T_MAX, K, feature_groups, named_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("tag,make", named_cases(), ids=[t for t, _ in named_cases()])
def test_named_input_is_fit_for_the_rule(tag, make):
    case = make()
    print(f"[measured] {tag}: M/n {case.M / case.n:.2f} e_ref_T {case.e_ref_T:.2e} e_ref_S {case.e_ref_S:.2e}")
    assert case.e_ref_T <= E_REF_T_MAX == CAP_REF / K, (tag, case.e_ref_T)
    assert case.e_ref_T <= CAP_REF and case.e_ref_S <= CAP_SRC, (tag, case.e_ref_T, case.e_ref_S)      # wide32 inside the caps
    assert case.e_ref_S <= CAP_SRC / K, (tag, case.e_ref_S)


def test_feature_groups():
    sizes = {d: [c for _, c in feature_groups(d)] for d in range(1, 17)}
    assert all(sizes[d] == [d] for d in range(1, 8))
    assert sizes[8] == [4, 4] and sizes[9] == [5, 4] and sizes[14] == [7, 7] and sizes[15] == [5, 5, 5] and sizes[16] == [6, 5, 5]
    for d in range(1, 17):
        for cap in range(1, 8):
            gs = feature_groups(d, cap)
            assert [k for k, _ in gs] == [sum(c for _, c in gs[:i]) for i in range(len(gs))]
            assert sum(c for _, c in gs) == d and max(c for _, c in gs) <= cap and len(gs) == -(-d // cap)
            assert max(c for _, c in gs) - min(c for _, c in gs) <= 1
    assert [c for _, c in feature_groups(5, 2)] == [2, 2, 1] and [c for _, c in feature_groups(5, 3)] == [3, 2]


def test_filter_grad_max_d_is_the_headers():
    import phl

    with open(os.path.join(ROOT, "include", "phl.h")) as fh:
        m = re.search(r"^#define\s+PHL_FILTER_GRAD_MAX_D\s+(\d+)\s*$", fh.read(), re.M)
    assert m and int(m.group(1)) == 16 and phl.FILTER_GRAD_MAX_D == 16
