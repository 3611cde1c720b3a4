"""CPU pin of what tests/test_gpu_blur3_every_d.py compares the blur kernels with: the numpy float32 model of the blur
(tests/_blur3_util.py) reproduces the CPU oracle's blur stage bit for bit from the oracle's own neighbour table, and the
inputs of the GPU tests have the properties they are chosen for (triples per d, a long line along the last group's axis,
d + 1 vertices for constant features).  No GPU here."""
import numpy as np
import pytest

from _blur3_util import RANDOM_SCALE, _features, blur_model_f32, expected_groups, last_group_axis, longest_line


@pytest.mark.parametrize("d", [1, 2, 3, 5, 8, 13, 16])
def test_model_is_the_oracles_blur(d):
    from oracle import phl_oracle as po

    n, vd = 1500, 8
    rng = np.random.default_rng(100 + n + d)
    ref = (rng.random((n, d), dtype=np.float32) * np.float32(RANDOM_SCALE[d])).astype(np.float32)
    src = rng.standard_normal((n, vd)).astype(np.float32)
    O = po.Oracle(ref)
    _, splat_o, blur_o = O.filter(src, stages=True)
    nbr = O.neighbors()
    assert (nbr >= 0).any() and (nbr < 0).any()             # both kinds of operand occur
    got = blur_model_f32(nbr, splat_o)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), blur_o.view(np.uint32))


def test_expected_groups():
    # d + 1 = 3q + r axes: q triples (r = 0), q triples + one pair (r = 2), q - 1 triples + two pairs (r = 1)
    assert [expected_groups(d) for d in range(1, 17)] == [0, 1, 0, 1, 2, 1, 2, 3, 2, 3, 4, 3, 4, 5, 4, 5]
    for d in range(1, 17):
        n3 = expected_groups(d)
        pairs, rest = divmod(d + 1 - 3 * n3, 2)
        assert 0 <= n3 and rest == 0 and pairs <= 2 and (n3 > 0 or d + 1 in (2, 4))
    # the tail layouts above d = 6, as (triples, pairs)
    assert [(expected_groups(d), (d + 1 - 3 * expected_groups(d)) // 2) for d in range(8, 17)] == [
        (3, 0), (2, 2), (3, 1), (4, 0), (3, 2), (4, 1), (5, 0), (4, 2), (5, 1)]


@pytest.mark.parametrize("d", [5, 8, 16])
def test_ramp_along_the_last_groups_axis_makes_one_long_line(d):
    from oracle import phl_oracle as po

    c = last_group_axis(d)
    assert c == {5: 5, 8: 8, 16: 14}[d]
    O = po.Oracle(_features("axis_ramp", d, c=c, n=2048))
    nbr = O.neighbors()
    assert longest_line(nbr[c]) > 4 * 32                    # longer than four items of the largest item size
    for g in range(expected_groups(d) - 1):                 # the other groups' lines stay short
        assert longest_line(nbr[3 * g + 2]) <= 2


@pytest.mark.parametrize("d", [1, 2, 5, 6, 16])
def test_constant_features_make_one_simplex(d):
    from oracle import phl_oracle as po

    assert po.Oracle(_features("constant", d)).M == d + 1
