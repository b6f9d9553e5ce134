"""Without a GPU: the long-split cases of tests/test_gpu_conv3d_wgrad.py and tests/test_gpu_deconv3d_k4_bwd.py really have
more bricks than splits.  From the size entries alone (the split count a launch will use is what they report) every LONG
case must have a split of at least two bricks, a brick count that is no multiple of the split count and a split that holds
bricks of two batch items; the cases of before must still be what their files say they are, one brick per split, so that
the two kinds of case stay apart.  The claim of coverage is then checked where no kernel runs, too."""
import pytest

from diffuvolume_amd import _build


@pytest.fixture(scope="module")
def lib():
    _build.build()
    from diffuvolume_amd import _lib
    return _lib.load()


def test_conv3d_long_cases_walk_several_bricks(lib):
    import test_gpu_conv3d_wgrad as T
    assert {(k, s) for _, _, k, s, _, _ in T.LONG} == set(T.BRICK)               # k3 s1, k3 s2 and k1
    for cin, cout, k, s, b, dims in T.LONG:
        nbricks, splits, per_item = T.split_plan(b, cin, dims, cout, k, s)
        assert lib.dv_conv3d_wgrad_workspace_floats(b, cin, *dims, cout, k, s) == splits * cout * cin * k ** 3
        T.assert_long_splits(nbricks, splits, per_item)
        assert b >= 2 and nbricks == b * per_item


def test_conv3d_cases_of_before_are_one_brick_per_split(lib):
    import test_gpu_conv3d_wgrad as T
    for cin, cout, k, s, b, dims in T.CONV:
        nbricks, splits, _ = T.split_plan(b, cin, dims, cout, k, s)
        assert splits == nbricks, (cin, cout, k, s, b, dims)


def test_deconv3d_k4_long_cases_walk_several_bricks(lib):
    import test_gpu_deconv3d_k4_bwd as T
    assert {T.k_waves(ci, co) for ci, co, _, _ in T.LONG} == {1, 2, 4}          # every wave layout of the kernel
    for ci, co, b, dims in T.LONG:
        nbricks, splits, per_item = T.split_plan(ci, co, b, dims)
        assert lib.dv_deconv3d_k4s2_wgrad_workspace_floats(b, ci, *dims, co) == splits * ci * co * 64
        T.assert_long_splits(nbricks, splits, per_item)
        assert b >= 2 and nbricks == b * per_item


def test_deconv3d_k4_cases_of_before_are_one_brick_per_split(lib):
    import test_gpu_deconv3d_k4_bwd as T
    for ci, co, b, dims in T.SHAPES:
        nbricks, splits, _ = T.split_plan(ci, co, b, dims)
        assert splits == nbricks, (ci, co, b, dims)


def test_the_conditions_refuse_cases_that_do_not_meet_them():
    from test_gpu_conv3d_wgrad import assert_long_splits
    assert assert_long_splits(81, 28, 27) == [(26, 28)]
    for nbricks, splits, per_item in ((24, 24, 8),       # one brick per split
                                      (64, 32, 16),      # two bricks per split, but evenly: no ragged range
                                      (36, 32, 12),      # ragged, but no split crosses a batch boundary
                                      (9, 4, 9)):        # one batch item
        with pytest.raises(AssertionError):
            assert_long_splits(nbricks, splits, per_item)
