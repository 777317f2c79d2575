"""The parts of tests/side_stream.py and tests/test_streams_gpu.py that need no GPU: the poison check and the choice of cases."""
import numpy as np
import pytest
import torch

import side_stream as SS


def test_poison_must_match_in_shape_and_type_and_differ_in_bits():
    a, b = torch.arange(6.0).reshape(2, 3), torch.arange(6.0).reshape(2, 3) + 1
    SS.check_poison([a, None], [b, None])
    SS.check_poison([a, a], [a, b])                                   # one differing input is enough
    with pytest.raises(AssertionError, match="equals the real inputs"):
        SS.check_poison([a], [a.clone()])
    with pytest.raises(AssertionError):
        SS.check_poison([a], [b.reshape(3, 2)])
    with pytest.raises(AssertionError):
        SS.check_poison([a], [b.double()])
    with pytest.raises(AssertionError):
        SS.check_poison([a], [b, b])
    SS.check_poison([torch.tensor([0.0])], [torch.tensor([-0.0])])      # bits, not values


def test_the_window_cases_have_full_batches_and_one_has_a_ragged_last_batch():
    from seunet_amd.sliding_window import window_table
    import test_streams_gpu as T
    ragged = 0
    for size, (full, rest) in T.WINDOW_CASES.items():
        n = len(window_table(size, 32, 16))
        assert (n // 2, n % 2) == (full, rest) and n >= 4             # n >= 2 * batch: the graph path records a graph
        ragged += rest
    assert ragged == 1 and (48, 32, 64) in T.WINDOW_CASES


def test_the_poison_of_a_volume_is_another_volume_of_that_shape():
    import test_streams_gpu as T
    v = (np.random.default_rng(0).random((3, 4, 5)) < 0.5).astype(np.uint8)
    for a in (v, np.ones((2, 2, 3), np.uint8) * np.arange(3, dtype=np.uint8)):
        p = T.other(a)
        assert p.shape == a.shape and p.dtype == a.dtype and p.flags.c_contiguous and not np.array_equal(p, a)
    sym = np.zeros((3, 3, 4), np.uint8)
    sym[1, 1, 1:3] = 1                                                  # symmetric under the turn: rolled instead
    assert not np.array_equal(T.other(sym), sym)
