"""`cut_calls` (watsor_amd/detection/hip_gpu.py), the one rule that cuts a list of frames into consecutive calls: a new call starts when the
key changes, when the cost would pass max_batch, or when a camera that may appear once per call appears again.  The expected cuts below
are written out by hand from that rule."""
from watsor_amd.detection.hip_gpu import cut_calls

K, L = ("tiled", 0.6, 1.0), ("tiled", 0.5, 1.0)


def test_a_key_change_cuts():
    assert cut_calls([(K, 1, None), (K, 1, None), (L, 1, None), (K, 1, None)], 8) == [[0, 1], [2], [3]]


def test_cost_at_exactly_max_batch_fits_and_one_more_does_not():
    assert cut_calls([(K, 3, None), (K, 5, None)], 8) == [[0, 1]]                       # 3 + 5 = max_batch
    assert cut_calls([(K, 3, None), (K, 6, None)], 8) == [[0], [1]]                     # 3 + 6 = max_batch + 1
    assert cut_calls([(K, 3, None), (K, 5, None), (K, 1, None)], 8) == [[0, 1], [2]]    # the ninth unit opens the next call
    assert cut_calls([(K, 1, None)] * 10, 8) == [list(range(8)), [8, 9]]                # a cost of 1 each: max_batch items
    assert cut_calls([(K, 9, None), (K, 1, None)], 8) == [[0], [1]]                     # an item beyond max_batch alone is still a call of its own


def test_a_repeated_once_per_call_camera_cuts():
    assert cut_calls([(K, 2, 0), (K, 2, 1), (K, 2, 0), (K, 2, 1)], 8) == [[0, 1], [2, 3]]
    assert cut_calls([(K, 1, 4), (K, 1, 4), (K, 1, 4)], 8) == [[0], [1], [2]]
    assert cut_calls([(K, 2, 0), (K, 2, None), (K, 2, 0)], 8) == [[0, 1], [2]]          # frames without such a camera share the call


def test_a_repeated_camera_that_is_not_once_per_call_does_not_cut():
    assert cut_calls([(K, 2, None), (K, 2, None), (K, 2, None)], 8) == [[0, 1, 2]]


def test_the_cut_forgets_the_previous_call():
    # camera 0 may appear again after a cut made for another reason, and the cost starts from nothing
    assert cut_calls([(K, 5, 0), (L, 5, 0), (L, 3, 1), (L, 1, 2)], 8) == [[0], [1, 2], [3]]


def test_an_empty_input_is_no_call():
    assert cut_calls([], 8) == []
