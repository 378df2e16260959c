"""Host-side policy shared by every graph site: when a signature is captured (ops.seen_enough), which captured graphs stay
(ops.lru_put), and the decode classes' bookkeeping (llm.stop_id_list / token_budget / live_state_rows / empty_state_rows).
Pure host code: no GPU, no library call."""
import collections

import pytest

from vlm_fo1_amd import llm, ops


def test_a_key_is_captured_on_the_sighting_after_the_eager_ones():
    seen = {}
    assert ops.seen_enough(seen, "a", 1) is False          # first sighting: eager
    assert ops.seen_enough(seen, "a", 1) is True           # second: capture
    assert ops.seen_enough(seen, "a", 1) is True           # (an evicted graph's signature is captured again at once)
    assert ops.seen_enough(seen, "b", 1) is False          # keys count separately
    seen = {}
    assert [ops.seen_enough(seen, "a", 2) for _ in range(4)] == [False, False, True, True]
    assert ops.seen_enough({}, "a", 0) is True             # CAPTURE_AFTER = 0: captured on first sight


def test_the_sightings_table_is_bounded_and_drops_its_oldest_key():
    seen = {}
    for k in range(ops.SEEN_MAX):
        assert ops.seen_enough(seen, k, 1) is False
    assert len(seen) == ops.SEEN_MAX == 4096 and next(iter(seen)) == 0
    assert ops.seen_enough(seen, "new", 1) is False
    assert len(seen) == 4096 and 0 not in seen and next(iter(seen)) == 1 and "new" in seen
    for k in range(5000, 5100):
        ops.seen_enough(seen, k, 1)
        assert len(seen) <= 4096
    assert ops.seen_enough(seen, 0, 1) is False            # the dropped key starts over
    assert ops.seen_enough(seen, 4095, 1) is True          # a kept one is still known


def test_lru_keeps_the_last_cap_entries_and_a_hit_survives():
    c = collections.OrderedDict()
    for k in "abc":
        assert ops.lru_put(c, k, k.upper(), 2) == k.upper()
    assert list(c.items()) == [("b", "B"), ("c", "C")]
    c.move_to_end("b")                                     # what a hit does at both engines
    ops.lru_put(c, "d", "D", 2)
    assert list(c) == ["b", "d"]
    ops.lru_put(c, "e", "E", 1)                            # a smaller cap (an instance's GRAPH_CACHE override) evicts down to it
    assert list(c) == ["e"]


def test_state_rows_are_the_rows_both_decode_classes_wrote():
    seqs = [(0, 7, 7), (9, 12, 5, 2, 7)]                   # (off, L, Lp) and a shared-prefix (off, L, Lp, poff, P)
    deltas = [-3, 4]
    # BatchDecoder.start: sequence b at base b * slot, stop set 0
    slot = 1024
    assert llm.live_state_rows([b * slot for b in range(2)], seqs, deltas, 64) == \
        [[0 * slot + 7, 7 - 3, 0, 0, 0, 64, 0, 0], [1 * slot + 12, 12 + 4, 1 * slot, 0, 0, 64, 0, 0]]
    # DecodePool._join_slots: slots 5 and 9 of 2048 rows, stop set 3
    R = 2048
    assert llm.live_state_rows([5 * R, 9 * R], seqs, deltas, 17, 3) == \
        [[5 * R + 7, 4, 5 * R, 0, 0, 17, 3, 0], [9 * R + 12, 16, 9 * R, 0, 0, 17, 3, 0]]
    rows = llm.empty_state_rows([0, R, 7 * R])
    assert rows == [[0, 0, 0, 1, 0, 0, 0, 0], [R, 0, R, 1, 0, 0, 0, 0], [7 * R, 0, 7 * R, 1, 0, 0, 0, 0]]
    for base, row in zip([0, R, 7 * R], rows):
        assert len(row) == 8 and row[3] == 1 and row[0] == row[2] == base


def test_stop_ids_are_normalised_and_refused_with_each_class_s_text():
    assert llm.stop_id_list([7, 3, 7, 5, 3], 16, "X") == [3, 5, 7]
    assert llm.stop_id_list((t for t in (2.0, 1)), 16, "X") == [1, 2]
    assert llm.stop_id_list([], 16, "X") == []
    assert llm.stop_id_list(list(range(16)) * 2, 16, "X") == list(range(16))      # 16 distinct ids are the limit, not the count given
    with pytest.raises(ValueError) as e:
        llm.stop_id_list(range(17), llm.BatchDecoder.MAX_STOP, "BatchDecoder", "; use the host loop")
    assert str(e.value) == "BatchDecoder evaluates at most 16 stop ids on the device (got 17); use the host loop"
    with pytest.raises(ValueError) as e:
        llm.stop_id_list(range(17), llm.DecodePool.MAX_STOP, "DecodePool")
    assert str(e.value) == "DecodePool evaluates at most 16 stop ids on the device (got 17)"


def test_token_budget_is_at_least_one_and_refused_with_each_class_s_text():
    assert llm.token_budget(0, 4096, "X") == 1 and llm.token_budget(-5, 4096, "X") == 1
    assert llm.token_budget(4096, 4096, "X") == 4096 and llm.token_budget(64.0, 4096, "X") == 64
    with pytest.raises(ValueError) as e:
        llm.token_budget(4097, llm.BatchDecoder.IDS_CAP, "BatchDecoder", "; use the host loop")
    assert str(e.value) == "BatchDecoder keeps at most 4096 generated ids per sequence (max_new_tokens=4097); use the host loop"
    with pytest.raises(ValueError) as e:
        llm.token_budget(4097, llm.DecodePool.IDS_CAP, "DecodePool")
    assert str(e.value) == "DecodePool keeps at most 4096 generated ids per sequence (max_new_tokens=4097)"
