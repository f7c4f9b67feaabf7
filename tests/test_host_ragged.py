"""vqvae_amd.ragged on the host: the prefix sums, the one greedy planner (also against BOTH plain-loop restatements,
tests/ragged_frontend_ref.plan_chunks and tests/metrics_ref.plan_chunks), the length check and the slicing."""
import numpy as np
import pytest

import metrics_ref
import ragged_frontend_ref
from vqvae_amd import ragged


def test_offsets_in_both_forms():
    off = ragged.offsets([3, 1, 4])
    assert off.dtype == np.int64 and off.tolist() == [0, 3, 4]
    off = ragged.offsets(np.array([3, 1, 4], np.int32), total=True)
    assert off.dtype == np.int64 and off.tolist() == [0, 3, 4, 8]
    for empty in ([], np.zeros(0, np.int32)):
        assert ragged.offsets(empty).dtype == np.int64 and ragged.offsets(empty).shape == (0,)
        assert ragged.offsets(empty, total=True).dtype == np.int64 and ragged.offsets(empty, total=True).tolist() == [0]


def test_offsets_accumulate_in_int64_whatever_the_input():
    sizes = np.full(3, 2 ** 30, np.int32)                            # the int32 sum wraps at the second element
    assert ragged.offsets(sizes, total=True).tolist() == [0, 2 ** 30, 2 ** 31, 3 * 2 ** 30]
    assert ragged.offsets(sizes).tolist() == [0, 2 ** 30, 2 ** 31]
    assert ragged.offsets(np.array([2 ** 31 - 1, 2 ** 31 - 1], np.uint32), total=True).tolist() == [0, 2 ** 31 - 1, 2 ** 32 - 2]


def test_plan_runs_documented_behaviours():
    one = np.array([[10, 10, 10, 10, 10]], np.int64)
    assert ragged.plan_runs(one, 120) == [(0, 3), (3, 5)]             # closed when the NEXT utterance would pass the budget
    assert ragged.plan_runs(one, 119) == [(0, 2), (2, 4), (4, 5)]     # exactly the budget still fits, one byte less does not
    assert ragged.plan_runs(one, 1 << 40) == [(0, 5)] and ragged.plan_runs(one, 1) == [(u, u + 1) for u in range(5)]
    assert ragged.plan_runs(np.zeros((1, 0), np.int64), 100) == []
    two = np.array([[1, 1, 1, 1], [5, 1, 1, 30]], np.int64)           # the largest running sum over the stages decides
    assert ragged.plan_runs(two, 4 * 7) == [(0, 3), (3, 4)]
    assert ragged.plan_runs(two[:1], 4 * 7) == [(0, 4)]


def test_plan_runs_an_oversize_utterance_stands_alone():
    assert ragged.plan_runs(np.array([[2, 1000, 2, 2]], np.int64), 40) == [(0, 1), (1, 2), (2, 4)]
    assert ragged.plan_runs(np.array([[1000, 2]], np.int64), 40) == [(0, 1), (1, 2)]


def test_plan_runs_cap():
    big = np.array([[2 ** 30, 2 ** 30 - 1, 1, 2 ** 30]], np.int64)
    assert ragged.plan_runs(big, 1 << 62) == [(0, 4)]
    assert ragged.plan_runs(big, 1 << 62, cap=2 ** 31) == [(0, 2), (2, 4)]          # a run stays BELOW the cap: 2^31 - 1 fits, 2^31 does not
    assert ragged.plan_runs(big, 1 << 62, cap=2 ** 31 + 1) == [(0, 3), (3, 4)]


@pytest.mark.parametrize('seed', range(4))
def test_plan_runs_is_both_restated_planners(seed):
    """The same loop behind frontend.plan_chunks (a table of stages, a cap of 2^31 elements) and metrics.plan_chunks (one
    width): 200 random lists per seed against each plain-loop restatement, budgets from below the smallest utterance to
    above the whole list."""
    from vqvae_amd import frontend, metrics
    rs = np.random.RandomState(1000 + seed)
    for _ in range(200):
        n = int(rs.randint(1, 12))
        lengths = rs.randint(1, 5000, n).astype(np.int64)
        widths = [1] + [int(w) for w in rs.randint(1, 600, rs.randint(0, 7))]
        table = frontend.stage_lengths(lengths, len(widths) - 1) * np.asarray(widths, np.int64)[:, None]
        budget = int(rs.choice([1, 4 * int(table.max()), 4 * int(table.sum(axis=1).max()) // int(rs.randint(1, 6)) + int(rs.randint(0, 3)),
                                1 << 40]))
        want = ragged_frontend_ref.plan_chunks(lengths.tolist(), widths, budget)
        assert ragged.plan_runs(table, budget, cap=2 ** 31) == want == frontend.plan_chunks(lengths, widths, budget)
        frames, width = rs.randint(0, 400, n).astype(np.int64), int(rs.randint(1, 600))
        budget = int(rs.choice([1, 4 * width * int(frames.max()) + 1, 4 * width * int(frames.sum()) // int(rs.randint(1, 6)) + 1, 1 << 40]))
        want = metrics_ref.plan_chunks(frames.tolist(), width, budget)
        assert ragged.plan_runs((width * frames)[None], budget) == want == metrics.plan_chunks(frames, width, budget)


def test_plan_runs_at_the_element_cap_is_the_restated_front_end_planner():
    lengths, widths = [2 ** 30, 2 ** 30 - 2, 2, 5], [1, 1]           # stage 0 reaches 2^31 with the third utterance
    table = np.array([lengths, [ragged_frontend_ref.stage_lengths(t, 1)[1] for t in lengths]], np.int64)
    want = ragged_frontend_ref.plan_chunks(lengths, widths, 1 << 62)
    assert want == [(0, 2), (2, 4)] and ragged.plan_runs(table, 1 << 62, cap=2 ** 31) == want


def test_check_lengths_messages():
    tl = ragged.check_lengths(np.array([3, 1], np.int64), 'LatentCodes')
    assert tl.tolist() == [3, 1]
    assert ragged.check_lengths([2], 'x').tolist() == [2]
    for bad in ([], [[1, 2]], [1.0, 2.0], [3, 0], 5):
        for who in ('LatentCodes', 'LatentCondition'):
            with pytest.raises(ValueError) as e:
                ragged.check_lengths(bad, who)
            assert str(e.value) == '%s: tl must be (N,) latent lengths >= 1 with N >= 1, got %r' % (who, np.asarray(bad))


def test_both_classes_use_the_check():
    from vqvae_amd.frontend import LatentCodes
    from vqvae_amd.generation import LatentCondition
    with pytest.raises(ValueError, match=r'^LatentCodes: tl must be \(N,\) latent lengths >= 1 with N >= 1, got array\(\[2, 0\]\)$'):
        LatentCodes(np.array([2, 0]), np.zeros(2, np.int32), 4)
    with pytest.raises(ValueError, match=r'^LatentCondition: tl must be \(N,\) latent lengths >= 1 with N >= 1, got array\(\[2, 0\]\)$'):
        LatentCondition(np.array([2, 0]), 4, 2, 64)
    assert LatentCodes([2, 3], np.zeros(5, np.int32), 4).offsets.tolist() == [0, 2, 5]
    assert LatentCondition([2, 3], 4, 2, 64).local_off.tolist() == [0, 8]


def test_split_round_trip():
    rs = np.random.RandomState(3)
    sizes = [3, 1, 5, 2]
    off = ragged.offsets(sizes, total=True)
    flat = rs.standard_normal(11).astype(np.float32)
    parts = ragged.split(flat, off)
    assert [p.shape for p in parts] == [(s,) for s in sizes] and np.array_equal(np.concatenate(parts), flat)
    parts[0][:] = 7                                                  # copies: the flat array is not written through them
    assert flat[0] != 7
    z = rs.standard_normal((4, 11)).astype(np.float32)
    parts = ragged.split(z, off)
    assert [p.shape for p in parts] == [(4, s) for s in sizes] and all(p.flags['C_CONTIGUOUS'] for p in parts)
    assert np.array_equal(np.concatenate(parts, axis=1), z)
    rows = ragged.split(z.T.copy(), off, axis=0)
    assert [p.shape for p in rows] == [(s, 4) for s in sizes] and np.array_equal(np.concatenate(rows, axis=0), z.T)
    assert np.array_equal(ragged.split(z, off[1:3])[0], z[:, 3:4])     # one slice
