"""size_runs, the grouping every device LiDAR export walks its frames with: runs of consecutive records of one size,
at most group_size long, which concatenate back to the input."""
import pytest

from fsnet_amd.monodepth.evaluation.kitti_unsupervised_eval import size_runs

A, B = (375, 1242), (370, 1224)


def _records(sizes):
    return [("scan_%d" % k,) + s for k, s in enumerate(sizes)]


@pytest.mark.parametrize("sizes, group_size, lengths", [
    ([], 4, []),                                            # an empty split
    ([A] * 7, 3, [3, 3, 1]),                                # one size, a length that is no multiple of group_size
    ([A] * 4 + [B] * 3 + [A], 3, [3, 1, 3, 1]),             # a size change in mid-run closes the group early
    ([A, A, B], 1, [1, 1, 1]),                              # group_size = 1
    ([A, B, A, B], 8, [1, 1, 1, 1]),                        # only consecutive frames share a group
])
def test_size_runs(sizes, group_size, lengths):
    records = _records(sizes)
    runs = list(size_runs(records, lambda r: r[1:], group_size))
    assert [len(r) for r in runs] == lengths
    assert [r for run in runs for r in run] == records      # nothing lost, nothing reordered
    for run in runs:
        assert isinstance(run, list) and 1 <= len(run) <= group_size and len({r[1:] for r in run}) == 1
    for prev, nxt in zip(runs, runs[1:]):                   # a run ends only where it must
        assert len(prev) == group_size or prev[-1][1:] != nxt[0][1:]


def test_size_runs_takes_unhashable_keys():
    """the nuScenes export's key is the list of its six cameras' sizes"""
    records = [("a", [A, A]), ("b", [A, A]), ("c", [A, B])]
    assert list(size_runs(records, lambda r: r[1], 4)) == [records[:2], records[2:]]
