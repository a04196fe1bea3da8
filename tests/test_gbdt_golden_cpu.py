"""train_gbdt_quantized against a record (tests/golden/gbdt_trees.json): the trees of two cases in the
three level modes, and the collective schedule, the ``(operator, element count)`` of every allreduce the
trainer issues.  The other GBDT tests compare the modes with each other and the GPU with the CPU; an
edit that shifts all of them the same way passes those and fails here.  The record was written once by
running this module as a script; the tests never regenerate it."""
import json
import os

import pytest

torch = pytest.importorskip("torch")

import gbdt_cases as cases  # noqa: E402

RUNS = [(c, m) for c in cases.GOLDEN_CASES for m in cases.GOLDEN_MODES]


class RecordingComm:
    """Two ranks as far as the trainer can tell; an allreduce is recorded and leaves the array as it is
    (an identity sum), so the trees are the one-rank trees."""

    def __init__(self):
        self.schedule = []

    def getSlaveNum(self):
        return 2

    def allreduceArray(self, arr, operand, operator, lo, hi):
        self.schedule.append([repr(operator), hi - lo])
        return arr


def _recorded(case, mode):
    comm = RecordingComm()
    return dict(trees=cases.golden_trees(case, mode, comm), schedule=comm.schedule)


@pytest.fixture(scope="module")
def record():
    return cases.golden_record()


def _levels(tree):
    """The nodes of every level of a recorded tree."""
    levels, level = [], [0]
    while level:
        levels.append(level)
        level = [c for nd in level if tree["left"][nd] >= 0 for c in (tree["left"][nd], tree["right"][nd])]
    return levels


def test_the_record_has_levels_where_some_nodes_split_and_others_are_final(record):
    """Where the partition's segment bookkeeping can go wrong: the next table is a subset of ``seg2``."""
    for mode in cases.GOLDEN_MODES:
        for tree in record["b"][mode]["trees"]:
            mixed = [lv for lv in _levels(tree) if len({tree["left"][nd] >= 0 for nd in lv}) == 2]
            assert mixed and 25 <= len(tree["value"]) <= 33
        assert record["b"][mode]["trees"] == record["b"]["sort"]["trees"]
        assert record["a"][mode]["trees"] == record["a"]["sort"]["trees"]


@pytest.mark.parametrize("case,mode", RUNS)
def test_one_rank_grows_the_recorded_trees(record, case, mode):
    assert cases.golden_trees(case, mode) == record[case][mode]["trees"]


@pytest.mark.parametrize("case,mode", RUNS)
def test_the_collective_schedule_is_the_recorded_one(record, case, mode):
    """The number, order, operator and length of the allreduces: what keeps ranks in step and the wire
    cost where it is."""
    got = _recorded(case, mode)
    assert got["schedule"] == record[case][mode]["schedule"]
    assert got["trees"] == record[case][mode]["trees"]


def _case_b(comm):
    return {m: cases.golden_trees("b", m, comm, share=(comm.getRank(), comm.getSlaveNum())) for m in cases.GOLDEN_MODES}


def test_two_ranks_grow_the_recorded_trees(record):
    from harness import run_ranks
    res, _, _ = run_ranks(2, _case_b, timeout=120)
    assert sorted(res) == [0, 1]
    for trees in res.values():
        assert trees == {m: record["b"][m]["trees"] for m in cases.GOLDEN_MODES}


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.makedirs(os.path.dirname(cases.GOLDEN_PATH), exist_ok=True)

    def run(c, m):                                            # one line a tree, one for the schedule
        got = _recorded(c, m)
        return '{"trees": [\n' + ",\n".join(json.dumps(t) for t in got["trees"]) + '],\n"schedule": ' + \
            json.dumps(got["schedule"]) + "}"
    text = "{" + ",\n".join(f'"{c}": {{' + ",\n".join(f'"{m}": ' + run(c, m) for m in cases.GOLDEN_MODES) + "}"
                            for c in cases.GOLDEN_CASES) + "}\n"
    json.loads(text)
    with open(cases.GOLDEN_PATH, "w") as f:
        f.write(text)
