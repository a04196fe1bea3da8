"""train_gbdt_quantized on GPU tensors against the record of tests/test_gbdt_golden_cpu.py: both cases,
the three level modes, Tree for Tree and value bit for value bit."""
import pytest

torch = pytest.importorskip("torch")

import gbdt_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", sorted(cases.GOLDEN_CASES))
def test_gpu_trees_equal_the_record_in_every_mode(case):
    record = cases.golden_record()[case]
    for mode in cases.GOLDEN_MODES:
        assert cases.golden_trees(case, mode, device="cuda") == record[mode]["trees"], mode
