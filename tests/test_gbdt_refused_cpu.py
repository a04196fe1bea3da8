"""What the definitions of the fixed-point GBDT (mp4x/parallel/gbdt.py) refuse on the CPU: every bad call
of ``gbdt_cases.REFUSED`` that both forms refuse raises ValueError, and a call that only the device
wrapper refuses (a limit of the kernels) is accepted.  tests/test_gbdt_refused_gpu.py holds the wrappers
to the same table."""
import pytest

torch = pytest.importorskip("torch")

import gbdt_cases as cases  # noqa: E402
from mp4x.parallel import gbdt  # noqa: E402


ROWS = [(op, name) for op, name in cases.REFUSED_ROWS if cases.REFUSED[op][name][1] != cases.DEVICE_ONLY]


@pytest.mark.parametrize("op,name", ROWS)
def test_the_definition_refuses_what_the_table_says(op, name):
    definition, _, args, who = cases.refused_call(op, name)
    if who == cases.BOTH:
        with pytest.raises(ValueError):
            getattr(gbdt, definition)(**args)
    else:
        getattr(gbdt, definition)(**args)


@pytest.mark.parametrize("op", sorted(cases.OPS))
def test_the_good_call_is_accepted(op):
    definition, _, good = cases.OPS[op]
    getattr(gbdt, definition)(**good())
