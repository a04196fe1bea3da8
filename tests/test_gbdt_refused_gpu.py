"""What the GBDT wrappers of mp4x.ops.device_ops refuse on GPU tensors: every bad call of
``gbdt_cases.REFUSED`` raises ValueError.  The refusal comes before any launch, so nothing of the
project's runs on the device here."""
import pytest

torch = pytest.importorskip("torch")

import gbdt_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("op,name", cases.REFUSED_ROWS)
def test_the_wrapper_refuses_every_row_of_the_table(op, name):
    from mp4x.ops import device_ops
    _, wrapper, args, _ = cases.refused_call(op, name, device="cuda")
    with pytest.raises(ValueError):
        getattr(device_ops, wrapper)(**args)
