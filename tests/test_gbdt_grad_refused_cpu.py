"""What the GBDT loss ops (K21) refuse, on the CPU: the definitions over gbdt_grad_cases.BOTH, and the trainer's
``loss`` and ``classes``."""
import pytest

torch = pytest.importorskip("torch")

import gbdt_grad_cases as gcases  # noqa: E402
from mp4x.parallel import gbdt  # noqa: E402


@pytest.mark.parametrize("name", sorted(gcases.BOTH))
def test_the_definitions_refuse(name):
    args = gcases.good()
    args.update(gcases.BOTH[name](args))
    C = args["pred"].shape[0] if args["pred"].dim() == 2 else 1
    with pytest.raises(ValueError):
        gbdt.gbdt_grad_absmax_torch(**args)
    with pytest.raises(ValueError):
        gbdt.gbdt_grad_quantize_torch(**args, sg=torch.zeros(C, dtype=torch.int32), sh=torch.zeros(C, dtype=torch.int32))


@pytest.mark.parametrize("change", [dict(loss="hinge"), dict(loss="logistic", classes=2), dict(classes=2),
                                    dict(loss="softmax"), dict(loss="softmax", classes=65),
                                    dict(loss="softmax", classes=True)], ids=str)
def test_the_trainer_refuses(change):
    bins, cls = gcases.class_data()
    with pytest.raises(ValueError):
        gbdt.train_gbdt_quantized(None, bins[:50], cls[:50], 16, trees=1, **change)
    good = gcases.good()
    with pytest.raises(ValueError):
        gbdt.gbdt_grad_quantize_torch(**good, sg=torch.zeros(3, dtype=torch.int64), sh=torch.zeros(3, dtype=torch.int32))
