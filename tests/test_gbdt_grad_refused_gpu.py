"""What the wrappers of the GBDT loss kernels (K21) refuse: gbdt_grad_cases.BOTH, which the definitions refuse too,
and gbdt_grad_cases.WRAPPER, the device's own."""
import pytest

torch = pytest.importorskip("torch")

import gbdt_grad_cases as gcases  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(gcases.BOTH) + sorted(gcases.WRAPPER))
def test_the_wrappers_refuse(name):
    from mp4x.ops import device_ops
    args = gcases.good("cuda")
    args.update({**gcases.BOTH, **gcases.WRAPPER}[name](args))
    C = args["pred"].shape[0] if args["pred"].dim() == 2 else 1
    with pytest.raises(ValueError):
        device_ops.gbdt_grad_absmax(**args)
    if name != "out_of_the_wrong_dtype":
        args["out"] = None
    with pytest.raises(ValueError):
        device_ops.gbdt_grad_quantize(**args, sg=torch.zeros(C, dtype=torch.int32, device="cuda"),
                                      sh=torch.zeros(C, dtype=torch.int32, device="cuda"))
