"""Fixed cases of the GBDT loss tests (K21), shared by the CPU and the GPU files."""
import numpy as np
import torch

LOSSES = ("squared", "logistic", "softmax")
NAN, INF = float("nan"), float("inf")
# +-0, a denormal, the float32-denormal hessians around +-100, both sides of the clamp at 708, huge, not finite
HOSTILE = [s * v for v in (0.0, 1e-320, 0.5, 36.7, 100.0, 708.0, 709.0, 800.0, 1e300) for s in (1.0, -1.0)]
NOT_FINITE = [NAN, INF, -INF]


def margins(loss, n, C=1, seed=0, finite=False):
    """``(pred, y)`` on the CPU: the hostile margins first (as many as fit), then a seeded spread; softmax rows
    with equal entries, with a spread of more than 708 and with labels -1 and C among them."""
    gen = torch.Generator().manual_seed(100 * seed + 7 * n + C)
    hostile = torch.tensor(HOSTILE + ([] if finite else NOT_FINITE), dtype=torch.float64)
    pred = torch.randn(C, n, dtype=torch.float64, generator=gen) * 12
    k = min(n, hostile.numel())
    pred[0, :k] = hostile[:k]
    if loss != "softmax":
        return pred[0].contiguous(), torch.rand(n, dtype=torch.float64, generator=gen).round()
    y = torch.randint(0, C, (n,), generator=gen)
    for r, row in zip(range(k, n), ([3.25] * C, [0.0, -709.5] + [1.0] * (C - 2), [900.0, 0.0] + [-900.0] * (C - 2))):
        pred[:, r] = torch.tensor(row, dtype=torch.float64)
    y[n // 2:n // 2 + 2] = torch.tensor([-1, C])[:len(y[n // 2:n // 2 + 2])]
    return pred, y


def shifts(C, wide=False):
    """``(sg, sh)`` int32 ``[C]``, different per class; ``wide``: the limits +-200 and values past them."""
    base = torch.tensor([200, -200, 230, -1000] if wide else [29, 30, 27, 31], dtype=torch.int32)
    return base.repeat(C)[:C].contiguous(), base.flip(0).repeat(C)[:C].contiguous()


def same_floats(a, b):
    """Equal as bits, any NaN equal to any NaN."""
    return a.shape == b.shape and torch.equal(a.isnan(), b.isnan()) and \
        torch.equal(a.nan_to_num(nan=0.0).view(torch.int32), b.nan_to_num(nan=0.0).view(torch.int32))


def class_data():
    """gbdt_cases.model_data with its target cut into three classes."""
    import gbdt_cases as cases
    Bq, y = cases.model_data()
    return torch.from_numpy(Bq.astype(np.uint8)), torch.from_numpy(np.digitize(y, [0.5, 1.5]))


# what is refused: name -> (the arguments a bad call replaces in good(), on the good call's device)
def good(device="cpu"):
    pred, y = margins("softmax", 9, 3)
    return dict(pred=pred.to(device), y=y.to(device), loss="softmax")


BOTH = {
    "unknown_loss": lambda a: dict(loss="hinge"),
    "pred_float32": lambda a: dict(pred=a["pred"].float()),
    "pred_of_rank_1_for_softmax": lambda a: dict(pred=a["pred"][0].contiguous()),
    "pred_of_rank_2_for_logistic": lambda a: dict(loss="logistic", y=a["y"].double()),
    "y_float64_for_softmax": lambda a: dict(y=a["y"].double()),
    "y_int64_for_squared": lambda a: dict(loss="squared", pred=a["pred"][0].contiguous()),
    "y_of_another_length": lambda a: dict(y=a["y"][:-1].contiguous()),
    "C_65": lambda a: dict(pred=torch.zeros(65, 9, dtype=torch.float64, device=a["pred"].device)),
}
WRAPPER = {
    "cpu_tensor": lambda a: dict(y=a["y"].cpu()),
    "out_of_the_wrong_dtype": lambda a: dict(out=torch.zeros(3, 2, dtype=torch.float64, device="cuda")),
    "pred_not_contiguous": lambda a: dict(pred=a["pred"].t().contiguous().t()),
}
