"""Fixed cases of the GBDT level tests (K17), shared by the CPU and the GPU files."""
import torch

import gbdt_cases as cases


def part_case(n, F, k, seed=0, edges=True, thr=None, **kw):
    """bins, rows, seg of ``gbdt_cases.hist_case`` (B = 256) and feature, threshold, first_right int32 [k]:
    random splits; with ``edges`` threshold -1 at node 0 and 255 at node 1 (k >= 3), feature -1 at the last
    node (k >= 3) and F at the one before (k >= 4).  ``thr``: every threshold."""
    bins, _, rows, seg = cases.hist_case(n, F, 256, k, seed=seed, **kw)
    k = seg.numel() - 1
    gen = torch.Generator().manual_seed(77 + seed + n + F + k)
    feature = torch.randint(0, F, (k,), dtype=torch.int32, generator=gen)
    threshold = torch.randint(40, 200, (k,), dtype=torch.int32, generator=gen)
    first_right = torch.randint(0, 2, (k,), dtype=torch.int32, generator=gen)
    if thr is not None:
        threshold[:] = thr
    if edges and k >= 3:
        threshold[0], threshold[1], feature[k - 1] = -1, 255, -1
    if edges and k >= 4:
        feature[k - 2] = F
    return bins, rows, seg, feature, threshold, first_right


TILE, SCAN = 4096, 256          # gbdt_hist_map.hpp: kTile; gbdt_part_map.hpp: kScan, the width of a scan pass
M_TWO_PASSES = (SCAN + 1) * TILE + 17
PARTITION = [dict(n=5000, F=5, k=1, one_node=True), dict(n=5000, F=5, k=3), dict(n=5000, F=16, k=64),
             dict(n=5000, F=5, k=2048), dict(n=5000, F=1, k=3), dict(n=5000, F=37, k=3),
             dict(n=5000, F=1, k=1, thr=-1), dict(n=5000, F=37, k=1, thr=255), dict(n=5000, F=37, k=1, thr=-2 ** 31),
             dict(n=5000, F=5, k=3, bad_rows=True), dict(n=600, F=5, k=3, one_node=True)] + \
            [dict(n=5000, F=5, k=4, seg=s, edges=False) for s in cases.HOSTILE.values()] + \
            [dict(n=M_TWO_PASSES, F=1, k=2, seg=[0, 400000, M_TWO_PASSES])]
