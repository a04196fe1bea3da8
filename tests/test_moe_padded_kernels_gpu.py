"""The padded K9 route (csrc/kernels/moe.hip: the padded scatter, the pad fill, the pad counts and the
combine that carries the row count), one process, against the definition of tests/moe_padded_ref.py:
``slots``, ``kept`` and ``dropped`` exactly, the whole ``[E*S, ...]`` buffer bit for bit (pads are +0
bits), its ``row_scale`` form and the combine through the padded slots.  The buffer is pre-filled with
NaN and carries sentinel guard rows past ``E*S`` that must survive; every launch runs twice and must
give the same bits."""
import pytest

torch = pytest.importorskip("torch")

import moe_padded_ref as pad  # noqa: E402
import moe_ref  # noqa: E402
from moe_ref import bits, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD, SENTINEL = 3, 1024.0             # no token value (|x| <= 8) times a gate weight (< 1) reaches it


def _run(x, ids, w, E, S, scaled, group=None, group_pad=None):
    from mp4x.ops import device_ops as ops
    T = x.shape[0]
    K = ids.shape[1]
    xd, idd, wd = x.to(DEV), ids.to(DEV), w.to(DEV)
    rc = ops.moe_route_count(idd.reshape(-1), E)
    buf = torch.full((E * S + GUARD,) + tuple(x.shape[1:]), float("nan"), dtype=x.dtype, device=DEV)
    buf[E * S:] = SENTINEL
    slots = ops.moe_route_scatter_pad(rc, xd, K, buf[:E * S], S, row_scale=wd.reshape(-1) if scaled else None)
    kept, dropped = ops.moe_pad_counts(rc, S, group=group, group_pad=group_pad)
    comb = ops.moe_combine_rows(buf[:E * S], slots, None if scaled else wd, T, K)
    torch.cuda.synchronize()
    return slots.cpu(), buf[:E * S].cpu(), buf[E * S:].cpu(), comb.cpu(), kept.cpu(), dropped.cpu()


def _check(x, ids, w, E, S, what):
    T, K = x.shape[0], ids.shape[1]
    _, slots, kept, dropped = pad.cut_ids(ids, E, S)
    for scaled in (False, True):
        send = pad.send_buffer(x, slots, K, E, S, w if scaled else None)
        comb = moe_ref.ref_combine(send, slots, None if scaled else w, T, K)
        got = _run(x, ids, w, E, S, scaled)
        again = _run(x, ids, w, E, S, scaled)
        assert torch.equal(got[0], slots), (what, scaled, "slots")
        assert same_bits(got[1], send), (what, scaled, "rows and pads")
        for e in range(E):                                       # pads: +0 bits, not merely == 0
            assert not bool(bits(got[1][e * S + kept[e]:(e + 1) * S]).any()), (what, scaled, "pad bits", e)
        assert bool((got[2] == SENTINEL).all()) and got[2].shape[0] == GUARD, (what, scaled, "guard rows")
        assert same_bits(got[3], comb), (what, scaled, "combine")
        assert got[4].tolist() == kept and got[5].tolist() == dropped, (what, scaled, "kept / dropped")
        for a, b in zip(got, again):
            assert same_bits(a, b) if a.is_floating_point() else torch.equal(a, b), (what, scaled, "run to run")


def _later_rank(name, S, p):
    """A rank other than 0 that keeps something (case A's rank 1 has no token: that is n == 0)."""
    return 2 if (name == "A" and p == 3) else 1


@pytest.mark.parametrize("p", [2, 3])
@pytest.mark.parametrize("name,S", pad.TABLE)
def test_every_table_row_rank_0_and_a_later_rank(name, S, p):
    for r in (0, _later_rank(name, S, p)):
        want = pad.end_to_end(name, p, S)[r]
        x, ids, w, E = want["x"], want["ids"], want["w"], want["E"]
        _check(x, ids, w, E, S, (name, S, p, r))
        if r == 0:
            other = torch.int32 if ids.dtype == torch.int64 else torch.int64    # both id dtypes
            _check(x, ids.to(other), w, E, S, (name, S, p, other))


def _shares(ids, E):
    """S for T = 150, K = 2, E = 5: 1; a cut inside a wave (between two assignments of expert 2 in one
    wave); expert 1's count inside the first 256 assignments (the tile boundary); the largest demand."""
    flat = ids.reshape(-1)
    where = [(flat == e).nonzero().view(-1).tolist() for e in range(E)]
    demand = [len(ix) for ix in where]
    at_tile = sum(1 for a in where[1] if a < 256)
    assert 0 < at_tile < demand[1]
    mid = next(j for j in range(5, demand[2]) if where[2][j - 1] // 64 == where[2][j] // 64 and where[2][j] % 64)
    return [1, mid, at_tile, max(demand)]


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("vecs", [1, 3, 24, 65])      # 24 and 65: tiles split over 3 and 8 blocks
def test_dtypes_row_widths_and_shares(dtype, vecs):
    dt = getattr(torch, dtype)
    width = vecs * 16 // torch.empty(0, dtype=dt).element_size()
    T, K, E = 150, 2, 5                                                      # n = 300: two tiles
    x = moe_ref.tokens(T, width, dt, 31 + vecs)
    w = moe_ref.gate_weights(T, K, 32 + vecs)
    ids = torch.randint(-1, E, (T, K), generator=torch.Generator().manual_seed(33 + vecs))
    shares = _shares(ids, E)
    assert len(set(shares)) == 4
    for S in shares:
        _check(x, ids, w, E, S, (dtype, vecs, S))


def test_no_assignment_at_all_is_a_buffer_of_pads():
    for width, E, S in ((4, 5, 3), (260, 2, 7)):
        x = torch.empty(0, width)
        _check(x, torch.empty(0, 2, dtype=torch.int64), torch.empty(0, 2), E, S, ("n == 0", width))
    # ... and ids that place nothing
    x = moe_ref.tokens(4, 4, torch.float32, 1)
    _check(x, torch.tensor([[-1, 9], [7, -2], [-1, -1], [5, 5]]), moe_ref.gate_weights(4, 2, 2), 5, 2, "nothing placed")


def test_the_largest_expert_count_with_one_row_each():
    E = 2048
    x = moe_ref.tokens(600, 4, torch.float32, 3)
    w = moe_ref.gate_weights(600, 2, 4)
    ids = ((torch.arange(1200) * 37) % (E // 4)).view(600, 2)                # 512 experts asked for 2 or 3 times
    _check(x, ids, w, E, 1, "E = 2048, S = 1")


def test_the_wire_layout_of_the_kept_counts():
    """kept in groups of el padded to el_pad (every destination's counts on a 16-byte boundary)."""
    want = pad.end_to_end("A", 3, 40)[0]
    E, el = want["E"], want["E"] // 3
    for el_pad in (el, el + 2):
        got = _run(want["x"], want["ids"], want["w"], E, 40, False, group=el, group_pad=el_pad)[4].view(3, el_pad)
        assert torch.equal(got[:, :el].reshape(-1), want["kept"]) and not bool(got[:, el:].any())
    want = pad.end_to_end("B", 3, 3)[1]                                      # el = 1 -> el_pad = 2
    got = _run(want["x"], want["ids"], want["w"], 3, 3, False, group=1, group_pad=2)[4].view(3, 2)
    assert torch.equal(got[:, 0], want["kept"]) and not bool(got[:, 1].any())


def test_the_wrappers_refuse_bad_arguments_before_a_launch():
    from mp4x.ops import device_ops as ops
    ids = torch.zeros(8, dtype=torch.int64, device=DEV)
    rc = ops.moe_route_count(ids, 4)
    x = torch.zeros(4, 4, device=DEV)
    out = torch.empty(8, 4, device=DEV)
    for S in (0, -1, True, 2.0, torch.tensor(2), 1 << 30):
        with pytest.raises(ValueError):
            ops.moe_route_scatter_pad(rc, x, 2, out, S)
        with pytest.raises(ValueError):
            ops.moe_pad_counts(rc, S)
    for bad_out in (torch.empty(7, 4, device=DEV), torch.empty(9, 4, device=DEV), torch.empty(8, 8, device=DEV),
                    torch.empty(8, 4, device=DEV, dtype=torch.float16), torch.empty(8, 4), torch.empty(8, 8, device=DEV)[:, :4]):
        with pytest.raises(ValueError):
            ops.moe_route_scatter_pad(rc, x, 2, bad_out, 2)
    with pytest.raises(ValueError):
        ops.moe_route_scatter_pad(rc, x, 3, out, 2)                           # 4 rows x 3 != 8 ids
    with pytest.raises(ValueError):
        ops.moe_route_scatter_pad(rc, x, 2, out, 2, row_scale=torch.ones(7, device=DEV))
    with pytest.raises(ValueError):
        ops.moe_pad_counts(rc, 2, group=3)
    with pytest.raises(ValueError):
        ops.moe_pad_counts(rc, 2, group=2, group_pad=1)
    with pytest.raises(ValueError):
        ops.moe_pad_counts(rc, 2, kept=torch.empty(3, dtype=torch.int64, device=DEV))
    slots = ops.moe_route_scatter_pad(rc, x, 2, out, 2)
    assert slots.cpu().tolist() == [0, 1, -1, -1, -1, -1, -1, -1]
    for bad in (slots[:7], slots.to(torch.int32)):
        with pytest.raises(ValueError):
            ops.moe_combine_rows(out, bad, None, 4, 2)
    with pytest.raises(ValueError):
        ops.moe_combine_rows(out[:0], slots, None, 4, 2)
    with pytest.raises(ValueError):
        ops.moe_combine_rows(out, slots, torch.ones(8, device=DEV, dtype=torch.float64), 4, 2)
    assert same_bits(ops.moe_combine_rows(out, slots, None, 4, 2).cpu(), torch.zeros(4, 4))
