"""`iisan_score_rank` and `iisan_score_topk` (csrc/score.hip) at `embedding_dim` 128, 192 and 256: one chain of 16 E / 64 MFMAs per
score, the same chain for a target, a history item, a table tile and a tile of the top-k kernel.

  a. exact inputs - `prec` and `item_emb` drawn from {-2, -1.75, .., 2}: every product is a multiple of 1/16 and every float32 sum of
     E of them is exact in any order, so the float64 definition is THE answer, ties included: ranks and top-k lists (ids and score
     bits) equal for every user;
  b. random inputs - `test_gpu_topk.py::test_topk_kernel_shapes_histories_and_ties` as it stands at 64, at the wide widths;
  c. a target `iisan_score_rank` puts at r <= k is entry r - 1 of the list, one ranked beyond k is not in it;
  d. widths 32 / 96 / 320 are refused by both entries."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from iisan_amd import _lib, ops  # noqa: E402
from test_gpu_topk import _definition  # noqa: E402

WIDTHS = (128, 192, 256)
U_EXACT, N1_EXACT, H_EXACT = 97, 2001, 40


@functools.lru_cache(maxsize=None)
def _exact_problem(E):
    """97 users x 2,001 table rows on the grid of quarters: histories of 40 entries with zeros, duplicates and out-of-range ids, every
    ninth user's target inside its own history, one invalid target; the float64 scores, ranks and stable descending order."""
    g = torch.Generator().manual_seed(E)
    item = torch.randint(-8, 9, (N1_EXACT, E), generator=g).float() / 4
    prec = torch.randint(-8, 9, (U_EXACT, E), generator=g).float() / 4
    hist = torch.randint(0, N1_EXACT, (U_EXACT, H_EXACT), generator=g, dtype=torch.int32)
    hist[:, 0] = hist[:, -1]                     # a duplicate
    hist[:, 3] = 0                               # padding in the middle
    hist[::5, 7] = N1_EXACT + 11                 # out of range: ignored
    hist[1::5, 9] = -4
    tgt = torch.randint(1, N1_EXACT, (U_EXACT,), generator=g, dtype=torch.int32)
    tgt[::9] = hist[::9, 20]                     # the target in its own history (where that entry is an item)
    tgt[5] = 0                                   # an invalid target
    sc = prec.double() @ item.double().t()
    assert torch.equal((prec @ item.t()).double(), sc), "the inputs are not exact in float32"
    raw = sc.clone()
    ok = (hist >= 0) & (hist < N1_EXACT)
    for u in range(U_EXACT):
        sc[u, hist[u][ok[u]].long()] = -math.inf
    sc[:, 0] = -math.inf
    srt, order = torch.sort(sc[:, 1:], dim=1, descending=True, stable=True)
    for i, u in enumerate(range(10, 27)):        # targets inside the lists: user 10's at position 1, .., user 26's at 17 (beyond k = 16)
        if u % 9:
            tgt[u] = order[u, i] + 1
    ranks = torch.empty(U_EXACT, dtype=torch.int64)
    ids = torch.arange(N1_EXACT)
    for u in range(U_EXACT):
        t = int(tgt[u])
        if t <= 0 or t >= N1_EXACT:
            ranks[u] = -1
            continue
        st = sc[u, t]
        ahead = (sc[u] > st) | ((sc[u] == st) & (ids < t))
        ahead[0] = False
        ahead[t] = False
        ranks[u] = 1 + int(ahead.sum())
    ties = sum(int((srt[u, :11].diff() == 0).any()) for u in range(U_EXACT))
    assert ties >= 10, ties                      # exact ties inside the first eleven scores: the tie rule decides lists
    in_hist = [u for u in range(U_EXACT) if int(tgt[u]) > 0 and bool((hist[u] == tgt[u]).any())]
    assert len(in_hist) >= 5
    return dict(item=item, prec=prec, hist=hist, tgt=tgt, ranks=ranks, order=order + 1, srt=srt, raw=raw, in_hist=in_hist)


@pytest.mark.parametrize("E", WIDTHS)
def test_ranks_and_lists_equal_the_fp64_definition_on_exact_inputs(lib, E):
    """(a) and (c): rank = 1 + #{c: s_c > s_t or (s_c == s_t and c < t)} with history and column 0 at -inf, -1 for the invalid target;
    top-k (k = 1, 10, 16) = the stable descending argsort of the float64 row, ids and score bits, every user.  Negative control: the
    definition evaluated on the first 64 features alone gives other ranks and other lists."""
    p = _exact_problem(E)
    prec, item, hist, tgt = p["prec"].cuda(), p["item"].cuda(), p["hist"].cuda(), p["tgt"].cuda()
    ranks = ops.score_rank(prec, item, hist, tgt).cpu().long()
    assert torch.equal(ranks, p["ranks"]), torch.nonzero(ranks != p["ranks"]).flatten()[:8].tolist()
    assert int(ranks[5]) == -1
    lists = {}
    for k in (1, 10, 16):
        ids, sc = ops.score_topk(prec, item, hist, k)
        ids, sc = ids.cpu().long(), sc.cpu()
        assert torch.equal(ids, p["order"][:, :k]), (k, torch.nonzero((ids != p["order"][:, :k]).any(1)).flatten()[:8].tolist())
        assert torch.equal(sc.double(), p["srt"][:, :k]), k
        lists[k] = ids
    # (c) the two kernels agree on where the target sits
    n_in = 0
    for u in range(U_EXACT):
        r, t = int(ranks[u]), int(tgt[u])
        if 1 <= r <= 16:
            assert int(lists[16][u, r - 1]) == t, (u, r, t)
            n_in += 1
        else:
            assert t not in lists[16][u].tolist()
    assert n_in >= 14 and int(ranks[26]) == 17
    for u in p["in_hist"]:                        # a target inside its own history scores -inf: behind every other item
        assert int(ranks[u]) > N1_EXACT - 1 - H_EXACT
    # negative control: one feature block
    s64 = p["prec"][:, :64].double() @ p["item"][:, :64].double().t()
    assert not torch.equal(torch.sort(s64[:, 1:], dim=1, descending=True, stable=True)[1][:, :10] + 1, p["order"][:, :10])


CASES_B = [(1, 17, 0, 16), (5, 12, 4, 10), (33, 500, 3, 10), (97, 2001, 40, 16), (64, 4096, 130, 5)]


@pytest.mark.parametrize("case", CASES_B)
@pytest.mark.parametrize("E", WIDTHS)
def test_topk_kernel_shapes_histories_and_ties_at_wide_widths(lib, E, case):
    """(b): `test_gpu_topk.py::test_topk_kernel_shapes_histories_and_ties` at E, generator seed U * 7 + n1 + H + E, near-tie threshold
    1e-5 * E / 64 (the summation-order noise of E products).  On (97, 2001, 40, 16) also (c) against `iisan_score_rank`."""
    U, n1, H, k = case
    g = torch.Generator().manual_seed(U * 7 + n1 + H + E)
    item = torch.randn(n1, E, generator=g)
    prec = torch.randn(U, E, generator=g)
    planted = n1 > 40
    if planted:
        item[7] = item[3]
        item[30] = item[11]
        prec[0] = 3 * item[3]
        if U > 1:
            prec[1] = 3 * item[11]
    hist = torch.zeros(U, 0, dtype=torch.int32)
    if H:
        hist = torch.randint(0, n1, (U, H), generator=g, dtype=torch.int32)
        hist[:, 0] = hist[:, -1]
        if planted and U > 2:
            prec[2] = 3 * item[3]
            hist[2, H // 2] = 3
    hist_d = hist.cuda() if H else torch.zeros(U, 0, dtype=torch.int32).cuda()
    ids, sc = ops.score_topk(prec.cuda(), item.cuda(), hist_d, k)
    ids, sc = ids.cpu().long(), sc.cpu()
    ref_ids, ref_val = _definition(prec.cuda(), item.cuda(), hist.cuda(), k)
    ref_ids, ref_val = ref_ids.cpu(), ref_val.cpu()
    kk = ref_ids.shape[1]
    if planted:
        assert ids[0, :2].tolist() == [3, 7]
        if U > 1:
            assert ids[1, :2].tolist() == [11, 30]
        if H and U > 2:
            assert ids[2, 0].item() == 7 and 3 not in ids[2].tolist()
    n_close = 0
    for u in range(U):
        want = ref_ids[u, :k].tolist() + [0] * (k - min(k, kk))
        gaps = (ref_val[u, :-1] - ref_val[u, 1:]).abs() if kk > 1 else torch.ones(1)
        finite = torch.isfinite(ref_val[u, :-1]) & torch.isfinite(ref_val[u, 1:]) if kk > 1 else torch.zeros(1, dtype=torch.bool)
        close = bool(((gaps < 1e-5 * E / 64) & (gaps > 0) & finite).any())
        got = ids[u].tolist()
        if close:
            n_close += 1
            assert sorted(got[:k - 1]) == sorted(want[:k - 1]) or sorted(got) == sorted(want), (u, got, want)
            continue
        assert got == want, (u, got, want)
        for r in range(k):
            if want[r] == 0:
                assert sc[u, r].item() == -math.inf
            else:
                assert abs(sc[u, r].item() - ref_val[u, r].item()) < 1e-4 * (1 + abs(ref_val[u, r].item()))
    assert n_close <= max(2, U // 20)
    if case == (97, 2001, 40, 16):
        tgt = torch.randint(1, n1, (U,), generator=g, dtype=torch.int32)
        tgt[:3] = torch.tensor([7, 30, 7], dtype=torch.int32)         # the planted ties: ranks 2, 2 and 1
        ranks = ops.score_rank(prec.cuda(), item.cuda(), hist_d, tgt.cuda()).cpu().long()
        assert ranks[:3].tolist() == [2, 2, 1]
        n_in = 0
        for u in range(U):
            r, t = int(ranks[u]), int(tgt[u])
            if 1 <= r <= k:
                assert int(ids[u, r - 1]) == t, (u, r, t)
                n_in += 1
            else:
                assert t not in ids[u].tolist(), (u, r, t)
        assert n_in >= 3


@pytest.mark.parametrize("E", [32, 96, 320])
def test_rank_and_topk_refuse_widths_outside_the_set(lib, E):
    p, it = torch.randn(4, E).cuda(), torch.randn(50, E).cuda()
    h = torch.zeros(4, 2, dtype=torch.int32).cuda()
    t = torch.ones(4, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    before = _lib.dev_state(True)
    with pytest.raises(_lib.IisanHipError, match=rf"score_topk: embedding_dim must be 64, 128, 192 or 256 \(got {E}\)"):
        ops.score_topk(p, it, h, 5)
    with pytest.raises(_lib.IisanHipError, match=rf"score_rank: embedding_dim must be 64, 128, 192 or 256 \(got {E}\)"):
        ops.score_rank(p, it, h, t)
    assert _lib.dev_state(True) == before
