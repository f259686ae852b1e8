"""The user-store kernels on the device (`iisan_amd/csrc/users.hip`): `iisan_user_windows`, `iisan_user_history`, `iisan_rank_histogram`
through the C ABI, every output between guard regions and pre-filled with a poison pattern.

Expected values: EVAL / INPUT windows are `evaluate._pack_users` on the same lists (the host packing the eval routes use today), `x` is
`item_emb[tokens]`; TRAIN windows are the reference's own formula, `[0] * mask_len + seq` and `[0] * mask_len + [1] * (L - 1)`
(`Code_Uncached/data_utils/dataset.py:59-62`), on the last `S + 1` items.  All comparisons are bitwise."""
import functools

import numpy as np
import pytest
import torch

from iisan_amd import _lib, dp, evaluate, ops, userstore

pytestmark = pytest.mark.gpu

EBADSHAPE = -1
GUARD = 64                      # elements in front of and behind every output
ITEMS = 90                      # item ids 1..ITEMS
SS = (1, 5, 10, 32)
LENGTHS = sorted({l for S in SS for l in (1, 2, S, S + 1, S + 2, 3 * S)})
POISON = {torch.int64: -7777, torch.int32: -7777, torch.float32: float("nan")}


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _users(with_empty: bool):
    """One user per length (twice: different items), in a shuffled order; `with_empty` adds two users without any item."""
    rs = np.random.RandomState(7)
    lens = LENGTHS * 2 + ([0, 0] if with_empty else [])
    rs.shuffle(lens)
    seqs = [rs.randint(1, ITEMS + 1, size=l).tolist() for l in lens]          # repeats allowed: lists are longer than the catalogue
    return seqs, userstore.UserStore(seqs, item_num=ITEMS)


@functools.lru_cache(maxsize=None)
def _table(E: int):
    g = torch.Generator().manual_seed(E)
    return torch.randn(ITEMS + 1, E, generator=g).cuda()                      # row 0 is NOT zero: padded positions must copy it


def _index(B: int, U: int, seed: int):
    """B = 1: one user; 7: a permutation's head; 257: any order with duplicates, -1 and n_users (padding rows) — rows cross workgroups."""
    rs = np.random.RandomState(seed)
    if B <= U:
        return rs.permutation(U)[:B].astype(np.int64)
    idx = rs.randint(0, U, size=B).astype(np.int64)
    idx[[0, 5, B - 1]] = [-1, U, U + 1000]
    idx[3], idx[B - 2] = -(1 << 40), idx[1]
    return idx


def _guarded(shape, dtype):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), POISON[dtype], dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(shape)


def _guards_intact(buf, what):
    for g in (buf[:GUARD], buf[-GUARD:]):
        ok = torch.isnan(g).all() if buf.dtype == torch.float32 else (g == POISON[buf.dtype]).all()
        assert bool(ok), f"{what}: guard region written"


def _expected(mode, S, seqs, idx):
    """(ids, log_mask, target | None) on the host."""
    U, B = len(seqs), len(idx)
    W = S + 1 if mode == userstore.TRAIN else S
    ids, lm, tgt = torch.zeros(B, W, dtype=torch.int64), torch.zeros(B, S), torch.zeros(B, dtype=torch.int32)
    rows = [b for b in range(B) if 0 <= idx[b] < U]
    picked = [seqs[idx[b]] for b in rows]
    if mode == userstore.TRAIN:
        for b, seq in zip(rows, picked):
            seq = seq[-(S + 1):] if len(seq) else []
            L = len(seq)
            mask_len = S + 1 - L
            ids[b] = torch.tensor([0] * mask_len + seq)
            if L:                                                             # an empty sequence: the all-padding row
                lm[b] = torch.tensor([0] * mask_len + [1] * (L - 1), dtype=torch.float32)
        return ids, lm, None
    if mode == userstore.INPUT:
        picked = [s + [0] for s in picked]
    tok, m, _, t = evaluate._pack_users(picked, [[] for _ in picked], S, 1)
    if rows:
        ids[rows], lm[rows], tgt[rows] = tok, m, t
    return ids, lm, (tgt if mode == userstore.EVAL else None)


@pytest.mark.parametrize("B", [1, 7, 257])
@pytest.mark.parametrize("S", SS)
@pytest.mark.parametrize("mode", [userstore.TRAIN, userstore.EVAL, userstore.INPUT])
def test_windows_equal_the_host_packing(lib, mode, S, B):
    seqs, st = _users(with_empty=mode != userstore.EVAL)
    idx = _index(B, len(seqs), seed=100 * S + B)
    index = torch.from_numpy(idx).cuda()
    W = S + 1 if mode == userstore.TRAIN else S
    want_ids, want_lm, want_tgt = _expected(mode, S, seqs, idx)
    lens = {len(seqs[u]) for u in idx if 0 <= u < len(seqs)}
    if B == 257:
        assert lens >= set(LENGTHS) or len(lens) > 10                         # the sweep of lengths is in the batch
    for E in ((None,) if mode == userstore.TRAIN else (None, 64, 256)):
        bi, ids = _guarded((B, W), torch.int64)
        bm, lm = _guarded((B, S), torch.float32)
        bt, tgt = _guarded((B,), torch.int32)
        bx, x = _guarded((B, S, E or 4), torch.float32)
        emb = _table(E) if E else None
        rc = lib.iisan_user_windows(st.seq_off.data_ptr(), st.seq_items.data_ptr(), st.n_users, index.data_ptr(), B, S, mode,
                                    ids.data_ptr(), lm.data_ptr(), tgt.data_ptr() if mode == userstore.EVAL else None,
                                    emb.data_ptr() if E else None, ITEMS + 1 if E else 0, E or 0, x.data_ptr() if E else None, _stream())
        assert rc == 0, lib.iisan_last_error()
        torch.cuda.synchronize()
        what = f"mode {mode} S {S} B {B} E {E}"
        for b in (bi, bm, bt, bx):
            _guards_intact(b, what)
        assert torch.equal(ids.cpu(), want_ids), what                         # equal => every element was written (the poison is gone)
        assert torch.equal(lm.cpu(), want_lm), what
        if mode == userstore.EVAL:
            assert torch.equal(tgt.cpu(), want_tgt), what
        else:
            assert bool((tgt == POISON[torch.int32]).all()), what             # no target pointer given: untouched
        if E:
            assert torch.equal(x, emb[want_ids.cuda()]), what                 # padded positions: row 0 of the table, bit for bit
        else:
            assert bool(torch.isnan(x).all()), what
    pad = torch.from_numpy((idx < 0) | (idx >= len(seqs)))
    if pad.any():                                                             # out-of-range user numbers: all-zero rows
        assert not want_ids[pad].any() and not want_lm[pad].any() and (want_tgt is None or not want_tgt[pad].any())


def test_windows_guards_and_optional_outputs(lib):
    """An item id beyond the table is not dereferenced (zero row); a target pointer outside EVAL mode is written 0; and the store's own
    methods return what the raw calls do."""
    seqs, st = _users(with_empty=False)
    U, S, E = len(seqs), 10, 64
    index = torch.arange(U, device="cuda")
    want_ids, want_lm, want_tgt = _expected(userstore.EVAL, S, seqs, np.arange(U))
    small = _table(E)[:40].contiguous()                                       # ids 40..90 are beyond this table
    ids, lm, tgt, x = st.windows(userstore.EVAL, S, index, small)
    assert torch.equal(ids.cpu(), want_ids) and torch.equal(lm.cpu(), want_lm) and torch.equal(tgt.cpu(), want_tgt)
    inside = (want_ids < 40).cuda()
    assert bool((~inside).any())
    want_x = torch.where(inside[..., None], small[want_ids.cuda().clamp(max=39)], torch.zeros((), device="cuda"))
    assert torch.equal(x, want_x)
    bt, tgt = _guarded((U,), torch.int32)
    ids2 = torch.empty(U, S, dtype=torch.int64, device="cuda")
    lm2 = torch.empty(U, S, device="cuda")
    rc = lib.iisan_user_windows(st.seq_off.data_ptr(), st.seq_items.data_ptr(), U, index.data_ptr(), U, S, userstore.INPUT, ids2.data_ptr(),
                                lm2.data_ptr(), tgt.data_ptr(), None, 0, 0, None, _stream())
    assert rc == 0 and not tgt.any()
    _guards_intact(bt, "optional target")
    t_ids, t_lm = st.train_batch(index, S)
    w_ids, w_lm, _ = _expected(userstore.TRAIN, S, seqs, np.arange(U))
    assert torch.equal(t_ids.cpu(), w_ids) and torch.equal(t_lm.cpu(), w_lm)
    assert st.nbytes() == 8 * (U + 1) + 4 * sum(len(s) for s in seqs)
    e = st.epoch_index(1, 3, 2, seed=4)
    assert e.is_cuda and e.dtype == torch.int64 and e.tolist() == dp.shard_indices(U, 1, 3, 2, 4)
    assert st.eval_index(1, 2, 16).tolist() == dp.sequential_shard(U, 1, 2, 16)
    for bad in (index.cpu(), index.int(), index.view(1, -1)):
        with pytest.raises(ValueError):
            st.windows(userstore.INPUT, S, bad)
    with pytest.raises(ValueError, match="without histories"):
        st.history(index, 4)


@pytest.mark.parametrize("stride", [1, 8, 256])
def test_history_equals_the_host_packing(lib, stride):
    rs = np.random.RandomState(stride)
    lens = sorted({l for s in (1, 8, 256) for l in (0, 1, s, s + 1, 300)}) * 2
    rs.shuffle(lens)
    hists = [rs.randint(1, ITEMS + 1, size=l).tolist() for l in lens]
    U = len(hists)
    st = userstore.UserStore([[1]] * U, hists, item_num=ITEMS)
    assert st.max_hist == 300 and st.long_users.tolist() == [u for u in range(U) if len(hists[u]) > 256]
    for B in (1, 7, 257):
        idx = _index(B, U, seed=B)
        rows = [b for b in range(B) if 0 <= idx[b] < U]
        want = torch.zeros(B, stride, dtype=torch.int32)
        want[rows] = evaluate._pack_users([[1]] * len(rows), [hists[idx[b]][:stride] for b in rows], 1, stride)[2]
        buf, out = _guarded((B, stride), torch.int32)
        index = torch.from_numpy(idx).cuda()
        rc = lib.iisan_user_history(st.hist_off.data_ptr(), st.hist_items.data_ptr(), U, index.data_ptr(), B, stride, out.data_ptr(), _stream())
        assert rc == 0, lib.iisan_last_error()
        torch.cuda.synchronize()
        _guards_intact(buf, f"history stride {stride} B {B}")
        assert torch.equal(out.cpu(), want), (stride, B)
        assert torch.equal(st.history(index, stride), out)


def _bins(r, K):
    b = torch.where(r < 1, torch.zeros_like(r), torch.where(r > K, torch.full_like(r, K + 1), r)).long()
    return torch.bincount(b, minlength=K + 2)


@pytest.mark.parametrize("K", [1, 10, 64])
@pytest.mark.parametrize("U", [1, 1000])
def test_rank_histogram_equals_bincount(lib, U, K):
    g = torch.Generator().manual_seed(U + K)
    if U == 1:
        cases = [torch.tensor([v], dtype=torch.int32) for v in (-1, 0, 1, K, K + 1, 1 << 30)]
    else:
        r = torch.randint(-1, K + 4, (U,), generator=g, dtype=torch.int32)                 # repeats of every bin
        r[:6] = torch.tensor([-1, 1, K, K + 1, 1, K], dtype=torch.int32)
        cases = [r, torch.randint(1, 20316, (U,), generator=g, dtype=torch.int32)]          # ranks as an eval pass has them
    for r in cases:
        buf, counts = _guarded((K + 2,), torch.int64)
        counts.zero_()
        assert lib.iisan_rank_histogram(r.cuda().data_ptr(), U, K, counts.data_ptr(), _stream()) == 0, lib.iisan_last_error()
        torch.cuda.synchronize()
        _guards_intact(buf, "histogram")
        assert torch.equal(counts.cpu(), _bins(r, K)) and int(counts.sum()) == U
        assert torch.equal(ops.rank_histogram(r.cuda(), K).cpu(), _bins(r, K))
    # counts are accumulated into: two calls == one call on the concatenation
    a, b = cases[0], cases[-1]
    acc = ops.rank_histogram(a.cuda(), K)
    assert ops.rank_histogram(b.cuda(), K, acc) is acc
    assert torch.equal(acc.cpu(), _bins(torch.cat([a, b]), K))
    assert torch.equal(acc, ops.rank_histogram(torch.cat([a, b]).cuda(), K))


def test_bad_arguments_are_refused_before_any_launch(lib):
    seqs, st = _users(with_empty=False)
    U, S, E, B = len(seqs), 10, 64, 5
    index = torch.arange(B, device="cuda")
    emb = _table(E)
    ids = torch.full((B, S + 1), 5, dtype=torch.int64, device="cuda")
    lm = torch.full((B, S), 5.0, device="cuda")
    tgt = torch.full((B,), 5, dtype=torch.int32, device="cuda")
    x = torch.full((B, S, E), 5.0, device="cuda")
    hist = torch.full((B, 8), 5, dtype=torch.int32, device="cuda")
    counts = torch.full((66,), 5, dtype=torch.int64, device="cuda")
    ranks = torch.ones(B, dtype=torch.int32, device="cuda")
    hst = userstore.UserStore([[1]] * U, [[2, 3]] * U)
    so, si, ho, hi = st.seq_off.data_ptr(), st.seq_items.data_ptr(), hst.hist_off.data_ptr(), hst.hist_items.data_ptr()
    ip, dp_, lp, tp, ep, xp = index.data_ptr(), ids.data_ptr(), lm.data_ptr(), tgt.data_ptr(), emb.data_ptr(), x.data_ptr()
    T, EV, IN = userstore.TRAIN, userstore.EVAL, userstore.INPUT
    win = lambda *a: lib.iisan_user_windows(*a, _stream())
    his = lambda *a: lib.iisan_user_history(*a, _stream())
    hgm = lambda *a: lib.iisan_rank_histogram(*a, _stream())
    cases = [
        (win, (so, si, U, ip, 0, S, EV, dp_, lp, tp, ep, ITEMS + 1, E, xp), "B"),
        (win, (so, si, U, ip, -3, S, EV, dp_, lp, tp, ep, ITEMS + 1, E, xp), "B"),
        (win, (so, si, U, ip, B, 0, EV, dp_, lp, tp, ep, ITEMS + 1, E, xp), "S"),
        (win, (so, si, U, ip, B, 64, T, dp_, lp, None, None, 0, 0, None), "S"),
        (win, (so, si, U, ip, B, S, 3, dp_, lp, tp, ep, ITEMS + 1, E, xp), "mode"),
        (win, (None, si, U, ip, B, S, EV, dp_, lp, tp, ep, ITEMS + 1, E, xp), "seq_off"),
        (win, (so, None, U, ip, B, S, EV, dp_, lp, tp, ep, ITEMS + 1, E, xp), "seq_items"),
        (win, (so, si, U, None, B, S, EV, dp_, lp, tp, ep, ITEMS + 1, E, xp), "user_index"),
        (win, (so, si, U, ip, B, S, EV, None, lp, tp, ep, ITEMS + 1, E, xp), "ids"),
        (win, (so, si, U, ip, B, S, IN, dp_, None, tp, ep, ITEMS + 1, E, xp), "log_mask"),
        (win, (so, si, U, ip, B, S, EV, dp_, lp, None, ep, ITEMS + 1, E, xp), "target"),
        (win, (so, si, U, ip, B, S, IN, dp_, lp, tp, None, ITEMS + 1, E, xp), "item_emb"),
        (win, (so, si, U, ip, B, S, T, dp_, lp, tp, ep, ITEMS + 1, E, xp), "TRAIN"),
        (win, (so, si, U, ip, B, S, EV, dp_, lp, tp, ep, ITEMS + 1, 6, xp), "E"),
        (win, (so, si, U, ip, B, S, EV, dp_, lp, tp, ep, ITEMS + 1, 0, xp), "E"),
        (win, (so, si, U, ip, B, S, EV, dp_, lp, tp, ep + 4, ITEMS, E, xp), "16-byte"),
        (win, (so, si, U, ip, B, S, EV, dp_, lp, tp, ep, ITEMS + 1, E, xp + 8), "16-byte"),
        (his, (ho, hi, U, ip, 0, 8, hist.data_ptr()), "B"),
        (his, (ho, hi, U, ip, B, 0, hist.data_ptr()), "hist_stride"),
        (his, (ho, hi, U, ip, B, -1, hist.data_ptr()), "hist_stride"),
        (his, (None, hi, U, ip, B, 8, hist.data_ptr()), "hist_off"),
        (his, (ho, hi, U, ip, B, 8, None), "history"),
        (hgm, (ranks.data_ptr(), B, 0, counts.data_ptr()), "K"),
        (hgm, (ranks.data_ptr(), B, 65, counts.data_ptr()), "K"),
        (hgm, (ranks.data_ptr(), 0, 10, counts.data_ptr()), "U"),
        (hgm, (ranks.data_ptr(), B, 10, None), "counts"),
        (hgm, (None, B, 10, counts.data_ptr()), "ranks"),
    ]
    names = ("user_windows", "user_history", "rank_histogram")
    for n in names:
        _lib.dev_set("count:" + n, 0)
    for fn, args, word in cases:
        assert fn(*args) == EBADSHAPE, (word, args)
        msg = lib.iisan_last_error().decode()
        assert word in msg, (word, msg)                                       # the message names the argument
    torch.cuda.synchronize()
    assert [_lib.dev_get("count:" + n) for n in names] == [0, 0, 0]           # nothing was launched
    for t in (ids, lm, tgt, x, hist, counts):
        assert bool((t == 5).all())                                           # and nothing was written
    # the Python layer reports them as the library's error
    with pytest.raises(_lib.IisanHipError, match="S = 64"):
        st.windows(IN, 64, index)
    with pytest.raises(_lib.IisanHipError, match="hist_stride"):
        hst.history(index, 0)
    with pytest.raises(_lib.IisanHipError, match="K = 65"):
        ops.rank_histogram(ranks, 65)
    # one accepted call of each moves its counter by one
    st.windows(IN, S, index, emb)
    hst.history(index, 8)
    ops.rank_histogram(ranks, 10)
    assert [_lib.dev_get("count:" + n) for n in names] == [1, 1, 1]
    for n in names:
        _lib.dev_set("count:" + n, 0)
