"""Host half of the device-resident user store (`iisan_amd/userstore.py`): CSR construction, validation, the long-history bookkeeping
and the two index rules (epoch permutation, contiguous eval shard) against `iisan_amd.dp` — plain numpy / torch, no GPU."""
import numpy as np
import pytest
import torch

from iisan_amd import _lib, dp, evaluate, userstore


SEQS = [[3, 1, 4], [1], [5, 9, 2, 6, 5], [], [7, 7]]
HISTS = [[3, 1], [], [5, 9, 2, 6], [8], [7]]


def _check_csr(h, seqs, hists):
    assert h.n_users == len(seqs)
    assert h.seq_off.dtype == np.int64 and h.seq_items.dtype == np.int32
    assert h.seq_off.tolist() == [0] + np.cumsum([len(s) for s in seqs]).tolist()
    assert h.seq_items.tolist() == [i for s in seqs for i in s]
    for u, s in enumerate(seqs):
        assert h.sequence(u).tolist() == list(s)
    assert h.min_len == min(len(s) for s in seqs)
    if hists is None:
        assert h.hist_off is None and h.hist_items is None and h.max_hist == 0 and h.long_users.size == 0
        return
    assert h.hist_off.dtype == np.int64 and h.hist_items.dtype == np.int32
    assert h.hist_off.tolist() == [0] + np.cumsum([len(s) for s in hists]).tolist()
    for u, s in enumerate(hists):
        assert h.history(u).tolist() == list(s)
    assert h.max_hist == max(len(s) for s in hists)


def test_csr_from_lists_and_from_dicts():
    _check_csr(userstore.pack_users(SEQS), SEQS, None)
    _check_csr(userstore.pack_users(SEQS, HISTS, item_num=9), SEQS, HISTS)
    # the reference holds `users_train` / `eval_seq` / `user_history` as dicts keyed by user number, in any insertion order
    order = [4, 0, 2, 1, 3]
    as_dict = userstore.pack_users({u: SEQS[u] for u in order}, {u: np.array(HISTS[u], dtype=np.int64) for u in order})
    _check_csr(as_dict, SEQS, HISTS)
    _check_csr(userstore.pack_users(tuple(tuple(s) for s in SEQS)), SEQS, None)
    tensors = {u: torch.tensor(h, dtype=torch.int64) for u, h in enumerate(HISTS)}       # `user_history` holds LongTensors
    _check_csr(userstore.pack_users(SEQS, tensors), SEQS, HISTS)
    empty = userstore.pack_users([])
    assert empty.n_users == 0 and empty.seq_off.tolist() == [0] and empty.min_len == 0
    assert userstore.pack_users(SEQS).target(2) == 5 and userstore.pack_users(SEQS).target(0) == 4


def test_validation_errors():
    with pytest.raises(ValueError, match="negative item id in seqs"):
        userstore.pack_users([[1, 2], [3, -1]])
    with pytest.raises(ValueError, match="negative item id in histories"):
        userstore.pack_users([[1, 2], [3]], [[1], [-4]])
    with pytest.raises(ValueError, match="item id 10 in seqs above item_num = 9"):
        userstore.pack_users([[1, 10]], item_num=9)
    with pytest.raises(ValueError, match="above item_num"):
        userstore.pack_users([[1, 2]], [[11]], item_num=9)
    userstore.pack_users([[1, 10]])                                   # no item_num: no upper bound
    userstore.pack_users([[1, 9]], item_num=9)
    with pytest.raises(ValueError, match="histories for"):
        userstore.pack_users([[1], [2]], [[1]])
    with pytest.raises(ValueError, match="keyed 0..1"):
        userstore.pack_users({0: [1], 2: [2]})
    with pytest.raises(ValueError, match="does not fit 32 bits"):
        userstore.pack_users([[1 << 31]])
    # like ItemStore: the store lives on a GPU
    with pytest.raises(ValueError, match="no CPU path"):
        userstore.UserStore(SEQS, HISTS, device="cpu")


def test_empty_sequence_is_refused_by_the_eval_windows_with_the_message_of_pack_users():
    """A store may hold an empty sequence (TRAIN / INPUT windows serve it: an all-padding row); EVAL windows need a target.  The refusal is
    host-side, before anything else — the message is `_pack_users`' own."""
    with pytest.raises(ValueError) as ref:
        evaluate._pack_users([[1, 2], []], [[], []], 5, 1)
    store = object.__new__(userstore.UserStore)              # the host half only: no device in this test
    store.host = userstore.pack_users([[1, 2], []])
    with pytest.raises(ValueError) as got:
        store.windows(userstore.EVAL, 5, torch.zeros(1, dtype=torch.int64))
    assert str(got.value) == str(ref.value)


def test_long_history_bookkeeping():
    H = evaluate.HIST_MAX
    hists = [list(range(1, H + 1)), list(range(1, H + 2)), [], list(range(1, 601)), [5]]
    seqs = [[9, 1], [9, 2], [9, 3], [9, 4], [9, 5]]
    h = userstore.pack_users(seqs, hists)
    assert h.long_users.dtype == np.int64 and h.long_users.tolist() == [1, 3]          # exactly HIST_MAX entries is not long
    assert h.max_hist == 600
    for u in h.long_users:
        assert h.history(int(u)).tolist() == hists[u]                                  # the FULL list, not the first HIST_MAX
        assert h.target(int(u)) == seqs[u][-1]
    assert userstore.pack_users(seqs, [[1]] * 5).long_users.size == 0


@pytest.mark.parametrize("n,world,epoch", [(10, 1, 0), (10, 3, 2), (7, 4, 1)])
def test_epoch_index_equals_shard_indices(n, world, epoch):
    for seed in (0, 12):
        for shuffle in (True, False):
            for rank in range(world):
                got = userstore.epoch_index_host(n, rank, world, epoch, seed, shuffle)
                assert got.dtype == torch.int64 and got.is_contiguous()
                assert got.tolist() == dp.shard_indices(n, rank, world, epoch, seed, shuffle), (rank, seed, shuffle)


@pytest.mark.parametrize("U,world,batch", [(50, 1, 16), (50, 2, 16), (5, 4, 2)])
def test_shard_rule_equals_sequential_shard(U, world, batch):
    for rank in range(world):
        first, count = userstore.shard_range(U, rank, world, batch)
        got = torch.arange(first, first + count).clamp_(max=U - 1).tolist()               # what UserStore.eval_index makes on the device
        want = dp.sequential_shard(U, rank, world, batch) if world > 1 else list(range(U))   # evaluate_ranks' own rule
        assert got == want, rank
    if world > 1:                                                                         # the padded shards tile [0, U) in rank order
        cat = sum((dp.sequential_shard(U, r, world, batch) for r in range(world)), [])
        assert cat[:U] == list(range(U))


class _RaisingEncoder(torch.nn.Module):
    """A model whose user encoder fails: what an eval route leaves behind when a batch raises."""

    def user_encoder(self, x, mask, local_rank):
        raise RuntimeError("user encoder failed")


@pytest.mark.parametrize("training", [True, False])
def test_a_raise_inside_an_eval_loop_leaves_the_models_mode_as_it_was(training):
    item_emb = torch.arange(20, dtype=torch.float32).view(5, 4)
    for route in (lambda m: evaluate.evaluate_ranks(m, item_emb, [[1, 2, 3]], [[1, 2]], 4),
                  lambda m: evaluate.recommend_topk(m, item_emb, [[1, 2]], [[1, 2]], 4, k=2)):
        model = _RaisingEncoder().train(training)
        with pytest.raises(RuntimeError, match="user encoder failed"):
            route(model)
        assert model.training is training


def test_fill_short_lists_appends_the_history_in_ascending_id_order():
    """k = 4 over items 1..5: the slots the kernel left 0 take the user's in-range, distinct history ids, ascending (the reference's stable
    argsort lists the -inf items there); a full list is not touched, a list stays short when the history has too few such ids."""
    ids = torch.tensor([[4, 2, 5, 1],            # no empty slot
                        [3, 5, 0, 0],            # two: history [4, 1, 2] -> 1, 2
                        [2, 0, 0, 0]],           # three: history [0, 9, 5, 3, 5] -> 3, 5 (0 is padding, 9 is above the table, 5 twice)
                       dtype=torch.int32)
    hist = [[3], [4, 1, 2], [0, 9, 5, 3, 5]]
    out = evaluate._fill_short_lists(ids, 4, 5, lambda row: hist[row])
    assert out.dtype == torch.int32
    assert out.tolist() == [[4, 2, 5, 1], [3, 5, 1, 2], [2, 3, 5, 0]]


def test_new_symbols_are_bound():
    for name, n_args in (("iisan_user_windows", 15), ("iisan_user_history", 8), ("iisan_rank_histogram", 5)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args
    assert (_lib.IISAN_WIN_TRAIN, _lib.IISAN_WIN_EVAL, _lib.IISAN_WIN_INPUT) == (0, 1, 2)
    assert (userstore.TRAIN, userstore.EVAL, userstore.INPUT) == (0, 1, 2)
