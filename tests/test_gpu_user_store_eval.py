"""The eval and training routes over a device-resident user store (`iisan_amd/userstore.py`, `evaluate.*_from_store`) against the
host-packed routes they replace: the same kernels on the same values, so every comparison is bitwise — ranks, top-k ids and scores, the
loss and the flat gradient of a training step.  Only nDCG, summed in another order on the host, carries a tolerance (below)."""
import functools
import os
import socket
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import golden_io as gio  # noqa: E402
import helpers  # noqa: E402
from iisan_amd import evaluate, ops, synth, tapstore, trainer, userstore, weights  # noqa: E402

pytestmark = pytest.mark.gpu


# ---- the reference's eval fixture (50 users x 300 items) ------------------------------------------------------------------------

def test_store_routes_on_the_eval_golden():
    z, seqs, tables, P = gio.eval_inputs()
    n = int(z["item_num"])
    model = helpers.build_model(helpers.make_args(), n, torch.ones(n + 1), cached=True)
    helpers.load_trainables(model, {k: v for k, v in P.items() if k.startswith("user_encoder.") or k.startswith("com_dense.")})
    item_emb = ops.LinearFn.apply(torch.cat(tables, 1).cuda(), model.com_dense.weight, model.com_dense.bias).detach()
    hists = [s[:-1] for s in seqs]
    users = userstore.UserStore(dict(enumerate(seqs)), dict(enumerate(hists)), item_num=n)
    inputs = userstore.UserStore(hists, hists, item_num=n)
    ref = torch.from_numpy(z["ranks"])
    in_hist = torch.tensor([s[-1] in s[:-1] for s in seqs])
    for batch in (16, 1024):
        want = evaluate.evaluate_ranks(model, item_emb, seqs, hists, max_seq_len=10, batch=batch)
        got = evaluate.evaluate_ranks_from_store(model, item_emb, users, 10, batch=batch)
        assert got.dtype == want.dtype and torch.equal(got, want)
        assert torch.equal(got.cpu().long()[~in_hist], ref[~in_hist])                     # ... and so the reference's own ranks
        w_ids, w_sc = evaluate.recommend_topk(model, item_emb, hists, hists, max_seq_len=10, k=10, batch=batch)
        for st, holdout in ((inputs, False), (users, True)):                              # INPUT windows / EVAL windows of `eval_seq`
            ids, sc = evaluate.recommend_topk_from_store(model, item_emb, st, 10, k=10, batch=batch, holdout=holdout)
            assert ids.dtype == w_ids.dtype and torch.equal(ids, w_ids) and torch.equal(sc, w_sc)
        assert torch.equal(w_ids.cpu().long(), torch.from_numpy(z["top10"]).long())
    hit, ndcg = evaluate.eval_metrics_from_store(model, item_emb, users, 10, batch=16)
    w_hit, w_ndcg = evaluate.hit_ndcg(evaluate.evaluate_ranks(model, item_emb, seqs, hists, max_seq_len=10))
    assert hit == w_hit and abs(ndcg - w_ndcg) <= 1e-9 * w_ndcg
    assert model.training                                                                 # the routes restore the caller's mode


# ---- a seeded synthetic set -----------------------------------------------------------------------------------------------------

ITEMS = 700


@functools.lru_cache(maxsize=None)
def _synthetic():
    """300 users with 2..25 items, every seventh with a repeat purchase; user 40 excludes 257 items (its target among them), user 41
    excludes 600; user 42's sequence is only its target."""
    rs = np.random.RandomState(2024)
    seqs = []
    for u in range(300):
        L = int(rs.randint(2, 26))
        s = (rs.permutation(ITEMS)[:L] + 1).tolist()
        if u % 7 == 0:
            s[-1 if u % 14 == 0 else L // 2] = s[0]                                       # bought again (every 14th: as the target)
        seqs.append(s)
    seqs[42] = [int(rs.randint(1, ITEMS + 1))]
    hists = [s[:-1] for s in seqs]
    hists[40] = [seqs[40][-1]] + [int(i) for i in (rs.permutation(ITEMS)[:256] + 1)]
    hists[40] = list(dict.fromkeys(hists[40]))[:256] + [hists[40][0]]                      # 257 entries, one a duplicate of the target
    hists[41] = [int(i) for i in rs.permutation(ITEMS) + 1 if i != seqs[41][-1]][:600]       # the target stays rankable
    assert len(hists[40]) == 257 and len(hists[41]) == 600 and len(seqs[42]) == 1
    g = torch.Generator().manual_seed(8)
    item_emb = (torch.randn(ITEMS + 1, 64, generator=g) * 0.5).cuda()
    return seqs, hists, item_emb, userstore.UserStore(seqs, hists, item_num=ITEMS)


@functools.lru_cache(maxsize=None)
def _model(S):
    torch.manual_seed(100 + S)
    return helpers.build_model(helpers.make_args(max_seq_len=S), ITEMS, torch.ones(ITEMS + 1), cached=True)


@pytest.mark.parametrize("S", [5, 10, 20])
@pytest.mark.parametrize("batch", [16, 1024])
def test_store_routes_on_a_synthetic_set(batch, S):
    seqs, hists, item_emb, users = _synthetic()
    assert users.long_users.tolist() == [40, 41] and users.max_hist == 600
    model = _model(S)
    want = evaluate.evaluate_ranks(model, item_emb, seqs, hists, max_seq_len=S, batch=batch)
    got = evaluate.evaluate_ranks_from_store(model, item_emb, users, S, batch=batch)
    assert torch.equal(got, want)
    assert int(want[41]) <= ITEMS - 600 + 1                                               # the 600 exclusions were applied
    w_ids, w_sc = evaluate.recommend_topk(model, item_emb, hists, hists, max_seq_len=S, k=10, batch=batch)
    ids, sc = evaluate.recommend_topk_from_store(model, item_emb, userstore.UserStore(hists, hists, item_num=ITEMS), S, k=10, batch=batch)
    assert torch.equal(ids, w_ids) and torch.equal(sc, w_sc)
    assert not set(ids[41].tolist()) & set(hists[41])
    # metrics from the histogram: Hit@10 equal; nDCG@10 is a float64 sum of at most U positive terms taken in another order (the host sums
    # counts[r] / log2(r + 1) over r, hit_ndcg averages one term per user): they differ by at most U * 2^-53 relative — 3.3e-14 here, 1.1e-11
    # at 1e5 users — so 1e-9 relative is a bound with a 90-fold margin at that size, not a measured tolerance
    hit, ndcg = evaluate.eval_metrics_from_store(model, item_emb, users, S, batch=batch)
    w_hit, w_ndcg = evaluate.hit_ndcg(want)
    assert hit == w_hit and w_ndcg > 0 and abs(ndcg - w_ndcg) <= 1e-9 * w_ndcg


def test_topk_filler_when_fewer_than_k_items_remain():
    """A catalogue so small that `n_items - hs < k`: the excluded items follow in ascending id, taken from the store's host lists."""
    seqs, hists, item_emb, _ = _synthetic()
    small = item_emb[:13].contiguous()                                                    # items 1..12
    rs = np.random.RandomState(3)
    inputs = [(rs.permutation(12)[:int(rs.randint(0, 9))] + 1).tolist() for _ in range(37)]
    excl = [(rs.permutation(12)[:int(rs.randint(0, 13))] + 1).tolist() for _ in range(37)]
    excl[5] = list(range(1, 13))                                                          # nothing left outside the history
    model = _model(10)
    st = userstore.UserStore(inputs, excl, item_num=12)
    for batch in (16, 1024):
        w_ids, w_sc = evaluate.recommend_topk(model, small, inputs, excl, max_seq_len=10, k=10, batch=batch)
        ids, sc = evaluate.recommend_topk_from_store(model, small, st, 10, k=10, batch=batch)
        assert torch.equal(ids, w_ids) and torch.equal(sc, w_sc)
    assert ids[5].tolist() == list(range(1, 11))
    filled = 0
    for u, e in enumerate(excl):                                                          # the tail of a short list: its excluded items, ascending
        free = 12 - len(set(e))
        if free < 10:
            assert ids[u, free:].tolist() == sorted(set(e))[:10 - free], u
            filled += 1
    assert filled > 10


def test_invalid_target_raises_like_evaluate_ranks():
    seqs, hists, item_emb, _ = _synthetic()
    model = _model(10)
    bad_seqs = [list(s) for s in seqs[:40]]
    bad_seqs[7][-1] = ITEMS + 5                                                           # beyond the table: the kernel reports -1
    st = userstore.UserStore(bad_seqs, hists[:40])
    with pytest.raises(IndexError) as ref:
        evaluate.evaluate_ranks(model, item_emb, bad_seqs, hists[:40], max_seq_len=10)
    for fn in (evaluate.evaluate_ranks_from_store, evaluate.eval_metrics_from_store):
        with pytest.raises(IndexError) as got:
            fn(model, item_emb, st, 10)
        assert str(got.value) == str(ref.value) and "users [7]" in str(got.value)
    with pytest.raises(ValueError, match="at least its target"):
        evaluate.evaluate_ranks_from_store(model, item_emb, userstore.UserStore([[1, 2], []], [[1], []]), 10)


# ---- a training step fed from the store -------------------------------------------------------------------------------------------

def test_training_step_from_the_store_equals_the_host_built_batch():
    """A Cached model over a `TapStore`: `train_batch` ids / mask against the same batch built on the host as the reference's dataset does
    (`dataset.py:59-62`).  Same tensors in, same kernels: loss and flat gradient after `FlatTrainer.step` are bitwise equal.

    bs = 2 (22 slots) on purpose: the step itself is a bit-exact function of its inputs only while every bias / gate gradient — summed
    across the 16-row workgroups of the side network with float atomics — has at most TWO adders (a + b = b + a).  From three row tiles on
    the host-built batch does not reproduce ITSELF: measured on an MI355X, four runs of one batch, tensors of 146 whose gradient bits moved
    — 0 at 11, 15, 16 and 22 slots, 35 at 33 slots, 53 at 66 slots (all bias and gate sums); the loss never moved."""
    items, S, bs = 40, 10, 2
    rs = np.random.RandomState(11)
    train = [(rs.permutation(items)[:l] + 1).tolist() for l in (3, 14, 6, 2, 11, 4, 8, 5, 12, 7, 9, 10)]
    users = userstore.UserStore(train, item_num=items)
    args = helpers.make_args(drop_rate=0.0, side_adapter_vit_list="0,1,2,3,4,5", side_adapter_bert_list="0,1,2,3,4,5")
    model = helpers.build_model(args, items, synth.make_pop_prob(items), cached=True)
    g = torch.Generator().manual_seed(5)
    tabs = [torch.randn(items + 1, 7, 768, generator=g) * 0.25 for _ in range(2)]
    model.tap_stores = tuple(tapstore.TapStore(t.cuda(), model.mm_encoder.packed_layers(), "cuda", "fp32") for t in tabs)
    shapes = {n: tuple(p.shape) for n, p in model.named_parameters() if p.requires_grad}
    helpers.load_trainables(model, weights.fill_params_seeded(shapes, seed=557))
    model.train()
    tr = trainer.FlatTrainer(model, args, 1)
    flat0 = tr.flat.clone()
    order = users.epoch_index(0, 2, epoch=3, seed=1)                      # this rank's users for the epoch, on the device
    first = int(order[0])
    index = torch.stack([order[0], order.new_tensor(1 if first != 1 else 8)])     # ... its first user and one longer than the window
    picked = [train[u][-(S + 1):] for u in index.tolist()]
    assert len(picked) == bs and len(train[int(index[1])]) > S + 1

    def step(ids, lm):
        tr.flat.copy_(flat0)
        tr.m.zero_()
        tr.v.zero_()
        tr.step_no = 0
        loss = tr.step(ids, None, None, lm)
        return loss.detach().clone(), tr.grad.clone(), tr.flat.clone()

    h_ids = torch.tensor([[0] * (S + 1 - len(s)) + s for s in picked])
    h_lm = torch.tensor([[0] * (S + 1 - len(s)) + [1] * (len(s) - 1) for s in picked], dtype=torch.float32)
    want = step(h_ids.cuda(), h_lm.cuda())
    ids, lm = users.train_batch(index, S)
    assert torch.equal(ids.cpu(), h_ids) and torch.equal(lm.cpu(), h_lm)
    got = step(ids, lm)
    assert torch.isfinite(want[0]) and want[1].abs().max() > 0
    for a, b, what in zip(got, want, ("loss", "flat gradient", "parameters after the step")):
        assert torch.equal(a, b), what


# ---- world 2 ----------------------------------------------------------------------------------------------------------------------

def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_shard_the_store():
    """Two fresh processes on cuda:0 over gloo (as tests/test_gpu_dp.py starts its ranks): the sharded store routes equal the single-rank
    ones — and the host-packed routes — on every rank."""
    import user_store_dp_worker as W
    world = 2
    out = tempfile.mkdtemp(prefix="iisan_users_dp_")
    env = dict(os.environ, WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), DP_OUT=out,
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    logs = [open(os.path.join(out, f"rank{r}.log"), "w+") for r in range(world)]       # one file per rank: a full pipe would block a rank
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "user_store_dp_worker.py")], env=dict(env, RANK=str(r)), stdout=logs[r],
                              stderr=subprocess.STDOUT, text=True) for r in range(world)]

    def tail(r):
        logs[r].flush()
        logs[r].seek(0)
        return logs[r].read()[-4000:]

    try:
        for p in procs:
            p.wait(timeout=300)
    except subprocess.TimeoutExpired:
        for q in procs:
            q.kill()
        raise AssertionError("ranks timed out:\n" + "\n".join(f"--- rank {r} ---\n{tail(r)}" for r in range(world)))
    for r, p in enumerate(procs):
        assert p.returncode == 0, "rank %d failed:\n" % r + "\n".join(f"--- rank {q} ---\n{tail(q)}" for q in range(world))
    for f in logs:
        f.close()
    dumps = [torch.load(os.path.join(out, f"rank{r}.pt"), weights_only=False) for r in range(world)]
    for d in dumps:
        assert d["n"] == W.USERS
        assert d["ranks_equal"] and d["ranks_equal_host"] and d["topk_equal"] and d["topk_equal_host"] and d["metrics_equal"], d
        assert torch.equal(d["ranks"], dumps[0]["ranks"])
