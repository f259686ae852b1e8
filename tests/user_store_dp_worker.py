"""One rank of `tests/test_gpu_user_store_eval.py::test_two_ranks_shard_the_store`: `evaluate_ranks_from_store` / `recommend_topk_from_store`
with (rank, world = 2) over gloo, both ranks on cuda:0, against the single-rank result of the same process.  Environment as
`tests/dp_gpu_worker.py`: RANK, WORLD_SIZE, MASTER_ADDR, MASTER_PORT, DP_OUT."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ITEM_NUM, USERS, S, BATCH = 120, 23, 10, 4


def problem(dev):
    """Model, item table and users — the same on every rank (seeded)."""
    from iisan_amd import factory
    torch.manual_seed(31)
    model = factory.build_model(factory.make_args(max_seq_len=S), ITEM_NUM, torch.ones(ITEM_NUM + 1), cached=True, device=dev)
    g = torch.Generator().manual_seed(5)
    item_emb = (torch.randn(ITEM_NUM + 1, 64, generator=g) * 0.5).to(dev)
    seqs, hists = [], []
    for u in range(USERS):
        L = int(torch.randint(1, 16, (1,), generator=g))
        s = (torch.randperm(ITEM_NUM, generator=g)[:L] + 1).tolist()
        seqs.append(s)
        hists.append(s[:-1])
    hists[USERS - 1] = (torch.randperm(ITEM_NUM, generator=g)[:ITEM_NUM - 4] + 1).tolist()     # the padded tail repeats this user; top-k filler
    return model, item_emb, seqs, hists


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from iisan_amd import evaluate, userstore
    model, item_emb, seqs, hists = problem(dev)
    users = userstore.UserStore(seqs, hists, item_num=ITEM_NUM, device=dev)
    r_w = evaluate.evaluate_ranks_from_store(model, item_emb, users, S, batch=BATCH, rank=rank, world=world)
    r_1 = evaluate.evaluate_ranks_from_store(model, item_emb, users, S, batch=BATCH)
    r_h = evaluate.evaluate_ranks(model, item_emb, seqs, hists, S, batch=BATCH)
    t_w, s_w = evaluate.recommend_topk_from_store(model, item_emb, users, S, k=10, batch=BATCH, rank=rank, world=world, holdout=True)
    t_1, s_1 = evaluate.recommend_topk_from_store(model, item_emb, users, S, k=10, batch=BATCH, holdout=True)
    t_h, s_h = evaluate.recommend_topk(model, item_emb, [s[:-1] for s in seqs], hists, S, k=10, batch=BATCH)
    m_w = evaluate.eval_metrics_from_store(model, item_emb, users, S, batch=BATCH, rank=rank, world=world)
    out = dict(rank=rank, n=int(r_w.numel()), ranks_equal=bool(torch.equal(r_w, r_1)), ranks_equal_host=bool(torch.equal(r_1, r_h)),
               topk_equal=bool(torch.equal(t_w, t_1) and torch.equal(s_w, s_1)),
               topk_equal_host=bool(torch.equal(t_1, t_h) and torch.equal(s_1, s_h)),
               metrics_equal=m_w == evaluate.eval_metrics_from_store(model, item_emb, users, S, batch=BATCH), ranks=r_w.cpu())
    torch.save(out, os.path.join(os.environ["DP_OUT"], f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
