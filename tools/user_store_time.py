#!/usr/bin/env python
"""An eval pass by where the user side of its batches is built (profiles/user_store.md).

Scientific size: 12,076 users x 20,315 table rows, S = 10, E = 64, batch 1,024; seeded synthetic sequences with the length histogram
of `synth.SCI_LEN_HIST`, exclusion list = the sequence without its target (`user_history`).  Two routes per output, in the same process,
ALTERNATING pass by pass after a warm-up, host clock around a device synchronise:

  ranks  host   `evaluate.evaluate_ranks`: `_pack_users` on the host, four tensors shipped per user batch
         store  `evaluate.evaluate_ranks_from_store`: windows, masks, targets, exclusion lists built on the device from a `UserStore`
  topk   host   `evaluate.recommend_topk`            store  `evaluate.recommend_topk_from_store`
  hit    host   `hit_ndcg(evaluate_ranks(...))`      store  `evaluate.eval_metrics_from_store` (rank histogram, 12 integers copied back)

Prints one JSON line per (output, route): median, min, max in ms over `--repeats` passes, and whether the two routes' results were
bit-equal.  The store's one-off construction (CSR on the host + upload) is reported on its own line; it is not part of a pass.

`--trace DIR`: instead of timing, runs the store route under `rocprofv3 --kernel-trace --memory-copy-trace --stats` in two child processes
of their own (4 and 12 passes of ranks + topk) and prints, per pass (the difference of the two runs / 8), the kernel lines and the copies
left in the loop.
"""
import argparse
import json
import os
import sqlite3
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

USERS, S, E, BATCH, K = 12076, 10, 64, 1024, 10


def problem(dev):
    from iisan_amd import factory, synth
    rs = np.random.RandomState(12345)
    ls = np.array(sorted(synth.SCI_LEN_HIST))
    pr = np.array([synth.SCI_LEN_HIST[int(l)] for l in ls], dtype=np.float64)
    lens = rs.choice(ls, size=USERS, p=pr / pr.sum())
    seqs = [rs.randint(1, synth.SCI_ITEM_NUM + 1, size=int(l)).tolist() for l in lens]
    hists = [s[:-1] for s in seqs]
    torch.manual_seed(7)
    model = factory.build_model(factory.make_args(max_seq_len=S, embedding_dim=E), synth.SCI_ITEM_NUM, torch.ones(synth.SCI_ITEM_NUM + 1),
                                cached=True, device=dev)
    g = torch.Generator().manual_seed(8)
    item_emb = (torch.randn(synth.SCI_ITEM_NUM + 1, E, generator=g) * 0.5).to(dev)
    return model, item_emb, seqs, hists


def routes(model, item_emb, seqs, hists, users):
    from iisan_amd import evaluate
    return {
        "ranks": (lambda: evaluate.evaluate_ranks(model, item_emb, seqs, hists, S, batch=BATCH),
                  lambda: evaluate.evaluate_ranks_from_store(model, item_emb, users, S, batch=BATCH)),
        "topk": (lambda: evaluate.recommend_topk(model, item_emb, hists, hists, S, k=K, batch=BATCH),
                 lambda: evaluate.recommend_topk_from_store(model, item_emb, users, S, k=K, batch=BATCH, holdout=True)),
        "hit": (lambda: evaluate.hit_ndcg(evaluate.evaluate_ranks(model, item_emb, seqs, hists, S, batch=BATCH), K),
                lambda: evaluate.eval_metrics_from_store(model, item_emb, users, S, batch=BATCH, topk=K)),
    }


def same(a, b):
    if isinstance(a, torch.Tensor):
        return bool(torch.equal(a, b))
    if isinstance(a[0], torch.Tensor):
        return all(bool(torch.equal(x, y)) for x, y in zip(a, b))
    return a[0] == b[0] and abs(a[1] - b[1]) <= 1e-9 * abs(b[1])


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def run(a):
    from iisan_amd import userstore
    dev = torch.device("cuda:0")
    model, item_emb, seqs, hists = problem(dev)
    t = time.perf_counter()
    users = userstore.UserStore(seqs, hists, item_num=item_emb.shape[0] - 1, device=dev)
    torch.cuda.synchronize()
    print(json.dumps({"case": "store_build", "ms_once": round((time.perf_counter() - t) * 1e3, 2), "device_bytes": users.nbytes(),
                      "users": USERS, "interactions": int(users.seq_items.numel())}), flush=True)
    for name, (host, store) in routes(model, item_emb, seqs, hists, users).items():
        if name not in a.outputs.split(","):
            continue
        if a.route == "store":                           # the profiled child: the store route alone
            for _ in range(a.warmup + a.repeats):
                store()
            torch.cuda.synchronize()
            continue
        for _ in range(a.warmup):
            host(), store()
        ms = {"host": [], "store": []}
        equal = True
        for _ in range(a.repeats):                       # alternating: host, store, host, store, ...
            th, oh = timed(host)
            ts, os_ = timed(store)
            ms["host"].append(th)
            ms["store"].append(ts)
            equal = equal and same(os_, oh)
        for r in ("host", "store"):
            v = np.array(ms[r])
            print(json.dumps({"case": name, "route": r, "median_ms": round(float(np.median(v)), 3), "min_ms": round(float(v.min()), 3),
                              "max_ms": round(float(v.max()), 3), "repeats": a.repeats, "results_equal": equal}), flush=True)


def trace(a):
    """Two profiled children (no GPU state in this process); per-pass figures from their difference."""
    n = (4, 12)
    agg = []
    for r in n:
        out = os.path.join(a.trace, f"passes{r}")
        os.makedirs(out, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--memory-copy-trace", "--stats", "-d", out, "-o", "users", "--", sys.executable,
               os.path.abspath(__file__), "--route", "store", "--warmup", "0", "--repeats", str(r), "--outputs", "ranks,topk"]
        with open(os.path.join(out, "child.log"), "w") as log:
            subprocess.run(cmd, check=True, stdout=log, stderr=subprocess.STDOUT, timeout=600)
        dbs = [os.path.join(d, f) for d, _, fs in os.walk(out) for f in fs if f.endswith(".db")]
        db = sqlite3.connect(dbs[0])
        kern = {}
        for name, dur in db.execute("select name, duration from kernels"):
            k = kern.setdefault(name, [0, 0])
            k[0] += 1
            k[1] += dur
        copies = {}
        try:
            cols = [c[1] for c in db.execute("pragma table_info(memory_copies)")]
            kind = next(c for c in ("name", "kind", "direction") if c in cols)
            size = next((c for c in ("size", "bytes") if c in cols), None)
            for row in db.execute(f"select {kind}, duration{', ' + size if size else ''} from memory_copies"):
                c = copies.setdefault(str(row[0]), [0, 0, 0])
                c[0] += 1
                c[1] += row[1]
                c[2] += row[2] if size else 0
        except Exception as e:                           # a rocprofv3 without that view: say so instead of guessing
            copies = {"(memory_copies view not readable: %s)" % e: [0, 0, 0]}
        db.close()
        for f in dbs:
            os.remove(f)
        agg.append((kern, copies))
    d = n[1] - n[0]
    print(f"per pass of ranks + topk on the store route ((run of {n[1]} passes - run of {n[0]}) / {d}):\n")
    print("| kernel | launches | total us | avg us |\n|---|---|---|---|")
    rows = []
    for name in agg[1][0]:
        c1, t1 = agg[1][0][name]
        c0, t0 = agg[0][0].get(name, [0, 0])
        if c1 > c0:
            rows.append((name, (c1 - c0) / d, (t1 - t0) / d / 1e3, (t1 - t0) / (c1 - c0) / 1e3))
    for name, c, tot, avg in sorted(rows, key=lambda r: -r[2]):
        print(f"| `{name if len(name) < 100 else name[:97] + '...'}` | {c:g} | {tot:.1f} | {avg:.2f} |")
    print(f"\nkernel time per pass: {sum(r[2] for r in rows):.1f} us over {sum(r[1] for r in rows):g} launches\n")
    print("| copy | per pass | total us | bytes |\n|---|---|---|---|")
    for name in agg[1][1]:
        c1, t1, b1 = agg[1][1][name]
        c0, t0, b0 = agg[0][1].get(name, [0, 0, 0])
        print(f"| {name} | {(c1 - c0) / d:g} | {(t1 - t0) / d / 1e3:.1f} | {(b1 - b0) / d:g} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--outputs", default="ranks,topk,hit")
    ap.add_argument("--route", default="both", choices=["both", "store"])
    ap.add_argument("--trace", default=None, metavar="DIR")
    a = ap.parse_args()
    trace(a) if a.trace else run(a)


if __name__ == "__main__":
    main()
