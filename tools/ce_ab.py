#!/usr/bin/env python3
"""Same-box A/B of two builds of the in-batch loss (csrc/ce.hip): bits and time.  IISAN_LIB=tools/lib_prev.so selects the other build.

    python tools/ce_ab.py digest      SHA-1 of the raw bytes of loss, d_score and d_prec at d_loss = 1 and -0.3, for ce_fast 0 / 2 / 4 / 3
                                      at (bs, S) = (37, 10), (3, 15), (7, 5), (64, 4), (1024, 10): run once per build and diff the outputs
                                      (the split route's only atomic is an atomicMax, every combine has a fixed order: all of it reproduces)
    python tools/ce_ab.py time [reps] forward + backward of `ops.InbatchCeFn` alone, HIP-event timed (as tools/ce_sweep.py), us per call:
                                      bs = 128 and bs = 1024 on default knobs, bs = 1024 under ce_fast = 4 and ce_fast = 0
    python tools/ce_ab.py time reps bs   that batch size on default knobs alone (under rocprofv3 --kernel-trace: bs = 128 is bound by the
                                      host's launches, its kernel times are read from the trace)
Alternate the builds over at least three rounds (one process each, as tools/ab_lib.sh does) and read the new build's median against the
spread the old one shows against itself."""
import ctypes as C
import hashlib
import os
import random
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from iisan_amd import _lib, ops, synth

if os.environ.get("IISAN_LIB"):
    _lib.LIB_PATH = os.path.abspath(os.environ["IISAN_LIB"])
    # a build from before an entry point was added: `digest` calls the 64-wide ABI alone and still runs (`time` goes through `ops`, which
    # asks iisan_inbatch_ce_ws_bytes_e; tools/wide_emb_time.py times either build through the ABI)
    for name in [n for n in _lib.SIGNATURES if not hasattr(C.CDLL(_lib.LIB_PATH), n)]:
        del _lib.SIGNATURES[name]
lib = _lib.load()
E = 64


def problem(bs, S):
    """ragged sequence lengths, history padding, a duplicated item: the recipe of the loss tests"""
    rnd = random.Random(bs + S)
    lengths = [rnd.randint(2, S + 1) for _ in range(bs)]
    b = synth.scientific_batch(bs=bs, seed=90 + bs + S, item_num=max(40, bs * 3), res=2, words=2, lengths=lengths, dup_items=True, seq_len=S)
    g = torch.Generator().manual_seed(bs + S)
    score = (torch.randn(bs * (S + 1), E, generator=g) * 0.4).cuda()
    prec = (torch.randn(bs * S, E, generator=g) * 0.4).cuda()
    return b.ids.view(-1).cuda(), score, prec, b.log_mask.float().cuda(), b.pop_prob.float().cuda()


def sha(t):
    return hashlib.sha1(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def digest():
    st = torch.cuda.current_stream().cuda_stream
    for bs, S in ((37, 10), (3, 15), (7, 5), (64, 4), (1024, 10)):
        ids, score, prec, lm, pop = problem(bs, S)
        for ce_fast in (0, 2, 4, 3):
            with _lib.dev(ce_fast=ce_fast):
                route = lib.iisan_inbatch_ce_route(bs, S)
                ws = torch.zeros(lib.iisan_inbatch_ce_ws_bytes(bs, S), dtype=torch.uint8, device="cuda")
                loss, tok = torch.zeros((), device="cuda"), C.c_uint64(0)
                _lib.check(lib.iisan_inbatch_ce_fwd(ids.data_ptr(), score.data_ptr(), prec.data_ptr(), lm.data_ptr(), pop.data_ptr(), pop.numel(),
                                                    bs, S, E, loss.data_ptr(), ws.data_ptr(), ws.numel(), C.byref(tok), st), "iisan_inbatch_ce_fwd")
                out = [f"loss {sha(loss)}"]
                for d in (1.0, -0.3):
                    ds, dp = torch.full_like(score, float("nan")), torch.full_like(prec, float("nan"))
                    _lib.check(lib.iisan_inbatch_ce_bwd(ids.data_ptr(), score.data_ptr(), prec.data_ptr(), lm.data_ptr(), pop.data_ptr(), bs, S, E, d,
                                                        ds.data_ptr(), dp.data_ptr(), ws.data_ptr(), ws.numel(), tok.value, st), "iisan_inbatch_ce_bwd")
                    out.append(f"d_loss {d}: d_score {sha(ds)} d_prec {sha(dp)}")
            print(f"bs {bs} S {S} ce_fast {ce_fast} route {route}: " + "  ".join(out) + f"  (loss {loss.item():.7f})", flush=True)
    _lib.dev_set("count:ce16", 0)


def timed(bs, reps, **knobs):
    ids, score, prec, lm, pop = problem(bs, 10)
    score.requires_grad_(True)
    prec.requires_grad_(True)
    ts = []
    with _lib.dev(**knobs):
        for _ in range(3):
            ops.InbatchCeFn.apply(ids, score, prec, lm, pop).backward()
        for _ in range(5):                    # five batches of `reps` calls between two events; the median batch is the figure
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                ops.InbatchCeFn.apply(ids, score, prec, lm, pop).backward()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / reps * 1e3)
    print(f"bs {bs} {knobs or 'default'}: median {sorted(ts)[2]:.1f} us per call (batches: {' '.join(f'{t:.1f}' for t in ts)})", flush=True)


if __name__ == "__main__":
    print(f"library: {_lib.LIB_PATH}")
    if len(sys.argv) > 1 and sys.argv[1] == "digest":
        digest()
    elif len(sys.argv) > 1 and sys.argv[1] == "time":
        reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
        if len(sys.argv) > 3:                 # one batch size on default knobs alone: what a kernel trace wants
            sys.exit(timed(int(sys.argv[3]), reps))
        timed(128, reps)
        timed(1024, reps, ce_fast=4)
        timed(1024, reps)
        timed(1024, max(3, reps // 4), ce_fast=0)
    else:
        sys.exit(__doc__)
