#!/usr/bin/env python3
"""Bits and time of the loss and eval kernels per embedding width, through the C ABI alone (workspace and outputs allocated once, HIP
events around batches of calls).  IISAN_LIB=path selects another build of the library - also one from before the width-aware entry
points (`iisan_inbatch_ce_ws_bytes_e`, `iisan_inbatch_ce_route_e`): it is then asked at 64 only.

    python tools/wide_emb_time.py digest         SHA-1 of loss, d_score, d_prec (d_loss 1 and -0.3) at E = 64 for ce_fast 0 / 2 / 4 / 3 at
                                                 bs = 37, 128, 1024 (S = 10), and of the ranks / top-10 ids / scores of one Scientific-size
                                                 eval pass: run once per build and diff
    python tools/wide_emb_time.py loss [reps]    forward + backward, us per call (median and range of five batches), per width, bs = 128
                                                 and 1024, on the fused (ce_fast 4), row-pass (2) and generic (0) routes; at 64 also default
    python tools/wide_emb_time.py eval [reps]    one rank pass and one top-10 pass at 12,076 users x 20,315 items per width, us
Alternate the builds (one process each) and read a build's median against the spread the other shows against itself."""
import ctypes as C
import hashlib
import os
import random
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from iisan_amd import _lib, synth

if os.environ.get("IISAN_LIB"):
    _lib.LIB_PATH = os.path.abspath(os.environ["IISAN_LIB"])
    have = C.CDLL(_lib.LIB_PATH)
    for name in [n for n in _lib.SIGNATURES if not hasattr(have, n)]:
        del _lib.SIGNATURES[name]
lib = _lib.load()
WIDE = "iisan_inbatch_ce_ws_bytes_e" in _lib.SIGNATURES
WIDTHS = (64, 128, 192, 256) if WIDE else (64,)
if os.environ.get("IISAN_WIDTHS"):             # e.g. IISAN_WIDTHS=64 for the rounds of an A/B against an older build
    WIDTHS = tuple(int(w) for w in os.environ["IISAN_WIDTHS"].split(",") if int(w) in WIDTHS)


def st():
    return torch.cuda.current_stream().cuda_stream


def sha(t):
    return hashlib.sha1(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


class Loss:
    def __init__(self, bs, S, E):
        rnd = random.Random(bs + S)
        lengths = [rnd.randint(2, S + 1) for _ in range(bs)]
        b = synth.scientific_batch(bs=bs, seed=90 + bs + S, item_num=max(40, bs * 3), res=2, words=2, lengths=lengths, dup_items=True, seq_len=S)
        g = torch.Generator().manual_seed(bs + S + E)
        self.bs, self.S, self.E = bs, S, E
        self.score = (torch.randn(bs * (S + 1), E, generator=g) * 0.4 * (64 / E) ** 0.5).cuda()
        self.prec = (torch.randn(bs * S, E, generator=g) * 0.4).cuda()
        self.ids, self.lm, self.pop = b.ids.view(-1).cuda(), b.log_mask.float().cuda(), b.pop_prob.float().cuda()
        need = lib.iisan_inbatch_ce_ws_bytes_e(bs, S, E) if WIDE else lib.iisan_inbatch_ce_ws_bytes(bs, S)
        self.need = need
        self.ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
        self.loss = torch.zeros((), device="cuda")
        self.ds, self.dp = torch.empty_like(self.score), torch.empty_like(self.prec)
        self.tok = C.c_uint64(0)

    def fwd(self):
        _lib.check(lib.iisan_inbatch_ce_fwd(self.ids.data_ptr(), self.score.data_ptr(), self.prec.data_ptr(), self.lm.data_ptr(), self.pop.data_ptr(),
                                            self.pop.numel(), self.bs, self.S, self.E, self.loss.data_ptr(), self.ws.data_ptr(), self.need,
                                            C.byref(self.tok), st()), "iisan_inbatch_ce_fwd")

    def bwd(self, d=1.0):
        _lib.check(lib.iisan_inbatch_ce_bwd(self.ids.data_ptr(), self.score.data_ptr(), self.prec.data_ptr(), self.lm.data_ptr(), self.pop.data_ptr(),
                                            self.bs, self.S, self.E, d, self.ds.data_ptr(), self.dp.data_ptr(), self.ws.data_ptr(), self.need,
                                            self.tok.value, st()), "iisan_inbatch_ce_bwd")


class Eval:
    def __init__(self, E, U=12076, n1=20315, k=10):
        g = torch.Generator().manual_seed(2026 + E)
        self.U, self.n1, self.E, self.k = U, n1, E, k
        self.item = (torch.randn(n1, E, generator=g) * 0.5).cuda()
        self.prec = torch.randn(U, E, generator=g).cuda()
        lens = torch.randint(2, 12, (U,), generator=g)
        hist = torch.randint(1, n1, (U, 11), generator=g, dtype=torch.int32)
        hist[torch.arange(11)[None, :] >= lens[:, None]] = 0
        self.hist = hist.cuda()
        self.tgt = torch.randint(1, n1, (U,), generator=g, dtype=torch.int32).cuda()
        self.ranks = torch.empty(U, dtype=torch.int32, device="cuda")
        self.ids = torch.empty(U, k, dtype=torch.int32, device="cuda")
        self.sc = torch.empty(U, k, device="cuda")
        self.nb = lib.iisan_score_topk_ws_bytes(U, n1, k)
        self.ws = torch.empty(max(self.nb, 16), dtype=torch.uint8, device="cuda")

    def rank(self):
        _lib.check(lib.iisan_score_rank(self.prec.data_ptr(), self.item.data_ptr(), self.U, self.n1, self.E, self.hist.data_ptr(), 11,
                                        self.tgt.data_ptr(), self.ranks.data_ptr(), st()), "iisan_score_rank")

    def topk(self):
        _lib.check(lib.iisan_score_topk(self.prec.data_ptr(), self.item.data_ptr(), self.U, self.n1, self.E, self.hist.data_ptr(), 11, self.k,
                                        self.ids.data_ptr(), self.sc.data_ptr(), self.ws.data_ptr(), self.nb, st()), "iisan_score_topk")


def timed(what, f, reps):
    for _ in range(3):
        f()
    ts = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            f()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / reps * 1e3)
    print(f"{what}: median {sorted(ts)[2]:.1f} us (min {min(ts):.1f}, max {max(ts):.1f})", flush=True)


def digest():
    for bs in (37, 128, 1024):
        c = Loss(bs, 10, 64)
        for ce_fast in (0, 2, 4, 3):
            with _lib.dev(ce_fast=ce_fast):
                c.fwd()
                out = [f"loss {sha(c.loss)}"]
                for d in (1.0, -0.3):
                    c.ds.fill_(float("nan"))
                    c.dp.fill_(float("nan"))
                    c.bwd(d)
                    out.append(f"d_loss {d}: d_score {sha(c.ds)} d_prec {sha(c.dp)}")
            print(f"E 64 bs {bs} ce_fast {ce_fast}: " + "  ".join(out) + f"  (loss {c.loss.item():.7f})", flush=True)
    _lib.dev_set("count:ce16", 0)
    e = Eval(64)
    e.rank()
    e.topk()
    print(f"E 64 eval: ranks {sha(e.ranks)} top-10 ids {sha(e.ids)} scores {sha(e.sc)}", flush=True)


def loss_times(reps):
    for E in WIDTHS:
        for bs in (128, 1024):
            c = Loss(bs, 10, E)

            def both():
                c.fwd()
                c.bwd()

            routes = (("fused", 4), ("rowpass", 2), ("generic", 0)) + ((("default", 1),) if E == 64 else ())
            for name, ce_fast in routes:
                with _lib.dev(ce_fast=ce_fast):
                    timed(f"loss E {E} bs {bs} {name} (workspace {c.need / 1e6:.1f} MB)", both, reps if ce_fast else max(3, reps // 4))
    _lib.dev_set("count:ce16", 0)


def eval_times(reps):
    for E in WIDTHS:
        e = Eval(E)
        timed(f"rank E {E} 12076 x 20315", e.rank, reps)
        timed(f"top-10 E {E} 12076 x 20315", e.topk, reps)
        print(f"E {E} eval: ranks {sha(e.ranks)} top-10 ids {sha(e.ids)} scores {sha(e.sc)}", flush=True)


if __name__ == "__main__":
    print(f"library: {_lib.LIB_PATH}")
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    if mode == "digest":
        digest()
    elif mode == "loss":
        loss_times(reps)
    elif mode == "eval":
        eval_times(reps)
    else:
        sys.exit(__doc__)
