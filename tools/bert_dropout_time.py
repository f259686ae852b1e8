#!/usr/bin/env python
"""What the opt-in train-mode dropout of the frozen BERT tower costs (profiles/r8_bert_dropout.md).

Three comparisons at the bench shape (bs = 128: M = 1408 item slots, 30 words, BERT-base, the IISAN tap list 0,2,..,12, every block on
every token as `bench.py` runs it), each in interleaved rounds — eval, dropout, eval, dropout, ... — so that a drift of the box hits
both sides alike; the eval-mode route is the yardstick on the same box, in the same process:

  attention   `iisan_attention16` against `iisan_attention16_dropout` (p = 0.1) on one layer's QKV: S = 30, 1408 items, 12 heads
  tower       `PackedBert.forward_taps` without and with `dropout=(0.1, 0.1, seed)`
  step        one `FlatTrainer.step` (fwd + bwd + Adam from the same state) with `Text_Encoder.train_dropout` off and on

and one check: with the switch off the step launches no train-mode kernel — neither the attention kernel of csrc/bert_drop.hip nor a
keep-functor instantiation of the row kernels of csrc/rowops.hip: `count:bert_drop` counts both and stays 0 (37 per step with the
switch on) — and the same number of encoder GEMMs as before the switch existed in the process.  Prints one JSON line per comparison."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def interleaved(fns, rounds, reps, warmup=2):
    """{name: [ms per call, one per round]}: every round times each function in turn, `reps` calls between two device syncs."""
    out = {k: [] for k in fns}
    for k, f in fns.items():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, f in fns.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(reps):
                f()
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t) / reps * 1e3)
    return out


def summary(name, res, base, other, **kw):
    b, o = statistics.median(res[base]), statistics.median(res[other])
    r = {"case": name, base + "_ms": round(b, 4), other + "_ms": round(o, 4), "delta_ms": round(o - b, 4),
         "ratio": round(o / b, 4), "rounds_" + base: [round(x, 4) for x in res[base]], "rounds_" + other: [round(x, 4) for x in res[other]]}
    r.update(kw)
    print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cases", default="attention,tower,step")
    a = ap.parse_args()
    from iisan_amd import _lib, encoders, factory, synth, trainer, weights
    lib = _lib.load()
    dev = torch.device("cuda:0")
    cases = a.cases.split(",")
    b = synth.scientific_batch(bs=a.bs, seed=12345, device="cuda", images_on_device=True)
    M, W, H = b.text.shape[0], b.text.shape[1] // 2, 12
    stream = torch.cuda.current_stream().cuda_stream
    bw = weights.make_bert_weights()

    if "attention" in cases:
        g = torch.Generator(device=dev).manual_seed(4)
        qkv = (torch.randn(M, H, 3, W, 64, device=dev, generator=g) * 1.5).half()
        kb = torch.where(b.text[:, W:] != 0, 0.0, -1.0).float().contiguous()
        ctx = torch.empty(M * W, H * 64, dtype=torch.float16, device=dev)
        res = interleaved({
            "eval": lambda: _lib.check(lib.iisan_attention16(0, qkv.data_ptr(), kb.data_ptr(), ctx.data_ptr(), M, W, H, stream), "attention16"),
            "dropout": lambda: _lib.check(lib.iisan_attention16_dropout(0, qkv.data_ptr(), kb.data_ptr(), ctx.data_ptr(), M, W, H, 0.1, 7, 1, 0, stream),
                                          "attention16_dropout"),
        }, a.rounds, a.reps * 20)
        summary("attention S=%d items=%d heads=%d" % (W, M, H), res, "eval", "dropout")

    if "tower" in cases:
        pk = encoders.PackedBert(bw, weights.BERT_BASE, dev)
        pk.full_blocks = True
        taps = [0, 2, 4, 6, 8, 10, 12]
        res = interleaved({
            "eval": lambda: pk.forward_taps(b.text, taps),
            "dropout": lambda: pk.forward_taps(b.text, taps, dropout=(0.1, 0.1, 7)),
        }, a.rounds, a.reps)
        summary("text tower M=%d words=%d" % (M, W), res, "eval", "dropout")
        del pk

    if "step" in cases:
        torch.manual_seed(20260)
        args = factory.make_args()
        model = factory.build_model(args, synth.SCI_ITEM_NUM, b.pop_prob, weights.make_vit_weights(), weights.VIT_BASE, bw, weights.BERT_BASE,
                                    cached=False, device=dev)
        enc = model.mm_encoder
        title = enc.bert_encoder.text_encoders["title"]
        enc.cv_encoder.full_blocks = True
        title.full_blocks = True
        model.train()
        tr = trainer.FlatTrainer(model, args, 1)
        flat0, rng0 = tr.flat.clone(), torch.get_rng_state()
        ids, lm = b.ids.view(-1), b.log_mask

        def step(on):       # bench.py's step: every step is the same computation from the same state
            title.train_dropout = on
            torch.set_rng_state(rng0)
            tr.flat.copy_(flat0)
            tr.m.zero_()
            tr.v.zero_()
            tr.step_no = 0
            return tr.step(ids, b.images, b.text, lm)

        counters = ["count:bert_drop", "count:gemm16_h256", "count:gemm16_s256", "count:gemm16_v1"]
        launches = {}
        for on in (False, True):
            step(on)
            for c in counters:
                _lib.dev_set(c, 0)
            loss = float(step(on).detach())
            launches["on" if on else "off"] = dict({c: _lib.dev_get(c) for c in counters}, loss=loss)
        res = interleaved({"off": lambda: step(False), "on": lambda: step(True)}, a.rounds, a.reps)
        title.train_dropout = False
        summary("FlatTrainer.step bs=%d" % a.bs, res, "off", "on", launches_per_step=launches)


if __name__ == "__main__":
    main()
