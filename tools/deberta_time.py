#!/usr/bin/env python3
"""Timings and tap errors that go with the DeBERTa-v2/v3 text tower (profiles/deberta_tower.md).

    python3 tools/deberta_time.py [rounds]

Attention: `iisan_attention16_disent` beside `iisan_attention16` (the BERT kernel, the yardstick) on the same shape — 1,408 items x 30 words
x 12 heads, masked tails, fp16 and bf16 — and at 128 words; the CLS forms of both.  The two kernels alternate inside every round — same
operands, same process — and each sample is device-event time over 20 launches after a warm-up; the table gives the median over the
rounds, the spread (min .. max) and the ratio of the medians.
Tower: all 13 taps of DeBERTa-v3-base (vocab 128100, 30 words) beside BERT-base, 1,408 slots (bs = 128), fp16 and bf16, default dead-work
policy and full_blocks = 1; device-event time per call over 5 calls after a warm-up, the two towers alternating inside every round.
Tap errors: the four towers of tests/golden/deberta_v2.npz against HF's hidden states, per tap layer, fp16 and bf16."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from iisan_amd import _lib, encoders, weights  # noqa: E402

T16 = {_lib.IISAN_F16: torch.float16, _lib.IISAN_BF16: torch.bfloat16}
NAMES = {_lib.IISAN_F16: "fp16", _lib.IISAN_BF16: "bf16"}


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def report(what, ms):
    med = {k: statistics.median(v) for k, v in ms.items()}
    for k, v in ms.items():
        print(f"{what} {k}: median {med[k] * 1e3:.1f} us ({min(v) * 1e3:.1f} .. {max(v) * 1e3:.1f})", flush=True)
    a, b = list(med)
    print(f"{what} ratio {b} / {a}: {med[b] / med[a]:.2f}", flush=True)


def attention(rounds):
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    items, heads, span = 1408, 12, 256
    for S in (30, 128):
        for dt in (_lib.IISAN_F16, _lib.IISAN_BF16):
            g = torch.Generator(device="cuda").manual_seed(S)
            qkv = (torch.randn(items, heads, 3, S, 64, device="cuda", generator=g) * 1.5).to(T16[dt])
            rel = (torch.randn(heads, 3, 2 * span, 64, device="cuda", generator=g) * 1.5).to(T16[dt])
            kb = torch.zeros(items, S, device="cuda")
            lens = torch.randint(3, S + 1, (items,), device="cuda", generator=g)
            kb[torch.arange(S, device="cuda")[None] >= lens[:, None]] = -1.0
            ctx = torch.empty(items * S, heads * 64, device="cuda", dtype=T16[dt])
            cls = torch.empty(items, heads * 64, device="cuda", dtype=T16[dt])
            calls = {
                "attention16": lambda: _lib.check(lib.iisan_attention16(dt, qkv.data_ptr(), kb.data_ptr(), ctx.data_ptr(), items, S, heads, st), "a"),
                "attention16_disent": lambda: _lib.check(lib.iisan_attention16_disent(dt, qkv.data_ptr(), rel.data_ptr(), kb.data_ptr(), ctx.data_ptr(),
                                                                                      items, S, heads, span, st), "d"),
            }
            cls_calls = {
                "attention_cls16": lambda: _lib.check(lib.iisan_attention_cls16(dt, qkv.data_ptr(), kb.data_ptr(), cls.data_ptr(), items, S, heads, st), "a"),
                "attention_cls16_disent": lambda: _lib.check(lib.iisan_attention_cls16_disent(dt, qkv.data_ptr(), rel.data_ptr(), kb.data_ptr(),
                                                                                              cls.data_ptr(), items, S, heads, span, st), "d"),
            }
            for group in (calls, cls_calls):
                ms = {k: [] for k in group}
                for _ in range(rounds):
                    for k, fn in group.items():
                        ms[k].append(timed(fn, 20))
                report(f"{items} items x {S} words x {heads} heads, {NAMES[dt]},", ms)


def towers(rounds):
    words, slots = 30, 1408
    bcfg, dcfg = weights.BERT_BASE, weights.DEBERTA_V3_BASE
    bw, dw = weights.make_bert_weights(bcfg, seed=12), weights.make_deberta_weights(dcfg, seed=61)
    g = torch.Generator(device="cuda").manual_seed(7)
    lens = torch.randint(3, words + 1, (slots,), device="cuda", generator=g)
    mask = (torch.arange(words, device="cuda")[None] < lens[:, None]).long()
    text = torch.cat([torch.randint(1, 30000, (slots, words), device="cuda", generator=g) * mask, mask], 1).contiguous()
    layers = list(range(13))
    for dt in (_lib.IISAN_F16, _lib.IISAN_BF16):
        pk = {"BERT-base": encoders.PackedBert(bw, bcfg, "cuda", dt), "DeBERTa-v3-base": encoders.PackedBert(dw, dcfg, "cuda", dt)}
        for fb in (False, True):
            ms = {k: [] for k in pk}
            for _ in range(rounds):
                for k, p in pk.items():
                    p.full_blocks = fb
                    ms[k].append(timed(lambda: p.forward_taps(text, layers), 5))
            report(f"tower, {slots} slots x {words} words, 13 taps, {NAMES[dt]}, full_blocks={int(fb)},", ms)
        del pk


def tap_errors():
    import deberta_oracle as DO
    for name in DO.TOWERS:
        cfg, w, x, gold = DO.load_golden(name)
        for dt in (_lib.IISAN_F16, _lib.IISAN_BF16):
            got = encoders.PackedBert(w, cfg, "cuda", dt).forward_taps(x.cuda(), list(range(cfg.layers + 1))).cpu()
            print(f"tap errors {name} {NAMES[dt]}: " + " ".join(f"{e:.2e}" for e in DO.tap_errors(got, gold)), flush=True)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("deberta_time.py measures on the GPU: no device visible")
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    tap_errors()
    attention(n)
    towers(n)
