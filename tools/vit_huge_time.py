#!/usr/bin/env python3
"""ViT-H/14 timings for profiles/vit_huge.md (development aid; bench.py is the contract benchmark).  One process, device events around
each launch, the first launch of everything dropped, medians reported:

    python3 tools/vit_huge_time.py [--items 1408] [--attn-items 128] [--reps 20] [--iters 2]

  attention   `iisan_attention16_hd80` at --attn-items x 16 heads x 257 tokens (one layer of the tower), and beside it, in the same run,
              `iisan_attention16_long` at the same S with 20 heads of 64: the same Q / K / V / context bytes, the yardstick.
  tower       `weights.VIT_HUGE` (32 layers), random weights drawn on the device, the taps of all 33 hidden states over --items slots —
              what `evaluate.build_tap_cache` asks for; items/s from a host clock around work that ends in a synchronise.
Prints one JSON line per measurement and the markdown lines of the profile."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _event_us(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return statistics.median(out), min(out), max(out)


def attention(a):
    import torch
    from iisan_amd import _lib
    if os.environ.get("IISAN_LIB"):            # another build of the library (the parent's, copied aside), timed beside this one
        _lib.LIB_PATH = os.path.abspath(os.environ["IISAN_LIB"])
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    items, S = a.attn_items, 257
    res = {}
    for name, entry, heads, hd in (("hd80", "iisan_attention16_hd80", 16, 80), ("long", "iisan_attention16_long", 20, 64)):
        D = heads * hd
        qkv = (torch.randn(items * S * 3 * D, device="cuda") * 1.5).half()       # row-major for hd80, head-major for long: the same bytes
        ctx = torch.empty(items * S, D, dtype=torch.float16, device="cuda")
        fn = lambda: _lib.check(getattr(lib, entry)(0, qkv.data_ptr(), None, ctx.data_ptr(), items, S, heads, s), entry)
        med, lo, hi = _event_us(fn, a.reps)
        assert torch.isfinite(ctx.float()).all()
        flop = 4.0 * items * heads * S * S * hd
        res[name] = dict(kernel=entry, items=items, heads=heads, head_dim=hd, S=S, median_us=round(med, 1), min_us=round(lo, 1), max_us=round(hi, 1),
                         tflops=round(flop / med / 1e6, 1), gbytes=round(items * S * 4 * D * 2 / 1e9, 3))
        print(json.dumps(res[name]))
    return res


def tower(a):
    import torch
    from iisan_amd import encoders, weights
    from tools.wide_time import device_weights
    cfg = weights.VIT_HUGE
    vit = encoders.PackedVit(device_weights(cfg, True), cfg, "cuda", 0)
    x = torch.randn(a.items, 3, cfg.image, cfg.image, device="cuda").clamp_(-1, 1)
    taps = list(range(cfg.layers + 1))
    out = vit.forward_taps(x, taps, a.chunk)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.iters):
        out = vit.forward_taps(x, taps, a.chunk)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / a.iters * 1e3
    assert out.shape == (a.items, 33, 1280) and torch.isfinite(out).all()
    res = dict(tower="vit-huge-patch14-224", items=a.items, chunk_items=a.chunk, tokens=cfg.tokens, taps=33, forwards=a.iters,
               wall_ms_per_forward=round(ms, 1), items_per_s=round(a.items / ms * 1e3, 1))
    print(json.dumps(res))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1408)
    ap.add_argument("--chunk", type=int, default=0)
    ap.add_argument("--attn-items", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--skip-tower", action="store_true")
    a = ap.parse_args()
    at = attention(a)
    print(f"\n| kernel | items x heads x head width | S | median us (min - max, {a.reps} launches) | TFLOP/s |\n|---|---|---|---|---|")
    for k in ("hd80", "long"):
        r = at[k]
        print(f"| `{r['kernel']}` | {r['items']} x {r['heads']} x {r['head_dim']} | {r['S']} | {r['median_us']} ({r['min_us']} - {r['max_us']}) | {r['tflops']} |")
    if not a.skip_tower:
        t = tower(a)
        print(f"\nViT-H/14, {t['items']} slots, all 33 taps: {t['wall_ms_per_forward']} ms per forward = {t['items_per_s']} items/s")


if __name__ == "__main__":
    main()
