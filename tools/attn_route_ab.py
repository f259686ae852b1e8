"""Isolated A/B of the two ViT attention routes (dev switch attn_route: 1 = attention16_kernel, 2 = the LDS-DMA kernel of attn16_dma.hip)
at the production launch, 1,408 items x 12 heads x 197 tokens, fp16 and bf16: the routes alternate in ONE process, `--rounds` interleaved
rounds of `--launches` launches under HIP events; prints median and min-max of the per-round means per route.  The BERT shape (S = 30, key
bias: always attention16_kernel) is timed under both settings as the control: it must not move.

    python tools/attn_route_ab.py [--lib path/to/libiisan_hip.so] [--rounds 5] [--launches 40]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from iisan_amd import _lib  # noqa: E402


def timed(lib, dt, qkv, kb, ctx, launches):
    items, heads, _, S, _ = qkv.shape
    st = torch.cuda.current_stream().cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        _lib.check(lib.iisan_attention16(dt, qkv.data_ptr(), kb.data_ptr() if kb is not None else None, ctx.data_ptr(), items, S, heads, st),
                   "attention16")
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches          # us per launch


def ab(lib, name, dt, qkv, kb, rounds, launches, settings):
    """settings: [(label, {switch: value})]; the labels alternate inside every round"""
    ctx = torch.empty(qkv.shape[0] * qkv.shape[3], qkv.shape[1] * 64, dtype=qkv.dtype, device="cuda")
    t = {label: [] for label, _ in settings}
    try:
        for r in range(rounds + 1):                        # round 0 = warm-up, not reported
            for label, knobs in settings:
                _lib.dev_reset()
                for k, v in knobs.items():
                    _lib.dev_set(k, v)
                us = timed(lib, dt, qkv, kb, ctx, launches)
                if r:
                    t[label].append(us)
    finally:
        _lib.dev_reset()
    for label, _ in settings:
        v = t[label]
        print(f"{name:28s} {label:16s} median {statistics.median(v):7.1f} us   min-max {min(v):7.1f} - {max(v):7.1f}   (spread {max(v) - min(v):5.1f})",
              flush=True)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=40)
    a = ap.parse_args()
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    lib = _lib.load()
    routes = [("route 1 (old)", {"attn_route": 1}), ("route 2 (dma)", {"attn_route": 2})]
    g = torch.Generator(device="cuda").manual_seed(1)
    for dt, T in ((0, torch.float16), (1, torch.bfloat16)):
        qkv = torch.randn(1408, 12, 3, 197, 64, device="cuda", generator=g).to(T)
        ab(lib, f"ViT 1408x12x197 {str(T)[6:]}", dt, qkv, None, a.rounds, a.launches, routes)
        del qkv
    # control: BERT, 1,408 items x 12 heads x 30 tokens with a key bias — attention16_kernel under every setting
    qkv = torch.randn(1408, 12, 3, 30, 64, device="cuda", generator=g).half()
    kb = torch.zeros(1408, 30, device="cuda")
    kb[:, 20:] = -1.0
    ab(lib, "BERT 1408x12x30 float16", 0, qkv, kb, a.rounds, a.launches, [("route 1 (old)", {"attn_route": 1}), ("route 2 (dma)", {"attn_route": 2})])


if __name__ == "__main__":
    main()
