#!/usr/bin/env python3
"""Micro-benchmark of the streaming-softmax attention kernel (csrc/attn16_long.hip; development aid): us per launch in isolation at the
lengths the long towers run, with the achieved TF/s and the bytes of Q / K / V / context over that time — and the kernel forced at
S = 197 beside the production route, alternating in the same run.  Device events around every launch, warm-up first, median of N."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from iisan_amd import _lib  # noqa: E402

if os.environ.get("IISAN_LIB"):            # a variant build (make -C iisan_amd/csrc EXTRA=-DATTN_LONG_NQ=2), copied aside
    _lib.LIB_PATH = os.path.abspath(os.environ["IISAN_LIB"])
lib = _lib.load()
N = int(sys.argv[1]) if len(sys.argv) > 1 else 21


def problem(items, S, heads, masked):
    g = torch.Generator(device="cuda").manual_seed(S)
    qkv = (torch.randn(items, heads, 3, S, 64, device="cuda", generator=g) * 1.5).half()
    ctx = torch.empty(items * S, heads * 64, device="cuda", dtype=torch.float16)
    kb = None
    if masked:          # titles of mixed lengths, item 0 all padding
        n = torch.randint(1, S + 1, (items,), device="cuda", generator=g)
        kb = torch.where(torch.arange(S, device="cuda")[None] < n[:, None], 0.0, -1.0).contiguous()
        kb[0] = -1.0
    return qkv, kb, ctx


def timed(entries, items, S, heads, masked):
    """median us per launch of each entry, the entries alternating launch by launch"""
    qkv, kb, ctx = problem(items, S, heads, masked)
    st = torch.cuda.current_stream().cuda_stream
    kbp = kb.data_ptr() if kb is not None else None
    call = lambda e: _lib.check(getattr(lib, e)(0, qkv.data_ptr(), kbp, ctx.data_ptr(), items, S, heads, st), e)
    for _ in range(3):
        for e in entries:
            call(e)
    torch.cuda.synchronize()
    us = {e: [] for e in entries}
    for _ in range(N):
        for e in entries:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call(e)
            b.record()
            b.synchronize()
            us[e].append(a.elapsed_time(b) * 1e3)
    flops = items * heads * 4.0 * S * S * 64            # QK^T and PV
    nbytes = items * heads * 4.0 * S * 64 * 2           # Q, K, V read once, the context written once
    for e in entries:
        t = statistics.median(us[e])
        print(f"{e:24s} items {items:5d} heads {heads} S {S:5d} {'masked' if masked else 'plain ':6s}: {t:9.1f} us median of {N} "
              f"(min {min(us[e]):.1f}, max {max(us[e]):.1f})  {flops / t / 1e6:7.1f} TF/s  {nbytes / t / 1e6:6.3f} TB/s of Q/K/V/ctx")


timed(["iisan_attention16"], 128, 577, 12, False)
timed(["iisan_attention16"], 128, 1024, 12, False)
timed(["iisan_attention16"], 128, 512, 12, True)
# what the streaming form costs where both exist: the ViT production shape
timed(["iisan_attention16", "iisan_attention16_long"], 1408, 197, 12, False)
