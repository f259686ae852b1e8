#!/usr/bin/env python3
"""Timings that go with the CLIP vision tower (profiles/clip_tower.md): the FC1 product under the erf-GELU (mode 1) and the quick-GELU
(mode 8) epilogue, and one CLIP-B/32 tower forward at 1,408 item slots.

    python3 tools/clip_time.py [rounds]

FC1: M rows x 3072 x 768, fp16, default dispatch (gemm16_h256), row-major and block-major output, at M = 277,376 (ViT-B/16: 1,408 x 197
tokens) and M = 70,400 (CLIP-B/32: 1,408 x 50).  The two modes alternate inside every round — same operands, same process — and each
sample is device-event time over 20 launches after a warm-up; the table gives the median over the rounds and the spread (min .. max).
tools/gemm_time.py sweeps the kernel variants of ONE mode and needs a -DGEMM16_DEBUG_BITS build for its ablation columns; this tool
compares two modes of the product build.  Tower: all 13 taps of CLIP-B/32 (12 layers, 50 tokens), fp16 and bf16, uint8 input, default
dead-work policy and full_blocks = 1; device-event time per call over 5 calls after a warm-up."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from iisan_amd import _lib, encoders, weights  # noqa: E402


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


def fc1(rounds):
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    N, K = 3072, 768
    for M in (277376, 70400):
        Mp = (M + 255) // 256 * 256
        A = (torch.randn(Mp, K, device="cuda") * 0.5).half()
        W = (torch.randn(N, K, device="cuda") * 0.05).half()
        b = torch.randn(N, device="cuda")
        out = torch.empty(Mp, N, device="cuda", dtype=torch.float16)
        assert lib.iisan_gemm16_route(0, 8, M, N, K, 0, 0, 0, 0) == 2 == lib.iisan_gemm16_route(0, 1, M, N, K, 0, 0, 0, 0)
        for blk in (0, 1):
            call = lambda mode: _lib.check(lib.iisan_gemm16_blk32(0, mode, A.data_ptr(), W.data_ptr(), b.data_ptr(), out.data_ptr(), None,
                                                                  M, N, K, 0, blk, st), "gemm16_blk32")
            ms = {1: [], 8: []}
            for _ in range(rounds):
                for mode in (1, 8):
                    ms[mode].append(timed(lambda: call(mode), 20))
            for mode in (1, 8):
                med = statistics.median(ms[mode])
                print(f"FC1 M={M} N={N} K={K} {'block-major' if blk else 'row-major'} out, mode {mode}: median {med:.4f} ms "
                      f"({min(ms[mode]):.4f} .. {max(ms[mode]):.4f}), {2.0 * M * N * K / med / 1e9:.0f} TFLOP/s", flush=True)


def tower():
    cfg = weights.CLIP_VIT_B32
    w = weights.make_vit_weights(cfg, seed=51)
    g = torch.Generator(device="cuda").manual_seed(5)
    img = torch.randint(0, 256, (1408, 3, cfg.image, cfg.image), generator=g, dtype=torch.uint8, device="cuda")
    layers = list(range(cfg.layers + 1))
    for dt, name in ((_lib.IISAN_F16, "fp16"), (_lib.IISAN_BF16, "bf16")):
        pk = encoders.PackedVit(w, cfg, "cuda", dt)
        for fb in (False, True):
            pk.full_blocks = fb
            for c in ("gemm16_h256", "gemm16_blk32", "gemm16_v1"):
                _lib.dev_set("count:" + c, 0)
            ms = timed(lambda: pk.forward_taps(img, layers), 5)
            cnt = {c: _lib.dev_get("count:" + c) // 6 for c in ("gemm16_h256", "gemm16_blk32", "gemm16_v1")}
            print(f"CLIP-B/32 tower, 1408 slots, 13 taps, {name}, full_blocks={int(fb)}: {ms:.2f} ms per call; GEMM launches per call {cnt}", flush=True)
        del pk


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("clip_time.py measures on the GPU: no device visible")
    fc1(int(sys.argv[1]) if len(sys.argv) > 1 else 5)
    tower()
