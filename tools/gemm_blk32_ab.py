"""Isolated A/B of the block-major ("blk32") intermediates at the bench shapes, fp16: level 1 = F1 (FC1 writes it, FC2 reads
it), level 2 = the ViT stream as well (FC1 reads it, O and FC2 read-modify-write it).  ViT: M = 277,376, FC1 with LayerNorm in the
epilogue, O / FC2 adding into the fp16 stream; BERT: M = 42,240, plain FC1 / FC2 / O (O has no block-major operand there: the control).
The layouts alternate in ONE process, `--rounds` interleaved rounds of `--launches` launches under HIP events; prints median and min-max
of the per-round means and whether a level's median lies below the row-major minimum (the keep rule of profiles/blk32_layout.md).

    python tools/gemm_blk32_ab.py [--lib path/to/libiisan_hip.so] [--rounds 5] [--launches 40]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from iisan_amd import _lib  # noqa: E402

D, F, S = 768, 3072, 197


def timed(call, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches          # us per launch


def ab(name, calls, rounds, launches, flops):
    """calls: [(label, callable)]; the labels alternate inside every round (round 0 = warm-up, not reported)"""
    t = {label: [] for label, _ in calls}
    for r in range(rounds + 1):
        for label, call in calls:
            us = timed(call, launches)
            if r:
                t[label].append(us)
    base = t[calls[0][0]]
    for label, _ in calls:
        v = t[label]
        med = statistics.median(v)
        verdict = "" if v is base else ("   GAINS" if med < min(base) else "   no gain")
        print(f"{name:22s} {label:10s} median {med:8.1f} us ({flops / med * 1e-6:6.0f} TFLOP/s)   min-max {min(v):8.1f} - {max(v):8.1f}{verdict}", flush=True)
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
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(1)
    W1 = (torch.randn(F, D, device="cuda", generator=g) * 0.03).half()
    W2 = (torch.randn(D, F, device="cuda", generator=g) * 0.01).half()
    Wo = (torch.randn(D, D, device="cuda", generator=g) * 0.02).half()
    b1, b2 = torch.randn(F, device="cuda", generator=g) * 0.1, torch.randn(D, device="cuda", generator=g) * 0.02

    def chk(rc):
        _lib.check(rc, "gemm16")

    for tower, M in (("ViT", 1408 * S), ("BERT", 1408 * 30)):
        Mp = (M + 255) // 256 * 256
        x = torch.zeros(Mp, D, dtype=torch.float16, device="cuda")
        x[:M] = torch.randn(M, D, device="cuda", generator=g).half()
        rstd = torch.rand(Mp, device="cuda", generator=g) * 0.5 + 0.75
        F1 = torch.zeros(Mp, F, dtype=torch.float16, device="cuda")
        # FC2 reads F1 as FC1 left it: a real GELU image, in the layout under test (written once per layout, outside the timed loops)
        F1b = torch.zeros(Mp, F, dtype=torch.float16, device="cuda")
        out = torch.zeros(Mp, D, dtype=torch.float16, device="cuda")
        part = torch.zeros(D // 64, Mp, 2, device="cuda")
        rs = rstd.data_ptr() if tower == "ViT" else None
        vit = tower == "ViT"
        # (the block-major A of level 2 is the same bytes read in another order: timing only)
        fc1 = lambda ablk, oblk, dst: chk(lib.iisan_gemm16_blk32(0, 1, x.data_ptr(), W1.data_ptr(), b1.data_ptr(), dst.data_ptr(), rs, M, F, D, ablk, oblk, st))
        calls = [("row-major", lambda: fc1(0, 0, F1)), ("level 1", lambda: fc1(0, 1, F1b))] + ([("level 2", lambda: fc1(1, 1, F1b))] if vit else [])
        ab(f"{tower} FC1 M={M}", calls, a.rounds, a.launches, 2.0 * M * F * D)
        if vit:
            fc2 = lambda ablk, xblk, src: chk(lib.iisan_gemm16_stream_blk32(src.data_ptr(), W2.data_ptr(), b2.data_ptr(), out.data_ptr(), part.data_ptr(), M, D, F, S, ablk, xblk, st))
            calls = [("row-major", lambda: fc2(0, 0, F1)), ("level 1", lambda: fc2(1, 0, F1b)), ("level 2", lambda: fc2(1, 1, F1b))]
            o = lambda xblk: chk(lib.iisan_gemm16_stream_blk32(x.data_ptr(), Wo.data_ptr(), b2.data_ptr(), out.data_ptr(), part.data_ptr(), M, D, D, S, 0, xblk, st))
            ocalls = [("row-major", lambda: o(0)), ("level 2", lambda: o(1))]
        else:
            fc2 = lambda ablk, src: chk(lib.iisan_gemm16_blk32(0, 0, src.data_ptr(), W2.data_ptr(), b2.data_ptr(), out.data_ptr(), None, M, D, F, ablk, 0, st))
            calls = [("row-major", lambda: fc2(0, F1)), ("level 1", lambda: fc2(1, F1b))]
            o = lambda: chk(lib.iisan_gemm16_blk32(0, 0, x.data_ptr(), Wo.data_ptr(), b2.data_ptr(), out.data_ptr(), None, M, D, D, 0, 0, st))
            ocalls = [("row-major", o), ("same", o)]          # control: the same launch under both labels
        ab(f"{tower} FC2 M={M}", calls, a.rounds, a.launches, 2.0 * M * D * F)
        ab(f"{tower} O M={M}", ocalls, a.rounds, a.launches, 2.0 * M * D * D)
        del x, F1, F1b, out, part
    print("dev switches:", _lib.dev_knobs() or "(defaults)")


if __name__ == "__main__":
    main()
