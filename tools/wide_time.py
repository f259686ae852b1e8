#!/usr/bin/env python3
"""One frozen tower at catalogue-building size, for a kernel trace (development aid; bench.py is the contract benchmark):

    rocprofv3 --kernel-trace --stats -d OUT -o trace -- python3 tools/wide_time.py --tower vit-large

runs `--iters` forwards of ViT-L/16, BERT-large, ViT-B/16 or BERT-base over `--items` slots with the taps of ALL hidden states (what
`evaluate.build_tap_cache` asks for), on random weights drawn on the device, and prints the wall time per forward.  The 768-wide towers
are there for the side-by-side of the row kernels: run them with IISAN_DEV_KNOBS=ln_fold=0 to put the ViT on the LayerNorm-image route
the 1024-wide towers always take."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from iisan_amd import _lib, encoders, weights  # noqa: E402

TOWERS = {"vit-large": weights.VIT_LARGE, "bert-large": weights.BERT_LARGE, "vit-base": weights.VIT_BASE, "bert-base": weights.BERT_BASE}


def device_weights(cfg, is_vit, seed=0):
    """The canonical weight dict of `iisan_amd.weights` with random values drawn on the device (a 24-layer tower is 300 M numbers)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    D, F = cfg.hidden, cfg.mlp
    mat = lambda *s: torch.randn(*s, device="cuda", generator=g) * 0.02
    gain = lambda: 1.0 + torch.randn(D, device="cuda", generator=g) * 0.05
    w = {}
    if is_vit:
        w.update(cls_token=mat(D), pos_emb=mat(cfg.tokens, D), patch_w=mat(D, cfg.patch_dim), patch_b=mat(D))
    else:
        w.update(word_emb=mat(cfg.vocab, D), pos_emb=mat(cfg.max_pos, D), type_emb=mat(2, D), emb_ln_w=gain(), emb_ln_b=mat(D))
    for l in range(cfg.layers):
        p = f"L{l}."
        w.update({p + "qkv_w": mat(3 * D, D), p + "qkv_b": mat(3 * D), p + "o_w": mat(D, D), p + "o_b": mat(D),
                  p + "fc1_w": mat(F, D), p + "fc1_b": mat(F), p + "fc2_w": mat(D, F), p + "fc2_b": mat(D),
                  p + "ln1_w": gain(), p + "ln1_b": mat(D), p + "ln2_w": gain(), p + "ln2_b": mat(D)})
    return w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tower", choices=sorted(TOWERS), default="vit-large")
    ap.add_argument("--items", type=int, default=1408)
    ap.add_argument("--iters", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dtype", default="fp16")
    ap.add_argument("--words", type=int, default=30)
    a = ap.parse_args()
    cfg, is_vit = TOWERS[a.tower], a.tower.startswith("vit")
    dt = encoders.DTYPE_NAMES[a.dtype]
    w = device_weights(cfg, is_vit)
    M = a.items
    if is_vit:
        tower = encoders.PackedVit(w, cfg, "cuda", dt)
        x = torch.randn(M, 3, cfg.image, cfg.image, device="cuda").clamp_(-1, 1)
        rows = M * cfg.tokens
    else:
        tower = encoders.PackedBert(w, cfg, "cuda", dt)
        x = torch.zeros(M, 2 * a.words, dtype=torch.int64, device="cuda")
        x[:, :a.words] = torch.randint(1000, cfg.vocab, (M, a.words), device="cuda")
        x[:, a.words:] = 1
        rows = M * a.words
    del w
    taps = list(range(cfg.layers + 1))
    for _ in range(a.warmup):
        out = tower.forward_taps(x, taps)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.iters):
        out = tower.forward_taps(x, taps)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / a.iters * 1e3
    assert torch.isfinite(out).all()
    print(f"{a.tower} ({a.dtype}): {ms:.2f} ms per forward of {M} items = {rows} token rows, {len(taps)} taps of width {cfg.hidden}, "
          f"{M / ms * 1e3:.0f} items/s; dev switches {_lib.dev_knobs()!r}")


if __name__ == "__main__":
    main()
