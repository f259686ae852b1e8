#!/usr/bin/env python3
"""The narrow towers (hidden 128 - 384) at catalogue-building size: what profiles/narrow_towers.md reports (development aid; bench.py is
the contract benchmark).  Three phases, each a process of its own under a kernel trace, and one report over their rocpd databases:

    rocprofv3 --kernel-trace --stats -d OUT/vit  -o t -- python3 tools/narrow_towers.py run --phase vit-tiny
    rocprofv3 --kernel-trace --stats -d OUT/bert -o t -- python3 tools/narrow_towers.py run --phase bert-tiny
    rocprofv3 --kernel-trace --stats -d OUT/prim -o t -- python3 tools/narrow_towers.py run --phase prims
    python3 tools/narrow_towers.py report OUT > OUT/narrow_towers.md

vit-tiny / bert-tiny: one warm-up and `--iters` forwards of the full `weights.VIT_TINY` / `weights.BERT_TINY` over `--items` slots, the taps
of ALL hidden states (what `evaluate.build_tap_cache` asks for), random weights drawn on the device; the wall time per forward is printed
(a host clock around work that ends in a synchronise) and the report sums the trace's kernel times per kernel family.
prims: (a) `iisan_layernorm` (layernorm768_kernel, 16-bit output) over the same number of rows at 128 / 192 / 256 / 384 / 768 / 1024; (b) a
2-layer ViT of width 192 / 384 / 768 on the LayerNorm-image route (ln_fold = 0), whose steady-state add + LayerNorm launches are
layernorm768_mixed_kernel at that width; (c) the 128x128 GEMM (gemm16_variant = 1) at N = 192 and N = 256, equal M and K.  The report turns
kernel times into bytes/s from the bytes the kernels must move, computed from the shapes here."""
import argparse
import glob
import json
import os
import re
import sqlite3
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WIDTHS = (128, 192, 256, 384, 768, 1024)
MX_BYTES = {15: ("x16 += dO + dF; LN (LN1)", 10), 5: ("LN(x16 + dO) (LN2)", 6)}      # bytes per element: fp16 stream / 16-bit deltas / 16-bit image


def _forward_phase(a, cfg, is_vit, tag):
    import torch
    from iisan_amd import _lib, encoders
    from tools.wide_time import device_weights
    M = a.items
    w = device_weights(cfg, is_vit)
    if is_vit:
        tower = encoders.PackedVit(w, cfg, "cuda", 0)
        x = torch.randn(M, 3, cfg.image, cfg.image, device="cuda").clamp_(-1, 1)
        T = cfg.tokens
    else:
        tower = encoders.PackedBert(w, cfg, "cuda", 0)
        x = torch.zeros(M, 2 * a.words, dtype=torch.int64, device="cuda")
        x[:, :a.words] = torch.randint(1000, cfg.vocab, (M, a.words), device="cuda")
        x[:, a.words:] = 1
        T = a.words
    taps = list(range(cfg.layers + 1))
    out = tower.forward_taps(x, taps)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.iters):
        out = tower.forward_taps(x, taps)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / a.iters * 1e3
    assert torch.isfinite(out).all()
    print(json.dumps({"phase": tag, "items": M, "tokens": T, "hidden": cfg.hidden, "layers": cfg.layers, "forwards_traced": a.iters + 1,
                      "wall_ms_per_forward": round(ms, 3), "items_per_s": round(M / ms * 1e3)}))


def _prims_phase(a):
    import torch
    from iisan_amd import _lib, encoders, weights
    from tools.wide_time import device_weights
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    rows = a.items * 197
    for D in WIDTHS:                                   # (a) the fp32 kernel: 4 bytes read, 2 written per element
        x = torch.randn(rows, D, device="cuda")
        g, b = torch.ones(D, device="cuda"), torch.zeros(D, device="cuda")
        o = torch.empty(rows, D, dtype=torch.float16, device="cuda")
        for _ in range(a.reps + 1):
            _lib.check(lib.iisan_layernorm(0, x.data_ptr(), g.data_ptr(), b.data_ptr(), 1e-12, o.data_ptr(), None, rows, D, s), "layernorm")
        torch.cuda.synchronize()
        del x, o
    for D in (192, 384, 768):                          # (b) the mixed kernel on the LayerNorm-image route
        cfg = weights.VitConfig(hidden=D, layers=2, heads=D // 64, mlp=4 * D)
        tower = encoders.PackedVit(device_weights(cfg, True), cfg, "cuda", 0)
        x = torch.randn(a.items, 3, 224, 224, device="cuda").clamp_(-1, 1)
        with _lib.dev(ln_fold=0, full_blocks=1):
            for _ in range(2):
                tower.forward_taps(x, [0, 1, 2])
        torch.cuda.synchronize()
        del tower, x
    M, K = rows, 192                                   # (c) ragged against whole last column tile
    Mp = (M + 255) // 256 * 256
    A = (torch.randn(Mp, K, device="cuda") * 0.5).half()
    for N in (192, 256):
        W = (torch.randn(N, K, device="cuda") * 0.05).half()
        bias = torch.randn(N, device="cuda")
        out = torch.empty(M, N, dtype=torch.float16, device="cuda")
        with _lib.dev(gemm16_variant=1):
            for _ in range(a.reps + 1):
                _lib.check(lib.iisan_gemm16(0, 0, A.data_ptr(), W.data_ptr(), bias.data_ptr(), out.data_ptr(), None, M, N, K, s), "gemm16")
        torch.cuda.synchronize()
    print(json.dumps({"phase": "prims", "rows": rows, "items": a.items, "tokens": 197, "reps": a.reps + 1, "gemm": {"M": M, "K": K}}))


def _kernels(out_dir, phase):
    dbs = glob.glob(os.path.join(out_dir, phase, "**", "*.db"), recursive=True)
    if not dbs:
        return None
    return sqlite3.connect(dbs[0]).execute("select name, grid_x, duration from kernels order by start").fetchall()


def _family(name):
    for pat, fam in (("gemm16", "GEMM (gemm16_*)"), ("attention", "attention"), ("layernorm768_mixed", "add + LayerNorm (mixed stream)"),
                     ("layernorm768", "LayerNorm (fp32 rows)"), ("bert_embed", "BERT embedding + LayerNorm"), ("im2col", "patch extraction"),
                     ("gather", "CLS gathers"), ("vit_cls_rows", "CLS gathers")):
        if pat in name:
            return fam
    return None             # torch's own kernels: the random weights and inputs of the set-up, not the forward


def _ragged_name(name):          # gemm16_kernel<T, EPI, true> — mangled (Lb1E) or demangled
    tail = name.split("gemm16_kernel", 1)[1]
    return "Lb1E" in tail or "true" in tail


def _meta(out_dir, phase):
    try:
        for line in open(os.path.join(out_dir, phase + ".log")):
            if line.startswith("{"):
                return json.loads(line)
    except OSError:
        pass
    return None


def report(out_dir):
    print("## Measured on the MI355X (tools/narrow_towers.py)\n")
    for phase, title in (("vit-tiny", "ViT-tiny (192 / 12 layers / 3 heads / mlp 768, 197 tokens)"), ("bert-tiny", "BERT-tiny (128 / 2 layers / 2 heads / mlp 512, 30 words)")):
        rows, meta = _kernels(out_dir, phase), _meta(out_dir, phase)
        if rows is None or meta is None:
            print(f"### {title}\n\nnot measured\n")
            continue
        n = meta["forwards_traced"]
        agg = {}
        for name, _, dur in rows:
            if _family(name) is None:
                continue
            a = agg.setdefault(_family(name), [0, 0]); a[0] += 1; a[1] += dur
        tot = sum(v[1] for v in agg.values())
        print(f"### {title}: one forward over {meta['items']} slots, all {meta['layers'] + 1} taps\n")
        print(f"Wall time per forward (host clock around a synchronise, in the traced process: tracing slows the host, an upper bound): {meta['wall_ms_per_forward']} ms = "
              f"{meta['items_per_s']} items/s.  Kernel time per forward (trace, {n} forwards averaged): {tot / n / 1e6:.3f} ms.\n")
        print("| kernel family | launches per forward | kernel ms per forward | share |\n|---|---|---|---|")
        for fam, (c, d) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
            print(f"| {fam} | {c / n:.0f} | {d / n / 1e6:.3f} | {100 * d / tot:.1f}% |")
        print()
    rows, meta = _kernels(out_dir, "prims"), _meta(out_dir, "prims")
    if rows is None or meta is None:
        print("### Row kernels and the ragged GEMM tile\n\nnot measured\n")
        return
    R = meta["rows"]
    print(f"### Row kernels: achieved bytes/s by width, {R} rows per launch\n")
    print("Bytes = what the kernel must move (fp32 kernel: 4 read + 2 written per element; mixed kernel: fp16 stream, 16-bit deltas and image), over the "
          "trace's kernel time; first launch of each kernel dropped.\n")
    print("| kernel | width | lanes x pieces per row | operand set | launches | avg us | TB/s |\n|---|---|---|---|---|---|---|")
    byk = {}
    for name, gx, dur in rows:
        byk.setdefault(name, []).append(dur)
    lay32 = {128: "32 x 1", 192: "16 x 3", 256: "64 x 1", 384: "32 x 3", 768: "64 x 3", 1024: "64 x 4"}
    laymx = {128: "16 x 1", 192: "8 x 3", 256: "32 x 1", 384: "16 x 3", 768: "32 x 3", 1024: "32 x 4"}
    lines = []
    for name, durs in byk.items():
        m = re.search(r"layernorm768(_mixed)?_kernel(?:I3F16Li(\d+)ELi(\d+)E|<\s*F16,\s*(\d+),\s*(\d+))", name)       # mangled or demangled
        if not m:
            continue
        mixed, V, D = bool(m.group(1)), int(m.group(2) or m.group(4)), int(m.group(3) or m.group(5))
        if mixed and V not in MX_BYTES:
            continue
        if not mixed and len(durs) < 3:                 # (the CLS-block launches of the phase-(b) towers: a handful of rows)
            continue
        durs = durs[1:] if len(durs) > 1 else durs
        what, bpe = MX_BYTES[V] if mixed else ("LN(x) -> 16-bit image", 6)
        avg = sum(durs) / len(durs)
        lines.append((mixed, D, V, f"| `layernorm768{'_mixed' if mixed else ''}_kernel` | {D} | {(laymx if mixed else lay32)[D]} | {what} | {len(durs)} | {avg / 1e3:.1f} | "
                                  f"{R * D * bpe / avg / 1e3:.2f} |"))
    for _, _, _, l in sorted(lines):
        print(l)
    print(f"\n### The ragged last column tile: N = 192 against N = 256, M = {meta['gemm']['M']}, K = {meta['gemm']['K']}, 128x128 kernel\n")
    print("| N | column tiles | launches | avg us (min - max) | TFLOP/s (useful) |\n|---|---|---|---|---|")
    tm = (meta["gemm"]["M"] + 127) // 128
    for N in (192, 256):
        # (grid_x of the trace counts threads; the towers of phase (b) launch the same shapes earlier: the last `reps` launches are phase (c)'s)
        durs = [d for name, gx, d in rows if "gemm16_kernel" in name and gx == tm * ((N + 127) // 128) * 256 and _ragged_name(name) == (N == 192)]
        durs = durs[-meta["reps"]:][1:]
        if not durs:
            print(f"| {N} | not measured | | | |")
            continue
        avg = sum(durs) / len(durs)
        print(f"| {N} | {(N + 127) // 128} ({'last one half dead' if N % 128 else 'whole'}) | {len(durs)} | {avg / 1e3:.1f} ({min(durs) / 1e3:.1f} - {max(durs) / 1e3:.1f}) | {2.0 * meta['gemm']['M'] * N * meta['gemm']['K'] / avg / 1e3:.1f} |")
    print()


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--phase", choices=("vit-tiny", "bert-tiny", "prims"), required=True)
    r.add_argument("--items", type=int, default=1408)
    r.add_argument("--iters", type=int, default=2)
    r.add_argument("--reps", type=int, default=5)
    r.add_argument("--words", type=int, default=30)
    p = sub.add_parser("report")
    p.add_argument("out_dir")
    a = ap.parse_args()
    if a.cmd == "report":
        return report(a.out_dir)
    from iisan_amd import weights
    if a.phase == "vit-tiny":
        _forward_phase(a, weights.VIT_TINY, True, a.phase)
    elif a.phase == "bert-tiny":
        _forward_phase(a, weights.BERT_TINY, False, a.phase)
    else:
        _prims_phase(a)


if __name__ == "__main__":
    main()
