#!/usr/bin/env python3
"""The measured figures behind tests/test_gpu_tower_plan_ladder.py, assertion E: for every case of that file, per tap (1, 2), the relative
Frobenius error of the plan under test over the compared slots, its worst per-slot error, and the worst per-slot error of the route the golden
fixtures pin to the reference (gemm16_variant = 1, chunk_items = 8) on the SAME slots against the SAME float64 oracle.

    python3 tools/tower_plan_ladder.py              prints the table of profiles/tower_plan_ladder.md and the SLOT_TOL literal (2 x the last figure)
    python3 tools/tower_plan_ladder.py deb clip     ... for the cases whose names start with one of the given prefixes only

The cases of all four tower families (ViT, BERT, CLIP, DeBERTa) are measured the same way: the pinned route is set here and nowhere else.

Reads the cases, inputs and oracle from the test module, so the two cannot drift apart."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_tower_plan_ladder as L  # noqa: E402
from iisan_amd import _lib, encoders  # noqa: E402


def main():
    assert torch.cuda.is_available(), "tower_plan_ladder: needs the GPU"
    _lib.load()
    rows, tol = [], []
    prefixes = tuple(sys.argv[1:])
    for case in [c for c in L.CASES if not prefixes or c.name.startswith(prefixes)]:
        rec, _, _ = L._record(case)
        x, _, subset = L._inputs(case)
        per_slot, per_tap = L.slot_errors(rec.t_sub, rec.o)
        enc = L._packed(case.tower, case.dt)
        enc.ws = encoders._Workspace()
        enc.full_blocks = bool(case.full)
        try:
            with _lib.dev(gemm16_variant=1):
                pinned = enc.forward_taps(x[subset].contiguous().cuda(), L.TAPS, chunk_items=8).cpu()
        finally:
            enc.full_blocks = False
            enc.ws = encoders._Workspace()
        pin_slot, pin_tap = L.slot_errors(pinned, rec.o)
        w, p = per_slot.max(0).values, pin_slot.max(0).values
        rows.append(f"| {case.name} | {case.plan} | {len(subset)} | {per_tap[0]:.2e} | " +
                    " | ".join(f"{per_tap[l]:.3e} | {w[l]:.3e} | {pin_tap[l]:.3e} | {p[l]:.3e}" for l in (1, 2)) + " |")
        tol.append(f'    "{case.name}": ({2 * p[1].item():.3e}, {2 * p[2].item():.3e}),')
        print(rows[-1], flush=True)
    print("\n| case | plan | slots | tap 0 | tap 1: per tap | worst slot | pinned per tap | pinned worst slot | tap 2: per tap | worst slot | pinned per tap "
          "| pinned worst slot |\n|" + "---|" * 12)
    print("\n".join(rows))
    print("\nSLOT_TOL = {\n" + "\n".join(tol) + "\n}")
    c = L._record(L.BY_NAME[L.CONTROL])[0]
    print("control: relative distance of the last two compared slots' tap 2:",
          ((c.t_sub[-1, 2] - c.t_sub[-2, 2]).norm() / c.t_sub[-1, 2].norm()).item())


if __name__ == "__main__":
    main()
