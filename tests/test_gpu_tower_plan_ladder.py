"""The frozen towers on every plan the library defaults reach, slot by slot.

At the defaults the plan of an encoder call (encoders.hip: vit_plan / bert_plan) is a function of the batch size alone; the ladders and their
derivation are pinned in tests/test_tower_plan_ladder_host.py.  This file runs ONE case per ladder step (the 197-token ladder: both ends
of each step) with no development switch set — every case first asserts its plan string through `iisan_encoder_plan` and
`_lib.dev_state() == ""`, so a case that silently ran another route fails — and checks what `model.forward_item3(item_ids=...)`,
`forward_item3_indexed(dedup=True)` and the grow-only workspace rely on:

  A  duplicates     the content of one item planted into slot 1, the last slot and the slots either side of every 256-row tile boundary and
                    32-row block boundary of the first and the last tile: all copies carry identical taps (bitwise)
  B  permutation    taps(x[perm]) == taps(x)[perm] (bitwise)
  C  composition    a same-plan sub-batch (the first M - 40 items; where M - 40 lies below the case's step or does not exist — 22 of the
                    35 cases — the step's first M or half the batch, and where the case IS the step's first M, the case inside M + 5
                    items: profiles/tower_plan_ladder.md) gives the same bits;
                    the chunked call equals the unchunked one; the indexed entry equals the materialised call
  D  stale scratch  the workspace filled with 0x00, 0xFF (NaN in fp16 / bf16 / fp32) and 0x7B (61,280 in fp16, 1.3e36 in bf16 / fp32: finite,
                    but every sum over it overflows) gives the same, finite bits, and so does the case after a larger call on the same
                    packed tower (`_Workspace` is grow-only).  The poison changes DATA only: every pointer and size is the ordinary call's
  E  oracle         at most 24 slots (slot 0, the last, the duplicates, the tile-boundary neighbours, seeded others) against the float64
                    oracle run on those slots alone (rows are independent in the reference): per tap the relative Frobenius error within
                    TAP_TOL of tests/test_gpu_long_towers.py, and PER SLOT within SLOT_TOL = 2 x the worst per-slot error the route the golden
                    fixtures pin (gemm16_variant = 1, chunk_items = 8) leaves on the same slots — two correct fp16 routes decorrelate to
                    about sqrt(2) of one route's noise, and 2 x leaves room for the fold route's second weight rounding.  Measured by
                    tools/tower_plan_ladder.py, recorded per case and tap in profiles/tower_plan_ladder.md.

Same seeded 2-layer towers and taps [0, 1, 2] as the other encoder tests; what varies is batch size, slot position and what lies behind the
live rows.  Negative controls at the end show that each comparison can fail.

Four tower families run here: the plain ViT and BERT towers, the CLIP vision towers (the ViT executor behind a pre-LayerNorm, quick-GELU, no
patch bias: oracle tests/clip_oracle.py) and the DeBERTa-v2/v3 text towers (the BERT executor with the masked-LayerNorm embedding step and
the disentangled attention kernel: oracle tests/deberta_oracle.py).  The CLIP-L/14 case at its real 257 tokens compares 8 slots in E, not
24 — slot 0, the last slot, the planted item and its tile-boundary duplicates come first in the subset, so these stay — which keeps the
float64 oracle of 257 x 1024-wide tokens per slot to seconds on the CPU."""
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import clip_oracle as CO  # noqa: E402
import deberta_oracle as DO  # noqa: E402
from iisan_amd import _lib, encoders, synth, weights  # noqa: E402
from oracle import iisan_oracle as O  # noqa: E402
from test_tower_plan_ladder_host import BERT, CLIP, DEBERTA, VIT, plan_code  # noqa: E402

TAPS = [0, 1, 2]
TAP_TOL = {_lib.IISAN_F16: 1.5e-3, _lib.IISAN_BF16: 1.2e-2}      # relative Frobenius error per tap (tests/test_gpu_long_towers.py)
TAP0_VIT, TAP0_BERT = 1e-6, 1e-5                                  # tap 0: no 16-bit arithmetic on the CLS row / fp32 gather + LayerNorm
TAP0 = {VIT: TAP0_VIT, BERT: TAP0_BERT, CLIP: 1e-5, DEBERTA: 1e-5}  # CLIP: the pre-LayerNorm of the CLS row; DeBERTa: LayerNorm(word row) * mask
F16, BF16 = _lib.IISAN_F16, _lib.IISAN_BF16
SRC = 2                 # the item whose content is planted
OTHERS = 2203           # items of the larger call of the grow-only sequence
POISON = (0x00, 0xFF, 0x7B)

_CLIP = dict(eps=1e-5, pre_ln=True, act="quick_gelu", patch_bias=False)
TOWERS = {
    "vit5": weights.VitConfig(hidden=768, layers=2, heads=12, mlp=3072, image=32, patch=16),
    "vit10": weights.VitConfig(hidden=768, layers=2, heads=12, mlp=3072, image=48, patch=16),
    "vit197": weights.VitConfig(hidden=768, layers=2, heads=12, mlp=3072, image=224, patch=16),
    "vit5w": weights.VitConfig(hidden=1024, layers=2, heads=16, mlp=4096, image=32, patch=16),
    "vit5n": weights.VitConfig(hidden=192, layers=2, heads=3, mlp=768, image=32, patch=16),
    "bert30": weights.BertConfig(hidden=768, layers=2, heads=12, mlp=3072, vocab=512, max_pos=64),
    "bert8n": weights.BertConfig(hidden=128, layers=2, heads=2, mlp=512, vocab=512, max_pos=64),
    "deb30": weights.DebertaConfig(hidden=768, layers=2, heads=12, mlp=3072, vocab=DO.VOCAB, position_buckets=256),
    "deb128": weights.DebertaConfig(hidden=768, layers=2, heads=12, mlp=3072, vocab=DO.VOCAB, position_buckets=256),
    "debL30": weights.DebertaConfig(hidden=1024, layers=2, heads=16, mlp=4096, vocab=DO.VOCAB, position_buckets=256),
    "debX30": weights.DebertaConfig(hidden=384, layers=2, heads=6, mlp=1536, vocab=DO.VOCAB, position_buckets=256),
    "clip5": weights.VitConfig(hidden=768, layers=2, heads=12, mlp=3072, image=32, patch=16, **_CLIP),
    "clip50": weights.VitConfig(hidden=768, layers=2, heads=12, mlp=3072, image=224, patch=32, **_CLIP),           # B/32 at 224 px
    "clipL5": weights.VitConfig(hidden=1024, layers=2, heads=16, mlp=4096, image=28, patch=14, **_CLIP),
    "clipL257": weights.VitConfig(hidden=1024, layers=2, heads=16, mlp=4096, image=224, patch=14, **_CLIP),        # L/14 at 224 px
}
WORDS = {"bert30": 30, "bert8n": 8, "deb30": 30, "deb128": 128, "debL30": 30, "debX30": 30}
# weight and pool seeds: the seven towers of the first twenty cases keep theirs (80 + their rank by name), the later towers follow
SEEDS = {name: 80 + i for i, name in enumerate(["bert30", "bert8n", "vit10", "vit197", "vit5", "vit5n", "vit5w",
                                                "deb30", "deb128", "debL30", "debX30", "clip5", "clip50", "clipL5", "clipL257"])}

Case = namedtuple("Case", "name tower dt M plan chunk full", defaults=(0, 0))
CASES = [
    Case("vit5-1075", "vit5", F16, 1075, "I"),
    Case("vit5-2150", "vit5", F16, 2150, "F"),
    Case("vit5-2203", "vit5", F16, 2203, "Sfx"),            # 11,015 rows = 43 tiles + 7 rows, and a ragged 32-row block
    Case("vit5-full-2203", "vit5", F16, 2203, "Sfx", 0, 1),
    Case("vit5-full-720", "vit5", F16, 720, "F", 0, 1),     # no K/V product: F from 717
    Case("vit10-1077", "vit10", F16, 1077, "Sfx"),
    Case("vit197-27", "vit197", F16, 27, "I"),
    Case("vit197-28", "vit197", F16, 28, "F"),
    Case("vit197-54", "vit197", F16, 54, "F"),
    Case("vit197-55", "vit197", F16, 55, "Sfx"),
    Case("vit5-bf16-2203", "vit5", BF16, 2203, "If"),
    Case("vit5w-1603", "vit5w", F16, 1603, "If"),
    Case("bert30-358", "bert30", F16, 358, "Ma"),
    Case("bert30-367", "bert30", F16, 367, "Maf"),
    Case("bert30-bf16-367", "bert30", BF16, 367, "Mf"),
    Case("vit5-chunk-4363", "vit5", F16, 4363, "Sfx", 2200),
    Case("vit5-chunk-3300", "vit5", F16, 3300, "F", 2200),
    Case("vit5-chunk-2300", "vit5", F16, 2300, "I", 2200),
    Case("vit5n-37", "vit5n", F16, 37, "I"),                # the narrow towers: row kernels that share a wave between rows, odd row counts
    Case("bert8n-37", "bert8n", F16, 37, "Ma"),
    Case("deb30-358", "deb30", F16, 358, "Ma"),             # 10,740 rows of the masked-LayerNorm embedding step, every product on 128x128
    Case("deb30-367", "deb30", F16, 367, "Maf"),            # head-major QKV of gemm16_h256 into the disentangled kernel, block-major F1
    Case("deb30-bf16-367", "deb30", BF16, 367, "Mf"),
    Case("deb128-85", "deb128", F16, 85, "Maf"),            # the 128-word instantiation: one workgroup per CU
    Case("debL30-265", "debL30", F16, 265, "Maf"),
    Case("debX30-367", "debX30", F16, 367, "Ma"),           # N % 256 != 0: never f
    Case("deb30-chunk-759", "deb30", F16, 759, "Maf", 400), # the tables projected once, read by both chunks
    Case("clip5-2150", "clip5", F16, 2150, "I"),
    Case("clip5-2203", "clip5", F16, 2203, "If"),
    Case("clip5-full-2203", "clip5", F16, 2203, "If", 0, 1),
    Case("clip5-bf16-2203", "clip5", BF16, 2203, "If"),
    Case("clip50-216", "clip50", F16, 216, "If"),
    Case("clipL5-1603", "clipL5", F16, 1603, "If"),         # 14-pixel patches: the padded patch matrix
    Case("clipL257-31", "clipL257", F16, 31, "If"),         # streaming-softmax attention, 14-pixel patches, quick-GELU on gemm16_h256 at once
    Case("clip5-chunk-4363", "clip5", F16, 4363, "If", 2200),
]
SUBSET = {"clipL257-31": 8}     # slots E compares where it is not 24 (module docstring)
BY_NAME = {c.name: c for c in CASES}
CONTROL = "vit5-2203"           # the Sfx case whose recorded taps the negative controls and the indexed entry use

# E, per slot and tap (1, 2): 2 x the worst per-slot relative error of the pinned 128x128 route on the same slots against the same oracle,
# as measured on an MI355X — profiles/tower_plan_ladder.md, written by tools/tower_plan_ladder.py
SLOT_TOL = {
    "vit5-1075": (1.624e-03, 1.716e-03),
    "vit5-2150": (1.685e-03, 1.810e-03),
    "vit5-2203": (1.611e-03, 1.681e-03),
    "vit5-full-2203": (1.611e-03, 1.681e-03),
    "vit5-full-720": (1.648e-03, 1.820e-03),
    "vit10-1077": (1.672e-03, 1.779e-03),
    "vit197-27": (1.279e-03, 1.443e-03),
    "vit197-28": (1.263e-03, 1.414e-03),
    "vit197-54": (1.295e-03, 1.443e-03),
    "vit197-55": (1.279e-03, 1.405e-03),
    "vit5-bf16-2203": (1.251e-02, 1.323e-02),
    "vit5w-1603": (1.687e-03, 1.885e-03),
    "bert30-358": (3.961e-04, 5.741e-04),
    "bert30-367": (4.086e-04, 5.741e-04),
    "bert30-bf16-367": (3.217e-03, 4.529e-03),
    "vit5-chunk-4363": (1.602e-03, 1.681e-03),
    "vit5-chunk-3300": (1.628e-03, 1.757e-03),
    "vit5-chunk-2300": (1.602e-03, 1.683e-03),
    "vit5n-37": (1.365e-03, 1.556e-03),
    "bert8n-37": (7.623e-05, 1.101e-04),
    "deb30-358": (6.153e-04, 7.396e-04),
    "deb30-367": (6.153e-04, 7.396e-04),
    "deb30-bf16-367": (4.758e-03, 5.914e-03),
    "deb128-85": (5.837e-04, 7.354e-04),
    "debL30-265": (6.183e-04, 8.439e-04),
    "debX30-367": (5.025e-04, 5.478e-04),
    "deb30-chunk-759": (6.153e-04, 7.396e-04),
    "clip5-2150": (3.832e-04, 5.350e-04),
    "clip5-2203": (3.931e-04, 5.289e-04),
    "clip5-full-2203": (3.931e-04, 5.289e-04),
    "clip5-bf16-2203": (3.188e-03, 4.170e-03),
    "clip50-216": (3.389e-04, 4.643e-04),
    "clipL5-1603": (5.035e-04, 6.901e-04),
    "clipL257-31": (4.405e-04, 5.949e-04),
    "clip5-chunk-4363": (4.033e-04, 5.292e-04),
}

_TOWER, _PACKED, _REC = {}, {}, {}


# ---- the comparisons -------------------------------------------------------------------------------------------------------------------

def check_dups(t, slots, what=""):
    """A: every slot that holds the planted content carries the same bits."""
    for s in slots[1:]:
        assert torch.equal(t[s], t[slots[0]]), f"{what}: slot {s} differs from slot {slots[0]}, which holds the same item"


def check_perm(t, t_perm, perm, what=""):
    """B."""
    assert torch.equal(t_perm, t[perm]), f"{what}: taps(x[perm]) != taps(x)[perm]"


def check_bits(a, b, what=""):
    """C, D."""
    assert a.shape == b.shape and torch.equal(a, b), f"{what}: {(a != b).any(-1).any(-1).sum().item()} slots differ"


def slot_errors(t, o):
    """[slots, taps] relative error per slot and tap, and the relative Frobenius error per tap."""
    d, o = (t.double() - o), o.double()
    return d.norm(dim=-1) / o.norm(dim=-1), d.norm(dim=(0, 2)) / o.norm(dim=(0, 2))


def check_oracle(t, o, dt, tap0, slot_tol, what=""):
    """E: per tap over the subset, then per slot.  Every figure is printed before it is asserted."""
    assert torch.isfinite(t).all(), what
    per_slot, per_tap = slot_errors(t, o)
    worst = per_slot.max(0).values
    print(f"{what}: per tap {[f'{e:.3e}' for e in per_tap.tolist()]} worst slot {[f'{e:.3e}' for e in worst.tolist()]}")
    bad = [f"tap 0: {per_tap[0]:.3e} >= {tap0:.0e}"] if not per_tap[0] < tap0 else []
    bad += [f"tap {l}: {per_tap[l]:.3e} >= {TAP_TOL[dt]:.1e}" for l in (1, 2) if not per_tap[l] < TAP_TOL[dt]]
    if slot_tol is None:
        bad.append("no measured per-slot bound")
    else:
        bad += [f"tap {l}: slot {per_slot[:, l].argmax().item()} of the subset is {worst[l]:.3e} off, bound {slot_tol[l - 1]:.3e}"
                for l in (1, 2) if not worst[l] <= slot_tol[l - 1]]
    assert not bad, f"{what}: " + "; ".join(bad)


# ---- towers and inputs ------------------------------------------------------------------------------------------------------------------

def _family(cfg):
    if isinstance(cfg, weights.VitConfig):
        return CLIP if cfg.pre_ln else VIT
    return DEBERTA if isinstance(cfg, weights.DebertaConfig) else BERT


def _is_vit(cfg):
    """An image tower (ViT or CLIP): image inputs, the ViT executor."""
    return _family(cfg) in (VIT, CLIP)


def _tokens(case):
    cfg = TOWERS[case.tower]
    return cfg.tokens if _is_vit(cfg) else WORDS[case.tower]


def _titles(n, W, vocab, seed):
    """[n, 2W]: titles of random length 0..W with a prefix mask; item 0 is the padding item (zero ids, all-zero mask)."""
    g = torch.Generator().manual_seed(seed)
    ln = torch.randint(0, W + 1, (n,), generator=g)
    ln[0], ln[SRC] = 0, W // 2 + 1
    keep = (torch.arange(W)[None] < ln[:, None]).long()
    return torch.cat([torch.randint(1, vocab, (n, W), generator=g) * keep, keep], 1)


def _tower(name):
    """Weights (fp32 and float64) and the pool of items every case of the tower draws its first M from: built once, never modified."""
    if name not in _TOWER:
        cfg = TOWERS[name]
        n = max(c.M for c in CASES if c.tower == name) + 5
        seed = SEEDS[name]
        if _is_vit(cfg):
            w = weights.make_vit_weights(cfg, seed=seed)
            pool = synth.make_images(np.arange(n), cfg.image, seed=seed)          # slot 0 (id 0) is the zero image
        else:
            w = (weights.make_deberta_weights if _family(cfg) == DEBERTA else weights.make_bert_weights)(cfg, seed=seed)
            pool = _titles(n, WORDS[name], cfg.vocab, seed)
        _TOWER[name] = SimpleNamespace(cfg=cfg, w=w, w64={k: v.double() for k, v in w.items()}, pool=pool)
    return _TOWER[name]


def _packed(name, dt):
    if (name, dt) not in _PACKED:
        tw = _tower(name)
        cls = encoders.PackedVit if _is_vit(tw.cfg) else encoders.PackedBert
        _PACKED[name, dt] = cls(tw.w, tw.cfg, "cuda", dt)
    return _PACKED[name, dt]


def _boundary_slots(M, T, chunk):
    """The slots that hold the token rows either side of the 256-row tile boundaries and 32-row block boundaries of the first and the last
    tile of the first and the last chunk (T = 5, one chunk: rows 31 / 32 and 255 / 256 of the first tile; the last row of the tile before the
    last one, and rows 0, 31 / 32 of the last).  `tile`: only those at the 256-row boundaries."""
    Mc = chunk if 0 < chunk < M else M
    block, tile = set(), set()
    for m0 in {0, (M - 1) // Mc * Mc}:
        tok = min(Mc, M - m0) * T
        for t0 in {0, (tok - 1) // 256 * 256}:
            for r, at_tile in ((t0 - 1, 1), (t0, t0 > 0), (t0 + 31, 0), (t0 + 32, 0), (t0 + 255, 1), (t0 + 256, 1)):
                if 0 <= r < tok:
                    block.add(m0 + r // T)
                    if at_tile:
                        tile.add(m0 + r // T)
    return block, tile


def _plan(case, M=None):
    cfg = TOWERS[case.tower]
    fam = _family(cfg)
    # the last argument: PackedVit supplies the folded set where the executor has the route; a CLIP tower has none; DeBERTa: the span
    last = {VIT: int(case.dt == F16 and cfg.hidden == 768), CLIP: 0, BERT: 0}.get(fam)
    if fam == DEBERTA:
        last = cfg.position_buckets
    got = _lib.load().iisan_encoder_plan(fam, case.dt, cfg.hidden, cfg.heads, cfg.mlp, _tokens(case), M or case.M, case.chunk, 2, case.full, last)
    return plan_code(fam, got)


def _inputs(case):
    """x [M, ...] on the CPU, the slots that hold the planted content (SRC first), and the subset E compares."""
    tw, M, T = _tower(case.tower), case.M, _tokens(case)
    x = tw.pool[:M].clone()
    block, tile = _boundary_slots(M, T, case.chunk)
    dups = sorted(({1, M - 1} | block) - {0, SRC})
    x[dups] = x[SRC].clone()
    if not _is_vit(tw.cfg):         # one full-length title, on a slot of its own
        W, full = WORDS[case.tower], next(s for s in range(3, M) if s not in dups)
        x[full, :W] = torch.randint(1, tw.cfg.vocab, (W,), generator=torch.Generator().manual_seed(M))
        x[full, W:] = 1
    assert x[0].abs().max() == 0
    near = sorted({s + d for s in tile for d in (-1, 1)} - set(dups) - {0, SRC})
    near = [s for s in near if 0 < s < M]
    g = torch.Generator().manual_seed(1000 + M)
    others = [s for s in torch.randperm(M, generator=g).tolist() if s not in (0, SRC, M - 1) and s not in dups and s not in near][:10]
    subset = list(dict.fromkeys([0, M - 1, SRC] + dups + near + others))[:SUBSET.get(case.name, 24)]
    return x, [SRC] + dups, subset


def _call(enc, xg, chunk=0):
    return enc.forward_taps(xg, TAPS, chunk_items=chunk).cpu()


def _other_items(case):
    """OTHERS items that are not the case's, for the larger call of the grow-only sequence (224-pixel images: raw pixels drawn on the device)."""
    cfg = TOWERS[case.tower]
    if not _is_vit(cfg):
        return _titles(OTHERS, WORDS[case.tower], cfg.vocab, 7).cuda()
    if cfg.image > 64:
        return torch.randint(0, 256, (OTHERS, 3, cfg.image, cfg.image), dtype=torch.uint8, device="cuda", generator=torch.Generator("cuda").manual_seed(7))
    return synth.make_images(np.arange(1, OTHERS + 1), cfg.image, seed=7).cuda()


def _oracle(case, x, subset):
    tw = _tower(case.tower)
    fam = _family(tw.cfg)
    with torch.no_grad():
        if fam == CLIP:
            return CO.clip_cls_taps(x[subset].double(), tw.w64, tw.cfg)
        if fam == DEBERTA:
            return DO.deberta_cls_taps(x[subset], tw.w64, tw.cfg)
        if fam == VIT:
            return O.vit_cls_taps(x[subset].double(), tw.w64, tw.cfg)
        return O.bert_cls_taps(x[subset], tw.w64, tw.cfg)


def _record(case):
    """The case's first call on a fresh workspace, its plan asserted first; kept for E and the controls (the subset's rows; all rows of CONTROL)."""
    if case.name not in _REC:
        assert _lib.dev_state() == ""
        assert _plan(case) == case.plan, (case.name, _plan(case))
        enc = _packed(case.tower, case.dt)
        x, dups, subset = _inputs(case)
        enc.ws = encoders._Workspace()
        enc.full_blocks = bool(case.full)
        try:
            t = _call(enc, x.cuda(), case.chunk)
        finally:
            enc.full_blocks = False
        assert t.shape == (case.M, 3, tw_hidden(case))
        _REC[case.name] = SimpleNamespace(t=t if case.name == CONTROL else None, t_sub=t[subset].clone(), dups=dups, subset=subset,
                                          o=_oracle(case, x, subset))
        return _REC[case.name], t, x
    return _REC[case.name], None, None


def tw_hidden(case):
    return TOWERS[case.tower].hidden


def _same_plan_sub_batch(case):
    """C: M - 40 (M <= 40: half the batch) where that is on the case's plan, else the first M of the case's step above it; M itself = the case
    is the first M of its step."""
    lo = case.M - 40 if case.M > 40 else case.M // 2
    return next(m for m in range(lo, case.M + 1) if _plan(case, m) == case.plan)


# ---- A - D -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(BY_NAME))
def test_slots_are_independent_of_position_batch_and_stale_workspace(lib, name):
    case = BY_NAME[name]
    rec, t, x = _record(case)
    if t is None:       # recorded by an earlier test of this process: the same call again
        x = _inputs(case)[0]
    enc = _packed(case.tower, case.dt)
    enc.ws = encoders._Workspace()
    enc.full_blocks = bool(case.full)
    try:
        xg = x.cuda()
        t0 = _call(enc, xg, case.chunk)
        if t is not None:
            check_bits(t0, t, f"{name}: the same call twice")
        t = t0
        assert torch.isfinite(t).all()
        check_dups(t, rec.dups, name)                                                                        # A
        perm = torch.randperm(case.M, generator=torch.Generator().manual_seed(case.M))
        t_perm = _call(enc, xg[perm.cuda()].contiguous(), case.chunk)
        check_perm(t, t_perm, perm, name)                                                                    # B
        if name == CONTROL:
            _REC[name].perm, _REC[name].t_perm = perm, t_perm
        sub = _same_plan_sub_batch(case)                                                                     # C
        if sub < case.M:
            assert _plan(case, sub) == case.plan
            check_bits(_call(enc, xg[:sub].contiguous(), case.chunk), t[:sub], f"{name}: the first {sub} items alone")
        else:
            assert _plan(case, case.M + 5) == case.plan
            more = torch.cat([xg, _tower(case.tower).pool[case.M:case.M + 5].cuda()])
            check_bits(_call(enc, more, case.chunk)[:case.M], t, f"{name}: inside {case.M + 5} items")
        need = enc.ws.buf.numel()                                                                            # D
        for byte in POISON:
            enc.ws.buf.fill_(byte)
            check_bits(_call(enc, xg, case.chunk), t, f"{name}: workspace filled with 0x{byte:02X}")
            assert enc.ws.buf.numel() == need
        other = _other_items(case)
        assert torch.isfinite(enc.forward_taps(other, TAPS)).all()
        del other
        assert enc.ws.buf.numel() >= need
        check_bits(_call(enc, xg, case.chunk), t, f"{name}: after a call with {OTHERS} other items on the same packed tower")
    finally:
        enc.full_blocks = False
        enc.ws = encoders._Workspace()


def test_chunked_call_equals_the_unchunked_one(lib):
    """C: 4,363 items in chunks of 2,200 (a 2,163-item last chunk) against the same items in one call, both on Sfx."""
    case = BY_NAME["vit5-chunk-4363"]
    assert _lib.dev_state() == ""
    assert _plan(case) == "Sfx" and _plan(case._replace(chunk=0)) == "Sfx"
    enc = _packed(case.tower, case.dt)
    enc.ws = encoders._Workspace()
    xg = _inputs(case)[0].cuda()
    try:
        check_bits(_call(enc, xg, case.chunk), _call(enc, xg, 0), "4,363 items: chunks of 2,200 against one call")
    finally:
        enc.ws = encoders._Workspace()


def test_indexed_entry_equals_the_materialised_call(lib):
    """C: `forward_taps_indexed` over a 64-row uint8 catalogue on Sfx: the index holds the planted duplicates and two out-of-range values
    (padding slots), the materialised call sees the same normalised pixels."""
    case = BY_NAME[CONTROL]
    assert _lib.dev_state() == ""
    assert _plan(case) == "Sfx"
    enc = _packed(case.tower, case.dt)
    enc.ws = encoders._Workspace()
    _, dups, _ = _inputs(case)
    g = torch.Generator().manual_seed(11)
    cat = torch.randint(0, 256, (64, 3, 32, 32), generator=g, dtype=torch.uint8)
    index = torch.randint(0, 64, (case.M,), generator=g)
    index[dups] = 7
    index[0], index[1000] = -1, 64 + 5
    pad = (index < 0) | (index >= 64)
    direct = ((cat.float().div(255) - 0.5) / 0.5)[index.clamp(0, 63)].clone()
    direct[pad] = 0
    try:
        want = _call(enc, direct.cuda())
        got = enc.forward_taps_indexed(cat.cuda(), index.cuda(), TAPS).cpu()
        check_bits(got, want, "indexed against materialised")
        check_dups(got, dups, "indexed")
        check_bits(got[1000], got[0], "the two padding slots")
    finally:
        enc.ws = encoders._Workspace()


def test_deberta_chunked_call_equals_the_unchunked_one(lib):
    """C: 759 titles in chunks of 400 (a 359-title last chunk) against the same titles in one call, both on Maf: every chunk reads the
    position tables that were projected once."""
    case = BY_NAME["deb30-chunk-759"]
    assert _lib.dev_state() == ""
    assert _plan(case) == "Maf" and _plan(case._replace(chunk=0)) == "Maf"
    enc = _packed(case.tower, case.dt)
    enc.ws = encoders._Workspace()
    xg = _inputs(case)[0].cuda()
    try:
        check_bits(_call(enc, xg, case.chunk), _call(enc, xg, 0), "759 titles: chunks of 400 against one call")
    finally:
        enc.ws = encoders._Workspace()


def test_deberta_indexed_entry_equals_the_materialised_call(lib):
    """C: `forward_taps_indexed` over a 64-row title table on Maf: the index holds the planted duplicates and two out-of-range values
    (padding slots: ids and mask zero), the materialised call sees the same rows."""
    case = BY_NAME["deb30-367"]
    assert _lib.dev_state() == ""
    assert _plan(case) == "Maf"
    enc = _packed(case.tower, case.dt)
    enc.ws = encoders._Workspace()
    _, dups, _ = _inputs(case)
    table = _titles(64, WORDS[case.tower], DO.VOCAB, 11)
    index = torch.randint(0, 64, (case.M,), generator=torch.Generator().manual_seed(11))
    index[dups] = 7
    index[0], index[300] = -1, 64 + 5
    assert 300 not in dups
    pad = (index < 0) | (index >= 64)
    direct = table[index.clamp(0, 63)].clone()
    direct[pad] = 0
    try:
        want = _call(enc, direct.cuda())
        got = enc.forward_taps_indexed(table.cuda(), index.cuda(), TAPS).cpu()
        check_bits(got, want, "indexed against materialised")
        check_dups(got, dups, "indexed")
        check_bits(got[300], got[0], "the two padding slots")
    finally:
        enc.ws = encoders._Workspace()


def test_deberta_tables_projected_by_the_call_give_the_same_bits(lib):
    """D: the Maf case on a `PackedDeberta(..., project_tables=False)`: the position tables live in the call's workspace and are projected
    on every call, behind the chunk buffers.  The same bits as the tower that projected them once, under all three poisons, and in chunks
    of 200 titles (200 + 167: both towers on Ma)."""
    case = BY_NAME["deb30-367"]
    assert _lib.dev_state() == ""
    assert _plan(case) == "Maf" and _plan(case._replace(chunk=200)) == "Ma"
    tw, enc = _tower(case.tower), _packed(case.tower, case.dt)
    own = encoders.PackedDeberta(tw.w, tw.cfg, "cuda", case.dt, project_tables=False)
    assert enc.struct.rel_proj and not own.struct.rel_proj
    enc.ws = encoders._Workspace()
    xg = _inputs(case)[0].cuda()
    try:
        want, want200 = _call(enc, xg), _call(enc, xg, 200)
        assert torch.isfinite(want).all() and torch.isfinite(want200).all()
        check_bits(_call(own, xg), want, "tables projected by the call")
        need = own.ws.buf.numel()
        assert need > enc.ws.buf.numel()
        for byte in POISON:
            own.ws.buf.fill_(byte)
            check_bits(_call(own, xg), want, f"tables projected by the call: workspace filled with 0x{byte:02X}")
            own.ws.buf.fill_(byte)
            check_bits(_call(own, xg, 200), want200, f"tables projected by the call, chunks of 200: workspace filled with 0x{byte:02X}")
            assert own.ws.buf.numel() == need
    finally:
        enc.ws = encoders._Workspace()


# ---- E ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(BY_NAME))
def test_slots_match_the_float64_oracle(lib, name):
    case = BY_NAME[name]
    rec = _record(case)[0]
    assert len(rec.subset) <= SUBSET.get(name, 24)
    check_oracle(rec.t_sub, rec.o, case.dt, TAP0[_family(TOWERS[case.tower])], SLOT_TOL.get(name), name)


# ---- negative controls: on the CPU, on the recorded taps of the Sfx case -----------------------------------------------------------------

def _control():
    case = BY_NAME[CONTROL]
    rec = _record(case)[0]
    if getattr(rec, "t_perm", None) is None:
        enc = _packed(case.tower, case.dt)
        enc.ws = encoders._Workspace()
        rec.perm = torch.randperm(case.M, generator=torch.Generator().manual_seed(case.M))
        rec.t_perm = _call(enc, _inputs(case)[0][rec.perm].contiguous().cuda(), case.chunk)
        enc.ws = encoders._Workspace()
    return case, rec


def test_control_swapped_slots_fail_duplicates_and_permutation(lib):
    case, rec = _control()
    check_dups(rec.t, rec.dups)
    check_perm(rec.t, rec.t_perm, rec.perm)
    bad = rec.t.clone()
    a, b = rec.dups[2], rec.dups[2] + 1         # a planted slot and the distinct item behind it
    assert b not in rec.dups
    bad[[a, b]] = bad[[b, a]]
    with pytest.raises(AssertionError):
        check_dups(bad, rec.dups)
    with pytest.raises(AssertionError):
        check_perm(bad, rec.t_perm, rec.perm)


def test_control_one_ulp_in_one_element_fails_every_bitwise_check(lib):
    case, rec = _control()
    bad = rec.t.clone()
    s = rec.dups[-1]
    bad[s, 2, 5] = torch.nextafter(bad[s, 2, 5], torch.tensor(float("inf")))
    assert (bad != rec.t).sum() == 1
    with pytest.raises(AssertionError):
        check_dups(bad, rec.dups)               # A
    with pytest.raises(AssertionError):
        check_perm(bad, rec.t_perm, rec.perm)   # B
    with pytest.raises(AssertionError):
        check_bits(bad, rec.t)                  # C, D: every one of them is this comparison against the case's own taps


def test_control_a_wrong_slot_fails_the_per_slot_check(lib):
    """One compared slot's tap 2 replaced by its neighbour's fails E's per-slot check.  With these seeded towers two items' taps are about as
    far apart as they are long (relative distance 0.6 - 1.3), so that replacement is gross enough to fail the per-tap Frobenius figure as
    well (about 1 / sqrt(24) of it) — both are asserted.  What the per-slot check adds shows on a smaller error of the same kind: the
    slot moved towards its neighbour by 2 x the per-slot bound passes every per-tap figure, which averages over the subset, and fails
    per slot."""
    case, rec = _control()
    tol = SLOT_TOL.get(CONTROL)
    assert tol is not None
    check_oracle(rec.t_sub, rec.o, case.dt, TAP0_VIT, tol, "control, untouched")
    k = len(rec.subset) - 1         # a seeded other and the one before it
    bad = rec.t_sub.clone()
    bad[k, 2] = rec.t_sub[k - 1, 2]
    with pytest.raises(AssertionError, match="slot"):
        check_oracle(bad, rec.o, case.dt, TAP0_VIT, tol, "control, neighbour's tap 2")
    assert slot_errors(bad, rec.o)[1][2] > TAP_TOL[case.dt]
    step = rec.t_sub[k - 1, 2] - rec.t_sub[k, 2]
    bad = rec.t_sub.clone()
    bad[k, 2] += step * (2 * tol[1] * rec.o[k, 2].norm() / step.double().norm()).float()
    per_slot, per_tap = slot_errors(bad, rec.o)
    assert per_tap[2] < TAP_TOL[case.dt] and per_slot[k, 2] > tol[1], (per_tap[2].item(), per_slot[k, 2].item())
    with pytest.raises(AssertionError, match=f"slot {k} of the subset"):
        check_oracle(bad, rec.o, case.dt, TAP0_VIT, tol, "control, 2 x the bound towards the neighbour")
