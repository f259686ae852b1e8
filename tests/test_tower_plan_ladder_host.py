"""The plan ladders of the two frozen-tower executors (four tower families) at the library defaults, as literal `(case, M) -> plan` rows.

At the defaults (`_lib.dev_state() == ""`) the plan of a call (encoders.hip: vit_plan / bert_plan, asked through `iisan_encoder_plan`) is a
function of the batch size alone, because gemm16_route hands a product to the 256x256 kernel `gemm16_h256` — the only kernel with LayerNorm
and the residual add in its epilogue and with block-major operands — exactly where

    ceil(rows / 256) * (N / 256) >= 128          (gemm16.hip, gemm16_route: "at least half a tile per CU" of 256 compute units)

and a plan needs EVERY product of a list, for every chunk size of the call, on that kernel (Products::all_h256).  With rows = M * T token
rows, the first row count at which a product of N columns reaches 128 tiles is (ceil(128 / (N / 256)) - 1) * 256 + 1:

    product            N        N / 256   row tiles   first rows
    O, FC2 (768)       768      3         43          42 * 256 + 1 = 10,753
    K/V  (768)         1,536    6         22          21 * 256 + 1 =  5,377
    QKV  (768)         2,304    9         15          14 * 256 + 1 =  3,585
    FC1  (768)         3,072    12        11          10 * 256 + 1 =  2,561
    O, FC2 (1024)      1,024    4         32          31 * 256 + 1 =  7,937

  * ViT 768 fp16, `F` (LayerNorm in the QKV / FC1 epilogues) needs QKV, FC1 and — unless every block runs on all tokens — the K/V product of
    the CLS-only last block: 5,377 rows (3,585 with full_blocks).  `Sfx` (the adds in the O / FC2 epilogues, F1 and the stream block-major)
    needs O and FC2 as well: 10,753 rows.  First M of a step = ceil(rows / T):
        T = 197:  ceil(5,377 / 197) = 28       ceil(10,753 / 197) = 55
        T = 10:   ceil(5,377 / 10) = 538       ceil(10,753 / 10) = 1,076
        T = 5:    ceil(5,377 / 5) = 1,076      ceil(3,585 / 5) = 717 (full_blocks)      ceil(10,753 / 5) = 2,151
  * bf16 and 1024-wide ViTs have no folded route (vit_fold_routes): `I` throughout; the `f` (block-major F1) needs FC1 and FC2 on gemm16_h256:
        768 bf16, T = 5:  ceil(10,753 / 5) = 2,151          1024, T = 5:  ceil(7,937 / 5) = 1,588
  * BERT 768, 30 words: `a` (stream and 16-bit image share a buffer) is fp16 only and independent of M; `f` from ceil(10,753 / 30) = 359.
  * A chunked call has two chunk sizes, Mc and the last one, and the smaller decides: M = 2,300 in chunks of 2,200 ends on 100 items (`I`),
    3,300 on 1,100 (>= 1,076, < 2,151: `F`), 4,363 on 2,163 (>= 2,151: `Sfx`).
  * The narrow towers (hidden 128 - 384) have no 256x256 route at these sizes at all.
  * A CLIP vision tower (tower kind 2, the ViT letters) never takes the folded routes (vit_fold_routes: its pre-LayerNorm stream keeps the
    LayerNorm images), at 768 with fp16 operands included: `I` throughout, and `f` where FC1 and FC2 are on gemm16_h256, quick-GELU
    epilogue and all; `full_blocks` changes neither.  768: 10,753 rows, 1024: 7,937 rows.  First M = ceil(rows / T):
        768, T = 5 (32 px, patch 16):     ceil(10,753 / 5) = 2,151        768, T = 50 (B/32 at 224 px):    ceil(10,753 / 50) = 216
        1024, T = 5 (28 px, patch 14):    ceil(7,937 / 5) = 1,588         1024, T = 257 (L/14 at 224 px):  ceil(7,937 / 257) = 31
        768, T = 5, chunks of 2,200:      2,200 + 2,151 = 4,351 (the last chunk decides)
  * A DeBERTa text tower (tower kind 3, the BERT letters; the last argument of `iisan_encoder_plan` carries the span) runs the BERT
    executor's plan: `a` with fp16 operands, `f` from the same row counts.
        768, 30 words:   ceil(10,753 / 30) = 359       768, 128 words:  ceil(10,753 / 128) = 85       1024, 30 words:  ceil(7,937 / 30) = 265
        768, 30 words, chunks of 400:  400 + 359 = 759
        384 (N = 384, 1,536: N % 256 != 0, no 256x256 route): never `f`.

A changed rule moves a threshold and fails the row at the step's first M or at M - 1.  Plan letters: tests/test_host_logic.py::
test_encoder_plan_table.  The GPU file tests/test_gpu_tower_plan_ladder.py runs one case per step and asserts the same strings."""
import pytest

VIT, BERT, CLIP, DEBERTA, F16, BF16 = 0, 1, 2, 3, 0, 1


def vit(dt=F16, hidden=768, tokens=5, chunk=0, full=0):
    """(tower, dtype16, hidden, heads, mlp, tokens, chunk_items, deepest tap, full_blocks, folded set supplied): a 2-block tower tapped at
    [0, 1, 2]; PackedVit supplies the folded set exactly where the executor has the folded routes (fp16, 768)."""
    return (VIT, dt, hidden, hidden // 64, 4 * hidden, tokens, chunk, 2, full, int(dt == F16 and hidden == 768))


def bert(dt=F16, hidden=768, words=30):
    return (BERT, dt, hidden, hidden // 64, 4 * hidden, words, 0, 2, 0, 0)


def clip(dt=F16, hidden=768, tokens=5, chunk=0, full=0):
    """A CLIP vision tower: the ViT executor, never the folded set."""
    return (CLIP, dt, hidden, hidden // 64, 4 * hidden, tokens, chunk, 2, full, 0)


def deberta(dt=F16, hidden=768, words=30, chunk=0, span=256):
    """A DeBERTa-v2/v3 text tower: the BERT executor; the last argument carries the span."""
    return (DEBERTA, dt, hidden, hidden // 64, 4 * hidden, words, chunk, 2, 0, span)


LADDERS = [
    # ViT 768, fp16, 197 tokens: I from 1, F from 28, Sfx from 55
    (vit(tokens=197), [(1, "I"), (27, "I"), (28, "F"), (54, "F"), (55, "Sfx"), (1408, "Sfx")]),
    # ViT 768, fp16, 5 tokens (32 px): I from 1, F from 1,076, Sfx from 2,151
    (vit(), [(1, "I"), (1075, "I"), (1076, "F"), (2150, "F"), (2151, "Sfx"), (2203, "Sfx")]),
    # ... every block on all tokens: no K/V product, F from 717
    (vit(full=1), [(1, "I"), (716, "I"), (717, "F"), (720, "F"), (2150, "F"), (2151, "Sfx"), (2203, "Sfx")]),
    # ViT 768, fp16, 10 tokens (48 px): F from 538, Sfx from 1,076
    (vit(tokens=10), [(537, "I"), (538, "F"), (1075, "F"), (1076, "Sfx"), (1077, "Sfx")]),
    # ViT 768, bf16, 5 tokens: I from 1, If from 2,151
    (vit(dt=BF16), [(1, "I"), (2150, "I"), (2151, "If"), (2203, "If")]),
    # ViT 1024, fp16, 5 tokens: I from 1, If from 1,588
    (vit(hidden=1024), [(1, "I"), (1587, "I"), (1588, "If"), (1603, "If")]),
    # BERT 768, 30 words: fp16 Ma from 1, Maf from 359; bf16 M, then Mf
    (bert(), [(1, "Ma"), (358, "Ma"), (359, "Maf"), (367, "Maf")]),
    (bert(dt=BF16), [(1, "M"), (358, "M"), (359, "Mf"), (367, "Mf")]),
    # 5 tokens in chunks of 2,200 items: the last chunk decides for the whole call
    (vit(chunk=2200), [(2300, "I"), (3275, "I"), (3276, "F"), (3300, "F"), (4350, "F"), (4351, "Sfx"), (4363, "Sfx")]),
    # the narrow towers of the GPU file
    (vit(hidden=192), [(37, "I")]),
    (bert(hidden=128, words=8), [(37, "Ma")]),
    # DeBERTa 768, 30 words, span 256: fp16 Ma from 1, Maf from 359; bf16 M, then Mf
    (deberta(), [(1, "Ma"), (358, "Ma"), (359, "Maf"), (367, "Maf")]),
    (deberta(dt=BF16), [(358, "M"), (359, "Mf")]),
    # DeBERTa 768, 128 words (the longest title): Maf from 85
    (deberta(words=128), [(84, "Ma"), (85, "Maf")]),
    # DeBERTa 1024 (v2-large's width), 30 words: Maf from 265
    (deberta(hidden=1024), [(264, "Ma"), (265, "Maf")]),
    # DeBERTa 384 (v3-xsmall's width): N % 256 != 0, never f
    (deberta(hidden=384), [(367, "Ma"), (1408, "Ma")]),
    # 30 words in chunks of 400 titles: the last chunk decides
    (deberta(chunk=400), [(758, "Ma"), (759, "Maf")]),
    # CLIP 768, fp16, 5 tokens: no folded route, I from 1, If from 2,151; full_blocks changes nothing
    (clip(), [(2150, "I"), (2151, "If"), (2203, "If")]),
    (clip(full=1), [(2150, "I"), (2151, "If"), (2203, "If")]),
    (clip(dt=BF16), [(2150, "I"), (2151, "If")]),
    # CLIP 768, 50 tokens (B/32 at 224 px): If from 216
    (clip(tokens=50), [(215, "I"), (216, "If")]),
    # CLIP 1024, 5 tokens (28 px, patch 14) and 257 tokens (L/14 at 224 px)
    (clip(hidden=1024), [(1587, "I"), (1588, "If")]),
    (clip(hidden=1024, tokens=257), [(30, "I"), (31, "If")]),
    # CLIP 768, 5 tokens in chunks of 2,200 items
    (clip(chunk=2200), [(4350, "I"), (4351, "If")]),
]


def plan_code(tower, w):
    """The letters of tests/test_host_logic.py::test_encoder_plan_table."""
    if w < 0:
        return "!"
    if tower in (VIT, CLIP):
        return "RIFS"[w & 3] + ("f" if w & 4 else "") + ("x" if w & 8 else "") + ("w" if w & 16 else "")
    return ("M" if w & 1 else "P") + ("a" if w & 2 else "") + ("f" if w & 4 else "")


def plan_of(case, M):
    from iisan_amd import _lib
    return plan_code(case[0], _lib.load().iisan_encoder_plan(*case[:6], M, *case[6:]))


@pytest.mark.parametrize("case,rows", LADDERS, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else None)
def test_default_plan_ladder(case, rows):
    from iisan_amd import _lib
    assert _lib.dev_state() == ""
    got = [(M, plan_of(case, M)) for M, _ in rows]
    assert got == rows, (case, got)


def test_thresholds_follow_the_half_a_tile_per_cu_rule():
    """The arithmetic of the module docstring, recomputed from the rule's two constants (256-row tiles, 128 tiles) and compared with
    gemm16_route itself through `iisan_gemm16_route`, then with the first M of every ladder step above."""
    from iisan_amd import _lib
    lib = _lib.load()
    assert _lib.dev_state() == ""
    first_rows = lambda N: (-(-128 // (N // 256)) - 1) * 256 + 1
    assert [first_rows(N) for N in (768, 1536, 2304, 3072, 1024)] == [10753, 5377, 3585, 2561, 7937]
    EPI_OUT16, G16_V1, G16_H256 = 0, lib.iisan_gemm16_route(F16, 0, 1, 768, 768, 0, 0, 0, 0), lib.iisan_gemm16_route(F16, 0, 10753, 768, 768, 0, 0, 0, 0)
    assert G16_V1 != G16_H256
    for N in (768, 1024, 1536, 2304, 3072):
        assert lib.iisan_gemm16_route(F16, EPI_OUT16, first_rows(N), N, 768, 0, 0, 0, 0) == G16_H256, N
        assert lib.iisan_gemm16_route(F16, EPI_OUT16, first_rows(N) - 1, N, 768, 0, 0, 0, 0) == G16_V1, N
    up = lambda rows, T: -(-rows // T)
    assert (up(5377, 197), up(10753, 197)) == (28, 55)
    assert (up(5377, 10), up(10753, 10)) == (538, 1076)
    assert (up(5377, 5), up(3585, 5), up(10753, 5)) == (1076, 717, 2151)
    assert (up(7937, 5), up(10753, 30)) == (1588, 359)
    assert (2300 % 2200, 3300 % 2200, 4363 % 2200) == (100, 1100, 2163) and 2200 + 1076 == 3276 and 2200 + 2151 == 4351
    # the CLIP and DeBERTa ladders: B/32 at 224 px, 128-word titles, the 1024-wide towers, the chunked sums
    assert (up(10753, 50), up(10753, 128), up(7937, 30), up(7937, 257)) == (216, 85, 265, 31)
    assert 2200 + up(10753, 5) == 4351 and 400 + up(10753, 30) == 759 and 759 % 400 == 359 and 758 % 400 == 358
