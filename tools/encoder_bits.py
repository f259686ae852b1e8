#!/usr/bin/env python3
"""Bit fingerprint of the frozen-encoder executors: one SHA-256 of the tap bytes per case, over toy towers and every route the
executors choose between.  Seeded and self-contained (this one file: copy it into a checkout of the parent if the parent lacks a case),
so two builds of the library can be compared line by line:

    python3 tools/encoder_bits.py > child.txt        (and the same in a checkout of the parent)        diff parent.txt child.txt

IISAN_LIB=path fingerprints another build of the library with this tree's Python.

Cases: the two-block hidden-768 towers of tests/golden_io.py on 70 items (whole, and in chunks of 32 whose last one holds 6), fp16 and
bf16, under gemm16_variant 0 / 4 x ln_fold 0 / 1 / 2 x full_blocks 0 / 1, and under resid32 = 1; a tapped prefix; the ViT from fp32
pixels, uint8 pixels and the indexed uint8 catalogue; BERT direct and indexed, in eval mode and with train-mode dropout; toy towers at
hidden 192 / 128, 384 / 256 and 1024; one tower each past 224 tokens (a 256-pixel image at patch 16, titles of 226 words); the two-layer
hidden-1,280 toy ViT-H/14 of tests/vit_huge_io.py (80-wide heads), fp16 and bf16; and the two streaming-softmax attention primitives
directly, `iisan_attention16_long` and `iisan_attention16_hd80`, at S = 17 / 129 / 257 / 577 / 1,024 with 2 heads, unmasked and under
the random-length mask of the tests (tests/attn_stream_io.py)."""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import attn_stream_io as aio  # noqa: E402
import golden_io as gio  # noqa: E402
import vit_huge_io as vio  # noqa: E402
from iisan_amd import _lib, encoders, weights  # noqa: E402

if os.environ.get("IISAN_LIB"):            # another build of the library (the parent's, copied aside)
    _lib.LIB_PATH = os.path.abspath(os.environ["IISAN_LIB"])

ITEMS = 70
DTYPES = (("fp16", _lib.IISAN_F16), ("bf16", _lib.IISAN_BF16))


def sha(*tensors) -> str:
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def inputs(vcfg, words, items=ITEMS, vocab=512, seed=5):
    g = torch.Generator().manual_seed(seed)
    images = torch.randn(items, 3, vcfg.image, vcfg.image, generator=g)
    pixels = torch.randint(0, 256, (items, 3, vcfg.image, vcfg.image), generator=g, dtype=torch.uint8)
    ids = torch.randint(1, vocab, (items, words), generator=g)
    mask = (torch.arange(words)[None, :] < torch.randint(2, words + 1, (items, 1), generator=g)).long()
    index = torch.randint(-1, items + 1, (items,), generator=g)        # -1 and `items` are padding slots
    return images.cuda(), pixels.cuda(), torch.cat([ids * mask, mask], 1).contiguous().cuda(), index.cuda()


def knobs(**kw):
    _lib.dev_reset()
    for name, value in kw.items():
        _lib.dev_set(name, value)


def main():
    assert torch.cuda.is_available(), "encoder_bits: needs the GPU"
    lib = _lib.load()
    out = []

    def emit(name, *tensors):
        out.append(f"{name} {sha(*tensors)}")
        print(out[-1], flush=True)

    try:
        for dname, dt in DTYPES:
            vit = encoders.PackedVit(weights.make_vit_weights(gio.E2E_VIT, seed=11), gio.E2E_VIT, "cuda", dt)
            bert = encoders.PackedBert(weights.make_bert_weights(gio.E2E_BERT, seed=12), gio.E2E_BERT, "cuda", dt)
            images, pixels, text, index = inputs(gio.E2E_VIT, 8)
            for variant in (0, 4):
                for ln_fold in (0, 1, 2):
                    for fb in (0, 1):
                        for chunk in (0, 32):
                            knobs(gemm16_variant=variant, ln_fold=ln_fold, full_blocks=fb)
                            tag = f"{dname} v{variant} ln{ln_fold} fb{fb} c{chunk}"
                            emit(f"vit {tag}", vit.forward_taps(images, [0, 1, 2], chunk_items=chunk))
                            emit(f"bert {tag}", bert.forward_taps(text, [0, 1, 2], chunk_items=chunk))
                for chunk in (0, 32):
                    knobs(gemm16_variant=variant, resid32=1)
                    emit(f"vit {dname} v{variant} resid32 c{chunk}", vit.forward_taps(images, [0, 1, 2], chunk_items=chunk))
                    emit(f"bert {dname} v{variant} resid32 c{chunk}", bert.forward_taps(text, [0, 1, 2], chunk_items=chunk))
                knobs(gemm16_variant=variant)
                for chunk in (0, 32):
                    tag = f"{dname} v{variant} c{chunk}"
                    emit(f"vit prefix {tag}", vit.forward_taps(images, [0, 1], chunk_items=chunk))
                    emit(f"bert prefix {tag}", bert.forward_taps(text, [0, 1], chunk_items=chunk))
                    emit(f"vit u8 {tag}", vit.forward_taps(pixels, [0, 1, 2], chunk_items=chunk))
                    emit(f"vit indexed {tag}", vit.forward_taps_indexed(pixels, index, [0, 1, 2], chunk_items=chunk))
                    emit(f"bert indexed {tag}", bert.forward_taps_indexed(text, index, [0, 1, 2], chunk_items=chunk))
                    for fb in (0, 1):
                        knobs(gemm16_variant=variant, full_blocks=fb)
                        emit(f"bert dropout fb{fb} {tag}", bert.forward_taps(text, [0, 1, 2], chunk_items=chunk, dropout=(0.1, 0.1, 77)))
                        emit(f"bert dropout indexed fb{fb} {tag}",
                             bert.forward_taps_indexed(text, index, [0, 1, 2], chunk_items=chunk, dropout=(0.1, 0.1, 77)))
                    knobs(gemm16_variant=variant)
        # the other widths, and the towers past 224 tokens (fp16; 0 = the route the shape takes by itself, 4 = the production kernel forced)
        towers = [
            ("192/128", weights.VitConfig(hidden=192, layers=2, heads=3, mlp=256, image=32, patch=16),
             weights.BertConfig(hidden=128, layers=2, heads=2, mlp=256, vocab=512, max_pos=64), 8, ITEMS),
            ("384/256", weights.VitConfig(hidden=384, layers=2, heads=6, mlp=256, image=32, patch=16),
             weights.BertConfig(hidden=256, layers=2, heads=4, mlp=256, vocab=512, max_pos=64), 8, ITEMS),
            ("1024", weights.VitConfig(hidden=1024, layers=2, heads=16, mlp=512, image=32, patch=16),
             weights.BertConfig(hidden=1024, layers=2, heads=16, mlp=512, vocab=512, max_pos=64), 8, ITEMS),
            ("long", weights.VitConfig(hidden=768, layers=2, heads=12, mlp=512, image=256, patch=16),
             weights.BertConfig(hidden=768, layers=2, heads=12, mlp=512, vocab=512, max_pos=512), 226, 12),
        ]
        for name, vcfg, bcfg, words, items in towers:
            vit = encoders.PackedVit(weights.make_vit_weights(vcfg, seed=21), vcfg, "cuda", _lib.IISAN_F16)
            bert = encoders.PackedBert(weights.make_bert_weights(bcfg, seed=22), bcfg, "cuda", _lib.IISAN_F16)
            images, _, text, _ = inputs(vcfg, words, items=items)
            for variant in (0, 4):
                for fb in (0, 1):
                    for chunk in (0, items // 2 - 1):
                        knobs(gemm16_variant=variant, full_blocks=fb)
                        tag = f"{name} v{variant} fb{fb} c{chunk}"
                        emit(f"vit {tag}", vit.forward_taps(images, [0, 1, 2], chunk_items=chunk))
                        emit(f"bert {tag}", bert.forward_taps(text, [0, 1, 2], chunk_items=chunk))
        # 80-wide heads: the toy ViT-H/14 (17 tokens, 16 heads of 80)
        for dname, dt in DTYPES:
            knobs()
            vit = encoders.PackedVit(weights.make_vit_weights(vio.GEOM_VIT, seed=vio.GEOM_SEED_W), vio.GEOM_VIT, "cuda", dt)
            x = vio.images(vio.GEOM_ITEMS, vio.GEOM_VIT.image, vio.GEOM_SEED_X).cuda()
            emit(f"vit huge {dname}", vit.forward_taps(x, [0, 1, 2]))
        # the streaming-softmax primitives themselves
        for entry, hd, lay in (("iisan_attention16_long", 64, aio.head_major), ("iisan_attention16_hd80", 80, None)):
            for dname, dt in DTYPES:
                for S in (17, 129, 257, 577, 1024):
                    for masked in (False, True):
                        items, heads = 3, 2
                        qkv, kb = aio.problem(dt, items, S, heads, hd, masked=masked)
                        qkvd = lay(qkv, items, S, heads, hd) if lay else qkv.cuda()
                        ctx = aio.run(lib, entry, dt, qkvd, kb.cuda() if masked else None, items, S, heads, items * S, hd)
                        emit(f"{entry} {dname} S{S} {'masked' if masked else 'plain'}", ctx.view(torch.int16))
    finally:
        _lib.dev_reset()
    print(f"# {len(out)} cases, all {hashlib.sha256(chr(10).join(out).encode()).hexdigest()}")


if __name__ == "__main__":
    main()
