"""The frozen towers past 224 tokens: ViTs at 240 / 256 / 384 pixels (226 / 257 / 577 tokens) and BERT titles of 226 / 300 / 512 words
through both executors and every entry point, against the CPU oracle on seeded inputs — the attention steps run the streaming-softmax
kernel (csrc/attn16_long.hip) and, in the CLS-only last block, the 1,024-key score row of `attention_cls_kernel` — plus the refusals.

Pattern and tolerances are those of tests/test_gpu_wide_encoders.py (the per-GEMM operand rounding is relative and does not depend on the
token count; every tower here is 2 layers deep).  Measured values: profiles/long_sequences.md."""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

import golden_io as gio  # noqa: E402,F401  (the shared fixtures' module: imported as the other encoder tests do)
from iisan_amd import _lib, encoders, evaluate, synth, weights  # noqa: E402
from iisan_amd import factory as helpers  # noqa: E402
from oracle import iisan_oracle as O  # noqa: E402

TAP_TOL = {_lib.IISAN_F16: 1.5e-3, _lib.IISAN_BF16: 1.2e-2}      # relative Frobenius error per tap
TAP0_VIT, TAP0_BERT = 1e-6, 1e-5                                  # tap 0: no 16-bit arithmetic on the CLS row / fp32 gather + LayerNorm
N_ITEMS = 6
GEMM_FAMILIES = ("gemm16_h256", "gemm16_s256", "gemm16_v1")

VITS = {
    "vit240": weights.VitConfig(hidden=768, layers=2, heads=12, mlp=512, image=240, patch=16),       # 226 tokens
    "vit256": weights.VitConfig(hidden=768, layers=2, heads=12, mlp=512, image=256, patch=16),       # 257 tokens
    "vit384_full": weights.VitConfig(hidden=768, layers=2, heads=12, mlp=3072, image=384, patch=16), # 577 tokens, ViT-B/16-384 geometry
    "vit256_wide": weights.VitConfig(hidden=1024, layers=2, heads=16, mlp=512, image=256, patch=16),
}
BERT = weights.BertConfig(hidden=768, layers=2, heads=12, mlp=512, vocab=512, max_pos=512)
BERT_WORDS = (226, 300, 512)

_FIX = {}


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm()).item()


def _images(n, res, seed):
    g = torch.Generator().manual_seed(seed)
    images = torch.randn(n, 3, res, res, generator=g).clamp_(-1.0, 1.0)
    images[0] = 0                                       # the padding item
    return images


def _titles(n, words, vocab, seed):
    """item 0 is all padding (zero ids, zero mask: HF attends uniformly), item 1's title ends after 5 words, the others carry titles of
    mixed lengths."""
    g = torch.Generator().manual_seed(seed)
    text = torch.zeros(n, 2 * words, dtype=torch.int64)
    for m in range(1, n):
        ln = 5 if m == 1 else int(torch.randint(6, words + 1, (1,), generator=g))
        text[m, :ln] = torch.randint(1, vocab, (ln,), generator=g)
        text[m, words:words + ln] = 1
    return text


def _vit_fixture(name):
    """(weights, inputs, oracle taps) of one ViT: computed once on the CPU, shared, never modified; packed once per operand type."""
    if name not in _FIX:
        cfg = VITS[name]
        w = weights.make_vit_weights(cfg, seed=71)
        x = _images(N_ITEMS, cfg.image, 73)
        with torch.no_grad():
            o = O.vit_cls_taps(x, w, cfg)
        _FIX[name] = SimpleNamespace(cfg=cfg, w=w, x=x, o=o, packed={})
    return _FIX[name]


def _bert_fixture(words):
    if words not in _FIX:
        w = weights.make_bert_weights(BERT, seed=72)
        x = _titles(N_ITEMS, words, BERT.vocab, 74)
        with torch.no_grad():
            o = O.bert_cls_taps(x, w, BERT)
        _FIX[words] = SimpleNamespace(cfg=BERT, w=w, x=x, o=o, packed={})
    return _FIX[words]


def _packed(fx, dt):
    if dt not in fx.packed:
        cls = encoders.PackedVit if isinstance(fx.cfg, weights.VitConfig) else encoders.PackedBert
        fx.packed[dt] = cls(fx.w, fx.cfg, "cuda", dt)
    return fx.packed[dt]


def _check_against_oracle(t, o, dt, tap0, what=""):
    assert torch.isfinite(t).all()
    assert _rel(t[:, 0], o[:, 0]) < tap0, (what, _rel(t[:, 0], o[:, 0]))
    for l in range(1, o.shape[1]):
        e = _rel(t[:, l], o[:, l])
        print(f"{what} tap {l}: {e:.3e}")
        assert e < TAP_TOL[dt], f"{what} tap {l}: {e:.3e}"


def _tower(fx, dt, M, tap0, what):
    """Taps {0, 1, 2} of M items against the oracle — CLS-only last block (the default) and all-token last block; a subset of taps, a
    chunked run and the same rows inside a larger batch give the same bits."""
    enc = _packed(fx, dt)
    x = fx.x[:M].contiguous().cuda()
    assert x[0].abs().max() == 0
    _lib.dev_set("count:attn16_long", 0)
    t = enc.forward_taps(x, [0, 1, 2]).cpu()
    assert _lib.dev_get("count:attn16_long") == 1          # block 0 all tokens; block 1 is the CLS-only one
    assert t.shape == (M, 3, fx.cfg.hidden)
    _check_against_oracle(t, fx.o[:M], dt, tap0, f"{what} dt {dt} M {M} full_blocks 0")
    with _lib.dev(full_blocks=1):
        f = enc.forward_taps(x, [0, 1, 2]).cpu()
    assert _lib.dev_get("count:attn16_long") == 3          # ... and here both blocks ran on all tokens
    assert torch.equal(f[:, :2], t[:, :2])
    _check_against_oracle(f, fx.o[:M], dt, tap0, f"{what} dt {dt} M {M} full_blocks 1")
    assert torch.equal(enc.forward_taps(x, [0, 2]).cpu(), t[:, [0, 2]])
    assert torch.equal(enc.forward_taps(x, [0, 1, 2], chunk_items=3).cpu(), t)
    assert torch.equal(enc.forward_taps(fx.x.cuda(), [0, 1, 2]).cpu()[:M], t)


# ---- 1. every tower against the oracle ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", [1, 2, 5])
@pytest.mark.parametrize("dt", [_lib.IISAN_F16, _lib.IISAN_BF16])
@pytest.mark.parametrize("name", list(VITS))
def test_long_vit_matches_the_oracle(lib, name, dt, M):
    _tower(_vit_fixture(name), dt, M, TAP0_VIT, name)


@pytest.mark.parametrize("M", [1, 2, 5])
@pytest.mark.parametrize("dt", [_lib.IISAN_F16, _lib.IISAN_BF16])
@pytest.mark.parametrize("words", BERT_WORDS)
def test_long_bert_matches_the_oracle(lib, words, dt, M):
    _tower(_bert_fixture(words), dt, M, TAP0_BERT, f"bert {words} words")


@pytest.mark.parametrize("dt", [_lib.IISAN_F16, _lib.IISAN_BF16])
def test_full_width_384_pixel_vit_on_the_256x256_gemm_family(lib, dt):
    """577 tokens per image with the production 256x256 GEMM kernel forced (the batch is too small to reach it by itself): LayerNorm and the
    residual adds in the GEMM epilogues, the block-major stream and F1, the head-major QKV scatter at S = 577."""
    fx = _vit_fixture("vit384_full")
    enc = _packed(fx, dt)
    x = fx.x.cuda()
    base = enc.forward_taps(x, [0, 1, 2]).cpu()
    for full_blocks in (0, 1):
        with _lib.dev(gemm16_variant=4, full_blocks=full_blocks):
            _lib.dev_set("count:gemm16_h256", 0)
            t = enc.forward_taps(x, [0, 1, 2]).cpu()
            assert _lib.dev_get("count:gemm16_h256") > 0
            assert torch.equal(enc.forward_taps(x, [0, 1, 2], chunk_items=4).cpu(), t)
        _check_against_oracle(t, fx.o, dt, TAP0_VIT, f"vit384_full h256 dt {dt} full_blocks {full_blocks}")
    assert torch.equal(base[:, 0], t[:, 0])


# ---- 2. the other entry points --------------------------------------------------------------------------------------------------------

def test_u8_and_indexed_entries_equal_the_direct_ones_at_257_tokens_and_300_words(lib):
    vit, bert = _packed(_vit_fixture("vit256"), _lib.IISAN_F16), _packed(_bert_fixture(300), _lib.IISAN_F16)
    g = torch.Generator().manual_seed(7)
    u8 = torch.randint(0, 256, (5, 3, 256, 256), generator=g, dtype=torch.uint8)
    norm = (u8.float().div(255) - 0.5) / 0.5
    t_f32 = vit.forward_taps(norm.cuda(), [0, 1, 2]).cpu()
    assert torch.equal(vit.forward_taps(u8.cuda(), [0, 1, 2]).cpu(), t_f32)
    index = torch.tensor([3, 5, 0, -1, 4, 3, 99], dtype=torch.int64)                   # 5, -1, 99: outside the 5-row catalogue
    pad = (index < 0) | (index >= 5)
    direct = norm[index.clamp(0, 4)].clone()
    direct[pad] = 0
    want = vit.forward_taps(direct.cuda(), [0, 1, 2]).cpu()
    assert torch.equal(vit.forward_taps_indexed(u8.cuda(), index.cuda(), [0, 1, 2]).cpu(), want)
    assert torch.equal(vit.forward_taps_indexed(u8.cuda(), index.cuda(), [0, 1, 2], chunk_items=3).cpu(), want)
    text = _bert_fixture(300).x
    table = text[1:6].contiguous()                                                    # 5 real rows
    txt = table[index.clamp(0, 4)].clone()
    txt[pad] = 0
    want_t = bert.forward_taps(txt.cuda(), [0, 1, 2]).cpu()
    assert torch.equal(bert.forward_taps_indexed(table.cuda(), index.cuda(), [0, 1, 2]).cpu(), want_t)
    assert torch.equal(bert.forward_taps_indexed(table.cuda(), index.cuda(), [0, 1, 2], chunk_items=3).cpu(), want_t)
    assert torch.equal(want_t[3], bert.forward_taps(text[:1].cuda(), [0, 1, 2]).cpu()[0])      # a pad slot IS the all-padding item


def test_build_tap_cache_over_a_256_pixel_vit_and_300_word_titles(lib):
    vfx, bfx = _vit_fixture("vit256"), _bert_fixture(300)
    images, text = vfx.x, bfx.x
    pop = synth.make_pop_prob(N_ITEMS - 1)
    args = helpers.make_args(side_adapter_vit_list="0,1", side_adapter_bert_list="0,1", num_words_title=300)
    model = helpers.build_model(args, N_ITEMS - 1, pop, vfx.w, vfx.cfg, bfx.w, bfx.cfg, cached=False, device="cuda")
    taps_cv, taps_tx = evaluate.build_tap_cache(model, images.cuda(), text.cuda(), batch=4)
    assert taps_cv.shape == (N_ITEMS, 3, 768) and taps_tx.shape == (N_ITEMS, 3, 768)
    assert taps_cv.dtype == torch.float32 and torch.isfinite(taps_cv).all() and torch.isfinite(taps_tx).all()
    enc = model.mm_encoder
    assert torch.equal(taps_cv, enc.cv_encoder.packed("cuda").forward_taps(images.cuda(), [0, 1, 2]))
    assert torch.equal(taps_tx, enc.bert_encoder.text_encoders["title"].packed("cuda").forward_taps(text.cuda(), [0, 1, 2]))
    # the cache builder runs every block on all tokens or the CLS-only last one as the direct call does: against the oracle either way
    _check_against_oracle(taps_cv.cpu(), vfx.o, _lib.IISAN_F16, TAP0_VIT, "tap cache ViT")
    _check_against_oracle(taps_tx.cpu(), bfx.o, _lib.IISAN_F16, TAP0_BERT, "tap cache BERT")


# ---- 3. refusals: an error code and a message, nothing launched --------------------------------------------------------------------

def _launch_counts():
    return [_lib.dev_get("count:" + n) for n in GEMM_FAMILIES + ("attn16_long", "bert_drop")]


def test_bert_dropout_past_224_words_is_refused(lib):
    bert = _packed(_bert_fixture(300), _lib.IISAN_F16)
    txt = _bert_fixture(300).x.cuda()
    torch.cuda.synchronize()
    before = _launch_counts()
    with pytest.raises(_lib.IisanHipError, match="300.*eval mode"):
        bert.forward_taps(txt, [0, 1, 2], dropout=(0.1, 0.1, 5))
    assert _launch_counts() == before


def test_lengths_past_the_limits_are_refused(lib):
    bert = _packed(_bert_fixture(300), _lib.IISAN_F16)
    txt = torch.zeros(2, 2 * 513, dtype=torch.int64, device="cuda")
    vcfg = weights.VitConfig(hidden=768, layers=1, heads=12, mlp=128, image=528, patch=16)       # 33 x 33 + 1 = 1,090 tokens
    vit = encoders.PackedVit(weights.make_vit_weights(vcfg, seed=1), vcfg, "cuda")
    torch.cuda.synchronize()
    before = _launch_counts()
    with pytest.raises(_lib.IisanHipError, match="513"):
        bert.forward_taps(txt, [0, 1, 2])
    with pytest.raises(_lib.IisanHipError, match="1090"):
        vit.forward_taps(torch.zeros(1, 3, 528, 528, device="cuda"), [0, 1])
    assert _launch_counts() == before
