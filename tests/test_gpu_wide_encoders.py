"""The frozen towers at hidden size 1024 (16 heads x 64): ViT-L/16 and BERT-large geometry through both executors, every entry
point, against the CPU oracle on seeded inputs — plus the width-parameterised LayerNorm primitive and the refusals.

Tolerances are the project's own (tests/test_gpu_encoders.py, tests/test_gpu_primitives.py): the per-GEMM operand rounding is
relative and does not depend on K, and every tower here is shallower than the 12 layers those bounds were measured at.
Measured values: profiles/wide_towers.md."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

import golden_io as gio  # noqa: E402,F401  (the shared fixtures' module: imported as the other encoder tests do)
from iisan_amd import _lib, encoders, weights  # noqa: E402
from oracle import iisan_oracle as O  # noqa: E402

TAP_TOL = {_lib.IISAN_F16: 1.5e-3, _lib.IISAN_BF16: 1.2e-2}      # relative Frobenius error per tap
TAP0_VIT, TAP0_BERT = 1e-6, 1e-5                                  # tap 0: no 16-bit arithmetic on the CLS row / fp32 gather + LayerNorm
CLS_ONLY_TOL = 5e-4                                               # CLS-only last block against the full one
T16 = {0: torch.float16, 1: torch.bfloat16}
LN16_TOL = {0: 2e-3, 1: 1.6e-2}                                   # test_layernorm768_vs_torch: one 16-bit rounding of the result

WORDS = 30
TOY_VIT = weights.VitConfig(hidden=1024, layers=2, heads=16, mlp=512, image=32, patch=16)
TOY_BERT = weights.BertConfig(hidden=1024, layers=2, heads=16, mlp=512, vocab=512, max_pos=64)
# ViT-L/16 and BERT-large geometry cut to 4 layers: N = 1024 / 3072 / 4096 and K = 1024 / 4096 on every GEMM family, 16 heads through the
# head-major QKV scatter, S = 197 through the DMA attention kernel
FULL_VIT = weights.VitConfig(hidden=1024, layers=4, heads=16, mlp=4096)
FULL_BERT = weights.BertConfig(hidden=1024, layers=4, heads=16, mlp=4096, vocab=4096, max_pos=64)


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm()).item()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _inputs(n, res, vocab, seed):
    """n items: item 0 is all padding (zero image, zero ids, zero mask: HF attends uniformly), item 1's title ends early (5 words),
    the others carry titles of mixed lengths."""
    g = torch.Generator().manual_seed(seed)
    images = torch.randn(n, 3, res, res, generator=g).clamp_(-1.0, 1.0)
    images[0] = 0
    text = torch.zeros(n, 2 * WORDS, dtype=torch.int64)
    for m in range(1, n):
        ln = 5 if m == 1 else int(torch.randint(6, WORDS + 1, (1,), generator=g))
        text[m, :ln] = torch.randint(1, vocab, (ln,), generator=g)
        text[m, WORDS:WORDS + ln] = 1
    return images, text


def _tower_fixture(vcfg, bcfg, n_img, n_txt, res, seed):
    vw, bw = weights.make_vit_weights(vcfg, seed=seed), weights.make_bert_weights(bcfg, seed=seed + 1)
    images, _ = _inputs(n_img, res, bcfg.vocab, seed + 2)
    _, text = _inputs(n_txt, 16, bcfg.vocab, seed + 3)
    with torch.no_grad():
        oc, ot = O.vit_cls_taps(images, vw, vcfg), O.bert_cls_taps(text, bw, bcfg)
    return SimpleNamespace(vw=vw, bw=bw, images=images, text=text, oc=oc, ot=ot, packed={})


@pytest.fixture(scope="module")
def toy():
    return _tower_fixture(TOY_VIT, TOY_BERT, 6, 6, 32, seed=31)


@pytest.fixture(scope="module")
def full():
    return _tower_fixture(FULL_VIT, FULL_BERT, 3, 4, 224, seed=41)


def _packed(fx, vcfg, bcfg, dt):
    """The packed pair of a fixture, one per operand type (packed once, shared by the tests of the module)."""
    if dt not in fx.packed:
        fx.packed[dt] = (encoders.PackedVit(fx.vw, vcfg, "cuda", dt), encoders.PackedBert(fx.bw, bcfg, "cuda", dt))
    return fx.packed[dt]


def _check_against_oracle(tc, tt, oc, ot, dt, what=""):
    assert torch.isfinite(tc).all() and torch.isfinite(tt).all()
    assert _rel(tc[:, 0], oc[:, 0]) < TAP0_VIT, (what, _rel(tc[:, 0], oc[:, 0]))
    assert _rel(tt[:, 0], ot[:, 0]) < TAP0_BERT, (what, _rel(tt[:, 0], ot[:, 0]))
    for l in range(1, oc.shape[1]):
        ev, eb = _rel(tc[:, l], oc[:, l]), _rel(tt[:, l], ot[:, l])
        print(f"{what} tap {l}: ViT {ev:.3e} BERT {eb:.3e}")
        assert ev < TAP_TOL[dt], f"{what} ViT tap {l}: {ev:.3e}"
        assert eb < TAP_TOL[dt], f"{what} BERT tap {l}: {eb:.3e}"


# ---- 1. toy shapes, every entry point ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", [1, 2, 5])
@pytest.mark.parametrize("dt", [_lib.IISAN_F16, _lib.IISAN_BF16])
def test_toy_wide_towers_match_the_oracle(toy, dt, M):
    """Taps {0, 1, 2} of a 1024-wide 2-layer ViT and BERT, batches far below one GEMM tile, an all-padding item and a title whose mask
    ends early among them; a subset of taps, a chunked run and the same rows inside a larger batch return the same bits."""
    vit, bert = _packed(toy, TOY_VIT, TOY_BERT, dt)
    img, txt = toy.images[:M].contiguous().cuda(), toy.text[:M].contiguous().cuda()
    assert img[0].abs().max() == 0 and txt[0].abs().max() == 0
    tc, tt = vit.forward_taps(img, [0, 1, 2]).cpu(), bert.forward_taps(txt, [0, 1, 2]).cpu()
    assert tc.shape == (M, 3, 1024) and tt.shape == (M, 3, 1024)
    _check_against_oracle(tc, tt, toy.oc[:M], toy.ot[:M], dt, f"toy dt {dt} M {M}")
    # a subset of taps (the deepest one kept: the same blocks run)
    assert torch.equal(vit.forward_taps(img, [0, 2]).cpu(), tc[:, [0, 2]])
    assert torch.equal(bert.forward_taps(txt, [0, 2]).cpu(), tt[:, [0, 2]])
    # chunked execution
    assert torch.equal(vit.forward_taps(img, [0, 1, 2], chunk_items=3).cpu(), tc)
    assert torch.equal(bert.forward_taps(txt, [0, 1, 2], chunk_items=3).cpu(), tt)
    # the same rows inside a larger batch
    assert torch.equal(vit.forward_taps(toy.images.cuda(), [0, 1, 2]).cpu()[:M], tc)
    assert torch.equal(bert.forward_taps(toy.text.cuda(), [0, 1, 2]).cpu()[:M], tt)


@pytest.mark.parametrize("dt", [_lib.IISAN_F16, _lib.IISAN_BF16])
def test_toy_wide_towers_with_the_fp32_residual_stream(lib, toy, dt):
    """Dev switch resid32 = 1 (the whole stream in fp32: `layernorm768_kernel` at width 1024 instead of the mixed kernel): the same
    tolerance, and really another route."""
    vit, bert = _packed(toy, TOY_VIT, TOY_BERT, dt)
    img, txt = toy.images[:5].contiguous().cuda(), toy.text[:5].contiguous().cuda()
    mc, mt = vit.forward_taps(img, [0, 1, 2]).cpu(), bert.forward_taps(txt, [0, 1, 2]).cpu()
    with _lib.dev(resid32=1):
        tc, tt = vit.forward_taps(img, [0, 1, 2]).cpu(), bert.forward_taps(txt, [0, 1, 2]).cpu()
        fc, ft = vit.forward_taps(img, [0, 1, 2], chunk_items=2).cpu(), bert.forward_taps(txt, [0, 1, 2], chunk_items=2).cpu()
    _check_against_oracle(tc, tt, toy.oc[:5], toy.ot[:5], dt, f"toy resid32 dt {dt}")
    assert torch.equal(fc, tc) and torch.equal(ft, tt)
    assert torch.equal(tc[:, 0], mc[:, 0]) and torch.equal(tt[:, 0], mt[:, 0])       # tap 0 is the embedding on either route
    assert not torch.equal(tc, mc) and not torch.equal(tt, mt)


def test_toy_wide_u8_and_indexed_entries_equal_the_direct_ones(toy):
    """The u8 entry against the fp32 entry on the normalised image; the two indexed entries against the direct ones, an out-of-range
    index as the padding slot (zero normalised image; zero ids and mask)."""
    vit, bert = _packed(toy, TOY_VIT, TOY_BERT, _lib.IISAN_F16)
    g = torch.Generator().manual_seed(7)
    u8 = torch.randint(0, 256, (5, 3, 32, 32), generator=g, dtype=torch.uint8)
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
    table = toy.text[1:6].contiguous()                                                # 5 real rows
    txt = table[index.clamp(0, 4)].clone()
    txt[pad] = 0
    want_t = bert.forward_taps(txt.cuda(), [0, 1, 2]).cpu()
    assert torch.equal(bert.forward_taps_indexed(table.cuda(), index.cuda(), [0, 1, 2]).cpu(), want_t)
    assert torch.equal(bert.forward_taps_indexed(table.cuda(), index.cuda(), [0, 1, 2], chunk_items=3).cpu(), want_t)
    assert torch.equal(want_t[3], bert.forward_taps(toy.text[:1].cuda(), [0, 1, 2]).cpu()[0])      # a pad slot IS the all-padding item


def test_toy_wide_dropout_entry_without_dropout_is_the_eval_entry(lib, toy):
    """`iisan_bert_forward_taps_dropout` with drop == NULL, and with both probabilities 0: the bits of the eval entry."""
    _, bert = _packed(toy, TOY_VIT, TOY_BERT, _lib.IISAN_F16)
    txt = toy.text.cuda()
    want = bert.forward_taps(txt, [0, 1, 2])
    M = txt.shape[0]
    tl = (C.c_int32 * 3)(0, 1, 2)
    nbytes = lib.iisan_bert_forward_taps_ws_bytes(C.byref(bert.struct), M, WORDS, 0)
    ws = torch.empty(int(nbytes), dtype=torch.uint8, device="cuda")
    for drop in (None, C.byref(_lib.BertDropout(0.0, 0.0, 77))):
        taps = torch.full((M, 3, 1024), float("nan"), device="cuda")
        _lib.check(lib.iisan_bert_forward_taps_dropout(C.byref(bert.struct), txt.data_ptr(), 0, None, M, WORDS, tl, 3, taps.data_ptr(), 0,
                                                       drop, ws.data_ptr(), ws.numel(), _stream()), "iisan_bert_forward_taps_dropout")
        torch.cuda.synchronize()
        assert torch.equal(taps, want)


# ---- 2. full-width shapes through every GEMM family --------------------------------------------------------------------------------

@pytest.fixture
def gemm_variant(lib, request):
    _lib.dev_set("gemm16_variant", request.param)
    yield request.param
    _lib.dev_set("gemm16_variant", 0)


@pytest.mark.parametrize("gemm_variant", [0, 1, 3, 4], indirect=True)
def test_full_width_taps_match_the_oracle_on_every_gemm_family(full, gemm_variant):
    """ViT-L/16 geometry (197 tokens, mlp 4096, 16 heads) on 3 images and BERT-large geometry (30 words) on 4 titles, 4 layers each,
    all 5 taps, once per GEMM kernel family (0 = auto, 1 = 128x128, 3 = staggered 256x256, 4 = the production 256x256 kernel)."""
    vit, bert = _packed(full, FULL_VIT, FULL_BERT, _lib.IISAN_F16)
    layers = list(range(5))
    tc, tt = vit.forward_taps(full.images.cuda(), layers).cpu(), bert.forward_taps(full.text.cuda(), layers).cpu()
    _check_against_oracle(tc, tt, full.oc, full.ot, _lib.IISAN_F16, f"full variant {gemm_variant}")
    # S = 197 goes to the DMA attention kernel by default; attention16_kernel gives the same bits, as at 768
    _lib.dev_set("count:attn16_dma", 0)
    assert torch.equal(vit.forward_taps(full.images.cuda(), layers).cpu(), tc)
    assert _lib.dev_get("count:attn16_dma") > 0
    with _lib.dev(attn_route=1):
        _lib.dev_set("count:attn16_dma", 0)
        assert torch.equal(vit.forward_taps(full.images.cuda(), layers).cpu(), tc)
        assert _lib.dev_get("count:attn16_dma") == 0


# ---- 3. dead-work policy ---------------------------------------------------------------------------------------------------------------

def test_full_width_cls_only_last_block_and_tapped_prefix(lib, full):
    """full_blocks 1 against 0 at 1024: the shallower taps bit-equal, the last one within 5e-4; a tapped prefix [0, 2] of the 4-layer
    tower does not run blocks 3 - 4 and equals the full run's taps 0 and 2 under the same rule."""
    vit, bert = _packed(full, FULL_VIT, FULL_BERT, _lib.IISAN_F16)
    img, txt = full.images.cuda(), full.text.cuda()
    layers = list(range(5))
    with _lib.dev(full_blocks=1):
        fc, ft = vit.forward_taps(img, layers).cpu(), bert.forward_taps(txt, layers).cpu()
    pc, pt = vit.forward_taps(img, layers).cpu(), bert.forward_taps(txt, layers).cpu()
    assert torch.equal(pc[:, :4], fc[:, :4]) and torch.equal(pt[:, :4], ft[:, :4])
    print(f"cls-only vs full, tap 4: ViT {_rel(pc[:, 4], fc[:, 4]):.3e} BERT {_rel(pt[:, 4], ft[:, 4]):.3e}")
    assert _rel(pc[:, 4], fc[:, 4]) < CLS_ONLY_TOL, _rel(pc[:, 4], fc[:, 4])
    assert _rel(pt[:, 4], ft[:, 4]) < CLS_ONLY_TOL, _rel(pt[:, 4], ft[:, 4])
    _check_against_oracle(fc, ft, full.oc, full.ot, _lib.IISAN_F16, "full_blocks")
    # the tapped prefix: blocks 3 - 4 are dead code (counted: launches of the encoder GEMM per family)
    fam = ("gemm16_h256", "gemm16_s256", "gemm16_v1")

    def launches(fn):
        for n in fam:
            _lib.dev_set("count:" + n, 0)
        out = fn()
        return out, sum(_lib.dev_get("count:" + n) for n in fam)

    (sc, st), n_prefix = launches(lambda: (vit.forward_taps(img, [0, 2]).cpu(), bert.forward_taps(txt, [0, 2]).cpu()))
    _, n_whole = launches(lambda: (vit.forward_taps(img, layers), bert.forward_taps(txt, layers)))
    assert n_prefix < n_whole, (n_prefix, n_whole)
    assert torch.equal(sc[:, 0], fc[:, 0]) and torch.equal(st[:, 0], ft[:, 0])
    print(f"prefix [0, 2] vs full, tap 2: ViT {_rel(sc[:, 1], fc[:, 2]):.3e} BERT {_rel(st[:, 1], ft[:, 2]):.3e}")
    assert _rel(sc[:, 1], fc[:, 2]) < CLS_ONLY_TOL and _rel(st[:, 1], ft[:, 2]) < CLS_ONLY_TOL
    assert _rel(sc[:, 1], full.oc[:, 2]) < TAP_TOL[_lib.IISAN_F16] and _rel(st[:, 1], full.ot[:, 2]) < TAP_TOL[_lib.IISAN_F16]


# ---- 4. the block-major F1 intermediate at 1024 ---------------------------------------------------------------------------------------

def test_full_width_blk32_off_gives_the_same_bits(lib, full):
    """At 1024 the block-major F1 (FC1 -> FC2 intermediate) applies once both products reach the 256x256 kernel under the auto dispatch:
    at least 128 tiles of the [rows, 1024] FC2 output = 32 row tiles — 42 images x 197 tokens, 274 titles x 30 words.  blk32 = 0 writes it
    row-major: the same kernels, the same arithmetic, bit-equal taps — and the counter shows the default really was block-major."""
    vit, bert = _packed(full, FULL_VIT, FULL_BERT, _lib.IISAN_F16)
    g = torch.Generator().manual_seed(9)
    img = torch.randn(42, 3, 224, 224, generator=g).clamp_(-1.0, 1.0).cuda()
    _, text = _inputs(274, 16, FULL_BERT.vocab, 10)
    txt = text.cuda()
    layers = list(range(5))
    out = {}
    for blk in (2, 0):
        with _lib.dev(blk32=blk, full_blocks=1):
            _lib.dev_set("count:gemm16_blk32", 0)
            out[blk] = (vit.forward_taps(img, layers), bert.forward_taps(txt, layers))
            torch.cuda.synchronize()
            n = _lib.dev_get("count:gemm16_blk32")
        assert n == (0 if blk == 0 else 2 * 2 * 4), (blk, n)        # FC1 + FC2 of 4 blocks, two towers
    assert torch.isfinite(out[2][0]).all() and torch.isfinite(out[2][1]).all()
    assert torch.equal(out[0][0], out[2][0]) and torch.equal(out[0][1], out[2][1])


# ---- 5. the primitive ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows", [1, 7, 8, 9, 1001])
@pytest.mark.parametrize("dt", [0, 1])
def test_layernorm_width_1024_vs_torch(lib, dt, rows):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(rows, 1024, generator=g) * 3 + 0.7
    w = 1 + 0.1 * torch.randn(1024, generator=g)
    b = 0.1 * torch.randn(1024, generator=g)
    ref = torch.nn.functional.layer_norm(x.double(), (1024,), w.double(), b.double(), 1e-12)
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    o16 = torch.empty(rows + 1, 1024, dtype=T16[dt], device="cuda").fill_(7.0)        # one guard row behind each output
    o32 = torch.empty(rows + 1, 1024, dtype=torch.float32, device="cuda").fill_(7.0)
    _lib.check(lib.iisan_layernorm(dt, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), 1e-12, o16.data_ptr(), o32.data_ptr(), rows, 1024,
                                   _stream()), "layernorm 1024")
    torch.cuda.synchronize()
    assert (o32[:rows].cpu().double() - ref).abs().max().item() < 5e-6 * ref.abs().max().item() + 1e-5
    assert (o16[:rows].cpu().double() - ref).abs().max().item() < LN16_TOL[dt] * ref.abs().max().item()
    assert (o32[rows] == 7.0).all() and (o16[rows] == 7.0).all()
    # in-place fp32 output
    _lib.check(lib.iisan_layernorm(dt, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), 1e-12, None, xd.data_ptr(), rows, 1024, _stream()),
               "layernorm 1024 in place")
    torch.cuda.synchronize()
    assert (xd.cpu().double() - ref).abs().max().item() < 5e-6 * ref.abs().max().item() + 1e-5


@pytest.mark.parametrize("dt", [0, 1])
def test_layernorm_width_768_is_layernorm768(lib, dt):
    g = torch.Generator().manual_seed(4)
    rows = 1001
    x = (torch.randn(rows, 768, generator=g) * 3 + 0.7).cuda()
    w, b = (1 + 0.1 * torch.randn(768, generator=g)).cuda(), (0.1 * torch.randn(768, generator=g)).cuda()
    outs = []
    for call in ("old", "new"):
        o16 = torch.zeros(rows, 768, dtype=T16[dt], device="cuda")
        o32 = torch.zeros(rows, 768, dtype=torch.float32, device="cuda")
        if call == "old":
            _lib.check(lib.iisan_layernorm768(dt, x.data_ptr(), w.data_ptr(), b.data_ptr(), 1e-12, o16.data_ptr(), o32.data_ptr(), rows, _stream()), "layernorm768")
        else:
            _lib.check(lib.iisan_layernorm(dt, x.data_ptr(), w.data_ptr(), b.data_ptr(), 1e-12, o16.data_ptr(), o32.data_ptr(), rows, 768, _stream()), "layernorm")
        torch.cuda.synchronize()
        outs.append((o16, o32))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert outs[0][1].abs().max() > 0


# ---- 6. refusals: an error code and a message, nothing launched --------------------------------------------------------------------

@pytest.mark.parametrize("hidden,heads", [(1280, 20), (512, 8), (1024, 12)])
def test_unsupported_widths_are_refused(lib, hidden, heads):
    vcfg = weights.VitConfig(hidden=hidden, layers=1, heads=heads, mlp=128, image=32, patch=16)
    bcfg = weights.BertConfig(hidden=hidden, layers=1, heads=heads, mlp=128, vocab=64, max_pos=32)
    vit = encoders.PackedVit(weights.make_vit_weights(vcfg, seed=1), vcfg, "cuda")
    bert = encoders.PackedBert(weights.make_bert_weights(bcfg, seed=2), bcfg, "cuda")
    fam = ("gemm16_h256", "gemm16_s256", "gemm16_v1")
    for n in fam:
        _lib.dev_set("count:" + n, 0)
    with pytest.raises(_lib.IisanHipError, match="768.*1024"):
        vit.forward_taps(torch.zeros(2, 3, 32, 32, device="cuda"), [0, 1])
    with pytest.raises(_lib.IisanHipError, match="768.*1024"):
        bert.forward_taps(torch.zeros(2, 16, dtype=torch.int64, device="cuda"), [0, 1])
    assert sum(_lib.dev_get("count:" + n) for n in fam) == 0


def test_layernorm_refuses_width_512(lib):
    x = torch.ones(4, 512, device="cuda")
    o = torch.full((4, 512), 7.0, device="cuda")
    w = torch.ones(512, device="cuda")
    rc = lib.iisan_layernorm(0, x.data_ptr(), w.data_ptr(), w.data_ptr(), 1e-12, None, o.data_ptr(), 4, 512, _stream())
    with pytest.raises(_lib.IisanHipError, match="512"):
        _lib.check(rc, "layernorm 512")
    torch.cuda.synchronize()
    assert (o == 7.0).all()


def test_wide_bert_refuses_dropout_and_wide_vit_has_no_folded_set(lib, toy):
    vit, bert = _packed(toy, TOY_VIT, TOY_BERT, _lib.IISAN_F16)
    with pytest.raises(_lib.IisanHipError, match="1024"):
        bert.forward_taps(toy.text.cuda(), [0, 1, 2], dropout=(0.1, 0.1, 5))
    with pytest.raises(_lib.IisanHipError, match="1024"):
        bert.forward_taps(toy.text.cuda(), [0, 1, 2], dropout=(0.0, 0.1, 5))
    assert lib.iisan_vit_fold_bytes(C.byref(vit.struct)) == 0
    assert not vit.struct.folded and vit.struct.layer[0].qkv_w32 is None
    for cfg in (weights.VIT_LARGE, weights.BERT_LARGE):
        assert (cfg.hidden, cfg.layers, cfg.heads, cfg.mlp) == (1024, 24, 16, 4096)
    assert weights.BERT_LARGE.vocab == 30522 and weights.BERT_LARGE.eps == 1e-12 and weights.VIT_LARGE.tokens == 197
