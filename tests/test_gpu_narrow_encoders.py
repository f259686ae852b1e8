"""The frozen towers at hidden 128 - 384 (2 / 3 / 4 / 6 heads x 64): ViT-tiny / ViT-small and BERT-tiny / BERT-mini geometry through both
executors, every entry point, against the CPU oracle on seeded inputs — plus the two primitives the narrow widths add (the row kernels
with several rows per wave, the 128x128 GEMM with a ragged last column tile) and the refusals.

Tolerances are the project's own (tests/test_gpu_wide_encoders.py, tests/test_gpu_primitives.py).  Measured values:
profiles/narrow_towers.md."""
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
GEMM_TOL = {0: 2e-3, 1: 1.6e-2}                                   # test_gemm16_vs_torch: one 16-bit rounding of the result

WORDS = 30
# (ViT hidden / heads, BERT hidden / heads): 2 layers, mlp 256, image 32 / patch 16 (5 tokens), 30 words, vocab 512
TOYS = {"192+128": ((192, 3), (128, 2)), "384+256": ((384, 6), (256, 4))}


def _toy_cfgs(key):
    (vh, vn), (bh, bn) = TOYS[key]
    return (weights.VitConfig(hidden=vh, layers=2, heads=vn, mlp=256, image=32, patch=16),
            weights.BertConfig(hidden=bh, layers=2, heads=bn, mlp=256, vocab=512, max_pos=64))


# ViT-tiny geometry cut to 4 layers (197 tokens, mlp 768: N = 192 / 576 ragged, 768 whole) and BERT-tiny as it is (2 layers; a 4,096-word
# vocabulary: the embedding gather does not depend on its length)
FULL_VIT = weights.VitConfig(hidden=192, layers=4, heads=3, mlp=768)
FULL_BERT = weights.BertConfig(hidden=128, layers=2, heads=2, mlp=512, vocab=4096, max_pos=64)


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
    return SimpleNamespace(vcfg=vcfg, bcfg=bcfg, vw=vw, bw=bw, images=images, text=text, oc=oc, ot=ot, packed={})


_TOY_CACHE = {}


@pytest.fixture(params=sorted(TOYS))
def toy(request):
    """One oracle run per toy pair for the whole module (computed on first use, left unchanged)."""
    if request.param not in _TOY_CACHE:
        vcfg, bcfg = _toy_cfgs(request.param)
        _TOY_CACHE[request.param] = _tower_fixture(vcfg, bcfg, 6, 6, 32, seed=71 + 10 * sorted(TOYS).index(request.param))
    return _TOY_CACHE[request.param]


@pytest.fixture(scope="module")
def full():
    return _tower_fixture(FULL_VIT, FULL_BERT, 3, 4, 224, seed=91)


def _packed(fx, dt):
    """The packed pair of a fixture, one per operand type (packed once, shared by the tests of the module)."""
    if dt not in fx.packed:
        fx.packed[dt] = (encoders.PackedVit(fx.vw, fx.vcfg, "cuda", dt), encoders.PackedBert(fx.bw, fx.bcfg, "cuda", dt))
    return fx.packed[dt]


def _check_against_oracle(tc, tt, oc, ot, dt, what=""):
    assert torch.isfinite(tc).all() and torch.isfinite(tt).all()
    e0v, e0b = _rel(tc[:, 0], oc[:, 0]), _rel(tt[:, 0], ot[:, 0])
    print(f"{what} tap 0: ViT {e0v:.3e} BERT {e0b:.3e}")
    assert e0v < TAP0_VIT, (what, e0v)
    assert e0b < TAP0_BERT, (what, e0b)
    for l in range(1, max(oc.shape[1], ot.shape[1])):
        if l < oc.shape[1]:
            ev = _rel(tc[:, l], oc[:, l])
            print(f"{what} tap {l}: ViT {ev:.3e}")
            assert ev < TAP_TOL[dt], f"{what} ViT tap {l}: {ev:.3e}"
        if l < ot.shape[1]:
            eb = _rel(tt[:, l], ot[:, l])
            print(f"{what} tap {l}: BERT {eb:.3e}")
            assert eb < TAP_TOL[dt], f"{what} BERT tap {l}: {eb:.3e}"


# ---- 1. toy towers, every entry point ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", [1, 2, 5])
@pytest.mark.parametrize("dt", [_lib.IISAN_F16, _lib.IISAN_BF16])
def test_toy_narrow_towers_match_the_oracle(toy, dt, M):
    """Taps {0, 1, 2} of a 192- / 384-wide 2-layer ViT (3 heads: one head per attention workgroup; 6 heads) and a 128- / 256-wide BERT,
    batches far below one GEMM tile, an all-padding item and a title whose mask ends at 5 words among them; a subset of taps, a chunked
    run and the same rows inside a larger batch return the same bits."""
    vit, bert = _packed(toy, dt)
    Dv, Db = toy.vcfg.hidden, toy.bcfg.hidden
    img, txt = toy.images[:M].contiguous().cuda(), toy.text[:M].contiguous().cuda()
    assert img[0].abs().max() == 0 and txt[0].abs().max() == 0
    tc, tt = vit.forward_taps(img, [0, 1, 2]).cpu(), bert.forward_taps(txt, [0, 1, 2]).cpu()
    assert tc.shape == (M, 3, Dv) and tt.shape == (M, 3, Db)
    _check_against_oracle(tc, tt, toy.oc[:M], toy.ot[:M], dt, f"toy {Dv}+{Db} dt {dt} M {M}")
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
def test_toy_narrow_towers_with_the_fp32_residual_stream(lib, toy, dt):
    """Dev switch resid32 = 1 (the whole stream in fp32: `layernorm768_kernel` at the narrow widths instead of the mixed kernel, the
    fp32-residual patch epilogue on a ragged tile at 192): the same tolerance, and really another route."""
    vit, bert = _packed(toy, dt)
    img, txt = toy.images[:5].contiguous().cuda(), toy.text[:5].contiguous().cuda()
    mc, mt = vit.forward_taps(img, [0, 1, 2]).cpu(), bert.forward_taps(txt, [0, 1, 2]).cpu()
    with _lib.dev(resid32=1):
        tc, tt = vit.forward_taps(img, [0, 1, 2]).cpu(), bert.forward_taps(txt, [0, 1, 2]).cpu()
        fc, ft = vit.forward_taps(img, [0, 1, 2], chunk_items=2).cpu(), bert.forward_taps(txt, [0, 1, 2], chunk_items=2).cpu()
    _check_against_oracle(tc, tt, toy.oc[:5], toy.ot[:5], dt, f"toy {toy.vcfg.hidden}+{toy.bcfg.hidden} resid32 dt {dt}")
    assert torch.equal(fc, tc) and torch.equal(ft, tt)
    assert torch.equal(tc[:, 0], mc[:, 0]) and torch.equal(tt[:, 0], mt[:, 0])       # tap 0 is the embedding on either route
    assert not torch.equal(tc, mc) and not torch.equal(tt, mt)


def test_toy_narrow_full_blocks_against_the_cls_only_last_block(lib, toy):
    """full_blocks 1 against 0: the shallower taps bit-equal, the last one within 5e-4."""
    vit, bert = _packed(toy, _lib.IISAN_F16)
    img, txt = toy.images.cuda(), toy.text.cuda()
    with _lib.dev(full_blocks=1):
        fc, ft = vit.forward_taps(img, [0, 1, 2]).cpu(), bert.forward_taps(txt, [0, 1, 2]).cpu()
    pc, pt = vit.forward_taps(img, [0, 1, 2]).cpu(), bert.forward_taps(txt, [0, 1, 2]).cpu()
    assert torch.equal(pc[:, :2], fc[:, :2]) and torch.equal(pt[:, :2], ft[:, :2])
    ev, eb = _rel(pc[:, 2], fc[:, 2]), _rel(pt[:, 2], ft[:, 2])
    print(f"toy {toy.vcfg.hidden}+{toy.bcfg.hidden} cls-only vs full, tap 2: ViT {ev:.3e} BERT {eb:.3e}")
    assert ev < CLS_ONLY_TOL and eb < CLS_ONLY_TOL, (ev, eb)
    _check_against_oracle(fc, ft, toy.oc, toy.ot, _lib.IISAN_F16, f"toy {toy.vcfg.hidden}+{toy.bcfg.hidden} full_blocks")


def test_toy_narrow_u8_and_indexed_entries_equal_the_direct_ones(toy):
    """The u8 entry against the fp32 entry on the normalised image; the two indexed entries against the direct ones, an out-of-range
    index as the padding slot (zero normalised image; zero ids and mask)."""
    vit, bert = _packed(toy, _lib.IISAN_F16)
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


def test_toy_narrow_dropout_entry_without_dropout_is_the_eval_entry(lib, toy):
    """`iisan_bert_forward_taps_dropout` with drop == NULL, and with both probabilities 0: the bits of the eval entry."""
    _, bert = _packed(toy, _lib.IISAN_F16)
    txt = toy.text.cuda()
    want = bert.forward_taps(txt, [0, 1, 2])
    M = txt.shape[0]
    tl = (C.c_int32 * 3)(0, 1, 2)
    nbytes = lib.iisan_bert_forward_taps_ws_bytes(C.byref(bert.struct), M, WORDS, 0)
    ws = torch.empty(int(nbytes), dtype=torch.uint8, device="cuda")
    for drop in (None, C.byref(_lib.BertDropout(0.0, 0.0, 77))):
        taps = torch.full((M, 3, toy.bcfg.hidden), float("nan"), device="cuda")
        _lib.check(lib.iisan_bert_forward_taps_dropout(C.byref(bert.struct), txt.data_ptr(), 0, None, M, WORDS, tl, 3, taps.data_ptr(), 0,
                                                       drop, ws.data_ptr(), ws.numel(), _stream()), "iisan_bert_forward_taps_dropout")
        torch.cuda.synchronize()
        assert torch.equal(taps, want)


# ---- 2. real geometry through every GEMM family ------------------------------------------------------------------------------------

@pytest.fixture
def gemm_variant(lib, request):
    _lib.dev_set("gemm16_variant", request.param)
    yield request.param
    _lib.dev_set("gemm16_variant", 0)


@pytest.mark.parametrize("gemm_variant", [0, 1, 3, 4], indirect=True)
def test_real_geometry_taps_match_the_oracle_on_every_gemm_family(full, gemm_variant):
    """ViT-tiny geometry (197 tokens, 3 heads, mlp 768) on 3 images, 4 layers, and BERT-tiny (30 words) on 4 titles, all taps, once per
    GEMM kernel family switch.  The 192- and 576-column products of the 192-wide tower have a ragged last column tile: the 128x128 kernel
    under every variant (a forced 256x256 kernel takes only the 768-column FC1)."""
    vit, bert = _packed(full, _lib.IISAN_F16)
    lv, lb = list(range(5)), list(range(3))
    img, txt = full.images.cuda(), full.text.cuda()
    _lib.dev_set("count:gemm16_v1", 0)
    tc = vit.forward_taps(img, lv).cpu()
    assert _lib.dev_get("count:gemm16_v1") > 0
    tt = bert.forward_taps(txt, lb).cpu()
    assert tc.shape == (3, 5, 192) and tt.shape == (4, 3, 128)
    _check_against_oracle(tc, tt, full.oc, full.ot, _lib.IISAN_F16, f"real variant {gemm_variant}")
    # S = 197 goes to the DMA attention kernel by default; attention16_kernel gives the same bits, as at 768
    _lib.dev_set("count:attn16_dma", 0)
    assert torch.equal(vit.forward_taps(img, lv).cpu(), tc)
    assert _lib.dev_get("count:attn16_dma") > 0
    with _lib.dev(attn_route=1):
        _lib.dev_set("count:attn16_dma", 0)
        assert torch.equal(vit.forward_taps(img, lv).cpu(), tc)
        assert _lib.dev_get("count:attn16_dma") == 0


# ---- 3. the LayerNorm primitive: several rows per wave -----------------------------------------------------------------------------

@pytest.mark.parametrize("rows", [1, 7, 8, 9, 1001])
@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("width", [128, 192, 256, 384])
def test_layernorm_narrow_widths_vs_torch(lib, width, dt, rows):
    """`iisan_layernorm` at 32 x 1, 16 x 3, 64 x 1 and 32 x 3 lanes x pieces per row (2 / 4 / 1 / 2 rows per wave): against float64
    `layer_norm`, a guard row behind each output, the fp32 output in place — the bounds of test_layernorm_width_1024_vs_torch."""
    g = torch.Generator().manual_seed(3 + width)
    x = torch.randn(rows, width, generator=g) * 3 + 0.7
    w = 1 + 0.1 * torch.randn(width, generator=g)
    b = 0.1 * torch.randn(width, generator=g)
    ref = torch.nn.functional.layer_norm(x.double(), (width,), w.double(), b.double(), 1e-12)
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    o16 = torch.empty(rows + 1, width, dtype=T16[dt], device="cuda").fill_(7.0)        # one guard row behind each output
    o32 = torch.empty(rows + 1, width, dtype=torch.float32, device="cuda").fill_(7.0)
    _lib.check(lib.iisan_layernorm(dt, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), 1e-12, o16.data_ptr(), o32.data_ptr(), rows, width,
                                   _stream()), f"layernorm {width}")
    torch.cuda.synchronize()
    e32 = (o32[:rows].cpu().double() - ref).abs().max().item() / ref.abs().max().item()
    e16 = (o16[:rows].cpu().double() - ref).abs().max().item() / ref.abs().max().item()
    print(f"layernorm width {width} dt {dt} rows {rows}: fp32 {e32:.3e} 16-bit {e16:.3e}")
    assert (o32[:rows].cpu().double() - ref).abs().max().item() < 5e-6 * ref.abs().max().item() + 1e-5
    assert (o16[:rows].cpu().double() - ref).abs().max().item() < LN16_TOL[dt] * ref.abs().max().item()
    assert (o32[rows] == 7.0).all() and (o16[rows] == 7.0).all()
    # in-place fp32 output
    _lib.check(lib.iisan_layernorm(dt, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), 1e-12, None, xd.data_ptr(), rows, width, _stream()),
               f"layernorm {width} in place")
    torch.cuda.synchronize()
    assert (xd.cpu().double() - ref).abs().max().item() < 5e-6 * ref.abs().max().item() + 1e-5


# ---- 4. the GEMM primitive: a ragged last column tile ------------------------------------------------------------------------------

def _ragged_operands(M, N, K, dt, seed):
    """A [Mpad, K] (whole 256-row tiles, as the entry asks), W and bias as the LEADING N rows of buffers whose remaining rows are NaN:
    a read past row N - 1 that reaches an accumulator, or a bias read past N, shows up as a NaN in the output."""
    g = torch.Generator().manual_seed(seed)
    A = (torch.randn(M, K, generator=g) * 0.5).to(T16[dt])
    W = (torch.randn(N, K, generator=g) * 0.05 + torch.linspace(-0.02, 0.03, N)[:, None]).to(T16[dt])
    bias = torch.randn(N, generator=g) * 0.3
    Mp = (M + 255) // 256 * 256
    Ad = torch.zeros(Mp, K, dtype=T16[dt], device="cuda")
    Ad[:M] = A.cuda()
    Wd = torch.full((N + 130, K), float("nan"), dtype=T16[dt], device="cuda")
    Wd[:N] = W.cuda()
    bd = torch.full((N + 130,), float("nan"), dtype=torch.float32, device="cuda")
    bd[:N] = bias.cuda()
    ref = A.double() @ W.double().t() + bias.double()
    return Ad, Wd, bd, ref


@pytest.mark.parametrize("M", [1, 129, 300])
@pytest.mark.parametrize("K", [128, 192, 768])
@pytest.mark.parametrize("N", [64, 192, 576])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("dt", [0, 1])
def test_gemm16_ragged_last_column_tile(lib, dt, mode, N, K, M):
    """N % 128 == 64 on the 128x128 kernel (plain and GELU epilogues): against a float64 product of the rounded operands, no NaN from the
    rows behind W and bias, guard columns (ldo = N + 72) and a guard row intact."""
    Ad, Wd, bd, ref = _ragged_operands(M, N, K, dt, seed=M * 7 + N + K + mode)
    if mode == 1:
        ref = torch.nn.functional.gelu(ref)
    ldo = N + 72
    out = torch.full((M + 1, ldo), 7.0, dtype=T16[dt], device="cuda")
    _lib.dev_set("count:gemm16_v1", 0)
    _lib.check(lib.iisan_gemm16_ld(dt, mode, Ad.data_ptr(), Wd.data_ptr(), bd.data_ptr(), out.data_ptr(), M, N, K, K, K, ldo, _stream()),
               "gemm16_ld")
    torch.cuda.synchronize()
    assert _lib.dev_get("count:gemm16_v1") == 1
    got = out.cpu().double()
    assert not torch.isnan(got).any()
    assert (got[:M, N:] == 7.0).all() and (got[M] == 7.0).all()
    err, scale = (got[:M, :N] - ref).abs().max().item(), ref.abs().max().item()
    print(f"gemm16 ragged dt {dt} mode {mode} M {M} N {N} K {K}: {err / scale:.3e}")
    assert err <= GEMM_TOL[dt] * scale, f"max err {err:.3e} > {GEMM_TOL[dt] * scale:.3e}"


@pytest.mark.parametrize("M", [5, 300])
def test_gemm16_ragged_head_major_qkv_and_fp32_residual(lib, M):
    """The head-major QKV epilogue at N = 576 (3 heads, S = 5): the float64 product scattered on the host into [item][head][q|k|v][S][64];
    and the fp32-residual epilogue (mode 2, in place) at N = 192."""
    N, K, S, heads = 576, 192, 5, 3
    Ad, Wd, bd, ref = _ragged_operands(M, N, K, 0, seed=11 + M)
    assert M % S == 0
    items = M // S
    out = torch.full((items * heads * 3 * S * 64 + 64,), 7.0, dtype=torch.float16, device="cuda")
    _lib.check(lib.iisan_gemm16_lna(4, Ad.data_ptr(), Wd.data_ptr(), bd.data_ptr(), out.data_ptr(), None, M, N, K, S, _stream()), "gemm16 qkv")
    torch.cuda.synchronize()
    got = out.cpu().double()
    assert not torch.isnan(got).any() and (got[-64:] == 7.0).all()
    # ref [M, 3 * 192] = [item, tok, which, head, d] -> [item, head, which, tok, d]
    want = ref.view(items, S, 3, heads, 64).permute(0, 3, 2, 1, 4).contiguous().view(-1)
    err, scale = (got[:-64] - want).abs().max().item(), want.abs().max().item()
    print(f"gemm16 ragged head-major QKV M {M}: {err / scale:.3e}")
    assert err <= GEMM_TOL[0] * scale
    # mode 2: out32 = acc + bias + resid32, in place
    N2 = 192
    Ad, Wd, bd, ref = _ragged_operands(M, N2, K, 0, seed=13 + M)
    g = torch.Generator().manual_seed(M)
    resid = torch.randn(M, N2, generator=g)
    o32 = torch.full((M + 1, N2), 7.0, device="cuda")
    o32[:M] = resid.cuda()
    _lib.check(lib.iisan_gemm16(0, 2, Ad.data_ptr(), Wd.data_ptr(), bd.data_ptr(), o32.data_ptr(), o32.data_ptr(), M, N2, K, _stream()), "gemm16 resid32")
    torch.cuda.synchronize()
    got = o32.cpu().double()
    want = ref + resid.double()
    assert not torch.isnan(got).any() and (got[M] == 7.0).all()
    err, scale = (got[:M] - want).abs().max().item(), want.abs().max().item()
    print(f"gemm16 ragged fp32 residual M {M}: {err / scale:.3e}")
    assert err <= 2e-5 * scale


# ---- 5. refusals: an error code and a message, nothing launched --------------------------------------------------------------------

@pytest.mark.parametrize("hidden,heads", [(192, 4), (320, 5)])
def test_unsupported_narrow_shapes_are_refused(lib, hidden, heads):
    vcfg = weights.VitConfig(hidden=hidden, layers=1, heads=heads, mlp=128, image=32, patch=16)
    bcfg = weights.BertConfig(hidden=hidden, layers=1, heads=heads, mlp=128, vocab=64, max_pos=32)
    vit = encoders.PackedVit(weights.make_vit_weights(vcfg, seed=1), vcfg, "cuda")
    bert = encoders.PackedBert(weights.make_bert_weights(bcfg, seed=2), bcfg, "cuda")
    fam = ("gemm16_h256", "gemm16_s256", "gemm16_v1")
    for n in fam:
        _lib.dev_set("count:" + n, 0)
    taps = {}
    for name, enc, x in (("vit", vit, torch.zeros(2, 3, 32, 32, device="cuda")), ("bert", bert, torch.zeros(2, 16, dtype=torch.int64, device="cuda"))):
        with pytest.raises(_lib.IisanHipError, match=str(hidden)):
            taps[name] = enc.forward_taps(x, [0, 1])
    assert sum(_lib.dev_get("count:" + n) for n in fam) == 0


def test_narrow_bert_refuses_dropout_and_narrow_vit_has_no_folded_set(lib):
    vcfg, bcfg = _toy_cfgs("192+128")
    vit = encoders.PackedVit(weights.make_vit_weights(vcfg, seed=1), vcfg, "cuda")
    bert = encoders.PackedBert(weights.make_bert_weights(bcfg, seed=2), bcfg, "cuda")
    txt = torch.zeros(2, 2 * WORDS, dtype=torch.int64, device="cuda")
    fam = ("gemm16_h256", "gemm16_s256", "gemm16_v1")
    for n in fam:
        _lib.dev_set("count:" + n, 0)
    with pytest.raises(_lib.IisanHipError, match="128"):
        bert.forward_taps(txt, [0, 1, 2], dropout=(0.1, 0.1, 5))
    with pytest.raises(_lib.IisanHipError, match="128"):
        bert.forward_taps(txt, [0, 1, 2], dropout=(0.0, 0.1, 5))
    assert sum(_lib.dev_get("count:" + n) for n in fam) == 0
    assert lib.iisan_vit_fold_bytes(C.byref(vit.struct)) == 0
    assert not vit.struct.folded and vit.struct.layer[0].qkv_w32 is None
