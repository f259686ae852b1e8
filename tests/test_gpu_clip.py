"""GPU tests of the frozen CLIP vision tower: the quick-GELU epilogue (mode 8) of the encoder GEMM as a primitive, the towers of the
HuggingFace golden (tests/golden/clip_vit.npz) through every entry point, the production kernels on a CLIP-B/32 batch, and the model on
top (`ClipVit_Encoder` through `ModelMM`, `evaluate.build_tap_cache`, a Versa step).  Host side: tests/test_clip_host.py."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import clip_oracle as CO  # noqa: E402
import helpers  # noqa: E402
from iisan_amd import _lib, encoders, evaluate, synth, tapstore, weights  # noqa: E402
from oracle import iisan_oracle as O  # noqa: E402
from test_gpu_blk32 import deblock  # noqa: E402

F16, BF16 = _lib.IISAN_F16, _lib.IISAN_BF16
T16 = {F16: torch.float16, BF16: torch.bfloat16}
PRIM_TOL = {F16: 2e-3, BF16: 1.6e-2}        # tests/test_gpu_primitives.py: relative to the output scale, one 16-bit rounding of the result
TAP_TOL = {F16: 1.5e-3, BF16: 1.2e-2}       # tests/test_gpu_encoders.py: test_full_size_taps_match_reference_golden
GELU16, QGELU16 = _lib.EPI_GELU16, _lib.EPI_QGELU16
H256_M = 127 * 256 + 1                      # with N = 256, K = 128: the smallest product the auto policy sends to gemm16_h256 (128 tiles)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm()).item()


# ---- c. the epilogue primitive ---------------------------------------------------------------------------------------------------------

def _operands(M, N, K, dt):
    g = torch.Generator().manual_seed(M * 7 + N + K)
    A = (torch.randn(M, K, generator=g) * 0.5).to(T16[dt])
    # rows of W with an offset and a wide bias: pre-activations over about [-6, 6], where quick-GELU and erf-GELU differ by up to 2e-2
    W = (torch.randn(N, K, generator=g) * 0.2 + torch.linspace(-0.02, 0.03, N)[:, None]).to(T16[dt])
    bias = torch.randn(N, generator=g) * 0.5
    pre = A.double() @ W.double().t() + bias.double()
    Ap = torch.zeros((M + 255) // 256 * 256, K, dtype=T16[dt])
    Ap[:M] = A
    return Ap.cuda(), W.cuda(), bias.cuda(), pre


def _check_quick_gelu(got, pre, dt, what):
    """`got` against float64 quick_gelu(pre) at the bound of the mode-1 primitive test — and the negative control: erf-GELU of the same
    pre-activations must FAIL the same check.  The control is an fp16 statement: the two activations differ by up to 2.1e-2 (near
    |x| = 2.2), the bound is 2e-3 of an output scale of 1.8 to 6.7 here; the bf16 bound, 1.6e-2 of the scale — one bf16 rounding of the
    result — is wider than that difference at any scale above 1.3, so no max-error check at that bound can tell the two apart."""
    ref = CO.quick_gelu(pre)
    scale = ref.abs().max().item()
    err = (got.double().cpu() - ref).abs().max().item()
    print(f"{what}: max err {err:.3e}, bound {PRIM_TOL[dt] * scale:.3e}")
    assert err <= PRIM_TOL[dt] * scale, f"{what}: max err {err:.3e} > {PRIM_TOL[dt] * scale:.3e}"
    if dt == F16:
        erf = torch.nn.functional.gelu(pre).to(T16[dt]).double()
        assert (erf - ref).abs().max().item() > PRIM_TOL[dt] * scale, f"{what}: the check would accept erf-GELU"
    return scale


@pytest.mark.parametrize("dt", [F16, BF16])
@pytest.mark.parametrize("K", [64, 128])
@pytest.mark.parametrize("N", [128, 192])
@pytest.mark.parametrize("M", [1, 37, 300])
def test_quick_gelu_epilogue_on_the_128_kernel(lib, dt, M, N, K):
    """iisan_gemm16 mode 8 on the 128x128 kernel: one row, a ragged row tile, three row tiles; whole column tiles and the ragged N % 128 == 64
    tile; one and two K-steps."""
    A, W, bias, pre = _operands(M, N, K, dt)
    assert lib.iisan_gemm16_route(dt, QGELU16, M, N, K, 0, 0, 0, 0) == 0
    out = torch.full((M, N), float("nan"), dtype=T16[dt], device="cuda")
    before = _lib.dev_get("count:gemm16_v1")
    _lib.check(lib.iisan_gemm16(dt, QGELU16, A.data_ptr(), W.data_ptr(), bias.data_ptr(), out.data_ptr(), None, M, N, K, _stream()), "gemm16")
    torch.cuda.synchronize()
    assert _lib.dev_get("count:gemm16_v1") == before + 1
    scale = _check_quick_gelu(out, pre, dt, f"v1 dt={dt} {M}x{N}x{K}")
    # the control again on the device: mode 1 of the same product does not pass as mode 8
    erf = torch.empty_like(out)
    _lib.check(lib.iisan_gemm16(dt, GELU16, A.data_ptr(), W.data_ptr(), bias.data_ptr(), erf.data_ptr(), None, M, N, K, _stream()), "gemm16")
    assert dt != F16 or (erf.double().cpu() - CO.quick_gelu(pre)).abs().max().item() > PRIM_TOL[dt] * scale
    assert not torch.equal(erf, out)


@pytest.mark.parametrize("dt", [F16, BF16])
def test_quick_gelu_epilogue_on_the_256_kernel_plain_and_block_major(lib, dt):
    """The smallest (M, N, K) iisan_gemm16_route sends to gemm16_h256 — 128 tiles of 256 x 256 with a last row tile of ONE row, K = 128: a
    first and a last K-step — through iisan_gemm16, and once more with a block-major output through iisan_gemm16_blk32: the same words
    where the block-major layout puts them, pad rows untouched."""
    M, N, K = H256_M, 256, 128
    assert lib.iisan_gemm16_route(dt, QGELU16, M, N, K, 0, 0, 0, 0) == 2 and lib.iisan_gemm16_route(dt, QGELU16, M - 1, N, K, 0, 0, 0, 0) == 0
    assert lib.iisan_gemm16_route(dt, QGELU16, M, N, 64, 0, 0, 0, 0) == 0          # (one K-step: not on this kernel)
    A, W, bias, pre = _operands(M, N, K, dt)
    out = torch.full((M, N), float("nan"), dtype=T16[dt], device="cuda")
    before = _lib.dev_get("count:gemm16_h256"), _lib.dev_get("count:gemm16_blk32")
    _lib.check(lib.iisan_gemm16(dt, QGELU16, A.data_ptr(), W.data_ptr(), bias.data_ptr(), out.data_ptr(), None, M, N, K, _stream()), "gemm16")
    torch.cuda.synchronize()
    _check_quick_gelu(out, pre, dt, f"h256 dt={dt}")
    Mp = A.shape[0]
    nan16 = 0x7E00 if dt == F16 else 0x7FC0
    blk = torch.full((Mp, N), nan16, dtype=torch.int16, device="cuda")
    _lib.check(lib.iisan_gemm16_blk32(dt, QGELU16, A.data_ptr(), W.data_ptr(), bias.data_ptr(), blk.data_ptr(), None, M, N, K, 0, 1, _stream()), "gemm16_blk32")
    torch.cuda.synchronize()
    assert (_lib.dev_get("count:gemm16_h256"), _lib.dev_get("count:gemm16_blk32")) == (before[0] + 2, before[1] + 1)
    rows = deblock(blk, Mp, N)
    assert torch.equal(rows[:M], out.view(torch.int16)), "block-major output differs from the row-major one"
    assert (rows[M:] == nan16).all(), "pad rows of the block-major output were written"
    _check_quick_gelu(rows[:M].view(T16[dt]), pre, dt, f"h256 block-major dt={dt}")


# ---- d. the towers ---------------------------------------------------------------------------------------------------------------------

# beside the golden's towers: 14-pixel patches on an image the uint8 entries take (a side that is a multiple of 8 and of 14) — the padded
# patch extraction with a source index and with statistics; no golden, the uint8 tests compare entry points with each other
P14 = weights.VitConfig(hidden=128, layers=2, heads=2, mlp=256, image=56, patch=14, eps=1e-5, pre_ln=True, act="quick_gelu", patch_bias=False)


@functools.lru_cache(maxsize=None)
def _tower(name, dt=F16):
    if name == "p14":
        w = weights.make_vit_weights(P14, seed=59)
        return P14, w, None, None, encoders.PackedVit(w, P14, "cuda", dt)
    cfg, w, x, gold = CO.load_golden(name)
    return cfg, w, x, gold, encoders.PackedVit(w, cfg, "cuda", dt)


def _u8_images(n, res, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, 3, res, res), generator=g, dtype=torch.uint8)


@pytest.mark.parametrize("dt", [F16, BF16])
@pytest.mark.parametrize("name", sorted(CO.TOWERS))
def test_clip_taps_match_the_huggingface_golden(name, dt):
    """Every CLS tap of the three golden towers against HF's own hidden states, per tap layer, at the project's tap bound.

    Measured on MI355X (fp16 / bf16, |got - ref| / |ref| per layer) and the CPU emulation of 16-bit operand rounding alone: profiles/clip_tower.md."""
    cfg, w, x, gold, pk = _tower(name, dt)
    layers = list(range(cfg.layers + 1))
    got = pk.forward_taps(x.cuda(), layers).cpu()
    assert torch.isfinite(got).all() and pk.struct.folded is None and pk.struct.act == (1 if cfg.act == "quick_gelu" else 0)
    errs = CO.tap_errors(got, gold)
    print(f"{name} dt={dt} tap errors: " + " ".join(f"{e:.2e}" for e in errs))
    # tap 0 is LN_pre(cls + pos[0]) in fp32: no 16-bit arithmetic touches the CLS row before block 0
    assert errs[0] < 1e-5, errs[0]
    for l, e in enumerate(errs):
        assert e < TAP_TOL[dt], f"{name} tap {l}: {e:.3e}"
    # a subset of the taps is the same rows; a call that taps hidden state 0 alone runs the pre-LayerNorm on the CLS rows only
    sel = [0, cfg.layers]
    assert torch.equal(pk.forward_taps(x.cuda(), sel).cpu(), got[:, sel])
    assert torch.equal(pk.forward_taps(x.cuda(), [0]).cpu(), got[:, [0]])
    # the padding image (all zero, item 0) is an item like any other
    assert got[0].abs().max() > 0


@pytest.mark.parametrize("name", ["b32", "gelutoy", "p14"])
def test_clip_entry_points_chunks_and_pad_slots_are_bit_equal(name):
    """fp32 / uint8 / uint8-indexed entries give the same bits; padding index slots give the zero-image taps; chunk_items changes nothing."""
    cfg, w, _, _, pk = _tower(name)
    layers = list(range(cfg.layers + 1))
    u8 = _u8_images(5, cfg.image, 91)
    f32 = ((u8.float().div(255) - 0.5) / 0.5).cuda()          # torchvision ToTensor + Normalize, on the CPU: IEEE divisions, as in the kernel
    u8 = u8.cuda()
    t32 = pk.forward_taps(f32.contiguous(), layers)
    t8 = pk.forward_taps(u8, layers)
    assert torch.equal(t32, t8)
    index = torch.tensor([3, -1, 0, 4, 4, 5, 1, 2], device="cuda")          # pads: negative and == rows
    ti = pk.forward_taps_indexed(u8, index, layers)
    zero = pk.forward_taps(torch.zeros(1, 3, cfg.image, cfg.image, device="cuda"), layers)
    want = torch.stack([t8[i] if 0 <= i < 5 else zero[0] for i in index.tolist()])
    assert torch.equal(ti, want)
    for chunk in (1, 3):
        assert torch.equal(pk.forward_taps(u8, layers, chunk_items=chunk), t8)
        assert torch.equal(pk.forward_taps_indexed(u8, index, layers, chunk_items=chunk), ti)
    # the dev switch of the fp32 stream runs a CLIP tower too (the pre-LayerNorm as a launch of its own), inside the tap bound of the mixed one
    with _lib.dev(resid32=1):
        r32 = pk.forward_taps(u8, layers)
    e32 = CO.tap_errors(r32, t8)
    assert e32[0] < 1e-5 and max(e32) < TAP_TOL[F16], e32
    # ln_fold selects nothing for a CLIP tower, at 768 either
    for lf in (0, 1):
        with _lib.dev(ln_fold=lf):
            assert torch.equal(pk.forward_taps(u8, layers), t8)


def test_clip_cls_only_last_block_matches_full_blocks():
    """Shallower taps with the CLS-only last block are bit-equal to full_blocks = 1; the tap the CLS-only block produces is within the 5e-4
    of test_cls_only_last_block_matches_full_blocks; blocks past the deepest tap are not run."""
    cfg, w, x, gold, pk = _tower("b32")
    xs = x.cuda()
    layers = list(range(cfg.layers + 1))
    pk.full_blocks = True
    try:
        full = pk.forward_taps(xs, layers)
    finally:
        pk.full_blocks = False
    pruned = pk.forward_taps(xs, layers)
    assert torch.equal(pruned[:, :-1], full[:, :-1]) and _rel(pruned[:, -1], full[:, -1]) < 5e-4
    short = pk.forward_taps(xs, [0, 1, 3])
    assert torch.equal(short[:, :2], full[:, [0, 1]]) and _rel(short[:, 2], full[:, 3]) < 5e-4
    assert _rel(short[:, 2], gold[:, 3]) < TAP_TOL[F16]
    cfg2, _, x2, gold2, pk2 = _tower("l14toy", BF16)
    one = pk2.forward_taps(x2.cuda(), [1])          # block 0 is the CLS-only block: K / V of x0 from the opening kernel's image
    assert _rel(one[:, 0], gold2[:, 1]) < TAP_TOL[BF16]


@pytest.mark.parametrize("name", ["b32", "p14"])
def test_clip_statistics_on_the_uint8_route_equal_host_normalisation(name):
    """Non-default per-channel statistics (OpenAI's) on the uint8 and the indexed entry = the fp32 entry fed with (p / 255 - mean) / std
    computed in fp32 on the host; patch 32 takes the 8-pixel extraction kernel, patch 14 the padded one.  All-zero statistics are the
    (.5, .5) transform."""
    cfg, w, _, _, pk = _tower(name)
    ncfg = dataclasses.replace(cfg, norm_mean=weights.CLIP_MEAN, norm_std=weights.CLIP_STD)
    pkn = encoders.PackedVit(w, ncfg, "cuda")
    layers = [0, cfg.layers]
    u8 = _u8_images(3, cfg.image, 92)
    # on the CPU: IEEE fp32 divisions, as in the kernel (a division by a scalar on the device is a multiplication by its reciprocal)
    mean, std = torch.tensor(weights.CLIP_MEAN).view(1, 3, 1, 1), torch.tensor(weights.CLIP_STD).view(1, 3, 1, 1)
    host = ((u8.float().div(255) - mean) / std).contiguous().cuda()
    u8 = u8.cuda()
    want = pkn.forward_taps(host, layers)
    got = pkn.forward_taps(u8, layers)
    assert torch.equal(got, want)
    assert not torch.equal(got, pk.forward_taps(u8, layers))
    index = torch.tensor([2, 7, 0, 1, -5], device="cuda")
    zero = pkn.forward_taps(torch.zeros(1, 3, cfg.image, cfg.image, device="cuda"), layers)
    assert torch.equal(pkn.forward_taps_indexed(u8, index, layers), torch.stack([want[2], zero[0], want[0], want[1], zero[0]]))
    # a zero std beside set statistics is refused before any launch
    bad = encoders.PackedVit(w, dataclasses.replace(cfg, norm_mean=(0.5, 0.5, 0.5), norm_std=(0.5, 0.0, 0.5)), "cuda")
    with pytest.raises(_lib.IisanHipError, match="norm_std"):
        bad.forward_taps(u8, layers)


# ---- e. the production kernels ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("f1_block_major", [False, True])
def test_clip_b32_batch_on_the_production_kernels_matches_the_128_kernel(lib, f1_block_major):
    """CLIP-B/32 shapes at toy depth (2 layers), every block on every token, against every GEMM forced onto the 128x128 kernel — at the
    smallest item count at which iisan_gemm16_route sends FC1 (50 tokens per item) to gemm16_h256, where every other product is still on the
    128x128 kernel and F1 row-major; and at the smallest count at which FC2 gets there too and the executor makes F1 block-major
    (iisan_encoder_plan, bit 4).  Both kernel families walk K in ascending order into fp32 accumulators: the bound is the 4e-4 of
    test_production_batch_dispatch_matches_the_golden_pinned_kernels, the expectation 0."""
    cfg = dataclasses.replace(weights.CLIP_VIT_B32, layers=2)
    route = lambda items: lib.iisan_gemm16_route(F16, QGELU16, items * 50, 3072, 768, 0, 0, 0, 0)
    plan = lambda items: lib.iisan_encoder_plan(_lib.IISAN_TOWER_CLIP, F16, 768, 12, 3072, 50, items, 0, 2, 1, 0)
    if f1_block_major:
        items = next(m for m in range(1, 4096) if plan(m) == (1 | 4))
        assert plan(items - 1) == 1
    else:
        items = next(m for m in range(1, 4096) if route(m) == 2)
        assert route(items - 1) == 0 and plan(items) == 1
    w = weights.make_vit_weights(cfg, seed=57)
    pk = encoders.PackedVit(w, cfg, "cuda")
    pk.full_blocks = True
    x = CO.images(items, cfg.image, 58).cuda()
    for c in ("gemm16_h256", "gemm16_blk32"):
        _lib.dev_set("count:" + c, 0)
    got = pk.forward_taps(x, [0, 1, 2])
    h256, blk = _lib.dev_get("count:gemm16_h256"), _lib.dev_get("count:gemm16_blk32")
    print(f"{items} items: {h256} launches of gemm16_h256, {blk} with a block-major operand")
    # FC1 of both blocks at least; block-major F1: written by both FC1 products, read by both FC2 products
    assert h256 >= 2 and blk == (4 if f1_block_major else 0), (items, h256, blk)
    with _lib.dev(gemm16_variant=1):
        _lib.dev_set("count:gemm16_h256", 0)
        ref = pk.forward_taps(x, [0, 1, 2], chunk_items=64)
        assert _lib.dev_get("count:gemm16_h256") == 0
    assert torch.isfinite(got).all() and torch.equal(got[:, 0], ref[:, 0])
    for k in (1, 2):
        d = _rel(got[:, k], ref[:, k])
        print(f"production vs 128x128, tap {k}: {d:.3e}")
        assert d < 4e-4, f"tap {k}: {d:.3e}"
        per = ((got[:, k] - ref[:, k]).norm(dim=1) / ref[:, k].norm(dim=1)).max().item()
        assert per < 4e-4, f"tap {k}: one slot off by {per:.3e}"
    # against float64 on a few items, so that the pair is not wrong together
    want = CO.clip_cls_taps(x[:3].cpu(), w, cfg)
    assert max(CO.tap_errors(got[:3], want)) < TAP_TOL[F16]


# ---- f. the model ----------------------------------------------------------------------------------------------------------------------

E2E_CLIP = weights.VitConfig(hidden=768, layers=2, heads=12, mlp=512, image=32, patch=16, eps=1e-5, pre_ln=True, act="quick_gelu", patch_bias=False)
E2E_BERT = weights.BertConfig(hidden=768, layers=2, heads=12, mlp=512, vocab=512, max_pos=64)


def test_uncached_model_with_a_clip_tower_matches_the_float64_oracle():
    """`ModelMM` Uncached, args.CV_model_load = "clip-vit-base-patch32": MM_Encoder builds a ClipVit_Encoder, the side network consumes its
    taps.  Loss and the three item embeddings against `O.model_loss_from_taps` fed the float64 CLIP taps (and the oracle's BERT taps), at
    the bounds of the e2e_small test: 1e-3 relative (fp16 encoder operands)."""
    from iisan_amd.model import encoders as menc
    b = synth.scientific_batch(bs=3, seed=31, lengths=[3, 11, 6], dup_items=True, res=32, words=8, vocab=512, item_num=40)
    vw, bw = weights.make_vit_weights(E2E_CLIP, seed=13), weights.make_bert_weights(E2E_BERT, seed=12)
    P = weights.make_trainable_params(seed=101, n_side=3)
    args = helpers.make_args(side_adapter_vit_list="0,1", side_adapter_bert_list="0,1", num_words_title=8, drop_rate=0.0,
                             CV_model_load="clip-vit-base-patch32")
    model = helpers.build_model(args, 40, b.pop_prob, vw, E2E_CLIP, bw, E2E_BERT, cached=False)
    assert type(model.mm_encoder.cv_encoder) is menc.ClipVit_Encoder
    helpers.load_trainables(model, P)
    model.eval()
    ids, lm, img, txt = b.ids.cuda().view(-1), b.log_mask.cuda(), b.images.cuda(), b.text.cuda()
    cv, (text, mm) = model.mm_encoder(img, txt)
    loss = model(ids, img, txt, lm, 0)
    loss.backward()
    with torch.no_grad():
        tc = CO.clip_cls_taps(b.images, vw, E2E_CLIP).float()
        tt = O.bert_cls_taps(b.text, bw, E2E_BERT)
        ref, aux = O.model_loss_from_taps(b.ids, tc, tt, b.log_mask, b.pop_prob, P, O.side_layer_list("0,1", False))
    real = (b.ids.view(-1) != 0)
    for got, key in ((cv, "cv"), (text, "text"), (mm, "mm")):
        rel = ((got.detach().cpu().double() - aux[key].double())[real].norm() / aux[key].double()[real].norm()).item()
        print(f"{key}: rel {rel:.3e}")
        assert rel < 1e-3, f"{key}: rel {rel:.3e}"
    rel = abs(loss.item() - ref.item()) / abs(ref.item())
    print(f"loss {loss.item():.6f} oracle {ref.item():.6f} rel {rel:.2e}")
    assert rel < 1e-3
    # the tower's taps themselves, and: a plain-ViT reading of the same weights is NOT what ran
    taps = model.mm_encoder.cv_encoder.forward_taps(img, [0, 1, 2]).cpu()
    assert max(CO.tap_errors(taps, tc)) < TAP_TOL[F16]
    for n, p in model.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and torch.isfinite(p.grad).all(), n


def test_tap_cache_through_a_clip_tower_feeds_a_versa_step():
    """`evaluate.build_tap_cache` through the CLIP tower gives [N, L + 1, D]; a Versa model (image_embedding_dim 768) takes one training step
    on stores of those taps: loss against the oracle on the same taps (3e-5, tests/test_gpu_narrow_versa.py), finite gradients everywhere."""
    N, WORDS = 24, 8
    images = synth.make_images(np.arange(N), 32, seed=5)
    g = torch.Generator().manual_seed(6)
    text = torch.zeros(N, 2 * WORDS, dtype=torch.int64)
    for m in range(1, N):
        n = int(torch.randint(3, WORDS + 1, (1,), generator=g))
        text[m, :n] = torch.randint(1, 512, (n,), generator=g)
        text[m, WORDS:WORDS + n] = 1
    pop = synth.make_pop_prob(N - 1)
    args_u = helpers.make_args(side_adapter_vit_list="0,1", side_adapter_bert_list="0,1", num_words_title=WORDS, CV_model_load="clip-vit-base-patch32")
    vw, bw = weights.make_vit_weights(E2E_CLIP, seed=13), weights.make_bert_weights(E2E_BERT, seed=12)
    builder = helpers.build_model(args_u, N - 1, pop, vw, E2E_CLIP, bw, E2E_BERT, cached=False, device="cuda")
    taps_cv, taps_tx = evaluate.build_tap_cache(builder, images.cuda(), text.cuda(), batch=10)
    assert taps_cv.shape == (N, 3, 768) and taps_tx.shape == (N, 3, 768) and torch.isfinite(taps_cv).all()
    assert max(CO.tap_errors(taps_cv, CO.clip_cls_taps(images, vw, E2E_CLIP))) < TAP_TOL[F16]
    args = helpers.make_args(image_embedding_dim=768, text_embedding_dim=768, side_adapter_vit_list="1", side_adapter_bert_list="1",
                             image_layers=2, text_layers=2, drop_rate=0.0, adapter_dropout_rate=0.0)
    model = helpers.build_model(args, N - 1, pop, cached="versa", device="cuda")
    shapes = {n: tuple(p.shape) for n, p in model.named_parameters() if p.requires_grad}
    P = weights.fill_params_seeded(shapes, seed=555)
    helpers.load_trainables(model, P)
    model.train()
    lay_cv, lay_tx = model.mm_encoder.packed_layers()
    model.tap_stores = (tapstore.TapStore(taps_cv, lay_cv, "cuda", "fp32"), tapstore.TapStore(taps_tx, lay_tx, "cuda", "fp32"))
    ids_np, lm_np = synth.make_ids(3, 10, N - 1, np.random.RandomState(78), lengths=[5, 11, 3])
    ids, log_mask = torch.from_numpy(ids_np), torch.from_numpy(lm_np)
    bs, S = log_mask.shape
    loss = model(ids.view(-1).cuda(), None, None, log_mask.cuda(), 0)
    loss.backward()
    flat = ids.view(-1)
    real = (flat != 0).view(-1, 1, 1).float()
    oc, ot = taps_cv.cpu()[flat] * real, taps_tx.cpu()[flat] * real
    with torch.no_grad():
        cv, tx, mm = O.versa_side_network(oc, ot, P, O.side_layer_list("1", False), O.side_layer_list("1", False))
        score = torch.nn.functional.linear(torch.cat([cv, tx, mm], 1), P["com_dense.weight"], P["com_dense.bias"])
        prec = O.sasrec(score.view(bs, S + 1, 64)[:, :-1], log_mask, P, 2, 2).reshape(-1, 64)
        ref = O.inbatch_ce(ids, score, prec, log_mask, pop)
    assert abs(loss.item() - ref.item()) <= 3e-5 * abs(ref.item()), (loss.item(), ref.item())
    n_grads = sum(1 for n, p in model.named_parameters() if p.requires_grad and p.grad is not None and torch.isfinite(p.grad).all())
    assert n_grads == len(shapes) and n_grads > 20
