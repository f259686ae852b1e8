"""GPU tests of the opt-in train-mode dropout of the frozen BERT tower (`iisan_bert_forward_taps_dropout`: the attention kernel of
csrc/bert_drop.hip, the keep-functor instantiations of the row kernels of csrc/rowops.hip): the attention kernel with dropped
probabilities against fp64, the taps against the HF-pinned restatement of tests/test_bert_dropout_host.py fed the masks the kernels
draw, the bit-level properties of the mask convention, every train-mode kernel against its eval-mode twin, and the model switch.

Measured (MI355X): profiles/r8_bert_dropout.md."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import golden_io as gio  # noqa: E402
import helpers  # noqa: E402
from iisan_amd import _lib, encoders, evaluate, trainer, weights  # noqa: E402
from test_bert_dropout_host import bert_hidden_states_dropped, drop_masks, dropout_text  # noqa: E402

T16 = {0: torch.float16, 1: torch.bfloat16}
TOL = {0: 2e-3, 1: 1.6e-2}            # one 16-bit rounding of the result, relative to the output scale (tests/test_gpu_primitives.py)
TAP_TOL = {_lib.IISAN_F16: 1.5e-3, _lib.IISAN_BF16: 1.2e-2}      # tests/test_gpu_encoders.py
M, WORDS, P_DROP, SEED = 7, 30, 0.1, 0x1234_5678_9ABC


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm()).item()


# ---- 5. the attention primitive ---------------------------------------------------------------------------------------------------

def _attn_ref(qkv, key_bias, items, S, heads, keep):
    """fp64 drop(softmax(Q K^T / 8 + key_bias)) V: the keep factor multiplies the probabilities, the denominator is the undropped row's."""
    x = qkv.double().view(items, S, 3, heads, 64)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
    s = q @ k.transpose(-1, -2) / 8.0
    if key_bias is not None:
        s = torch.where((key_bias < 0)[:, None, None, :], torch.full_like(s, torch.finfo(torch.float32).min), s)
    p = torch.softmax(s, -1) * keep.double()
    return (p @ v).transpose(1, 2).reshape(items * S, heads * 64)


ATTN_CASES = [(3, 1, 2, False, 0.1), (2, 7, 12, True, 0.1), (5, 30, 12, True, 0.1), (2, 16, 2, False, 0.1), (2, 17, 2, True, 0.1),
              (2, 33, 3, True, 0.1), (2, 64, 2, False, 0.1), (1, 100, 2, True, 0.1), (1, 224, 2, False, 0.1), (5, 30, 12, True, 0.5),
              (1, 200, 2, True, 0.1)]          # 13 key tiles: the 16-key tail product (the key bias keeps the p = 0 comparison on attention16_kernel)


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("case", ATTN_CASES)
def test_attention16_dropout_vs_torch(lib, dt, case):
    items, S, heads, masked, p = case
    site, seed = 4, 987654321 + S
    g = torch.Generator().manual_seed(S * 13 + heads)
    D = heads * 64
    qkv = (torch.randn(items * S, 3 * D, generator=g) * 1.5).to(T16[dt])
    kb = None
    if masked:
        kb = torch.zeros(items, S)
        for i in range(items):
            kb[i, int(torch.randint(1, S + 1, (1,), generator=g)):] = -1.0
        kb[0, :] = -1.0                       # an all-masked (padding) item attends uniformly
    keep = helpers.drop_factors(seed, site, items * heads * S * S, p).view(items, heads, S, S)
    ref = _attn_ref(qkv, kb, items, S, heads, keep)
    kbd = kb.cuda() if kb is not None else None
    kbp = kbd.data_ptr() if kbd is not None else None
    qkvd = qkv.view(items, S, 3, heads, 64).permute(0, 3, 2, 1, 4).contiguous().cuda()      # head-major [items, heads, 3, S, 64]
    ctx = torch.empty(items * S, D, dtype=T16[dt], device="cuda")
    _lib.check(lib.iisan_attention16_dropout(dt, qkvd.data_ptr(), kbp, ctx.data_ptr(), items, S, heads, p, seed, site, 0, _stream()),
               "attention16_dropout")
    torch.cuda.synchronize()
    tol = 2.5 * TOL[dt] * ref.abs().max().item()     # P and O are both rounded to 16 bit; the keep factor is exact
    err = (ctx.cpu().double() - ref).abs().max().item()
    print(f"attention16_dropout dt={dt} {case}: max err {err:.3e} (bound {tol:.3e})")
    assert err <= tol, f"attention16_dropout dt={dt} {case}: max err {err:.3e} > {tol:.3e}"
    # the CLS-query form draws the masks of row q = 0
    ctx_cls = torch.empty(items, D, dtype=T16[dt], device="cuda")
    _lib.check(lib.iisan_attention16_dropout(dt, qkvd.data_ptr(), kbp, ctx_cls.data_ptr(), items, S, heads, p, seed, site, 1, _stream()),
               "attention16_dropout cls")
    torch.cuda.synchronize()
    err = (ctx_cls.cpu().double() - ref.view(items, S, D)[:, 0]).abs().max().item()
    assert err <= tol, f"attention16_dropout cls dt={dt} {case}: max err {err:.3e} > {tol:.3e}"
    # p = 0: the bits of the eval-mode kernel
    c0, c1 = torch.empty_like(ctx), torch.empty_like(ctx)
    _lib.check(lib.iisan_attention16_dropout(dt, qkvd.data_ptr(), kbp, c0.data_ptr(), items, S, heads, 0.0, seed, site, 0, _stream()),
               "attention16_dropout p=0")
    _lib.check(lib.iisan_attention16(dt, qkvd.data_ptr(), kbp, c1.data_ptr(), items, S, heads, _stream()), "attention16")
    torch.cuda.synchronize()
    assert torch.equal(c0.view(torch.int16), c1.view(torch.int16))


def test_attention16_dropout_refuses_bad_arguments(lib):
    q = torch.zeros(1, 2, 3, 4, 64, dtype=torch.float16, device="cuda")
    ctx = torch.zeros(4, 128, dtype=torch.float16, device="cuda")
    for p in (-0.1, 1.0):
        with pytest.raises(_lib.IisanHipError):
            _lib.check(lib.iisan_attention16_dropout(0, q.data_ptr(), None, ctx.data_ptr(), 1, 4, 2, p, 1, 0, 0, _stream()), "p range")
    with pytest.raises(_lib.IisanHipError):
        _lib.check(lib.iisan_attention16_dropout(0, q.data_ptr(), None, ctx.data_ptr(), 1, 225, 2, 0.1, 1, 0, 0, _stream()), "S > 224")


# ---- 6. taps against the restatement fed the same masks ----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _fixture():
    """(weights, text, dropped oracle taps): computed once on the CPU, shared, never modified."""
    cfg = gio.E2E_BERT
    bw = weights.make_bert_weights(cfg, seed=12)
    text = dropout_text(M, WORDS, cfg.vocab)
    masks = drop_masks(SEED, M, WORDS, cfg, P_DROP, P_DROP)
    with torch.no_grad():
        ref = torch.stack([h[:, 0] for h in bert_hidden_states_dropped(text, bw, cfg, masks)], 1)
    return bw, text, ref


@functools.lru_cache(maxsize=None)
def _packed(dt):
    return encoders.PackedBert(_fixture()[0], gio.E2E_BERT, "cuda", dt)


@pytest.mark.parametrize("full_blocks", [False, True])
@pytest.mark.parametrize("dt", [_lib.IISAN_F16, _lib.IISAN_BF16])
def test_dropped_taps_match_the_hf_pinned_restatement(lib, dt, full_blocks):
    bw, text, ref = _fixture()
    pk = _packed(dt)
    pk.full_blocks = full_blocks
    try:
        got = pk.forward_taps(text.cuda(), [0, 1, 2], dropout=(P_DROP, P_DROP, SEED)).cpu()
    finally:
        pk.full_blocks = False
    assert torch.isfinite(got).all()
    errs = [_rel(got[:, l], ref[:, l]) for l in range(3)]
    print(f"dropped taps dt={dt} full_blocks={full_blocks}: " + " / ".join(f"{e:.2e}" for e in errs))
    # tap 0 is fp32 gather + LayerNorm times an exact-or-zero factor; a mask at a wrong site or index costs ~3e-1
    assert errs[0] < 1e-5, errs
    for l in (1, 2):
        assert errs[l] < TAP_TOL[dt], (l, errs)


# ---- 7. bit-level properties ---------------------------------------------------------------------------------------------------------

def _raw(lib, pk, text_or_table, index, drop, chunk_items=0, taps_l=(0, 1, 2)):
    """`iisan_bert_forward_taps_dropout` called directly (drop: None = a NULL pointer, or a `_lib.BertDropout`)."""
    words = text_or_table.shape[1] // 2
    m = index.shape[0] if index is not None else text_or_table.shape[0]
    taps = torch.empty(m, len(taps_l), pk.cfg.hidden, device="cuda")
    tl = (C.c_int32 * len(taps_l))(*taps_l)
    ws = pk.ws.get(lib.iisan_bert_forward_taps_ws_bytes(C.byref(pk.struct), m, words, chunk_items), "cuda")
    _lib.check(lib.iisan_bert_forward_taps_dropout(C.byref(pk.struct), text_or_table.data_ptr(), text_or_table.shape[0] if index is not None else 0,
                                                   index.data_ptr() if index is not None else None, m, words, tl, len(taps_l), taps.data_ptr(),
                                                   chunk_items, C.byref(drop) if drop is not None else None, ws.data_ptr(), ws.numel(),
                                                   _stream()), "iisan_bert_forward_taps_dropout")
    return taps.cpu()


@pytest.mark.parametrize("dt", [_lib.IISAN_F16, _lib.IISAN_BF16])
def test_mask_convention_bit_level(lib, dt):
    bw, text, ref = _fixture()
    pk = _packed(dt)
    td = text.cuda()
    plain = pk.forward_taps(td, [0, 1, 2]).cpu()
    # NULL and p = 0 / 0 through the new entry: the eval-mode launches, the same bits
    assert torch.equal(_raw(lib, pk, td, None, None), plain)
    assert torch.equal(_raw(lib, pk, td, None, _lib.BertDropout(0.0, 0.0, SEED)), plain)
    assert torch.equal(pk.forward_taps(td, [0, 1, 2], dropout=(0.0, 0.0, 5)).cpu(), plain)
    # the same seed twice; another seed
    d = (P_DROP, P_DROP, SEED)
    a = pk.forward_taps(td, [0, 1, 2], dropout=d).cpu()
    assert torch.equal(pk.forward_taps(td, [0, 1, 2], dropout=d).cpu(), a)
    b = pk.forward_taps(td, [0, 1, 2], dropout=(P_DROP, P_DROP, SEED + 1)).cpu()
    for t in (a, b):
        # tap 0 scaled back: a tenth of it is zero, the rest is the eval-mode embedding row
        zeros = (t[:, 0] == 0)
        assert 0.05 < zeros.float().mean().item() < 0.15
        back = t[:, 0] * (1 - P_DROP)
        assert _rel(back[~zeros], plain[:, 0][~zeros]) < 1e-6
    assert not torch.equal(a[:, 0] == 0, b[:, 0] == 0)
    assert not torch.equal(a, plain)
    # only one of the two probabilities
    h_only = pk.forward_taps(td, [0, 1, 2], dropout=(P_DROP, 0.0, SEED)).cpu()
    a_only = pk.forward_taps(td, [0, 1, 2], dropout=(0.0, P_DROP, SEED)).cpu()
    assert torch.equal(h_only[:, 0], a[:, 0]) and not torch.equal(h_only[:, 1], a[:, 1])
    assert torch.equal(a_only[:, 0], plain[:, 0]) and not torch.equal(a_only[:, 1], plain[:, 1])
    # chunked = whole call: m is the slot's position in the whole call
    assert torch.equal(pk.forward_taps(td, [0, 1, 2], chunk_items=3, dropout=d).cpu(), a)
    # the indexed route (one index outside the table: a padding slot) = the direct route on the same contents
    table = text[[3, 1, 5, 2, 4, 6]].contiguous()            # rows of the table in another order than the slots
    index = torch.tensor([3, 1, 6, 0, 4, 2, 5])              # slot 2 names row 6: outside the 6-row table
    direct = torch.stack([table[i] if i < table.shape[0] else torch.zeros_like(table[0]) for i in index.tolist()])
    want = pk.forward_taps(direct.cuda(), [0, 1, 2], dropout=d).cpu()
    assert torch.equal(pk.forward_taps_indexed(table.cuda(), index.cuda(), [0, 1, 2], dropout=d).cpu(), want)
    assert torch.equal(pk.forward_taps_indexed(table.cuda(), index.cuda(), [0, 1, 2], chunk_items=2, dropout=d).cpu(), want)
    assert torch.equal(_raw(lib, pk, table.cuda(), index.cuda(), None), pk.forward_taps_indexed(table.cuda(), index.cuda(), [0, 1, 2]).cpu())
    # a probability outside [0, 1)
    with pytest.raises(_lib.IisanHipError):
        pk.forward_taps(td, [0, 1, 2], dropout=(1.0, 0.1, 1))
    with pytest.raises(_lib.IisanHipError):
        pk.forward_taps(td, [0, 1, 2], dropout=(0.1, -0.5, 1))


# ---- 8. pruned against full_blocks -----------------------------------------------------------------------------------------------------

def test_cls_only_last_block_draws_the_masks_of_row_zero(lib):
    bw, text, ref = _fixture()
    pk = _packed(_lib.IISAN_F16)
    d = (P_DROP, P_DROP, SEED)
    pk.full_blocks = True
    try:
        full = pk.forward_taps(text.cuda(), [0, 1, 2], dropout=d).cpu()
    finally:
        pk.full_blocks = False
    pruned = pk.forward_taps(text.cuda(), [0, 1, 2], dropout=d).cpu()
    assert torch.equal(pruned[:, :2], full[:, :2])
    print(f"pruned vs full_blocks, tap 2: {_rel(pruned[:, 2], full[:, 2]):.2e}")
    assert _rel(pruned[:, 2], full[:, 2]) < 5e-4, _rel(pruned[:, 2], full[:, 2])
    # a tapped prefix: block 1 is not run at all, block 0 is the CLS-only one
    pre = pk.forward_taps(text.cuda(), [0, 1], dropout=d).cpu()
    assert torch.equal(pre[:, 0], full[:, 0]) and _rel(pre[:, 1], full[:, 1]) < 5e-4


# ---- 8b. every train-mode instantiation against its eval twin ---------------------------------------------------------------------------

# make_drop (csrc/common.h) turns p = 1e-9 into thr24 = 0 and inv_keep = 1.0f: every keep factor is exactly 1 — yet the call is a
# train-mode one (p > 0), so the executor launches the train-mode kernel at every site
IDENTITY = (1e-9, 1e-9, SEED)


def _counted(fn):
    """(taps on the CPU, train-mode launches of the call)"""
    _lib.dev_set("count:bert_drop", 0)
    out = fn().cpu()
    return out, _lib.dev_get("count:bert_drop")


@pytest.mark.parametrize("dt", [_lib.IISAN_F16, _lib.IISAN_BF16])
def test_identity_mask_ties_every_train_mode_kernel_to_its_eval_twin(lib, dt):
    """The train-mode kernels of the three hidden sites are instantiations of the eval-mode row kernels (csrc/rowops.hip) and the
    attention one shares its block core with the eval-mode kernel (csrc/attn16_block.h): with the identity mask every tap is
    bit-equal to the eval-mode tap, direct and indexed, chunked and not, all-token and pruned.  The pruned last block included, though
    its train-mode attention is `attention16_drop_kernel<.., CLS>` where eval mode runs `attention_cls_kernel`, another kernel: on
    this fixture the two agree bit for bit, and did so at the commit before the row kernels were unified — which makes equality the
    contract there too (profiles/rowops_shared_body.md)."""
    bw, text, ref = _fixture()
    pk = _packed(dt)
    td = text.cuda()
    table, index = text[[3, 1, 5, 2, 4, 6]].contiguous().cuda(), torch.tensor([3, 1, 6, 0, 4, 2, 5]).cuda()     # slot 2: a padding slot
    taps_l, per_chunk = [0, 1, 2], 1 + 3 * pk.cfg.layers         # embeddings + (attention, two add + LayerNorm steps) per block
    routes = {"direct": (lambda d: pk.forward_taps(td, taps_l, dropout=d), 1),
              "direct, chunks of 3": (lambda d: pk.forward_taps(td, taps_l, chunk_items=3, dropout=d), 3),
              "indexed": (lambda d: pk.forward_taps_indexed(table, index, taps_l, dropout=d), 1),
              "indexed, chunks of 2": (lambda d: pk.forward_taps_indexed(table, index, taps_l, chunk_items=2, dropout=d), 4)}
    for full_blocks in (True, False):
        pk.full_blocks = full_blocks
        try:
            for name, (run, chunks) in routes.items():
                plain, n_eval = _counted(lambda: run(None))
                train, n_train = _counted(lambda: run(IDENTITY))
                assert n_eval == 0 and n_train == chunks * per_chunk, (name, n_eval, n_train)
                print(f"identity mask dt={dt} full_blocks={full_blocks} {name}: taps 0, 1 equal {torch.equal(train[:, :2], plain[:, :2])}, "
                      f"tap 2 equal {torch.equal(train[:, 2], plain[:, 2])} (rel {_rel(train[:, 2], plain[:, 2]):.2e})")
                assert torch.equal(train, plain), (full_blocks, name)
        finally:
            pk.full_blocks = False
    # negative control: a real mask at the hidden sites alone moves every tap
    plain = pk.forward_taps(td, taps_l).cpu()
    dropped = pk.forward_taps(td, taps_l, dropout=(P_DROP, 0.0, SEED)).cpu()
    for l in range(3):
        assert not torch.equal(dropped[:, l], plain[:, l]), l


# ---- 9. model level ------------------------------------------------------------------------------------------------------------------------

def _model():
    z, vw, bw, b, P = gio.e2e_small_inputs()
    args = helpers.make_args(side_adapter_vit_list="0,1", side_adapter_bert_list="0,1", num_words_title=8, drop_rate=0.0)
    model = helpers.build_model(args, 40, b.pop_prob, vw, gio.E2E_VIT, bw, gio.E2E_BERT, cached=False)
    helpers.load_trainables(model, P)
    return model, args, b


def test_model_switch(lib):
    model, args, b = _model()
    title = model.mm_encoder.bert_encoder.text_encoders["title"]
    ids, lm, img, txt = b.ids.cuda().view(-1), b.log_mask.cuda(), b.images.cuda(), b.text.cuda()
    assert title.train_dropout is False
    model.train()
    with torch.no_grad():
        off_train = model(ids, img, txt, lm, 0).item()
    off_train_grad = model(ids, img, txt, lm, 0).item()
    assert off_train_grad == off_train                    # SASRec dropout is 0 here: the switch off means a deterministic step
    cache_off = evaluate.build_tap_cache(model, img, txt, batch=7)
    table_off = evaluate.item_table(model, img, txt, batch=7)
    model.eval()
    off_eval = model(ids, img, txt, lm, 0).item()
    assert off_eval == off_train

    title.train_dropout = True
    model.eval()
    assert model(ids, img, txt, lm, 0).item() == off_eval                 # eval(): bit-equal to the model with the switch off
    model.train()
    l1, l2 = model(ids, img, txt, lm, 0).item(), model(ids, img, txt, lm, 0).item()
    assert l1 != l2 and l1 != off_eval and l2 != off_eval
    assert l1 == l1 and l2 == l2 and abs(l1) != float("inf") and abs(l2) != float("inf")      # finite
    # the seed comes from the torch CPU generator: reproducible
    torch.manual_seed(77)
    r1 = model(ids, img, txt, lm, 0).item()
    torch.manual_seed(77)
    assert model(ids, img, txt, lm, 0).item() == r1
    # the eval hooks do not call model.eval(): still deterministic, still the eval-mode tower
    cache_on = evaluate.build_tap_cache(model, img, txt, batch=7)
    assert torch.equal(cache_on[0], cache_off[0]) and torch.equal(cache_on[1], cache_off[1])
    assert torch.equal(evaluate.item_table(model, img, txt, batch=7), table_off)
    # one encoding per distinct id cannot draw independent masks for two slots of one item
    model.dedup_items = True
    with pytest.raises(ValueError, match="train_dropout"):
        model(ids, img, txt, lm, 0)
    with pytest.raises(ValueError, match="train_dropout"):
        model.mm_encoder.forward_item3_indexed(torch.zeros(1, 3, 32, 32, dtype=torch.uint8, device="cuda"), txt[:1].contiguous(),
                                               torch.zeros(4, dtype=torch.int64, device="cuda"), dedup=True)
    model.dedup_items = False
    # the fp32 residual stream of the dev switch has no dropout variants: refused by name, never eval mode silently
    try:
        _lib.dev_set("resid32", 1)
        with pytest.raises(_lib.IisanHipError, match="resid32"):
            model(ids, img, txt, lm, 0)
    finally:
        _lib.dev_set("resid32", 0)


def test_a_training_step_with_the_switch_on(lib):
    model, args, b = _model()
    model.mm_encoder.bert_encoder.text_encoders["title"].train_dropout = True
    model.train()
    tr = trainer.FlatTrainer(model, args)
    before = tr.flat.clone()
    loss = tr.step(b.ids.cuda().view(-1), b.images.cuda(), b.text.cuda(), b.log_mask.cuda())
    torch.cuda.synchronize()
    assert torch.isfinite(loss).item()
    assert torch.isfinite(tr.flat).all() and not torch.equal(tr.flat, before)
