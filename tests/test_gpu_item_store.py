"""GPU checks of the device item store / host feed of the Uncached path (`iisan_amd/itemstore.py`, the two
`*_indexed` encoder entries).  The reference of every test is the EXISTING entry point fed with the materialised equivalent —
`normalise(catalogue[index])` in fp32 with zeros on padding slots, `table[index]` with zero rows on padding slots — and the
comparison is `torch.equal`: the patch matrices / embedding rows are the same bits and the rest of the executor is unchanged."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import golden_io as gio  # noqa: E402
import helpers  # noqa: E402
from iisan_amd import _lib, encoders, evaluate, itemstore, synth, weights  # noqa: E402

INDEX = [4, 4, -1, 0, 8, 1, -1, 4, 7, 2, 8]        # repeats, pads, row 0 as a real row, the last row; M = 11
TAPS = [0, 1, 2]
WORDS = 8


def _normalise(u8):
    return (u8.float().div(255) - 0.5) / 0.5          # torchvision ToTensor + Normalize(.5, .5), dataset.py:46-50


def _materialise_images(cat_u8, index):
    """fp32 [M,C,R,R]: normalise(catalogue[index]), the all-zero normalised image where index is outside the catalogue."""
    idx = torch.as_tensor(index)
    pad = (idx < 0) | (idx >= cat_u8.shape[0])
    img = _normalise(cat_u8[idx.masked_fill(pad, 0)])
    img[pad] = 0
    return img


def _materialise_text(table, index):
    idx = torch.as_tensor(index)
    pad = (idx < 0) | (idx >= table.shape[0])
    txt = table[idx.masked_fill(pad, 0)].clone()
    txt[pad] = 0
    return txt


@functools.lru_cache(maxsize=None)
def _catalogue(rows=9, res=32, seed=3):
    """(uint8 [rows,3,res,res], int64 [rows, 2*WORDS]) — EVERY row real content, row 0 included (the kernels must not treat it
    specially; only the stores map item id 0 to a padding index)."""
    g = torch.Generator().manual_seed(seed)
    cat = torch.randint(0, 256, (rows, 3, res, res), generator=g, dtype=torch.uint8)
    table = torch.from_numpy(synth.make_text(np.arange(1, rows + 1), WORDS, gio.E2E_BERT.vocab, np.random.RandomState(seed)))
    return cat, table


@functools.lru_cache(maxsize=None)
def _towers(dt):
    """Packed tiny towers + the reference taps of INDEX through the existing entries, computed once per operand type."""
    vit = encoders.PackedVit(weights.make_vit_weights(gio.E2E_VIT, seed=11), gio.E2E_VIT, "cuda", dt)
    bert = encoders.PackedBert(weights.make_bert_weights(gio.E2E_BERT, seed=12), gio.E2E_BERT, "cuda", dt)
    cat, table = _catalogue()
    ref_c = vit.forward_taps(_materialise_images(cat, INDEX).cuda(), TAPS).cpu()
    ref_t = bert.forward_taps(_materialise_text(table, INDEX).cuda(), TAPS).cpu()
    return vit, bert, ref_c, ref_t


@pytest.mark.parametrize("chunk", [0, 4])             # 4: three chunks, the last ragged — the index offset of the chunk loop
@pytest.mark.parametrize("dt", [_lib.IISAN_F16, _lib.IISAN_BF16])
def test_vit_indexed_equals_the_materialised_batch(dt, chunk):
    vit, _, ref_c, _ = _towers(dt)
    cat, _ = _catalogue()
    got = vit.forward_taps_indexed(cat.cuda(), torch.tensor(INDEX).cuda(), TAPS, chunk_items=chunk).cpu()
    assert torch.equal(got, ref_c)
    assert not torch.equal(got[0], got[2])            # a real slot and a pad slot are different items (the check is not vacuous)


@pytest.mark.parametrize("chunk", [0, 4])
@pytest.mark.parametrize("dt", [_lib.IISAN_F16, _lib.IISAN_BF16])
def test_bert_indexed_equals_the_materialised_batch(dt, chunk):
    _, bert, _, ref_t = _towers(dt)
    _, table = _catalogue()
    got = bert.forward_taps_indexed(table.cuda(), torch.tensor(INDEX).cuda(), TAPS, chunk_items=chunk).cpu()
    assert torch.equal(got, ref_t)
    # a pad slot equals an all-zero row through the existing entry
    zero = bert.forward_taps(torch.zeros(1, 2 * WORDS, dtype=torch.int64).cuda(), TAPS).cpu()
    assert torch.equal(got[2], zero[0]) and torch.equal(got[6], zero[0])


@pytest.mark.parametrize("pad_value", [9, 2 ** 40])     # `rows` itself and far outside the catalogue
def test_any_index_outside_the_catalogue_is_a_padding_slot(pad_value):
    vit, bert, ref_c, ref_t = _towers(_lib.IISAN_F16)
    cat, table = _catalogue()
    index = torch.tensor([pad_value if i == -1 else i for i in INDEX]).cuda()
    assert torch.equal(vit.forward_taps_indexed(cat.cuda(), index, TAPS, chunk_items=4).cpu(), ref_c)
    assert torch.equal(bert.forward_taps_indexed(table.cuda(), index, TAPS, chunk_items=4).cpu(), ref_t)


def test_production_geometry_addressing():
    """ViT-B geometry (224 / 16): 150,528-byte catalogue rows and a 14 x 14 patch grid.  `tap_layers = [0]` with the default dead-work
    policy runs no transformer block; the CLS row of hidden state 0 is `cls + pos[0]`, independent of the pixels, so the same call
    with taps [0, 1] (one block, CLS query only) is what makes the check depend on which bytes the patch kernel read."""
    cfg = weights.VIT_BASE
    vit = encoders.PackedVit(weights.make_vit_weights(cfg, seed=5), cfg, "cuda")
    g = torch.Generator().manual_seed(9)
    cat = torch.randint(0, 256, (3, 3, 224, 224), generator=g, dtype=torch.uint8)
    index = [2, -1, 0, 2, 1]
    mat = _materialise_images(cat, index).cuda()
    for taps in ([0], [0, 1]):
        got = vit.forward_taps_indexed(cat.cuda(), torch.tensor(index).cuda(), taps).cpu()
        assert torch.equal(got, vit.forward_taps(mat, taps).cpu()), taps
    assert not torch.equal(got[2, 1], got[4, 1]) and not torch.equal(got[1, 1], got[4, 1])


# ---- model level ---------------------------------------------------------------------------------------------------------------
ITEM_NUM = 14


@functools.lru_cache(maxsize=None)
def _item_catalogue():
    """14 items + the padding row 0.  Row 0 holds junk on purpose: no path may read it (id 0 -> index -1 -> zero content)."""
    cat, _ = _catalogue(rows=ITEM_NUM + 1, seed=21)
    table = torch.from_numpy(synth.make_text(np.arange(ITEM_NUM + 1), WORDS, gio.E2E_BERT.vocab, np.random.RandomState(0)))
    table[0] = table[3]
    return cat, table


def _batch(lengths, seed, ids=None):
    """(ids [bs, 11] int64, log_mask, materialised images fp32, materialised text) for the item catalogue, on the device."""
    if ids is None:
        ids, _ = synth.make_ids(len(lengths), 10, ITEM_NUM, np.random.RandomState(seed), lengths)
    ids = torch.as_tensor(ids)
    cat, table = _item_catalogue()
    index = torch.where(ids.view(-1) == 0, -1, ids.view(-1))
    lm = (ids[:, :-1] != 0).float()
    return ids.cuda(), lm.cuda(), _materialise_images(cat, index).cuda(), _materialise_text(table, index).cuda()


def _model(**kw):
    vw, bw = weights.make_vit_weights(gio.E2E_VIT, seed=11), weights.make_bert_weights(gio.E2E_BERT, seed=12)
    args = helpers.make_args(side_adapter_vit_list="0,1", side_adapter_bert_list="0,1", num_words_title=WORDS, drop_rate=0.0, **kw)
    m = helpers.build_model(args, ITEM_NUM, synth.make_pop_prob(ITEM_NUM), vw, gio.E2E_VIT, bw, gio.E2E_BERT, cached=False)
    helpers.load_trainables(m, weights.make_trainable_params(seed=101, n_side=3))
    return m


def _loss_and_grads(m, ids, images, text, lm):
    m.zero_grad()
    loss = m(ids.view(-1), images, text, lm, None)
    loss.backward()
    return loss.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("dedup", [False, True])
def test_model_on_the_resident_store_equals_the_materialised_path(dedup):
    ids, lm, images, text = _batch([3, 11, 6, 4, 11, 2], seed=77)
    flat = ids.view(-1)
    assert flat.unique().numel() < (flat != 0).sum().item()           # repeats among the real items, plus padding
    m = _model()
    m.dedup_items = dedup
    m.train()
    l0, g0 = _loss_and_grads(m, ids, images, text, lm)
    cat, table = _item_catalogue()
    store = itemstore.ItemStore(cat.numpy(), table, "cuda", chunk_bytes=4 * cat[0].numel())     # 4 rows per chunk: 4 uploads, ragged
    assert store.nbytes() == cat.numel() + table.numel() * 8
    assert torch.equal(store.images.cpu(), cat) and torch.equal(store.text.cpu(), table)
    m.item_stores = store
    l1, g1 = _loss_and_grads(m, ids, None, None, lm)
    assert torch.equal(l0, l1)
    assert g0.keys() == g1.keys() and len(g0) > 50
    for k in g0:       # the backward kernels reduce with atomics: equal up to summation order (the bound of the dedup test)
        assert torch.allclose(g0[k], g1[k], rtol=1e-4, atol=1e-7), (k, (g0[k] - g1[k]).abs().max().item())


def test_a_wider_content_table_is_narrowed_to_the_title_once():
    ids, lm, images, text = _batch([3, 11, 6], seed=5)
    m = _model(num_words_abstract=4, news_attributes=["title", "abstract"])
    cat, table = _item_catalogue()
    wide = torch.cat([table, torch.full((ITEM_NUM + 1, 8), 7, dtype=torch.int64)], 1)
    with torch.no_grad():
        ref = m(ids.view(-1), images, torch.cat([text, torch.full((text.shape[0], 8), 7, dtype=torch.int64, device="cuda")], 1), lm, None)
        m.item_stores = store = itemstore.ItemStore(cat, wide)
        got = m(ids.view(-1), None, None, lm, None)
        held = store.text
        assert held.shape == (ITEM_NUM + 1, 2 * WORDS) and held.is_contiguous()
        again = m(ids.view(-1), None, None, lm, None)
    assert store.text is held
    assert torch.equal(ref, got) and torch.equal(ref, again)


def test_feed_one_step_ahead_equals_the_materialised_path():
    cap = 12
    full = np.zeros((3, 11), dtype=np.int64)          # exactly `cap` distinct real items
    perm = np.random.RandomState(4).permutation(np.arange(1, ITEM_NUM + 1))[:cap]
    full[0, -5:], full[1, -4:], full[2, -3:] = perm[:5], perm[5:9], perm[9:]
    batches = [_batch([3, 6, 2], seed=1), _batch([4, 4, 4], seed=2), _batch(None, 0, ids=full), _batch([2, 7, 3], seed=3),
               _batch([5, 2, 4], seed=4)]
    assert len(np.unique(full)) - 1 == cap
    m = _model()
    m.eval()
    with torch.no_grad():
        ref = [m(ids.view(-1), img, txt, lm, None).clone() for ids, lm, img, txt in batches]
        cat, table = _item_catalogue()
        feed = itemstore.ItemFeed(cat.numpy(), table.numpy(), "cuda", slots=2, capacity=cap)
        m.item_stores = feed
        feed.submit(batches[0][0].cpu())
        got = []
        for i, (ids, lm, _, _) in enumerate(batches):
            if i + 1 < len(batches):
                feed.submit(batches[i + 1][0].cpu())   # one step ahead of its use; from batch 2 on it reuses a slot
            got.append(m(ids.view(-1), None, None, lm, None).clone())
        with pytest.raises(RuntimeError):
            feed.lookup(batches[0][0])                 # nothing submitted
    for i, (r, g) in enumerate(zip(ref, got)):
        assert torch.equal(r, g), (i, r.item(), g.item())
    assert len({r.item() for r in ref}) == len(ref)    # five different batches
    over = full.copy()
    over[0, 0] = [i for i in range(1, ITEM_NUM + 1) if i not in perm][0]
    with pytest.raises(ValueError):
        feed.submit(over)                              # capacity + 1 distinct items


def test_eval_hooks_over_a_store_equal_the_materialised_catalogue():
    m = _model()
    m.eval()
    cat, table = _item_catalogue()
    every = [-1] + list(range(1, ITEM_NUM + 1))          # row 0 = the padding item, then items 1..14
    images, text = _materialise_images(cat, every).cuda(), _materialise_text(table, every).cuda()
    store = itemstore.ItemStore(cat, table)
    ref = evaluate.item_table(m, images, text, batch=4)
    assert torch.equal(evaluate.item_table_from_store(m, store, batch=4), ref)
    feed = itemstore.ItemFeed(cat, table, capacity=4)
    assert torch.equal(evaluate.item_table_from_store(m, feed, batch=4), ref)
    rc, rt = evaluate.build_tap_cache(m, images, text, batch=7)
    gc, gt = evaluate.build_tap_cache_from_store(m, store, batch=7)
    assert torch.equal(gc, rc) and torch.equal(gt, rt)


def test_bad_arguments_are_reported_not_executed(lib):
    """`rows = 0`, a null index, a non-uint8 catalogue: IISAN_EBADSHAPE (-1) with a message, nothing launched (the taps buffer keeps
    its sentinel)."""
    vit, bert, _, _ = _towers(_lib.IISAN_F16)
    cat, table = _catalogue()
    cat, table, index = cat.cuda(), table.cuda(), torch.tensor(INDEX).cuda()
    M = index.numel()
    taps = torch.full((M, 1, 768), 123.0, device="cuda")
    tl = (C.c_int32 * 1)(0)
    s = torch.cuda.current_stream().cuda_stream

    def vit_call(cat_ptr, rows, idx_ptr):
        n = lib.iisan_vit_forward_taps_ws_bytes(C.byref(vit.struct), M, 0)
        ws = torch.empty(n, dtype=torch.uint8, device="cuda")
        return lib.iisan_vit_forward_taps_u8_indexed(C.byref(vit.struct), cat_ptr, rows, idx_ptr, M, tl, 1, taps.data_ptr(), 0,
                                                     ws.data_ptr(), n, s)

    def bert_call(tab_ptr, rows, idx_ptr):
        n = lib.iisan_bert_forward_taps_ws_bytes(C.byref(bert.struct), M, WORDS, 0)
        ws = torch.empty(n, dtype=torch.uint8, device="cuda")
        return lib.iisan_bert_forward_taps_indexed(C.byref(bert.struct), tab_ptr, rows, idx_ptr, M, WORDS, tl, 1, taps.data_ptr(), 0,
                                                   ws.data_ptr(), n, s)

    for call, ptr in ((vit_call, cat.data_ptr()), (bert_call, table.data_ptr())):
        for args in ((ptr, 0, index.data_ptr()), (ptr, 9, None), (None, 9, index.data_ptr())):
            assert call(*args) == -1, args                       # IISAN_EBADSHAPE
            assert lib.iisan_last_error().decode().strip()
    torch.cuda.synchronize()
    assert bool((taps == 123.0).all())
    with pytest.raises(AssertionError):
        vit.forward_taps_indexed(cat.float(), index, [0])        # not a uint8 catalogue
    with pytest.raises(AssertionError):
        vit.forward_taps_indexed(cat, index.int(), [0])          # not an int64 index
    with pytest.raises(AssertionError):
        bert.forward_taps_indexed(table, index.cpu(), [0])       # no CPU path
    with pytest.raises(_lib.IisanHipError):
        vit.forward_taps_indexed(cat, index, [0, 99])            # tap layer outside the tower, reported through the same checks
