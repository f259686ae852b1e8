"""Versa plumbing on taps built by the ViT-H/14 executor: `evaluate.build_tap_cache` over a 1280-wide ViT (16 heads of 80, 14-pixel
patches) and a 768-wide BERT -> `TapStore`s -> `VersaIISANAdaptedMModel` (image_embedding_dim 1280, text_embedding_dim 768) + `ModelMM`,
one forward / backward against the CPU oracle fed the SAME HIP-built taps, at the bounds of tests/test_gpu_wide_versa.py.  This checks the
hand-over, not the tower a second time (tests/test_gpu_vit_huge_tower.py)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import golden_io as gio  # noqa: E402,F401
import helpers  # noqa: E402
from iisan_amd import evaluate, synth, tapstore, weights  # noqa: E402
from oracle import iisan_oracle as O  # noqa: E402

N_ITEMS, WORDS = 40, 8          # catalogue rows (row 0 = the padding item), words per title
VIT = weights.VitConfig(hidden=1280, layers=4, heads=16, mlp=512, image=56, patch=14)
BERT = weights.BertConfig(hidden=768, layers=4, heads=12, mlp=512, vocab=512, max_pos=64)


def _close(a, b, rtol, atol, what):       # tests/test_gpu_trainable.py
    a = torch.as_tensor(a, dtype=torch.float64).cpu()
    b = torch.as_tensor(b, dtype=torch.float64).cpu()
    err = (a - b).abs().max().item()
    ref = b.abs().max().item()
    assert err <= atol + rtol * ref, f"{what}: max|err| {err:.3e} vs scale {ref:.3e}"


def test_versa_trains_on_a_tap_cache_built_by_the_vit_huge_executor():
    item_ids = np.arange(N_ITEMS)
    images = synth.make_images(item_ids, 56, seed=5)                                     # zeros on row 0
    g = torch.Generator().manual_seed(6)
    text = torch.zeros(N_ITEMS, 2 * WORDS, dtype=torch.int64)                             # W ids, then the W-wide attention mask
    for m in range(1, N_ITEMS):
        n = int(torch.randint(3, WORDS + 1, (1,), generator=g))
        text[m, :n] = torch.randint(1, BERT.vocab, (n,), generator=g)
        text[m, WORDS:WORDS + n] = 1
    assert images[0].abs().max() == 0 and text[0].abs().max() == 0
    pop = synth.make_pop_prob(N_ITEMS - 1)
    # the tap builder: an Uncached model owns the two frozen towers (its 768-wide side network is not used here)
    args_u = helpers.make_args(side_adapter_vit_list="0,1", side_adapter_bert_list="0,1", num_words_title=WORDS)
    vw, bw = weights.make_vit_weights(VIT, seed=61), weights.make_bert_weights(BERT, seed=62)
    builder = helpers.build_model(args_u, N_ITEMS - 1, pop, vw, VIT, bw, BERT, cached=False, device="cuda")
    taps_cv, taps_tx = evaluate.build_tap_cache(builder, images.cuda(), text.cuda(), batch=16)
    assert taps_cv.shape == (N_ITEMS, 5, 1280) and taps_tx.shape == (N_ITEMS, 5, 768)
    assert taps_cv.dtype == torch.float32 and torch.isfinite(taps_cv).all() and torch.isfinite(taps_tx).all()
    enc = builder.mm_encoder
    assert torch.equal(taps_cv, enc.cv_encoder.packed("cuda").forward_taps(images.cuda(), list(range(5))))
    assert torch.equal(taps_tx, enc.bert_encoder.text_encoders["title"].packed("cuda").forward_taps(text.cuda(), list(range(5))))
    assert taps_cv[1:].abs().max() > 0 and not torch.equal(taps_cv[1], taps_cv[2])

    # the Versa model on stores of those taps: two SANBs per tower (layer 0 + one listed layer each)
    vlist, blist = "1", "3"
    args = helpers.make_args(image_embedding_dim=1280, text_embedding_dim=768, side_adapter_vit_list=vlist, side_adapter_bert_list=blist,
                             image_layers=4, text_layers=4, drop_rate=0.0, adapter_dropout_rate=0.0)
    model = helpers.build_model(args, N_ITEMS - 1, pop, cached="versa", device="cuda")
    shapes = {n: tuple(p.shape) for n, p in model.named_parameters() if p.requires_grad}
    P = weights.fill_params_seeded(shapes, seed=555)
    helpers.load_trainables(model, P)
    model.train()
    lay_cv, lay_tx = model.mm_encoder.packed_layers()
    assert lay_cv == [0, 2] and lay_tx == [0, 4]
    model.tap_stores = (tapstore.TapStore(taps_cv, lay_cv, "cuda", "fp32"), tapstore.TapStore(taps_tx, lay_tx, "cuda", "fp32"))
    assert model.tap_stores[0].dim == 1280 and model.tap_stores[1].dim == 768
    ids_np, lm_np = synth.make_ids(3, 10, N_ITEMS - 1, np.random.RandomState(78), lengths=[5, 11, 3])
    ids, log_mask = torch.from_numpy(ids_np), torch.from_numpy(lm_np)
    bs, S = log_mask.shape
    loss = model(ids.view(-1).cuda(), None, None, log_mask.cuda(), 0)
    loss.backward()

    # the oracle on the same taps, as the stores hand them over: row 0 (the padding item) all zeros
    flat = ids.view(-1)
    real = (flat != 0).view(-1, 1, 1).float()
    oc, ot = taps_cv.cpu()[flat] * real, taps_tx.cpu()[flat] * real
    Po = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    lc, lt = O.side_layer_list(vlist, False), O.side_layer_list(blist, False)
    cv, tx, mm = O.versa_side_network(oc, ot, Po, lc, lt)
    score = torch.nn.functional.linear(torch.cat([cv, tx, mm], 1), Po["com_dense.weight"], Po["com_dense.bias"])
    prec = O.sasrec(score.view(bs, S + 1, 64)[:, :-1], log_mask, Po, 2, 2).reshape(-1, 64)
    ref = O.inbatch_ce(ids, score, prec, log_mask, pop)
    ref.backward()
    print(f"loss {loss.item():.7f} oracle {ref.item():.7f} rel {abs(loss.item() - ref.item()) / abs(ref.item()):.2e}")
    _close(loss, ref.detach(), 3e-5, 0, "loss")
    n_grads = 0
    for n, p in model.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and Po[n].grad is not None, n
            err = (p.grad.cpu() - Po[n].grad).abs().max().item() / (Po[n].grad.abs().max().item() + 1e-30)
            print(f"grad {n}: {err:.2e}")
            _close(p.grad, Po[n].grad, 6e-4, 3e-7, f"grad {n}")
            n_grads += 1
    assert n_grads > 20
