"""Helpers shared by the parity tests: load the golden fixtures and rebuild the exact seeded inputs they were
generated from (`tests/golden/make_golden.py`), checking the stored input checksums so generator drift is loud."""
from __future__ import annotations

import hashlib
import os

import numpy as np
import torch

from iisan_amd import synth, weights

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GRAD_STRIDE = 97
GRAD_FULL_MAX = 5000


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def load(name: str):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


def sample_like_golden(t: torch.Tensor) -> np.ndarray:
    g = t.detach().cpu().reshape(-1)
    return (g if g.numel() <= GRAD_FULL_MAX else g[::GRAD_STRIDE]).numpy()


def sample_like_hparams(t: torch.Tensor) -> np.ndarray:
    """`hparam_sample` of tests/golden/make_golden.py (sidenet_hparams.npz)."""
    g = t.detach().cpu().reshape(-1)
    return (g if g.numel() <= 256 else g[::37] if g.numel() <= 5000 else g[::389]).numpy()


def encoders_full_inputs():
    z = load("encoders_full.npz")
    vw = weights.make_vit_weights(weights.VIT_BASE, seed=int(z["vit_seed"]))
    bw = weights.make_bert_weights(weights.BERT_BASE, seed=int(z["bert_seed"]))
    assert sha(vw["L11.fc2_w"]) == str(z["w_sha"][0]) and sha(bw["word_emb"]) == str(z["w_sha"][1]), \
        "seeded weight generator drifted from the golden fixture"
    b = synth.scientific_batch(bs=1, seed=int(z["batch_seed"]), seq_len=3, lengths=[3])
    assert sha(b.images) == str(z["images_sha"]), "seeded image generator drifted from the golden fixture"
    assert np.array_equal(b.text.numpy(), z["text"])
    return z, vw, bw, b


def sidenet_full_inputs(variant: str = "default"):
    z = load("sidenet_full.npz")
    b = synth.scientific_batch(bs=3, seed=77, lengths=[4, 11, 7], dup_items=True, res=16, item_num=50)
    assert np.array_equal(b.ids.numpy(), z["ids"]) and np.array_equal(b.pop_prob.numpy(), z["pop"])
    taps_cv = synth.cached_taps(b.ids, 12, 768, seed=5)
    taps_tx = synth.cached_taps(b.ids, 12, 768, seed=6)
    assert sha(taps_cv) == str(z["taps_sha"][0]) and sha(taps_tx) == str(z["taps_sha"][1])
    P = weights.make_trainable_params(seed=99, cached=True, n_side=6 if variant == "rmfirst" else 7)
    kw = dict(default={}, gelu=dict(activation="GELU"), rmfirst=dict(remove_first=True))[variant]
    return z, b, taps_cv, taps_tx, P, kw


ALL_LAYERS = ",".join(str(i) for i in range(12))
HPARAM_ITEMS = 100
HPARAM_VARIANTS = {
    # name: (launcher arguments off their defaults, sequence lengths incl. the target) - as in tests/golden/make_golden.py
    "down32": (dict(cv_adapter_down_size=32, bert_adapter_down_size=32), [4, 11, 7]),
    "down128_gelu": (dict(cv_adapter_down_size=128, bert_adapter_down_size=128, adapter_activation="GELU"), [4, 11, 7]),
    "s20_l3_h4": (dict(max_seq_len=20, transformer_block=3, num_attention_heads=4), [21, 3, 12, 16, 17]),
    "s32_l1_h1": (dict(max_seq_len=32, transformer_block=1, num_attention_heads=1), [33, 2, 17]),
    "s5_h1": (dict(max_seq_len=5, num_attention_heads=1), [6, 2, 4]),
    "layers12": (dict(side_adapter_vit_list=ALL_LAYERS, side_adapter_bert_list=ALL_LAYERS), [4, 11, 7]),
    "one_layer_rmfirst": (dict(side_adapter_vit_list="11", side_adapter_bert_list="11", remove_first="TRUE"), [4, 11, 7]),
}


def sidenet_hparams_inputs(variant: str):
    """Batch, taps, seeded parameters (shapes from the product's module tree) and the oracle's keyword arguments of one
    `sidenet_hparams.npz` variant."""
    import helpers
    z = load("sidenet_hparams.npz")
    kw, lengths = HPARAM_VARIANTS[variant]
    args = helpers.make_args(**kw)
    pre = variant + "/"
    b = synth.scientific_batch(bs=len(lengths), seed=79, seq_len=args.max_seq_len, lengths=lengths, dup_items=True, res=2, words=2,
                               item_num=HPARAM_ITEMS)
    assert np.array_equal(b.ids.numpy(), z[pre + "ids"]) and np.array_equal(b.pop_prob.numpy(), z[pre + "pop"])
    assert np.array_equal(b.log_mask.numpy(), z[pre + "log_mask"])
    taps_cv = synth.cached_taps(b.ids, 12, 768, seed=25)
    taps_tx = synth.cached_taps(b.ids, 12, 768, seed=26)
    assert sha(taps_cv) == str(z[pre + "taps_sha"][0]) and sha(taps_tx) == str(z[pre + "taps_sha"][1])
    model = helpers.build_model(args, HPARAM_ITEMS, b.pop_prob, cached=True, device="cpu")
    shapes = {n: tuple(p.shape) for n, p in model.named_parameters() if p.requires_grad}
    assert hashlib.sha256("\n".join(sorted(shapes)).encode()).hexdigest()[:16] == str(z[pre + "names_sha"]), \
        "the module tree differs from the reference's"
    P = weights.fill_params_seeded(shapes, seed=557)
    rm = args.remove_first == "TRUE"
    okw = dict(heads=args.num_attention_heads, n_layers=args.transformer_block, activation=args.adapter_activation, remove_first=rm,
               cv_head="mm_encoder.cv_pre_fc.", text_head="mm_encoder.bert_pre_fc.")
    layers = [int(i) + 1 for i in args.side_adapter_vit_list.split(",")]
    return z, b, taps_cv, taps_tx, P, (layers if rm else [0] + layers), okw


def hparams_grads(z, variant: str, names):
    """{name: (sampled gradient, [norm, sum])} of one `sidenet_hparams.npz` variant (stored back to back in sorted-name order)."""
    pre = variant + "/"
    names = sorted(names)
    g, end, gn = z[pre + "g"], z[pre + "g_end"], z[pre + "gn"]
    assert len(names) == len(end) == len(gn)
    return {n: (g[(end[i - 1] if i else 0):end[i]], gn[i]) for i, n in enumerate(names)}


E2E_VIT = weights.VitConfig(hidden=768, layers=2, heads=12, mlp=512, image=32, patch=16)
E2E_BERT = weights.BertConfig(hidden=768, layers=2, heads=12, mlp=512, vocab=512, max_pos=64)


E2E_BS8_LENGTHS = (3, 11, 6, 4, 9, 5, 7, 11)


def e2e_small_inputs(name="e2e_small", lengths=(3, 11, 6), modality="intra_inter"):
    z = load(name + ".npz")
    vw, bw = weights.make_vit_weights(E2E_VIT, seed=11), weights.make_bert_weights(E2E_BERT, seed=12)
    b = synth.scientific_batch(bs=len(lengths), seed=31, lengths=list(lengths), dup_items=True, res=32, words=8, vocab=512,
                               item_num=40)
    assert sha(b.images) == str(z["images_sha"]) and np.array_equal(b.text.numpy(), z["text"])
    assert np.array_equal(b.ids.numpy(), z["ids"])
    P = weights.make_trainable_params(seed=101, n_side=3, modality=modality)
    return z, vw, bw, b, P


def eval_inputs():
    z = load("eval.npz")
    lens = z["seq_len"]
    flat = z["seq_flat"]
    seqs, o = [], 0
    for l in lens:
        seqs.append([int(x) for x in flat[o:o + int(l)]])
        o += int(l)
    P = weights.make_trainable_params(seed=99, cached=True)
    tables = [torch.from_numpy(z[k]) for k in ("table_cv", "table_text", "table_mm")]
    return z, seqs, tables, P


VERSA_VARIANTS = {
    "text_wide_long": (256, 512, 6, 10, "0,2,4", "1,3,5,7,8", {}),
    "image_wide_long": (512, 256, 7, 5, "0,1,2,3,5", "1,3", dict(adapter_activation="GELU")),
    "equal_rmfirst": (256, 256, 5, 5, "0,2,3", "1,2,3", dict(remove_first="TRUE")),
}


def versa_inputs(variant: str, device="cpu"):
    """Batch, taps, product model (wired like Code_Cached_Asym/run.py:185-190) and seeded parameters of one Versa fixture."""
    import helpers
    z = load("versa.npz")
    Di, Dt, Lc, Lt, vlist, blist, extra = VERSA_VARIANTS[variant]
    b = synth.scientific_batch(bs=3, seed=78, lengths=[5, 11, 3], dup_items=True, res=16, item_num=50)
    assert np.array_equal(b.ids.numpy(), z["ids"])
    taps_cv = synth.cached_taps(b.ids, Lc - 1, Di, seed=15)
    taps_tx = synth.cached_taps(b.ids, Lt - 1, Dt, seed=16)
    assert sha(taps_cv) == str(z[variant + "/taps_sha"][0]) and sha(taps_tx) == str(z[variant + "/taps_sha"][1])
    args = helpers.make_args(text_embedding_dim=Dt, image_embedding_dim=Di, side_adapter_vit_list=vlist,
                             side_adapter_bert_list=blist, image_layers=Lc - 1, text_layers=Lt - 1, **extra)
    model = helpers.build_model(args, 50, b.pop_prob, cached="versa", device=device)
    shapes = {n: tuple(p.shape) for n, p in model.named_parameters() if p.requires_grad}
    assert sorted(shapes) == [str(x) for x in z[variant + "/names"]], "Versa module tree differs from the reference's"
    P = weights.fill_params_seeded(shapes, seed=555)
    return z, b, taps_cv, taps_tx, args, model, P
