"""CPU side of the opt-in train-mode dropout of the frozen BERT tower (`iisan_bert_forward_taps_dropout`: the attention kernel of
csrc/bert_drop.hip, the keep-functor instantiations of the row kernels of csrc/rowops.hip): where HF's `BertModel` applies dropout
under `train()` and with which masks — pinned against HF itself —, the struct layout of the ABI argument, the Python switch, and the
code-object metadata of the train-mode kernels.

`bert_hidden_states_dropped` is `oracle.bert_hidden_states` with the four keep-factor multiplications inserted; the GPU tests
(tests/test_gpu_bert_dropout.py) feed it the masks the kernels draw."""
import ctypes as C
import os
import subprocess
import types

import pytest
import torch
import torch.nn.functional as F

import golden_io as gio
import helpers
from iisan_amd import _lib, weights
from oracle import iisan_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def drop_masks(seed, M, T, cfg, hidden_p, attn_p):
    """Keep factors of one forward call, in HF's call order: site 0 [M,T,D] (embeddings), then per block l site 1 + 3l [M,H,T,T]
    (attention probabilities), 2 + 3l and 3 + 3l [M,T,D] (the two dense outputs).  Element index = the row-major position in that
    shape: (m T + t) D + c and ((m H + h) T + q) T + k with m the slot's position in the whole call (include/iisan_hip.h)."""
    D, H = cfg.hidden, cfg.heads
    masks = [helpers.drop_factors(seed, 0, M * T * D, hidden_p).view(M, T, D)]
    for l in range(cfg.layers):
        masks.append(helpers.drop_factors(seed, 1 + 3 * l, M * H * T * T, attn_p).view(M, H, T, T))
        masks.append(helpers.drop_factors(seed, 2 + 3 * l, M * T * D, hidden_p).view(M, T, D))
        masks.append(helpers.drop_factors(seed, 3 + 3 * l, M * T * D, hidden_p).view(M, T, D))
    return masks


def bert_hidden_states_dropped(text, w, cfg, masks):
    """`oracle.bert_hidden_states` (same statements, same order) with masks[k] multiplied in where HF's k-th dropout call sits."""
    n = text.shape[1] // 2
    ids, mask = text[:, :n].long(), text[:, n:]
    B, D, H = ids.shape[0], cfg.hidden, cfg.heads
    d = D // H
    it = iter(masks)
    x = w["word_emb"][ids] + w["pos_emb"][:n][None] + w["type_emb"][0][None, None]
    x = F.layer_norm(x, (D,), w["emb_ln_w"], w["emb_ln_b"], cfg.eps) * next(it)                     # 1. embeddings: hidden state 0
    key_bias = (1.0 - mask.to(torch.float32)) * torch.finfo(torch.float32).min
    hs = [x]
    for l in range(cfg.layers):
        p = f"L{l}."
        qkv = F.linear(x, w[p + "qkv_w"], w[p + "qkv_b"]).view(B, n, 3, H, d)
        q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))
        s = torch.matmul(q, k.transpose(-1, -2)) * (d ** -0.5) + key_bias[:, None, None, :]
        pr = torch.softmax(s, dim=-1) * next(it)                                                   # 2. probabilities, no renormalisation
        ctx = torch.matmul(pr, v).transpose(1, 2).reshape(B, n, D)
        a = F.linear(ctx, w[p + "o_w"], w[p + "o_b"]) * next(it)                                   # 3. BertSelfOutput
        a = F.layer_norm(a + x, (D,), w[p + "ln1_w"], w[p + "ln1_b"], cfg.eps)
        f = F.linear(F.gelu(F.linear(a, w[p + "fc1_w"], w[p + "fc1_b"])), w[p + "fc2_w"], w[p + "fc2_b"]) * next(it)   # 4. BertOutput
        x = F.layer_norm(f + a, (D,), w[p + "ln2_w"], w[p + "ln2_b"], cfg.eps)
        hs.append(x)
    return hs


def dropout_text(M=5, T=30, vocab=512, seed=5):
    """[M, 2T] ids | attention mask: item 0 all-masked (a padding slot), item 1 partly masked."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, vocab, (M, T), generator=g)
    mask = torch.ones(M, T, dtype=torch.int64)
    ids[0] = 0
    mask[0] = 0
    mask[1, T // 3:] = 0
    ids[1, T // 3:] = 0
    return torch.cat([ids, mask], 1)


def test_masks_sit_where_hf_applies_dropout(monkeypatch):
    transformers = pytest.importorskip("transformers")
    cfg = gio.E2E_BERT
    M, T, p = 5, 30, 0.1
    hf_cfg = transformers.BertConfig(hidden_size=cfg.hidden, num_hidden_layers=cfg.layers, num_attention_heads=cfg.heads,
                                     intermediate_size=cfg.mlp, vocab_size=cfg.vocab, max_position_embeddings=cfg.max_pos,
                                     layer_norm_eps=cfg.eps, hidden_dropout_prob=p, attention_probs_dropout_prob=p)
    hf_cfg._attn_implementation = "eager"
    torch.manual_seed(3)
    model = transformers.BertModel(hf_cfg, add_pooling_layer=False)
    model.train()
    w = weights.bert_from_hf(model.state_dict())
    text = dropout_text(M, T, cfg.vocab)
    masks = drop_masks(1234567, M, T, cfg, p, p)
    for m in masks:
        assert abs((m != 0).float().mean().item() - (1 - p)) < 0.01
        assert set(m.unique().tolist()) == {0.0, float(torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p)))}

    calls = []

    def prepared_dropout(input, p=0.5, training=True, inplace=False):
        assert training and abs(p - 0.1) < 1e-9
        k = len(calls)
        calls.append(tuple(input.shape))
        return input * masks[k]

    monkeypatch.setattr(torch.nn.functional, "dropout", prepared_dropout)
    with torch.no_grad():
        out = model(input_ids=text[:, :T], attention_mask=text[:, T:], output_hidden_states=True)
    monkeypatch.undo()
    D, H = cfg.hidden, cfg.heads
    assert calls == [(M, T, D)] + [(M, H, T, T), (M, T, D), (M, T, D)] * cfg.layers
    with torch.no_grad():
        mine = bert_hidden_states_dropped(text, w, cfg, masks)
        ones = bert_hidden_states_dropped(text, w, cfg, [torch.ones_like(m) for m in masks])
        plain = O.bert_hidden_states(text, w, cfg)
    assert len(out.hidden_states) == cfg.layers + 1
    for l, (a, b) in enumerate(zip(mine, out.hidden_states)):
        err = (a - b).abs().max().item()
        print(f"hidden state {l}: max |restatement - HF| = {err:.2e} at values up to {b.abs().max().item():.2f}")
        assert err < 1e-5, (l, err)
    for a, b in zip(ones, plain):
        assert torch.equal(a, b)
    # the effect is not small: every CLS tap moves by tens of per cent
    for a, b in zip(mine, plain):
        assert ((a[:, 0] - b[:, 0]).norm() / b[:, 0].norm()).item() > 0.1


def test_dropout_struct_layout_matches_c(tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "iisan_hip.h"\nint main(){printf("%zu %zu %zu %zu\\n",'
                    'sizeof(iisan_bert_dropout),offsetof(iisan_bert_dropout,hidden_p),offsetof(iisan_bert_dropout,attn_p),'
                    'offsetof(iisan_bert_dropout,seed));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(_lib.BertDropout), _lib.BertDropout.hidden_p.offset, _lib.BertDropout.attn_p.offset, _lib.BertDropout.seed.offset]
    assert got == want == [16, 0, 4, 8], (got, want)


def test_the_python_switch():
    from iisan_amd.model import encoders as menc
    args = helpers.make_args()
    frozen = menc.FrozenBert({}, weights.BertConfig())
    te = menc.Text_Encoder(frozen, args, 64, 768)
    assert te.train_dropout is False
    te.train()
    assert te.step_dropout() is None                  # switch off
    te.train_dropout = True
    te.eval()
    assert te.step_dropout() is None                  # eval mode
    te.train()
    a, b = te.step_dropout(), te.step_dropout()
    assert a[:2] == (0.1, 0.1) and b[:2] == (0.1, 0.1) and a[2] != b[2]
    assert 0 <= a[2] < 2 ** 62
    with torch.no_grad():                             # evaluate.item_table: forward_item3 under no_grad, the model still in train()
        assert te.step_dropout() is None
    # the seed comes from the torch CPU generator
    torch.manual_seed(11)
    s1 = te.step_dropout()[2]
    torch.manual_seed(11)
    assert te.step_dropout()[2] == s1
    # other probabilities in the container's config; both zero = nothing to do
    te2 = menc.Text_Encoder(menc.FrozenBert({}, weights.BertConfig(hidden_dropout=0.25, attn_dropout=0.0)), args, 64, 768)
    te2.train_dropout = True
    assert te2.train().step_dropout()[:2] == (0.25, 0.0)
    te3 = menc.Text_Encoder(menc.FrozenBert({}, weights.BertConfig(hidden_dropout=0.0, attn_dropout=0.0)), args, 64, 768)
    te3.train_dropout = True
    assert te3.train().step_dropout() is None
    # a HuggingFace module: the probabilities of its config
    hf = torch.nn.Module()
    hf.config = types.SimpleNamespace(hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    te4 = menc.Text_Encoder(hf, args, 64, 768)
    te4.train_dropout = True
    assert te4.train().step_dropout()[:2] == (0.1, 0.1)
    # Bert_Encoder passes the question on to its title encoder
    be = menc.Bert_Encoder(args, frozen)
    assert be.train().step_dropout() is None
    be.text_encoders["title"].train_dropout = True
    assert be.step_dropout()[:2] == (0.1, 0.1)


def test_the_python_switch_reads_a_real_hf_config():
    transformers = pytest.importorskip("transformers")
    from iisan_amd.model import encoders as menc
    cfg = gio.E2E_BERT
    model = transformers.BertModel(transformers.BertConfig(hidden_size=cfg.hidden, num_hidden_layers=1, num_attention_heads=cfg.heads,
                                                           intermediate_size=cfg.mlp, vocab_size=cfg.vocab,
                                                           max_position_embeddings=cfg.max_pos), add_pooling_layer=False)
    te = menc.Text_Encoder(model, helpers.make_args(), 64, 768)
    te.train_dropout = True
    assert te.train().step_dropout()[:2] == (0.1, 0.1)
    bc = menc._bert_canonical(model)[1]
    assert (bc.hidden_dropout, bc.attn_dropout) == (0.1, 0.1)


def test_dropout_kernels_have_no_scratch_and_no_spilled_vgpr(tmp_path):
    import test_isa_screen as isa
    meta, txt = isa._kernel_meta(os.path.join(isa.CSRC, "bert_drop.hip"), tmp_path)
    assert sum("attention16_drop_kernel" in k for k in meta) == len(meta) == 20, sorted(meta)
    # the three hidden sites: the instantiations of the eval-mode row kernels that carry the keep functor (`7RowKeep` in the mangled
    # name; the eval-mode ones carry `11RowKeepNone`), 768 wide
    rows_meta, rows_txt = isa._kernel_meta(os.path.join(isa.CSRC, "rowops.hip"), tmp_path)
    train = {k: m for k, m in rows_meta.items() if "Li768E7RowKeepE" in k}
    for family, n in (("25layernorm768_mixed_kernelI", 3), ("19layernorm768_kernelI", 2), ("20bert_embed_ln_kernelI", 4)):
        assert sum(family in k for k in train) == n, (family, sorted(train))
    assert len(train) == 9 and not any("7RowKeepE" in k for k in set(rows_meta) - set(train)), sorted(train)
    meta.update(train)
    for name, m in meta.items():
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0, (name, m)
    # the text tower's instantiations (S <= 32) leave room for several waves per SIMD
    for name, m in meta.items():
        if "attention16_drop_kernel" in name and "Li2E" in name:
            assert m["vgpr"] <= 128, (name, m)
    assert not isa._opsel_sites(txt) and not isa._opsel_sites(rows_txt)
