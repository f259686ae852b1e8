"""DeBERTa-v2/v3 text towers, the part that needs no GPU: the config presets, the state-dict key map, the HF module at the boundary, the
refusals of unsupported configurations, the float64 restatement against HuggingFace's own outputs, the padded-id invariant, the C struct,
the executor's plan and the ABI-level refusals that come before any launch.  The GPU side is tests/test_gpu_deberta.py."""
import ctypes as C
import os
import subprocess
import types

import pytest
import torch

import deberta_oracle as DO
import helpers
from iisan_amd import _lib, weights
from iisan_amd.model import encoders as menc

HERE = os.path.dirname(os.path.abspath(__file__))
F16, BF16 = _lib.IISAN_F16, _lib.IISAN_BF16
TOY = weights.DebertaConfig(hidden=128, layers=2, heads=2, mlp=256, vocab=64, position_buckets=16)


def test_config_presets_and_config_dict():
    P = {"XSMALL": (384, 12, 6, 1536), "SMALL": (768, 6, 12, 3072), "BASE": (768, 12, 12, 3072), "LARGE": (1024, 24, 16, 4096)}
    for name, (hidden, layers, heads, mlp) in P.items():
        cfg = getattr(weights, "DEBERTA_V3_" + name)
        assert (cfg.hidden, cfg.layers, cfg.heads, cfg.mlp) == (hidden, layers, heads, mlp) and cfg.hidden == 64 * cfg.heads
        assert cfg.vocab == 128100 and cfg.position_buckets == 256 and cfg.eps == 1e-7 and cfg.max_words == 128
    d = weights.config_dict(weights.DEBERTA_V3_BASE)
    assert d == dict(hidden=768, layers=12, heads=12, mlp=3072, vocab=128100, max_pos=512, position_buckets=256, eps=1e-7,
                     hidden_dropout=0.1, attn_dropout=0.1)
    assert weights.DebertaConfig(**d) == weights.DEBERTA_V3_BASE and TOY.max_words == 8


def test_key_map_round_trips_with_and_without_the_prefix():
    w = weights.make_deberta_weights(TOY, seed=3)
    assert "pos_emb" not in w and "type_emb" not in w and w["rel_emb"].shape == (32, 128) and w["L1.qkv_w"].shape == (384, 128)
    assert weights.make_deberta_weights(TOY, seed=3)["L1.fc2_w"].equal(w["L1.fc2_w"])
    for prefix in ("", "deberta."):
        sd = weights.deberta_to_hf(w, TOY, prefix)
        assert all(k.startswith(prefix) for k in sd)
        assert sd[prefix + "encoder.layer.1.attention.self.key_proj.weight"].equal(w["L1.qkv_w"][128:256])
        assert prefix + "encoder.rel_embeddings.weight" in sd and prefix + "encoder.LayerNorm.bias" in sd
        # what a task checkpoint carries beside the tower is dropped
        sd["cls.predictions.bias"] = torch.zeros(3)
        sd[prefix + "embeddings.position_ids"] = torch.arange(4)[None]
        back = weights.deberta_from_hf(sd)
        assert set(back) == set(w) and all(torch.equal(back[k], w[k]) for k in w)
    # state dicts of unsupported configurations are named by the key that shows them
    sd = weights.deberta_to_hf(w, TOY)
    for key, field in (("embeddings.position_embeddings.weight", "position_biased_input"), ("encoder.conv.conv.weight", "conv_kernel_size"),
                       ("embeddings.embed_proj.weight", "embedding_size"), ("encoder.layer.0.attention.self.pos_key_proj.weight", "share_att_key")):
        with pytest.raises(ValueError, match=field):
            weights.deberta_from_hf({**sd, key: torch.zeros(1)})
    with pytest.raises(ValueError, match="rel_embeddings"):
        weights.deberta_from_hf({k: v for k, v in sd.items() if "rel_embeddings" not in k})


def _args():
    return helpers.make_args(num_words_title=8, word_embedding_dim=128)


def test_huggingface_module_at_the_boundary_yields_the_canonical_weights():
    tf = pytest.importorskip("transformers")
    hc = tf.DebertaV2Config(**weights.deberta_hf_config_kwargs(TOY))
    model = tf.DebertaV2Model(hc).eval()
    assert model.config.model_type == "deberta-v2"
    w = weights.make_deberta_weights(TOY, seed=4)
    model.load_state_dict(weights.deberta_to_hf(w, TOY))
    te = menc.Text_Encoder(model, _args(), 64, 128)
    got, cfg = menc._bert_canonical(te.bert_model)
    assert cfg == TOY and set(got) == set(w) and all(torch.equal(got[k], w[k]) for k in w)
    te.train_dropout = True
    te.train()
    assert te.dropout_probs() == (0.1, 0.1) and te.step_dropout() is None


class _FakeHF:
    """the surface `_bert_canonical` reads of an HF module: `.config` and `.state_dict()`"""

    def __init__(self, **over):
        kw = weights.deberta_hf_config_kwargs(TOY)
        kw.update(model_type="deberta-v2", conv_kernel_size=0, embedding_size=TOY.hidden)
        kw.update(over)
        self.config = types.SimpleNamespace(**kw)

    def state_dict(self):
        return weights.deberta_to_hf(weights.make_deberta_weights(TOY, seed=4), TOY)


def test_unsupported_configurations_are_refused_by_name():
    w, cfg = menc._bert_canonical(_FakeHF())
    assert cfg == TOY and "rel_emb" in w
    for field, over in (("conv_kernel_size", dict(conv_kernel_size=3)), ("position_biased_input", dict(position_biased_input=True)),
                        ("share_att_key", dict(share_att_key=False)), ("pos_att_type", dict(pos_att_type=["c2p"])),
                        ("pos_att_type", dict(pos_att_type=[])), ("embedding_size", dict(embedding_size=64)),
                        ("relative_attention", dict(relative_attention=False)), ("norm_rel_ebd", dict(norm_rel_ebd="none"))):
        with pytest.raises(ValueError, match=field):
            menc._bert_canonical(_FakeHF(**over))
    # a BERT module still goes the BERT way, a container by its config
    fz = menc.FrozenDeberta(weights.make_deberta_weights(TOY, seed=4), TOY)
    assert menc._is_deberta(fz) and menc._bert_canonical(fz)[1] is TOY
    bcfg = weights.BertConfig(hidden=128, layers=2, heads=2, mlp=256, vocab=64, max_pos=16)
    assert not menc._is_deberta(menc.FrozenBert(weights.make_bert_weights(bcfg, seed=1), bcfg))
    with pytest.raises(ValueError, match="DebertaConfig"):
        menc.FrozenDeberta({}, bcfg)


def test_step_dropout_is_none_for_a_deberta_tower_whatever_train_dropout_says():
    te = menc.Text_Encoder(menc.FrozenDeberta(weights.make_deberta_weights(TOY, seed=4), TOY), _args(), 64, 128)
    te.train_dropout = True
    te.train()
    assert te.dropout_probs() == (0.1, 0.1) and te.step_dropout() is None
    bcfg = weights.BertConfig(hidden=128, layers=2, heads=2, mlp=256, vocab=64, max_pos=16)
    tb = menc.Text_Encoder(menc.FrozenBert(weights.make_bert_weights(bcfg, seed=1), bcfg), _args(), 64, 128)
    tb.train_dropout = True
    tb.train()
    assert tb.step_dropout() is not None


@pytest.mark.parametrize("name", sorted(DO.TOWERS))
def test_float64_restatement_matches_the_huggingface_golden(name):
    """`deberta_oracle.deberta_cls_taps` against `hidden_states[l][:, 0]` of HF's DebertaV2Model (fp32, eager attention), every layer and
    every slot — the all-masked one too — at the 2e-5 relative per tap that tests/test_oracle_vs_golden.py holds fp32 HF output to."""
    cfg, w, x, gold = DO.load_golden(name)
    assert gold.shape == (4, cfg.layers + 1, cfg.hidden) and gold.dtype == torch.float32
    got = DO.deberta_cls_taps(x, w, cfg)
    errs = DO.tap_errors(got, gold)
    print(name, " ".join(f"{e:.1e}" for e in errs))
    assert max(errs) <= 2e-5, errs
    assert (gold[0, 0] == 0).all() and gold[0, 1].abs().max() > 0       # the padding item: a zero row in, a real row out of block 0


def test_the_restatement_is_not_berts():
    """Without the positional terms, or with the tables indexed the other way round, the restatement is far off the golden."""
    cfg, w, x, gold = DO.load_golden("n8")
    orig = DO.disentangled_attention
    try:
        for kw in (dict(c2p=False, p2c=False), dict(flip=True)):
            DO.disentangled_attention = lambda *a, _kw=kw, **k: orig(*a, **{**k, **_kw})
            assert max(DO.tap_errors(DO.deberta_cls_taps(x, w, cfg)[:, 1:], gold[:, 1:])) > 1e-3
    finally:
        DO.disentangled_attention = orig


def test_taps_of_real_items_do_not_depend_on_the_ids_at_padded_positions():
    """On real items, every tap is bit-independent of the ids stored at padded positions: a masked token's row is exactly zero after the
    embedding step, and it is a key of no real query."""
    cfg, w, x, gold = DO.load_golden("n8")
    W = x.shape[1] // 2
    y = x.clone()
    pad = y[:, W:] == 0
    y[:, :W][pad] = torch.randint(1, cfg.vocab, (int(pad.sum()),), generator=torch.Generator().manual_seed(5))
    assert not torch.equal(x, y)
    a, b = DO.deberta_cls_taps(x, w, cfg), DO.deberta_cls_taps(y, w, cfg)
    assert torch.equal(a[1:], b[1:])


def test_bert_weights_struct_carries_the_deberta_fields_where_c_puts_them(tmp_path):
    """The ctypes mirror against gcc's layout of the new trailing fields (tests/test_abi.py compares the sizes)."""
    src = tmp_path / "l.c"
    fields = ("layer", "rel_emb", "rel_ln_w", "rel_ln_b", "span", "rel_proj")
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "iisan_hip.h"\nint main(){printf("%zu' + " %zu" * len(fields) + ' %d\\n",sizeof(iisan_bert_weights),'
                   + ",".join(f"offsetof(iisan_bert_weights,{f})" for f in fields) + ',IISAN_TOWER_DEBERTA);return 0;}\n')
    exe = tmp_path / "l"
    subprocess.check_call(["gcc", "-I", os.path.join(os.path.dirname(HERE), "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_lib.BertWeights)] + [getattr(_lib.BertWeights, f).offset for f in fields] + [_lib.IISAN_TOWER_DEBERTA]
    z = _lib.BertWeights()
    assert not z.rel_emb and not z.rel_proj and z.span == 0       # zero = today's BERT


def test_encoder_plan_answers_for_a_deberta_tower(lib):
    """IISAN_TOWER_DEBERTA = 3: the BERT executor's plan behind the DeBERTa refusals; the last argument is the span.  The four golden
    towers' shapes as a literal table (BERT bits: 1 mixed stream, 2 stream and image share a buffer — fp16 —, 4 block-major FC1 -> FC2 —
    where both products reach the 256x256 kernel: the wide towers at the production item count)."""
    DEB, BERT = _lib.IISAN_TOWER_DEBERTA, _lib.IISAN_TOWER_BERT
    plan = lambda tower, dt, D, H, F, W, M, L, span: lib.iisan_encoder_plan(tower, dt, D, H, F, W, M, 0, L, 0, span)
    shapes = {"b30": (768, 12, 512, 30, 2, 256), "x12": (384, 6, 1536, 30, 12, 256), "n8": (128, 2, 256, 8, 2, 16), "l128": (1024, 16, 512, 128, 2, 256)}
    table = {("b30", F16, 4): 3, ("b30", F16, 1408): 7, ("b30", BF16, 4): 1, ("b30", BF16, 1408): 5,
             ("x12", F16, 4): 3, ("x12", F16, 1408): 3, ("x12", BF16, 4): 1, ("x12", BF16, 1408): 1,
             ("n8", F16, 4): 3, ("n8", F16, 1408): 3, ("n8", BF16, 4): 1, ("n8", BF16, 1408): 1,
             ("l128", F16, 4): 3, ("l128", F16, 1408): 7, ("l128", BF16, 4): 1, ("l128", BF16, 1408): 5}
    for (name, dt, M), want in table.items():
        D, H, F, W, L, span = shapes[name]
        assert plan(DEB, dt, D, H, F, W, M, L, span) == want, (name, dt, M)
        assert plan(BERT, dt, D, H, F, W, M, L, 0) == want, (name, dt, M)
    with _lib.dev(resid32=1):
        assert plan(DEB, F16, 768, 12, 512, 30, 4, 2, 256) & 3 == 0
    EBADSHAPE = -1
    assert plan(DEB, F16, 768, 12, 512, 129, 4, 2, 256) == EBADSHAPE and b"129 words" in lib.iisan_last_error()
    assert plan(DEB, F16, 128, 2, 256, 9, 4, 2, 16) == EBADSHAPE and b"span / 2" in lib.iisan_last_error()
    assert plan(DEB, F16, 128, 2, 256, 8, 4, 2, 16) == 3
    assert plan(DEB, F16, 768, 12, 512, 30, 4, 2, 0) == EBADSHAPE and plan(DEB, F16, 768, 12, 512, 30, 4, 2, 257) == EBADSHAPE
    assert plan(DEB, F16, 512, 8, 512, 30, 4, 2, 256) == EBADSHAPE and plan(DEB, F16, 1280, 16, 512, 30, 4, 2, 256) == EBADSHAPE


def test_abi_refusals_come_before_any_launch(lib):
    """Dropout on a DeBERTa struct, a too-small workspace, a struct with a position table beside rel_emb: refused on a machine without a
    device — the checks precede the first launch.  (Null device pointers: nothing may dereference them.)"""
    s = _lib.BertWeights()
    s.hidden, s.layers, s.heads, s.mlp, s.vocab, s.max_pos, s.dtype16, s.eps = 128, 2, 2, 256, 64, 512, F16, 1e-7
    keep = torch.zeros(16)
    s.rel_emb = s.rel_ln_w = s.rel_ln_b = keep.data_ptr()
    s.span = 16
    taps = (C.c_int32 * 1)(1)
    drop = _lib.BertDropout(0.1, 0.1, 1)
    EBADSHAPE, EWORKSPACE = -1, -2
    rc = lib.iisan_bert_forward_taps_dropout(C.byref(s), keep.data_ptr(), 0, None, 4, 8, taps, 1, None, 0, C.byref(drop), None, 0, None)
    assert rc == EBADSHAPE and b"eval mode only" in lib.iisan_last_error()
    need = lib.iisan_bert_forward_taps_ws_bytes(C.byref(s), 4, 8, 0)
    rel, rel_ws = lib.iisan_deberta_rel_bytes(C.byref(s)), lib.iisan_deberta_rel_ws_bytes(C.byref(s))
    assert rel == 2 * 3 * 32 * 128 * 2 and rel_ws == 256 * 128 * 2
    b = _lib.BertWeights()
    b.hidden, b.layers, b.heads, b.mlp, b.vocab, b.max_pos, b.dtype16, b.eps = 128, 2, 2, 256, 64, 512, F16, 1e-7
    # the workspace grows by the tables and their scratch for a DeBERTa struct without rel_proj only
    assert need == lib.iisan_bert_forward_taps_ws_bytes(C.byref(b), 4, 8, 0) + rel + rel_ws
    assert lib.iisan_deberta_rel_bytes(C.byref(b)) == 0 and lib.iisan_deberta_rel_ws_bytes(C.byref(b)) == 0
    s.rel_proj = keep.data_ptr()
    assert lib.iisan_bert_forward_taps_ws_bytes(C.byref(s), 4, 8, 0) == need - rel - rel_ws
    s.rel_proj = None
    rc = lib.iisan_bert_forward_taps(C.byref(s), keep.data_ptr(), 4, 8, taps, 1, None, 0, keep.data_ptr(), need - 1, None)
    assert rc == EWORKSPACE and b"workspace too small" in lib.iisan_last_error()
    rc = lib.iisan_bert_forward_taps(C.byref(s), keep.data_ptr(), 4, 9, taps, 1, None, 0, keep.data_ptr(), 1 << 40, None)
    assert rc == EBADSHAPE and b"span / 2" in lib.iisan_last_error()
    s.pos_emb = keep.data_ptr()
    rc = lib.iisan_bert_forward_taps(C.byref(s), keep.data_ptr(), 4, 8, taps, 1, None, 0, keep.data_ptr(), 1 << 40, None)
    assert rc == EBADSHAPE and b"pos_emb" in lib.iisan_last_error()
    s.pos_emb = None
    assert lib.iisan_deberta_rel_project(C.byref(s), keep.data_ptr(), keep.data_ptr(), rel_ws - 1, None) == EWORKSPACE
    s.span = 300
    assert lib.iisan_deberta_rel_project(C.byref(s), keep.data_ptr(), keep.data_ptr(), 1 << 30, None) == EBADSHAPE
    for fn in (lib.iisan_attention16_disent, lib.iisan_attention_cls16_disent):
        assert fn(F16, keep.data_ptr(), keep.data_ptr(), None, keep.data_ptr(), 1, 129, 2, 256, None) == EBADSHAPE
        assert fn(F16, keep.data_ptr(), keep.data_ptr(), None, keep.data_ptr(), 1, 17, 2, 16, None) == EBADSHAPE
