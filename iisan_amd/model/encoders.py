"""Encoders mirroring `Code_Uncached/model/encoders.py`: `MM_Encoder`, `Vit_Encoder`, `ClipVit_Encoder`, `Bert_Encoder`,
`Text_Encoder`, `User_Encoder` — same constructors, attribute paths and state-dict keys.

The frozen ViT/BERT are accepted as HuggingFace modules (`ViTForImageClassification`, `BertModel` or `DebertaV2Model`, either
state-dict layout) or as the light `FrozenVit` / `FrozenBert` / `FrozenDeberta` containers below; their weights are packed once into
kernel layout (`iisan_amd.encoders.PackedVit/PackedBert`) the first time a forward runs on the GPU.
"""
import torch
import torch.nn as nn
from torch.nn.init import constant_, xavier_normal_

from .. import _lib, encoders as enc, ops, weights
from .modules import TransformerEncoder

__all__ = ["MM_Encoder", "Vit_Encoder", "ClipVit_Encoder", "Bert_Encoder", "Text_Encoder", "User_Encoder", "FrozenVit", "FrozenBert", "FrozenDeberta"]


class FrozenVit(nn.Module):
    """Minimal stand-in for `ViTForImageClassification`: the frozen canonical weights (a plain dict, NOT part of
    `state_dict()`: a checkpoint of a model built on this container holds the trainable tensors only) + the trainable
    `classifier` head the reference re-creates (`Code_Uncached/run.py:56-61`).  Hand a real HF module to `ModelMM`
    instead when checkpoints must carry the encoder weights under the reference's keys."""

    def __init__(self, w: dict, cfg: weights.VitConfig, embedding_dim: int = 64):
        super().__init__()
        self.cfg = cfg
        self.canonical = {k: v for k, v in w.items()}
        self.classifier = nn.Linear(cfg.hidden, embedding_dim)
        xavier_normal_(self.classifier.weight.data)
        constant_(self.classifier.bias.data, 0)

    def canonical_weights(self):
        return self.canonical, self.cfg


class FrozenBert(nn.Module):
    def __init__(self, w: dict, cfg: weights.BertConfig):
        super().__init__()
        self.cfg = cfg
        self.canonical = {k: v for k, v in w.items()}

    def canonical_weights(self):
        return self.canonical, self.cfg


def _vit_canonical(image_net):
    if hasattr(image_net, "canonical_weights"):
        return image_net.canonical_weights()
    c = image_net.config                                   # HuggingFace module
    cfg = weights.VitConfig(hidden=c.hidden_size, layers=c.num_hidden_layers, heads=c.num_attention_heads,
                            mlp=c.intermediate_size, image=c.image_size, patch=c.patch_size, channels=c.num_channels,
                            eps=c.layer_norm_eps)
    return weights.vit_from_hf({k: v for k, v in image_net.state_dict().items() if not k.startswith("classifier")}), cfg


def _clip_canonical(image_net):
    """(canonical weights, config) of a CLIP vision tower: a `FrozenVit` on a CLIP config, or an HF `CLIPVisionModel` /
    `CLIPVisionTransformer` (`clip_model.vision_model`, `Code_Uncached/run.py:47-48`) — either key prefix."""
    if hasattr(image_net, "canonical_weights"):
        w, cfg = image_net.canonical_weights()
        if not cfg.pre_ln:
            raise ValueError("ClipVit_Encoder: the FrozenVit container holds a plain ViT config (pre_ln = False); wrap it in Vit_Encoder")
        return w, cfg
    c = getattr(image_net.config, "vision_config", image_net.config)       # (a whole CLIPModel's config nests the tower's)
    if c.hidden_act not in ("quick_gelu", "gelu"):
        raise ValueError(f"ClipVit_Encoder: hidden_act {c.hidden_act!r} is neither 'quick_gelu' (OpenAI) nor 'gelu' (LAION)")
    w = weights.clip_vit_from_hf({k: v for k, v in image_net.state_dict().items() if not k.startswith("classifier")})
    cfg = weights.VitConfig(hidden=c.hidden_size, layers=c.num_hidden_layers, heads=c.num_attention_heads,
                            mlp=c.intermediate_size, image=c.image_size, patch=c.patch_size, channels=c.num_channels,
                            eps=c.layer_norm_eps, pre_ln=True, act=c.hidden_act, patch_bias="patch_b" in w)
    return w, cfg


class FrozenDeberta(FrozenBert):
    """The same stand-in for `DebertaV2Model` (`Code_Uncached/run.py:71-81`): canonical DeBERTa weights + a `weights.DebertaConfig`."""

    def __init__(self, w: dict, cfg: weights.DebertaConfig):
        if not isinstance(cfg, weights.DebertaConfig):
            raise ValueError(f"FrozenDeberta: a weights.DebertaConfig is needed, not {type(cfg).__name__}")
        super().__init__(w, cfg)


def _deberta_canonical(bert_model):
    """(canonical weights, DebertaConfig) of an HF `DebertaV2Model` in the one configuration the executor implements — what the v3 xsmall /
    small / base / large checkpoints carry; anything else is refused here, naming the config field, never run approximately."""
    c = bert_model.config
    pos_att = set(c.pos_att_type or ())
    refusals = (
        ("conv_kernel_size", int(getattr(c, "conv_kernel_size", 0) or 0) > 0, "the convolutional v2-xlarge / xxlarge variants are not implemented"),
        ("position_biased_input", bool(c.position_biased_input), "absolute position embeddings in the input are not implemented"),
        ("relative_attention", not c.relative_attention, "the tower is built around relative attention"),
        ("share_att_key", not getattr(c, "share_att_key", False), "separate pos_key_proj / pos_query_proj matrices are not implemented"),
        ("pos_att_type", pos_att != {"c2p", "p2c"}, f"{sorted(pos_att)}: both terms, c2p and p2c, are needed"),
        ("embedding_size", getattr(c, "embedding_size", c.hidden_size) != c.hidden_size, "embedding_size != hidden_size (embed_proj) is not implemented"),
        ("norm_rel_ebd", "layer_norm" not in str(getattr(c, "norm_rel_ebd", "none")).lower(), "the relative-position table must be LayerNorm'd (layer_norm)"),
        ("type_vocab_size", int(c.type_vocab_size) > 0, "token-type embeddings are not implemented"),
    )
    for field, bad, why in refusals:
        if bad:
            raise ValueError(f"DeBERTa tower: config.{field} = {getattr(c, field, None)!r} is not supported: {why}")
    buckets = int(c.position_buckets) if c.position_buckets > 0 else int(c.max_relative_positions)
    cfg = weights.DebertaConfig(hidden=c.hidden_size, layers=c.num_hidden_layers, heads=c.num_attention_heads, mlp=c.intermediate_size,
                                vocab=c.vocab_size, max_pos=c.max_position_embeddings, position_buckets=buckets, eps=c.layer_norm_eps,
                                hidden_dropout=float(c.hidden_dropout_prob), attn_dropout=float(c.attention_probs_dropout_prob))
    return weights.deberta_from_hf(bert_model.state_dict()), cfg


def _is_deberta(bert_model) -> bool:
    if hasattr(bert_model, "canonical_weights"):
        return isinstance(bert_model.canonical_weights()[1], weights.DebertaConfig)
    return getattr(bert_model.config, "model_type", "") == "deberta-v2"


def _bert_canonical(bert_model):
    if hasattr(bert_model, "canonical_weights"):
        return bert_model.canonical_weights()
    if _is_deberta(bert_model):
        return _deberta_canonical(bert_model)
    c = bert_model.config
    cfg = weights.BertConfig(hidden=c.hidden_size, layers=c.num_hidden_layers, heads=c.num_attention_heads,
                             mlp=c.intermediate_size, vocab=c.vocab_size, max_pos=c.max_position_embeddings,
                             eps=c.layer_norm_eps, hidden_dropout=float(c.hidden_dropout_prob),
                             attn_dropout=float(c.attention_probs_dropout_prob))
    return weights.bert_from_hf(bert_model.state_dict()), cfg


def _drop_packed(module, incompatible_keys):
    module._packed = None


class Vit_Encoder(nn.Module):                      # encoders.py:23-31
    def __init__(self, image_net, dtype16: int = _lib.IISAN_F16):
        super().__init__()
        self.image_net = image_net
        self.activate = nn.GELU()
        self.dtype16 = dtype16
        self.chunk_items = 0
        self._packed = None
        # the kernel-layout copy is built lazily from the module's weights: a later load_state_dict must not leave a stale one
        self.register_load_state_dict_post_hook(_drop_packed)

    def packed(self, device) -> enc.PackedVit:
        if self._packed is None or self._packed.device != torch.device(device):
            w, cfg = self._canonical()
            self._packed = enc.PackedVit(w, cfg, device, self.dtype16)
        return self._packed

    def _canonical(self):
        return _vit_canonical(self.image_net)

    @property
    def n_layers(self):
        return self._canonical()[1].layers if self._packed is None else self._packed.cfg.layers

    def forward_taps(self, item_content, tap_layers):
        """CLS rows of the requested hidden states, [M, len(tap_layers), D] fp32 (no grad); D = the tower's hidden size (768 or 1024)."""
        with torch.no_grad():
            pk = self.packed(item_content.device)
            pk.full_blocks = getattr(self, "full_blocks", False)      # True: every block on every token, like HF (bench.py)
            return pk.forward_taps(item_content.contiguous(), list(tap_layers), self.chunk_items)

    def forward_taps_indexed(self, catalogue_u8, index, tap_layers):
        """The same for slots that name rows of a device-resident uint8 catalogue (`iisan_amd.itemstore`); index values
        outside the catalogue are padding slots."""
        with torch.no_grad():
            pk = self.packed(index.device)
            pk.full_blocks = getattr(self, "full_blocks", False)
            return pk.forward_taps_indexed(catalogue_u8, index, list(tap_layers), self.chunk_items)

    def forward(self, item_content):
        """Reference signature (`encoders.py:29-31`).  Returns `(None, hidden_states)` where each hidden state is the
        [M,1,768] CLS row (`h[:,0]` is what IISAN reads, `model.py:212`); the dead GELU(classifier(...)) output of
        the reference is not produced."""
        L = self.packed(item_content.device).cfg.layers
        taps = self.forward_taps(item_content, range(L + 1))
        return None, tuple(taps[:, l:l + 1] for l in range(L + 1))


class ClipVit_Encoder(Vit_Encoder):
    """The image tower `MM_Encoder` builds when `'clip-vit' in args.CV_model_load` (`Code_Uncached/model/encoders.py:9-10`; the reference
    calls the class and never defines it): a frozen CLIP vision transformer — pre-LayerNorm, quick-GELU (or erf-GELU, by `hidden_act`), no
    patch bias — with the `forward` / `forward_taps` / `forward_taps_indexed` surface of `Vit_Encoder`.  `hidden_states[0]` is the
    pre-LayerNorm's output, as in HF; `post_layernorm` and any projection are not part of it.
    The trainable head is `classifier`, `Linear(hidden, item_dim)`, where the reference's forward looks for it
    (`Code_Uncached/model/model.py:261-262`: `self.cv_encoder.classifier`).  The same module is also reachable as
    `image_net.classifier` — created there when the tower has none (an HF module), taken from there when it has (`FrozenVit`) — the
    path the side network and the Cached wrapper read for every image tower."""

    def __init__(self, image_net, item_dim, dtype16: int = _lib.IISAN_F16):
        super().__init__(image_net, dtype16)
        hidden = _clip_canonical(image_net)[1].hidden
        head = getattr(image_net, "classifier", None)
        if head is None:
            head = nn.Linear(hidden, item_dim)
            xavier_normal_(head.weight.data)
            constant_(head.bias.data, 0)
            image_net.classifier = head
        elif head.in_features != hidden or head.out_features != item_dim:
            raise ValueError(f"ClipVit_Encoder: the tower's classifier is {head.in_features} -> {head.out_features}, expected {hidden} -> {item_dim}")
        self.classifier = head

    def _canonical(self):
        return _clip_canonical(self.image_net)


class User_Encoder(nn.Module):                     # encoders.py:44-65
    def __init__(self, item_num, max_seq_len, item_dim, num_attention_heads, dropout, n_layers):
        super().__init__()
        self.transformer_encoder = TransformerEncoder(n_vocab=item_num, n_position=max_seq_len, d_model=item_dim,
                                                      n_heads=num_attention_heads, dropout=dropout, n_layers=n_layers)
        self.apply(self._init_weights)

    def _init_weights(self, module):
        if isinstance(module, nn.Embedding):
            xavier_normal_(module.weight.data)
        elif isinstance(module, nn.Linear):
            xavier_normal_(module.weight.data)
            if module.bias is not None:
                constant_(module.bias.data, 0)

    def forward(self, input_embs, log_mask, local_rank=None):
        return self.transformer_encoder(input_embs, log_mask, None)


class Text_Encoder(nn.Module):                     # encoders.py:68-91
    def __init__(self, bert_model, args, item_embedding_dim, word_embedding_dim, dtype16: int = _lib.IISAN_F16):
        super().__init__()
        self.bert_model = bert_model
        self.fc = nn.Linear(word_embedding_dim, item_embedding_dim)
        self.activate = nn.GELU()
        self.args = args
        self.dtype16 = dtype16
        self.chunk_items = 0
        self._packed = None
        # opt-in: the frozen tower's own dropout on the TRAINING forward, as HF's BertModel applies it under model.train()
        # (Code_Uncached/run.py:394).  Off (the default): the tower always runs in eval mode.  INTEGRATION.md, "Numeric deviations".
        self.train_dropout = False
        self.register_load_state_dict_post_hook(_drop_packed)

    def dropout_probs(self):
        """(hidden_dropout_prob, attention_probs_dropout_prob) of the wrapped tower: the HF config's, or the `BertConfig` fields of a
        `FrozenBert` container."""
        if hasattr(self.bert_model, "canonical_weights"):
            cfg = self.bert_model.canonical_weights()[1]
            return float(cfg.hidden_dropout), float(cfg.attn_dropout)
        c = self.bert_model.config
        return float(c.hidden_dropout_prob), float(c.attention_probs_dropout_prob)

    def step_dropout(self):
        """The `dropout` argument of one training forward: None unless `train_dropout and self.training`, else `(hidden_p, attn_p,
        seed)` with a fresh seed.  Only the training forward (`IISANAdaptedMModel.forward_item3[_indexed]`) asks for it: a bare
        `forward_taps(...)` is deterministic whatever the module's mode (evaluate.py builds its tap caches through it).  A forward
        under `torch.no_grad()` is not a training step either: `evaluate.item_table` goes through `forward_item3` that way, without
        `model.eval()`, and must give the same table whatever the switch says.
        A DeBERTa tower answers None whatever `train_dropout` says: its embedding step and its disentangled attention have no train-mode
        instantiation, the executor refuses a non-zero probability on such a tower, and the tower is eval only — like every BERT tower of a
        width other than 768 ("Numeric deviations")."""
        if not (self.train_dropout and self.training and torch.is_grad_enabled()):
            return None
        if _is_deberta(self.bert_model):
            return None
        hidden_p, attn_p = self.dropout_probs()
        if hidden_p <= 0.0 and attn_p <= 0.0:
            return None
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())      # CPU generator: no device sync (modules.TransformerEncoder.forward)
        return hidden_p, attn_p, seed

    def packed(self, device) -> enc.PackedBert:
        if self._packed is None or self._packed.device != torch.device(device):
            w, cfg = _bert_canonical(self.bert_model)
            self._packed = enc.PackedBert(w, cfg, device, self.dtype16)
        return self._packed

    def forward_taps(self, text, tap_layers, dropout=None):
        with torch.no_grad():
            pk = self.packed(text.device)
            pk.full_blocks = getattr(self, "full_blocks", False)
            return pk.forward_taps(text.contiguous().to(torch.int64), list(tap_layers), self.chunk_items, dropout=dropout)

    def forward_taps_indexed(self, table, index, tap_layers, dropout=None):
        with torch.no_grad():
            pk = self.packed(index.device)
            pk.full_blocks = getattr(self, "full_blocks", False)
            return pk.forward_taps_indexed(table, index, list(tap_layers), self.chunk_items, dropout=dropout)

    def forward(self, text):
        L = self.packed(text.device).cfg.layers
        taps = self.forward_taps(text, range(L + 1))
        return None, tuple(taps[:, l:l + 1] for l in range(L + 1))


class Bert_Encoder(nn.Module):                     # encoders.py:116-159
    def __init__(self, args, bert_model):
        super().__init__()
        self.args = args
        self.attributes2length = {'title': args.num_words_title * 2, 'abstract': args.num_words_abstract * 2,
                                  'body': args.num_words_body * 2}
        for key in list(self.attributes2length.keys()):
            if key not in args.news_attributes:
                self.attributes2length[key] = 0
        self.attributes2start = {key: sum(list(self.attributes2length.values())[:list(self.attributes2length.keys()).index(key)])
                                 for key in self.attributes2length.keys()}
        assert len(args.news_attributes) > 0
        self.text_encoders = nn.ModuleDict({'title': Text_Encoder(bert_model, args, args.embedding_dim, args.word_embedding_dim)})
        self.newsname = [name for name in set(args.news_attributes) & {'title', 'abstract', 'body'}]

    def _title(self, news):
        return torch.narrow(news, 1, self.attributes2start['title'], self.attributes2length['title'])

    def forward_taps(self, news, tap_layers, dropout=None):
        return self.text_encoders['title'].forward_taps(self._title(news), tap_layers, dropout=dropout)

    def step_dropout(self):
        """`Text_Encoder.step_dropout` of the title encoder (None: eval mode)."""
        return self.text_encoders['title'].step_dropout()

    def title_columns(self):
        """(start, length) of the title columns in an item-content row.  An item store narrows a wider table to them ONCE and keeps
        that contiguous copy (`iisan_amd.itemstore`: `narrow_text`), so that no step narrows or copies text."""
        return self.attributes2start['title'], self.attributes2length['title']

    def forward_taps_indexed(self, title_table, index, tap_layers, dropout=None):
        """`title_table` [rows, 2W]: the title columns only (see `title_columns`)."""
        if title_table.shape[1] != self.attributes2length['title']:
            raise ValueError(f"Bert_Encoder.forward_taps_indexed: the table is {title_table.shape[1]} columns wide, the title "
                             f"{self.attributes2length['title']}: narrow it once with the store's narrow_text(*title_columns())")
        return self.text_encoders['title'].forward_taps_indexed(title_table, index, tap_layers, dropout=dropout)

    def forward(self, news):
        return self.text_encoders['title'](self._title(news))


class MM_Encoder(nn.Module):                       # encoders.py:6-21
    def __init__(self, args, image_net, bert_model):
        super().__init__()
        if "clip-vit" in getattr(args, "CV_model_load", ""):       # encoders.py:9-12
            self.cv_encoder = ClipVit_Encoder(image_net=image_net, item_dim=args.embedding_dim)
        else:
            self.cv_encoder = Vit_Encoder(image_net=image_net)
        self.bert_encoder = Bert_Encoder(args=args, bert_model=bert_model)

    def forward(self, sample_items_images, sample_items_text):
        raise NotImplementedError("MM_Encoder without the IISAN wrapper is the reference's full-fine-tuning baseline "
                                  "(encoders.py:17-21), outside the IISAN hot path; wrap it with IISANAdaptedMModel")
