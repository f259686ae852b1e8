"""Frozen-encoder weight containers for the IISAN hot path.

The reference never owns ViT/BERT weights itself: it loads HuggingFace checkpoints
(`Code_Uncached/run.py:50-100`) and only calls the two models' forward
(`Code_Uncached/model/encoders.py:30,86`).  The checkpoints are not shipped and there is no
network, so this module provides

* a *canonical* flat naming of the encoder tensors (what the HIP path packs into HBM),
* converters from both HuggingFace state-dict layouts (4.x `vit.encoder.layer.N.attention.attention.query`
  and 5.x `vit.layers.N.attention.q_proj`) into the canonical naming and back (5.x),
* a seeded generator (`numpy.random.RandomState`, whose stream is frozen by NumPy's compatibility
  policy) used by bench.py, the tests and the golden-fixture script so that the GPU box can rebuild the
  exact weights a fixture was generated with, without `transformers` and without shipping 800 MB.

Canonical names
---------------
ViT  : cls_token[D] pos_emb[T,D] patch_w[D,3*P*P] patch_b[D] lnf_w[D] lnf_b[D]
       CLIP vision towers (`VitConfig.pre_ln`): + pre_ln_w[D] pre_ln_b[D], no patch_b (`patch_bias = False`)
       L{l}.ln1_w L{l}.ln1_b L{l}.qkv_w[3D,D] L{l}.qkv_b[3D] L{l}.o_w[D,D] L{l}.o_b[D]
       L{l}.ln2_w L{l}.ln2_b L{l}.fc1_w[F,D] L{l}.fc1_b[F] L{l}.fc2_w[D,F] L{l}.fc2_b[D]
BERT : word_emb[V,D] pos_emb[P,D] type_emb[2,D] emb_ln_w emb_ln_b
       L{l}.qkv_w L{l}.qkv_b L{l}.o_w L{l}.o_b L{l}.ln1_w L{l}.ln1_b   (post-attention LayerNorm)
       L{l}.fc1_w L{l}.fc1_b L{l}.fc2_w L{l}.fc2_b L{l}.ln2_w L{l}.ln2_b (post-FFN LayerNorm)
DeBERTa-v2/v3 (`DebertaConfig`): the BERT names without pos_emb / type_emb, + rel_emb[2*position_buckets, D] rel_ln_w rel_ln_b
       (encoder.rel_embeddings, encoder.LayerNorm); qkv_w stacks query_proj / key_proj / value_proj
"""
from __future__ import annotations

from dataclasses import dataclass, asdict
from typing import Dict, Optional, Tuple

import math

import numpy as np
import torch


@dataclass(frozen=True)
class VitConfig:
    """Shape of the image tower (`pretrained_models/vit-base-patch16-224/config.json`)."""
    hidden: int = 768
    layers: int = 12
    heads: int = 12
    mlp: int = 3072
    image: int = 224
    patch: int = 16
    channels: int = 3
    eps: float = 1e-12
    # CLIP vision towers (HF `CLIPVisionModel`); the defaults are HF ViT
    pre_ln: bool = False            # a LayerNorm between the embeddings and block 0 (`pre_layrnorm`); hidden state 0 is its output
    act: str = "gelu"               # MLP activation, `config.hidden_act`: "gelu" (erf) or "quick_gelu" (x * sigmoid(1.702 x))
    patch_bias: bool = True         # the patch convolution has a bias (CLIP: none)
    # per-channel statistics of the uint8 entry points, None = the reference's transform (mean .5, std .5); fp32 images come normalised
    norm_mean: Optional[Tuple[float, float, float]] = None
    norm_std: Optional[Tuple[float, float, float]] = None

    def __post_init__(self):
        if self.act not in ("gelu", "quick_gelu"):
            raise ValueError(f"VitConfig.act {self.act!r}: 'gelu' or 'quick_gelu'")
        if (self.norm_mean is None) != (self.norm_std is None):
            raise ValueError("VitConfig.norm_mean and norm_std come together")

    @property
    def tokens(self) -> int:
        return (self.image // self.patch) ** 2 + 1

    @property
    def patch_dim(self) -> int:
        return self.channels * self.patch * self.patch

    @property
    def patch_ld(self) -> int:
        """Columns of a row of the PACKED patch weight (and of the patch matrix): `patch_dim`, zero-padded to the next multiple of 64
        when the patch side is no multiple of 8 (patch 14: 588 -> 640), so that the patch-embedding product keeps K % 64 == 0."""
        return self.patch_dim if self.patch % 8 == 0 else -(-self.patch_dim // 64) * 64


@dataclass(frozen=True)
class BertConfig:
    """Shape of the text tower (`pretrained_models/bert/bert_base_uncased/config.json`)."""
    hidden: int = 768
    layers: int = 12
    heads: int = 12
    mlp: int = 3072
    vocab: int = 30522
    max_pos: int = 512
    eps: float = 1e-12
    # hidden_dropout_prob / attention_probs_dropout_prob of the same config: read only by the opt-in train-mode dropout of the tower
    # (`Text_Encoder.train_dropout`); the eval-mode path never looks at them
    hidden_dropout: float = 0.1
    attn_dropout: float = 0.1


VIT_BASE = VitConfig()
BERT_BASE = BertConfig()
# the 1024-wide pair (HF `vit-large-patch16-224` / `bert-large-uncased`: 24 layers, 16 heads x 64, mlp 4096; 30522 words, eps 1e-12):
# the towers whose taps the Versa variant consumes (`Code_Cached_Asym/parameters.py`: text_embedding_dim 1024, text_layers 24)
VIT_LARGE = VitConfig(hidden=1024, layers=24, heads=16, mlp=4096)
BERT_LARGE = BertConfig(hidden=1024, layers=24, heads=16, mlp=4096)
# the edge towers (`Code_Cached_Asym/preprocess_edge_small.py` caches the per-layer CLS rows of `prajjwal1/bert-tiny` and
# `WinKawaks/vit-tiny-patch16-224`) and their next sizes up (`WinKawaks/vit-small-patch16-224`, `prajjwal1/bert-mini`): 64-wide heads
# like every tower here, hidden 128 - 384 (`vit_from_hf` / `bert_from_hf` read every shape off the state dict)
VIT_TINY = VitConfig(hidden=192, layers=12, heads=3, mlp=768)
VIT_SMALL = VitConfig(hidden=384, layers=12, heads=6, mlp=1536)
# ViT-H/14 (`Code_Cached_Asym/preprocess_vectors_vit_large.py:111` caches the CLS rows of all 33 hidden states of
# `google/vit-huge-patch14-224-in21k`): 16 heads of 80, 14-pixel patches (257 tokens at 224 pixels, a patch vector of 588)
VIT_HUGE = VitConfig(hidden=1280, layers=32, heads=16, mlp=5120, patch=14)
# CLIP vision towers (`Code_Uncached/run.py:46-49` loads `openai/clip-vit-base-patch32`): pre-LayerNorm, quick-GELU, no patch bias, eps 1e-5.
# OpenAI's pixel statistics are CLIP_MEAN / CLIP_STD; the constants keep the reference's (.5, .5) transform of the uint8 entries unless a
# caller sets them: `dataclasses.replace(CLIP_VIT_B32, norm_mean=CLIP_MEAN, norm_std=CLIP_STD)`
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
_CLIP = dict(eps=1e-5, pre_ln=True, act="quick_gelu", patch_bias=False)
CLIP_VIT_B32 = VitConfig(patch=32, **_CLIP)
CLIP_VIT_B16 = VitConfig(patch=16, **_CLIP)
CLIP_VIT_L14 = VitConfig(hidden=1024, layers=24, heads=16, mlp=4096, patch=14, **_CLIP)
@dataclass(frozen=True)
class DebertaConfig:
    """Shape of a DeBERTa-v2/v3 text tower (`Code_Uncached/run.py:71-81`: `DebertaV2Model` when 'deberta' is in `bert_model_load`), in the
    one configuration the v3 checkpoints carry: relative_attention, share_att_key, pos_att_type = c2p|p2c, norm_rel_ebd = layer_norm,
    position_biased_input = False, type_vocab_size = 0.  `position_buckets` is the `span` of the relative-position table [2 span, D];
    titles of at most span / 2 words are served (there HF's log-bucket map is the identity)."""
    hidden: int = 768
    layers: int = 12
    heads: int = 12
    mlp: int = 3072
    vocab: int = 128100
    max_pos: int = 512
    position_buckets: int = 256
    eps: float = 1e-7
    # of the HF config, for completeness: the tower runs in eval mode only (`Text_Encoder.step_dropout`)
    hidden_dropout: float = 0.1
    attn_dropout: float = 0.1

    @property
    def max_words(self) -> int:
        return min(self.position_buckets // 2, 128)


DEBERTA_V3_XSMALL = DebertaConfig(hidden=384, layers=12, heads=6, mlp=1536)
DEBERTA_V3_SMALL = DebertaConfig(hidden=768, layers=6, heads=12, mlp=3072)
DEBERTA_V3_BASE = DebertaConfig(hidden=768, layers=12, heads=12, mlp=3072)
DEBERTA_V3_LARGE = DebertaConfig(hidden=1024, layers=24, heads=16, mlp=4096)
BERT_TINY = BertConfig(hidden=128, layers=2, heads=2, mlp=512, vocab=30522, eps=1e-12)
BERT_MINI = BertConfig(hidden=256, layers=4, heads=4, mlp=1024, vocab=30522, eps=1e-12)


def _normal(rs: np.random.RandomState, shape, std: float) -> torch.Tensor:
    return torch.from_numpy((rs.standard_normal(size=shape) * std).astype(np.float32))


def make_vit_weights(cfg: VitConfig = VIT_BASE, seed: int = 1234, std: float = 0.02,
                     ln_jitter: float = 0.05) -> Dict[str, torch.Tensor]:
    """Seeded random ViT weights (fp32, CPU).  LayerNorm gains/biases and Linear biases are jittered away
    from their (1, 0, 0) defaults so that a kernel dropping one of them cannot pass a parity test."""
    rs = np.random.RandomState(seed)
    D, F = cfg.hidden, cfg.mlp
    w = {
        "cls_token": _normal(rs, (D,), std),
        "pos_emb": _normal(rs, (cfg.tokens, D), std),
        "patch_w": _normal(rs, (D, cfg.patch_dim), std),
        "patch_b": _normal(rs, (D,), std),
        "lnf_w": 1.0 + _normal(rs, (D,), ln_jitter),
        "lnf_b": _normal(rs, (D,), ln_jitter),
    }
    for l in range(cfg.layers):
        p = f"L{l}."
        w[p + "ln1_w"] = 1.0 + _normal(rs, (D,), ln_jitter)
        w[p + "ln1_b"] = _normal(rs, (D,), ln_jitter)
        w[p + "qkv_w"] = _normal(rs, (3 * D, D), std)
        w[p + "qkv_b"] = _normal(rs, (3 * D,), std)
        w[p + "o_w"] = _normal(rs, (D, D), std)
        w[p + "o_b"] = _normal(rs, (D,), std)
        w[p + "ln2_w"] = 1.0 + _normal(rs, (D,), ln_jitter)
        w[p + "ln2_b"] = _normal(rs, (D,), ln_jitter)
        w[p + "fc1_w"] = _normal(rs, (F, D), std)
        w[p + "fc1_b"] = _normal(rs, (F,), std)
        w[p + "fc2_w"] = _normal(rs, (D, F), std)
        w[p + "fc2_b"] = _normal(rs, (D,), std)
    # the extra tensors of a CLIP config are drawn LAST: every tensor above is, for a given seed, what a plain ViT config of the same shape gets
    if cfg.pre_ln:
        w["pre_ln_w"] = 1.0 + _normal(rs, (D,), ln_jitter)
        w["pre_ln_b"] = _normal(rs, (D,), ln_jitter)
    if not cfg.patch_bias:
        del w["patch_b"]
    return w


def make_bert_weights(cfg: BertConfig = BERT_BASE, seed: int = 4321, std: float = 0.02,
                      ln_jitter: float = 0.05) -> Dict[str, torch.Tensor]:
    rs = np.random.RandomState(seed)
    D, F = cfg.hidden, cfg.mlp
    w = {
        "word_emb": _normal(rs, (cfg.vocab, D), std),
        "pos_emb": _normal(rs, (cfg.max_pos, D), std),
        "type_emb": _normal(rs, (2, D), std),
        "emb_ln_w": 1.0 + _normal(rs, (D,), ln_jitter),
        "emb_ln_b": _normal(rs, (D,), ln_jitter),
    }
    for l in range(cfg.layers):
        p = f"L{l}."
        w[p + "qkv_w"] = _normal(rs, (3 * D, D), std)
        w[p + "qkv_b"] = _normal(rs, (3 * D,), std)
        w[p + "o_w"] = _normal(rs, (D, D), std)
        w[p + "o_b"] = _normal(rs, (D,), std)
        w[p + "ln1_w"] = 1.0 + _normal(rs, (D,), ln_jitter)
        w[p + "ln1_b"] = _normal(rs, (D,), ln_jitter)
        w[p + "fc1_w"] = _normal(rs, (F, D), std)
        w[p + "fc1_b"] = _normal(rs, (F,), std)
        w[p + "fc2_w"] = _normal(rs, (D, F), std)
        w[p + "fc2_b"] = _normal(rs, (D,), std)
        w[p + "ln2_w"] = 1.0 + _normal(rs, (D,), ln_jitter)
        w[p + "ln2_b"] = _normal(rs, (D,), ln_jitter)
    return w


def make_deberta_weights(cfg: DebertaConfig = DEBERTA_V3_BASE, seed: int = 2468, std: float = 0.02,
                         ln_jitter: float = 0.05) -> Dict[str, torch.Tensor]:
    """Seeded random DeBERTa weights: the BERT layer names, no pos_emb / type_emb, + rel_emb [2 span, D] and its LayerNorm rel_ln_w / rel_ln_b."""
    rs = np.random.RandomState(seed)
    D, F = cfg.hidden, cfg.mlp
    w = {
        "word_emb": _normal(rs, (cfg.vocab, D), std),
        "emb_ln_w": 1.0 + _normal(rs, (D,), ln_jitter),
        "emb_ln_b": _normal(rs, (D,), ln_jitter),
        "rel_emb": _normal(rs, (2 * cfg.position_buckets, D), std),
        "rel_ln_w": 1.0 + _normal(rs, (D,), ln_jitter),
        "rel_ln_b": _normal(rs, (D,), ln_jitter),
    }
    for l in range(cfg.layers):
        p = f"L{l}."
        w[p + "qkv_w"] = _normal(rs, (3 * D, D), std)
        w[p + "qkv_b"] = _normal(rs, (3 * D,), std)
        w[p + "o_w"] = _normal(rs, (D, D), std)
        w[p + "o_b"] = _normal(rs, (D,), std)
        w[p + "ln1_w"] = 1.0 + _normal(rs, (D,), ln_jitter)
        w[p + "ln1_b"] = _normal(rs, (D,), ln_jitter)
        w[p + "fc1_w"] = _normal(rs, (F, D), std)
        w[p + "fc1_b"] = _normal(rs, (F,), std)
        w[p + "fc2_w"] = _normal(rs, (D, F), std)
        w[p + "fc2_b"] = _normal(rs, (D,), std)
        w[p + "ln2_w"] = 1.0 + _normal(rs, (D,), ln_jitter)
        w[p + "ln2_b"] = _normal(rs, (D,), ln_jitter)
    return w


# ----------------------------------------------------------------------------------------------------------------
# HuggingFace state-dict <-> canonical
# ----------------------------------------------------------------------------------------------------------------

def _strip_prefix(sd: Dict[str, torch.Tensor], prefixes) -> Dict[str, torch.Tensor]:
    out = {}
    for k, v in sd.items():
        for p in prefixes:
            if k.startswith(p):
                k = k[len(p):]
                break
        out[k] = v
    return out


def vit_from_hf(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Canonical ViT weights from a `ViTForImageClassification`/`ViTModel` state dict (either HF layout).
    The classifier head is NOT part of the frozen encoder (it is the trainable `classifier` the reference
    re-creates at `Code_Uncached/run.py:57-61`) and is ignored here."""
    sd = _strip_prefix(sd, ("vit.",))
    w = {
        "cls_token": sd["embeddings.cls_token"].reshape(-1),
        "pos_emb": sd["embeddings.position_embeddings"].reshape(-1, sd["embeddings.position_embeddings"].shape[-1]),
        "patch_w": sd["embeddings.patch_embeddings.projection.weight"].reshape(
            sd["embeddings.patch_embeddings.projection.weight"].shape[0], -1),
        "patch_b": sd["embeddings.patch_embeddings.projection.bias"],
        "lnf_w": sd["layernorm.weight"],
        "lnf_b": sd["layernorm.bias"],
    }
    new = any(k.startswith("layers.") for k in sd)
    l = 0
    while True:
        if new:
            b = f"layers.{l}."
            names = dict(q=b + "attention.q_proj", k=b + "attention.k_proj", v=b + "attention.v_proj",
                         o=b + "attention.o_proj", fc1=b + "mlp.fc1", fc2=b + "mlp.fc2")
        else:
            b = f"encoder.layer.{l}."
            names = dict(q=b + "attention.attention.query", k=b + "attention.attention.key",
                         v=b + "attention.attention.value", o=b + "attention.output.dense",
                         fc1=b + "intermediate.dense", fc2=b + "output.dense")
        if names["q"] + ".weight" not in sd:
            break
        p = f"L{l}."
        w[p + "ln1_w"] = sd[b + "layernorm_before.weight"]
        w[p + "ln1_b"] = sd[b + "layernorm_before.bias"]
        w[p + "ln2_w"] = sd[b + "layernorm_after.weight"]
        w[p + "ln2_b"] = sd[b + "layernorm_after.bias"]
        w[p + "qkv_w"] = torch.cat([sd[names[x] + ".weight"] for x in "qkv"], 0)
        w[p + "qkv_b"] = torch.cat([sd[names[x] + ".bias"] for x in "qkv"], 0)
        for x in ("o", "fc1", "fc2"):
            w[p + x + "_w"] = sd[names[x] + ".weight"]
            w[p + x + "_b"] = sd[names[x] + ".bias"]
        l += 1
    return {k: v.detach().float().contiguous() for k, v in w.items()}


def clip_vit_from_hf(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Canonical weights of a CLIP vision tower from a `CLIPVisionModel` / `CLIPVisionTransformer` / `CLIPModel` state dict: keys with or
    without the `vision_model.` prefix.  `post_layernorm` (applied to the pooled output only, never to a hidden state), `position_ids`,
    any projection and, of a whole `CLIPModel`, the text tower are dropped; `pre_layrnorm` is HF's own spelling."""
    if any(k.startswith("vision_model.") for k in sd):
        sd = {k[len("vision_model."):]: v for k, v in sd.items() if k.startswith("vision_model.")}
    pos = sd["embeddings.position_embedding.weight"]
    pw = sd["embeddings.patch_embedding.weight"]
    w = {
        "cls_token": sd["embeddings.class_embedding"].reshape(-1),
        "pos_emb": pos.reshape(-1, pos.shape[-1]),
        "patch_w": pw.reshape(pw.shape[0], -1),
        "pre_ln_w": sd["pre_layrnorm.weight"],
        "pre_ln_b": sd["pre_layrnorm.bias"],
    }
    if "embeddings.patch_embedding.bias" in sd:
        w["patch_b"] = sd["embeddings.patch_embedding.bias"]
    l = 0
    while f"encoder.layers.{l}.self_attn.q_proj.weight" in sd:
        b, p = f"encoder.layers.{l}.", f"L{l}."
        w[p + "ln1_w"], w[p + "ln1_b"] = sd[b + "layer_norm1.weight"], sd[b + "layer_norm1.bias"]
        w[p + "ln2_w"], w[p + "ln2_b"] = sd[b + "layer_norm2.weight"], sd[b + "layer_norm2.bias"]
        w[p + "qkv_w"] = torch.cat([sd[b + f"self_attn.{x}_proj.weight"] for x in "qkv"], 0)
        w[p + "qkv_b"] = torch.cat([sd[b + f"self_attn.{x}_proj.bias"] for x in "qkv"], 0)
        w[p + "o_w"], w[p + "o_b"] = sd[b + "self_attn.out_proj.weight"], sd[b + "self_attn.out_proj.bias"]
        for x in ("fc1", "fc2"):
            w[p + x + "_w"], w[p + x + "_b"] = sd[b + f"mlp.{x}.weight"], sd[b + f"mlp.{x}.bias"]
        l += 1
    return {k: v.detach().float().contiguous() for k, v in w.items()}


def clip_vit_to_hf(w: Dict[str, torch.Tensor], cfg: VitConfig, prefix: str = "vision_model.") -> Dict[str, torch.Tensor]:
    """Canonical -> `CLIPVisionModel` state dict (`prefix = ""`: `CLIPVisionTransformer`), the inverse of `clip_vit_from_hf`;
    `post_layernorm`, which no hidden state passes through, is left to the caller.  Used by the golden-fixture script and the tests."""
    D = cfg.hidden
    sd = {
        "embeddings.class_embedding": w["cls_token"].reshape(D),
        "embeddings.position_embedding.weight": w["pos_emb"].reshape(cfg.tokens, D),
        "embeddings.patch_embedding.weight": w["patch_w"].reshape(D, cfg.channels, cfg.patch, cfg.patch),
        "pre_layrnorm.weight": w["pre_ln_w"],
        "pre_layrnorm.bias": w["pre_ln_b"],
    }
    if "patch_b" in w:
        sd["embeddings.patch_embedding.bias"] = w["patch_b"]
    for l in range(cfg.layers):
        p, b = f"L{l}.", f"encoder.layers.{l}."
        for x, ww, bb in zip("qkv", w[p + "qkv_w"].split(D, 0), w[p + "qkv_b"].split(D, 0)):
            sd[b + f"self_attn.{x}_proj.weight"], sd[b + f"self_attn.{x}_proj.bias"] = ww, bb
        sd[b + "self_attn.out_proj.weight"], sd[b + "self_attn.out_proj.bias"] = w[p + "o_w"], w[p + "o_b"]
        sd[b + "layer_norm1.weight"], sd[b + "layer_norm1.bias"] = w[p + "ln1_w"], w[p + "ln1_b"]
        sd[b + "layer_norm2.weight"], sd[b + "layer_norm2.bias"] = w[p + "ln2_w"], w[p + "ln2_b"]
        for x in ("fc1", "fc2"):
            sd[b + f"mlp.{x}.weight"], sd[b + f"mlp.{x}.bias"] = w[p + x + "_w"], w[p + x + "_b"]
    return {prefix + k: v for k, v in sd.items()}


def bert_from_hf(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Canonical BERT weights from a `BertModel` state dict (`bert.` prefix tolerated; pooler ignored —
    the reference freezes it and IISAN never reads it, `Code_Uncached/run.py:83-100`)."""
    sd = _strip_prefix(sd, ("bert.",))
    w = {
        "word_emb": sd["embeddings.word_embeddings.weight"],
        "pos_emb": sd["embeddings.position_embeddings.weight"],
        "type_emb": sd["embeddings.token_type_embeddings.weight"],
        "emb_ln_w": sd["embeddings.LayerNorm.weight"],
        "emb_ln_b": sd["embeddings.LayerNorm.bias"],
    }
    l = 0
    while f"encoder.layer.{l}.attention.self.query.weight" in sd:
        b = f"encoder.layer.{l}."
        p = f"L{l}."
        w[p + "qkv_w"] = torch.cat([sd[b + f"attention.self.{x}.weight"] for x in ("query", "key", "value")], 0)
        w[p + "qkv_b"] = torch.cat([sd[b + f"attention.self.{x}.bias"] for x in ("query", "key", "value")], 0)
        w[p + "o_w"] = sd[b + "attention.output.dense.weight"]
        w[p + "o_b"] = sd[b + "attention.output.dense.bias"]
        w[p + "ln1_w"] = sd[b + "attention.output.LayerNorm.weight"]
        w[p + "ln1_b"] = sd[b + "attention.output.LayerNorm.bias"]
        w[p + "fc1_w"] = sd[b + "intermediate.dense.weight"]
        w[p + "fc1_b"] = sd[b + "intermediate.dense.bias"]
        w[p + "fc2_w"] = sd[b + "output.dense.weight"]
        w[p + "fc2_b"] = sd[b + "output.dense.bias"]
        w[p + "ln2_w"] = sd[b + "output.LayerNorm.weight"]
        w[p + "ln2_b"] = sd[b + "output.LayerNorm.bias"]
        l += 1
    return {k: v.detach().float().contiguous() for k, v in w.items()}


def vit_to_hf5(w: Dict[str, torch.Tensor], cfg: VitConfig) -> Dict[str, torch.Tensor]:
    """Canonical -> `ViTForImageClassification` state dict in the transformers-5.x layout (classifier excluded).
    Used only by the golden-fixture script to load generated weights into the imported reference."""
    D = cfg.hidden
    sd = {
        "vit.embeddings.cls_token": w["cls_token"].reshape(1, 1, D),
        "vit.embeddings.position_embeddings": w["pos_emb"].reshape(1, cfg.tokens, D),
        "vit.embeddings.patch_embeddings.projection.weight": w["patch_w"].reshape(D, cfg.channels, cfg.patch, cfg.patch),
        "vit.embeddings.patch_embeddings.projection.bias": w["patch_b"],
        "vit.layernorm.weight": w["lnf_w"],
        "vit.layernorm.bias": w["lnf_b"],
    }
    for l in range(cfg.layers):
        p, b = f"L{l}.", f"vit.layers.{l}."
        q, k, v = w[p + "qkv_w"].split(D, 0)
        qb, kb, vb = w[p + "qkv_b"].split(D, 0)
        sd[b + "attention.q_proj.weight"], sd[b + "attention.q_proj.bias"] = q, qb
        sd[b + "attention.k_proj.weight"], sd[b + "attention.k_proj.bias"] = k, kb
        sd[b + "attention.v_proj.weight"], sd[b + "attention.v_proj.bias"] = v, vb
        sd[b + "attention.o_proj.weight"], sd[b + "attention.o_proj.bias"] = w[p + "o_w"], w[p + "o_b"]
        sd[b + "layernorm_before.weight"], sd[b + "layernorm_before.bias"] = w[p + "ln1_w"], w[p + "ln1_b"]
        sd[b + "layernorm_after.weight"], sd[b + "layernorm_after.bias"] = w[p + "ln2_w"], w[p + "ln2_b"]
        sd[b + "mlp.fc1.weight"], sd[b + "mlp.fc1.bias"] = w[p + "fc1_w"], w[p + "fc1_b"]
        sd[b + "mlp.fc2.weight"], sd[b + "mlp.fc2.bias"] = w[p + "fc2_w"], w[p + "fc2_b"]
    return sd


def bert_to_hf(w: Dict[str, torch.Tensor], cfg: BertConfig) -> Dict[str, torch.Tensor]:
    """Canonical -> `BertModel` state dict (pooler excluded)."""
    D = cfg.hidden
    sd = {
        "embeddings.word_embeddings.weight": w["word_emb"],
        "embeddings.position_embeddings.weight": w["pos_emb"],
        "embeddings.token_type_embeddings.weight": w["type_emb"],
        "embeddings.LayerNorm.weight": w["emb_ln_w"],
        "embeddings.LayerNorm.bias": w["emb_ln_b"],
    }
    for l in range(cfg.layers):
        p, b = f"L{l}.", f"encoder.layer.{l}."
        q, k, v = w[p + "qkv_w"].split(D, 0)
        qb, kb, vb = w[p + "qkv_b"].split(D, 0)
        for n, (ww, bb) in dict(query=(q, qb), key=(k, kb), value=(v, vb)).items():
            sd[b + f"attention.self.{n}.weight"], sd[b + f"attention.self.{n}.bias"] = ww, bb
        sd[b + "attention.output.dense.weight"], sd[b + "attention.output.dense.bias"] = w[p + "o_w"], w[p + "o_b"]
        sd[b + "attention.output.LayerNorm.weight"], sd[b + "attention.output.LayerNorm.bias"] = w[p + "ln1_w"], w[p + "ln1_b"]
        sd[b + "intermediate.dense.weight"], sd[b + "intermediate.dense.bias"] = w[p + "fc1_w"], w[p + "fc1_b"]
        sd[b + "output.dense.weight"], sd[b + "output.dense.bias"] = w[p + "fc2_w"], w[p + "fc2_b"]
        sd[b + "output.LayerNorm.weight"], sd[b + "output.LayerNorm.bias"] = w[p + "ln2_w"], w[p + "ln2_b"]
    return sd


_DEBERTA_LAYER_KEYS = (("o_w", "attention.output.dense.weight"), ("o_b", "attention.output.dense.bias"),
                       ("ln1_w", "attention.output.LayerNorm.weight"), ("ln1_b", "attention.output.LayerNorm.bias"),
                       ("fc1_w", "intermediate.dense.weight"), ("fc1_b", "intermediate.dense.bias"),
                       ("fc2_w", "output.dense.weight"), ("fc2_b", "output.dense.bias"),
                       ("ln2_w", "output.LayerNorm.weight"), ("ln2_b", "output.LayerNorm.bias"))


def deberta_from_hf(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Canonical DeBERTa weights from a `DebertaV2Model` state dict (`deberta.` prefix tolerated): query_proj / key_proj / value_proj are
    stacked into qkv_w / qkv_b.  A checkpoint outside the supported configuration is named by the key that shows it."""
    sd = _strip_prefix(sd, ("deberta.",))
    for bad, why in (("embeddings.position_embeddings.weight", "position_biased_input"), ("encoder.conv.conv.weight", "conv_kernel_size > 0"),
                     ("embeddings.embed_proj.weight", "embedding_size != hidden_size"),
                     ("encoder.layer.0.attention.self.pos_key_proj.weight", "share_att_key = False")):
        if bad in sd:
            raise ValueError(f"deberta_from_hf: the state dict has {bad!r} ({why}): not a supported DeBERTa-v2/v3 configuration")
    for need in ("encoder.rel_embeddings.weight", "encoder.LayerNorm.weight"):
        if need not in sd:
            raise ValueError(f"deberta_from_hf: the state dict lacks {need!r} (relative_attention with norm_rel_ebd = layer_norm is required)")
    w = {
        "word_emb": sd["embeddings.word_embeddings.weight"],
        "emb_ln_w": sd["embeddings.LayerNorm.weight"],
        "emb_ln_b": sd["embeddings.LayerNorm.bias"],
        "rel_emb": sd["encoder.rel_embeddings.weight"],
        "rel_ln_w": sd["encoder.LayerNorm.weight"],
        "rel_ln_b": sd["encoder.LayerNorm.bias"],
    }
    l = 0
    while f"encoder.layer.{l}.attention.self.query_proj.weight" in sd:
        b, p = f"encoder.layer.{l}.", f"L{l}."
        w[p + "qkv_w"] = torch.cat([sd[b + f"attention.self.{x}_proj.weight"] for x in ("query", "key", "value")], 0)
        w[p + "qkv_b"] = torch.cat([sd[b + f"attention.self.{x}_proj.bias"] for x in ("query", "key", "value")], 0)
        for ours, theirs in _DEBERTA_LAYER_KEYS:
            w[p + ours] = sd[b + theirs]
        l += 1
    return {k: v.detach().float().contiguous() for k, v in w.items()}


def deberta_to_hf(w: Dict[str, torch.Tensor], cfg: DebertaConfig, prefix: str = "") -> Dict[str, torch.Tensor]:
    """Canonical -> `DebertaV2Model` state dict (prefix "deberta.": the key names of a task model's checkpoint)."""
    D = cfg.hidden
    sd = {
        "embeddings.word_embeddings.weight": w["word_emb"],
        "embeddings.LayerNorm.weight": w["emb_ln_w"],
        "embeddings.LayerNorm.bias": w["emb_ln_b"],
        "encoder.rel_embeddings.weight": w["rel_emb"],
        "encoder.LayerNorm.weight": w["rel_ln_w"],
        "encoder.LayerNorm.bias": w["rel_ln_b"],
    }
    for l in range(cfg.layers):
        p, b = f"L{l}.", f"encoder.layer.{l}."
        for n, ww, bb in zip(("query", "key", "value"), w[p + "qkv_w"].split(D, 0), w[p + "qkv_b"].split(D, 0)):
            sd[b + f"attention.self.{n}_proj.weight"], sd[b + f"attention.self.{n}_proj.bias"] = ww, bb
        for ours, theirs in _DEBERTA_LAYER_KEYS:
            sd[b + theirs] = w[p + ours]
    return {prefix + k: v for k, v in sd.items()}


def deberta_hf_config_kwargs(cfg: DebertaConfig) -> dict:
    """The `DebertaV2Config` arguments of the supported configuration at the shape of `cfg` (the golden generator and the tests build HF
    modules from it)."""
    return dict(vocab_size=cfg.vocab, hidden_size=cfg.hidden, num_hidden_layers=cfg.layers, num_attention_heads=cfg.heads,
                intermediate_size=cfg.mlp, max_position_embeddings=cfg.max_pos, layer_norm_eps=cfg.eps, type_vocab_size=0,
                relative_attention=True, position_buckets=cfg.position_buckets, max_relative_positions=-1, norm_rel_ebd="layer_norm",
                share_att_key=True, pos_att_type=["p2c", "c2p"], position_biased_input=False, hidden_act="gelu",
                hidden_dropout_prob=cfg.hidden_dropout, attention_probs_dropout_prob=cfg.attn_dropout, pad_token_id=0)


def config_dict(cfg) -> dict:
    return asdict(cfg)


# ----------------------------------------------------------------------------------------------------------------
# seeded trainable tensors (side network + SASRec + heads), keyed by the reference's state-dict names
# ----------------------------------------------------------------------------------------------------------------

def trainable_shapes(n_side: int = 7, dim_cv: int = 768, dim_text: int = 768, down: int = 64, emb: int = 64,
                     seq_len: int = 10, n_blocks: int = 2, cached: bool = False, modality: str = "intra_inter") -> Dict[str, tuple]:
    """Shapes of the 146 trainable tensors of IISAN mode in `named_parameters()` order-independent form
    (`Code_Uncached/model/model.py:166-205`, `modules.py:35-116`, `model.py:36-37`)."""
    ue = "user_encoder.transformer_encoder."
    s = {ue + "position_embedding.weight": (seq_len, emb),
         ue + "layer_norm.weight": (emb,), ue + "layer_norm.bias": (emb,)}
    for b in range(n_blocks):
        a = ue + f"transformer_blocks.{b}.multi_head_attention."
        f = ue + f"transformer_blocks.{b}.feed_forward."
        for n in ("w_Q", "w_K", "w_V", "fc"):
            s[a + n + ".weight"] = (emb, emb)
        s[a + "layer_norm.weight"] = (emb,)
        s[a + "layer_norm.bias"] = (emb,)
        s[f + "w_1.weight"] = (4 * emb, emb)
        s[f + "w_1.bias"] = (4 * emb,)
        s[f + "w_2.weight"] = (emb, 4 * emb)
        s[f + "w_2.bias"] = (emb,)
        s[f + "layer_norm.weight"] = (emb,)
        s[f + "layer_norm.bias"] = (emb,)
    s["com_dense.weight"] = (emb, 3 * emb if "intra_inter" in modality else emb)       # model.py:36-41 ("inter": the mm tower only)
    s["com_dense.bias"] = (emb,)
    m = "mm_encoder."
    cvh = m + ("cv_pre_fc." if cached else "cv_encoder.image_net.classifier.")
    txh = m + ("bert_pre_fc." if cached else "bert_encoder.text_encoders.title.fc.")
    s[cvh + "weight"], s[cvh + "bias"] = (emb, dim_cv), (emb,)
    s[txh + "weight"], s[txh + "bias"] = (emb, dim_text), (emb,)
    intra = "intra" in modality                     # model.py:178-205: the cv / text towers exist only with "intra"
    for tower, d in (("cv", dim_cv), ("bert", dim_text), ("mm", dim_text)):
        if tower != "mm" and not intra:
            continue
        for k in range(n_side):
            p = m + f"{tower}_adapter_list.{k}."
            s[p + "fc_down.weight"], s[p + "fc_down.bias"] = (down, d), (down,)
            s[p + "fc_up.weight"], s[p + "fc_up.bias"] = (d, down), (d,)
    if intra:
        s[m + "fc_bert.weight"], s[m + "fc_bert.bias"] = (dim_text, dim_text), (dim_text,)
        s[m + "fc_cv.weight"], s[m + "fc_cv.bias"] = (dim_cv, dim_cv), (dim_cv,)
    s[m + "fc_mm.weight"], s[m + "fc_mm.bias"] = (dim_text, dim_text), (dim_text,)
    s[m + "fc_mm_down.weight"], s[m + "fc_mm_down.bias"] = (emb, dim_text), (emb,)
    for g in ("text", "cv", "mm"):
        if g != "mm" and not intra:
            continue
        for k in range(n_side):
            s[m + f"side_gate_params_{g}.{k}"] = (1,)
    return s


def make_trainable_params(seed: int = 99, **shape_kw) -> Dict[str, torch.Tensor]:
    """Seeded, deliberately NON-default values for every trainable tensor (biases and gates away from zero,
    LayerNorm gains away from one, adapter weights at std 0.05 so the bottleneck path is not negligible):
    parity tests on these catch a dropped bias/gate that the reference initialisers (zeros) would hide.
    Product modules initialise like the reference (`modules.py:101-110`, `encoders.py:52-58`); this generator is
    for tests, fixtures and the benchmark only."""
    rs = np.random.RandomState(seed)
    out = {}
    for name, shape in trainable_shapes(**shape_kw).items():
        if "side_gate_params" in name:
            t = _normal(rs, shape, 0.08)
        elif name.endswith("layer_norm.weight"):
            t = 1.0 + _normal(rs, shape, 0.1)
        elif name.endswith("bias"):
            t = _normal(rs, shape, 0.05)
        elif "adapter_list" in name:
            t = _normal(rs, shape, 0.05)
        elif "position_embedding" in name:
            t = _normal(rs, shape, 0.2)
        else:
            fan_out, fan_in = shape[0], shape[-1]
            t = _normal(rs, shape, math.sqrt(2.0 / (fan_in + fan_out)))
        out[name] = t
    return out


def fill_params_seeded(named_shapes: Dict[str, tuple], seed: int) -> Dict[str, torch.Tensor]:
    """Seeded non-default values for an arbitrary set of named tensors (sorted by name), with the same value rules as
    `make_trainable_params`.  Used for the Versa fixtures, whose tensor set depends on the depth/width configuration."""
    rs = np.random.RandomState(seed)
    out = {}
    for name in sorted(named_shapes):
        shape = tuple(named_shapes[name])
        if "side_gate_params" in name:
            t = _normal(rs, shape, 0.08)
        elif name.endswith("layer_norm.weight"):
            t = 1.0 + _normal(rs, shape, 0.1)
        elif name.endswith("bias"):
            t = _normal(rs, shape, 0.05)
        elif "adapter_list" in name:
            t = _normal(rs, shape, 0.05)
        elif "position_embedding" in name:
            t = _normal(rs, shape, 0.2)
        else:
            t = _normal(rs, shape, math.sqrt(2.0 / (shape[0] + shape[-1])))
        out[name] = t
    return out
