"""The arithmetic of a DeBERTa-v2/v3 text tower restated in float64, and the seeded inputs of the HuggingFace golden
`tests/golden/deberta_v2.npz` (tests/golden/make_deberta_golden.py) that both sides rebuild.

Source: HF `transformers/models/deberta_v2/modeling_deberta_v2.py` in the configuration the v3 checkpoints carry (relative_attention,
share_att_key, pos_att_type = c2p|p2c, norm_rel_ebd = layer_norm, position_biased_input = False, type_vocab_size = 0):
  * `DebertaV2Embeddings.forward` (518-560): LayerNorm(word_emb[ids]) * mask — hidden state 0;
  * `DebertaV2Encoder.get_rel_embedding` (595-599): rel = LayerNorm(rel_embeddings.weight), once;
  * `DisentangledSelfAttention.forward` (191-274): scale = sqrt(64 * 3) (237-242), scores + `disentangled_attention_bias`, masked_fill with
    finfo.min under the query x key mask (257), a plain softmax (259);
  * `disentangled_attention_bias` (276-345): PK = key_proj(rel), PQ = query_proj(rel) (296-302); c2p gathers Q_i . PK at i - j + span (316-324),
    p2c gathers K_j . PQ at -(j - i) + span and transposes (327-343) — the same index i - j + span;
  * `build_relative_position` / `make_log_bucket_position` (57-102): the identity for |i - j| <= position_buckets / 2, the supported range;
  * the rest of the block is BERT's post-LN block (`DebertaV2Attention` 350-382, `DebertaV2Intermediate` / `DebertaV2Output` 385-414).
Mask convention: a key bias only (masked keys take fp32-min, so an all-masked row attends uniformly), as the kernels do.  HF's query x key
mask differs from it on the rows of padded tokens alone, and no tap of a real item depends on those."""
import hashlib
import os

import numpy as np
import torch
import torch.nn.functional as F

from iisan_amd import weights

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deberta_v2.npz")
VOCAB = 512


def _cfg(hidden, heads, layers, mlp, buckets):
    return weights.DebertaConfig(hidden=hidden, layers=layers, heads=heads, mlp=mlp, vocab=VOCAB, position_buckets=buckets)


# name: (config, words, weight seed, text seed).  Every tower has 4 items: an all-masked padding item, a full-length one, one of 5 tokens,
# one of half length.
TOWERS = {
    "b30": (_cfg(768, 12, 2, 512, 256), 30, 61, 62),         # base width at the reference's title length
    "x12": (_cfg(384, 6, 12, 1536, 256), 30, 63, 64),        # v3-xsmall's true depth: error growth over 12 layers
    "n8": (_cfg(128, 2, 2, 256, 16), 8, 65, 66),             # words = span / 2; any hard-coded 256
    "l128": (_cfg(1024, 16, 2, 512, 256), 128, 67, 68),      # the longest supported title; every table row a head can reach
}
ITEMS = 4


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def texts(words: int, seed: int, vocab: int = VOCAB) -> torch.Tensor:
    """int64 [4, 2 W] (W ids then W mask values): item 0 the padding item (ids and mask zero), item 1 full length, item 2 of 5 tokens (or
    fewer, at W < 5), item 3 of half length; ids of padded positions are zero, as the reference's tokenizer call pads them."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, vocab, (ITEMS, words), generator=g)
    lens = [0, words, min(5, words), max(1, words // 2)]
    mask = torch.zeros(ITEMS, words, dtype=torch.int64)
    for m, n in enumerate(lens):
        mask[m, :n] = 1
    return torch.cat([ids * mask, mask], dim=1)


def tower_inputs(name: str):
    """(config, canonical weights, text) of one tower of the golden."""
    cfg, words, seed_w, seed_x = TOWERS[name]
    return cfg, weights.make_deberta_weights(cfg, seed=seed_w), texts(words, seed_x, cfg.vocab)


def load_golden(name: str):
    """(config, weights, text, expected CLS rows [items, layers + 1, D] of HF's hidden states) — the seeded inputs checked against the
    checksums the generator stored."""
    z = np.load(GOLDEN)
    cfg, w, x = tower_inputs(name)
    assert str(z[name + "_text_sha"]) == sha(x) and str(z[name + "_w_sha"]) == sha(w["L1.fc2_w"]), "the seeded inputs are not those of the golden"
    return cfg, w, x, torch.from_numpy(z[name + "_taps"])


def rel_tables(w, cfg, l: int, dtype=torch.float64):
    """(PQ, PK) of layer l, each [heads, 2 span, 64]: query_proj / key_proj of the LayerNorm'd table, split into heads."""
    D = cfg.hidden
    rel = F.layer_norm(w["rel_emb"].to(dtype), (D,), w["rel_ln_w"].to(dtype), w["rel_ln_b"].to(dtype), cfg.eps)
    qkv_w, qkv_b = w[f"L{l}.qkv_w"].to(dtype), w[f"L{l}.qkv_b"].to(dtype)
    split = lambda t: t.view(-1, cfg.heads, 64).transpose(0, 1)
    return split(F.linear(rel, qkv_w[:D], qkv_b[:D])), split(F.linear(rel, qkv_w[D:2 * D], qkv_b[D:2 * D]))


def disentangled_attention(q, k, v, pq, pk, key_bias, span: int, c2p: bool = True, p2c: bool = True, flip: bool = False):
    """q, k, v [B, H, S, 64]; pq, pk [H, 2 span, 64]; key_bias [B, S] (< 0: masked) or None -> context [B, H, S, 64], in the dtype of q.
    c2p / p2c = False drop a positional term, flip = True indexes the tables at j - i + span: the negative controls of the GPU test."""
    S = q.shape[2]
    i = torch.arange(S).view(S, 1)
    j = torch.arange(S).view(1, S)
    d = ((j - i) if flip else (i - j)) + span                                # [S, S]
    s = q @ k.transpose(-1, -2)
    if c2p:
        s = s + torch.gather(q @ pk.transpose(-1, -2)[None], 3, d.expand(q.shape[0], q.shape[1], S, S))
    if p2c:     # K_j . PQ[d(i, j)]: [B, H, j, 2 span] gathered at d(i, j) for every i, then transposed
        s = s + torch.gather(k @ pq.transpose(-1, -2)[None], 3, d.t().expand(q.shape[0], q.shape[1], S, S)).transpose(-1, -2)
    s = s / (64 * 3) ** 0.5
    if key_bias is not None:
        s = s.masked_fill((key_bias < 0)[:, None, None, :], torch.finfo(torch.float32).min)
    return torch.softmax(s, dim=-1) @ v


def deberta_hidden_states(text: torch.Tensor, w, cfg, dtype=torch.float64):
    """All layers + 1 hidden states [B, W, D] of the tower in `dtype`."""
    w = {k: v.to(dtype) for k, v in w.items()}
    B, W = text.shape[0], text.shape[1] // 2
    D, H, span = cfg.hidden, cfg.heads, cfg.position_buckets
    assert W <= span // 2, "titles past position_buckets / 2 reach HF's log buckets"
    ids, mask = text[:, :W], text[:, W:]
    x = F.layer_norm(w["word_emb"][ids], (D,), w["emb_ln_w"], w["emb_ln_b"], cfg.eps) * mask[:, :, None].to(dtype)
    key_bias = torch.where(mask != 0, 0.0, -1.0)
    hs = [x]
    for l in range(cfg.layers):
        p = f"L{l}."
        pq, pk = rel_tables(w, cfg, l, dtype)
        qkv = F.linear(x, w[p + "qkv_w"], w[p + "qkv_b"]).view(B, W, 3, H, 64)
        q, k, v = (qkv[:, :, t].transpose(1, 2) for t in range(3))
        ctx = disentangled_attention(q, k, v, pq, pk, key_bias, span).transpose(1, 2).reshape(B, W, D)
        a = F.layer_norm(x + F.linear(ctx, w[p + "o_w"], w[p + "o_b"]), (D,), w[p + "ln1_w"], w[p + "ln1_b"], cfg.eps)
        f = F.linear(F.gelu(F.linear(a, w[p + "fc1_w"], w[p + "fc1_b"])), w[p + "fc2_w"], w[p + "fc2_b"])
        x = F.layer_norm(a + f, (D,), w[p + "ln2_w"], w[p + "ln2_b"], cfg.eps)
        hs.append(x)
    return hs


def deberta_cls_taps(text: torch.Tensor, w, cfg, dtype=torch.float64) -> torch.Tensor:
    """[B, layers + 1, D]: the CLS row of every hidden state."""
    return torch.stack([h[:, 0] for h in deberta_hidden_states(text, w, cfg, dtype)], dim=1)


def tap_errors(got: torch.Tensor, ref: torch.Tensor):
    """per tap layer: |got - ref| / |ref| in the 2-norm over the items — the measure of test_full_size_taps_match_reference_golden"""
    got, ref = got.double().cpu(), ref.double().cpu()
    return [float((got[:, l] - ref[:, l]).norm() / ref[:, l].norm()) for l in range(ref.shape[1])]
