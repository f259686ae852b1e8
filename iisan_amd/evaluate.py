"""Batched evaluation and tap caching on the HIP path — the callers on either side of the hot path.

* `recommend_topk`  the recommendation list itself: the first k item ids of `metrics_topK`'s argsort per user
  (`metrics.py:59-60`), selected on the device from the same score tiles as the ranks (`iisan_score_topk`).
* `evaluate_ranks` / `hit_ndcg`  replace the per-user Python loop of `eval_model` + the full argsort of `metrics_topK`
  (`Code_Uncached/data_utils/metrics.py:59-67,157-246`): user vectors from SASRec, scores against the whole item table
  and the target's rank are computed on the device in two launches per user batch; users are sharded contiguously
  across ranks like `SequentialDistributedSampler` and gathered on ALL ranks (the reference's rank-0-only test eval would
  deadlock for world_size > 1).
* `item_table`  replaces `get_MM_item_embeddings` (`metrics.py:69-107`): items are sharded across ranks instead of being
  encoded redundantly by every rank.
* `build_tap_cache`  is what `Code_Cached/preprocess_vectors.py:68-112` does with HuggingFace models: the per-layer CLS
  taps `[N, L+1, D]` of a catalogue, from the same encoder kernels as the Uncached path; D is each tower's OWN hidden size
  (768: ViT-B / BERT-base; 1024: ViT-L / BERT-large — the widths `Code_Cached_Asym/preprocess_*.py` caches for Versa).
* `item_table_from_store` / `build_tap_cache_from_store`  the same two over an item store (`iisan_amd.itemstore`): id ranges
  through the indexed encoder entries, no image batch on the host or the device.
* `evaluate_ranks_from_store` / `recommend_topk_from_store` / `eval_metrics_from_store`  the eval routes over a user store
  (`iisan_amd.userstore`): windows, masks, targets and exclusion lists of a user batch are built on the device by user number.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np
import torch

from . import dp, ops, userstore
from .userstore import HIST_MAX, _ragged  # noqa: F401  (the rank route reads `evaluate.HIST_MAX` when called: tests set it here)


def _all_layers(enc, cv_device, text_device):
    """The tap lists "every hidden state" (the embeddings and each layer's output) of the image and the text tower."""
    text = enc.bert_encoder.text_encoders["title"]
    return range(enc.cv_encoder.packed(cv_device).cfg.layers + 1), range(text.packed(text_device).cfg.layers + 1)


@torch.no_grad()
def build_tap_cache(model, images: torch.Tensor, text: torch.Tensor, batch: int = 256) -> Tuple[torch.Tensor, torch.Tensor]:
    """CLS taps of every hidden state for a catalogue: ([N, Lc+1, Dc], [N, Lt+1, Dt]) fp32 on the inputs' device.  The widths are
    the towers' own hidden sizes (768 or 1024, or the narrow towers' 128, 192, 256, 384; the two towers may differ), not the side
    network's: a 24-layer ViT-L/16 gives the [N, 25, 1024] image taps of the Versa variant, `weights.VIT_TINY` / `weights.BERT_TINY` the
    [N, 13, 192] / [N, 3, 128] taps of its edge configuration (`Code_Cached_Asym/preprocess_edge_small.py`).  Always eval mode (no tower
    dropout)."""
    enc = model.mm_encoder
    cvs, txs = [], []
    for i in range(0, images.shape[0], batch):
        img, txt = images[i:i + batch].contiguous(), text[i:i + batch].contiguous()
        cv_layers, text_layers = _all_layers(enc, img.device, txt.device)
        cvs.append(enc.cv_encoder.forward_taps(img, cv_layers))
        txs.append(enc.bert_encoder.forward_taps(txt, text_layers))
    return torch.cat(cvs), torch.cat(txs)


def _shard_and_gather(model, N: int, rank: int, world: int, device, item3_of) -> torch.Tensor:
    """Rows 0..N-1 of the item table, each rank fusing the `item3_of(lo, hi)` blocks of its contiguous shard lo..hi-1, gathered on all."""
    per = (N + world - 1) // world
    lo, hi = min(rank * per, N), min((rank + 1) * per, N)
    rows = [model.fuse_item3(item3) for item3 in item3_of(lo, hi)]
    emb = model.com_dense.weight.shape[0]
    mine = torch.cat(rows) if rows else torch.empty(0, emb, device=device)
    if world == 1:
        return mine
    pad = torch.zeros(per, emb, device=mine.device)
    pad[:mine.shape[0]] = mine
    return dp.gather_concat(pad, per * world)[:N]


@torch.no_grad()
def item_table(model, images_or_taps: torch.Tensor, text_or_taps: torch.Tensor, batch: int = 512, rank: int = 0,
               world: int = 1) -> torch.Tensor:
    """Item embedding table `com_dense(cat(cv, text, mm))` (modality 'inter': `com_dense(mm)`) [N, emb] for items 0..N-1
    (row 0 = the padding item)."""
    def item3_of(lo, hi):
        for i in range(lo, hi, batch):
            j = min(i + batch, hi)
            yield model.mm_encoder.forward_item3(images_or_taps[i:j].contiguous(), text_or_taps[i:j].contiguous())[0]
    return _shard_and_gather(model, images_or_taps.shape[0], rank, world, images_or_taps.device, item3_of)


def _store_batches(model, store, lo: int, hi: int, batch: int):
    """(catalogue_u8, title table, index) of item ids lo..hi-1 in id ranges of `batch`, through `store.lookup`.  A streaming source
    (one with `submit`: `ItemFeed`) is sent each range right before it is looked up — nothing is copied ahead here, the catalogue pass
    is bound by the encoders — so its `capacity` AND its index buffers must cover `batch`: the index buffers are sized by
    `batch_slots` or, without it, by the FIRST batch the feed ever saw, so a feed that trained on smaller batches needs
    `batch_slots >= batch` at construction (`submit` raises otherwise)."""
    store = model.prepare_item_store(store)
    for i in range(lo, hi, batch):
        j = min(i + batch, hi)
        if hasattr(store, "submit"):
            store.submit(np.arange(i, j, dtype=np.int64))
        yield store.lookup(torch.arange(i, j, dtype=torch.int64, device=store.device))


@torch.no_grad()
def build_tap_cache_from_store(model, store, batch: int = 256) -> Tuple[torch.Tensor, torch.Tensor]:
    """`build_tap_cache` over the catalogue of an item store (`iisan_amd.itemstore`): the encoders read the store's rows by index,
    no image batch is materialised.  Row 0 = the padding item (zero image, zero title).  Widths as in `build_tap_cache`: each
    tower's own hidden size."""
    enc = model.mm_encoder
    cvs, txs = [], []
    for cat, txt, index in _store_batches(model, store, 0, store.rows, batch):
        cv_layers, text_layers = _all_layers(enc, index.device, index.device)
        cvs.append(enc.cv_encoder.forward_taps_indexed(cat, index, cv_layers))
        txs.append(enc.bert_encoder.forward_taps_indexed(txt, index, text_layers))
    if hasattr(store, "release"):
        store.release()
    return torch.cat(cvs), torch.cat(txs)


@torch.no_grad()
def item_table_from_store(model, store, batch: int = 512, rank: int = 0, world: int = 1) -> torch.Tensor:
    """`item_table` over the catalogue of an item store: [N+1, emb] for item ids 0..N (row 0 = the padding item), the same values
    as `item_table` on the materialised catalogue at the same `batch`."""
    def item3_of(lo, hi):
        for cat, txt, index in _store_batches(model, store, lo, hi, batch):
            yield model.mm_encoder.forward_item3_indexed(cat, txt, index)[0]
        if hasattr(store, "release"):
            store.release()
    return _shard_and_gather(model, store.rows, rank, world, store.device, item3_of)


def _pack_users(seqs: Sequence[Sequence[int]], histories: Sequence[Sequence[int]], max_seq_len: int, hist_stride: int):
    """Left-padded history tokens / masks (BuildMMEvalDataset, dataset.py:183-189), 0-padded exclusion lists, targets.
    Vectorised: the per-user Python loop of the first version (two tensor constructions per user) was 95 % of an eval pass
    at Scientific size (12,076 users: 200 ms around 8 ms of device work)."""
    U = len(seqs)
    flat, lens, ends = _ragged(seqs, U)
    if U and int(lens.min()) < 1:
        raise ValueError("evaluate_ranks: every eval sequence needs at least its target item")
    tgt = flat[ends - 1] if U else np.zeros(0, np.int64)
    hl = np.minimum(lens - 1, max_seq_len)                           # history positions that fit the window
    tok = np.zeros((U, max_seq_len), dtype=np.int64)
    lm = np.zeros((U, max_seq_len), dtype=np.float32)
    rows = np.repeat(np.arange(U), hl)
    k = np.arange(int(hl.sum())) - np.repeat(np.cumsum(hl) - hl, hl)  # 0 .. hl[u]-1 within each user
    col = max_seq_len - hl[rows] + k
    tok[rows, col] = flat[(ends - 1 - hl)[rows] + k]
    lm[rows, col] = 1.0
    hflat, hlens, hends = _ragged(histories, U)
    hist = np.zeros((U, hist_stride), dtype=np.int32)
    hrows = np.repeat(np.arange(U), hlens)
    hk = np.arange(int(hlens.sum())) - np.repeat(hends - hlens, hlens)
    hist[hrows, hk] = hflat
    return torch.from_numpy(tok), torch.from_numpy(lm), torch.from_numpy(hist), torch.from_numpy(tgt.astype(np.int32))


def _rank_long_history(prec_u: torch.Tensor, item_emb: torch.Tensor, history: Sequence[int], target: int) -> int:
    """Exact rank of ONE user whose exclusion list exceeds HIST_MAX entries, from launches of `iisan_score_rank` alone.
    With R(H) the kernel's rank under exclusion set H and T0 = {target} if the target is itself excluded (its score is then -inf in
    every pass, metrics.py:204-205) else {}:   R(H) = R(T0) + sum_i [R(H_i + T0) - R(T0)]   over disjoint chunks H_i of H - T0 —
    each excluded item changes the count by the same integer whichever pass it sits in, because the target's effective score and
    every item's score bits (csrc/score.hip: one MFMA chain per score) are the same in all passes."""
    dev = prec_u.device
    uniq = list(dict.fromkeys(int(c) for c in history if int(c) != 0))        # order kept, duplicates and padding dropped
    t0 = [target] if target in set(uniq) else []
    rest = [c for c in uniq if c != target]
    step = HIST_MAX - len(t0)
    chunks = [t0] + [rest[i:i + step] + t0 for i in range(0, len(rest), step)]
    hist = torch.zeros((len(chunks), HIST_MAX), dtype=torch.int32)
    for i, ch in enumerate(chunks):
        hist[i, :len(ch)] = torch.tensor(ch, dtype=torch.int32)
    r = ops.score_rank(prec_u.expand(len(chunks), -1).contiguous(), item_emb, hist.to(dev),
                       torch.full((len(chunks),), target, dtype=torch.int32, device=dev)).to(torch.int64).cpu()
    if bool((r < 1).any()):
        return -1                                      # invalid target: reported like the kernel does
    return int(r[0] + (r[1:] - r[0]).sum())


# A rank's share of the users, from host lists or from a `UserStore`.  Either source has `n_users`; `count`, the shard's length
# (`dp.sequential_shard`); `hs`, the width of the exclusion matrix; `batch(i, j, item_emb)` = (x = item_emb[tokens], mask, exclusion matrix,
# targets | None) of shard positions i..j-1, on the device; on the host `user(position)` and, per user number, `history(u)` (the FULL
# exclusion list) and `target(u)`; `long`, the (position, user) pairs whose list exceeds `cap`, the entries per user a batch may carry
# (None: any) — iisan_score_rank keeps them in LDS (include/iisan_hip.h: hist_stride <= 256).  Such users (the reference masks histories of
# any length, metrics.py:198-207) keep their first `cap` entries in the batched pass and are re-ranked exactly by `_rank_long_history`.

class _ListUsers:
    """Host lists: the shard is packed once by `_pack_users`, a batch is its slices shipped to the device.  `targets` False: `seqs` are the
    encoder's inputs alone (`recommend_topk`)."""

    def __init__(self, seqs, histories, max_seq_len, cap, rank, world, batch, targets=True):
        self.n_users, self.seqs, self.full = len(seqs), seqs, histories
        self.idx = dp.sequential_shard(self.n_users, rank, world, batch) if world > 1 else list(range(self.n_users))
        self.count = len(self.idx)
        long_users = {u for u in range(self.n_users) if len(histories[u]) > cap} if cap else set()
        if long_users:
            histories = list(histories)
            for u in long_users:
                histories[u] = histories[u][:cap]
        self.long = [(k, u) for k, u in enumerate(self.idx) if u in long_users] if long_users else []
        self.hs = max(1, max((len(h) for h in histories), default=1))
        rows = [seqs[i] for i in self.idx] if targets else [list(seqs[i]) + [0] for i in self.idx]
        self.tok, self.lm, self.hist, tgt = _pack_users(rows, [histories[i] for i in self.idx], max_seq_len, self.hs)
        self.tgt = tgt if targets else None

    def batch(self, i, j, item_emb):
        dev = item_emb.device
        x = item_emb[self.tok[i:j].to(dev)]                          # == com_dense(cat(tables[tokens])), metrics.py:214
        return x, self.lm[i:j].to(dev), self.hist[i:j].to(dev), None if self.tgt is None else self.tgt[i:j].to(dev)

    def user(self, pos):
        return self.idx[pos]

    def history(self, u):
        return self.full[u]

    def target(self, u):
        return int(self.seqs[u][-1])


class _StoreUsers:
    """A `userstore.UserStore`: a batch is a slice of the shard's user numbers (made on the device), its windows, masks, targets, exclusion
    matrix and `item_emb[tokens]` are built there; the host answers from the store's CSR copy."""

    def __init__(self, users, max_seq_len, mode, cap, rank, world, batch):
        self.users, self.n_users, self.S, self.mode = users, users.n_users, max_seq_len, mode
        self.hs = max(1, min(users.max_hist, cap) if cap else users.max_hist)
        self.idx = users.eval_index(rank, world, batch)
        self.first, self.count = userstore.shard_range(self.n_users, rank, world, batch)[0], self.idx.numel()
        # (the tail that repeats user U - 1 to fill the last batch is cut off by the gather and needs no correction)
        self.long = [(int(u) - self.first, int(u)) for u in users.long_users if self.first <= int(u) < self.first + self.count] if cap else []

    def batch(self, i, j, item_emb):
        ib = self.idx[i:j]
        _, m, tgt, x = self.users.windows(self.mode, self.S, ib, item_emb)
        return x, m, self.users.history(ib, self.hs), tgt

    def user(self, pos):
        return min(self.first + pos, self.n_users - 1)

    def history(self, u):
        return self.users.host.history(u).tolist()

    def target(self, u):
        return self.users.host.target(u)


def _rank_loop(model, item_emb, src, batch, world) -> torch.Tensor:
    """The gathered ranks of a user source, invalid targets (-1) still in them."""
    was_training = model.training
    model.eval()
    out = []
    try:
        for i in range(0, src.count, batch):
            x, m, hist, tgt = src.batch(i, i + batch, item_emb)
            prec = model.user_encoder(x, m, None)[:, -1].contiguous()   # metrics.py:216
            r = ops.score_rank(prec, item_emb, hist, tgt)
            for k, u in src.long:
                if i <= k < i + batch:
                    r[k - i] = _rank_long_history(prec[k - i:k - i + 1], item_emb, src.history(u), src.target(u))
            out.append(r)
    finally:
        model.train(was_training)
    ranks = torch.cat(out)
    return dp.gather_concat(ranks, src.n_users) if world > 1 else ranks


def _topk_loop(model, item_emb, src, k, batch, world) -> Tuple[torch.Tensor, torch.Tensor]:
    """The gathered top-k lists (ids, scores) of a user source."""
    was_training = model.training
    model.eval()
    ids_out, sc_out = [], []
    try:
        for i in range(0, src.count, batch):
            x, m, hist, _ = src.batch(i, i + batch, item_emb)
            prec = model.user_encoder(x, m, None)[:, -1].contiguous()   # metrics.py:214-216
            ids, sc = ops.score_topk(prec, item_emb, hist, k)
            ids_out.append(ids)
            sc_out.append(sc)
    finally:
        model.train(was_training)
    ids, sc = torch.cat(ids_out), torch.cat(sc_out)
    n_items = item_emb.shape[0] - 1
    if n_items - src.hs < k:
        ids = _fill_short_lists(ids, k, n_items, lambda row: src.history(src.user(row)))
    if world > 1:
        ids, sc = dp.gather_concat(ids, src.n_users), dp.gather_concat(sc, src.n_users)
    return ids, sc


def _fill_short_lists(ids: torch.Tensor, k: int, n_items: int, history_of_row) -> torch.Tensor:
    """Fewer than k items outside some user's history: the reference's argsort lists the -inf (history) items next — for a stable sort in
    ascending id order — and the kernel leaves those slots 0 (include/iisan_hip.h).  `history_of_row(r)`: the exclusion list of row r."""
    ids_c = ids.cpu()
    for r in torch.nonzero((ids_c == 0).any(dim=1)).flatten().tolist():
        excl = sorted({int(c) for c in history_of_row(r) if 1 <= int(c) <= n_items})
        free = int((ids_c[r] != 0).sum())
        fill = excl[:k - free]
        ids_c[r, free:free + len(fill)] = torch.tensor(fill, dtype=torch.int32)
    return ids_c.to(ids.device)


@torch.no_grad()
def evaluate_ranks(model, item_emb: torch.Tensor, eval_seqs: Sequence[Sequence[int]], histories: Sequence[Sequence[int]],
                   max_seq_len: int, batch: int = 1024, rank: int = 0, world: int = 1) -> torch.Tensor:
    """1-based rank of every user's target (int32 [U], identical on all ranks).  `eval_seqs[u]` = history + target
    (`eval_seq`), `histories[u]` = items to exclude (`user_history`, metrics.py:204-205)."""
    ranks = _rank_loop(model, item_emb, _ListUsers(eval_seqs, histories, max_seq_len, HIST_MAX, rank, world, batch), batch, world)
    if bool((ranks < 1).any()):
        _raise_invalid_targets(ranks, item_emb)
    return ranks


def _raise_invalid_targets(ranks: torch.Tensor, item_emb: torch.Tensor):
    """`iisan_score_rank` reports -1 for a target outside 1..item_num; the reference indexes the score row with it and raises
    IndexError (metrics.py:206) — so do the eval routes, after the gather, on every rank alike."""
    bad = torch.nonzero(ranks < 1).flatten()[:8].tolist()
    raise IndexError(f"evaluate_ranks: target item id outside 1..{item_emb.shape[0] - 1} for users {bad}")


@torch.no_grad()
def recommend_topk(model, item_emb: torch.Tensor, input_seqs: Sequence[Sequence[int]], histories: Sequence[Sequence[int]],
                   max_seq_len: int, k: int = 10, batch: int = 1024, rank: int = 0, world: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """Each user's recommendation list: (int32 ids [U, k], fp32 scores [U, k]), identical on all ranks — the first k entries of
    `order = torch.argsort(y_score, descending=True)` that `metrics_topK` (`metrics.py:59-60`) computes for the row `eval_model`
    builds at `metrics.py:198-206`, as item ids (position + 1).  `input_seqs[u]` = the items fed to the user encoder (the last
    `max_seq_len` are used, `dataset.py:183-189`; for the reference's eval protocol `eval_seq[u][:-1]`), `histories[u]` = the items
    scored -inf.  Ties towards the lower item id (a stable argsort).  Consistent with `evaluate_ranks`: a target it ranks r <= k is
    `ids[u, r-1]`.  The [U, N] score matrix never exists (`iisan_score_topk`)."""
    return _topk_loop(model, item_emb, _ListUsers(input_seqs, histories, max_seq_len, None, rank, world, batch, targets=False), k, batch, world)


def _ranks_from_store(model, item_emb, users, max_seq_len, batch, rank, world) -> torch.Tensor:
    """The gathered ranks of `evaluate_ranks_from_store`, invalid targets (-1) still in them."""
    return _rank_loop(model, ops._f32c(item_emb), _StoreUsers(users, max_seq_len, userstore.EVAL, HIST_MAX, rank, world, batch), batch, world)


@torch.no_grad()
def evaluate_ranks_from_store(model, item_emb: torch.Tensor, users, max_seq_len: int, batch: int = 1024, rank: int = 0,
                              world: int = 1) -> torch.Tensor:
    """`evaluate_ranks` over a `userstore.UserStore` built from (`eval_seq`, `user_history`): the same kernels on the same values — bit-equal
    ranks — with the token windows, masks, targets, exclusion matrix and `item_emb[tokens]` of every user batch built on the device from
    the resident sequences.  The user shard is the `dp.sequential_shard` range made on the device; no per-user host work, no per-batch
    host-to-device copy (users with more than HIST_MAX excluded items are corrected as in `evaluate_ranks`)."""
    ranks = _ranks_from_store(model, item_emb, users, max_seq_len, batch, rank, world)
    if bool((ranks < 1).any()):
        _raise_invalid_targets(ranks, item_emb)
    return ranks


@torch.no_grad()
def eval_metrics_from_store(model, item_emb: torch.Tensor, users, max_seq_len: int, batch: int = 1024, rank: int = 0, world: int = 1,
                            topk: int = 10) -> Tuple[float, float]:
    """(Hit@k, nDCG@k) = `hit_ndcg(evaluate_ranks(...), topk)` without the rank vector leaving the device: `iisan_rank_histogram` counts the
    ranks 1..k, and k + 2 integers come back.  Hit@k = sum of counts[1..k] / U; nDCG@k = sum of counts[r] / log2(r + 1) / U in float64.
    An invalid target raises the IndexError of `evaluate_ranks`."""
    import math
    ranks = _ranks_from_store(model, item_emb, users, max_seq_len, batch, rank, world)
    counts = ops.rank_histogram(ranks, topk).cpu().tolist()
    if counts[0] > 0:
        _raise_invalid_targets(ranks, item_emb)
    U = users.n_users
    return sum(counts[1:topk + 1]) / U, sum(counts[r] / math.log2(r + 1) for r in range(1, topk + 1)) / U


@torch.no_grad()
def recommend_topk_from_store(model, item_emb: torch.Tensor, users, max_seq_len: int, k: int = 10, batch: int = 1024, rank: int = 0,
                              world: int = 1, holdout: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """`recommend_topk` over a `userstore.UserStore`: bit-equal ids and scores.  The store's sequences are the encoder's inputs (INPUT
    windows); with `holdout` the last item of every sequence is held out as in the reference's eval protocol (EVAL windows: a store built
    from `eval_seq` serves both this and `evaluate_ranks_from_store`).  The whole exclusion list of every user is applied
    (`iisan_score_topk` takes any stride), as `recommend_topk` does."""
    src = _StoreUsers(users, max_seq_len, userstore.EVAL if holdout else userstore.INPUT, None, rank, world, batch)
    return _topk_loop(model, ops._f32c(item_emb), src, k, batch, world)


def hit_ndcg(ranks: torch.Tensor, topk: int = 10) -> Tuple[float, float]:
    """Hit@k and nDCG@k as `metrics_topK` + `eval_concat` report them (metrics.py:50-67)."""
    r = ranks.to(torch.float64)
    ok = (r >= 1) & (r <= topk)              # a rank < 1 is the kernel's "invalid target" signal, never a hit
    hit = ok.to(torch.float64)
    ndcg = torch.where(ok, 1.0 / torch.log2(r.clamp(min=1.0) + 1.0), torch.zeros_like(r))
    return float(hit.mean()), float(ndcg.mean())


def print_metrics(x, Log_file, v_or_t):
    """The reference's result line (`metrics.py:35-36`): percentages with five decimals, tab separated."""
    Log_file.info(v_or_t + "_results   {}".format('\t'.join(["{:0.5f}".format(i * 100) for i in x])))


@torch.no_grad()
def eval_model(model, user_history, eval_seq, item_embeddings_image, item_embeddings_text, test_batch_size, args, item_num,
               Log_file, v_or_t, local_rank):
    """Same signature, log lines and return value (Hit@10) as the reference's `eval_model` (`metrics.py:157-246`),
    for the modalities the IISAN wrapper serves: `item_embeddings_text` is the pair `[text, inter]` that
    `get_MM_item_embeddings` returns; with `modality == "inter"` only `inter` is read (`metrics.py:175-178,192-199`).  `eval_seq` maps user index -> item sequence (last = target), `user_history[u]`
    the items whose scores are set to -inf.  Works with or without an initialised process group; with one, users are
    sharded like `SequentialDistributedSampler` and the ranks gathered on every rank."""
    if "inter" not in args.modality:
        raise NotImplementedError("eval_model: modality 'intra' is not served by the IISAN wrapper")
    m = model.module if hasattr(model, "module") else model
    text, inter = item_embeddings_text
    dev = torch.device("cuda", local_rank) if isinstance(local_rank, int) else torch.device(local_rank)
    topK = 10
    Log_file.info(v_or_t + "_methods   {}".format('\t'.join(['Hit{}'.format(topK), 'nDCG{}'.format(topK)])))
    m.eval()
    if args.modality == "inter":
        item3 = inter.to(dev).float().contiguous()                                      # metrics.py:175-178
    else:
        item3 = torch.cat([item_embeddings_image.to(dev), text.to(dev), inter.to(dev)], dim=1).float().contiguous()
    item_emb = ops.LinearFn.apply(item3, m.com_dense.weight, m.com_dense.bias)          # metrics.py:181
    users = range(len(eval_seq))
    seqs = [list(eval_seq[u]) for u in users]
    hists = [[int(i) for i in user_history[u]] for u in users]
    import torch.distributed as dist
    on = dist.is_available() and dist.is_initialized()
    rank, world = (dist.get_rank(), dist.get_world_size()) if on else (0, 1)
    ranks = evaluate_ranks(m, item_emb, seqs, hists, max_seq_len=args.max_seq_len, batch=test_batch_size, rank=rank, world=world)
    mean_eval = list(hit_ndcg(ranks, topK))
    print_metrics(mean_eval, Log_file, v_or_t)
    return mean_eval[0]
