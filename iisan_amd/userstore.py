"""User sequences resident on the device — the user half of the input pipeline (the item half: `iisan_amd.itemstore`, `iisan_amd.tapstore`).

The reference builds every user's left-padded window on the host, one `__getitem__` per user (`Code_Uncached/data_utils/dataset.py:65-92`
for training, `:183-189` for evaluation), and ships ids and masks per batch.  Here the sequences — and, for evaluation, the exclusion
lists `user_history` — are uploaded ONCE in CSR form (`off` int64 [U + 1], `items` int32 [nnz]); a batch is then an int64 index of user
numbers on the device, and `iisan_user_windows` / `iisan_user_history` build its windows, masks, targets, exclusion matrix and (for the
eval routes) the user encoder's input `item_emb[ids]` in one launch each.  `evaluate.evaluate_ranks_from_store`,
`evaluate.recommend_topk_from_store` and `evaluate.eval_metrics_from_store` run on it; `train_batch` + `epoch_index` replace the host
`Dataset` / `DistributedSampler` of a Cached or item-store epoch.

The host keeps the CSR arrays it was built from (numpy, a few bytes per interaction): the exclusion lists longer than
`HIST_MAX` are re-ranked from them (`evaluate._rank_long_history`), and so is the tail of a top-k list with fewer than k items
outside a user's history.
"""
from __future__ import annotations

import itertools
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib

__all__ = ["UserStore", "HostUsers", "pack_users", "epoch_index_host", "shard_range", "TRAIN", "EVAL", "INPUT"]

TRAIN, EVAL, INPUT = _lib.IISAN_WIN_TRAIN, _lib.IISAN_WIN_EVAL, _lib.IISAN_WIN_INPUT      # include/iisan_hip.h; 1 <= S <= 63
HIST_MAX = 256      # exclusion-list entries per user that iisan_score_rank takes in one launch (csrc/score.hip: MAXH)


def _ragged(rows, n):
    """(flat int64 array, lengths, end offsets) of a list of n integer sequences."""
    lens = np.fromiter((len(r) for r in rows), dtype=np.int64, count=n)
    flat = np.fromiter(itertools.chain.from_iterable(rows), dtype=np.int64, count=int(lens.sum()))
    return flat, lens, np.cumsum(lens)


@dataclass
class HostUsers:
    """The host half of a `UserStore` (plain numpy, no GPU).  `hist_*` are None without exclusion lists."""
    n_users: int
    seq_off: np.ndarray                 # int64 [U + 1]
    seq_items: np.ndarray               # int32 [nnz]
    hist_off: Optional[np.ndarray]
    hist_items: Optional[np.ndarray]
    min_len: int                        # shortest sequence (0 for an empty store)
    max_hist: int                       # longest exclusion list
    long_users: np.ndarray              # int64, ascending: users whose exclusion list exceeds HIST_MAX

    def sequence(self, u: int) -> np.ndarray:
        return self.seq_items[self.seq_off[u]:self.seq_off[u + 1]]

    def history(self, u: int) -> np.ndarray:
        """The FULL exclusion list of user u."""
        return self.hist_items[self.hist_off[u]:self.hist_off[u + 1]]

    def target(self, u: int) -> int:
        """The last item of user u's sequence (the eval target)."""
        return int(self.seq_items[self.seq_off[u + 1] - 1])


def _rows(x, what: str):
    """A list of sequences from a list / tuple or from a dict keyed 0..U-1 (the reference's `users_train`, `eval_seq`, `user_history`)."""
    if isinstance(x, dict):
        n = len(x)
        try:
            x = [x[u] for u in range(n)]
        except KeyError:
            raise ValueError(f"UserStore: {what} given as a dict must be keyed 0..{n - 1}") from None
    # (`user_history` holds LongTensors, preprocess.py:73-74)
    return [r.tolist() if isinstance(r, torch.Tensor) else r for r in x]


def _csr(rows, what: str, item_num: Optional[int]):
    n = len(rows)
    flat, lens, ends = _ragged(rows, n)
    if flat.size:
        if int(flat.min()) < 0:
            raise ValueError(f"UserStore: negative item id in {what}")
        top = int(flat.max())
        if item_num is not None and top > item_num:
            raise ValueError(f"UserStore: item id {top} in {what} above item_num = {item_num}")
        if top > np.iinfo(np.int32).max:
            raise ValueError(f"UserStore: item id {top} in {what} does not fit 32 bits")
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = ends
    return off, flat.astype(np.int32), lens


def pack_users(seqs, histories=None, item_num: Optional[int] = None) -> HostUsers:
    """CSR form of `seqs` (and `histories`) with the store's validation: ValueError for a negative id, for an id above `item_num` when it
    is given, and for `histories` that do not list every user."""
    rows = _rows(seqs, "seqs")
    off, items, lens = _csr(rows, "seqs", item_num)
    hoff = hitems = None
    max_hist, long_users = 0, np.zeros(0, dtype=np.int64)
    if histories is not None:
        hrows = _rows(histories, "histories")
        if len(hrows) != len(rows):
            raise ValueError(f"UserStore: {len(hrows)} histories for {len(rows)} sequences")
        hoff, hitems, hlens = _csr(hrows, "histories", item_num)
        max_hist = int(hlens.max()) if hlens.size else 0
        long_users = np.nonzero(hlens > HIST_MAX)[0].astype(np.int64)
    return HostUsers(len(rows), off, items, hoff, hitems, int(lens.min()) if lens.size else 0, max_hist, long_users)


def epoch_index_host(n: int, rank: int, world: int, epoch: int = 0, seed: int = 0, shuffle: bool = True) -> torch.Tensor:
    """`dp.shard_indices` as an int64 CPU tensor: the same CPU-generator permutation, wrap-around padding and `rank::world` stride."""
    if shuffle:
        g = torch.Generator()
        g.manual_seed(seed + epoch)
        idx = torch.randperm(n, generator=g)
    else:
        idx = torch.arange(n)
    total = math.ceil(n / world) * world
    pad = total - n
    if pad > 0:
        idx = torch.cat([idx, idx.repeat(math.ceil(pad / n))[:pad]])
    return idx[rank:total:world].contiguous()


def shard_range(n: int, rank: int, world: int, batch: int) -> Tuple[int, int]:
    """(first, count) of the contiguous eval shard of `dp.sequential_shard`: its entries are min(first + i, n - 1) for i < count.  One
    rank takes the n users as they are, without the padding to whole batches (what `evaluate_ranks` does for world = 1)."""
    if world == 1:
        return 0, n
    num = int(math.ceil(n / batch / world)) * batch
    return rank * num, num


class UserStore:
    """`seqs[u]`: the item ids of user u in time order — for the eval routes history + target (`eval_seq`), for `train_batch` the
    training sequence (`users_train`), for `recommend_topk_from_store` the encoder's inputs.  `histories[u]` (optional): the items
    scored -inf (`user_history`).  Lists / tuples, or dicts keyed 0..U-1 as the reference holds them.  ValueError for a negative id, an
    id above `item_num` (when given), a non-CUDA device; an EMPTY sequence is refused where it cannot be served — by EVAL windows
    (`windows(EVAL, ...)`, the eval routes), with the message of `evaluate_ranks`."""

    def __init__(self, seqs, histories=None, item_num: Optional[int] = None, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("UserStore: the store lives on a GPU; there is no CPU path")
        self.host = h = pack_users(seqs, histories, item_num)
        self.n_users, self.item_num = h.n_users, item_num
        self.max_hist, self.long_users = h.max_hist, h.long_users
        up = lambda a: torch.from_numpy(a).to(self.device)
        self.seq_off, self.seq_items = up(h.seq_off), up(h.seq_items)
        self.hist_off = self.hist_items = None
        if h.hist_off is not None:
            self.hist_off, self.hist_items = up(h.hist_off), up(h.hist_items)

    def nbytes(self) -> int:
        """Device bytes of the store."""
        ts = [self.seq_off, self.seq_items] + ([self.hist_off, self.hist_items] if self.hist_off is not None else [])
        return sum(t.numel() * t.element_size() for t in ts)

    def _index(self, index: torch.Tensor, what: str) -> torch.Tensor:
        if not isinstance(index, torch.Tensor) or not index.is_cuda or index.dtype != torch.int64 or index.dim() != 1:
            raise ValueError(f"UserStore.{what} needs a 1-d int64 index of user numbers on the store's device")
        return index.contiguous()

    def windows(self, mode: int, S: int, index: torch.Tensor, item_emb: Optional[torch.Tensor] = None):
        """(ids int64 [B, S + 1 | S], log_mask fp32 [B, S], target int32 [B] | None, x fp32 [B, S, E] | None) for the users `index`
        names (int64 [B] on the device; a value outside [0, U) gives an all-zero padding row): the TRAIN, EVAL or INPUT windows of
        `iisan_user_windows` (include/iisan_hip.h).  `target` exists in EVAL mode, `x = item_emb[ids]` with `item_emb` (fp32 [N + 1, E],
        EVAL / INPUT)."""
        if mode == EVAL and self.host.min_len < 1:
            raise ValueError("evaluate_ranks: every eval sequence needs at least its target item")
        lib = _lib.load()
        index = self._index(index, "windows")
        B, dev = index.numel(), self.device
        W = S + 1 if mode == TRAIN else S
        ids = torch.empty((B, max(W, 0)), dtype=torch.int64, device=dev)
        lm = torch.empty((B, max(S, 0)), dtype=torch.float32, device=dev)
        tgt = torch.empty(B, dtype=torch.int32, device=dev) if mode == EVAL else None
        x, E, n1 = None, 0, 0
        if item_emb is not None:
            if not item_emb.is_cuda or item_emb.dtype != torch.float32 or not item_emb.is_contiguous() or item_emb.dim() != 2:
                raise ValueError("UserStore.windows: item_emb must be a contiguous fp32 [N + 1, E] table on the device")
            n1, E = item_emb.shape
            x = torch.empty((B, max(S, 0), E), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.iisan_user_windows(self.seq_off.data_ptr(), self.seq_items.data_ptr(), self.n_users, index.data_ptr(), B, S,
                                              mode, ids.data_ptr(), lm.data_ptr(), tgt.data_ptr() if tgt is not None else None,
                                              item_emb.data_ptr() if item_emb is not None else None, n1, E,
                                              x.data_ptr() if x is not None else None, torch.cuda.current_stream().cuda_stream),
                       "iisan_user_windows")
        return ids, lm, tgt, x

    def history(self, index: torch.Tensor, stride: int) -> torch.Tensor:
        """int32 [B, stride]: the first `stride` entries of each named user's exclusion list, 0-padded (`iisan_user_history`)."""
        lib = _lib.load()
        if self.hist_off is None:
            raise ValueError("UserStore.history: the store was built without histories")
        index = self._index(index, "history")
        B = index.numel()
        out = torch.empty((B, max(stride, 0)), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(lib.iisan_user_history(self.hist_off.data_ptr(), self.hist_items.data_ptr(), self.n_users, index.data_ptr(), B,
                                              stride, out.data_ptr(), torch.cuda.current_stream().cuda_stream), "iisan_user_history")
        return out

    def train_batch(self, index: torch.Tensor, S: int):
        """(`sample_items_id` int64 [B, S + 1], `log_mask` fp32 [B, S]) of a training step, as `dataset.py:66-72` builds them."""
        ids, lm, _, _ = self.windows(TRAIN, S, index)
        return ids, lm

    def epoch_index(self, rank: int, world: int, epoch: int, seed: int = 0, shuffle: bool = True) -> torch.Tensor:
        """This rank's user numbers for one epoch on the device — `dp.shard_indices` (DistributedSampler semantics), one host-to-device
        copy per epoch.  Batches are slices of it."""
        return epoch_index_host(self.n_users, rank, world, epoch, seed, shuffle).to(self.device)

    def eval_index(self, rank: int, world: int, batch: int) -> torch.Tensor:
        """This rank's contiguous eval shard (`dp.sequential_shard`) as a device tensor, made on the device: no host list of U entries."""
        first, count = shard_range(self.n_users, rank, world, batch)
        return torch.arange(first, first + count, dtype=torch.int64, device=self.device).clamp_(max=self.n_users - 1)
