"""Item content for the Uncached path, looked up on the device — the host half of the input pipeline.

The reference builds `[M,3,224,224]` fp32 on the host for every step (`Code_Uncached/data_utils/dataset.py:56-86`: one LMDB
read, decode and transform per slot, padding slots as zeros) and ships it synchronously: 848 MB per step at bs = 128.  Here the
encoders read item content by ROW INDEX inside their first kernel (`iisan_vit_forward_taps_u8_indexed`,
`iisan_bert_forward_taps_indexed`), so a step needs a raw uint8 catalogue on the device, a title table and one int64 index per
slot.  Two sources implement the same protocol

    lookup(sample_items_id) -> (catalogue_u8 [rows,3,R,R], text_table [rows,2W], index int64 [M])        all on the device

* `ItemStore`  the whole catalogue resident in HBM (Scientific: 20,315 x 150,528 B = 3.06 GB), index = item id.
* `ItemFeed`   the catalogue stays on the host; every step's DISTINCT real items (~80 MB of uint8 at bs = 128) are copied ahead of
               the step into one of `slots` device mini-stores, index = position in that mini-store.

A padding slot (item id 0) gets index -1 in both: the kernels never dereference an index outside `[0, rows)` and feed the tower
the all-zero normalised image / the all-zero title the reference ships for pad slots (`dataset.py:73,79-84`).  Row 0 of the
catalogue is therefore never read.  Set `ModelMM.item_stores` to either object.
"""
from __future__ import annotations

from collections import deque
from typing import Optional, Tuple

import numpy as np
import torch

__all__ = ["ItemStore", "ItemFeed", "pack_unique"]


def _host_array(x, dtype, what: str) -> np.ndarray:
    """numpy view (no copy for arrays, memmaps and CPU tensors of the right type) of a host catalogue."""
    if isinstance(x, torch.Tensor):
        if x.is_cuda:
            raise ValueError(f"{what}: expected a host array (numpy array, memmap or CPU tensor)")
        x = x.numpy()
    if not isinstance(x, np.ndarray):
        x = np.asarray(x)
    if x.dtype != dtype:
        raise ValueError(f"{what}: dtype {x.dtype}, expected {np.dtype(dtype)}")
    return x


def _check_catalogue(images: np.ndarray, text: np.ndarray):
    if images.ndim != 4 or images.shape[2] != images.shape[3]:
        raise ValueError(f"images_u8 must be [N+1, C, R, R], got {images.shape}")
    if text.ndim != 2 or text.shape[0] != images.shape[0]:
        raise ValueError(f"text must be [N+1, width] with one row per image, got {text.shape} for {images.shape[0]} images")


def pack_unique(ids, capacity: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """The distinct real items of a batch and each slot's position among them (plain numpy, no GPU).
    `ids`: item ids of any shape, 0 = padding.  Returns (`uniq`: the sorted distinct non-zero ids, int64 [U]; `index`: int64 of the
    shape of `ids.reshape(-1)`, the position of the slot's id in `uniq`, -1 for id 0).  ValueError when U > `capacity` (None: no
    limit) or an id is negative."""
    flat = np.asarray(ids, dtype=np.int64).reshape(-1)
    if flat.size and int(flat.min()) < 0:
        raise ValueError("pack_unique: negative item id")
    uniq, inverse = np.unique(flat, return_inverse=True)
    index = inverse.reshape(-1).astype(np.int64)
    if uniq.size and uniq[0] == 0:          # the padding id sorts first: drop it, shifting every position down (its own to -1)
        uniq = uniq[1:]
        index -= 1
    if capacity is not None and uniq.size > capacity:
        raise ValueError(f"pack_unique: {uniq.size} distinct items in the batch, the feed holds {capacity} per slot")
    return uniq, index


class ItemStore:
    """The raw catalogue resident on the device.  `images_u8` [N+1,3,R,R] uint8 (numpy array, memmap or CPU tensor; row i = item
    i after the offline Resize, row 0 = the padding item, never read), `text` [N+1, width] int64 (the `item_content` rows)."""

    def __init__(self, images_u8, text, device="cuda", chunk_bytes: int = 64 << 20):
        images = _host_array(images_u8, np.uint8, "ItemStore images_u8")
        txt = _host_array(text, np.int64, "ItemStore text")
        _check_catalogue(images, txt)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("ItemStore: the store lives on a GPU; there is no CPU path")
        self.rows = images.shape[0]
        row_bytes = int(np.prod(images.shape[1:]))
        per = max(1, int(chunk_bytes) // row_bytes)                    # rows per staged chunk
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream()
            copy = torch.cuda.Stream()
            self.images = torch.empty(images.shape, dtype=torch.uint8, device=self.device)
            self.text = torch.empty(txt.shape, dtype=torch.int64, device=self.device)
            copy.wait_stream(cur)               # the two allocations may reuse blocks with work pending on the current stream
            stage = torch.empty((min(per, self.rows),) + images.shape[1:], dtype=torch.uint8, pin_memory=True)
            stage_np = stage.numpy()
            done = torch.cuda.Event()
            with torch.cuda.stream(copy):
                for i in range(0, self.rows, per):
                    j = min(i + per, self.rows)
                    done.synchronize()          # ONE staging buffer: the host refills it only after the copy out of it has finished
                    np.copyto(stage_np[:j - i], images[i:j])
                    self.images[i:j].copy_(stage[:j - i], non_blocking=True)
                    done.record(copy)
                tpin = torch.from_numpy(np.ascontiguousarray(txt)).pin_memory()
                self.text.copy_(tpin, non_blocking=True)
                done.record(copy)
            # whatever runs on the current stream after the constructor sees the whole catalogue
            cur.wait_event(done)
            done.synchronize()                  # `stage` / `tpin` are released on return: their copies must have left them
        self.text_width = self.text.shape[1]
        self.text_columns = None                # (start, length) once narrowed; None = the whole `item_content` row

    def nbytes(self) -> int:
        return self.images.numel() + self.text.numel() * self.text.element_size()

    def narrow_text(self, start: int, length: int) -> None:
        """Keep only columns [start, start + length) of the text table (the title of a wider `item_content` row), as one contiguous
        table made ONCE here — never per step (`Bert_Encoder.title_columns`)."""
        if self.text_columns is not None:
            raise RuntimeError(f"ItemStore.narrow_text: the table already holds columns {self.text_columns} only")
        self.text = self.text[:, start:start + length].contiguous()
        self.text_width, self.text_columns = self.text.shape[1], (int(start), int(length))

    def lookup(self, sample_items_id: torch.Tensor):
        """ids int64 [...] on the device -> (catalogue, text table, index [M]): index = id, -1 for the padding id 0.  An id beyond the
        catalogue cannot be reported here without a synchronisation: to the kernels it is a padding slot (never dereferenced, zero
        content).  `ModelMM` therefore refuses, when the store is assigned, a catalogue with fewer rows than the model has items."""
        ids = sample_items_id.reshape(-1)
        if not ids.is_cuda or ids.dtype != torch.int64:
            raise ValueError("ItemStore.lookup needs int64 item ids on the store's device")
        return self.images, self.text, torch.where(ids == 0, -1, ids)


class ItemFeed:
    """Streaming feed for a catalogue that stays on the host.  `submit(ids)` — one step ahead — packs the batch's distinct real items
    into pinned slot k and enqueues their copy into device slot k on the feed's own copy stream; `lookup(ids)` hands the oldest
    submitted batch to the step.  `capacity`: distinct items a slot holds (default 1,408 = every slot of a bs = 128 batch).

    The two hazards of reusing a slot, and where each is closed:
      (1) pinned slot k is refilled by the host only after its previous copy to the device has finished — `submit` waits on the slot's
          "ready" event on the HOST before it writes the pinned buffers;
      (2) device slot k is overwritten only after the step that read it has finished — a "consumed" event is recorded on the consumer's
          stream once that step's work is enqueued (at the next `lookup`, at `release()`, or at the `submit` that takes the slot again,
          whichever comes first) and the COPY STREAM waits for it before the new copies.
    A slot handed out by `lookup` must have all work that reads it enqueued before the next `lookup` / `release` / reuse."""

    def __init__(self, images_u8, text, device="cuda", slots: int = 2, capacity: int = 1408, batch_slots: Optional[int] = None):
        self.host_images = _host_array(images_u8, np.uint8, "ItemFeed images_u8")
        self.host_text = _host_array(text, np.int64, "ItemFeed text")
        _check_catalogue(self.host_images, self.host_text)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("ItemFeed: the feed targets a GPU; there is no CPU path")
        if slots < 2 or capacity < 1:
            raise ValueError("ItemFeed: needs at least 2 slots (one being read, one being filled) and capacity >= 1")
        self.rows, self.slots, self.capacity = self.host_images.shape[0], int(slots), int(capacity)
        self.batch_slots = batch_slots
        self.text_width = self.host_text.shape[1]
        self.text_columns = None                             # (start, length) once narrowed; None = the whole `item_content` row
        with torch.cuda.device(self.device):
            self.copy_stream = torch.cuda.Stream()          # the one extra stream of the feed
            self._ready = [torch.cuda.Event() for _ in range(self.slots)]
            self._consumed = [torch.cuda.Event() for _ in range(self.slots)]
        self._state = ["free"] * self.slots                  # free | submitted | in_use (handed out by lookup) | consumed
        self._m = [0] * self.slots                           # index length of the batch in each slot
        self._consumer = [None] * self.slots                 # stream the slot was handed to
        self._pending = deque()
        self._next = 0
        self.bytes_submitted = 0                             # host-to-device bytes of the last submit (tools/feed_time.py)
        shape_i = (self.capacity,) + self.host_images.shape[1:]
        with torch.cuda.device(self.device):
            self._pin_img = [torch.empty(shape_i, dtype=torch.uint8, pin_memory=True) for _ in range(self.slots)]
            self._dev_img = [torch.empty(shape_i, dtype=torch.uint8, device=self.device) for _ in range(self.slots)]
        self._alloc_text()
        self._pin_idx = self._dev_idx = None
        if batch_slots is not None:
            self._alloc_index(int(batch_slots))

    # The device slots are allocated on the stream current at construction, written on the copy stream and read on the consumers'
    # streams.  They live as long as the feed, so no stream has to be told about them while it runs; `close()` (also run when the
    # feed is dropped) waits for the work still pending on them before the allocator may hand the blocks to anyone else.
    def _alloc_text(self):
        shape_t = (self.capacity, self.text_width)
        with torch.cuda.device(self.device):
            self._pin_txt = [torch.empty(shape_t, dtype=torch.int64, pin_memory=True) for _ in range(self.slots)]
            # stale rows beyond a batch's distinct items are never indexed; zeroed once so that the tables hold defined values
            self._dev_txt = [torch.zeros(shape_t, dtype=torch.int64, device=self.device) for _ in range(self.slots)]
            self.copy_stream.wait_stream(torch.cuda.current_stream())     # covers the image slots allocated just before as well

    def _alloc_index(self, m: int):
        self.batch_slots = m
        with torch.cuda.device(self.device):
            self._pin_idx = [torch.empty(m, dtype=torch.int64, pin_memory=True) for _ in range(self.slots)]
            self._dev_idx = [torch.full((m,), -1, dtype=torch.int64, device=self.device) for _ in range(self.slots)]
            self.copy_stream.wait_stream(torch.cuda.current_stream())

    def nbytes(self) -> int:
        """Device bytes of the mini-stores."""
        n = sum(t.numel() for t in self._dev_img) + sum(t.numel() * 8 for t in self._dev_txt)
        return n + (sum(t.numel() * 8 for t in self._dev_idx) if self._dev_idx else 0)

    def narrow_text(self, start: int, length: int) -> None:
        """Keep only columns [start, start + length) of the host text table (one contiguous copy, made once) — before the first
        `submit`.  Only the text slots are allocated again; the image slots stay."""
        if self.text_columns is not None:
            raise RuntimeError(f"ItemFeed.narrow_text: the table already holds columns {self.text_columns} only")
        if any(s != "free" for s in self._state):
            raise RuntimeError("ItemFeed.narrow_text: the feed has been used; narrow the table before the first submit")
        self.host_text = np.ascontiguousarray(self.host_text[:, start:start + length])
        self.text_width, self.text_columns = self.host_text.shape[1], (int(start), int(length))
        self._alloc_text()

    def close(self) -> None:
        """Host wait for every copy into, and every step that was handed, a slot of this feed.  Call it (or drop the feed: `__del__`
        does) before the slots' memory may be reused — the buffers were written and read on streams other than the one they were
        allocated on."""
        self.release()
        self.copy_stream.synchronize()
        for k in range(self.slots):
            if self._state[k] == "consumed":
                self._consumed[k].synchronize()

    def __del__(self):
        try:
            self.close()
        except Exception:       # interpreter teardown: the runtime may be gone already
            pass

    def pack_unique(self, ids):
        return pack_unique(ids, self.capacity)

    def _mark_consumed(self, k: int):
        """Hazard (2), first half: every kernel that reads device slot k is on its consumer's stream by now; mark the point."""
        self._consumed[k].record(self._consumer[k])
        self._state[k] = "consumed"

    def release(self) -> None:
        """The step that took the last `lookup` has been enqueued completely: its slot may be refilled."""
        for k in range(self.slots):
            if self._state[k] == "in_use":
                self._mark_consumed(k)

    def synchronize(self) -> None:
        """Host wait until every submitted copy has landed on the device (measurement and teardown; a step never needs it)."""
        for ev in self._ready:
            ev.synchronize()

    def submit(self, ids_cpu) -> None:
        """Pack and send the batch with item ids `ids_cpu` (host tensor / array, any shape, 0 = padding)."""
        if isinstance(ids_cpu, torch.Tensor):
            ids_cpu = ids_cpu.cpu().numpy()
        uniq, index = self.pack_unique(ids_cpu)
        if uniq.size and int(uniq[-1]) >= self.rows:
            raise ValueError(f"ItemFeed.submit: item id {int(uniq[-1])} outside the catalogue of {self.rows} rows")
        m, n = index.shape[0], uniq.shape[0]
        if self._pin_idx is None:
            self._alloc_index(m)
        if m > self.batch_slots:
            raise ValueError(f"ItemFeed.submit: a batch of {m} slots exceeds the index buffers ({self.batch_slots}); pass batch_slots")
        k = self._next
        if self._state[k] == "submitted":
            raise RuntimeError(f"ItemFeed.submit: all {self.slots} slots hold batches that no lookup has taken yet")
        if self._state[k] == "in_use":
            self._mark_consumed(k)
        # hazard (1): the previous copy out of pinned slot k must have finished before the host overwrites it
        self._ready[k].synchronize()
        np.take(self.host_images, uniq, axis=0, out=self._pin_img[k].numpy()[:n], mode="clip")      # bounds checked above
        np.take(self.host_text, uniq, axis=0, out=self._pin_txt[k].numpy()[:n], mode="clip")
        self._pin_idx[k].numpy()[:m] = index
        with torch.cuda.device(self.device), torch.cuda.stream(self.copy_stream):
            # hazard (2), second half: the copy stream overwrites device slot k only after the step that read it
            if self._state[k] == "consumed":
                self.copy_stream.wait_event(self._consumed[k])
            if n:
                self._dev_img[k][:n].copy_(self._pin_img[k][:n], non_blocking=True)
                self._dev_txt[k][:n].copy_(self._pin_txt[k][:n], non_blocking=True)
            self._dev_idx[k][:m].copy_(self._pin_idx[k][:m], non_blocking=True)
            self._ready[k].record(self.copy_stream)
        self.bytes_submitted = n * (self._pin_img[k][0].numel() + self.text_width * 8) + m * 8
        self._state[k], self._m[k] = "submitted", m
        self._pending.append(k)
        self._next = (k + 1) % self.slots

    def lookup(self, sample_items_id: torch.Tensor):
        """The oldest submitted batch: (device slot images [capacity,3,R,R], text [capacity, width], index [M]).  `sample_items_id`
        must be the ids that batch was submitted with (its shape is checked; the values cannot be without a synchronisation)."""
        if not self._pending:
            raise RuntimeError("ItemFeed.lookup: no submitted batch (call submit(ids) one step ahead)")
        k = self._pending[0]
        if sample_items_id.numel() != self._m[k]:
            raise ValueError(f"ItemFeed.lookup: the step has {sample_items_id.numel()} slots, the oldest submitted batch {self._m[k]}")
        self._pending.popleft()
        self.release()                                       # the previous step is enqueued: its slot is consumed
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(self._ready[k])
        self._state[k], self._consumer[k] = "in_use", cur
        return self._dev_img[k], self._dev_txt[k], self._dev_idx[k][:self._m[k]]
