"""Frozen ViT / BERT encoders on the HIP path: weight packing + the two `*_forward_taps` calls.

Host-side counterpart of `Vit_Encoder` / `Bert_Encoder` (`Code_Uncached/model/encoders.py:23-31,116-159`) for the
IISAN mode, where only the per-layer CLS rows of the hidden states are consumed (`model.py:212-213`).  PyTorch is
used for device memory and the stream only; all arithmetic happens in libiisan_hip.so.
`PackedBert(w, cfg)` serves both text-tower families: a `weights.DebertaConfig` makes a `PackedDeberta` (the BERT executor with the
DeBERTa fields of `iisan_bert_weights` set; eval mode only).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Sequence

import torch

from . import _lib
from .weights import BertConfig, DebertaConfig, VitConfig

_TORCH16 = {_lib.IISAN_F16: torch.float16, _lib.IISAN_BF16: torch.bfloat16}
DTYPE_NAMES = {"fp16": _lib.IISAN_F16, "f16": _lib.IISAN_F16, "bf16": _lib.IISAN_BF16}


def _ptr(t: torch.Tensor) -> int:
    return t.data_ptr()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


class _Workspace:
    """Grow-only device scratch owned by the caller side of the ABI (the library never allocates)."""

    def __init__(self):
        self.buf = None

    def get(self, nbytes: int, device) -> torch.Tensor:
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != torch.device(device):
            self.buf = None
            self.buf = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        return self.buf


class _PackedEncoder:
    def __init__(self, w: Dict[str, torch.Tensor], device, dtype16: int):
        self.device = torch.device(device)
        self.dtype16 = dtype16
        self._keep = []
        self.ws = _Workspace()
        self._w = w

    # dead-work policy of the executor (include/iisan_hip.h): a field of the weights struct, i.e. part of every call
    @property
    def full_blocks(self) -> bool:
        return bool(self.struct.full_blocks)

    @full_blocks.setter
    def full_blocks(self, on: bool):
        self.struct.full_blocks = 1 if on else 0

    def _m16(self, name: str) -> int:      # matrix operand of an MFMA GEMM
        t = self._w[name].to(self.device, dtype=torch.float32).to(_TORCH16[self.dtype16]).contiguous()
        self._keep.append(t)
        return _ptr(t)

    def _v32(self, name: str) -> int:      # fp32 vector / table
        t = self._w[name].to(self.device, dtype=torch.float32).contiguous()
        self._keep.append(t)
        return _ptr(t)

    def _taps_call(self, name: str, head, M: int, tap_layers: Sequence[int], chunk_items: int, ws_bytes: int, device, extra=()):
        """One `*_forward_taps*` call: allocates the taps [M, len(tap_layers), D] and a workspace of ws_bytes, calls the entry point `name`
        with (weights, *head, tap array, n_taps, taps, chunk_items, *extra, workspace, its size, stream) and raises on a non-zero code."""
        taps = torch.empty((M, len(tap_layers), self.cfg.hidden), dtype=torch.float32, device=device)
        tl = (C.c_int32 * len(tap_layers))(*tap_layers)
        ws = self.ws.get(ws_bytes, device)
        _lib.check(getattr(_lib.load(), name)(C.byref(self.struct), *head, tl, len(tap_layers), _ptr(taps), chunk_items, *extra,
                                              _ptr(ws), ws.numel(), _stream()), name)
        return taps

    def _layers(self, struct, n_layers: int, masters: bool = False):
        """masters: also keep the fp32 originals of qkv_w / fc1_w on the device (`iisan_layer_weights.qkv_w32 / fc1_w32`): the ViT
        executor folds its LayerNorms into these two matrices and then rounds to fp16 once, not twice."""
        for l in range(n_layers):
            p, L = f"L{l}.", struct.layer[l]
            if masters:
                L.qkv_w32, L.fc1_w32 = self._v32(p + "qkv_w"), self._v32(p + "fc1_w")
            L.qkv_w, L.qkv_b = self._m16(p + "qkv_w"), self._v32(p + "qkv_b")
            L.o_w, L.o_b = self._m16(p + "o_w"), self._v32(p + "o_b")
            L.fc1_w, L.fc1_b = self._m16(p + "fc1_w"), self._v32(p + "fc1_b")
            L.fc2_w, L.fc2_b = self._m16(p + "fc2_w"), self._v32(p + "fc2_b")
            L.ln1_w, L.ln1_b = self._v32(p + "ln1_w"), self._v32(p + "ln1_b")
            L.ln2_w, L.ln2_b = self._v32(p + "ln2_w"), self._v32(p + "ln2_b")


class PackedVit(_PackedEncoder):
    """ViT weights resident in HBM in kernel layout (canonical names of `iisan_amd.weights`)."""

    def __init__(self, w: Dict[str, torch.Tensor], cfg: VitConfig, device="cuda", dtype16: int = _lib.IISAN_F16,
                 keep_masters: bool = False):
        """keep_masters: keep the fp32 originals of qkv_w / fc1_w resident after the one-time LayerNorm fold (tests that fold per call);
        by default they are released once `folded` is written — the executor only reads `folded` (~200 MB for ViT-B)."""
        super().__init__(w, device, dtype16)
        self.cfg = cfg
        s = _lib.VitWeights()
        s.hidden, s.layers, s.heads, s.mlp = cfg.hidden, cfg.layers, cfg.heads, cfg.mlp
        s.image, s.patch, s.channels, s.dtype16, s.eps = cfg.image, cfg.patch, cfg.channels, dtype16, cfg.eps
        if cfg.patch_ld != cfg.patch_dim:      # patch 14: rows zero-padded like the patch matrix (include/iisan_hip.h)
            self._w = dict(w, patch_w=torch.nn.functional.pad(w["patch_w"].float(), (0, cfg.patch_ld - cfg.patch_dim)))
        s.patch_w = self._m16("patch_w")
        # a CLIP vision tower (`VitConfig.pre_ln / act / patch_bias`): no patch bias, the pre-LayerNorm, quick-GELU — never guessed from the
        # dict: a config that asks for a tensor the weights lack, or weights with a tensor the config does not use, is an error
        if cfg.patch_bias != ("patch_b" in w) or cfg.pre_ln != ("pre_ln_w" in w):
            raise ValueError(f"PackedVit: the weights {'have' if 'patch_b' in w else 'lack'} patch_b and {'have' if 'pre_ln_w' in w else 'lack'} "
                             f"pre_ln_w, the config says patch_bias={cfg.patch_bias}, pre_ln={cfg.pre_ln}")
        s.patch_b = self._v32("patch_b") if cfg.patch_bias else None
        s.cls_token, s.pos_emb = self._v32("cls_token"), self._v32("pos_emb")
        if cfg.pre_ln:
            s.pre_ln_w, s.pre_ln_b = self._v32("pre_ln_w"), self._v32("pre_ln_b")
        s.act = {"gelu": 0, "quick_gelu": 1}[cfg.act]
        if cfg.norm_mean is not None:       # statistics of the uint8 entry points (all zero = the reference's (.5, .5))
            s.norm_mean, s.norm_std = (C.c_float * 3)(*cfg.norm_mean), (C.c_float * 3)(*cfg.norm_std)
        # LayerNorm 1 / 2 folded into the QKV / FC1 weights once, here, instead of at the start of every forward call — where the
        # executor has that route (fp16 operands, hidden 768; 0 bytes otherwise: a 1024-wide or a narrow tower keeps no fp32 masters)
        lib = _lib.load()
        nbytes = lib.iisan_vit_fold_bytes(C.byref(s))
        self._layers(s, cfg.layers, masters=nbytes > 0)
        self.struct = s
        self._w = None
        if nbytes and self.device.type == "cuda":
            self._folded = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
            with torch.cuda.device(self.device):
                _lib.check(lib.iisan_vit_fold_layernorm(C.byref(s), _ptr(self._folded), nbytes, _stream()), "iisan_vit_fold_layernorm")
            s.folded = _ptr(self._folded)
            # the fold ran on the stream current at construction; forwards may be issued on any other stream later: make the
            # folded set visible to all of them once, here (a one-time wait at pack time, never on the step)
            torch.cuda.current_stream(self.device).synchronize()
            if not keep_masters:
                masters = set()
                for l in range(cfg.layers):
                    L = s.layer[l]
                    masters.update((L.qkv_w32, L.fc1_w32))
                    L.qkv_w32 = L.fc1_w32 = None
                self._keep = [t for t in self._keep if _ptr(t) not in masters]

    def forward_taps(self, images: torch.Tensor, tap_layers: Sequence[int], chunk_items: int = 0) -> torch.Tensor:
        """images fp32 [M,C,R,R] (normalised) or uint8 [M,C,R,R] (raw pixels, normalised on the device) -> fp32
        [M, len(tap_layers), D] (`encoders.py:29-31` + `model.py:212`)."""
        lib = _lib.load()
        cfg = self.cfg
        assert images.is_cuda and images.dtype in (torch.float32, torch.uint8) and images.is_contiguous()
        assert images.shape[1:] == (cfg.channels, cfg.image, cfg.image), images.shape
        M = images.shape[0]
        nbytes = lib.iisan_vit_forward_taps_ws_bytes(C.byref(self.struct), M, chunk_items)
        return self._taps_call("iisan_vit_forward_taps_u8" if images.dtype == torch.uint8 else "iisan_vit_forward_taps", (_ptr(images), M),
                               M, tap_layers, chunk_items, nbytes, images.device)

    def forward_taps_indexed(self, catalogue_u8: torch.Tensor, index: torch.Tensor, tap_layers: Sequence[int],
                             chunk_items: int = 0) -> torch.Tensor:
        """catalogue uint8 [rows,C,R,R] resident on the device, index int64 [M] on the device -> fp32 [M, len(tap_layers), D]: slot m
        encodes row index[m]; a value outside [0, rows) is a padding slot (the zero normalised image, `dataset.py:73`).  No
        [M,C,R,R] tensor is built (`iisan_vit_forward_taps_u8_indexed`)."""
        lib = _lib.load()
        cfg = self.cfg
        assert catalogue_u8.is_cuda and catalogue_u8.dtype == torch.uint8 and catalogue_u8.is_contiguous()
        assert catalogue_u8.dim() == 4 and catalogue_u8.shape[1:] == (cfg.channels, cfg.image, cfg.image), catalogue_u8.shape
        assert index.is_cuda and index.device == catalogue_u8.device and index.dtype == torch.int64
        assert index.dim() == 1 and index.is_contiguous(), index.shape
        M = index.shape[0]
        nbytes = lib.iisan_vit_forward_taps_ws_bytes(C.byref(self.struct), M, chunk_items)
        return self._taps_call("iisan_vit_forward_taps_u8_indexed", (_ptr(catalogue_u8), catalogue_u8.shape[0], _ptr(index), M),
                               M, tap_layers, chunk_items, nbytes, index.device)


class PackedBert(_PackedEncoder):
    def __new__(cls, w=None, cfg=None, *args, **kw):
        # a DebertaConfig makes a PackedDeberta: `PackedBert(w, cfg)` serves both text-tower families
        if cls is PackedBert and isinstance(cfg, DebertaConfig):
            return super().__new__(PackedDeberta)
        return super().__new__(cls)

    def __init__(self, w: Dict[str, torch.Tensor], cfg: BertConfig, device="cuda", dtype16: int = _lib.IISAN_F16):
        super().__init__(w, device, dtype16)
        self.cfg = cfg
        s = _lib.BertWeights()
        s.hidden, s.layers, s.heads, s.mlp = cfg.hidden, cfg.layers, cfg.heads, cfg.mlp
        s.vocab, s.max_pos, s.dtype16, s.eps = cfg.vocab, cfg.max_pos, dtype16, cfg.eps
        self._tables(s)
        s.emb_ln_w, s.emb_ln_b = self._v32("emb_ln_w"), self._v32("emb_ln_b")
        self._layers(s, cfg.layers)
        self.struct = s
        self._w = None

    def _tables(self, s):
        s.word_emb, s.pos_emb, s.type_emb = self._v32("word_emb"), self._v32("pos_emb"), self._v32("type_emb")

    @staticmethod
    def _drop_struct(dropout):
        """`(hidden_p, attn_p, seed)` -> `iisan_bert_dropout` (sites and index formulas: include/iisan_hip.h)."""
        hidden_p, attn_p, seed = dropout
        return _lib.BertDropout(float(hidden_p), float(attn_p), int(seed))

    def forward_taps(self, text: torch.Tensor, tap_layers: Sequence[int], chunk_items: int = 0, dropout=None) -> torch.Tensor:
        """text int64 [M, 2W] -> fp32 [M, len(tap_layers), D] (`encoders.py:81-91` + `model.py:213`).
        dropout: None = eval mode; `(hidden_p, attn_p, seed)` = the tower as HF runs it under `train()`, one seed per call."""
        lib = _lib.load()
        assert text.is_cuda and text.dtype == torch.int64 and text.is_contiguous() and text.shape[1] % 2 == 0
        M, words = text.shape[0], text.shape[1] // 2
        nbytes = lib.iisan_bert_forward_taps_ws_bytes(C.byref(self.struct), M, words, chunk_items)
        if dropout is not None:
            return self._taps_call("iisan_bert_forward_taps_dropout", (_ptr(text), 0, None, M, words), M, tap_layers, chunk_items, nbytes,
                                   text.device, extra=(C.byref(self._drop_struct(dropout)),))
        return self._taps_call("iisan_bert_forward_taps", (_ptr(text), M, words), M, tap_layers, chunk_items, nbytes, text.device)

    def forward_taps_indexed(self, table: torch.Tensor, index: torch.Tensor, tap_layers: Sequence[int],
                             chunk_items: int = 0, dropout=None) -> torch.Tensor:
        """table int64 [rows, 2W] resident on the device, index int64 [M] on the device -> fp32 [M, len(tap_layers), D]: slot m
        encodes row index[m]; a value outside [0, rows) is a padding slot (all-zero ids and mask, `dataset.py:79-84`).
        dropout: as in `forward_taps`; the masks follow the SLOT m, not the table row."""
        lib = _lib.load()
        assert table.is_cuda and table.dtype == torch.int64 and table.is_contiguous()
        assert table.dim() == 2 and table.shape[1] % 2 == 0, table.shape
        assert index.is_cuda and index.device == table.device and index.dtype == torch.int64
        assert index.dim() == 1 and index.is_contiguous(), index.shape
        M, words = index.shape[0], table.shape[1] // 2
        nbytes = lib.iisan_bert_forward_taps_ws_bytes(C.byref(self.struct), M, words, chunk_items)
        head = (_ptr(table), table.shape[0], _ptr(index), M, words)
        if dropout is not None:
            return self._taps_call("iisan_bert_forward_taps_dropout", head, M, tap_layers, chunk_items, nbytes, index.device,
                                   extra=(C.byref(self._drop_struct(dropout)),))
        return self._taps_call("iisan_bert_forward_taps_indexed", head, M, tap_layers, chunk_items, nbytes, index.device)


class PackedDeberta(PackedBert):
    """A DeBERTa-v2/v3 text tower (`weights.DebertaConfig`; canonical names of `make_deberta_weights` / `deberta_from_hf`): the BERT executor
    with the trailing fields of `iisan_bert_weights` set.  The position tables are projected by every layer's query / key matrices ONCE here
    (`iisan_deberta_rel_project`), not at the start of every forward call.  Eval mode only: `dropout` must stay None."""

    def __init__(self, w: Dict[str, torch.Tensor], cfg: DebertaConfig, device="cuda", dtype16: int = _lib.IISAN_F16,
                 project_tables: bool = True):
        """project_tables = False leaves `rel_proj` null: every forward projects the tables into its workspace (tests; the same bits)."""
        for k in ("pos_emb", "type_emb"):
            if k in w:
                raise ValueError(f"PackedDeberta: the weights have {k!r}; a DeBERTa tower (position_biased_input = False, type_vocab_size = 0) has none")
        super().__init__(w, cfg, device, dtype16)
        if project_tables and self.device.type == "cuda":
            lib, s = _lib.load(), self.struct
            self._rel = torch.empty(int(lib.iisan_deberta_rel_bytes(C.byref(s))), dtype=torch.uint8, device=self.device)
            ws = torch.empty(int(lib.iisan_deberta_rel_ws_bytes(C.byref(s))), dtype=torch.uint8, device=self.device)
            with torch.cuda.device(self.device):
                _lib.check(lib.iisan_deberta_rel_project(C.byref(s), _ptr(self._rel), _ptr(ws), ws.numel(), _stream()), "iisan_deberta_rel_project")
                # forwards may be issued on any other stream later: make the tables visible to all of them once, at pack time
                torch.cuda.current_stream(self.device).synchronize()
            s.rel_proj = _ptr(self._rel)

    def _tables(self, s):
        s.word_emb = self._v32("word_emb")
        s.rel_emb, s.rel_ln_w, s.rel_ln_b = self._v32("rel_emb"), self._v32("rel_ln_w"), self._v32("rel_ln_b")
        s.span = self.cfg.position_buckets

    def _check(self, words: int, dropout):
        if dropout is not None and (dropout[0] > 0 or dropout[1] > 0):
            raise ValueError("PackedDeberta: the tower runs in eval mode only (no train-mode dropout)")
        if words > self.cfg.max_words:
            raise ValueError(f"PackedDeberta: titles of {words} words; at most position_buckets / 2 = {self.cfg.position_buckets // 2} "
                             "(and 128) are served")

    def forward_taps(self, text, tap_layers, chunk_items: int = 0, dropout=None):
        self._check(text.shape[1] // 2, dropout)
        return super().forward_taps(text, tap_layers, chunk_items, dropout)

    def forward_taps_indexed(self, table, index, tap_layers, chunk_items: int = 0, dropout=None):
        self._check(table.shape[1] // 2, dropout)
        return super().forward_taps_indexed(table, index, tap_layers, chunk_items, dropout)
