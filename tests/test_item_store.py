"""CPU checks of the item store's host logic (`iisan_amd/itemstore.py`) and of the ctypes mirror of the two indexed encoder entries."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "iisan_hip.h")


def test_pack_unique_gives_sorted_distinct_ids_and_slot_positions():
    from iisan_amd.itemstore import pack_unique
    ids, index = pack_unique([[0, 0, 5, 3, 5], [0, 7, 3, 3, 9]])
    assert ids.dtype == np.int64 and index.dtype == np.int64
    assert ids.tolist() == [3, 5, 7, 9]
    assert index.tolist() == [-1, -1, 1, 0, 1, -1, 2, 0, 0, 3]


def test_pack_unique_of_an_all_padding_batch():
    from iisan_amd.itemstore import pack_unique
    ids, index = pack_unique(np.zeros((2, 3), dtype=np.int64))
    assert ids.shape == (0,) and index.tolist() == [-1] * 6


def test_pack_unique_without_a_padding_slot():
    from iisan_amd.itemstore import pack_unique
    ids, index = pack_unique([4, 2, 4])
    assert ids.tolist() == [2, 4] and index.tolist() == [1, 0, 1]


def test_pack_unique_capacity_is_a_hard_limit():
    from iisan_amd.itemstore import pack_unique
    batch = [0, 9, 2, 9, 5, 0, 7]                    # 4 distinct real items
    ids, _ = pack_unique(batch, capacity=4)
    assert ids.tolist() == [2, 5, 7, 9]
    with pytest.raises(ValueError):
        pack_unique(batch + [11], capacity=4)
    with pytest.raises(ValueError):
        pack_unique([3, -1])                         # a negative id is not a padding convention of the HOST side


def _header_args(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in include/iisan_hip.h"
    return m.group(1), [" ".join(a.split()) for a in m.group(2).split(",")]


def _ctype_of(decl):
    """ctypes type of one C parameter declaration of the header, as `_lib.SIGNATURES` spells it."""
    from iisan_amd import _lib
    if "iisan_vit_weights*" in decl:
        return C.POINTER(_lib.VitWeights)
    if "iisan_bert_weights*" in decl:
        return C.POINTER(_lib.BertWeights)
    if decl.startswith("const int32_t* tap_layers"):
        return C.POINTER(C.c_int32)              # the one host array
    if "*" in decl:
        return C.c_void_p
    return {"int64_t": C.c_int64, "int32_t": C.c_int32, "size_t": C.c_size_t}[decl.split()[0]]


@pytest.mark.parametrize("name", ["iisan_vit_forward_taps_u8_indexed", "iisan_bert_forward_taps_indexed"])
def test_lib_binds_the_indexed_entries_with_the_headers_argument_lists(name):
    from iisan_amd import _lib
    ret, args = _header_args(name)
    assert ret == "int"
    res, argtypes = _lib.SIGNATURES[name]
    assert res is C.c_int32
    assert argtypes == [_ctype_of(a) for a in args], (args, argtypes)
    fn = getattr(_lib.load(), name)              # exported by the built library, bound with these types
    assert fn.argtypes == argtypes


def test_indexed_entry_comments_cite_the_reference_dataset():
    src = open(HEADER).read()
    for name in ("iisan_vit_forward_taps_u8_indexed", "iisan_bert_forward_taps_indexed"):
        comment = src[:src.index("int " + name)].rsplit("/*", 1)[1]
        assert "dataset.py:56-86" in comment, name
