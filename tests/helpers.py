"""Shared builders for the tests (the implementations live in the package: `iisan_amd/factory.py`), and the host restatement of
the SASRec dropout masks the HIP path draws."""
import numpy as np
import torch

from iisan_amd.factory import build_model, load_trainables, make_args  # noqa: F401


def drop_factors(seed, site, n, p):
    """numpy re-implementation of drop_scale() in iisan_amd/csrc/common.h."""
    M64 = np.uint64(0xFFFFFFFFFFFFFFFF)
    idx = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = np.uint64(seed) + np.uint64(site) * np.uint64(0x9E3779B97F4A7C15) + idx * np.uint64(0xD1B54A32D192ED03)
        for _ in range(2):
            x ^= x >> np.uint64(32)
            x = (x * np.uint64(0xD6E8FEB86659FD93)) & M64
        x ^= x >> np.uint64(32)
    u = ((x >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(np.int64)
    thr = int(np.float32(p) * np.float32(16777216.0))
    return torch.from_numpy(np.where(u >= thr, np.float32(1.0) / (np.float32(1.0) - np.float32(p)), np.float32(0.0)).astype(np.float32))
