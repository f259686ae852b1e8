"""Shared shapes and inputs of the ViT-H/14 tests (80-wide heads, 14-pixel patches, hidden 1280): the geometry of the HuggingFace golden
`tests/golden/vit_huge_geometry.npz` (tests/golden/make_golden_vit_huge.py), and the seeded weights / images both sides rebuild."""
import hashlib
import os

import numpy as np
import torch

from iisan_amd import weights

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vit_huge_geometry.npz")

# the golden geometry: every width of ViT-H/14 (1280 = 16 x 80, mlp 5120, patch 14) on a 56-pixel image (4 x 4 patches + CLS = 17 tokens), 2 layers
GEOM_VIT = weights.VitConfig(hidden=1280, layers=2, heads=16, mlp=5120, image=56, patch=14)
GEOM_SEED_W, GEOM_SEED_X, GEOM_ITEMS = 71, 72, 4


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def images(n: int, res: int, seed: int) -> torch.Tensor:
    """n seeded images in [-1, 1] (the normalised range), the first one all zero: the padding item the reference ships."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 3, res, res, generator=g).clamp_(-1.0, 1.0)
    x[0] = 0
    return x


def geometry_inputs():
    """(weights, images) of the golden: LayerNorm and bias vectors jittered (weights.make_vit_weights), 4 images, the first all zero."""
    return weights.make_vit_weights(GEOM_VIT, seed=GEOM_SEED_W), images(GEOM_ITEMS, GEOM_VIT.image, GEOM_SEED_X)


def load_golden():
    z = np.load(GOLDEN)
    vw, x = geometry_inputs()
    assert str(z["images_sha"]) == sha(x) and str(z["patch_w_sha"]) == sha(vw["patch_w"]), "the seeded inputs are not those of the golden"
    return z, vw, x
