#!/usr/bin/env python3
"""Generate tests/golden/vit_huge_geometry.npz from HuggingFace itself: `transformers.ViTModel` (eager attention, eval) at the widths of
`google/vit-huge-patch14-224-in21k` — hidden 1280, 16 heads of 80, mlp 5120, 14-pixel patches — on a 56-pixel image (17 tokens), 2 layers,
with the seeded weights of `iisan_amd.weights.make_vit_weights` (LayerNorm and bias vectors jittered) and 4 seeded images, the first all zero.
Stored: the inputs' seeds and checksums, and the CLS rows of the 3 hidden states [4, 3, 1280] — nothing else.  Needs `transformers`; the
tests only read the file.

Usage:  python tests/golden/make_golden_vit_huge.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import vit_huge_io as vio  # noqa: E402
from iisan_amd import weights  # noqa: E402


def main():
    from transformers import ViTConfig, ViTModel
    cfg = vio.GEOM_VIT
    vc = ViTConfig(hidden_size=cfg.hidden, num_hidden_layers=cfg.layers, num_attention_heads=cfg.heads, intermediate_size=cfg.mlp,
                   image_size=cfg.image, patch_size=cfg.patch, num_channels=cfg.channels, layer_norm_eps=cfg.eps, hidden_act="gelu",
                   hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, qkv_bias=True)
    vc._attn_implementation = "eager"
    vit = ViTModel(vc, add_pooling_layer=False)
    vw, images = vio.geometry_inputs()
    sd = {k[len("vit."):]: v for k, v in weights.vit_to_hf5(vw, cfg).items()}
    missing, unexpected = vit.load_state_dict(sd, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    vit.eval()
    torch.set_num_threads(8)
    with torch.no_grad():
        hs = vit(pixel_values=images, output_hidden_states=True).hidden_states
    assert len(hs) == cfg.layers + 1 and hs[0].shape == (vio.GEOM_ITEMS, cfg.tokens, cfg.hidden)
    taps = torch.stack([h[:, 0] for h in hs], 1).float().numpy()
    import transformers
    np.savez(vio.GOLDEN, taps=taps, seed_w=vio.GEOM_SEED_W, seed_x=vio.GEOM_SEED_X, images_sha=vio.sha(images),
             patch_w_sha=vio.sha(vw["patch_w"]), transformers=transformers.__version__)
    print(f"wrote {vio.GOLDEN}: taps {taps.shape}, transformers {transformers.__version__}")


if __name__ == "__main__":
    main()
