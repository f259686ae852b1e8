#!/usr/bin/env python3
"""Generates tests/golden/clip_vit.npz: the per-layer CLS rows HuggingFace's own CLIP vision tower produces for seeded inputs.

Run on a CPU with `transformers` installed (`python tests/golden/make_clip_golden.py`); no test imports `transformers`.  For every tower
of `tests/clip_oracle.py: TOWERS` an HF `CLIPVisionModel` is built from the config, the weights of `weights.make_vit_weights(cfg, seed)`
are loaded through the inverse key map `weights.clip_vit_to_hf`, and `hidden_states[l][:, 0]` of all layers is stored in fp32 together
with checksums of the seeded inputs (the inputs themselves are rebuilt from their seeds).  The generator confirms on the way that
`hidden_states[0]` IS the output of `pre_layrnorm`, that `clip_vit_from_hf` maps HF's state dict back to the canonical weights, and
that `post_layernorm` reaches no hidden state."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import clip_oracle as CO                    # noqa: E402
from iisan_amd import weights               # noqa: E402


def hf_tower(cfg, w):
    from transformers import CLIPVisionConfig, CLIPVisionModel
    hc = CLIPVisionConfig(hidden_size=cfg.hidden, intermediate_size=cfg.mlp, num_hidden_layers=cfg.layers, num_attention_heads=cfg.heads,
                          num_channels=cfg.channels, image_size=cfg.image, patch_size=cfg.patch, hidden_act=cfg.act,
                          layer_norm_eps=cfg.eps, attention_dropout=0.0)
    hc._attn_implementation = "eager"
    model = CLIPVisionModel(hc).eval()
    # (transformers 4.x nests the tower as `vision_model`, 5.x made CLIPVisionModel the tower itself: the keys lose the prefix)
    prefix = "vision_model." if hasattr(model, "vision_model") else ""
    missing, unexpected = model.load_state_dict(weights.clip_vit_to_hf(w, cfg, prefix), strict=False)
    assert not unexpected, unexpected
    assert all("post_layernorm" in k or "position_ids" in k for k in missing), missing
    return model


def main():
    out = {}
    for name in CO.TOWERS:
        cfg, w, x = CO.tower_inputs(name)
        model = hf_tower(cfg, w)
        # the key map round-trips, with and without the `vision_model.` prefix
        tower = getattr(model, "vision_model", model)
        for sd in (model.state_dict(), weights.clip_vit_to_hf(w, cfg, "vision_model."), weights.clip_vit_to_hf(w, cfg, "")):
            back = weights.clip_vit_from_hf(sd)
            assert set(back) == set(w) - {"lnf_w", "lnf_b"} and all(torch.equal(back[k], w[k]) for k in back), name
        with torch.no_grad():
            res = model(pixel_values=x, output_hidden_states=True)
            hs = res.hidden_states
            assert len(hs) == cfg.layers + 1
            # hidden_states[0] is the pre-LayerNorm's output, not the raw embeddings
            emb = tower.embeddings(x)
            pre = tower.pre_layrnorm(emb)
            assert torch.equal(hs[0], pre) and not torch.allclose(hs[0], emb), name
            # post_layernorm reaches the pooled output alone: the last hidden state is not normalised
            assert torch.allclose(res.pooler_output, tower.post_layernorm(hs[-1][:, 0]))
        taps = torch.stack([h[:, 0] for h in hs], 1).float()
        ref = CO.clip_cls_taps(x, w, cfg)
        print(name, "HF fp32 vs float64 restatement:", " ".join(f"{e:.1e}" for e in CO.tap_errors(taps, ref)))
        out[name + "_taps"] = taps.numpy()
        out[name + "_images_sha"] = np.array(CO.sha(x))
        out[name + "_w_sha"] = np.array(CO.sha(w["L1.fc2_w"]))
    path = os.path.join(HERE, "clip_vit.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
