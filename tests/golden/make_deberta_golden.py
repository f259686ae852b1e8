#!/usr/bin/env python3
"""Generates tests/golden/deberta_v2.npz: the per-layer CLS rows HuggingFace's own DeBERTa-v2 tower produces for seeded inputs.

Run on a CPU with `transformers` installed (`python tests/golden/make_deberta_golden.py`); no test imports `transformers` unguarded.  For
every tower of `tests/deberta_oracle.py: TOWERS` an HF `DebertaV2Model` is built from the config with eager attention, the weights of
`weights.make_deberta_weights(cfg, seed)` are loaded through the inverse key map `weights.deberta_to_hf`, and `hidden_states[l][:, 0]` of
all layers is stored in fp32 together with checksums of the seeded inputs (the inputs themselves are rebuilt from their seeds).  The
generator asserts on the way that the key map round-trips (with and without the `deberta.` prefix), that `hidden_states[0]` is the masked
LayerNorm of the word rows, and that the float64 restatement of `tests/deberta_oracle.py` agrees with HF to fp32 round-off on the CLS rows
of every slot and on every real-token row — and prints the numbers."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import deberta_oracle as DO                 # noqa: E402
from iisan_amd import weights               # noqa: E402

HF_TOL = 2e-5       # fp32 HF output against float64, relative per tap (the bound of tests/test_oracle_vs_golden.py)


def hf_tower(cfg, w):
    from transformers import DebertaV2Config, DebertaV2Model
    hc = DebertaV2Config(**weights.deberta_hf_config_kwargs(cfg))
    hc._attn_implementation = "eager"
    model = DebertaV2Model(hc).eval()
    missing, unexpected = model.load_state_dict(weights.deberta_to_hf(w, cfg), strict=False)
    assert not unexpected and not missing, (missing, unexpected)
    return model


def main():
    out = {}
    for name, (_, words, _, _) in DO.TOWERS.items():
        cfg, w, text = DO.tower_inputs(name)
        model = hf_tower(cfg, w)
        # the key map round-trips, with and without the `deberta.` prefix
        for sd in (model.state_dict(), weights.deberta_to_hf(w, cfg, "deberta."), weights.deberta_to_hf(w, cfg)):
            back = weights.deberta_from_hf(sd)
            assert set(back) == set(w) and all(torch.equal(back[k], w[k]) for k in back), name
        ids, mask = text[:, :words], text[:, words:]
        with torch.no_grad():
            hs = model(input_ids=ids, attention_mask=mask, output_hidden_states=True).hidden_states
        assert len(hs) == cfg.layers + 1
        # hidden_states[0] is the masked LayerNorm of the word rows: no position and no type table
        emb = F.layer_norm(w["word_emb"][ids], (cfg.hidden,), w["emb_ln_w"], w["emb_ln_b"], cfg.eps) * mask[:, :, None].float()
        assert torch.allclose(hs[0], emb, rtol=0, atol=1e-6), name
        ref = DO.deberta_hidden_states(text, w, cfg)
        taps = torch.stack([h[:, 0] for h in hs], 1).float()
        errs = DO.tap_errors(taps, torch.stack([h[:, 0] for h in ref], 1))
        real = mask.bool()
        row_errs = [float((hs[l][real].double() - ref[l][real]).norm() / ref[l][real].norm()) for l in range(cfg.layers + 1)]
        print(name, "HF fp32 vs float64 restatement, CLS rows of every slot:", " ".join(f"{e:.1e}" for e in errs))
        print(name, "                               every real-token row  :", " ".join(f"{e:.1e}" for e in row_errs))
        assert max(errs) <= HF_TOL and max(row_errs) <= HF_TOL, name
        out[name + "_taps"] = taps.numpy()
        out[name + "_text_sha"] = np.array(DO.sha(text))
        out[name + "_w_sha"] = np.array(DO.sha(w["L1.fc2_w"]))
    path = os.path.join(HERE, "deberta_v2.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
