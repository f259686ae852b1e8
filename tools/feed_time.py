#!/usr/bin/env python
"""Step time of the Uncached path by where its item content comes from (profiles/r7_item_feed.md).

bs = 128 Scientific-shaped batches, every block on every token (what `bench.py` measures), fwd + bwd + Adam from the same trainer
state every step, `--warmup` + `--steps` steps per case, wall time between two device synchronisations:

  device    the batch tensors already on the device (what `bench.py` times; the same-process yardstick)
  store     (a) `ItemStore`: the whole uint8 catalogue resident, the encoders read it by item id
  feed      (b) `ItemFeed`: a FRESH host batch every step, submitted one step ahead (distinct real items, uint8, own copy stream)
  host_fp32 (c) the reference's way: fp32 [M,3,224,224] built on the host, copied synchronously before the step
            (`Code_Uncached/data_utils/dataset.py:56-86` + `run.py:404-407`); the host batch is built once, outside the timed
            region (the reference builds it in DataLoader workers) — the copy is what is timed

Prints one JSON line per case: ms/step, host-to-device bytes/step, GB/s.  For `feed` and `host_fp32` `h2d_GBps` is the copy alone,
measured on an otherwise idle device; `h2d_GBps_sustained` is bytes/step over the step time.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=128)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--items", type=int, default=None, help="catalogue size (default: Scientific, 20,314)")
    ap.add_argument("--cases", default="device,store,feed,host_fp32")
    a = ap.parse_args()
    from iisan_amd import factory, itemstore, synth, trainer, weights
    dev = torch.device("cuda:0")
    item_num = a.items or synth.SCI_ITEM_NUM
    R, W, S1 = 224, 30, 11
    M = a.bs * S1
    n_batches = a.steps + a.warmup

    # ---- host catalogue: raw uint8 images (drawn on the device in chunks, kept on the host) + the title table -----------------
    t0 = time.perf_counter()
    g = torch.Generator(device=dev).manual_seed(1)
    images = np.empty((item_num + 1, 3, R, R), dtype=np.uint8)
    for i in range(0, item_num + 1, 2048):
        j = min(i + 2048, item_num + 1)
        images[i:j] = torch.randint(0, 256, (j - i, 3, R, R), generator=g, device=dev, dtype=torch.uint8).cpu().numpy()
    text = synth.make_text(np.arange(item_num + 1), W, 30522, np.random.RandomState(0))
    rs = np.random.RandomState(12345)
    batches = [synth.make_ids(a.bs, 10, item_num, rs) for _ in range(n_batches + 1)]
    print(f"# catalogue {images.nbytes / 1e9:.2f} GB uint8 + {text.nbytes / 1e6:.1f} MB text, {n_batches + 1} batches: "
          f"{time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)

    torch.manual_seed(20260)
    args = factory.make_args()
    pop = synth.make_pop_prob(item_num)
    model = factory.build_model(args, item_num, pop, weights.make_vit_weights(), weights.VIT_BASE, weights.make_bert_weights(),
                                weights.BERT_BASE, cached=False, device=dev)
    enc = model.mm_encoder
    enc.cv_encoder.full_blocks = True
    enc.bert_encoder.text_encoders["title"].full_blocks = True
    model.train()
    tr = trainer.FlatTrainer(model, args, 1)
    flat0, rng0 = tr.flat.clone(), torch.get_rng_state()

    def step(ids, img, txt, lm):       # bench.py's step: every step is the same computation from the same state
        torch.set_rng_state(rng0)
        tr.flat.copy_(flat0)
        tr.m.zero_()
        tr.v.zero_()
        tr.step_no = 0
        return tr.step(ids, img, txt, lm)

    def timed(fn):
        for i in range(a.warmup):
            fn(i)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for i in range(a.warmup, n_batches):
            out = fn(i)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / a.steps * 1e3, float(out.detach())

    def report(case, ms, loss, nbytes, gbps=None, **kw):
        r = {"case": case, "ms_per_step": round(ms, 3), "h2d_bytes_per_step": int(nbytes), "loss_last": loss}
        if nbytes:
            r["h2d_GBps"] = None if gbps is None else round(gbps, 2)
            r["h2d_GBps_sustained"] = round(nbytes / ms / 1e6, 2)
        r.update(kw)
        print(json.dumps(r), flush=True)

    store = itemstore.ItemStore(images, text, dev)
    ids0 = torch.from_numpy(batches[0][0]).to(dev).view(-1)
    lm0 = torch.from_numpy(batches[0][1]).to(dev)
    cases = a.cases.split(",")
    real = int((ids0 != 0).sum())
    print(f"# batch 0: {M} slots, {real} real, {int(ids0.unique().numel()) - 1} distinct; store {store.nbytes() / 1e9:.2f} GB on the device",
          file=sys.stderr, flush=True)

    def materialise(ids):              # what the reference's dataset builds: normalised fp32, zeros on padding slots
        img = (store.images[ids].float().div_(255) - 0.5) / 0.5
        img[ids == 0] = 0
        txt = store.text[ids].clone()
        txt[ids == 0] = 0
        return img, txt

    if "device" in cases:
        img0, txt0 = materialise(ids0)
        ms, loss = timed(lambda i: step(ids0, img0, txt0, lm0))
        report("device", ms, loss, 0)
        del img0, txt0
    if "store" in cases:
        model.item_stores = store
        ms, loss = timed(lambda i: step(ids0, None, None, lm0))
        report("store", ms, loss, 0, store_bytes=store.nbytes())
        model.item_stores = None
    if "feed" in cases:
        feed = itemstore.ItemFeed(images, text, dev, slots=2, capacity=M, batch_slots=M)
        # the copy alone, device otherwise idle: host pack time (gather into the pinned slot) and copy rate
        pack, copy, nb = [], [], []
        for k in range(4):
            t = time.perf_counter()
            feed.submit(batches[k][0])
            t1 = time.perf_counter()
            feed.synchronize()
            t2 = time.perf_counter()
            feed.lookup(ids0)
            feed.release()
            pack.append(t1 - t)
            copy.append(t2 - t1)
            nb.append(feed.bytes_submitted)
        torch.cuda.synchronize()
        model.item_stores = feed
        dev_ids = [(torch.from_numpy(b[0]).view(-1), torch.from_numpy(b[1])) for b in batches]
        sent = []
        feed.submit(batches[0][0])

        def fstep(i):
            feed.submit(batches[i + 1][0])                    # the NEXT step's batch: packed and copied under this step
            sent.append(feed.bytes_submitted)
            ids, lm = dev_ids[i]
            return step(ids.to(dev, non_blocking=True), None, None, lm.to(dev, non_blocking=True))

        ms, loss = timed(fstep)
        feed.lookup(ids0)                                      # drain the batch submitted ahead of the last step
        feed.release()
        report("feed", ms, loss, float(np.mean(sent[a.warmup:])) + M * 12, gbps=float(np.median(nb)) / float(np.median(copy)) / 1e9,
               host_pack_ms=round(float(np.median(pack)) * 1e3, 2), copy_ms_idle=round(float(np.median(copy)) * 1e3, 2))
        model.item_stores = None
        feed.close()
        del feed
    if "host_fp32" in cases:
        img0, txt0 = materialise(ids0)
        h_img, h_txt, h_ids, h_lm = img0.cpu(), txt0.cpu(), ids0.cpu(), lm0.cpu()       # pageable, as a DataLoader hands them over
        del img0, txt0
        nbytes = h_img.numel() * 4 + h_txt.numel() * 8 + M * 12
        cp = []
        for _ in range(3):
            torch.cuda.synchronize()
            t = time.perf_counter()
            h_img.to(dev)
            torch.cuda.synchronize()
            cp.append(time.perf_counter() - t)
        ms, loss = timed(lambda i: step(h_ids.to(dev), h_img.to(dev), h_txt.to(dev), h_lm.to(dev)))        # run.py:404-407
        report("host_fp32", ms, loss, nbytes, gbps=h_img.numel() * 4 / float(np.median(cp)) / 1e9,
               copy_ms_idle=round(float(np.median(cp)) * 1e3, 2))


if __name__ == "__main__":
    main()
