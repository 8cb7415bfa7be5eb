#!/usr/bin/env python3
"""Validation scoring cost on the GPU (docs/kernels.md, "score").

1. The scoring launch pair (score.hip: row kernel + reduce) against ``xent_fwd`` (row kernel + reduce)
   on the same buffer -- the BERT-base head's 640 x 30522 fp32 logits inside the 30720-wide padded
   buffer.  Both read the same bytes once.  The two are timed in alternating rounds in one process
   with device events around ``--iters`` back-to-back launches each.
2. One validation batch (``BertForPreTraining.score``, BERT-base, B x S) next to the forward of a
   training step (forward + backward timed with events in the same run, dropout on).

Prints one JSON line.  Needs a GPU: there is no CPU fallback.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us per call


def kernels(rows, V, iters, rounds):
    from hetseq_amd.ops import bert_ops
    from hetseq_amd.ops.score import mlm_nsp_score_, score_acc

    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(0)
    Vp = (V + 511) // 512 * 512
    buf = torch.zeros(rows, Vp, device=dev)
    buf[:, :V] = (torch.randn(rows, V, generator=g) * 2.0).to(dev)
    logits = buf[:, :V]
    labels = torch.randint(0, V, (rows,), generator=g).to(dev)
    nsp_logits = torch.randn(32, 2, generator=g).to(dev)
    nsp_labels = torch.randint(0, 2, (32,), generator=g).to(dev)
    acc = score_acc(dev)

    def score():
        mlm_nsp_score_(acc, logits, labels, nsp_logits, nsp_labels)

    def xent():
        bert_ops.xent_fwd(logits, labels)

    for fn in (score, xent):
        _timed(fn, 20)
    ts, tx = [], []
    for _ in range(rounds):
        ts.append(_timed(score, iters))
        tx.append(_timed(xent, iters))
    ts.sort()
    tx.sort()
    nbytes = rows * V * 4
    med_s, med_x = ts[len(ts) // 2], tx[len(tx) // 2]
    return {"rows": rows, "V": V, "ld": Vp, "score_us": round(med_s, 2), "xent_fwd_us": round(med_x, 2),
            "score_us_min_max": [round(ts[0], 2), round(ts[-1], 2)],
            "xent_fwd_us_min_max": [round(tx[0], 2), round(tx[-1], 2)], "ratio": round(med_s / med_x, 3),
            "score_GBps": round(nbytes / med_s / 1e3, 1), "xent_fwd_GBps": round(nbytes / med_x / 1e3, 1)}


def model(B, S, P, iters):
    from hetseq_amd.models.bert import BertConfig, BertForPreTraining
    from hetseq_amd.ops.score import score_acc
    from hetseq_amd.runtime import rng
    from hetseq_amd.runtime.flat import FlatParamStore

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    cfg = BertConfig(vocab_size_or_config_json_file=30522)
    m = BertForPreTraining(cfg).to(dev)
    store = FlatParamStore(m)
    m.attach_store(store, torch.float32)
    m.max_predictions_per_seq = m.max_predictions_per_seq_valid = P
    g = torch.Generator(device="cpu").manual_seed(1)
    ids = torch.randint(0, 30522, (B, S), generator=g).to(dev)
    tt = (torch.arange(S) > S // 2).long().expand(B, S).contiguous().to(dev)
    mask = torch.ones(B, S, dtype=torch.long, device=dev)
    labels = torch.full((B, S), -1, dtype=torch.long)
    for b in range(B):
        pos = torch.randperm(S - 2, generator=g)[:P] + 1
        labels[b, pos] = torch.randint(0, 30522, (P,), generator=g)
    nsp = torch.randint(0, 2, (B,), generator=g).to(dev)
    batch = (ids, tt, mask, labels.to(dev), nsp)
    acc = score_acc(dev)
    m.train()
    fwd, tot = [], []
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    for i in range(iters + 5):
        rng.set_seed(100 + i)
        store.zero_grad()
        ev[0].record()
        loss = m(*batch)
        ev[1].record()
        loss.backward()
        ev[2].record()
        ev[2].synchronize()
        if i >= 5:
            fwd.append(ev[0].elapsed_time(ev[1]))
            tot.append(ev[0].elapsed_time(ev[2]))
    m.eval()
    for _ in range(5):
        m.score(*batch, acc)
    torch.cuda.synchronize()
    val = _timed(lambda: m.score(*batch, acc), iters) / 1e3
    fwd.sort()
    tot.sort()
    return {"B": B, "S": S, "max_pred": P, "valid_batch_ms": round(val, 3),
            "train_forward_ms": round(fwd[len(fwd) // 2], 3), "train_fwd_bwd_ms": round(tot[len(tot) // 2], 3)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=640)
    ap.add_argument("--vocab", type=int, default=30522)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq", type=int, default=128)
    ap.add_argument("--max-pred", type=int, default=20)
    ap.add_argument("--no-model", action="store_true", help="the kernel comparison only")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_score.py needs a GPU")
    out = {"kernels": kernels(a.rows, a.vocab, a.iters, a.rounds)}
    if not a.no_model:
        out["model"] = model(a.batch, a.seq, a.max_pred, 20)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
