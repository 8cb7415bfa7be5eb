"""Validation on the CPU: the torch scoring path, the driver's --validate flow (MNIST end to end, best
checkpoints), uneven two-rank validation over gloo, BERT set-level metrics, and the off-by-default rule."""
import json
import math
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env():
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env["CUDA_VISIBLE_DEVICES"] = ""
    env["HIP_VISIBLE_DEVICES"] = ""
    env["OMP_NUM_THREADS"] = "2"
    return env


def oracle_scores(logits, labels, nsp_logits, nsp_labels, k, ignore=-1):
    """Independent definition (python loops over rows, a stable descending sort, fp64 losses)."""
    out = [0.0] * 8
    V = logits.shape[1]
    for r in range(logits.shape[0]):
        lab = int(labels[r])
        if lab == ignore or lab < 0 or lab >= V:
            continue
        x = logits[r].double()
        order = torch.sort(x, descending=True, stable=True).indices.tolist()
        rank = order.index(lab)
        out[0] += float(torch.logsumexp(x, 0) - x[lab])
        out[1] += 1
        out[2] += rank == 0
        out[3] += rank < k
    for b in range(nsp_logits.shape[0]):
        out[7] += 1
        lab = int(nsp_labels[b])
        if lab not in (0, 1):
            continue
        y = nsp_logits[b].double()
        out[4] += float(torch.logsumexp(y, 0) - y[lab])
        out[5] += 1
        out[6] += int(torch.argmax(y)) == lab
    return out


def _close(a, b, rel=1e-6):
    return abs(a - b) <= rel * abs(b) + 1e-9


# ------------------------------------------------------------------ C1
def test_torch_scoring_matches_oracle_with_ties():
    from hetseq_amd.ops.score import metrics, mlm_nsp_score_, score_acc

    g = torch.Generator().manual_seed(0)
    R, V = 23, 37
    logits = torch.randn(R, V, generator=g)
    labels = torch.randint(0, V, (R,), generator=g)
    labels[::5] = -1
    labels[1], labels[2], labels[3] = 0, V - 1, V + 3  # first, last, out of range (ignored)
    # ties (integer-valued logits): the maximum at indices 4, 9, 20; the label on each of them in turn
    for i, lab in enumerate((4, 9, 20)):
        row = 6 + i
        logits[row] = torch.randint(-3, 3, (V,), generator=g).float()
        logits[row, [4, 9, 20]] = 7.0
        labels[row] = lab
    logits[11] = 2.0  # all equal: rank == label
    labels[11] = 13
    nsp_logits = torch.randn(6, 2, generator=g)
    nsp_logits[2] = torch.tensor([0.5, 0.5])  # tie: argmax is index 0
    nsp_labels = torch.tensor([0, 1, 0, -1, 1, 1])
    want = oracle_scores(logits, labels, nsp_logits, nsp_labels, 5)
    acc = score_acc("cpu")
    acc += 3.0
    mlm_nsp_score_(acc, logits, labels, nsp_logits, nsp_labels, k=5)
    mlm_nsp_score_(acc, logits, labels, nsp_logits, nsp_labels, k=5)
    got = acc.tolist()
    for j in (1, 2, 3, 5, 6, 7):
        assert got[j] == 3.0 + 2 * want[j], (j, got, want)
    for j in (0, 4):
        assert _close(got[j], 3.0 + 2 * want[j]), (j, got, want)
    # the constructed rows, one by one: ranks 0, 1, 2 and rank == label
    for row, top1, top2 in ((6, 1, 1), (7, 0, 1), (8, 0, 0)):
        a = score_acc("cpu")
        mlm_nsp_score_(a, logits[row:row + 1], labels[row:row + 1], nsp_logits[:0], nsp_labels[:0], k=2)
        assert a.tolist()[1:4] == [1.0, float(top1), float(top2)], (row, a)
    a = score_acc("cpu")
    mlm_nsp_score_(a, logits[11:12], labels[11:12], nsp_logits[:0], nsp_labels[:0], k=13)
    assert a.tolist()[1:4] == [1.0, 0.0, 0.0]
    a.zero_()
    mlm_nsp_score_(a, logits[11:12], labels[11:12], nsp_logits[:0], nsp_labels[:0], k=14)
    assert a.tolist()[1:4] == [1.0, 0.0, 1.0]
    # a batch with every label ignored changes nothing
    before = acc.clone()
    mlm_nsp_score_(acc, logits, torch.full((R,), -1), nsp_logits[:0], nsp_labels[:0])
    assert torch.equal(acc, before)
    m = metrics(want)
    assert _close(m["loss"], want[0] / want[1] + want[4] / want[5]) and _close(m["mlm_ppl"], math.exp(m["mlm_loss"]))
    assert m["mlm_acc"] == want[2] / want[1] and m["mlm_acc5"] == want[3] / want[1] and m["nsentences"] == 6


# ------------------------------------------------------------------ C2
def _valid_records(path):
    with open(path) as f:
        recs = [json.loads(line) for line in f]
    return [r for r in recs if "valid_loss" in r]


def test_mnist_validate_end_to_end(tmp_path):
    from hetseq_amd.checkpoint_utils import load_checkpoint_to_cpu
    from hetseq_amd.data.synthetic import write_mnist

    d = tmp_path / "mnist"
    write_mnist(str(d), n_train=128, n_test=50, seed=2)
    save, jl = str(tmp_path / "ck"), str(tmp_path / "log.jsonl")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--task", "mnist", "--optimizer", "adadelta",
                          "--lr", "1.0", "--data", str(d), "--max-sentences", "16", "--max-sentences-valid", "8",
                          "--valid-subset", "test", "--max-epoch", "2", "--cpu", "--distributed-world-size", "1",
                          "--save-dir", save, "--clip-norm", "0", "--log-format", "simple", "--log-interval", "100",
                          "--validate", "--json-log", jl],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=_env(), timeout=300)
    assert out.returncode == 0, out.stdout[-3000:]
    lines = re.findall(r"\| epoch (\d+) \| valid on 'test' subset \| loss ([0-9.e+-]+) \| accuracy ([0-9.e+-]+)",
                       out.stdout)
    assert [int(e) for e, _, _ in lines] == [1, 2], out.stdout[-3000:]
    recs = _valid_records(jl)
    assert len(recs) == 2
    losses = [r["valid_loss"] for r in recs]
    for (_, text, _), full in zip(lines, losses):
        assert abs(float(text) - full) <= 1e-5 * abs(full) + 1e-6
    assert os.path.exists(os.path.join(save, "checkpoint_best.pt"))
    st = load_checkpoint_to_cpu(os.path.join(save, "checkpoint_last.pt"))
    assert st["extra_state"]["best"] == min(losses)
    assert st["extra_state"]["val_loss"] == losses[1]
    best = load_checkpoint_to_cpu(os.path.join(save, "checkpoint_best.pt"))
    assert best["extra_state"]["val_loss"] == min(losses)
    ev = subprocess.run([sys.executable, os.path.join(ROOT, "eval_mnist.py"), "--model_ckpt",
                         os.path.join(save, "checkpoint_last.pt"), "--mnist_dir", str(d), "--cpu"],
                        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=_env(), timeout=300)
    assert ev.returncode == 0, ev.stdout[-3000:]
    m = re.search(r"Average loss: ([0-9.]+), Accuracy: (\d+)/(\d+)", ev.stdout)
    assert m, ev.stdout[-2000:]
    correct, total = int(m.group(2)), int(m.group(3))
    assert total == 50 and recs[1]["valid_nsentences"] == 50
    assert recs[1]["valid_accuracy"] == 100.0 * correct / total
    assert abs(float(m.group(1)) - losses[1]) <= 1e-4  # (the evaluator prints four decimals)


# ------------------------------------------------------------------ C3
def _mnist_cmd(data, save, jl, extra):
    return [sys.executable, os.path.join(ROOT, "train.py"), "--task", "mnist", "--optimizer", "adadelta", "--lr", "1.0",
            "--data", data, "--max-sentences", "16", "--valid-subset", "test", "--max-epoch", "1", "--cpu",
            "--distributed-backend", "gloo", "--save-dir", save, "--clip-norm", "0", "--log-format", "none",
            "--lr", "0.0", "--validate", "--json-log", jl, "--no-save", "--seed", "3"] + extra


@pytest.mark.slow
def test_two_gloo_ranks_uneven_validation_matches_one_rank(tmp_path):
    """130 validation samples in batches of 16: 9 batches, 5 on rank 0 and 4 on rank 1 (whose padded
    shard ends with an empty batch).  The learning rate is 0, so both launches score the same model."""
    from hetseq_amd.data.synthetic import write_mnist

    d = tmp_path / "mnist"
    write_mnist(str(d), n_train=64, n_test=130, seed=5)
    one = str(tmp_path / "one.jsonl")
    r = subprocess.run(_mnist_cmd(str(d), str(tmp_path / "c1"), one, ["--distributed-world-size", "1"]),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=_env(), timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    init = "file://" + str(tmp_path / "rdzv")
    logs = [str(tmp_path / ("two%d.jsonl" % i)) for i in range(2)]
    procs = [subprocess.Popen(_mnist_cmd(str(d), str(tmp_path / "c2"), logs[i],
                                         ["--distributed-init-method", init, "--distributed-world-size", "2",
                                          "--distributed-rank", str(i), "--distributed-gpus", "1", "--fast-stat-sync"]),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=_env())
             for i in range(2)]
    try:
        outs = [p.communicate(timeout=300)[0] for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    (a,), (b,) = _valid_records(one), _valid_records(logs[0])
    assert a["valid_nsentences"] == b["valid_nsentences"] == 130
    assert a["valid_accuracy"] == b["valid_accuracy"]
    assert _close(b["valid_loss"], a["valid_loss"])


# ------------------------------------------------------------------ C4
def _bert_setup(tmp_path, n_valid=22):
    from hetseq_amd.data.synthetic import write_bert_config, write_bert_shards, write_vocab

    d = tmp_path / "data"
    write_bert_shards(str(d), num_shards=1, per_shard=8, seq_len=16, max_pred=3, vocab_size=200, split="train")
    write_bert_shards(str(d), num_shards=1, per_shard=n_valid, seq_len=16, max_pred=3, vocab_size=200, seed=9,
                      split="valid")
    vocab = write_vocab(str(tmp_path / "v.txt"), 200)
    cfg = write_bert_config(str(tmp_path / "c.json"), vocab_size=200, hidden_size=64, num_hidden_layers=1,
                            num_attention_heads=2, intermediate_size=128)
    return str(d), cfg, vocab


def _bert_controller(tmp_path, d, cfg, vocab, extra):
    from hetseq_amd import options, tasks
    from hetseq_amd.controller import Controller

    args = options.parse_cli(["--task", "bert", "--data", d, "--dict", vocab, "--config_file", cfg, "--max-sentences",
                              "4", "--cpu", "--distributed-world-size", "1", "--save-dir", str(tmp_path / "ck"),
                              "--lr", "1e-3", "--log-format", "none", "--seed", "7", "--validate"] + extra)
    torch.manual_seed(args.seed)
    task = tasks.setup_task(args)
    task.load_dataset("valid")
    model = task.build_model(args)
    return Controller(args, task, model), task


def test_bert_validate_is_set_level(tmp_path):
    d, cfg, vocab = _bert_setup(tmp_path)
    got = {}
    for bs in ("4", "16"):
        ctl, task = _bert_controller(tmp_path, d, cfg, vocab, ["--max-sentences-valid", bs])
        ctl.get_model().train()
        got[bs] = ctl.validate("valid")
        assert ctl.get_model().training and ctl.get_num_updates() == 0
        assert ctl.get_meter("valid_loss").avg == got[bs]["loss"]
    # a direct loop over the same samples, one at a time, through the module graph and the oracle
    model, ds = ctl.get_model().eval(), task.dataset("valid")
    want = [0.0] * 8
    with torch.no_grad():
        for i in range(len(ds)):
            ids, seg, mask, lab, nsp = [t[None] for t in ds[i]]
            mlm, rel = model(ids, seg, mask)
            for j, v in enumerate(oracle_scores(mlm[0], lab[0], rel, nsp.reshape(1), 5)):
                want[j] += v
    m = task.valid_metrics(want)
    assert m["nsentences"] == 22
    for bs in ("4", "16"):
        for key in ("mlm_acc", "mlm_acc5", "nsp_acc", "nsentences"):
            assert got[bs][key] == m[key], (bs, key, got[bs], m)
        for key in ("loss", "mlm_loss", "nsp_loss", "mlm_ppl"):
            assert _close(got[bs][key], m[key]), (bs, key, got[bs], m)
    assert got["4"]["loss"] == pytest.approx(got["16"]["loss"], rel=1e-6)


# ------------------------------------------------------------------ C5
def _cli(tmp_path, name, extra, d, cfg, vocab, monkeypatch):
    from hetseq_amd import checkpoint_utils
    from hetseq_amd.controller import Controller
    from hetseq_amd.parallel import distributed_utils
    from hetseq_amd.train import cli_main

    calls = []
    real = Controller.validate
    monkeypatch.setattr(Controller, "validate", lambda self, subset: calls.append(subset) or real(self, subset))
    if hasattr(checkpoint_utils.save_checkpoint, "best"):
        del checkpoint_utils.save_checkpoint.best  # (process-global: start every run clean)
    save = tmp_path / name
    cli_main(["--task", "bert", "--data", d, "--dict", vocab, "--config_file", cfg, "--max-sentences", "4", "--cpu",
              "--distributed-world-size", "1", "--save-dir", str(save), "--lr", "1e-3", "--log-format", "none",
              "--seed", "7", "--max-epoch", "1"] + extra)
    distributed_utils.restore_output()
    if hasattr(checkpoint_utils.save_checkpoint, "best"):
        del checkpoint_utils.save_checkpoint.best
    return calls, save


def test_validation_is_off_by_default(tmp_path, monkeypatch):
    from hetseq_amd import options

    d, cfg, vocab = _bert_setup(tmp_path, n_valid=6)
    calls, save = _cli(tmp_path, "plain", [], d, cfg, vocab, monkeypatch)
    assert calls == [] and (save / "checkpoint_last.pt").exists() and not (save / "checkpoint_best.pt").exists()
    calls, save = _cli(tmp_path, "disabled", ["--validate", "--disable-validation"], d, cfg, vocab, monkeypatch)
    assert calls == [] and not (save / "checkpoint_best.pt").exists()
    calls, save = _cli(tmp_path, "on", ["--validate"], d, cfg, vocab, monkeypatch)
    assert calls == ["valid"] and (save / "checkpoint_best.pt").exists()
    calls, save = _cli(tmp_path, "upd", ["--validate-interval-updates", "1", "--validate-interval", "5"], d, cfg, vocab,
                       monkeypatch)
    assert calls == ["valid", "valid"]  # 8 training samples / 4: two updates, no end-of-epoch pass
    base = ["--task", "bert", "--config_file", cfg, "--max-sentences", "4"]
    a = options.parse_cli(base)
    assert a.validate is False and a.validate_interval_updates == 0 and not options.validation_enabled(a)
    a = options.parse_cli(base + ["--validate-interval-updates", "50"])
    assert a.validate_interval_updates == 50 and options.validation_enabled(a)
    assert not options.validation_enabled(options.parse_cli(base + ["--validate", "--disable-validation"]))
    with pytest.raises(SystemExit):
        options.parse_cli(base + ["--validate", "--hip-graph"])
    with open(os.path.join(ROOT, "docs", "parameters.md")) as f:
        text = f.read()
    assert "--validate-interval-updates" in text and re.search(r"--validate\b(?!-)", text)
