"""Validation on the GPU: the scoring kernels against an fp64 oracle, the fused model's score()
against the module graph, and a validation pass in the middle of training."""
import copy
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ACC0 = [0.5, 3.0, 2.0, 7.0, 1.25, 4.0, 1.0, 9.0]  # the accumulator's non-zero starting values


def _oracle(logits, V, labels, nsp_logits, nsp_labels, k, ignore=-1):
    """fp64 torch definition over the same fp32 values: (per-row rank, the eight sums)."""
    x = logits[:, :V].double()
    valid = (labels != ignore) & (labels >= 0) & (labels < V)
    lab = labels.clamp(0, V - 1)
    xl = x.gather(1, lab[:, None])
    col = torch.arange(V, device=x.device)[None, :]
    rank = ((x > xl).sum(1) + ((x == xl) & (col < lab[:, None])).sum(1)).to(torch.int32)
    rank = torch.where(valid, rank, torch.full_like(rank, -1))
    loss = torch.logsumexp(x, 1) - xl[:, 0]
    y = nsp_logits.double()
    ok = (nsp_labels == 0) | (nsp_labels == 1)
    nl = nsp_labels.clamp(0, 1)
    nloss = torch.logsumexp(y, 1) - y.gather(1, nl[:, None])[:, 0]
    sums = [loss[valid].sum().item(), valid.sum().item(), (valid & (rank == 0)).sum().item(),
            (valid & (rank < k)).sum().item(), nloss[ok].sum().item(), ok.sum().item(),
            (ok & (torch.argmax(y, 1) == nl)).sum().item(), float(y.shape[0])]
    return rank, loss.float() * valid, sums


def _rows(cuda, V, ld):
    """37 rows + 4 tie rows of [*, ld] fp32 logits whose pad columns hold +inf / NaN."""
    g = torch.Generator().manual_seed(V)
    R = 41
    buf = torch.empty(R, ld)
    buf[:, :V] = torch.randn(R, V, generator=g)
    buf[3:6, :V] += 40.0
    buf[6:9, :V] -= 40.0
    labels = torch.randint(0, V, (R,), generator=g)
    labels[::5] = -1
    labels[1], labels[2], labels[3] = 0, V - 1, V + 2  # first, last, out of range (ignored)
    expect = {}
    if V >= 3:
        tie = sorted({0, V // 2, V - 1})  # the maximum at three indices; the label on each in turn
        for i, lab in enumerate(tie):
            row = 37 + i
            buf[row, :V] = torch.randint(-4, 4, (V,), generator=g).float()
            buf[row, tie] = 9.0
            labels[row] = lab
            expect[row] = i
    else:
        buf[37, :V], labels[37], expect[37] = 1.0, 1, 1
        labels[38:40] = -1
    buf[40, :V] = -2.0  # all equal: rank == label
    labels[40] = V - 1
    expect[40] = V - 1
    if ld > V:
        buf[:, V:] = float("inf")
        buf[::2, V:] = float("nan")
    nsp_logits = torch.randn(7, 2, generator=g)
    nsp_logits[2] = torch.tensor([0.25, 0.25])  # a tie: the argmax is index 0
    nsp_labels = torch.tensor([0, 1, 0, -1, 1, 1, 0])
    return buf.to(cuda), labels.to(cuda), nsp_logits.to(cuda), nsp_labels.to(cuda), expect


# (2, 2): 64 threads, scalar; (1000, 1000): 64 threads; (1026, 1028): float4 + 2-element tail;
# (30522, 30720): the head's padded layout; (30522, 30522): rows not 16-B aligned -> scalar, 256 threads
@pytest.mark.parametrize("V,ld", [(2, 2), (1000, 1000), (1026, 1028), (30522, 30720), (30522, 30522)])
def test_score_kernel_matches_fp64_oracle(cuda, V, ld):
    from hetseq_amd.ops._C import hip, stream_handle
    from hetseq_amd.ops.score import mlm_nsp_score_

    buf, labels, nsp_logits, nsp_labels, expect = _rows(cuda, V, ld)
    logits = buf[:, :V]
    k = 5
    want_rank, want_loss, want = _oracle(buf, V, labels, nsp_logits, nsp_labels, k)
    for row, r in expect.items():
        assert int(want_rank[row]) == r, (row, r)  # (the oracle itself, on the constructed rows)
    # per-row outputs, through the raw binding
    R = logits.shape[0]
    row_loss = torch.full((R,), 123.0, device=cuda)
    rank = torch.full((R,), 77, dtype=torch.int32, device=cuda)
    acc = torch.tensor(ACC0, dtype=torch.float64, device=cuda)
    rc = hip().mlm_nsp_score(0, logits.data_ptr(), labels.data_ptr(), R, V, logits.stride(0), -1, k,
                             nsp_logits.data_ptr(), nsp_labels.data_ptr(), nsp_logits.shape[0], row_loss.data_ptr(),
                             rank.data_ptr(), acc.data_ptr(), stream_handle())
    assert rc == 0
    assert hip().mlm_nsp_score(1, logits.data_ptr(), labels.data_ptr(), R, V, logits.stride(0), -1, k,
                               nsp_logits.data_ptr(), nsp_labels.data_ptr(), nsp_logits.shape[0],
                               row_loss.data_ptr(), rank.data_ptr(), acc.data_ptr(), stream_handle()) == -1
    assert torch.equal(rank, want_rank), (rank.tolist(), want_rank.tolist())
    assert (row_loss[want_rank < 0] == 0).all()
    torch.testing.assert_close(row_loss, want_loss, rtol=1e-5, atol=1e-6)
    # the op: twice into a pre-filled accumulator
    mlm_nsp_score_(acc, logits, labels, nsp_logits, nsp_labels, k=k)
    got = acc.tolist()
    print("V=%d ld=%d acc %s oracle (x2 + start) %s" % (V, ld, got, [a + 2 * w for a, w in zip(ACC0, want)]))
    for j in (1, 2, 3, 5, 6, 7):
        assert got[j] == ACC0[j] + 2 * want[j], (j, got, want)
    for j in (0, 4):
        assert abs(got[j] - ACC0[j] - 2 * want[j]) <= 1e-5 * abs(2 * want[j]) + 1e-6, (j, got, want)
    # a batch whose labels are all ignored: unchanged and finite
    before = acc.clone()
    mlm_nsp_score_(acc, logits, torch.full_like(labels, -1), nsp_logits[:0], nsp_labels[:0], k=k)
    assert torch.equal(acc, before) and torch.isfinite(acc).all()


def _tiny(cuda, V=1000):
    from hetseq_amd.models.bert import BertConfig, BertForPreTraining

    cfg = BertConfig(vocab_size_or_config_json_file=V, hidden_size=256, num_hidden_layers=2, num_attention_heads=4,
                     intermediate_size=1024)
    return BertForPreTraining(cfg).to(cuda), cfg


def _inputs(cuda, B, S, V, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, V, (B, S), generator=g).to(cuda)
    tt = (torch.arange(S) > S // 2).long().expand(B, S).contiguous().to(cuda)
    mask = torch.ones(B, S, dtype=torch.long)
    mask[0, S - 9:] = 0  # one sequence with padded keys
    return ids, tt, mask.to(cuda)


def _unfused(ref, *inputs):
    os.environ["HETSEQ_DISABLE_FUSED"] = "1"
    try:
        with torch.no_grad():
            return ref(*inputs)
    finally:
        del os.environ["HETSEQ_DISABLE_FUSED"]


def _margin_labels(mlm, nsp, per_class=8, margin=0.01):
    """Labelled positions chosen so every decision has ``margin`` in the oracle's logits: top-1 hits
    (label = argmax, s0 - s1 > margin), top-5-only rows (label = the third entry, s0 - s2 and
    s2 - s5 > margin), misses (a label of rank >= 100); NSP rows with |l0 - l1| > margin."""
    B, S, V = mlm.shape
    flat = mlm.reshape(-1, V)
    srt, order = torch.sort(flat, dim=1, descending=True, stable=True)
    hit_ok = (srt[:, 0] - srt[:, 1]) > margin
    five_ok = ((srt[:, 0] - srt[:, 2]) > margin) & ((srt[:, 2] - srt[:, 5]) > margin)
    miss_ok = (srt[:, 4] - srt[:, 100]) > margin
    labels = torch.full((B * S,), -1, dtype=torch.long, device=mlm.device)
    counts = [0, 0, 0]
    for i in range(B * S):
        r = i * 37 % (B * S)  # (spread over the sequences: the sparse head has a per-sequence capacity)
        c = i % 3
        ok = (hit_ok, five_ok, miss_ok)[c][r]
        if counts[c] < per_class + 2 and bool(ok):
            labels[r] = order[r, (0, 2, 100 + r % 50)[c]]
            counts[c] += 1
    nsp_ok = (nsp[:, 0] - nsp[:, 1]).abs() > margin
    nsp_labels = torch.where(nsp_ok, torch.arange(B, device=nsp.device) % 2, torch.full((B,), -1, device=nsp.device))
    return labels.view(B, S), nsp_labels, counts, int(nsp_ok.sum())


@pytest.mark.parametrize("engine,dtype", [("default", "fp32"), ("x6", "fp32"), ("default", "bf16")])
def test_fused_score_matches_module_graph(cuda, engine, dtype):
    """Tolerances on the loss sums: those of the fused-vs-reference loss comparisons of
    test_bert_gpu.py -- the tiny model on the default engine 1e-4 rel + 1e-5, x6 1e-5 rel (its
    BERT-base comparison), bf16 5e-2 rel."""
    from hetseq_amd.ops import bert_ops
    from hetseq_amd.ops import gemm as G
    from hetseq_amd.ops.score import score_acc
    from hetseq_amd.runtime.flat import FlatParamStore

    if engine != "default":
        G.set_fp32_mode(engine)  # (conftest restores the default after the test)
    torch.manual_seed(0)
    model, cfg = _tiny(cuda)
    model.train()
    ref = copy.deepcopy(model).eval()
    ref._hs_disable_fused = True
    ref.bert._hs_disable_fused = True
    if dtype == "bf16":
        model.attach_store(FlatParamStore(model, shadow_dtype=torch.bfloat16), torch.bfloat16)
    B, S, V = 4, 64, cfg.vocab_size
    inputs = _inputs(cuda, B, S, V, seed=1)
    mlm, nsp = _unfused(ref, *inputs)
    labels, nsp_labels, counts, n_nsp = _margin_labels(mlm.float(), nsp.float())
    assert min(counts) >= 8, counts  # (a seed yielding fewer: change the seed, never the margin)
    assert n_nsp >= 1
    want = score_acc(cuda)
    _unfused(lambda *a: ref.score(*a, want, k=5), *inputs, labels, nsp_labels)
    assert not ref.bert._can_fuse(inputs[0]) and model.bert._can_fuse(inputs[0])
    model.max_predictions_per_seq_valid = 32  # the sparse head's capacity: 32 rows per sequence
    assert int((labels >= 0).sum(1).max()) <= 32
    got = score_acc(cuda)
    model.score(*inputs, labels, nsp_labels, got, k=5)
    assert model.training  # score() restores the mode
    bert_ops.check_device_errors(cuda)
    got, want = got.tolist(), want.tolist()
    print("engine=%s dtype=%s fused %s oracle %s" % (engine, dtype, got, want))
    assert want[1] == sum(counts) and want[2] == counts[0] and want[3] == counts[0] + counts[1]
    exact = (1, 5, 7) if dtype == "bf16" else (1, 2, 3, 5, 6, 7)
    if any(got[j] != want[j] for j in exact):
        with torch.no_grad():
            fused_mlm, fused_nsp = model.eval()(*inputs)
        print("largest logit deviation: mlm %.3g nsp %.3g" % ((fused_mlm.float() - mlm).abs().max().item(),
                                                               (fused_nsp.float() - nsp).abs().max().item()))
    for j in exact:
        assert got[j] == want[j], (j, got, want)
    rel, ab = {"default": (1e-4, 1e-5), "x6": (1e-5, 0.0)}[engine] if dtype == "fp32" else (5e-2, 0.0)
    for j in (0, 4):
        assert abs(got[j] - want[j]) <= rel * abs(want[j]) + ab, (j, got[j], want[j])


def _train(tmp_path, tag, validate_after):
    from hetseq_amd import options
    from hetseq_amd.controller import Controller
    from hetseq_amd.data.synthetic import write_bert_config, write_bert_shards, write_vocab
    from hetseq_amd.ops import bert_ops
    from hetseq_amd.tasks import LanguageModelingTask

    V = 1000
    d = str(tmp_path / tag)
    write_bert_shards(os.path.join(d, "data"), num_shards=1, per_shard=32, seq_len=64, max_pred=10, vocab_size=V,
                      seed=5, split="train")
    write_bert_shards(os.path.join(d, "data"), num_shards=1, per_shard=20, seq_len=64, max_pred=12, vocab_size=V,
                      seed=6, split="valid")
    write_vocab(os.path.join(d, "vocab.txt"), V)
    cfg = write_bert_config(os.path.join(d, "cfg.json"), vocab_size=V, hidden_size=256, num_hidden_layers=2,
                            num_attention_heads=4, intermediate_size=1024)
    args = options.parse_cli(["--task", "bert", "--data", os.path.join(d, "data"), "--dict",
                              os.path.join(d, "vocab.txt"), "--config_file", cfg, "--max-sentences", "8",
                              "--max-sentences-valid", "8", "--lr", "1e-3", "--warmup-updates", "2", "--max-update",
                              "100", "--fast-stat-sync", "--clip-norm", "1.0", "--distributed-world-size", "1",
                              "--log-format", "none", "--validate"])
    torch.manual_seed(args.seed)
    task = LanguageModelingTask.setup_task(args)
    task.load_dataset("valid")
    model = task.build_model(args)
    ctl = Controller(args, task, model)
    task.load_dataset("train")
    task.prepare_model_for_data(ctl.get_model(), "train")
    itr = task.get_batch_iterator(task.dataset("train"), max_sentences=8, seed=args.seed, num_workers=1, epoch=0,
                                  device=ctl.device).next_epoch_itr(shuffle=False)
    metrics = None
    for step, s in zip(range(4), itr):
        ctl.train_step([s])
        if step + 1 == validate_after:
            metrics = ctl.validate("valid")
            assert ctl.get_model().training and ctl.get_num_updates() == validate_after
    ctl.store.params_ready()
    torch.cuda.synchronize()
    bert_ops.check_device_errors(ctl.device)
    state = [ctl.store.param.clone()] + [ctl.optimizer._state[k].clone() for k in sorted(ctl.optimizer._state)]
    return state, metrics, ctl


def test_validation_does_not_disturb_training(cuda, tmp_path):
    plain, _, _ = _train(tmp_path, "plain", validate_after=0)
    mixed, metrics, ctl = _train(tmp_path, "mixed", validate_after=2)
    assert ctl.optimizer.staged  # the staged update at its default
    assert metrics is not None and metrics["nsentences"] == 20 and 0 < metrics["mlm_loss"] < 20
    assert metrics["mlm_acc"] <= metrics["mlm_acc5"] <= 1.0
    assert len(plain) == len(mixed) >= 3
    for a, b in zip(plain, mixed):
        assert torch.equal(a, b)
