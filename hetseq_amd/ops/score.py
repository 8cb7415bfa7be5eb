"""Validation scoring of the pre-training heads (score.hip).

One persistent device accumulator per validation pass::

    acc[8] = [mlm_loss_sum, mlm_n, mlm_top1, mlm_topk, nsp_loss_sum, nsp_n, nsp_correct, nsentences]

``mlm_nsp_score_`` ADDS one batch into it: losses in nats (sums, not means), counts as doubles.  A
row is labelled when its label is not ``ignore_index`` and lies in ``[0, V)``.  The label's rank is
its position in a stable descending sort of the row,

    rank = #{j : x[j] > x[lab]} + #{j < lab : x[j] == x[lab]},

so ties resolve to the lowest index (``torch.argmax``'s rule) and top-k is ``rank < k``.  NSP rows
(``[B, 2]`` logits) are correct when the lowest-index argmax equals the label; labels outside
``{0, 1}`` are ignored; ``nsentences`` counts every NSP row.

fp32 logits on a GPU go to the HIP kernel pair (one read of the logits, no host sync); anything
else (CPU tensors, other dtypes) to the torch implementation of the same definition.
"""
from __future__ import annotations

import torch

ACC_FIELDS = ("mlm_loss_sum", "mlm_n", "mlm_top1", "mlm_topk", "nsp_loss_sum", "nsp_n", "nsp_correct", "nsentences")


def score_acc(device):
    """A zeroed accumulator (see the module docstring for its layout)."""
    return torch.zeros(len(ACC_FIELDS), dtype=torch.float64, device=device)


def _score_torch(logits, labels, nsp_logits, nsp_labels, k, ignore_index):
    """The eight sums of one batch as a float64 tensor on the logits' device (torch ops)."""
    out = torch.zeros(len(ACC_FIELDS), dtype=torch.float64, device=logits.device)
    V = logits.shape[1]
    valid = (labels != ignore_index) & (labels >= 0) & (labels < V)
    if logits.shape[0] > 0:
        x = logits.float()
        lab = labels.clamp(0, V - 1)
        xl = x.gather(1, lab[:, None])
        col = torch.arange(V, device=x.device)[None, :]
        rank = ((x > xl) | ((x == xl) & (col < lab[:, None]))).sum(1)
        loss = torch.logsumexp(x, 1) - xl[:, 0]
        out[0] = torch.where(valid, loss, torch.zeros_like(loss)).double().sum()
        out[1] = valid.sum()
        out[2] = (valid & (rank == 0)).sum()
        out[3] = (valid & (rank < k)).sum()
    if nsp_logits.shape[0] > 0:
        y = nsp_logits.float()
        ok = (nsp_labels == 0) | (nsp_labels == 1)
        nl = nsp_labels.clamp(0, 1)
        nloss = torch.logsumexp(y, 1) - y.gather(1, nl[:, None])[:, 0]
        out[4] = torch.where(ok, nloss, torch.zeros_like(nloss)).double().sum()
        out[5] = ok.sum()
        out[6] = (ok & ((y[:, 1] > y[:, 0]).long() == nl)).sum()
        out[7] = y.shape[0]
    return out


def mlm_nsp_score_(acc, logits, labels, nsp_logits, nsp_labels, k=5, ignore_index=-1):
    """``acc += `` the eight sums of one batch; returns ``acc``.

    ``logits`` [R, V] (any row stride; columns past V are never read), ``labels`` [R] int64,
    ``nsp_logits`` [B, 2], ``nsp_labels`` [B] int64."""
    assert acc.dtype == torch.float64 and acc.numel() == len(ACC_FIELDS) and acc.is_contiguous()
    assert logits.dim() == 2 and labels.numel() == logits.shape[0] and labels.dtype == torch.int64
    assert nsp_logits.dim() == 2 and nsp_logits.shape[1] == 2 and nsp_labels.numel() == nsp_logits.shape[0]
    assert nsp_labels.dtype == torch.int64
    labels, nsp_labels = labels.reshape(-1), nsp_labels.reshape(-1)
    if (logits.is_cuda and acc.is_cuda and logits.dtype == torch.float32 and nsp_logits.dtype == torch.float32
            and logits.stride(1) == 1 and logits.stride(0) >= logits.shape[1]):
        from hetseq_amd.ops._C import hip, stream_handle

        R, V = logits.shape
        dev = logits.device
        labels, nsp_labels, nsp_logits = labels.contiguous(), nsp_labels.contiguous(), nsp_logits.contiguous()
        row_loss = torch.empty(max(R, 1), dtype=torch.float32, device=dev)
        rank = torch.empty(max(R, 1), dtype=torch.int32, device=dev)
        rc = hip().mlm_nsp_score(0, logits.data_ptr(), labels.data_ptr(), R, V, logits.stride(0), ignore_index, k,
                                 nsp_logits.data_ptr(), nsp_labels.data_ptr(), nsp_logits.shape[0],
                                 row_loss.data_ptr(), rank.data_ptr(), acc.data_ptr(), stream_handle())
        if rc != 0:
            raise RuntimeError("mlm_nsp_score: the kernel does not serve this dtype")
        return acc
    acc += _score_torch(logits, labels, nsp_logits, nsp_labels, k, ignore_index).to(acc.device)
    return acc


def metrics(acc_host):
    """Set-level pre-training metrics from an accumulator's host values (losses in nats)."""
    import math
    from collections import OrderedDict

    a = [float(v) for v in acc_host]
    mlm_n, nsp_n = max(a[1], 1.0), max(a[5], 1.0)
    mlm_loss, nsp_loss = a[0] / mlm_n, a[4] / nsp_n
    out = OrderedDict()
    out["loss"] = mlm_loss + nsp_loss
    out["mlm_loss"] = mlm_loss
    out["nsp_loss"] = nsp_loss
    out["mlm_ppl"] = math.exp(min(mlm_loss, 700.0))
    out["mlm_acc"] = a[2] / mlm_n
    out["mlm_acc5"] = a[3] / mlm_n
    out["nsp_acc"] = a[6] / nsp_n
    out["nsentences"] = a[7]
    return out
