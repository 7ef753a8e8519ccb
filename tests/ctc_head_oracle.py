"""fp64 oracle of the whole-utterance CTC head (cpc2_amd/csrc/ctc_head.hip, cpc2_amd/eval/common_voices_eval.py): normalisation
over the first `len` frames, the strided classifier, CTC with input lengths (probe_oracle.ctc_one on logits[i, :len_i]) and the
criterion as a whole.  Values are numpy float64; gradients are closed forms, or torch.autograd in float64 on the CPU where the
chain runs through the LSTM."""
import numpy as np
import torch

import probe_oracle


def seqnorm_len(x, lengths, eps=1e-8):
    """y [B, S, H]: per (b, channel) mean and unbiased variance over the frames < lengths[b], applied to ALL frames."""
    x = np.asarray(x, np.float64)
    y = np.empty_like(x)
    for b, n in enumerate(lengths):
        n = int(n)
        m = x[b, :n].mean(axis=0, keepdims=True)
        with np.errstate(invalid="ignore", divide="ignore"):
            v = ((x[b, :n] - m) ** 2).sum(axis=0, keepdims=True) / (n - 1)
            y[b] = (x[b] - m) / np.sqrt(v + eps)
    return y


def seqnorm_len_backward(x, lengths, dy, eps=1e-8):
    """dx by torch.autograd in float64 through the reference's own statement of the branch (mean / var over x[b, :size])."""
    xt = torch.tensor(np.asarray(x, np.float64), requires_grad=True)
    rows = []
    for b, n in enumerate(lengths):
        n = int(n)
        m = xt[b, :n].mean(dim=0, keepdim=True)
        v = xt[b, :n].var(dim=0, keepdim=True)
        rows.append((xt[b] - m) / torch.sqrt(v + eps))
    torch.stack(rows).backward(torch.tensor(np.asarray(dy, np.float64)))
    return xt.grad.numpy()


def _unfold(x, ks):
    """[B, P, ks * H]: row j = frames stride j .. stride j + ks of x [B, S, H] (the oracle may build it; the library never does)."""
    b, s, h = x.shape
    stride = ks // 2
    p = (s - ks) // stride + 1
    return np.stack([x[:, stride * j:stride * j + ks].reshape(b, ks * h) for j in range(p)], axis=1)


def conv_head(x, weight, bias):
    """Conv1d(H, C, ks, stride = ks // 2) on channel-last x [B, S, H] with the torch weight [C, H, ks] -> [B, P, C]."""
    x, weight, bias = (np.asarray(a, np.float64) for a in (x, weight, bias))
    ks = weight.shape[2]
    wp = weight.transpose(0, 2, 1).reshape(weight.shape[0], -1)           # [C, ks * H]
    return _unfold(x, ks) @ wp.T + bias


def conv_head_backward(x, weight, dout):
    """(dW [C, H, ks], db [C], dx [B, S, H]) of conv_head."""
    x, weight, dout = (np.asarray(a, np.float64) for a in (x, weight, dout))
    b, s, h = x.shape
    c, _, ks = weight.shape
    stride = ks // 2
    rows = _unfold(x, ks)
    p = rows.shape[1]
    dwp = dout.reshape(b * p, c).T @ rows.reshape(b * p, ks * h)
    wp = weight.transpose(0, 2, 1).reshape(c, ks * h)
    drows = (dout @ wp).reshape(b, p, ks, h)
    dx = np.zeros_like(x)
    for j in range(p):
        dx[:, stride * j:stride * j + ks] += drows[:, j]
    return dwp.reshape(c, ks, h).transpose(0, 2, 1), dout.sum(axis=(0, 1)), dx


def ctc_len(logits, in_lengths, targets, tgt_lengths, reduction):
    """nn.CTCLoss(blank = K - 1, reduction, zero_infinity=True) of log_softmax(logits [B, T, K]) with input lengths:
    (loss, nll [B] with infinities zeroed, dlogits [B, T, K], exactly 0 at and beyond each input length)."""
    logits = np.asarray(logits, np.float64)
    B = logits.shape[0]
    nll = np.zeros(B)
    grad = np.zeros(logits.shape)
    loss = 0.0
    for i in range(B):
        T, L = int(in_lengths[i]), int(tgt_lengths[i])
        scale = 1.0 / (B * max(L, 1)) if reduction == "mean" else 1.0
        if T == 0:
            continue
        v, g = probe_oracle.ctc_one(logits[i, :T], np.asarray(targets[i][:L], np.int64))
        if np.isinf(v):
            continue
        nll[i] = v
        grad[i, :T] = g * scale
        loss += v * scale
    return loss, nll, grad


def ctc_long_case(seed=256):
    """(logits [9, 300, 41] f32, input lengths, targets [9, 150], target lengths): transcriptions of 128 to 150 labels, so that
    the 2 L + 1 extended states pass 256 (a workgroup of ctc_len_kernel owns state s in thread s % 256).  Rows: 128 labels
    (257 states); 129; 150 with labels 126..129 equal (no-skip transitions at states 253..261); 150 labels that all differ from
    their neighbours in 299 frames; in exactly 150 frames (one alignment); in 149 (none); 150 equal labels in 300 frames (299
    are needed); in 298 (no alignment); and an empty transcription."""
    rng = np.random.default_rng(seed)
    b, t, w, k = 9, 300, 150, 41
    logits = (2 * rng.standard_normal((b, t, k))).astype(np.float32)
    targets = rng.integers(0, k - 1, (b, w))
    targets[2, 126:130] = targets[2, 126]
    targets[3:6] = np.arange(w) % 40
    targets[6:8] = 3
    in_len = np.array([300, 300, 300, 299, 150, 149, 300, 298, 300], np.int64)
    tgt_len = np.array([128, 129, 150, 150, 150, 150, 150, 150, 0], np.int64)
    return logits, in_len, targets.astype(np.int64), tgt_len


CTC_LONG_INFEASIBLE = (5, 7)


def criterion(c, sizes, state, seqNorm, useLSTM, label=None, labelSize=None, reduction="mean", eps=1e-8):
    """CTCphone_criterion in float64 (eval mode: no dropout).  state: the module's state dict (any float dtype).  Returns a dict:
    pred [B, P, C]; with labels also loss, dc and grads {state-dict key: gradient} (the LSTM's are zero arrays without useLSTM)."""
    ct = torch.tensor(np.asarray(c, np.float64), requires_grad=True)
    params = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in state.items()}
    x = ct
    if seqNorm:
        rows = []
        for b, n in enumerate(sizes):
            n = int(n)
            m = x[b, :n].mean(dim=0, keepdim=True)
            v = x[b, :n].var(dim=0, keepdim=True)
            rows.append((x[b] - m) / torch.sqrt(v + eps))
        x = torch.stack(rows)
    if useLSTM:
        h = x.shape[2]
        lstm = torch.nn.LSTM(h, h, num_layers=1, batch_first=True).double()
        for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
            getattr(lstm, f"{n}_l0").data.copy_(params[f"conv1.{n}_l0"].data)
            params[f"conv1.{n}_l0"] = getattr(lstm, f"{n}_l0")             # (its gradient is read below)
        x = lstm(x)[0]
    w, bias = params["PhoneCriterionClassifier.weight"], params["PhoneCriterionClassifier.bias"]
    pred = torch.nn.functional.conv1d(x.permute(0, 2, 1), w, bias, stride=w.shape[2] // 2).permute(0, 2, 1)
    out = dict(pred=pred.detach().numpy())
    if label is None:
        return out
    in_len = np.minimum(np.asarray(sizes, np.int64) // 4, pred.shape[1])
    loss, nll, dlogits = ctc_len(out["pred"], in_len, np.asarray(label), np.asarray(labelSize), reduction)
    pred.backward(torch.tensor(dlogits))
    out.update(loss=loss, nll=nll, dc=ct.grad.numpy(),
               grads={k: (p.grad.numpy() if p.grad is not None else np.zeros(tuple(p.shape))) for k, p in params.items()})
    return out
