"""Linear-separability probe on the GPU (csrc/probe.hip): the cross-entropy and CTC heads against the fp64 oracle
(tests/probe_oracle.py), ties, reproducibility, the three criteria against the reference's recorded values and Adam
trajectories (golden g21), --unfrozen gradients through the model against an fp64 restatement, and the command line end
to end on the committed audio."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import probe_oracle as PO
from cpc2_amd import _lib
from cpc2_amd.criterion import CTCPhoneCriterion, PhoneCriterion, SpeakerCriterion
from cpc2_amd.train import FlatAdam

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DB = os.path.join(GOLDEN, "test_db")
PHONES = os.path.join(GOLDEN, "phone_labels.txt")
CKPT = os.path.join(GOLDEN, "ref_checkpoint", "checkpoint_7.pt")
DEV = torch.device("cuda:0")


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _rel_l2(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))


# --------------------------------------------------------------------------- cross-entropy head
# every C with every width; N (odd, up to 64 * 128 - 1) cycles through a list, shorter for the widest C
_XENT_CASES = [(c, h, (1, 63, 1001, 8191)[i % 4] if c <= 251 else (1, 63, 257)[i % 3])
               for i, (c, h) in enumerate([(c, h) for c in (1, 2, 41, 63, 64, 65, 251, 1000, 2338) for h in (256, 512, 77)])]


def _head_run(x, w, b, y):
    """loss, acc, dX, dW, db of the xent head through the criterion's autograd function (one row per frame)."""
    from cpc2_amd.criterion import _ProbeHeadFn
    xd = x.clone().requires_grad_(True)
    wd, bd = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    loss, acc = _ProbeHeadFn.apply(xd, wd, bd, "xent", y, None, False, True)
    loss.sum().backward()
    return loss, acc, xd.grad, wd.grad, bd.grad


@pytest.mark.parametrize("c,h,n", _XENT_CASES)
def test_xent_head_vs_fp64(c, h, n):
    g = torch.Generator().manual_seed(c * 7919 + h * 13 + n)
    x = torch.randn(n, h, generator=g)
    w = torch.randn(c, h, generator=g) / h ** 0.5
    b = torch.randn(c, generator=g) * 0.1
    y = torch.randint(0, c, (n,), generator=g)
    o = PO.xent(x.numpy(), w.numpy(), b.numpy(), y.numpy())
    loss, acc, dx, dw, db = _head_run(x.to(DEV), w.to(DEV), b.to(DEV), y.to(DEV))
    assert abs(loss.item() - o["loss"]) <= 1e-5 * abs(o["loss"])
    assert _rel_l2(dw.cpu(), o["dW"]) <= 1e-5
    assert _rel_l2(db.cpu(), o["db"]) <= 1e-5
    assert _rel_l2(dx.cpu(), o["dX"]) <= 1e-5
    assert acc.dtype == torch.float64
    # argmax: with labels = the oracle's prediction every row whose top-2 margin exceeds 1e-5 must count as correct
    z = o["logits"]
    top2 = np.sort(z, axis=1)[:, -2:] if c > 1 else np.concatenate([z, z - 1], axis=1)
    margin = (top2[:, 1] - top2[:, 0]) / np.maximum(np.abs(top2[:, 1]), 1e-30)
    pred_labels = torch.from_numpy(o["pred"]).to(DEV)
    _, acc2, _, _, _ = _head_run(x.to(DEV), w.to(DEV), b.to(DEV), pred_labels)
    correct = _correct_flags(x.to(DEV), w.to(DEV), b.to(DEV), pred_labels)
    assert np.all(correct[margin > 1e-5] == 1)
    assert float(acc2) == correct.mean()


def _correct_flags(x, w, b, y):
    lib = _lib.load()
    n, c = x.shape[0], w.shape[0]
    logits = x @ w.t() + b           # (the flags only: the kernel's own logits are tested above)
    nll = torch.empty(n, device=DEV)
    correct = torch.empty(n, dtype=torch.int32, device=DEV)
    loss = torch.empty(1, device=DEV)
    acc = torch.empty(1, dtype=torch.float64, device=DEV)
    _lib.check(lib.cpc_probe_xent(_p(logits), _p(y), n, c, 0, _p(nll), _p(correct), _p(loss), _p(acc), _st()), "probe_xent")
    return correct.cpu().numpy()


def test_xent_ties_go_to_the_lowest_index():
    lib = _lib.load()
    n, c = 6, 130
    logits = torch.full((n, c), -1.0)
    tied = [(3, 70), (0, 64), (5, 129), (1, 2), (64, 128), (10, 74)]
    for r, (i, j) in enumerate(tied):
        logits[r, i] = logits[r, j] = 2.5
    for labels, expect in (([i for i, _ in tied], 1), ([j for _, j in tied], 0)):
        lg = logits.to(DEV)
        y = torch.tensor(labels, device=DEV)
        nll = torch.empty(n, device=DEV)
        correct = torch.empty(n, dtype=torch.int32, device=DEV)
        loss = torch.empty(1, device=DEV)
        acc = torch.empty(1, dtype=torch.float64, device=DEV)
        _lib.check(lib.cpc_probe_xent(_p(lg), _p(y), n, c, 0, _p(nll), _p(correct), _p(loss), _p(acc), _st()), "probe_xent")
        assert correct.cpu().tolist() == [expect] * n
        assert float(acc) == float(expect)


def test_xent_head_bitwise_reproducible():
    g = torch.Generator().manual_seed(5)
    x, w, b = torch.randn(8191, 512, generator=g), torch.randn(251, 512, generator=g) / 20, torch.randn(251, generator=g)
    y = torch.randint(0, 251, (8191,), generator=g)
    runs = [[t.cpu() for t in _head_run(x.to(DEV), w.to(DEV), b.to(DEV), y.to(DEV))] for _ in range(2)]
    for a, bb in zip(*runs):
        assert torch.equal(a, bb)


# --------------------------------------------------------------------------- CTC head
def _ctc_case(B, K, seed, T=128):
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((B, T, K)) * 2).astype(np.float32)
    lengths, targets = [], []
    for i in range(B):
        kind = i % 6
        if kind == 0:
            L = min(int(rng.integers(15, 41)), T)
            tg = rng.integers(0, K - 1, size=L)
        elif kind == 1:
            L, tg = 0, np.zeros(0, np.int64)
        elif kind == 2:                                # repeated labels
            L = min(int(rng.integers(5, 30)), T)
            tg = np.repeat(rng.integers(0, K - 1, size=(L + 1) // 2), 2)[:L]
        elif kind == 3:                                # infeasible: T equal labels need 2T - 1 frames
            L, tg = T, np.full(T, int(rng.integers(0, K - 1)))
        elif kind == 4:                                # L = T, all different neighbours: feasible only on the diagonal
            L = T
            tg = np.arange(T) % (K - 1)
        else:
            L = int(rng.integers(1, T // 2))
            tg = rng.integers(0, K - 1, size=L)
        lengths.append(L)
        targets.append(np.asarray(tg, np.int64))
    padded = np.zeros((B, T), np.int64)
    for i, tg in enumerate(targets):
        padded[i, :len(tg)] = tg
    return logits, padded, np.array(lengths, np.int64), targets


def _ctc_run(logits, padded, lengths, grad=True, in_place=False):
    """in_place: the gradient overwrites the logits, which is how the criterion calls the entry."""
    lib = _lib.load()
    B, T, K = logits.shape
    lg = torch.from_numpy(logits).to(DEV)
    tg = torch.from_numpy(padded).to(DEV)
    ln = torch.from_numpy(lengths).to(DEV)
    nll = torch.empty(B, device=DEV)
    loss = torch.empty(1, device=DEV)
    dl = (lg if in_place else torch.empty_like(lg)) if grad else None
    nb = lib.cpc_probe_ctc_scratch_bytes(B, T, padded.shape[1])
    sc = torch.empty(nb, dtype=torch.uint8, device=DEV)
    _lib.check(lib.cpc_probe_ctc(_p(lg), B, T, K, _p(tg), padded.shape[1], _p(ln), _p(nll), _p(loss), _p(dl), _p(sc), nb, _st()),
               "probe_ctc")
    return float(loss), nll.cpu().numpy(), None if dl is None else dl.cpu().numpy()


# Bound: alpha and beta are f64, so the only f32 roundings are the output's cast and the f32 sum of the per-sequence losses,
# far below 2e-5 relative (an f32 alpha would not be: DESIGN.md section 9).
# (2, 2) at T = 3: one partial chunk of the gradient kernel and one label class; (3, 64) at T = 32: T K = 2 chunks exactly.
@pytest.mark.parametrize("B,K,T", [pytest.param(1, 42, 128, id="1-42"), pytest.param(8, 42, 128, id="8-42"),
                                   pytest.param(64, 42, 128, id="64-42"), pytest.param(8, 100, 128, id="8-100"),
                                   pytest.param(2, 2, 3, id="2-2-T3"), pytest.param(3, 64, 32, id="3-64-T32")])
def test_ctc_vs_fp64(B, K, T):
    logits, padded, lengths, targets = _ctc_case(B, K, seed=B * 31 + K, T=T)
    assert np.all((lengths >= 0) & (lengths <= T))
    ref_loss, ref_nll, ref_grad = PO.ctc(logits.astype(np.float64), targets, lengths)
    loss, nll, grad = _ctc_run(logits, padded, lengths)
    assert abs(loss - ref_loss) <= 2e-5 * abs(ref_loss)
    assert np.all(np.abs(nll - ref_nll) <= 2e-5 * np.abs(ref_nll))
    assert np.abs(grad - ref_grad).max() <= 2e-5 * np.abs(ref_grad).max()
    inf_rows = [i for i in range(B) if ref_nll[i] == 0.0 and lengths[i] > 0]
    for i in inf_rows:                                 # zero_infinity: exactly 0
        assert nll[i] == 0.0 and np.all(grad[i] == 0.0)
    if B >= 4:
        assert inf_rows, "the case must hold an infeasible target"
    # bitwise reproducible
    loss2, nll2, grad2 = _ctc_run(logits, padded, lengths)
    assert loss2 == loss and np.array_equal(nll2, nll) and np.array_equal(grad2, grad)


def test_ctc_gradient_in_place_equals_out_of_place():
    """The criterion passes the logits' buffer as the gradient's.  The forward and the gradient are two launches: an element of
    the gradient reads the logits at its own place only, so writing over them changes nothing."""
    logits, padded, lengths, _ = _ctc_case(6, 6, seed=11, T=20)
    apart = _ctc_run(logits, padded, lengths)
    over = _ctc_run(logits, padded, lengths, in_place=True)
    assert apart[0] == over[0] and np.array_equal(apart[1], over[1]) and np.array_equal(apart[2], over[2])
    assert not np.array_equal(over[2], logits)


def test_ctc_padded_width_does_not_matter():
    logits, padded, lengths, _ = _ctc_case(6, 42, seed=3)
    wide = _ctc_run(logits, padded, lengths)
    narrow = _ctc_run(logits, np.ascontiguousarray(padded[:, :int(lengths.max())]), lengths)
    assert wide[0] == narrow[0] and np.array_equal(wide[1], narrow[1]) and np.array_equal(wide[2], narrow[2])


def test_collapse_vs_reference(golden):
    from cpc2_amd.seq_alignment import collapseLabelChain
    z = golden("g21_linear_separability.npz")
    for tag, rows in (("all", slice(None)), ("three", slice(2, 5)), ("one", slice(7, 8))):
        out, sizes = collapseLabelChain(torch.from_numpy(z["phonem"][rows]).to(DEV))
        assert out.dtype == torch.int64 and np.array_equal(out.cpu().numpy(), z[f"collapse_{tag}_out"])
        assert np.array_equal(sizes.cpu().numpy(), z[f"collapse_{tag}_sizes"])
    # wider rows than one wave, with long runs
    rng = np.random.default_rng(0)
    lab = np.repeat(rng.integers(0, 5, size=(7, 100)), 3, axis=1)[:, :257]
    out, sizes = collapseLabelChain(torch.from_numpy(lab).to(DEV))
    ref_out, ref_sizes = PO.collapse(lab)
    assert np.array_equal(out.cpu().numpy(), ref_out) and np.array_equal(sizes.cpu().numpy(), ref_sizes)


# --------------------------------------------------------------------------- the criteria against the reference (g21)
def _g21():
    z = np.load(os.path.join(GOLDEN, "g21_linear_separability.npz"), allow_pickle=False)
    return z, json.loads(str(z["meta"]))


def _make(tag, meta, H):
    n = meta["n_phones"]
    return {"phone1": lambda: PhoneCriterion(H, n, False), "phone2": lambda: PhoneCriterion(H, n, False, nLayers=2),
            "speaker": lambda: SpeakerCriterion(H, meta["n_speakers"]), "ctc": lambda: CTCPhoneCriterion(H, n, False)}[tag]


def _labels(tag, z, meta):
    """The labels of the two feature windows, as the reference's AudioBatchData gave them: speaker index, or the pack's phone
    labels (files in (speaker, name) order) from offset // 160 on."""
    import bisect
    feats = z["feat_offsets"].tolist()
    if tag == "speaker":
        return torch.tensor([bisect.bisect_right(meta["speaker_label"], o) - 1 for o in feats])
    order = sorted((spk, os.path.splitext(os.path.basename(path))[0]) for spk, path in meta["seqs"])
    labels = np.concatenate([z[f"labels_{name}"] for _spk, name in order])
    return torch.from_numpy(np.stack([labels[o // 160:o // 160 + 128] for o in feats]))


@pytest.mark.parametrize("tag", ["phone1", "phone2", "speaker", "ctc"])
def test_criterion_vs_reference(tag):
    z, meta = _g21()
    c = torch.from_numpy(z["cfeature"]).to(DEV)
    H = c.shape[2]                                      # (the reference checkpoint's width)
    torch.manual_seed(meta[tag]["seed"])
    crit = _make(tag, meta, H)().to(DEV)
    proj = torch.from_numpy(np.random.default_rng(21).standard_normal((H, 8)))
    label = _labels(tag, z, meta).to(DEV)
    feat = c.clone().requires_grad_(True)
    loss, acc = crit(feat, feat, label)
    loss.sum().backward()
    assert loss.shape == (1, 1) and acc.shape == (1, 1)
    ref = z[f"{tag}_loss"]
    assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item())
    assert acc.item() == z[f"{tag}_acc"].item()
    # CTC: torch's f32 CTC (the recorded run) keeps alpha / beta in f32 log space, where one ulp of |log alpha| (~100-500 here)
    # is 1e-5 - 3e-5 of the occupancy; the kernel works in f64.  Its gradients are held to 1e-5 of the reference run in float64
    # and to 1e-4 of the f32 one.
    refs = [(tag, 1e-5)] if tag != "ctc" else [("ctc64", 1e-5), ("ctc", 1e-4)]
    for rtag, tol in refs:
        for name, p in crit.named_parameters():
            assert _rel_l2(p.grad.cpu(), z[f"{rtag}_grad_{name}"]) <= tol, (rtag, name)
        assert _rel_l2((feat.grad.double().cpu() @ proj).numpy(), z[f"{rtag}_dX_proj"]) <= tol, rtag
    # 20 Adam steps (FlatAdam, the reference's torch.optim.Adam arithmetic) on the fixed batches
    torch.manual_seed(meta[tag]["seed"])
    crit = _make(tag, meta, H)().to(DEV)
    opt = FlatAdam(list(crit.parameters()), lr=2e-4, eps=2e-8)
    batches = [slice(0, 1), slice(1, 2), slice(0, 2)]
    traj = []
    for i in range(20):
        rows = batches[i % 3]
        opt.zero_grad()
        loss, _ = crit(c[rows], c[rows], label[rows])
        loss.sum().backward()
        opt.step()
        traj.append(loss.detach())
    traj = torch.cat([t.view(1) for t in traj]).cpu().double().numpy()
    assert np.all(np.abs(traj - z[f"{tag}_traj"]) <= 1e-4 * np.abs(z[f"{tag}_traj"]))
    for name, p in crit.named_parameters():
        ref = z[f"{tag}_final_{name}"]
        assert np.abs(p.detach().cpu().numpy() - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max()), name


# --------------------------------------------------------------------------- --unfrozen: gradients through the model
@pytest.mark.parametrize("mode", ["GRU", "LSTM"])
def test_unfrozen_phone_gradients_vs_fp64(mode):
    import cpc2_amd
    from oracle import cpc_oracle as O
    from oracle import synth
    hidden, b, n_phones = 256, 4, 41
    mp = synth.encoder_params(hidden, 11)
    mp.update(synth.gru_params(hidden, hidden, 1, 41) if mode == "GRU" else synth.lstm_params(hidden, hidden, 1, 41))
    model = cpc2_amd.CPCModel(cpc2_amd.CPCEncoder(hidden), cpc2_amd.CPCAR(hidden, hidden, False, 1, mode=mode))
    model.load_state_dict(mp)
    torch.manual_seed(3)
    crit = PhoneCriterion(hidden, n_phones, False)
    cw = {k: v.clone() for k, v in crit.state_dict().items()}
    model, crit = model.to(DEV).train(), crit.to(DEV)
    x = synth.audio_windows(b, 20480, 12)
    label = torch.randint(0, n_phones, (b, 128), generator=torch.Generator().manual_seed(4))
    c, z, _ = model(x.to(DEV), None)
    assert c.shape == (b, 128, hidden)                   # every frame reaches the probe
    loss, _ = crit(c, z, label.to(DEV))
    loss.sum().backward()
    p64 = {k: v.double().requires_grad_(True) for k, v in mp.items()}
    w64 = cw["PhoneCriterionClassifier.weight"].double()
    b64 = cw["PhoneCriterionClassifier.bias"].double()
    c64, _ = O.model_forward(x.double(), p64, 1, ar=mode)
    ref = torch.nn.functional.cross_entropy(c64.reshape(-1, hidden) @ w64.t() + b64, label.reshape(-1))
    ref.backward()
    assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item())
    for name, p in model.named_parameters():
        if name in p64:
            assert _rel_l2(p.grad.cpu(), p64[name].grad) <= 1e-4, name


# --------------------------------------------------------------------------- the command line end to end
def _val_recompute(ckpt_dir, epoch, kind, val_names, n_phones, n_speakers, batch=1):
    """The logged validation numbers of `epoch` recomputed in fp64 from the saved classifier over the sequential validation
    windows (features from the package's model, as the run itself uses), with the reference's division by the last index."""
    from cpc2_amd import feature_loader as fl
    from cpc2_amd.dataset import AudioBatchData, filterSeqs, findAllSeqs, parseSeqLabels
    st = torch.load(os.path.join(ckpt_dir, f"checkpoint_{epoch}.pt"), map_location="cpu")
    model, _, _ = fl.loadModel([CKPT])
    model.load_state_dict(st["gEncoder"], strict=False)
    model = model.to(DEV).eval()
    seqs, speakers = findAllSeqs(DB, extension=".flac")
    phone = parseSeqLabels(PHONES)[0] if kind != "speaker" else None
    db = AudioBatchData(DB, 20480, filterSeqs(val_names, seqs), phone, len(speakers), device=DEV)
    cs = st["cpcCriterion"]
    key = "linearSpeakerClassifier" if kind == "speaker" else "PhoneCriterionClassifier"
    w, bias = cs[f"{key}.weight"].double(), cs[f"{key}.bias"].double()
    losses, accs = [], []
    for x, label in db.getDataLoader(batch, "sequential", False):
        with torch.no_grad():
            c, _, _ = model(x[:, 0], None)
        c = c.double().cpu()
        label = label.cpu()
        if kind == "speaker":
            o = PO.xent(c[:, -1].numpy(), w.numpy(), bias.numpy(), label.numpy())
            losses.append(o["loss"]), accs.append(o["acc"])
        elif kind == "phone":
            o = PO.xent(c.reshape(-1, c.shape[2]).numpy(), w.numpy(), bias.numpy(), label.reshape(-1).numpy())
            losses.append(o["loss"]), accs.append(o["acc"])
        else:
            logits = (c @ w.t() + bias).numpy()
            out, sizes = PO.collapse(label.numpy())
            loss, _, _ = PO.ctc(logits, list(out), sizes)
            losses.append(loss), accs.append(0.0)
    step = len(losses) - 1
    return sum(losses) / step, sum(accs) / step, len(losses)


@pytest.mark.parametrize("kind", ["phone", "ctc", "speaker", "unfrozen"])
def test_command_line_end_to_end(kind, tmp_path, capsys):
    from cpc2_amd.eval import linear_separability as LS
    train, val = tmp_path / "train.txt", tmp_path / "val.txt"
    if kind == "speaker":                              # all nine files: the seven of seq_list.txt train, the two labelled validate
        train.write_text(open(os.path.join(GOLDEN, "seq_list.txt")).read())
        val.write_text("2911-12359-0007\n4051-11218-0044\n")
    else:
        train.write_text("4051-11218-0044\n")
        val.write_text("2911-12359-0007\n")
    out = tmp_path / "out"
    argv = [DB, str(train), str(val), CKPT, "--batchSizeGPU", "1", "--n_epoch", "2", "--pathCheckpoint", str(out)]
    if kind != "speaker":
        argv += ["--pathPhone", PHONES]
    if kind == "ctc":
        argv += ["--CTC"]
    if kind == "unfrozen":
        argv += ["--unfrozen"]
    torch.manual_seed(0)
    LS.main(argv)
    printed = capsys.readouterr().out
    assert "Training loss" in printed and "Validation loss" in printed and "locLoss_val" in printed
    assert sorted(os.listdir(out)) == ["checkpoint_1.pt", "checkpoint_args.json", "checkpoint_logs.json"]
    st = torch.load(out / "checkpoint_1.pt", map_location="cpu")
    assert sorted(st) == ["best", "cpcCriterion", "gEncoder", "optimizer"]
    assert sorted(st["best"]) == sorted(st["gEncoder"])           # the feature maker's state
    logs = json.load(open(out / "checkpoint_logs.json"))
    assert logs["epoch"] == [0, 1] and logs["saveStep"] == 2
    args = json.load(open(out / "checkpoint_args.json"))
    assert args["nGPU"] == 1 and args["batchSizeGPU"] == 1
    rc_kind = {"phone": "phone", "unfrozen": "phone", "ctc": "ctc", "speaker": "speaker"}[kind]
    loss, acc, n_batches = _val_recompute(str(out), 1, rc_kind, str(val), 41, 6)
    if kind != "speaker":
        assert n_batches == 3                          # 81 280 samples: the logs divide by 2
    assert abs(logs["locLoss_val"][1][0] - loss) <= 1e-5 * abs(loss)
    assert abs(logs["locAcc_val"][1][0] - acc) <= 1e-5 * max(abs(acc), 1e-12)
    if kind == "ctc":
        assert logs["locAcc_val"][1][0] == 0.0 and logs["locAcc_train"][1][0] == 0.0
