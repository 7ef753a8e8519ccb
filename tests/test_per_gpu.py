"""Phone error rate on the GPU (csrc/seqalign.hip through cpc2_amd.seq_alignment and cpc2_amd.eval.phone_error_rate): the beam
search against the reference's recorded outputs (tests/golden/g26_per.npz) by EQUALITY -- label sequences in order and scores
as float32 bit patterns, all nKeep of them -- alone and in ragged batches; the alignment score against the reference's integers;
getPER and the command-line tool against tests/per_oracle.py window by window."""
import json
import os

import numpy as np
import pytest
import torch

import per_oracle
from cpc2_amd import criterion as cr
from cpc2_amd import feature_loader as fl
from cpc2_amd import seq_alignment as sa

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DB = os.path.join(GOLDEN, "test_db")
PHONES = os.path.join(GOLDEN, "phone_labels.txt")
CKPT = os.path.join(GOLDEN, "ref_checkpoint", "checkpoint_7.pt")
DEV = torch.device("cuda:0")
TIE_FREE = ["T1P2k1", "T7P3k1", "T32P9k20", "T32P9k20_blankmid", "T40P70k20_peaky", "T128P42k100_peaky", "T96P42k20_rand",
            "T128P42k20_rand_denormal"]
TIED = "T6P5k4_tied"


def cases(g):
    return {c["name"]: c for c in json.loads(str(g["meta"]))["search"]}


def recorded(g, tag):
    return [(int(b), [int(x) for x in lab[:n]]) for b, lab, n in zip(g[f"{tag}_score_bits"], g[f"{tag}_labels"], g[f"{tag}_lens"])]


def as_bits(out):
    return [(int(np.float32(s).view(np.uint32)), list(lab)) for s, lab in out]


def rows_of(scores, sizes, labels, counts, n):
    """Row n of a batch result as [(score bits, [labels])]; checks the padding on the way."""
    scores, sizes, labels = scores[n].cpu().numpy(), sizes[n].cpu().numpy(), labels[n].cpu().numpy()
    kept = int(counts[n])
    out = []
    for r in range(scores.shape[0]):
        if r < kept:
            assert (labels[r, sizes[r]:] == -1).all() and (labels[r, :sizes[r]] >= 0).all()
            out.append((int(scores[r].view(np.uint32)), [int(x) for x in labels[r, :sizes[r]]]))
        else:
            assert scores[r] == 0 and sizes[r] == 0 and (labels[r] == -1).all()
    return out


@pytest.mark.parametrize("name", TIE_FREE)
def test_single_sequence_equals_the_reference_bit_for_bit(golden, name):
    g = golden("g26_per.npz")
    case = cases(g)[name]
    probs = g[f"bs_{name}_probs"]
    want = recorded(g, f"bs_{name}")
    out = sa.beam_search(probs, case["nKeep"], case["blank"])
    assert all(isinstance(s, np.float32) for s, _ in out)
    assert as_bits(out) == want
    res = sa.beam_search_batch(torch.from_numpy(probs).to(DEV)[None], None, case["nKeep"], case["blank"])
    assert int(res[4][0]) == 0 and int(res[3][0]) == len(want)
    assert rows_of(*res[:4], 0) == want
    assert as_bits(sa.beam_search(torch.from_numpy(probs).to(DEV), case["nKeep"], case["blank"])) == want


def test_tied_case_sets_the_flag_and_repeats_its_bytes(golden):
    g = golden("g26_per.npz")
    case = cases(g)[TIED]
    probs = torch.from_numpy(g[f"bs_{TIED}_probs"]).to(DEV)[None]
    a = sa.beam_search_batch(probs, None, case["nKeep"], case["blank"])
    b = sa.beam_search_batch(probs, None, case["nKeep"], case["blank"])
    assert int(a[4][0]) == 1
    for x, y in zip(a, b):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    # the documented order of equal scores is the oracle's: (rank of the extended prefix, symbol)
    want, tie = per_oracle.beam_search(g[f"bs_{TIED}_probs"], case["nKeep"], case["blank"])
    assert tie and rows_of(*a[:4], 0) == as_bits(want)


def test_all_zero_scores_are_all_ties_and_stay_in_bounds():
    """Rows of 1e-30 underflow to exactly 0 within two frames: every candidate ties, the order is the documented one."""
    probs = np.full((5, 7), 1e-30, np.float32)
    a = sa.beam_search_batch(torch.from_numpy(probs).to(DEV)[None], None, 6, 0)
    want, tie = per_oracle.beam_search(probs, 6, 0)
    assert tie and int(a[4][0]) == 1 and rows_of(*a[:4], 0) == as_bits(want)


def test_limits_of_the_kernel_128_classes_128_prefixes():
    """nKeep = P = 128: 16384 candidates per frame, the 64 KiB of LDS and the 1024-thread launch."""
    g = torch.Generator().manual_seed(5)
    probs = torch.softmax(2.0 * torch.randn(5, 128, generator=g), 1).numpy()
    want, tie = per_oracle.beam_search(probs, 128, 77)
    res = sa.beam_search_batch(torch.from_numpy(probs).to(DEV)[None], None, 128, 77)
    assert int(res[4][0]) == int(tie) and rows_of(*res[:4], 0) == as_bits(want)


def test_ragged_batches_with_nan_behind_the_lengths(golden):
    """Every golden case in a batch [N, 128, P] beside the others of its (P, nKeep, blank) -- a launch has one nKeep and one
    blank -- and beside a shortened copy of itself (checked against the oracle); rows beyond lengths[n] are NaN.  The tied case
    is recorded in the reference's order of equal scores (by the prefixes' strings), which is not reproduced: its rows are held
    to the oracle, whose order is the documented one and which the kernel alone equals in the test above."""
    g = golden("g26_per.npz")
    groups = {}
    for name in TIE_FREE + [TIED]:
        c = cases(g)[name]
        groups.setdefault((c["P"], c["nKeep"], c["blank"]), []).append(name)
    assert len(groups[(42, 20, 41)]) == 2
    for (P, n_keep, blank), names in groups.items():
        rows = []
        for name in names:
            probs = g[f"bs_{name}_probs"]
            rows.append((probs, as_bits(per_oracle.beam_search(probs, n_keep, blank)[0]) if name == TIED
                         else recorded(g, f"bs_{name}")))
            short = probs[:max(1, probs.shape[0] // 3)]
            rows.append((short, as_bits(per_oracle.beam_search(short, n_keep, blank)[0])))
        batch = torch.full((len(rows), 128, P), float("nan"))
        for i, (probs, _) in enumerate(rows):
            batch[i, :probs.shape[0]] = torch.from_numpy(probs)
        lengths = torch.tensor([r[0].shape[0] for r in rows], device=DEV)
        full = sa.beam_search_batch(batch.to(DEV), lengths, n_keep, blank)
        best = sa.beam_search_batch(batch.to(DEV), lengths, n_keep, blank, best_only=True)
        assert best[0].shape == (len(rows), 1) and best[2].shape == (len(rows), 1, 128)
        for i, (_, want) in enumerate(rows):
            assert rows_of(*full[:4], i) == want, (names, i)
            assert rows_of(*best[:4], i) == want[:1], (names, i)
        assert torch.equal(full[4], best[4])


def test_alignment_scores_equal_the_reference(golden):
    g = golden("g26_per.npz")
    a, b = torch.from_numpy(g["al_seq1"]).to(DEV), torch.from_numpy(g["al_seq2"]).to(DEV)
    la, lb = torch.from_numpy(g["al_len1"]).to(DEV), torch.from_numpy(g["al_len2"]).to(DEV)
    assert sa.align_score_batch(a, la, b, lb, -1, -1, 0).cpu().tolist() == g["al_score_110"].tolist()
    assert sa.align_score_batch(a, la, b, lb, -2, -3, 1).cpu().tolist() == g["al_score_231"].tolist()
    assert sa.align_score_batch(a.long(), la.long(), b.long(), lb.long(), -1, -1, 0).cpu().tolist() == g["al_score_110"].tolist()
    assert sa.get_seq_PER_batch(a, la, b, lb).cpu().tolist() == g["al_per"].tolist()
    for i in (0, 1, 2, 7, 40):
        s1, s2 = g["al_seq1"][i, :g["al_len1"][i]].tolist(), g["al_seq2"][i, :g["al_len2"][i]].tolist()
        assert sa.get_seq_PER(s1, s2) == g["al_per"][i]
        assert sa.NeedlemanWunschAlignScore(s1, s2, -2, -3, 1, normalize=False) == g["al_score_231"][i]
    assert sa.get_seq_PER(torch.tensor([0, 1, 1, 2, 0, 2, 2], device=DEV), torch.tensor([1, 1, 2, 2, 0, 0], device=DEV)) == 4. / 7.


def test_alignment_of_sequences_longer_than_a_wave():
    """Rows of 150 and 200 labels: three and four 64-column strips, the carry between them."""
    rng = np.random.default_rng(3)
    s1, s2 = rng.integers(0, 5, (3, 150)), rng.integers(0, 5, (3, 200))
    s2[1, :150] = s1[1]
    l1, l2 = [150, 150, 64], [200, 193, 65]
    got = sa.align_score_batch(torch.from_numpy(s1).to(DEV), torch.tensor(l1, device=DEV), torch.from_numpy(s2).to(DEV),
                               torch.tensor(l2, device=DEV), -2, -3, 1).cpu().tolist()
    assert got == [per_oracle.align_score(s1[i, :l1[i]], s2[i, :l2[i]], -2, -3, 1) for i in range(3)]


def peaked_window(seed, chain, P=42, T=128, conf=0.9):
    """[T, P] probabilities whose frames follow `chain` (runs of random length with blanks between) at about `conf`, and the
    frame labels of the same runs, which collapse to `chain` with the silence label 0 between its members."""
    g = torch.Generator().manual_seed(seed)
    cuts = sorted(torch.randperm(T - 1, generator=g)[:2 * len(chain) - 1].add(1).tolist())
    bounds = [0] + cuts + [T]
    path = torch.empty(T, dtype=torch.long)
    labels = torch.empty(T, dtype=torch.long)
    for k in range(2 * len(chain)):
        sym = chain[k // 2]
        path[bounds[k]:bounds[k + 1]] = sym if k % 2 == 0 else P - 1
        labels[bounds[k]:bounds[k + 1]] = sym if k % 2 == 0 else 0
    logits = torch.randn(T, P, generator=g)
    logits[torch.arange(T), path] += float(np.log(conf / (1 - conf) * (P - 1)))
    return torch.softmax(logits, 1), labels


def test_getPER_equals_the_oracle_window_by_window():
    chains = [[3, 7, 3, 12], [5], [9, 9, 1, 40, 2, 17], [1, 2, 3, 4, 5, 6, 7, 8], [30, 31], [11, 4, 11], [6, 6, 6], [20, 21, 22, 23, 24]]
    windows = [peaked_window(100 + i, c) for i, c in enumerate(chains)]
    want = []
    for (probs, labels), chain in zip(windows, chains):
        collapsed = [int(x) for i, x in enumerate(labels.tolist()) if i == 0 or x != labels[i - 1]]
        assert collapsed == [x for c in chain for x in (c, 0)]
        out, tie = per_oracle.beam_search(probs.numpy(), 20, 41)
        assert not tie
        want.append(per_oracle.get_seq_PER(collapsed, out[0][1]))
    loader = [(None, torch.stack([w[1] for w in windows[i:i + 4]]).to(DEV)) for i in (0, 4)]
    probs = {id(b): torch.stack([w[0] for w in windows[i:i + 4]]).to(DEV) for b, i in zip(loader, (0, 4))}
    pers, tied = sa.window_PER(loader, lambda data: probs[id(data)], 41, nKeep=20)
    assert pers.tolist() == want and not tied.any()
    mean = 0
    for v in want:
        mean += v
    assert sa.getPER(loader, lambda data: probs[id(data)], 41, nKeep=20) == mean / 8
    assert 0 < mean / 8 < 1


def test_tool_scores_a_probe_directory(tmp_path, capsys):
    """A probe directory as linear_separability --CTC writes it, from the recorded CPC checkpoint and a seeded classifier.  A
    classifier of random weights gives near-uniform rows, whose scores underflow to 0 (all ties) within a window; its weights are
    therefore scaled by a fixed factor of 40, which makes the rows peaked.  Windows whose tie flag is set are left out of the
    comparison with the oracle: a quarter of them at most."""
    from cpc2_amd.dataset import AudioBatchData, filterSeqs, findAllSeqs, parseSeqLabels
    from cpc2_amd.eval import phone_error_rate as per
    n_keep, scale = 20, 40.0
    model, hidden_gar, _ = fl.loadModel([CKPT])
    _, n_phones = parseSeqLabels(PHONES)
    torch.manual_seed(26)
    crit = cr.CTCPhoneCriterion(hidden_gar, n_phones, False)
    with torch.no_grad():
        for p in crit.parameters():
            p.mul_(scale)
    val = tmp_path / "val.txt"
    val.write_text("2911-12359-0007\n4051-11218-0044\n")
    probe = tmp_path / "probe"
    probe.mkdir()
    (probe / "checkpoint_args.json").write_text(json.dumps(dict(
        pathDB=DB, pathTrain=str(val), pathVal=str(val), load=[CKPT], pathPhone=PHONES, CTC=True, pathCheckpoint=str(probe / "checkpoint"),
        nGPU=1, batchSizeGPU=8, n_epoch=1, debug=False, unfrozen=False, no_pretraining=False, file_extension=".flac", save_step=1,
        get_encoded=False, lr=2e-4, beta1=0.9, beta2=0.999, epsilon=2e-8, ignore_cache=False, size_window=20480)))
    fl.save_checkpoint(model.state_dict(), crit.state_dict(), {}, model.state_dict(), str(probe / "checkpoint_0.pt"))
    out = tmp_path / "per.json"
    mean = per.main([str(probe), "--nKeep", str(n_keep), "--batchSizeGPU", "4", "--debug", "--out", str(out)])
    res = json.loads(out.read_text())
    assert {"mean", "std", "windows", "nKeep", "tied_windows"} <= set(res)
    printed = capsys.readouterr().out
    assert f"Average PER {res['mean']}" in printed and f"Standard deviation PER {res['std']}" in printed
    assert res["mean"] == mean and res["nKeep"] == n_keep

    # the same loader by hand
    seqs, speakers = findAllSeqs(DB, extension=".flac")
    labels, _ = parseSeqLabels(PHONES)
    db = AudioBatchData(DB, 20480, filterSeqs(str(val), seqs), labels, len(speakers))
    loader = db.getDataLoader(4, 'sequential', False, numWorkers=0)
    model.to(DEV).eval()
    crit.to(DEV).eval()
    kept = []

    def maker(data):
        with torch.no_grad():
            probs = torch.softmax(crit.getPrediction(model(data[0][:, 0], None)[0]), dim=2)
        if len(kept) < 1:
            kept.append((probs.cpu().numpy(), data[1].cpu()))
        return probs
    pers, tied = sa.window_PER(loader, maker, crit.BLANK_LABEL, nKeep=n_keep)
    print(f"tool: {len(pers)} windows, {int(tied.sum())} tied, mean PER {res['mean']}, std {res['std']}, max prob per frame "
          f"{float(kept[0][0].max(2).mean()):.3f}, seconds {res.get('seconds')}")
    assert res["windows"] == len(pers) >= 8 and res["tied_windows"] == int(tied.sum())
    assert res["mean"] == sa.mean_std(pers)[0] and res["std"] == sa.mean_std(pers)[1]
    assert tied.sum() <= len(pers) / 4 and not tied[:4].all()
    probs, frame_labels = kept[0]
    assert probs.shape == (4, 128, n_phones + 1)
    for w in range(4):
        if tied[w]:
            continue
        lab = frame_labels[w].tolist()
        collapsed = [x for i, x in enumerate(lab) if i == 0 or x != lab[i - 1]]
        found, tie = per_oracle.beam_search(probs[w], n_keep, n_phones)
        assert not tie and pers[w] == per_oracle.get_seq_PER(collapsed, found[0][1])
