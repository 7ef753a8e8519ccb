"""Linear separability of CPC features -- cpc/eval/linear_separability.py of the reference: a linear classifier trained on
frozen (or, with --unfrozen, fine-tuned) features, for speakers (the default), frame-aligned phones (--pathPhone) or phones
under a CTC loss (--pathPhone --CTC).  Same command line, defaults, log lines and output files (checkpoint_args.json,
checkpoint_logs.json, checkpoint_{epoch}.pt = {gEncoder, cpcCriterion, optimizer, best}), quirks included:

    python -m cpc2_amd.eval.linear_separability pathDB pathTrain pathVal CKPT [--pathPhone F] [--CTC] [--unfrozen] ...

One GPU per process: --batchSizeGPU is the whole batch and --nGPU -1 resolves to 1; a larger --nGPU is refused before any work
(the reference's DataParallel sums per-replica mean losses, so its gradient grows with the device count).  Losses and accuracies
stay on the device during an epoch and come to the host once per epoch.  --ignore_cache is accepted and has no effect (there is
no sequence cache here).
"""
import argparse
import json
import sys
import time
from copy import deepcopy
from pathlib import Path

import numpy as np
import torch

from .. import criterion as cr
from .. import feature_loader as fl
from ..dataset import AudioBatchData, filterSeqs, findAllSeqs, parseSeqLabels
from ..train import FlatAdam, backward, show_logs, save_logs, sum_losses, update_logs


def _epoch_logs(losses, accs, prefix):
    """The reference's per-step `logs[key] += np.asarray([x.mean().item()])`, from the device values of the whole epoch (one
    copy to the host) summed in the same order in float64."""
    out = {f"locLoss_{prefix}": 0, f"locAcc_{prefix}": 0}
    if losses:
        lv = torch.stack([x.mean().double() for x in losses]).cpu().numpy()
        av = torch.stack([x.mean().double() for x in accs]).cpu().numpy()
        for a, b in zip(lv, av):
            out[f"locLoss_{prefix}"] += np.asarray([float(a)])
            out[f"locAcc_{prefix}"] += np.asarray([float(b)])
    return out


def train_step(feature_maker, criterion, data_loader, optimizer):
    if feature_maker.optimize:
        feature_maker.train()
    criterion.train()
    losses, accs = [], []
    for step, fulldata in enumerate(data_loader):
        optimizer.zero_grad()
        batch_data, label = fulldata
        batch_data = batch_data[:, 0]
        if feature_maker.optimize:
            c_feature, encoded_data, _ = feature_maker(batch_data, None)
        else:
            with torch.no_grad():
                c_feature, encoded_data, _ = feature_maker(batch_data, None)
        all_losses, all_acc = criterion(c_feature, encoded_data, label)
        backward(sum_losses(all_losses))
        optimizer.step()
        losses.append(all_losses.detach())
        accs.append(all_acc)
    logs = update_logs(_epoch_logs(losses, accs, "train"), step)
    logs["iter"] = step
    return logs


def val_step(feature_maker, criterion, data_loader):
    feature_maker.eval()
    criterion.eval()
    losses, accs = [], []
    for step, fulldata in enumerate(data_loader):
        with torch.no_grad():
            batch_data, label = fulldata
            batch_data = batch_data[:, 0]
            c_feature, encoded_data, _ = feature_maker(batch_data, None)
            all_losses, all_acc = criterion(c_feature, encoded_data, label)
            losses.append(all_losses)
            accs.append(all_acc)
    return update_logs(_epoch_logs(losses, accs, "val"), step)


def run(feature_maker, criterion, train_loader, val_loader, optimizer, logs, n_epochs, path_checkpoint):
    start_epoch = len(logs["epoch"])
    best_acc = -1
    start_time = time.time()
    for epoch in range(start_epoch, n_epochs):
        logs_train = train_step(feature_maker, criterion, train_loader, optimizer)
        logs_val = val_step(feature_maker, criterion, val_loader)
        print('')
        print('_' * 50)
        print(f'Ran {epoch + 1} epochs '
              f'in {time.time() - start_time:.2f} seconds')
        show_logs("Training loss", logs_train)
        show_logs("Validation loss", logs_val)
        print('_' * 50)
        print('')

        if logs_val["locAcc_val"] > best_acc:
            # (the feature maker's state, not the classifier's: linear_separability.py:98-99)
            best_state = deepcopy(fl.get_module(feature_maker).state_dict())
            best_acc = logs_val["locAcc_val"]

        logs["epoch"].append(epoch)
        for key, value in dict(logs_train, **logs_val).items():
            if key not in logs:
                logs[key] = [None for x in range(epoch)]
            if isinstance(value, np.ndarray):
                value = value.tolist()
            logs[key].append(value)

        if (epoch % logs["saveStep"] == 0 and epoch > 0) or epoch == n_epochs - 1:
            model_state_dict = fl.get_module(feature_maker).state_dict()
            criterion_state_dict = fl.get_module(criterion).state_dict()
            fl.save_checkpoint(model_state_dict, criterion_state_dict, optimizer.state_dict(), best_state,
                               f"{path_checkpoint}_{epoch}.pt")
            save_logs(logs, f"{path_checkpoint}_logs.json")


def parse_args(argv):
    parser = argparse.ArgumentParser(description='Linear separability trainer'
                                     ' (default test in speaker separability)')
    parser.add_argument('pathDB', type=str, help="Path to the directory containing the audio data.")
    parser.add_argument('pathTrain', type=str, help="Path to the list of the training sequences.")
    parser.add_argument('pathVal', type=str, help="Path to the list of the test sequences.")
    parser.add_argument('load', type=str, nargs='*', help="Path to the checkpoint to evaluate.")
    parser.add_argument('--pathPhone', type=str, default=None,
                        help="Path to the phone labels. If given, will compute the phone separability.")
    parser.add_argument('--CTC', action='store_true', help="Use the CTC loss (for phone separability only)")
    parser.add_argument('--pathCheckpoint', type=str, default='out',
                        help="Path of the output directory where the checkpoints should be dumped.")
    parser.add_argument('--nGPU', type=int, default=-1,
                        help='Number of GPUs. Default=-1, one; this package runs on one GPU per process.')
    parser.add_argument('--batchSizeGPU', type=int, default=8,
                        help='Batch size (one GPU per process: the whole batch).')
    parser.add_argument('--n_epoch', type=int, default=10)
    parser.add_argument('--debug', action='store_true', help='If activated, will load only a small number of audio data.')
    parser.add_argument('--unfrozen', action='store_true',
                        help="If activated, update the feature network as well as the linear classifier")
    parser.add_argument('--no_pretraining', action='store_true', help="If activated, work from an untrained model.")
    parser.add_argument('--file_extension', type=str, default=".flac", help="Extension of the audio files in pathDB.")
    parser.add_argument('--save_step', type=int, default=-1,
                        help="Frequency at which a checkpoint should be saved, et to -1 (default) to save only the best "
                             "checkpoint.")
    parser.add_argument('--get_encoded', action='store_true',
                        help="If activated, will work with the output of the convolutional encoder (see CPC's "
                             "architecture).")
    parser.add_argument('--lr', type=float, default=2e-4, help='Learning rate.')
    parser.add_argument('--beta1', type=float, default=0.9, help='Value of beta1 for the Adam optimizer.')
    parser.add_argument('--beta2', type=float, default=0.999, help='Value of beta2 for the Adam optimizer.')
    parser.add_argument('--epsilon', type=float, default=2e-8, help='Value of epsilon for the Adam optimizer.')
    parser.add_argument('--ignore_cache', action='store_true',
                        help="Activate if the sequences in pathDB have changed (no effect: there is no cache).")
    parser.add_argument('--size_window', type=int, default=20480, help="Number of frames to consider in each batch.")
    args = parser.parse_args(argv)
    if args.nGPU < 0:
        args.nGPU = 1
    if args.save_step <= 0:
        args.save_step = args.n_epoch

    args.load = [str(Path(x).resolve()) for x in args.load]
    args.pathCheckpoint = str(Path(args.pathCheckpoint).resolve())
    return args


def refuse_unsupported(args):
    """What this package does not do, refused before any work."""
    if args.nGPU > 1:
        raise SystemExit(f"--nGPU {args.nGPU}: this package runs one GPU per process (--batchSizeGPU is the whole batch). "
                         "The reference's DataParallel sums one mean loss per device, so its gradient grows with the device "
                         "count; run with --nGPU 1.")
    if len(args.load) != 1:
        raise SystemExit(f"{len(args.load)} checkpoints given: exactly one is supported (the reference's ConcatenatedModel "
                         "of several is not part of this package).")
    if args.pathPhone is not None and args.CTC and args.get_encoded:
        raise ValueError("On encoder version not implemented yet")


def main(argv):
    args = parse_args(argv)
    refuse_unsupported(args)
    logs = {"epoch": [], "iter": [], "saveStep": args.save_step}

    seqNames, speakers = findAllSeqs(args.pathDB, extension=args.file_extension)

    model, hidden_gar, hidden_encoder = fl.loadModel(args.load, loadStateDict=not args.no_pretraining)
    model.cuda()

    dim_features = hidden_encoder if args.get_encoded else hidden_gar

    # Now the criterion
    phone_labels = None
    if args.pathPhone is not None:
        phone_labels, n_phones = parseSeqLabels(args.pathPhone)
        if not args.CTC:
            print("Running phone separability with aligned phones")
            criterion = cr.PhoneCriterion(dim_features, n_phones, args.get_encoded)
        else:
            print("Running phone separability with CTC loss")
            criterion = cr.CTCPhoneCriterion(dim_features, n_phones, args.get_encoded)
    else:
        print("Running speaker separability")
        # (sized like the reference: hidden_encoder with --get_encoded, although it always reads cFeature)
        criterion = cr.SpeakerCriterion(dim_features, len(speakers))
    criterion.cuda()

    # Dataset
    seq_train = filterSeqs(args.pathTrain, seqNames)
    seq_val = filterSeqs(args.pathVal, seqNames)

    if args.debug:
        seq_train = seq_train[:1000]
        seq_val = seq_val[:100]

    db_train = AudioBatchData(args.pathDB, args.size_window, seq_train, phone_labels, len(speakers))
    db_val = AudioBatchData(args.pathDB, args.size_window, seq_val, phone_labels, len(speakers))

    batch_size = args.batchSizeGPU * args.nGPU

    train_loader = db_train.getDataLoader(batch_size, "uniform", True, numWorkers=0)
    val_loader = db_val.getDataLoader(batch_size, 'sequential', False, numWorkers=0)

    # Optimizer: the criterion's parameters first, then (fine-tuning) the model's
    g_params = list(criterion.parameters())
    model.optimize = False
    model.eval()
    if args.unfrozen:
        print("Working in full fine-tune mode")
        g_params += list(model.parameters())
        model.optimize = True
    else:
        print("Working with frozen features")
        for g in model.parameters():
            g.requires_grad = False

    optimizer = FlatAdam(g_params, lr=args.lr, betas=(args.beta1, args.beta2), eps=args.epsilon)

    # Checkpoint directory
    args.pathCheckpoint = Path(args.pathCheckpoint)
    args.pathCheckpoint.mkdir(exist_ok=True)
    args.pathCheckpoint = str(args.pathCheckpoint / "checkpoint")

    with open(f"{args.pathCheckpoint}_args.json", 'w') as file:
        json.dump(vars(args), file, indent=2)

    run(model, criterion, train_loader, val_loader, optimizer, logs, args.n_epoch, args.pathCheckpoint)


if __name__ == "__main__":
    main(sys.argv[1:])
