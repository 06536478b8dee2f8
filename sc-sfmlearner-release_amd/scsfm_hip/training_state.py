"""What train.py --save-state writes beside the four checkpoint files, and --resume reads: the part of a run's state that
the checkpoints' ``{'epoch', 'state_dict'}`` do not hold.

``<save_path>/train_state.pth.tar`` is one ``torch.save`` of a dict:

    version        1
    epoch          the NEXT epoch (the number of epochs completed)
    n_iter         train.py's global step counter
    best_error     the best decisive validation error so far
    optimizer      optimizer.state_dict() (torch.optim.Adam's layout, under either optimiser)
    log_rows       {'summary': n, 'full': n}: the data rows of the two TSV logs (the header not counted)
    rng            {'python', 'numpy', 'torch', 'device'}: random.getstate(), numpy's global generator, torch's CPU
                   generator and the generator of the device the run trains on (None without one)
    args           the arguments that decide whether a command line continues THIS run (``COMPATIBILITY``)

The file is written under a temporary name and moved into place, so a kill during the write leaves the previous state.
It is written after the epoch's checkpoints; ``load_nets`` therefore refuses checkpoints whose epoch is not the state's
(a kill between the two writes).

With the generators restored, a resumed run at world size 1 draws what the straight run drew from there on: the data
order, the augmentations, dropout-free nets.  Ranks other than 0 of a data-parallel run have no saved generators (rank 0
alone writes) and no saved BatchNorm statistics: they are reseeded from the seed, the epoch and the rank and continue with
rank 0's statistics.
"""
from __future__ import annotations

import os
import random

import numpy as np
import torch

VERSION = 1
STATE_FILE = "train_state.pth.tar"
CHECKPOINTS = ("dispnet_checkpoint.pth.tar", "exp_pose_checkpoint.pth.tar")
COMPATIBILITY = ("resnet_layers", "sequence_length", "num_scales", "optimizer", "freeze_bn", "seed", "batch_size")


def locate(path):
    """``path``: a run directory or its state file -> (the directory, the state file)"""
    if os.path.isdir(path):
        return path, os.path.join(path, STATE_FILE)
    return os.path.dirname(path) or ".", path


def log_rows(path):
    """the data rows of a TSV log: its lines without the header"""
    with open(path) as f:
        return max(sum(1 for _ in f) - 1, 0)


def truncate_log(path, rows):
    """Keep the header and the first ``rows`` data rows of a TSV log (the rows of an epoch that was cut short go)."""
    with open(path) as f:
        lines = f.readlines()
    if len(lines) < rows + 1:
        raise ValueError("{} has {} data rows, the saved state counted {}".format(path, max(len(lines) - 1, 0), rows))
    with open(path + ".tmp", "w") as f:
        f.writelines(lines[:rows + 1])
    os.replace(path + ".tmp", path)


def capture(args, next_epoch, n_iter, best_error, optimizer, device):
    """-> the dict described above, of a run that has completed ``next_epoch`` epochs"""
    cuda = device is not None and torch.device(device).type == "cuda"
    return {
        "version": VERSION,
        "epoch": int(next_epoch),
        "n_iter": int(n_iter),
        "best_error": float(best_error),
        "optimizer": optimizer.state_dict(),
        "log_rows": {"summary": log_rows(os.path.join(args.save_path, args.log_summary)),
                     "full": log_rows(os.path.join(args.save_path, args.log_full))},
        "rng": {"python": random.getstate(), "numpy": np.random.get_state(), "torch": torch.get_rng_state(),
                "device": torch.cuda.get_rng_state(device) if cuda else None},
        "args": {name: getattr(args, name) for name in COMPATIBILITY},
    }


def save(state, directory):
    """Atomically: a failure or a kill during the write leaves the file that was there.  -> the file's path"""
    path = os.path.join(directory, STATE_FILE)
    tmp = path + ".tmp"
    try:
        torch.save(state, tmp)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.unlink(tmp)
    return path


def load(path):
    """The state of a run directory or a state file, on the host (no device is touched)."""
    state = torch.load(locate(path)[1], map_location="cpu", weights_only=False)
    if not isinstance(state, dict) or state.get("version") != VERSION:
        raise ValueError("{} is not a training state of version {}".format(path, VERSION))
    return state


def refusal(args):
    """Why ``args`` (with ``args.resume`` set) cannot continue the run it names, or None.  Reads the state file on the
    host; touches no device and no data set."""
    if args.pretrained_disp or args.pretrained_pose:
        return "--resume takes both nets from the run's checkpoints: it cannot be combined with --pretrained-disp / " \
               "--pretrained-pose"
    directory, path = locate(args.resume)
    if not os.path.isfile(path):
        return "--resume: there is no state file {} (a run writes one with --save-state)".format(path)
    missing = [name for name in CHECKPOINTS if not os.path.isfile(os.path.join(directory, name))]
    if missing:
        return "--resume: {} lacks {}".format(directory, " and ".join(missing))
    try:
        state = load(path)
    except Exception as e:  # noqa: BLE001  (whatever makes the file unreadable is the reason)
        return "--resume: cannot read {}: {}".format(path, e)
    for name in COMPATIBILITY:
        if state["args"].get(name) != getattr(args, name):
            return "--resume: the run was started with {} {}, this command line says {}".format(
                name, state["args"].get(name), getattr(args, name))
    if state["epoch"] >= args.epochs:
        return "--resume: the run has completed {} epochs, --epochs {} leaves nothing to do".format(state["epoch"],
                                                                                                   args.epochs)
    return None


def load_nets(directory, epoch, disp_net, pose_net, device):
    """Both nets from the run's checkpoints, strictly; the checkpoints must be those of the state's epoch."""
    for name, net in zip(CHECKPOINTS, (disp_net, pose_net)):
        ckpt = torch.load(os.path.join(directory, name), map_location=device)
        if ckpt["epoch"] != epoch:
            raise SystemExit("--resume: {} is of epoch {}, the state file of epoch {} (the run was killed between the two "
                             "writes): nothing to continue from".format(name, ckpt["epoch"], epoch))
        net.load_state_dict(ckpt["state_dict"], strict=True)


def reseed(seed, epoch, rank):
    """The generators of a rank that has no saved ones: from the seed, the epoch and the rank."""
    s = (int(seed) + 1000003 * int(epoch) + 7919 * int(rank)) % (2 ** 31)
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)  # (the device generators too)


def restore(state, args, optimizer, device, rank=0, world=1, generators=True):
    """The optimiser's state, the logs' lengths (rank 0) and the generators -> (the epoch to start at, n_iter,
    best_error).  ``generators=False`` leaves the generators as they are (tests: a resume that is not exact)."""
    optimizer.load_state_dict(state["optimizer"])
    if rank == 0:
        truncate_log(os.path.join(args.save_path, args.log_summary), state["log_rows"]["summary"])
        truncate_log(os.path.join(args.save_path, args.log_full), state["log_rows"]["full"])
    if generators:
        if rank == 0:
            rng = state["rng"]
            random.setstate(rng["python"])
            np.random.set_state(rng["numpy"])
            torch.set_rng_state(rng["torch"])
            if rng["device"] is not None and device is not None and torch.device(device).type == "cuda":
                torch.cuda.set_rng_state(rng["device"], device)
        else:
            reseed(args.seed, state["epoch"], rank)
    return state["epoch"], state["n_iter"], state["best_error"]
