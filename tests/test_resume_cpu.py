"""The exactness claim of train.py --resume, on the deterministic host path (the loss kernels and the one-launch Adam on
tests/hostsim, swapped in from OUTSIDE as tests/test_trainer_cpu.py does): two epochs of two steps straight against one
epoch, a state file, then fresh nets, a fresh optimiser and fresh loaders, a restore, and one more epoch.  Every
parameter, every BatchNorm buffer, every Adam moment, n_iter and the four rows of the full log are equal bit for bit, once
per optimiser.  A restore that skips the generators must NOT give the straight run: the comparison can fail."""
import os
import random

import numpy as np
import pytest
import torch


class _Run:
    def __init__(self, T, root, name, optimizer):
        self.T = T
        self.args = T.parser.parse_args(["synthetic:8:64x96", "--with-pretrain", "0", "-b", "2", "--epoch-size", "2",
                                         "--epochs", "2", "-j", "0", "--name", "t", "--print-freq", "1", "--optimizer",
                                         optimizer])
        self.args.save_path = os.path.join(root, name)
        self.args.world = 1
        os.makedirs(self.args.save_path)

    def start_logs(self):
        for log in (self.args.log_summary, self.args.log_full):
            with open(os.path.join(self.args.save_path, log), "w") as f:
                f.write("header\n")

    def fresh(self, seed):
        """nets, an optimiser and loaders as main() forms them, initialised from ``seed``"""
        import models
        from logger import TermLogger
        T, args = self.T, self.args
        torch.manual_seed(seed)
        np.random.seed(seed)
        random.seed(seed)
        train_set, _ = T.build_datasets(args)
        self.loader = torch.utils.data.DataLoader(train_set, batch_size=args.batch_size, shuffle=True, num_workers=0)
        self.disp, self.pose = models.DispResNet(18, False), models.PoseResNet(18, False)
        self.opt = T.make_optimizer(args, [{"params": [p for p in net.parameters() if p.requires_grad], "lr": args.lr}
                                           for net in (self.disp, self.pose)])
        self.logger = TermLogger(n_epochs=2, train_size=2, valid_size=1)

    def epoch(self):
        self.logger.reset_train_bar()
        loss = self.T.train(self.args, self.loader, self.disp, self.pose, self.opt, self.args.epoch_size, self.logger,
                            self.T._ScalarLog())
        assert loss == loss

    def result(self):
        sd = self.opt.state_dict()
        tensors = [p.detach().clone() for net in (self.disp, self.pose) for p in net.parameters()]
        tensors += [b.detach().clone() for net in (self.disp, self.pose) for b in net.buffers()]
        for i in sorted(sd["state"]):
            tensors += [sd["state"][i]["step"].clone(), sd["state"][i]["exp_avg"].clone(),
                        sd["state"][i]["exp_avg_sq"].clone()]
        rows = open(os.path.join(self.args.save_path, self.args.log_full)).read().split("\n")[1:]
        return tensors, sorted(sd["state"]), self.T.n_iter, rows


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8) if a.dim() else a,
                                                                     b.view(torch.uint8) if b.dim() else b)


@pytest.mark.parametrize("optimizer", ["torch", "hip"])
def test_a_resumed_run_is_the_straight_run_bit_for_bit(tmp_path, monkeypatch, optimizer):
    import _hostsim_opt
    from hostsim import harness
    from scsfm_hip import _lib, config as hip_config, ops, optim, training_state as TS
    import train as T
    from utils import save_checkpoint
    lib = harness.lib()
    monkeypatch.setattr(_lib, "get", lambda: lib)
    monkeypatch.setattr(_lib, "get_opt", _hostsim_opt.lib)
    monkeypatch.setattr(ops, "_need_cuda", lambda *a: None)
    monkeypatch.setattr(optim, "_need_cuda", lambda *a: None)
    monkeypatch.setattr(T, "device", torch.device("cpu"))
    monkeypatch.setattr(T, "best_error", -1)
    monkeypatch.chdir(tmp_path)
    hip_config.set_weight_hint(1, 0.5)

    # A: two epochs straight
    monkeypatch.setattr(T, "n_iter", 0)
    a = _Run(T, str(tmp_path), "a", optimizer)
    a.start_logs()
    a.fresh(0)
    assert type(a.opt) is (optim.Adam if optimizer == "hip" else torch.optim.Adam)
    a.epoch()
    a.epoch()
    want = a.result()
    assert want[2] == 2 and len(want[3]) == 5 and want[3][4] == ""  # (n_iter skips each epoch's last step; four rows)

    # B: one epoch, the checkpoints and the state file, as main() writes them
    monkeypatch.setattr(T, "n_iter", 0)
    b = _Run(T, str(tmp_path), "b", optimizer)
    b.start_logs()
    b.fresh(0)
    b.epoch()
    save_checkpoint(b.args.save_path, {"epoch": 1, "state_dict": b.disp.state_dict()},
                    {"epoch": 1, "state_dict": b.pose.state_dict()}, False)
    path = TS.save(T.capture_training_state(b.args, 1, b.opt), b.args.save_path)
    with open(os.path.join(b.args.save_path, b.args.log_full), "a") as f:
        f.write("a row of an epoch that was cut short\n")
    one_epoch = open(os.path.join(b.args.save_path, b.args.log_full)).read()

    def resume(generators):
        """a new process, as far as a test can tell: other initial weights, other generators, counters at nonsense"""
        with open(os.path.join(b.args.save_path, b.args.log_full), "w") as f:
            f.write(one_epoch)
        monkeypatch.setattr(T, "n_iter", 999)
        monkeypatch.setattr(T, "best_error", 123.0)
        r = _Run.__new__(_Run)
        r.T, r.args = T, b.args
        b.args.resume = b.args.save_path
        assert TS.refusal(b.args) is None
        r.fresh(4321)
        state = TS.load(path)
        TS.load_nets(b.args.save_path, state["epoch"], r.disp, r.pose, T.device)
        assert T.restore_training_state(b.args, state, r.opt, generators=generators) == 1
        assert T.n_iter == 1 and T.best_error == -1
        r.epoch()
        return r.result()

    got = resume(True)
    assert got[1] == want[1] and got[2] == want[2] and got[3] == want[3]
    assert len(got[0]) == len(want[0]) and all(_same_bits(x, y) for x, y in zip(got[0], want[0]))
    # the unused scale heads of DispResNet never had a gradient: they have no state under either optimiser
    assert len(want[1]) < len(a.opt.state_dict()["param_groups"][0]["params"]) + \
        len(a.opt.state_dict()["param_groups"][1]["params"])

    other = resume(False)
    assert other[2] == want[2] and other[3][:2] == want[3][:2]  # (the first epoch's rows are the file's)
    assert other[3] != want[3] and not all(_same_bits(x, y) for x, y in zip(other[0], want[0]))
