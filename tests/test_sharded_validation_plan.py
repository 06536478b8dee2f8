"""Who validates which batch under train.py --shard-validation (no compiler, no device): scsfm_hip.validation.owner gives
every global batch exactly one rank, rank 0 the pinned ones, the others in turn; OwnedBatches yields, over all ranks,
exactly the batches the unsharded, unshuffled DataLoader forms, each once and none padded; train.py knows the flag; and
for the length of a sharded pass every rank holds rank 0's BatchNorm statistics (two processes on the host, gloo)."""
import socket

import pytest
import torch
import torch.multiprocessing as mp
from torch.utils.data import DataLoader

import _sharded_validation_ranks as R
from scsfm_hip.validation import OwnedBatches, owner

WORLDS = (1, 2, 3, 8)


@pytest.mark.parametrize("pinned", (0, 3))
@pytest.mark.parametrize("world", WORLDS)
def test_every_batch_has_one_owner_and_the_loads_are_even(world, pinned):
    for n in range(21):
        owners = [owner(i, world, pinned) for i in range(n)]
        assert all(isinstance(r, int) and 0 <= r < world for r in owners)
        assert owners[:pinned] == [0] * min(pinned, n)
        rest = owners[pinned:]
        loads = [rest.count(r) for r in range(world)]
        assert sum(loads) == max(n - pinned, 0) and max(loads) - min(loads) <= 1, (n, loads)
        # OwnedBatches deals by the same rule: every batch to exactly one rank, in ascending order
        per_rank = [OwnedBatches(n * 4, 4, r, world, pinned).indices for r in range(world)]
        assert sorted(i for idx in per_rank for i in idx) == list(range(n))
        for r, idx in enumerate(per_rank):
            assert idx == sorted(idx) == [i for i in range(n) if owners[i] == r]


@pytest.mark.parametrize("pinned", (0, 3))
@pytest.mark.parametrize("world", WORLDS)
def test_the_ranks_batches_are_the_unsharded_loaders(world, pinned):
    want = [b.tolist() for b in DataLoader(range(11), batch_size=4)]
    assert want == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10]]
    got = {}
    for rank in range(world):
        owned = OwnedBatches(11, 4, rank, world, pinned)
        assert owned.n_batches == 3 and len(owned) == len(owned.indices) == len(list(owned))
        through_loader = [b.tolist() for b in DataLoader(range(11), batch_sampler=owned)]
        assert through_loader == list(owned)
        for i, batch in zip(owned.indices, owned):
            assert i not in got  # each once
            got[i] = batch
    assert [got[i] for i in sorted(got)] == want  # no padding, no sample twice, the short last batch as it is


def test_owned_batches_of_nothing_and_bad_arguments():
    assert OwnedBatches(0, 4, 0, 2).indices == [] and list(OwnedBatches(0, 4, 1, 2)) == []
    assert OwnedBatches(3, 4, 1, 2).indices == [] and list(OwnedBatches(3, 4, 0, 2)) == [[0, 1, 2]]
    for bad in ((8, 0, 0, 1), (8, 4, 2, 2), (8, 4, -1, 2), (8, 4, 0, 0), (-1, 4, 0, 1)):
        with pytest.raises(ValueError):
            OwnedBatches(*bad)


def test_the_table_refuses_the_host():
    from scsfm_hip.validation import ValidationTable
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ValidationTable(4, torch.device("cpu"))


def test_train_py_knows_the_flag_and_leaves_it_off():
    import train as T
    base = ["data", "--name", "x"]
    assert T.parser.parse_args(base).shard_validation is False
    assert T.parser.parse_args(base + ["--shard-validation"]).shard_validation is True
    (action,) = [a for a in T.parser._actions if "--shard-validation" in a.option_strings]
    assert action.help and "\n" not in action.help
    # without the flag the loops average on the host over every batch of the loader, as before
    indices, table = T.validation_plan(T.parser.parse_args(base), [0, 1, 2])
    assert list(indices) == [0, 1, 2] and table is None


def test_every_rank_validates_with_rank_0s_statistics_and_gets_its_own_back():
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=R.statistics_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = dict(q.get(timeout=300) for _ in range(2))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for rank in (0, 1):
        own = [[10.0 * k + rank + 1, 100 * k + rank + 5] for k in range(2)]
        assert results[rank]["before"] == results[rank]["after"] == results[rank]["single"] == own
        assert results[rank]["inside"] == [[1.0, 5], [11.0, 105]]  # rank 0's, on both
