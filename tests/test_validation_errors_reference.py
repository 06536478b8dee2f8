"""The validation-error oracle (tests/validation_errors_oracle.py) pinned on the CPU: against the reference's own
compute_errors where the reference checkout is on this machine, and against the committed tests/golden/misc.npz
``errors/*`` entries (which oracle/make_golden.py recorded from it).  The oracle sums in float64 where the reference
takes fp32 means: that is the only difference, hence the existing golden test's rtol=1e-5, atol=1e-6."""
import ast
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _validation_errors_cases as C
import validation_errors_oracle as O

REFERENCE = os.environ.get("SCSFM_REFERENCE", "/root/reference")
LOSS_FUNCTIONS = os.path.join(REFERENCE, "loss_functions.py")


def _reference_compute_errors():
    """The reference's compute_errors alone, pulled out of its source (the module's other imports are not needed)."""
    tree = ast.parse(open(LOSS_FUNCTIONS).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "compute_errors"]
    ns = dict(torch=torch)
    exec(compile(ast.Module(body=keep, type_ignores=[]), LOSS_FUNCTIONS, "exec"), ns)
    return ns["compute_errors"]


@pytest.mark.skipif(not os.path.isfile(LOSS_FUNCTIONS), reason="the reference checkout is not on this machine")
@pytest.mark.parametrize("name", sorted(C.CASES))
def test_oracle_reproduces_the_reference(name):
    """validate_with_gt's sequence -- 1 / disp, F.interpolate to the ground truth's size, compute_errors -- on the
    cases of the kernel tests."""
    gt, disp, dataset = C.CASES[name]()
    depth = 1 / torch.tensor(disp)
    if depth.shape != gt.shape:
        depth = F.interpolate(depth.unsqueeze(1), list(gt.shape[1:])).squeeze(1)
    want = _reference_compute_errors()(torch.tensor(gt), depth, dataset)
    got = O.batch_mean(C.expected(name))
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("dataset", ("kitti", "nyu"))
def test_oracle_reproduces_the_goldens(dataset, golden_dir):
    gold = np.load(os.path.join(golden_dir, "misc.npz"))
    got = O.batch_mean(O.depth_errors(gold[f"errors/{dataset}/gt"], gold[f"errors/{dataset}/pred"], dataset))
    np.testing.assert_allclose(got, gold[f"errors/{dataset}/out"], rtol=1e-5, atol=1e-6)
