"""The table of a validation pass (csrc_val/scsfm_validation_table.hip, compiled unchanged against the host simulator):
scsfm_val_depth_errors_row gives the existing entry point's metrics, medians and count bit for bit and the batch's mean
as the sequential double sum divided by B; scsfm_val_losses_row is exact; scsfm_val_table_mean is logger.AverageMeter
fed the present rows in order, bit for bit; nothing is written outside the outputs; every rejected argument returns -1
and writes nothing."""
import ctypes

import numpy as np
import pytest

import _hostsim_val as S
import _validation_errors_cases as C
import validation_errors_oracle as O
from logger import AverageMeter

GUARD = 16
ROW_SENTINEL = -2468.25
NAN = float("nan")


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _row_buffer(n=1):
    return np.full(n * 8 + GUARD, ROW_SENTINEL, np.float64)


def _row_call(gt, src, dataset, is_disp, row, bufs=None, change=()):
    """scsfm_val_depth_errors_row's status for these inputs; ``change`` replaces arguments by name."""
    gt, src = np.ascontiguousarray(gt, np.float32), np.ascontiguousarray(src, np.float32)
    B, H, W = gt.shape
    h, w = src.shape[1:]
    y1, y2, x1, x2, cap = O.crop_and_cap(dataset, H, W)
    nbytes = S.lib().size("scsfm_val_workspace_bytes", B, H, W)
    ws = np.full(nbytes + 64, 0xAB, np.uint8)
    bufs = S.outputs(B) if bufs is None else bufs
    a = dict(B=B, h=h, w=w, src=_ptr(src), is_disp=int(is_disp), H=H, W=W, gt=_ptr(gt), y1=y1, y2=y2, x1=x1, x2=x2,
             min_gt=0.1, max_depth=float(cap), clamp_lo=1e-3, ws=_ptr(ws), ws_bytes=nbytes, metrics=_ptr(bufs["metrics"]),
             medians=_ptr(bufs["medians"]), count=_ptr(bufs["count"]), row=_ptr(row), stream=None)
    a.update(change)
    rc = S.lib()._fn["scsfm_val_depth_errors_row"](*a.values())
    assert (ws[nbytes:] == 0xAB).all()
    if rc != 0:
        assert (ws == 0xAB).all()
    return rc, bufs


def _sequential_mean(metrics):
    """(m[0][k] + m[1][k] + ...) / B in image order in double."""
    s = metrics[0].copy()
    for m in metrics[1:]:
        s = s + m
    return s / np.float64(len(metrics))


def _depth_errors_row(gt, src, dataset, is_disp):
    B = len(gt)
    row = _row_buffer()
    rc, bufs = _row_call(gt, src, dataset, is_disp, row)
    assert rc == 0 and S.untouched(bufs, B) and (row[8:] == ROW_SENTINEL).all()
    got = dict(metrics=bufs["metrics"][:B * 6].reshape(B, 6).copy(), medians=bufs["medians"][:B * 2].reshape(B, 2).copy(),
               count=bufs["count"][:B].copy())
    return got, row[:8].copy()


@pytest.mark.parametrize("name", ("A", "B"))
def test_depth_errors_row_is_the_existing_call_plus_the_batch_mean(name):
    gt, disp, dataset = C.CASES[name]()
    got, row = _depth_errors_row(gt, disp, dataset, True)
    want = S.depth_errors(gt, disp, dataset, is_disp=True)
    for k in want:
        assert C.same_bits(got[k], want[k]), k
    assert len(gt) == {"A": 3, "B": 2}[name] and np.isfinite(row).all()
    assert C.same_bits(row[:6], _sequential_mean(want["metrics"]))
    assert row[6] == 0.0 and not np.signbit(row[6]) and row[7] == 1.0
    # ... which is scsfm_hip.validation.batch_mean's division of the summed columns, to the rounding of a sum
    np.testing.assert_allclose(row[:6], want["metrics"].sum(0) / len(gt), rtol=4 * len(gt) * 2.0 ** -53, atol=0)


@pytest.mark.parametrize("kind", ("empty", "nan_pred"))
def test_a_nan_image_makes_the_columns_nan_and_the_row_present(kind):
    gt, src, dataset = C.edge(kind)
    got, row = _depth_errors_row(gt, src, dataset, False)
    want = S.depth_errors(gt, src, dataset)
    for k in want:
        assert C.same_bits(got[k], want[k]), k
    assert np.isnan(got["metrics"][1]).all() and np.isfinite(got["metrics"][[0, 2]]).all()
    assert np.isnan(row[:6]).all() and row[6] == 0.0 and row[7] == 1.0


def test_losses_row_is_exact():
    fn = S.lib()._fn["scsfm_val_losses_row"]
    denormal = np.float32(3e-42)
    assert 0 < denormal < np.finfo(np.float32).tiny
    for photo, smooth, geom in ((np.float32(0.1234567), np.float32(1e-3), np.float32(7.5)),
                                (np.float32(0.3), denormal, np.float32(NAN)),
                                (np.float32(NAN), np.float32(-0.0), np.float32(3.4e38))):
        scalars = [np.array([v, 99.0], np.float32) for v in (photo, smooth, geom)]
        row = _row_buffer()
        assert fn(*[_ptr(s) for s in scalars], _ptr(row), None) == 0
        want = np.array([float(photo), float(photo), float(smooth), float(geom), 0.0, 0.0, 0.0, 1.0])
        assert C.same_bits(row[:8], want) and (np.signbit(row[:8]) == np.signbit(want)).all(), (row[:8], want)
        assert (row[8:] == ROW_SENTINEL).all() and all(s[1] == 99.0 for s in scalars)


def _meter(rows):
    """logger.AverageMeter over the present rows in order -> (avg of the 7 values, count)."""
    meter = AverageMeter(i=7)
    for r in rows:
        if r[7] == 1.0:
            meter.update([float(v) for v in r[:7]])
    return np.array(meter.avg, np.float64), meter.count


def _table_mean(table):
    out = np.full(8 + GUARD, ROW_SENTINEL, np.float64)
    before = table.copy()
    assert S.lib()._fn["scsfm_val_table_mean"](len(table), _ptr(table), _ptr(out), None) == 0
    assert (out[8:] == ROW_SENTINEL).all() and C.same_bits(table, before)
    return out[:8].copy()


def test_table_mean_is_the_average_meter_over_the_present_rows():
    rng = np.random.default_rng(31)
    table = np.zeros((9, 8))
    table[:, :7] = rng.uniform(0.0, 3.0, (9, 7)) * 10.0 ** rng.integers(-3, 4, (9, 7))
    table[:, 7] = 1.0
    table[[2, 7]] = 0.0      # absent rows: as the caller zeroed them
    table[4, 1:6] = NAN      # a batch with a NaN image
    table[5, 6] = -1.5       # (the seventh column is a value like the others)
    want, count = _meter(table)
    got = _table_mean(table)
    assert count == 7 and got[7] == 7.0
    assert C.same_bits(got[:7], want)
    assert np.isnan(got[1:6]).all() and np.isfinite(got[[0, 6]]).all()
    # absent rows are skipped whatever they hold, and a mark other than 1.0 is no mark
    table[2, :7], table[7, :7] = 1e9, NAN
    table[7, 7] = 2.0
    assert C.same_bits(_table_mean(table), got)
    # the order is the contract: the rows reversed give the meter's result for that order
    back = np.ascontiguousarray(table[::-1])
    assert C.same_bits(_table_mean(back)[:7], _meter(back)[0])
    # one present row is that row
    assert C.same_bits(_table_mean(np.ascontiguousarray(table[5:6])), np.append(table[5, :7], 1.0))


def test_an_all_absent_table_gives_zeros_and_a_count_of_zero():
    got = _table_mean(np.zeros((5, 8)))
    assert C.same_bits(got, np.zeros(8)) and not np.signbit(got).any()
    assert _meter(np.zeros((5, 8)))[1] == 0 and AverageMeter(i=7).avg == [0] * 7


def test_rejected_arguments_return_minus_one_and_write_nothing():
    gt, disp, dataset = C.case_a()
    B, H, W = gt.shape
    nbytes = S.lib().size("scsfm_val_workspace_bytes", B, H, W)
    bad = [dict(row=None), dict(B=0), dict(B=-1), dict(h=0), dict(w=0), dict(H=0), dict(W=-3), dict(y1=-1), dict(y2=H + 1),
           dict(x1=-1), dict(x2=W + 1), dict(y1=36, y2=15), dict(x1=119, x2=4), dict(min_gt=80.0), dict(min_gt=90.0),
           dict(max_depth=NAN), dict(ws_bytes=nbytes - 1), dict(src=None), dict(gt=None), dict(ws=None),
           dict(metrics=None), dict(medians=None), dict(count=None)]
    for change in bad:
        row = _row_buffer()
        rc, bufs = _row_call(gt, disp, dataset, True, row, change=change)
        assert rc == -1, change
        assert S.untouched(bufs) and (row == ROW_SENTINEL).all(), change
    row = _row_buffer()  # ... and the unchanged arguments are accepted
    rc, bufs = _row_call(gt, disp, dataset, True, row)
    assert rc == 0 and S.untouched(bufs, B) and not S.untouched(bufs) and row[7] == 1.0

    fn = S.lib()._fn["scsfm_val_losses_row"]
    scalar = np.ones(1, np.float32)
    for k in range(4):
        row = _row_buffer()
        args = [_ptr(scalar), _ptr(scalar), _ptr(scalar), _ptr(row)]
        args[k] = None
        assert fn(*args, None) == -1 and (row == ROW_SENTINEL).all(), k

    fn = S.lib()._fn["scsfm_val_table_mean"]
    table = np.ones((3, 8))
    for n_rows, t, with_out in ((0, table, True), (-1, table, True), (1 << 28, table, True), ((1 << 28) + 5, table, True),
                                (3, None, True), (3, table, False)):
        out = _row_buffer()
        assert fn(n_rows, _ptr(t), _ptr(out) if with_out else None, None) == -1, (n_rows, t is None, with_out)
        assert (out == ROW_SENTINEL).all()
    out = _row_buffer()
    assert fn(3, _ptr(table), _ptr(out), None) == 0 and C.same_bits(out[:8], np.array([1.0] * 7 + [3.0]))


def test_the_simulator_carries_abi_2_and_the_new_entry_points():
    from scsfm_hip import _lib
    assert S.lib()._fn["scsfm_val_abi_version"]() == _lib.VAL_ABI_VERSION == 2
    assert {"scsfm_val_depth_errors_row", "scsfm_val_losses_row", "scsfm_val_table_mean"} <= set(S.lib().decls)
    i, p = ctypes.c_int, ctypes.c_void_p
    assert S.lib().decls["scsfm_val_table_mean"] == (i, [i, p, p, p])
    assert S.lib().decls["scsfm_val_losses_row"] == (i, [p, p, p, p, p])
    assert S.lib().decls["scsfm_val_depth_errors_row"][1] == S.lib().decls["scsfm_val_depth_errors"][1][:-1] + [p, p]
