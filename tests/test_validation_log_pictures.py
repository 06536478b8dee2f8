"""PictureLog, the stand-in for the SummaryWriters of train.py --log-output: where it writes, what a PNG decodes to, and
that the flag wires three of them up (and nothing without it).  No GPU."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import validation_log_oracle as O
from scsfm_hip import validation_log as VL


def test_round_trip_of_byte_pictures(tmp_path):
    log = VL.PictureLog(tmp_path / "valid" / "0")
    rng = np.random.default_rng(3)
    rgba = rng.integers(0, 256, (5, 7, 4), dtype=np.uint8)
    rgb = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    p4 = log.add_image("val Dispnet Output Normalized", torch.from_numpy(rgba), 3)
    p3 = log.add_image("val Input", rgb, 0)
    assert p4 == str(tmp_path / "valid" / "0" / "val_Dispnet_Output_Normalized" / "0003.png") == \
        log.path("val Dispnet Output Normalized", 3)
    assert p3 == str(tmp_path / "valid" / "0" / "val_Input" / "0000.png")
    with Image.open(p4) as im:
        assert im.mode == "RGBA" and im.size == (7, 5) and np.array_equal(np.asarray(im), rgba)
    with Image.open(p3) as im:
        assert im.mode == "RGB" and np.array_equal(np.asarray(im), rgb)
    log.add_image("val Input", rgb[::-1].copy(), 0)  # the same tag and step: overwritten
    with Image.open(p3) as im:
        assert np.array_equal(np.asarray(im), rgb[::-1])
    assert sorted(os.listdir(tmp_path / "valid" / "0")) == ["val_Dispnet_Output_Normalized", "val_Input"]
    assert log.add_image("val Depth Output", rgba, 12345).endswith(os.sep + "12345.png")


def test_float_pictures_go_through_the_byte_rule(tmp_path):
    log = VL.PictureLog(tmp_path)
    v = np.linspace(-0.25, 1.25, 4 * 6 * 9, dtype=np.float32).reshape(4, 6, 9)
    v[0, 0, 0], v[1, 1, 1], v[2, 2, 2] = np.nan, 1.0, np.float32(254.999 / 255)
    want = O.to_bytes(v).transpose(1, 2, 0)
    assert want[0, 0, 0] == 0 and want[1, 1, 1] == 255 and want[2, 2, 2] == 254
    assert want.min() == 0 and want.max() == 255 and np.array_equal(VL.to_bytes(v), O.to_bytes(v))
    with Image.open(log.add_image("floats", v, 1)) as im:
        assert im.mode == "RGBA" and np.array_equal(np.asarray(im), want)
    with Image.open(log.add_image("floats", torch.from_numpy(v[:3]), 2)) as im:
        assert im.mode == "RGB" and np.array_equal(np.asarray(im), want[..., :3])
    for bad in (np.zeros((5, 7), np.uint8), np.zeros((5, 7, 2), np.uint8), np.zeros((2, 5, 7), np.float32)):
        with pytest.raises(ValueError):
            log.add_image("bad", bad, 0)


def test_log_output_wires_up_three_picture_logs(tmp_path, monkeypatch, capsys):
    import train as T
    common = ["synthetic:8:64x96", "--with-pretrain", "0", "--name", "t"]
    args = T.parser.parse_args(common)
    args.save_path = str(tmp_path)
    assert T.make_output_writers(args) == []
    args = T.parser.parse_args(common + ["--log-output"])
    args.save_path = str(tmp_path)
    writers = T.make_output_writers(args)
    assert len(writers) == 3 and all(isinstance(w, VL.PictureLog) for w in writers)
    assert [w.directory for w in writers] == [os.path.join(str(tmp_path), "valid", str(i)) for i in range(3)]
    assert not os.path.exists(tmp_path / "valid")  # nothing is created before a picture is written

    # the validation pass of main() hands them to whichever loop runs, with the epoch
    seen = []
    monkeypatch.setattr(T, "validate_with_gt", lambda a, loader, d, epoch, logger, w=(): seen.append(("gt", d, epoch, w))
                        or ([0.0] * 6, ["gt"]))
    monkeypatch.setattr(T, "validate_without_gt", lambda a, loader, d, p, epoch, logger, w=():
                        seen.append(("no_gt", d, p, epoch, w)) or ([0.0] * 4, ["no_gt"]))
    assert T.validate(args, "loader", "disp", "pose", 4, "logger", writers) == ([0.0] * 4, ["no_gt"])
    args.with_gt = True
    assert T.validate(args, "loader", "disp", "pose", 5, "logger", writers) == ([0.0] * 6, ["gt"])
    assert seen == [("no_gt", "disp", "pose", 4, writers), ("gt", "disp", 5, writers)]
    assert seen[0][-1] is writers and seen[1][-1] is writers

    # the scalar stand-in still drops what it is given, and its notice no longer says that images are not written
    monkeypatch.setattr(T._ScalarLog, "_announced", False)
    log = T._ScalarLog()
    log.add_scalar("loss", 1.0, 0)
    log.add_image("tag", None, 0)
    notice = capsys.readouterr().out
    assert notice.count("\n") == 1 and "images" not in notice
