"""run_inference.py's command line without a GPU: the reference's flags, defaults and help texts (read from the
reference when it is here, otherwise from the list recorded in tests/golden/inference_vis.npz), the message when no
output is asked for, the file-naming rule, the listing and the batching."""
import argparse
import json
import os

import numpy as np
import pytest
from PIL import Image

import _inference_vis_ref as R
import run_inference as RI

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inference_vis.npz")


def reference_flags():
    if R.available():
        return [list(row) for row in R.parser_spec()]
    return json.loads(str(np.load(GOLDEN)["parser"]))


def own_flags():
    out = {}
    for a in RI.parser._actions:
        if not a.option_strings or a.option_strings[0] in ("-h", "--help"):
            continue
        action = "store_true" if isinstance(a, argparse._StoreTrueAction) else None
        default = None if action else a.default
        out[a.option_strings[0]] = [a.option_strings[0], default, action, a.help, bool(a.required)]
    return out


def test_recorded_flags_are_the_references():
    if not R.available():
        pytest.skip("the reference is not on this machine")
    assert json.loads(str(np.load(GOLDEN)["parser"])) == [list(r) for r in R.parser_spec()]


def test_flags_defaults_and_help_texts_are_the_references():
    want = reference_flags()
    assert [w[0] for w in want] == ["--output-disp", "--output-depth", "--pretrained", "--img-height", "--img-width",
                                    "--no-resize", "--dataset-list", "--dataset-dir", "--output-dir", "--img-exts",
                                    "--resnet-layers"]
    mine = own_flags()
    for row in want:
        assert mine[row[0]] == row, row[0]
    assert sorted(set(mine) - {w[0] for w in want}) == ["--batch-size"]
    assert mine["--batch-size"][1] == 1
    args = RI.parser.parse_args(["--pretrained", "x", "--resnet-layers", "18"])
    assert (args.img_height, args.img_width, args.img_exts, args.output_dir, args.dataset_dir, args.dataset_list) == \
        (256, 832, ["png", "jpg", "bmp"], "output", ".", None)
    with pytest.raises(SystemExit):
        RI.parser.parse_args(["--pretrained", "x", "--resnet-layers", "34"])
    with pytest.raises(SystemExit):
        RI.parser.parse_args(["--resnet-layers", "18"])


def test_at_least_one_output_must_be_asked_for(capsys, tmp_path):
    assert RI.main(["--pretrained", str(tmp_path / "none.pth.tar"), "--resnet-layers", "18",
                    "--output-dir", str(tmp_path / "out")]) is None
    assert capsys.readouterr().out == "You must at least output one value !\n"
    assert not (tmp_path / "out").exists()


def test_file_names_on_nested_paths(tmp_path):
    root = str(tmp_path)
    assert RI.output_stem(os.path.join(root, "0000000000.png"), root) == ("0000000000", ".png")
    assert RI.output_stem(os.path.join(root, "2011_09_26", "image_02", "data", "0000000007.jpg"), root) == \
        ("2011_09_26-image_02-data-0000000007", ".jpg")
    assert RI.output_stem(os.path.join(root, "a", "b.c", "d.e.bmp"), root + os.sep) == ("a-b.c-d.e", ".bmp")
    assert RI.output_stem(os.path.join("rel", "x", "y.png"), "rel") == ("x-y", ".png")


def _tree(tmp_path):
    (tmp_path / "sub").mkdir()
    for name, size in (("b.png", (6, 4)), ("a.png", (6, 4)), ("c.jpg", (8, 5)), ("d.bmp", (6, 4)), ("sub/e.png", (6, 4)),
                       ("notes.txt", None)):
        if size is None:
            (tmp_path / name).write_text("x")
        else:
            Image.fromarray(np.full((size[1], size[0]), 7, np.uint8)).save(tmp_path / name)  # grey frames
    return str(tmp_path)


def test_listing_is_sorted_and_a_list_keeps_its_order(tmp_path):
    root = _tree(tmp_path)
    base = ["--pretrained", "x", "--resnet-layers", "18", "--dataset-dir", root]
    names = lambda files: [os.path.relpath(f, root) for f in files]
    assert names(RI.list_files(RI.parser.parse_args(base))) == ["a.png", "b.png", "c.jpg", "d.bmp"]
    assert names(RI.list_files(RI.parser.parse_args(base + ["--img-exts", "png"]))) == ["a.png", "b.png"]
    lst = tmp_path / "list.txt"
    lst.write_text("sub/e.png\nb.png\n")
    assert names(RI.list_files(RI.parser.parse_args(base + ["--dataset-list", str(lst)]))) == ["sub/e.png", "b.png"]


def test_batches_hold_one_size_without_resize(tmp_path):
    root = _tree(tmp_path)
    base = ["--pretrained", "x", "--resnet-layers", "18", "--dataset-dir", root, "--batch-size", "3"]
    args = RI.parser.parse_args(base)
    got = list(RI.batches(RI.list_files(args), args))
    assert [[os.path.basename(f) for f, _ in b] for b in got] == [["a.png", "b.png", "c.jpg"], ["d.bmp"]]
    assert all(img.dtype == np.uint8 and img.shape[2] == 3 for b in got for _, img in b)  # grey frames become RGB
    args = RI.parser.parse_args(base + ["--no-resize"])
    got = list(RI.batches(RI.list_files(args), args))
    assert [[os.path.basename(f) for f, _ in b] for b in got] == [["a.png", "b.png"], ["c.jpg"], ["d.bmp"]]


def test_png_is_written_as_rgba_and_the_rest_as_rgb(tmp_path):
    rgba = np.random.default_rng(0).integers(0, 256, (5, 7, 4), dtype=np.uint8)
    rgba[..., 3] = 255
    RI.save_picture(str(tmp_path / "p.png"), rgba)
    back = Image.open(tmp_path / "p.png")
    assert back.mode == "RGBA" and np.array_equal(np.asarray(back), rgba)
    RI.save_picture(str(tmp_path / "p.bmp"), rgba)
    back = Image.open(tmp_path / "p.bmp")
    assert back.mode == "RGB" and np.array_equal(np.asarray(back), rgba[..., :3])
    RI.save_picture(str(tmp_path / "p.jpg"), rgba)
    assert Image.open(tmp_path / "p.jpg").size == (7, 5)
