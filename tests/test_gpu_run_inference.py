"""run_inference.py end to end on the GPU with a seeded random DispResNet: every picture written equals the oracle
(tests/inference_vis_oracle.py) applied to the disparity the network gave for that file."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import inference_vis_oracle as O
import run_inference as RI

pytestmark = pytest.mark.gpu
H, W = 64, 96


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """A checkpoint and a nested folder of three 64 x 96 PNGs (one of them grey) and one 70 x 100 JPEG."""
    import models
    root = tmp_path_factory.mktemp("inference")
    torch.manual_seed(0)
    net = models.DispResNet(18, False)
    ckpt = str(root / "dispnet_model_best.pth.tar")
    torch.save({"state_dict": net.state_dict()}, ckpt)
    data = root / "data"
    (data / "drive" / "image_02").mkdir(parents=True)
    rng = np.random.default_rng(0)
    rel = []
    for i in range(3):
        img = rng.integers(0, 256, (H, W) if i == 1 else (H, W, 3), dtype=np.uint8)
        rel.append(os.path.join("drive", "image_02", f"{i:010d}.png"))
        Image.fromarray(img).save(data / rel[-1])
    smooth = np.clip(np.add.outer(np.arange(70) * 3, np.arange(100) * 2)[..., None] + np.array([0, 20, 40]), 0, 255)
    rel.append(os.path.join("drive", "image_02", "0000000003.jpg"))
    Image.fromarray(smooth.astype(np.uint8)).save(data / rel[-1])
    lst = root / "list.txt"
    lst.write_text("\n".join(rel) + "\n")
    return dict(root=root, ckpt=ckpt, data=str(data), folder=str(data / "drive" / "image_02"), rel=rel, lst=str(lst))


def run(work, out, *extra):
    seen = {}

    def on_batch(files, disp):
        assert disp.dim() == 4 and disp.shape[1] == 1 and len(files) == len(disp)
        for f, d in zip(files, disp.cpu().numpy()):
            seen[f] = d[0]

    RI.main(["--pretrained", work["ckpt"], "--resnet-layers", "18", "--img-height", str(H), "--img-width", str(W),
             "--output-dir", out, *extra], on_batch=on_batch)
    return seen


def judge(work, out, seen, dataset_dir, kinds=("disp", "depth")):
    for file, disp in seen.items():
        name, ext = RI.output_stem(file, dataset_dir)
        want = dict(zip(("disp", "depth"), O.disparity_and_depth(disp[None])))
        for kind in ("disp", "depth"):
            path = os.path.join(out, f"{name}_{kind}{ext}")
            assert os.path.exists(path) == (kind in kinds), path
            if kind not in kinds:
                continue
            pic = Image.open(path)
            assert pic.size == (disp.shape[1], disp.shape[0])
            if ext == ".png":
                got = np.asarray(pic)
                assert pic.mode == "RGBA" and (got[..., 3] == 255).all()
                assert np.array_equal(got, want[kind][0]), path
            else:
                assert pic.mode == "RGB"


def test_both_pictures_of_a_folder(work, tmp_path, capsys):
    out = str(tmp_path / "out")
    seen = run(work, out, "--dataset-dir", work["folder"], "--batch-size", "2", "--output-disp", "--output-depth")
    assert "4 files to test" in capsys.readouterr().out
    assert sorted(os.path.basename(f) for f in seen) == [f"{i:010d}.png" for i in range(3)] + ["0000000003.jpg"]
    assert all(d.shape == (H, W) and np.isfinite(d).all() and (d > 0).all() for d in seen.values())
    judge(work, out, seen, work["folder"])
    assert sorted(os.listdir(out)) == sorted(f"{i:010d}_{k}.png" for i in range(3) for k in ("disp", "depth")) + \
        ["0000000003_depth.jpg", "0000000003_disp.jpg"]


def test_dataset_list_names_nested_files(work, tmp_path):
    out = str(tmp_path / "out")
    seen = run(work, out, "--dataset-dir", work["data"], "--dataset-list", work["lst"], "--batch-size", "2",
               "--output-depth")
    assert list(seen) == [os.path.join(work["data"], r) for r in work["rel"]]  # the list's order
    judge(work, out, seen, work["data"], kinds=("depth",))
    assert "drive-image_02-0000000000_depth.png" in os.listdir(out) and len(os.listdir(out)) == 4


def test_no_resize(work, tmp_path):
    out = str(tmp_path / "out")
    seen = run(work, out, "--dataset-dir", work["folder"], "--img-exts", "png", "--no-resize", "--batch-size", "2",
               "--img-height", "32", "--img-width", "32", "--output-disp")
    assert len(seen) == 3 and all(d.shape == (H, W) for d in seen.values())  # the frames' own size, not 32 x 32
    judge(work, out, seen, work["folder"], kinds=("disp",))
