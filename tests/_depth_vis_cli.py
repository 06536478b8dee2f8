"""A generated evaluation set on disk for eval_depth.py's visualisation tests: predictions, ground truth, photographs."""
import os

import numpy as np
from PIL import Image

import _depth_vis_cases as C


def write_set(root, dataset, gdt=np.float32, pdt=np.float32, skip=True, n_photos=None):
    """-> dict(argv, gts, pred, photos, sizes): ``sizes`` of the pictures, in picture order."""
    gts, pred = C.eval_set(dataset, gdt, pdt, skip=skip)
    os.makedirs(os.path.join(root, "img"), exist_ok=True)
    np.save(os.path.join(root, "pred.npy"), pred)
    if dataset == "kitti":
        os.makedirs(os.path.join(root, "gt"), exist_ok=True)
        for i, g in enumerate(gts):
            np.save(os.path.join(root, "gt", f"{i:06d}.npy"), g)
        gt_path = os.path.join(root, "gt")
    else:
        gt_path = os.path.join(root, "gt.npy")
        np.save(gt_path, gts)
    ev = [i for i in range(len(pred)) if pred[i].mean() != -1]
    sizes = [tuple(gts[i].shape) for i in ev]
    photos = C.photos(sizes if n_photos is None else sizes[:n_photos])
    for k, p in enumerate(photos):
        img = p[..., 0] if k == 1 else p  # the second photograph is a grey file
        if k == 1:
            photos[k] = np.repeat(img[..., None], 3, axis=2)
        Image.fromarray(img).save(os.path.join(root, "img", f"{k:010d}.png"))
    open(os.path.join(root, "img", "notes.txt"), "w").write("not a picture")
    argv = ["--dataset", dataset, "--pred_depth", os.path.join(root, "pred.npy"), "--gt_depth", gt_path]
    return dict(argv=argv, gts=gts, pred=pred, photos=photos, sizes=sizes, img=os.path.join(root, "img"))


def read_pictures(folder):
    names = sorted(os.listdir(folder))
    out = []
    for n in names:
        im = Image.open(os.path.join(folder, n))
        assert im.mode == "RGB"
        out.append(np.asarray(im))
    return names, out
