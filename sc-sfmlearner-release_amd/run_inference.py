"""Runs DispResNet over a folder (or list) of images and writes the bone-coloured disparity pictures and the
rainbow-coloured depth pictures -- the reference's run_inference.py (same flags, messages, file names and bytes), plus
--batch-size.

    python run_inference.py --pretrained checkpoints/dispnet_model_best.pth.tar --resnet-layers 18 \
        --dataset-dir kitti_raw/2011_09_26/2011_09_26_drive_0005_sync/image_02/data --output-dir pictures \
        --output-disp --output-depth

Per batch: the frames are decoded on the host with PIL, uploaded as bytes, resized on the device
(scsfm_hip.prepare.resize_u8) when their size differs and --no-resize is off, normalised
(scsfm_hip.visualise.normalise_u8), run through the network, coloured (scsfm_hip.visualise.colourise, once per picture
kind) and copied back once per picture kind.  An output is named after the input's path relative to --dataset-dir, its
components joined by '-', then _disp or _depth and the input's own extension.

Deliberate departures from the reference:
  - the files of a folder are processed in sorted order (a --dataset-list keeps its own order);
  - grey images are accepted (PIL's convert("RGB"));
  - the resize is Pillow's bilinear on the bytes, which is what scipy.misc.imresize did for a frame whose values span
    0 ... 255; its contrast stretch of other frames is not reproduced;
  - .png outputs are RGBA as the reference's are; every other extension is written as RGB, because Pillow refuses RGBA
    JPEG and reads an RGBA BMP back as RGB;
  - a name never starts with '-' (path.py's splitall() puts an empty component in front of a relative path);
  - with --no-resize a batch holds only frames of one size;
  - the script needs a HIP device and says so, as test_disp.py does.
"""
import argparse
import glob
import os

import numpy as np
import torch

parser = argparse.ArgumentParser(description='Inference script for DispNet learned with \
                                 Structure from Motion Learner inference on KITTI Dataset',
                                 formatter_class=argparse.ArgumentDefaultsHelpFormatter)
parser.add_argument("--output-disp", action='store_true', help="save disparity img")
parser.add_argument("--output-depth", action='store_true', help="save depth img")
parser.add_argument("--pretrained", required=True, type=str, help="pretrained DispResNet path")
parser.add_argument("--img-height", default=256, type=int, help="Image height")
parser.add_argument("--img-width", default=832, type=int, help="Image width")
parser.add_argument("--no-resize", action='store_true', help="no resizing is done")

parser.add_argument("--dataset-list", default=None, type=str, help="Dataset list file")
parser.add_argument("--dataset-dir", default='.', type=str, help="Dataset directory")
parser.add_argument("--output-dir", default='output', type=str, help="Output directory")
parser.add_argument("--img-exts", default=['png', 'jpg', 'bmp'], nargs='*', type=str, help="images extensions to glob")
parser.add_argument('--resnet-layers', required=True, type=int, default=18, choices=[18, 50],
                    help='depth network architecture.')
parser.add_argument("--batch-size", default=1, type=int, help="images per forward pass")


def output_stem(file, dataset_dir):
    """(name, extension): the path of ``file`` relative to ``dataset_dir`` without its extension, its components joined
    by '-', and the extension."""
    rel, ext = os.path.splitext(os.path.relpath(file, dataset_dir))
    parts = [p for p in os.path.normpath(rel).split(os.sep) if p]
    return '-'.join(parts), ext


def list_files(args):
    if args.dataset_list is not None:
        with open(args.dataset_list, 'r') as f:
            return [os.path.join(args.dataset_dir, line) for line in f.read().splitlines()]
    found = sum([glob.glob(os.path.join(glob.escape(args.dataset_dir), '*.{}'.format(ext))) for ext in args.img_exts], [])
    return sorted(f for f in found if os.path.isfile(f))


def batches(files, args):
    """Lists of (file, uint8 [H, W, 3] array) of at most --batch-size frames; with --no-resize a batch ends where the
    frame size changes."""
    from PIL import Image
    bs = max(1, args.batch_size)
    batch = []
    for file in files:
        img = np.asarray(Image.open(file).convert("RGB"), dtype=np.uint8)
        if batch and (len(batch) == bs or (args.no_resize and img.shape != batch[0][1].shape)):
            yield batch
            batch = []
        batch.append((file, img))
    if batch:
        yield batch


def stage(batch, args, device):
    """The frames of a batch as uint8 [n, H, W, 3] on the device: frames of one source size go up in one copy and,
    unless --no-resize, through one resize to (img_height, img_width)."""
    from scsfm_hip import prepare
    by_shape = {}
    for i, (_, img) in enumerate(batch):
        by_shape.setdefault(img.shape, []).append(i)
    staged = [None] * len(batch)
    for shape, idx in by_shape.items():
        frames = torch.from_numpy(np.stack([batch[i][1] for i in idx])).to(device)
        if (not args.no_resize) and shape[:2] != (args.img_height, args.img_width):
            frames = prepare.resize_u8(frames, args.img_height, args.img_width)
        for k, i in enumerate(idx):
            staged[i] = frames[k]
    return torch.stack(staged)


def save_picture(path, rgba):
    from PIL import Image
    if path.lower().endswith('.png'):
        Image.fromarray(np.ascontiguousarray(rgba)).save(path)  # four channels: RGBA
    else:
        Image.fromarray(np.ascontiguousarray(rgba[..., :3])).save(path)


@torch.no_grad()
def main(argv=None, on_batch=None):
    """``on_batch(files, disp)`` -- for the tests -- is handed every batch's file names and its disparities,
    float32 [n, 1, H, W] on the device."""
    args = parser.parse_args(argv)
    if not (args.output_disp or args.output_depth):
        print('You must at least output one value !')
        return
    if not torch.cuda.is_available():
        raise SystemExit("run_inference.py needs a HIP device")
    device = torch.device("cuda")
    import models
    from scsfm_hip import visualise

    disp_net = models.DispResNet(args.resnet_layers, False).to(device)
    weights = torch.load(args.pretrained, map_location=device)
    disp_net.load_state_dict(weights['state_dict'])
    disp_net.eval()

    os.makedirs(args.output_dir, exist_ok=True)
    test_files = list_files(args)
    print('{} files to test'.format(len(test_files)))

    for batch in batches(test_files, args):
        files = [f for f, _ in batch]
        tensor_img = visualise.normalise_u8(stage(batch, args, device))
        output = disp_net(tensor_img)
        if on_batch is not None:
            on_batch(files, output)
        maps = output[:, 0]
        pictures = []
        if args.output_disp:
            disp = visualise.colourise(maps, colormap='bone', max_value=None)
            pictures.append(('disp', disp.cpu().numpy()))
        if args.output_depth:
            depth = visualise.colourise(maps, colormap='rainbow', max_value=10, reciprocal=True)
            pictures.append(('depth', depth.cpu().numpy()))
        for kind, arr in pictures:
            for file, rgba in zip(files, arr):
                file_name, file_ext = output_stem(file, args.dataset_dir)
                save_picture(os.path.join(args.output_dir, '{}_{}{}'.format(file_name, kind, file_ext)), rgba)


if __name__ == '__main__':
    main()
