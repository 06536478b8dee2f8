"""Runs DispResNet over a folder (or list) of images and stores the depths for eval_depth.py -- the reference's
test_disp.py (same flags and output), plus --batch-size.

    python test_disp.py --resnet-layers 18 --img-height 256 --img-width 832 \
        --pretrained-dispnet checkpoints/dispnet_model_best.pth.tar --dataset-dir kitti_depth_test/color \
        --output-dir results

predictions.npy holds float64 copies of the float32 1 / disp, [N, img_height, img_width].  Images already of
(img_height, img_width) are used as they are; others are resized on the device (bilinear with antialiasing), where the
reference uses skimage.transform.resize.
"""
import argparse
import glob
import os
import time

import numpy as np
import torch

parser = argparse.ArgumentParser(description='Script for DispNet testing with corresponding groundTruth',
                                 formatter_class=argparse.ArgumentDefaultsHelpFormatter)
parser.add_argument("--pretrained-dispnet", required=True, type=str, help="pretrained DispNet path")
parser.add_argument("--img-height", default=256, type=int, help="Image height")
parser.add_argument("--img-width", default=832, type=int, help="Image width")
parser.add_argument("--min-depth", default=1e-3)
parser.add_argument("--max-depth", default=80)
parser.add_argument("--dataset-dir", default='.', type=str, help="Dataset directory")
parser.add_argument("--dataset-list", default=None, type=str, help="Dataset list file")
parser.add_argument("--output-dir", default=None, required=True, type=str,
                    help="Output directory for saving predictions in a big 3D numpy file")
parser.add_argument('--resnet-layers', required=True, type=int, default=18, choices=[18, 50],
                    help='depth network architecture.')
parser.add_argument("--batch-size", default=1, type=int, help="images per forward pass")


def load_tensor_image(filename, args, device):
    """[1, 3, img_height, img_width] normalised as (x / 255 - 0.45) / 0.225 on ``device``."""
    from PIL import Image
    img = np.asarray(Image.open(filename).convert("RGB"), dtype=np.float32)
    t = torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))).unsqueeze(0).to(device)
    if t.shape[-2:] != (args.img_height, args.img_width):
        t = torch.nn.functional.interpolate(t, size=(args.img_height, args.img_width), mode="bilinear",
                                            align_corners=False, antialias=True)
    return (t / 255 - 0.45) / 0.225


@torch.no_grad()
def main(argv=None):
    args = parser.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("test_disp.py needs a HIP device")
    device = torch.device("cuda")
    import models

    disp_net = models.DispResNet(args.resnet_layers, False).to(device)
    weights = torch.load(args.pretrained_dispnet, map_location=device)
    disp_net.load_state_dict(weights['state_dict'])
    disp_net.eval()

    if args.dataset_list is not None:
        with open(args.dataset_list, 'r') as f:
            test_files = list(f.read().splitlines())
    else:
        test_files = sorted(glob.glob(os.path.join(args.dataset_dir, '*.png')))
    print('{} files to test'.format(len(test_files)))
    os.makedirs(args.output_dir, exist_ok=True)

    predictions = np.zeros((len(test_files), args.img_height, args.img_width))
    avg_time = 0
    bs = max(1, args.batch_size)
    for j in range(0, len(test_files), bs):
        tgt_img = torch.cat([load_tensor_image(f, args, device) for f in test_files[j:j + bs]])
        torch.cuda.synchronize()
        t_start = time.time()
        output = disp_net(tgt_img)
        torch.cuda.synchronize()
        avg_time += time.time() - t_start
        predictions[j:j + bs] = 1 / output[:, 0].cpu().numpy()  # (float32, as the reference's 1 / pred_disp)

    np.save(os.path.join(args.output_dir, 'predictions.npy'), predictions)
    avg_time /= max(1, len(test_files))
    print('Avg Time: ', avg_time, ' seconds.')
    print('Avg Speed: ', 1.0 / avg_time if avg_time > 0 else float('inf'), ' fps')


if __name__ == '__main__':
    main()
