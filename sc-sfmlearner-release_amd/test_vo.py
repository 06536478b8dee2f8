"""Runs PoseResNet over a KITTI odometry sequence and writes the trajectory for kitti_eval/eval_odom.py -- the
reference's test_vo.py (same flags and output file), plus --batch-size.

    python test_vo.py --img-height 256 --img-width 832 --sequence 09 \
        --pretrained-posenet checkpoints/exp_pose_model_best.pth.tar --dataset-dir kitti_odom_test/sequences/ \
        --output-dir results/vo/

<output-dir><sequence>.txt holds one pose per frame, 12 numbers ('%1.8e'), the first one the identity.  The image pairs
(k, k + 1) go through the network in batches, the pose vectors stay on the device and are folded there
(scsfm_hip.odometry.chain_poses).  Images already of (img_height, img_width) are used as they are; others are resized
on the device (bilinear with antialiasing), where the reference uses skimage.transform.resize.
"""
import argparse
import glob
import os

import numpy as np
import torch

parser = argparse.ArgumentParser(description='Script for visualizing depth map and masks',
                                 formatter_class=argparse.ArgumentDefaultsHelpFormatter)
parser.add_argument("--pretrained-posenet", required=True, type=str, help="pretrained PoseNet path")
parser.add_argument("--img-height", default=256, type=int, help="Image height")
parser.add_argument("--img-width", default=832, type=int, help="Image width")
parser.add_argument("--no-resize", action='store_true', help="no resizing is done")

parser.add_argument("--dataset-dir", type=str, help="Dataset directory")
parser.add_argument("--output-dir", type=str, help="Output directory for saving predictions in a big 3D numpy file")
parser.add_argument("--img-exts", default=['png', 'jpg', 'bmp'], nargs='*', type=str, help="images extensions to glob")
parser.add_argument("--rotation-mode", default='euler', choices=['euler', 'quat'], type=str)

parser.add_argument("--sequence", default='09', type=str, help="sequence to test")
parser.add_argument("--batch-size", default=1, type=int, help="image pairs per forward pass")


def load_tensor_image(filename, args, device):
    """[1, 3, H, W] normalised as (x / 255 - 0.45) / 0.225 on ``device``."""
    from PIL import Image
    img = np.asarray(Image.open(filename).convert("RGB"), dtype=np.float32)
    t = torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))).unsqueeze(0).to(device)
    if (not args.no_resize) and t.shape[-2:] != (args.img_height, args.img_width):
        t = torch.nn.functional.interpolate(t, size=(args.img_height, args.img_width), mode="bilinear",
                                            align_corners=False, antialias=True)
    return (t / 255 - 0.45) / 0.225


@torch.no_grad()
def main(argv=None):
    args = parser.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("test_vo.py needs a HIP device")
    device = torch.device("cuda")
    import models
    from scsfm_hip.odometry import chain_poses

    weights_pose = torch.load(args.pretrained_posenet, map_location=device)
    pose_net = models.PoseResNet(18, False).to(device)  # (the weights come from the checkpoint)
    pose_net.load_state_dict(weights_pose['state_dict'], strict=False)
    pose_net.eval()

    image_dir = os.path.join(args.dataset_dir + args.sequence, "image_2")
    os.makedirs(args.output_dir, exist_ok=True)
    test_files = sorted(sum([glob.glob(os.path.join(image_dir, '*.{}'.format(ext))) for ext in args.img_exts], []))
    print('{} files to test'.format(len(test_files)))

    n = len(test_files)
    bs = max(1, args.batch_size)
    vecs = []
    last = load_tensor_image(test_files[0], args, device) if n else None
    for j in range(0, n - 1, bs):
        imgs = [last] + [load_tensor_image(f, args, device) for f in test_files[j + 1:j + 1 + bs]]
        batch = torch.cat(imgs)
        vecs.append(pose_net(batch[:-1], batch[1:]))
        last = imgs[-1]
    vec = torch.cat(vecs) if vecs else torch.zeros((0, 6), device=device)
    poses = chain_poses(vec.float(), args.rotation_mode).reshape(-1, 12).cpu().numpy()
    filename = args.output_dir + args.sequence + ".txt"
    np.savetxt(filename, poses, delimiter=' ', fmt='%1.8e')


if __name__ == '__main__':
    main()
