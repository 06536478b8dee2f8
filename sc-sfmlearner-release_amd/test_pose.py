"""Scores a trained PoseResNet on KITTI odometry snippets -- the reference's test_pose.py (same flags, layout and
printout), plus --batch-size.

    python test_pose.py checkpoints/exp_pose_model_best.pth.tar --img-height 256 --img-width 832 \
        --dataset-dir kitti_odom_test/ --sequences 09 10 --output-dir results/pose/

<dataset-dir>/sequences/<seq>/image_2/* and <dataset-dir>/poses/<seq>.txt.  Prints ATE and RE, mean and std over every
5-frame snippet; with --output-dir writes predictions.npy, float64 [N, 5, 3, 4].

Adjacent snippets share all but one of their image pairs, so each sequence's n - 1 distinct pairs (k, k + 1) go through
the network once, in batches; the pose vectors stay on the device, and one library call folds, compensates and scores
every snippet of every sequence (scsfm_hip.snippets.evaluate_snippets over libscsfm_snip.so).  The sequences are taken in
sorted order (the reference iterates a set).  Images already of (img_height, img_width) are used as they are; others are
resized on the device (bilinear with antialiasing), where the reference uses skimage.transform.resize (see
INTEGRATION.md).  --sequence-length, which the reference parses and then ignores, is honoured for odd values.
"""
import argparse
import os

import numpy as np
import torch

parser = argparse.ArgumentParser(description='Script for PoseNet testing with corresponding groundTruth from KITTI Odometry',
                                 formatter_class=argparse.ArgumentDefaultsHelpFormatter)
parser.add_argument("pretrained_posenet", type=str, help="pretrained PoseNet path")
parser.add_argument("--img-height", default=256, type=int, help="Image height")
parser.add_argument("--img-width", default=832, type=int, help="Image width")
parser.add_argument("--no-resize", action='store_true', help="no resizing is done")
parser.add_argument("--min-depth", default=1e-3)
parser.add_argument("--max-depth", default=80)

parser.add_argument("--dataset-dir", type=str, help="Dataset directory")
parser.add_argument('--sequence-length', type=int, metavar='N', help='sequence length for testing', default=5)
parser.add_argument("--sequences", default=['09'], type=str, nargs='*', help="sequences to test")
parser.add_argument("--output-dir", default=None, type=str, help="Output directory for saving predictions in a big 3D numpy file")
parser.add_argument("--img-exts", default=['png', 'jpg', 'bmp'], nargs='*', type=str, help="images extensions to glob")
parser.add_argument("--rotation-mode", default='euler', choices=['euler', 'quat'], type=str)
parser.add_argument("--batch-size", default=1, type=int, help="image pairs per forward pass")


@torch.no_grad()
def pair_vectors(pose_net, files, args, device):
    """[n - 1, 6] on the device: row k is pose_net(img_k, img_{k+1}); every image is loaded once."""
    from test_vo import load_tensor_image
    n, bs = len(files), max(1, args.batch_size)
    vecs = []
    last = load_tensor_image(files[0], args, device) if n else None
    for j in range(0, n - 1, bs):
        imgs = [last] + [load_tensor_image(f, args, device) for f in files[j + 1:j + 1 + bs]]
        batch = torch.cat(imgs)
        vecs.append(pose_net(batch[:-1], batch[1:]))
        last = imgs[-1]
    return torch.cat(vecs).float() if vecs else torch.zeros((0, 6), device=device)


@torch.no_grad()
def main(argv=None):
    args = parser.parse_args(argv)
    seq_length = args.sequence_length
    if seq_length < 3 or seq_length > 15 or seq_length % 2 == 0:
        parser.error("--sequence-length must be odd, at least 3 and at most 15 (a snippet is centred on its target frame)")
    if not torch.cuda.is_available():
        raise SystemExit("test_pose.py needs a HIP device")
    device = torch.device("cuda")
    import models
    from kitti_eval.pose_evaluation_utils import read_scene_data
    from scsfm_hip.snippets import evaluate_snippets

    weights = torch.load(args.pretrained_posenet, map_location=device)
    pose_net = models.PoseResNet(18, False).to(device)
    pose_net.load_state_dict(weights['state_dict'], strict=False)
    pose_net.eval()

    img_files, poses, indices = read_scene_data(args.dataset_dir, args.sequences, seq_length, 1, args.img_exts)
    print('{} snippets to test'.format(sum(len(i) for i in indices)))
    for files, gt in zip(img_files, poses):
        if len(gt) < len(files):
            raise SystemExit("{} images but {} ground-truth poses".format(len(files), len(gt)))
    vecs = [pair_vectors(pose_net, files, args, device) for files in img_files]
    gts = [gt[:len(files)] for files, gt in zip(img_files, poses)]
    res = evaluate_snippets(vecs, gts, seq_length, args.rotation_mode)
    for line in res.report_lines():
        print(line)
    if args.output_dir is not None:
        os.makedirs(args.output_dir, exist_ok=True)
        np.save(os.path.join(args.output_dir, 'predictions.npy'), res.predictions)


if __name__ == '__main__':
    main()
