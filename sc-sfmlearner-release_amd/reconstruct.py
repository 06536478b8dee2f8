"""Dense voxel reconstruction of a sequence from the estimated depth and poses: PoseResNet gives the trajectory,
DispResNet the depth of every frame, and both are fused into a truncated signed distance volume whose surface points are
written as a coloured point cloud.  The reference shows this use of scale-consistent predictions and ships no program for
it; this one follows test_vo.py's and run_inference.py's flags.

    python reconstruct.py --pretrained-dispnet checkpoints/dispnet_model_best.pth.tar \
        --pretrained-posenet checkpoints/exp_pose_model_best.pth.tar --resnet-layers 18 \
        --dataset-dir kitti_odom_test/sequences/09/image_2 --intrinsics kitti_256/09_2/cam.txt \
        --max-depth 10 --voxel-size 0.05 --output-dir results/recon/

Pass one runs the pose net over the consecutive pairs of frames and folds the pose vectors on the device
(scsfm_hip.odometry.chain_poses), as test_vo.py does.  The volume is the box of the camera centres grown by --max-depth on
every side.  Pass two runs the disparity net in batches and integrates every batch on the device
(scsfm_hip.fusion.Volume, libscsfm_fuse.so): no prediction is copied to the host.  <output-dir>/reconstruction.ply holds
the surface points (binary little-endian: float x y z, uchar red green blue), <output-dir>/poses.txt the trajectory in
test_vo.py's format (12 numbers a frame, '%1.8e', the first one the identity).  With --mesh, <output-dir>/mesh.ply also
holds the surface as an indexed triangle mesh (scsfm_hip.meshing, libscsfm_mesh.so: marching tetrahedra on the voxel
grid; the same vertex format, then faces of three int indices); the other two files are the same bytes with and without it.

With --render a third pass brings the fused model back into the image domain (scsfm_hip.raycast, libscsfm_cast.so: one ray
per pixel marched through the volume): the pose of every fused frame is cast, in batches of --batch-size views, into
<output-dir>/fused_depth.npy (float32 [n, H, W]: the units and layout of 1 / disp, as run_inference.py's predictions.npy,
0 where no surface is seen) and <output-dir>/render/<frame name>_shade.png (lit from the camera) and _colour.png.  The
pass runs the disparity net again, batch by batch, and prints how far each frame's own prediction is from the model all
frames agreed on.  --render-poses FILE casts the poses of a text file in poses.txt's format instead (novel views, or
another run's trajectory); its pictures are named by index.  The older files are the same bytes with and without it.

With --refine-poses pass two closes the loop, as KinectFusion does (scsfm_hip.tracking, libscsfm_track.so): the first fused
frame is integrated at its chained pose; the others are taken in groups of --refine-group, each frame's guess is the pose
net's relative motion applied to the refined pose of the last frame before the group, the group is aligned to the model
fused so far by --refine-iterations of point-to-plane ICP against its ray cast, and integrated at the refined poses.  A
frame that never finds enough pairs, or a well-conditioned system, keeps its guess.  poses.txt stays the chain;
<output-dir>/poses_refined.txt has the same format (a frame that is not fused follows the refined frame before it by the
chain's relative motion), and reconstruction.ply, mesh.ply and the casts of --render are of the refined model and poses.

With --refine-scale (beside --refine-poses) the alignment has a seventh degree of freedom, the scale of the frame's own
depth (scsfm_hip.similarity, libscsfm_sim3.so): the nets' depth is only softly scale-consistent along a sequence, and a
rigid tracker trades a frame whose depth is a few per cent too long or too short for a wrong pose.  The first fused frame
has scale 1 and is not tracked; a group starts from the scale of the last frame fused before it; every frame is integrated
from its scaled depth (as a depth) at its refined pose, and a frame that kept its guess keeps its starting scale too.  In
an iteration whose scale pivot ratio is not above --refine-scale-pivot -- a frame that sees nothing but planes -- the scale
is held and the step is the rigid one.  <output-dir>/scales_refined.txt holds one scale per frame ('%1.8e'; a frame that is
not fused follows the fused frame before it), one more line is printed, and --render's |pred - fused| / fused compares the
scaled prediction.  --consistency-weight keeps computing its weights from the unscaled chain, and --follow works
unchanged.  Without --refine-scale every file and printed line is what it was.

With --consistency-weight every observation enters the volume with the depth consistency of its pixel as its weight
(scsfm_hip.confidence, libscsfm_conf.so): pass two first runs the disparity net over all fused frames and keeps the
disparities on the device, every frame is compared with its --consistency-radius neighbours on either side among the fused
frames (with --every N they are N frames apart) at the chain's poses -- one minus the depth inconsistency of the training
loss, |D_computed - D_projected| / (D_computed + D_projected), averaged over the neighbours or, with --consistency-reduce
max, the best of them -- and the frames are then integrated from the stored disparities with that weight: a pixel below
--consistency-floor, or with fewer than --consistency-min-views neighbours to compare with, is not fused at all.  With
--refine-poses the weights are still those of the chain's poses (its relative poses do not depend on the refinement, and
the frames ahead are not refined yet), and the alignment itself stays unweighted.  --output-confidence writes
<output-dir>/confidence.npy (float32 [n, H, W]) and <output-dir>/confidence/<frame name>.png (8-bit grey).  Without
--consistency-weight every file and printed line is what it was.

With --follow the volume has a fixed size and moves with the camera (scsfm_hip.rolling, libscsfm_roll.so: KinectFusion's
moving volume), so memory is set by --max-depth and not by the length of the path, and a sequence of any length is fused at
one --voxel-size, which the flag requires.  The window is --follow-dims voxels (default a cube of side
2 (max-depth + trunc) / voxel-size + 2 step, rounded up to a multiple of 8) on a lattice fixed by its first corner, which
centres the first batch's middle camera.  Before each batch of pass two (each group under --refine-poses) the window is
placed from the camera centre of the batch's frame len // 2 -- the chain's pose, from the host copy that poses.txt is
written from, or under --refine-poses the group's guessed pose, one copy of 96 bytes per group -- and moves in whole
multiples of --follow-step voxels once that camera's cell is a step or more from the central cell.  The surface points
whose edges leave the window are extracted first and copied to the host, the planes are shifted, what enters is empty, and
space that was left is not entered again.  reconstruction.ply is the streamed points in the order of the shifts followed by
the points still in the window at the end; every edge of the lattice gives at most one point.  --consistency-weight works
unchanged (its weights do not depend on the volume).  --mesh, --render and --render-poses are refused beside --follow: a
mesh stitched over windows and casts of a volume that has moved on are not built.  Without --follow every file and printed
line is what it was.

Units: the predictions have the nets' own scale -- consistent along the sequence, which is what lets the frames be fused,
but not metric.  --max-depth, --voxel-size and --trunc are in those units (the nets' depth is 1 / disparity, between 0.1
and 100).  The frames are decoded on the host, resized on the device as run_inference.py resizes them, and --intrinsics
(a 3 x 3 text file like the prepared data's cam.txt, for the frames as they are stored) is rescaled with them.
"""
import argparse
import os

import numpy as np
import torch

import run_inference

parser = argparse.ArgumentParser(description='Dense voxel reconstruction from the estimated depth and poses (TSDF fusion '
                                 'on the device). All lengths are in the units of the nets\' predictions, which are '
                                 'consistent along a sequence but not metric.',
                                 formatter_class=argparse.ArgumentDefaultsHelpFormatter)
parser.add_argument("--pretrained-dispnet", required=True, type=str, help="pretrained DispResNet path")
parser.add_argument("--pretrained-posenet", required=True, type=str, help="pretrained PoseResNet path")
parser.add_argument('--resnet-layers', type=int, default=18, choices=[18, 50], help='depth network architecture.')
parser.add_argument("--dataset-dir", required=True, type=str, help="a folder of frames, taken in sorted order")
parser.add_argument("--intrinsics", required=True, type=str,
                    help="3x3 text file (as cam.txt) of the frames as stored; rescaled when they are resized")
parser.add_argument("--img-height", default=256, type=int, help="Image height")
parser.add_argument("--img-width", default=832, type=int, help="Image width")
parser.add_argument("--no-resize", action='store_true', help="no resizing is done")
parser.add_argument("--img-exts", default=['png', 'jpg', 'bmp'], nargs='*', type=str, help="images extensions to glob")
parser.add_argument("--rotation-mode", default='euler', choices=['euler', 'quat'], type=str)
parser.add_argument("--batch-size", default=8, type=int,
                    help="frames per forward pass; a batch is integrated in launches of --frames-per-launch, so keep it "
                         "at least that large")
parser.add_argument("--max-depth", default=10.0, type=float,
                    help="predicted depths beyond this are not fused, and the box is grown by it (the nets' units)")
parser.add_argument("--voxel-size", default=None, type=float, help="edge of a voxel (the nets' units)")
parser.add_argument("--resolution", default=None, type=int,
                    help="voxels along the longest side of the box, instead of --voxel-size (default 256)")
parser.add_argument("--trunc", default=None, type=float,
                    help="truncation distance; default 3 voxels (scsfm_hip.fusion.TRUNC_VOXELS)")
parser.add_argument("--min-weight", default=2.0, type=float,
                    help="a surface point needs both voxels of its edge seen at least this often")
parser.add_argument("--frames-per-launch", default=None, type=int,
                    help="frames one launch of the integration carries (default scsfm_hip.fusion.FRAMES_PER_LAUNCH)")
parser.add_argument("--every", default=1, type=int, metavar="N", help="fuse every N-th frame (all frames give the poses)")
parser.add_argument("--mesh", action='store_true',
                    help="also write <output-dir>/mesh.ply: the surface as an indexed triangle mesh (marching tetrahedra "
                         "on the device, scsfm_hip.meshing)")
parser.add_argument("--render", action='store_true',
                    help="also cast the pose of every fused frame through the volume: <output-dir>/fused_depth.npy and "
                         "<output-dir>/render/*_shade.png, *_colour.png (scsfm_hip.raycast)")
parser.add_argument("--render-poses", default=None, type=str, metavar="FILE",
                    help="cast these poses instead (poses.txt's format: 12 numbers a line, camera to world); implies "
                         "--render, names the pictures by index")
parser.add_argument("--render-step", default=None, type=float,
                    help="distance between two samples of a ray, as a depth (the nets' units); default the voxel size")
parser.add_argument("--render-near", default=0.0, type=float, help="depth of a ray's first sample (the nets' units)")
parser.add_argument("--refine-poses", action='store_true',
                    help="align every fused frame to the model fused so far before it is integrated (frame-to-model ICP, "
                         "scsfm_hip.tracking); also writes <output-dir>/poses_refined.txt")
parser.add_argument("--refine-iterations", default=10, type=int, metavar="N", help="ICP iterations per frame (1 .. 64)")
parser.add_argument("--refine-group", default=1, type=int, metavar="G",
                    help="frames aligned and integrated together: 1 is KinectFusion's loop; more trades the later "
                         "frames' view of the earlier ones for fewer and fuller launches")
parser.add_argument("--refine-max-dist", default=None, type=float, metavar="D",
                    help="a frame's point and the model's point pair up to this distance (the nets' units); default "
                         "the truncation distance")
parser.add_argument("--refine-scale", action='store_true',
                    help="also refine a scale of every fused frame's depth: ICP over seven degrees of freedom "
                         "(scsfm_hip.similarity); needs --refine-poses; also writes <output-dir>/scales_refined.txt")
parser.add_argument("--refine-scale-pivot", default=None, type=float, metavar="P",
                    help="a frame's scale is solved in an iteration whose scale pivot ratio is above this and held "
                         "otherwise; needs --refine-scale (default scsfm_hip.similarity.MIN_SCALE_PIVOT, 2e-3)")
parser.add_argument("--consistency-weight", action='store_true',
                    help="weigh every observation by the depth consistency of its pixel with the neighbouring fused frames "
                         "(scsfm_hip.confidence); the disparities of all fused frames are kept on the device")
parser.add_argument("--consistency-radius", default=None, type=int, metavar="R",
                    help="fused frames on either side a frame is compared with, 1 .. 4 (default 1)")
parser.add_argument("--consistency-reduce", default=None, choices=['mean', 'max'],
                    help="a pixel's weight over its neighbours: their mean, as the training loss averages, or the best "
                         "one, which is kinder to occlusions (default mean)")
parser.add_argument("--consistency-min-views", default=None, type=int, metavar="N",
                    help="a pixel that fewer neighbours can be compared with gets the weight 0 (default 1)")
parser.add_argument("--consistency-floor", default=None, type=float, metavar="T",
                    help="a weight below this becomes 0: the pixel is not fused (0 .. 1; default 0.0, nothing is cut)")
parser.add_argument("--output-confidence", action='store_true',
                    help="also write <output-dir>/confidence.npy and <output-dir>/confidence/*.png (needs "
                         "--consistency-weight)")
parser.add_argument("--follow", action='store_true',
                    help="a volume of fixed size that moves with the camera (scsfm_hip.rolling); needs --voxel-size; the "
                         "points that leave are streamed into reconstruction.ply")
parser.add_argument("--follow-dims", default=None, type=int, nargs=3, metavar=("NX", "NY", "NZ"),
                    help="voxels of the moving window (default a cube of side 2 (max-depth + trunc) / voxel-size + 2 "
                         "step, rounded up to a multiple of 8)")
parser.add_argument("--follow-step", default=None, type=int, metavar="N",
                    help="the window moves in whole multiples of this many voxels (default 8)")
parser.add_argument("--output-dir", default='output', type=str, help="Output directory")


def scaled_intrinsics(K, stored_hw, used_hw):
    """cam.txt's matrix for frames resized from stored_hw to used_hw: the first row scales with the width, the second
    with the height (as the data loaders and data/prepare_train_data.py scale it)"""
    K = np.array(K, np.float64).reshape(3, 3)
    K[0] *= used_hw[1] / stored_hw[1]
    K[1] *= used_hw[0] / stored_hw[0]
    return K.astype(np.float32)


def frames(files, args, device, bs):
    """(first index, normalised float32 [n, 3, H, W] on the device, stored (H, W)) per batch of at most bs frames"""
    from scsfm_hip import visualise
    args = argparse.Namespace(**{**vars(args), "batch_size": bs})
    k = 0
    for batch in run_inference.batches(files, args):
        yield k, visualise.normalise_u8(run_inference.stage(batch, args, device)), batch[0][1].shape[:2]
        k += len(batch)


def read_poses(path):
    """--render-poses' file -> float64 [n, 3, 4]: n >= 1 lines of 12 finite numbers, camera to world"""
    try:
        with open(path) as f:
            rows = [[float(v) for v in line.split()] for line in f if line.strip() and not line.lstrip().startswith("#")]
    except (OSError, ValueError) as e:
        raise SystemExit("--render-poses {}: {}".format(path, e))
    if not rows or any(len(r) != 12 for r in rows):
        raise SystemExit("--render-poses {}: every line must hold 12 numbers (a 3 x 4 camera-to-world matrix, as "
                         "poses.txt), and there must be at least one".format(path))
    poses = np.array(rows, np.float64)
    if not np.isfinite(poses).all():
        raise SystemExit("--render-poses {}: a pose that is not finite".format(path))
    return poses.reshape(-1, 3, 4)


def render(args, vol, disp_net, views, K_dev, hw, device, names, files=None, on_render=None, scales=None):
    """The third pass: casts ``views`` (float64 [n, 3, 4] on the device) in batches and writes fused_depth.npy and the
    pictures.  With ``files`` (the fused frames, one per view) the disparity net runs again batch by batch and the
    agreement of its depth with the fused one is summed on the device, in float64, and read back once; with ``scales``
    (--refine-scale: float64 [n], one per view) the depth compared is the scaled one that was fused."""
    from PIL import Image

    from scsfm_hip import raycast
    out_dir = os.path.join(args.output_dir, "render")
    os.makedirs(out_dir, exist_ok=True)
    mask = raycast.brick_mask(vol, args.min_weight)
    far = args.max_depth + vol.trunc
    sums = torch.zeros(3, dtype=torch.float64, device=device)  # pixels with a hit, pixels compared, sum of the ratios
    preds = frames(files, args, device, args.batch_size) if files is not None else None
    depths = []
    for k in range(0, len(views), args.batch_size):
        batch = views[k:k + args.batch_size].contiguous()
        got = vol.raycast(batch, K_dev, hw, args.render_near, far, step=args.render_step, min_weight=args.min_weight,
                          mask=mask)
        if on_render is not None:
            on_render(got, batch)
        hit = got.depth > 0
        sums[0] += hit.sum()
        if preds is not None:
            k0, imgs, _ = next(preds)
            assert k0 == k and len(imgs) == len(batch)
            if scales is None:
                pred = 1.0 / disp_net(imgs)[:, 0]
            else:   # (--refine-scale: the prediction as it was fused)
                from scsfm_hip import similarity
                pred = similarity.scaled_depth(disp_net(imgs).contiguous(), scales[k:k + len(batch)].contiguous(),
                                               is_disp=True)[:, 0]
            both = hit & (pred <= args.max_depth)
            ratio = (pred.double() - got.depth.double()).abs() / got.depth.double()
            sums[1] += both.sum()
            sums[2] += torch.where(both, ratio, torch.zeros_like(ratio)).sum()
        depths.append(got.depth.cpu().numpy())
        rgb, shade = got.rgb.cpu().numpy(), got.shade.cpu().numpy()
        for j in range(len(batch)):
            Image.fromarray(shade[j]).save(os.path.join(out_dir, names[k + j] + "_shade.png"))
            Image.fromarray(rgb[j]).save(os.path.join(out_dir, names[k + j] + "_colour.png"))
    path = os.path.join(args.output_dir, "fused_depth.npy")
    np.save(path, np.concatenate(depths))
    n_hit, n_both, total = sums.tolist()
    share = n_hit / (len(views) * hw[0] * hw[1])
    if preds is None:
        print('rendered {} views -> {}: {:.9g} of the pixels with a hit'.format(len(views), path, share))
    else:
        print('rendered {} views -> {}: {:.9g} of the pixels with a hit; mean |pred - fused| / fused {:.9g} over {} '
              'pixels'.format(len(views), path, share, total / n_both if n_both else float("nan"), int(n_both)))


def relative_to(anchor_refined, anchor, poses):
    """anchor_refined @ inverse(anchor) @ poses[i]: the chain's motion from the anchor frame to each of ``poses``
    (float64 [n, 3, 4], rigid, camera to world) applied to the anchor's refined pose -> float64 [n, 3, 4].  In double, with
    torch on the device; a rigid pose's inverse is (R^T, -R^T t)."""
    Ra, ta = anchor[:, :3], anchor[:, 3]
    Rr, tr = anchor_refined[:, :3], anchor_refined[:, 3]
    R = Rr @ (Ra.T @ poses[:, :, :3])
    t = (Rr @ (Ra.T @ (poses[:, :, 3] - ta).T)).T + tr
    return torch.cat([R, t[:, :, None]], dim=2).contiguous()


def refine(args, vol, disp_net, files, chosen, c2w, K_dev, device, on_batch=None, on_track=None, disps=None, weights=None,
           follow=None):
    """Pass two with --refine-poses (see the module's docstring) -> the refined poses of all frames, float64 [n, 3, 4] on
    the device.  The figures of the printed line are summed on the device, in float64, and read back once.  With
    ``disps`` and ``weights`` (--consistency-weight: the stored disparities [n, 1, H, W] and the weights [n, H, W] of the
    chosen frames) the net is not run again and every frame is integrated with its rows of the weights.  ``follow``
    (--follow) is handed the pose the window is placed from before every group is tracked: the first frame's chained pose,
    then each group's middle guess.  With --refine-scale the return value is (the refined poses, the refined scales of
    all frames, float64 [n] on the device): every frame carries a scale of its depth, a group starts from the scale of the
    last frame fused before it, is aligned over seven degrees of freedom (scsfm_hip.similarity) and is integrated from
    the scaled depth, as a depth."""
    from scsfm_hip import tracking
    if args.refine_scale:
        from scsfm_hip import similarity
        scales = torch.ones(len(c2w), dtype=torch.float64, device=device)
        pivot = similarity.MIN_SCALE_PIVOT if args.refine_scale_pivot is None else args.refine_scale_pivot
        held = torch.zeros(1, dtype=torch.float64, device=device)   # frames whose scale was held throughout
    refined = c2w.clone()
    done = 0                                # chosen frames fused so far
    sums = torch.zeros(6, dtype=torch.float64, device=device)  # rms first / last (sum, frames), pair share, kept

    def fuse(disp, imgs, idx, poses, at):
        if args.refine_scale:   # the depth the tracker saw, as a depth
            disp = similarity.scaled_depth(disp, scales[idx], is_disp=True)
        batch = (disp, imgs, poses.contiguous(), K_dev)
        if on_batch is not None:
            on_batch(*batch)
        vol.integrate(*batch, is_disp=not args.refine_scale, max_depth=args.max_depth,
                      weight=None if weights is None else weights[at:at + len(disp)])
        refined[idx] = poses

    for first, group in ((True, 1), (False, args.refine_group)):
        todo = chosen[:1] if first else chosen[1:]
        if not todo:
            continue
        for k, imgs, _ in frames([files[i] for i in todo], args, device, group):
            at = k if first else 1 + k      # the group's place among the chosen frames
            disp = disp_net(imgs).contiguous() if disps is None else disps[at:at + len(imgs)]
            ids = todo[k:k + len(imgs)]
            idx = torch.tensor(ids, device=device)
            if first:
                if follow is not None:
                    follow(c2w[ids[0]])
                fuse(disp, imgs, idx, c2w[idx], at)
                continue
            anchor = chosen[done]               # the last frame before the group
            guess = relative_to(refined[anchor], c2w[anchor], c2w[idx])
            if follow is not None:
                follow(guess[len(ids) // 2])
            if args.refine_scale:
                scale0 = scales[anchor].expand(len(ids)).contiguous()
                got = vol.track_scaled(disp, guess, scale0, K_dev, is_disp=True, max_depth=args.max_depth,
                                       iterations=args.refine_iterations, max_dist=args.refine_max_dist,
                                       min_scale_pivot=pivot)
                kept = similarity.kept_guess(got.report)
                scales[idx] = torch.where(kept, scale0, got.scale)
                held += similarity.held_scale(got.report).sum()
            else:
                got = vol.track(disp, guess, K_dev, is_disp=True, max_depth=args.max_depth,
                                iterations=args.refine_iterations, max_dist=args.refine_max_dist)
                kept = tracking.kept_guess(got.report)
            if on_track is not None:
                on_track(ids, guess, got, disp)
            fuse(disp, imgs, idx, torch.where(kept[:, None, None], guess, got.c2w), at)
            done += len(ids)
            count, rr = got.report[:, :, 0], got.report[:, :, 1]
            for j, it in ((0, 0), (2, -1)):
                some = count[:, it] > 0
                rms = torch.sqrt(rr[:, it] / torch.where(some, count[:, it], torch.ones_like(count[:, it])))
                sums[j] += torch.where(some, rms, torch.zeros_like(rms)).sum()
                sums[j + 1] += some.sum()
            sums[4] += count[:, -1].sum() / (disp.shape[-2] * disp.shape[-1])
            sums[5] += kept.sum()
    # a frame that is not fused follows the refined frame before it
    for a, b in zip(chosen, chosen[1:] + [len(c2w)]):
        if b > a + 1:
            refined[a + 1:b] = relative_to(refined[a], c2w[a], c2w[a + 1:b])
    path = os.path.join(args.output_dir, "poses_refined.txt")
    np.savetxt(path, refined.reshape(-1, 12).cpu().numpy(), delimiter=' ', fmt='%1.8e')
    first_sum, first_n, last_sum, last_n, share, kept = sums.tolist()
    n = len(chosen) - 1
    print('refined {} poses -> {}: mean rms residual {:.12g} -> {:.12g}, mean pair share {:.12g}, {} frames kept their '
          'guess'.format(n, path, first_sum / first_n if first_n else float("nan"),
                         last_sum / last_n if last_n else float("nan"), share / n if n else float("nan"), int(kept)))
    if args.refine_scale:
        # a frame that is not fused follows the fused frame before it
        for a, b in zip(chosen, chosen[1:] + [len(c2w)]):
            scales[a + 1:b] = scales[a]
        path = os.path.join(args.output_dir, "scales_refined.txt")
        np.savetxt(path, scales.cpu().numpy(), fmt='%1.8e')
        tracked = scales[torch.tensor(chosen[1:], dtype=torch.long, device=device)]
        if n:
            low, mean, high, n_held = torch.stack([tracked.min(), tracked.mean(), tracked.max(), held[0]]).tolist()
        else:
            low = mean = high = float("nan")
            n_held = 0
        print('refined {} scales -> {}: min {:.12g}, mean {:.12g}, max {:.12g}, {} frames held their scale '
              'throughout'.format(n, path, low, mean, high, int(n_held)))
        return refined, scales
    return refined


def too_many_pixels(args, n, hw):
    """--consistency-weight keeps n frames of hw on the device and weighs them in one call, whose sizes are ints"""
    if args.consistency_weight and n * hw[0] * hw[1] > 2 ** 31 - 1:
        raise SystemExit("--consistency-weight keeps the disparities of all {} fused frames of {} x {} on the device, and "
                         "their pixels are more than 2^31 - 1: fuse fewer frames (a larger --every)".format(n, *hw))


def consistency(args, disp_net, files, chosen, c2w, K_dev, hw, device, on_weights=None):
    """The first half of pass two with --consistency-weight -> (the disparities float32 [n, 1, H, W], the weights float32
    [n, H, W]) of the chosen frames, on the device.  The figures of the printed line are summed on the device, in
    float64, and read back once."""
    from scsfm_hip import confidence
    n = len(chosen)
    disps = torch.empty((n, 1) + tuple(hw), dtype=torch.float32, device=device)
    print('disparities of {} frames kept on the device: {:.1f} MB'.format(n, disps.numel() * 4 / 1e6))
    for k, imgs, _ in frames([files[i] for i in chosen], args, device, args.batch_size):
        disps[k:k + len(imgs)] = disp_net(imgs)
    idx = torch.tensor(chosen, device=device)
    weight = confidence.weights(disps, c2w[idx].contiguous(), K_dev, radius=args.consistency_radius, is_disp=True,
                                max_depth=args.max_depth, min_views=args.consistency_min_views,
                                floor=args.consistency_floor, reduce=args.consistency_reduce)
    if on_weights is not None:
        on_weights(weight, disps)
    total, zeros = torch.stack([weight.sum(dtype=torch.float64), (weight == 0).sum().double()]).tolist()
    print('confidence of {} frames: mean {:.9g}, {:.9g} of the pixels at zero'.format(
        n, total / weight.numel(), zeros / weight.numel()))
    if args.output_confidence:
        from PIL import Image
        out_dir = os.path.join(args.output_dir, "confidence")
        os.makedirs(out_dir, exist_ok=True)
        np.save(os.path.join(args.output_dir, "confidence.npy"), weight.cpu().numpy())
        grey = (weight * 255.0 + 0.5).to(torch.uint8).cpu().numpy()
        for j, i in enumerate(chosen):
            name = os.path.splitext(os.path.basename(str(files[i])))[0]
            Image.fromarray(grey[j]).save(os.path.join(out_dir, name + ".png"))
    return disps, weight


# Voxels the window of --follow moves by, in whole multiples.  A larger step means fewer, equally expensive shifts and a
# window 2 step voxels wider on every axis.  Measured (tools/bench_rolling.py, profiles/rolling_bench.json: a generated drive
# of 256 frames of 256 x 832 through a window of 184 voxels a side, batches of 8, medians of 15): at 8 the 31 shifts cost
# 0.12 ms each, the count's trip to the host and the points' copy included, 61 % of a pass two WITHOUT nets (6.25 ms); once
# the disparity net runs between two shifts that is a few per cent, so 8 stays, and a step of 16 would halve it for a window
# 16 voxels wider, which is unmeasured.
FOLLOW_STEP = 8


def follow_arguments(args):
    """--follow's flags, checked and completed before anything is loaded: args.follow_step and args.follow_dims are set"""
    given = [flag for flag, value in (("--follow-dims", args.follow_dims), ("--follow-step", args.follow_step))
             if value is not None]
    if given and not args.follow:
        raise SystemExit("{} needs --follow".format(given[0]))
    args.follow_step = FOLLOW_STEP if args.follow_step is None else args.follow_step
    if not args.follow:
        return
    if args.voxel_size is None:
        raise SystemExit("--follow needs --voxel-size: the lattice of a moving volume is fixed before the path is known")
    if not (args.voxel_size > 0 and np.isfinite(args.voxel_size)):
        raise SystemExit("--voxel-size must be positive")
    for flag, value in (("--mesh", args.mesh), ("--render-poses", args.render_poses is not None), ("--render", args.render)):
        if value:
            raise SystemExit("--follow cannot be combined with {}: the volume has moved on from what left it".format(flag))
    if args.follow_step < 1:
        raise SystemExit("--follow-step must be at least 1")
    if args.follow_dims is None:
        from scsfm_hip.fusion import TRUNC_VOXELS    # (imports torch and the table of libraries; loads none)
        trunc = TRUNC_VOXELS * args.voxel_size if args.trunc is None else args.trunc
        side = 2.0 * (args.max_depth + trunc) / args.voxel_size + 2 * args.follow_step
        if not side < 2 ** 31:
            raise SystemExit("--follow: a window of {:.6g} voxels a side is above the limit of 2^29 voxels: choose a "
                             "larger --voxel-size or give --follow-dims".format(side))
        args.follow_dims = [max(8, 8 * int(np.ceil(side / 8.0)))] * 3
    if min(args.follow_dims) < 1:
        raise SystemExit("--follow-dims must all be at least 1")
    if args.follow_dims[0] * args.follow_dims[1] * args.follow_dims[2] > 2 ** 29:
        raise SystemExit("--follow-dims: a window of {} x {} x {} voxels is above the limit of 2^29: choose a larger "
                         "--voxel-size or smaller --follow-dims".format(*args.follow_dims))


@torch.no_grad()
def main(argv=None, on_poses=None, on_batch=None, on_render=None, on_track=None, on_weights=None, on_shift=None):
    """``on_poses(vec)``, ``on_batch(disp, imgs, c2w, K)``, ``on_render(result, views)``, ``on_track(indices, guess,
    track, disp)`` and ``on_weights(weight, disp)`` -- for the tests -- are handed the pose vectors [n - 1, 6], every fused
    batch's tensors, every rendered batch's scsfm_hip.raycast.Cast with its poses [b, 3, 4], every tracked group's frame
    indices, guessed poses [g, 3, 4], scsfm_hip.tracking.Track and disparities, and the weights [n, H, W] of
    --consistency-weight with the stored disparities [n, 1, H, W] of the fused frames, all on the device.
    ``on_shift(shift, offset, xyz, rgb)`` is handed every move of --follow's window: the shift in voxels, the window's
    offset after it, and the points that left with it, on the device; it is called before the ``on_batch`` of the batch
    the window was moved for.  With --refine-scale ``on_batch``'s first tensor is the scaled depth that is integrated
    and ``on_track``'s track a scsfm_hip.similarity.Track."""
    args = parser.parse_args(argv)
    follow_arguments(args)
    given = [flag for flag, value in (("--consistency-radius", args.consistency_radius),
                                      ("--consistency-reduce", args.consistency_reduce),
                                      ("--consistency-min-views", args.consistency_min_views),
                                      ("--consistency-floor", args.consistency_floor),
                                      ("--output-confidence", args.output_confidence or None)) if value is not None]
    if given and not args.consistency_weight:
        raise SystemExit("{} needs --consistency-weight".format(given[0]))
    args.consistency_radius = 1 if args.consistency_radius is None else args.consistency_radius
    args.consistency_reduce = args.consistency_reduce or 'mean'
    args.consistency_min_views = 1 if args.consistency_min_views is None else args.consistency_min_views
    args.consistency_floor = 0.0 if args.consistency_floor is None else args.consistency_floor
    if not 1 <= args.consistency_radius <= 4:
        raise SystemExit("--consistency-radius must be between 1 and 4")
    if args.consistency_min_views < 1:
        raise SystemExit("--consistency-min-views must be at least 1")
    if not 0.0 <= args.consistency_floor <= 1.0:
        raise SystemExit("--consistency-floor must be between 0 and 1")
    if not 1 <= args.refine_iterations <= 64:
        raise SystemExit("--refine-iterations must be between 1 and 64")
    if args.refine_group < 1:
        raise SystemExit("--refine-group must be at least 1")
    if args.refine_max_dist is not None and not (args.refine_max_dist > 0 and np.isfinite(args.refine_max_dist)):
        raise SystemExit("--refine-max-dist must be positive")
    if args.refine_scale and not args.refine_poses:
        raise SystemExit("--refine-scale needs --refine-poses")
    if args.refine_scale_pivot is not None and not args.refine_scale:
        raise SystemExit("--refine-scale-pivot needs --refine-scale")
    if args.refine_scale_pivot is not None and not args.refine_scale_pivot > 0:
        raise SystemExit("--refine-scale-pivot must be positive")
    novel = read_poses(args.render_poses) if args.render_poses is not None else None
    if args.render_step is not None and not (args.render_step > 0 and np.isfinite(args.render_step)):
        raise SystemExit("--render-step must be positive")
    if not (args.render_near >= 0 and np.isfinite(args.render_near)):
        raise SystemExit("--render-near must not be negative")
    if not torch.cuda.is_available():
        raise SystemExit("reconstruct.py needs a HIP device")
    if args.voxel_size is not None and args.resolution is not None:
        raise SystemExit("give either --voxel-size or --resolution")
    if args.every < 1 or args.batch_size < 1:
        raise SystemExit("--every and --batch-size must be at least 1")
    device = torch.device("cuda")
    import models
    from scsfm_hip import fusion
    from scsfm_hip.odometry import chain_poses

    disp_net = models.DispResNet(args.resnet_layers, False).to(device)
    disp_net.load_state_dict(torch.load(args.pretrained_dispnet, map_location=device)['state_dict'])
    disp_net.eval()
    pose_net = models.PoseResNet(18, False).to(device)
    pose_net.load_state_dict(torch.load(args.pretrained_posenet, map_location=device)['state_dict'], strict=False)
    pose_net.eval()

    args.dataset_list = None
    files = run_inference.list_files(args)
    print('{} files to reconstruct from'.format(len(files)))
    if len(files) < 2:
        raise SystemExit("reconstruct.py needs at least two frames")
    chosen = list(range(0, len(files), args.every))
    if not args.no_resize:
        too_many_pixels(args, len(chosen), (args.img_height, args.img_width))
    os.makedirs(args.output_dir, exist_ok=True)

    # pass one: the trajectory
    vecs, last, sizes = [], None, set()
    for _, imgs, stored in frames(files, args, device, args.batch_size):
        sizes.add((stored, tuple(imgs.shape[-2:])))
        seq = imgs if last is None else torch.cat([last, imgs])
        if len(seq) > 1:
            vecs.append(pose_net(seq[:-1], seq[1:]))
        last = imgs[-1:]
    if len(sizes) != 1:
        raise SystemExit("the frames of a reconstruction must all have one size")
    (stored_hw, used_hw), = sizes
    too_many_pixels(args, len(chosen), used_hw)     # (again: with --no-resize the size is known only now)
    vec = torch.cat(vecs).float()
    if on_poses is not None:
        on_poses(vec)
    c2w = chain_poses(vec, args.rotation_mode).contiguous()  # float64 [n, 3, 4], on the device
    chain = c2w.reshape(-1, 12).cpu().numpy()
    np.savetxt(os.path.join(args.output_dir, "poses.txt"), chain, delimiter=' ', fmt='%1.8e')
    K = scaled_intrinsics(np.genfromtxt(args.intrinsics), stored_hw, used_hw)

    streamed, follow = [], None
    if args.follow:
        # the window: its first corner centres the middle camera of the first batch (under --refine-poses the first frame)
        from scsfm_hip import rolling
        dims, voxel = tuple(args.follow_dims), args.voxel_size
        middle = chosen[0] if args.refine_poses else chosen[min(args.batch_size, len(chosen)) // 2]
        origin = rolling.initial_origin(chain[middle].reshape(3, 4)[:, 3], dims, voxel)
        print('window: {} x {} x {} voxels of {:.6g}, {:.1f} MB, first corner ({:.4g}, {:.4g}, {:.4g})'.format(
            *dims, voxel, 40 * dims[0] * dims[1] * dims[2] / 1e6, *origin))
        vol = rolling.RollingVolume(dims, origin, voxel, args.trunc, device=device,
                                    frames_per_launch=args.frames_per_launch or fusion.FRAMES_PER_LAUNCH)

        def follow(pose):
            """places the window for the camera of ``pose`` ([3, 4], a host array or a device tensor: 96 bytes)"""
            pose = pose.cpu().numpy() if isinstance(pose, torch.Tensor) else pose
            shift = rolling.shift_for(pose.reshape(3, 4)[:, 3], vol.origin0, vol.offset, vol.dims, vol.voxel,
                                      args.follow_step)
            if any(shift):
                xyz, rgb = vol.shift(shift, args.min_weight)
                if on_shift is not None:
                    on_shift(shift, vol.offset, xyz, rgb)
                streamed.append((xyz.cpu().numpy(), rgb.cpu().numpy()))

    # the box
    if not args.follow:
        lo, hi = fusion.camera_box(c2w, args.max_depth)
        voxel = args.voxel_size if args.voxel_size is not None else float((hi - lo).max()) / (args.resolution or 256)
        origin, dims = fusion.bounds_from_cameras(c2w, args.max_depth, voxel)
        nvox = dims[0] * dims[1] * dims[2]
        print('volume: {} x {} x {} voxels of {:.6g}, {:.1f} MB, corner ({:.4g}, {:.4g}, {:.4g})'.format(
            *dims, voxel, 20 * nvox / 1e6, *origin))
        if nvox > fusion.MAX_VOXELS:
            raise SystemExit("a volume of {} voxels is above the limit of 2^29: choose a larger --voxel-size (or a smaller "
                             "--resolution or --max-depth)".format(nvox))
        vol = fusion.Volume(dims, origin, voxel, args.trunc, device=device,
                            frames_per_launch=args.frames_per_launch or fusion.FRAMES_PER_LAUNCH)
    K_dev = torch.from_numpy(K).to(device)

    # pass two: the depth of every N-th frame, fused batch by batch on the device
    disps = weights = None
    if args.consistency_weight:
        disps, weights = consistency(args, disp_net, files, chosen, c2w, K_dev, used_hw, device, on_weights)
    scales = None
    if args.refine_poses:
        c2w = refine(args, vol, disp_net, files, chosen, c2w, K_dev, device, on_batch, on_track, disps, weights, follow)
        if args.refine_scale:
            c2w, scales = c2w
    for k, imgs, _ in () if args.refine_poses else frames([files[i] for i in chosen], args, device, args.batch_size):
        disp = disp_net(imgs) if disps is None else disps[k:k + len(imgs)]
        idx = torch.tensor(chosen[k:k + len(imgs)], device=device)
        batch = (disp.contiguous(), imgs, c2w[idx].contiguous(), K_dev)
        if follow is not None:
            follow(chain[chosen[k + len(imgs) // 2]])
        if on_batch is not None:
            on_batch(*batch)
        vol.integrate(*batch, is_disp=True, max_depth=args.max_depth,
                      weight=None if weights is None else weights[k:k + len(imgs)])
    xyz, rgb = vol.extract(args.min_weight)
    path = os.path.join(args.output_dir, "reconstruction.ply")
    if args.follow:
        out = sum(len(p[0]) for p in streamed)
        xyz = np.concatenate([p[0] for p in streamed] + [xyz.cpu().numpy()])
        rgb = np.concatenate([p[1] for p in streamed] + [rgb.cpu().numpy()])
    fusion.write_ply(path, xyz, rgb)
    print('{} surface points from {} frames -> {}'.format(len(xyz), len(chosen), path))
    if args.follow:
        print('the window moved {} times to offset ({}, {}, {}); {} of the points were streamed out on the way'.format(
            len(streamed), *vol.offset, out))
    if args.mesh:
        from scsfm_hip import meshing
        path = os.path.join(args.output_dir, "mesh.ply")
        xyz, rgb, tri = vol.extract_mesh(args.min_weight)
        meshing.write_ply_mesh(path, xyz, rgb, tri)
        print('{} vertices, {} triangles -> {}'.format(len(xyz), len(tri), path))
    if novel is not None:
        render(args, vol, disp_net, torch.from_numpy(novel).to(device), K_dev, used_hw, device,
               ['{:06d}'.format(i) for i in range(len(novel))], on_render=on_render)
    elif args.render:
        fused = [files[i] for i in chosen]
        names = [os.path.splitext(os.path.basename(str(f)))[0] for f in fused]
        render(args, vol, disp_net, c2w[torch.tensor(chosen, device=device)], K_dev, used_hw, device, names, files=fused,
               on_render=on_render, scales=None if scales is None else scales[torch.tensor(chosen, device=device)])
    return vol


if __name__ == '__main__':
    main()
