"""KITTI odometry evaluation -- the reference's kitti_eval/eval_odom.py (same flags, files and printout) on the GPU
(scsfm_hip.odometry.evaluate_odometry), plus --gt-dir and --yes.

    python ./kitti_eval/eval_odom.py --result=results/vo/ --align='7dof' --gt-dir kitti_odom_test/poses/

Writes <result>/result.txt and <result>/errors/NN.txt, and, when matplotlib is installed, the trajectory and error
plots under <result>/plot_path and <result>/plot_error.
"""
import argparse
import os
import sys
from glob import glob

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

parser = argparse.ArgumentParser(description='KITTI evaluation')
parser.add_argument('--result', type=str, required=True,
                    help="Result directory")
parser.add_argument('--align', type=str,
                    choices=['scale', 'scale_7dof', '7dof', '6dof'],
                    default=None,
                    help="alignment type")
parser.add_argument('--seqs',
                    nargs="+",
                    type=int,
                    help="sequences to be evaluated",
                    default=None)
parser.add_argument('--gt-dir', type=str, default="./kitti_eval/gt_poses/",
                    help="ground truth poses (KITTI's NN.txt)")
parser.add_argument('--yes', action='store_true', help="do not ask before evaluating")


def load_poses_from_txt(file_name):
    """KITTI's format: 12 numbers per line (3x4, row-major), optionally preceded by a frame index.  -> [n, 12]"""
    rows = []
    with open(file_name) as f:
        for line in f:
            v = [float(x) for x in line.split(" ") if x.strip() != ""]
            if v:
                rows.append(v[len(v) - 12:])
    return np.array(rows, np.float64).reshape(-1, 12)


def plot(result_dir, res):
    try:
        import matplotlib
        matplotlib.use("Agg")
        from matplotlib import pyplot as plt
    except ImportError:
        print("matplotlib is not installed: no plots")
        return
    for d in ("plot_path", "plot_error"):
        os.makedirs(os.path.join(result_dir, d), exist_ok=True)
    for i, seq in enumerate(res.seqs):
        fig = plt.figure()
        plt.gca().set_aspect('equal')
        for key, poses in (("Ground Truth", res.gt_rel[i]), ("Ours", res.aligned[i])):
            plt.plot(poses[:, 0, 3], poses[:, 2, 3], label=key)
        plt.legend(loc="upper right", prop={'size': 20})
        plt.xticks(fontsize=20)
        plt.yticks(fontsize=20)
        plt.xlabel('x (m)', fontsize=20)
        plt.ylabel('z (m)', fontsize=20)
        fig.set_size_inches(10, 10)
        plt.savefig(os.path.join(result_dir, "plot_path", "sequence_{:02}.pdf".format(seq)), bbox_inches='tight',
                    pad_inches=0)
        plt.close(fig)
        errs = res.avg_segment_errs(i)
        for name, label, ylabel, k, factor in (("trans_err", "Translation Error", 'Translation Error (%)', 0, 100.0),
                                               ("rot_err", "Rotation Error", 'Rotation Error (deg/100m)', 1,
                                                180 / np.pi * 100)):
            fig = plt.figure()
            plt.plot(list(errs), [e[k] * factor if e else 0 for e in errs.values()], "bs-", label=label)
            plt.ylabel(ylabel, fontsize=10)
            plt.xlabel('Path Length (m)', fontsize=10)
            plt.legend(loc="upper right", prop={'size': 10})
            fig.set_size_inches(5, 5)
            plt.savefig(os.path.join(result_dir, "plot_error", "{}_{:02}.pdf".format(name, seq)), bbox_inches='tight',
                        pad_inches=0)
            plt.close(fig)


def evaluate(gt_dir, result_dir, alignment=None, seqs=None):
    from scsfm_hip.odometry import evaluate_odometry
    seq_list = ["{:02}".format(i) for i in range(0, 11)]
    if seqs is None:
        available = sorted(glob(os.path.join(result_dir, "*.txt")))
        seqs = [int(i[-6:-4]) for i in available if i[-6:-4] in seq_list]
    os.makedirs(os.path.join(result_dir, "errors"), exist_ok=True)
    pred = [load_poses_from_txt(result_dir + "/" + '{:02}.txt'.format(i)) for i in seqs]
    gt = [load_poses_from_txt(gt_dir + "/" + '{:02}.txt'.format(i)) for i in seqs]
    res = evaluate_odometry(gt, pred, alignment, seqs) if seqs else None
    with open(os.path.join(result_dir, "result.txt"), 'w') as f:
        f.write(res.result_txt() if res else "")
    if res is None:
        print("-------------------- For Copying ------------------------------")
        return None
    for k, i in enumerate(seqs):
        with open(os.path.join(result_dir, "errors", '{:02}.txt'.format(i)), 'w') as f:
            f.write(res.segment_errors(k))
    print("\n".join(res.report_lines()))
    plot(result_dir, res)
    print("\n".join(res.copy_block()))
    return res


def main(argv=None):
    args = parser.parse_args(argv)
    result_dir = args.result
    continue_flag = "y" if args.yes else input("Evaluate result in {}? [y/n]".format(result_dir))
    if continue_flag == "y":
        evaluate(args.gt_dir, result_dir, alignment=args.align, seqs=args.seqs)
    else:
        print("Double check the path!")


if __name__ == '__main__':
    main()
