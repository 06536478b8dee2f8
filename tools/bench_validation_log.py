"""Times one picture set of train.py --log-output (no dataset and no network needed): from a normalised input
[1, 3, 256, 832] and the network's disparity [1, 1, 256, 832] on the device to the three byte pictures on the host (the
input, the disparity in magma over its own maximum, the depth in rainbow over 10); writing the PNG files is the same
work on both paths and is left out.

    python tools/bench_validation_log.py [--reps 15] [--out profiles/validation_log_bench.json]

  library   scsfm_hip.validation_log.input_pictures / map_pictures (bytes only) and one copy of each picture's bytes: the
            maximum, the division, the table lookup and the byte conversion stay on the device
  host      the reference's chain per picture -- tensor.detach().cpu(), .max().item(), numpy's division, the matplotlib
            colour map (magma interpolated to 1000 entries, the rainbow of scsfm_hip.visualise's stops with 1000),
            float32, transpose -- and then the bytes of the float picture
Both are timed with the host clock between device synchronisations (both end in host memory), after a warm-up of each,
alternating in one process, over eight different picture sets: median, minimum and maximum of the repetitions.  The
pictures of the two paths are compared byte for byte on every set.  Writes one JSON file.  Needs a HIP device and
matplotlib."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sc-sfmlearner-release_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W = 256, 832
DISTINCT = 8


def host_maps():
    import matplotlib
    from matplotlib.colors import LinearSegmentedColormap, ListedColormap
    from scsfm_hip import visualise
    low = matplotlib.colormaps["magma"]
    x = np.linspace(0, 1, low.N)
    entries = low(x)
    new_x = np.linspace(0, 1, 1000)
    magma = ListedColormap(np.stack([np.interp(new_x, x, entries[:, i]) for i in range(entries.shape[1])], axis=1))
    return {"magma": magma, "rainbow": LinearSegmentedColormap.from_list("opencv_rainbow", visualise._RAINBOW, 1000)}


def host_picture(tensor, cmap=None, max_value=None):
    """What the reference's tensor2array does with a device tensor: fetch it, then for a map (a colour map is given) read
    its maximum back as a Python float, divide in numpy and look the colours up in matplotlib; for the input, undo the
    normalisation.  float32 [C, H, W]."""
    fetched = tensor.detach().cpu()
    if cmap is None:
        return fetched.numpy() * 0.225 + 0.45
    divisor = fetched.max().item() if max_value is None else max_value
    return cmap(fetched.numpy() / divisor).astype(np.float32).transpose(2, 0, 1)


def make_set(rng, dev):
    """A frame of random bytes, normalised, and a disparity like DispResNet's (sigmoid-scaled, nearer towards the bottom
    rows)."""
    frame = rng.integers(0, 256, (1, 3, H, W)).astype(np.float32)
    img = ((torch.from_numpy(frame) / 255 - 0.45) / 0.225).to(dev)
    ramp = np.linspace(0.02, 0.6, H, dtype=np.float32)[None, None, :, None]
    disp = (ramp * rng.uniform(0.7, 1.4, (1, 1, H, W))).astype(np.float32) + np.float32(0.01)
    return img, torch.from_numpy(disp).to(dev)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "validation_log_bench.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_validation_log.py needs a HIP device")
    from scsfm_hip import validation_log as VL
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    sets = [make_set(rng, dev) for _ in range(DISTINCT)]
    cmaps = host_maps()

    def library(img, disp):
        return (VL.input_pictures(img, floats=False)[1][0].cpu().numpy(),
                VL.map_pictures(disp[0], "magma", None, floats=False)[1][0].cpu().numpy(),
                VL.map_pictures(1 / disp[0], "rainbow", 10, floats=False)[1][0].cpu().numpy())

    def host(img, disp):
        arrays = (host_picture(img[0]), host_picture(disp[0, 0], cmaps["magma"]),
                  host_picture(1 / disp[0, 0], cmaps["rainbow"], 10))
        return tuple(np.ascontiguousarray(VL.to_bytes(a).transpose(1, 2, 0)) for a in arrays)

    def timed(fn, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(*sets[k % DISTINCT])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    differing = 0
    for s in sets:  # (also the warm-up of both paths)
        differing += sum(int((a != b).sum()) for a, b in zip(library(*s), host(*s)))

    runs = {"library": [], "host": []}
    for k in range(args.reps):
        runs["library"].append(timed(library, k))
        runs["host"].append(timed(host, k))

    def stats(v):
        return {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v)),
                "runs_ms": [float(x) for x in v]}

    result = {"device": torch.cuda.get_device_name(0), "height": H, "width": W, "pictures_per_set": 3,
              "reps": args.reps, "host_threads": torch.get_num_threads(),
              "one_set": {k: stats(v) for k, v in runs.items()},
              "ratio_host_over_library": float(np.median(runs["host"]) / np.median(runs["library"])),
              "differing_bytes": differing, "compared_sets": DISTINCT}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
    if differing:
        raise SystemExit(f"the pictures of the two paths differ in {differing} bytes")


if __name__ == "__main__":
    main()
