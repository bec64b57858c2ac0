"""The reference's dataset down-sampling scripts (data/Kitti/downsample_pcd.py, data/Kitti_360/downsample_pcd.py,
data/mulran/downsample_pcd_mulran.py) on the GPU: Open3D's voxel_down_sample(0.3) through lcr_voxel_down_sample.

    python tools/downsample_run.py --root KITTI_ROOT [--seqs 00 01 ...] [--xyz-only]
        reads  KITTI_ROOT/sequences/<seq>/velodyne/*.bin      (f32 [N,4]: x, y, z, intensity)
        writes KITTI_ROOT/downsampled_xyzi/<seq>/<frame>.npy  (f32 [M,4]: averaged x, y, z, intensity; [M,3] with --xyz-only)
    python tools/downsample_run.py --synthetic 2048
        times it without a dataset: synthetic scans plus a deterministic intensity column, 8 and 64 scans per call, and the fp64
        NumPy restatement on one core as the CPU baseline (Open3D itself is not used).  Prints one JSON line.
"""
import argparse
import concurrent.futures as cf
import glob
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VOXEL = 0.3


def _calls(rows_list, per_call, out_cols):
    """Yields (scan indices, f32 [M, out_cols] on the host, lengths) for groups of `per_call` scans."""
    from lcrnet_amd.downsample import voxel_down_sample
    for g in range(0, len(rows_list), per_call):
        grp = rows_list[g:g + per_call]
        rows = torch.from_numpy(np.concatenate(grp)).cuda(non_blocking=True)
        lens = torch.tensor([len(r) for r in grp], dtype=torch.int64, device="cuda")
        out, _, _, lh = voxel_down_sample(rows, lens, VOXEL, out_cols)
        yield range(g, g + len(grp)), out.cpu().numpy(), lh


def run_dataset(args):
    out_cols = 3 if args.xyz_only else 4
    seqs = args.seqs or sorted(os.path.basename(p) for p in glob.glob(os.path.join(args.root, "sequences", "*")))
    n_files, t0 = 0, time.perf_counter()
    with cf.ThreadPoolExecutor(max_workers=args.io_threads) as pool:
        for seq in seqs:
            files = sorted(glob.glob(os.path.join(args.root, "sequences", seq, "velodyne", "*.bin")))
            out_dir = os.path.join(args.root, "downsampled_xyzi", seq)
            os.makedirs(out_dir, exist_ok=True)
            for f0 in range(0, len(files), args.per_call):
                names = files[f0:f0 + args.per_call]
                rows = list(pool.map(lambda f: np.fromfile(f, dtype=np.float32).reshape(-1, 4), names))
                for idx, out, lh in _calls(rows, args.per_call, out_cols):
                    o, writes = 0, []
                    for k, n in zip(idx, lh):
                        frame = os.path.basename(names[k])[:-4]
                        writes.append(pool.submit(np.save, os.path.join(out_dir, frame + ".npy"), out[o:o + n]))
                        o += n
                    for w in writes:
                        w.result()
                n_files += len(names)
    dt = time.perf_counter() - t0
    print(json.dumps({"metric": "voxel_down_sample files", "scans": n_files, "seconds": round(dt, 3), "scans_per_s": round(n_files / max(dt, 1e-9), 1),
                      "layout": "downsampled_xyzi/<seq>/<frame>.npy f32 [M,%d]" % out_cols}), flush=True)


def run_synthetic(args):
    import lcrnet_amd.synthetic as synthetic
    from lcrnet_amd.downsample import voxel_down_sample
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from o3d_voxel_restatement import voxel_down_sample as restate
    base = []
    for u in range(args.unique):
        xyz = synthetic.synthetic_scan(2000 + u)
        inten = ((np.arange(len(xyz)) * 37 + u) % 101).astype(np.float32) / np.float32(101.0)
        base.append(np.ascontiguousarray(np.concatenate([xyz, inten[:, None]], axis=1)))
    out_cols = 3 if args.xyz_only else 4
    res = {"metric": "voxel_down_sample (Open3D semantics), synthetic raw scans", "scans": args.synthetic, "voxel": VOXEL,
           "raw_points_per_scan": int(np.mean([len(b) for b in base])), "out_cols": out_cols}
    for per_call in (8, 64):
        groups = []
        for g in range(0, args.synthetic, per_call):
            grp = [base[(g + k) % len(base)] for k in range(min(per_call, args.synthetic - g))]
            groups.append((torch.from_numpy(np.concatenate(grp)).cuda(), torch.tensor([len(r) for r in grp], dtype=torch.int64, device="cuda")))
        for rows, lens in groups[:2]:                     # warm-up (library load, LDS opt-in, allocator)
            voxel_down_sample(rows, lens, VOXEL, out_cols)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for rows, lens in groups:
            voxel_down_sample(rows, lens, VOXEL, out_cols)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        res["scans_per_s_at_%d" % per_call] = round(args.synthetic / dt, 1)
        res["ms_per_call_at_%d" % per_call] = round(dt / len(groups) * 1e3, 3)
    n_cpu = min(args.cpu_scans, len(base))
    t0 = time.perf_counter()
    for b in base[:n_cpu]:
        restate(b, VOXEL, out_cols)
    dt = time.perf_counter() - t0
    res["cpu_baseline"] = "the fp64 NumPy restatement (tests/o3d_voxel_restatement.py) on one core; Open3D is not installed"
    res["cpu_scans_per_s"] = round(n_cpu / dt, 2)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=None, help="KITTI-style dataset root (sequences/<seq>/velodyne/*.bin)")
    ap.add_argument("--seqs", nargs="*", default=None)
    ap.add_argument("--xyz-only", action="store_true", help="write [M,3] (MulRan's layout) instead of [M,4]")
    ap.add_argument("--per-call", type=int, default=64, help="scans per native call (<= 64)")
    ap.add_argument("--io-threads", type=int, default=4)
    ap.add_argument("--synthetic", type=int, default=0, help="time N synthetic scans instead of reading a dataset")
    ap.add_argument("--unique", type=int, default=16, help="distinct synthetic scans")
    ap.add_argument("--cpu-scans", type=int, default=4, help="scans timed through the CPU restatement")
    args = ap.parse_args()
    if not 1 <= args.per_call <= 64:
        ap.error("--per-call must be 1..64")
    if args.synthetic:
        run_synthetic(args)
    elif args.root:
        run_dataset(args)
    else:
        ap.error("give --root or --synthetic")


if __name__ == "__main__":
    main()
