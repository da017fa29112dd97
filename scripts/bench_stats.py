"""Time of the device statistics of build.py --device (hipvae.stats) with the inputs resident in HBM.
Usage: python scripts/bench_stats.py [--frames 1048576] [--iterations 10] [--train_file_pattern '.../*/*.bin'] [--no-host]

Synthetic records by default: F frames x 513 bins of 3 N(0, 1) - 8, utterances of about 680 frames dealt round robin to
10 speakers, 70 % voiced frames; with --train_file_pattern the frames of those .bin files instead.  One JSON line each:
  column_select   seconds per call for the four ranks of the 0.5 / 99.5 percentiles, the number of passes the select made
                  over x (1 + per further radix pass the distinct prefixes alive, averaged over the 64-column groups; derived
                  from the selected values), bytes read / second and that rate against the 6.3 TB/s copy rate
  speaker_stats   seconds per call, against two reads of sp
  host            seconds of the host path's two np.percentile calls on the same array (skipped by --no-host)
Run under `rocprofv3 --kernel-trace --stats` for the per-kernel split."""
import argparse
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'vae-npvc_amd'))
import torch  # noqa: E402
from hipvae import stats  # noqa: E402

COPY_RATE = 6.3e12      # bytes / s, the copy rate DESIGN.md section 13 uses
H = 513


def select_passes(vals):
    """Passes over x that column_select made for the selected values vals [n_rank, H] (float32): the first 8 key bits
    are one pass shared by every rank; each further pass runs once per slot that leads a distinct prefix in at least one
    column of a 64-column group."""
    b = vals.view(np.uint32)
    key = np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000))
    total = 1.0
    for p in (1, 2, 3):
        top = key >> np.uint32(32 - 8 * p)
        leads = np.stack([~np.any(top[:r] == top[r], axis=0) for r in range(len(top))])       # [n_rank, H]
        groups = [leads[:, c:c + 64].any(axis=1).sum() for c in range(0, leads.shape[1], 64)]
        total += float(np.mean(groups))
    return total


def timed(fn, iterations):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iterations):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iterations


def load_files(pattern):
    files = sorted(glob.glob(pattern))
    recs = [np.fromfile(f, '<f4').reshape(-1, 1029) for f in files]
    lengths = [len(r) for r in recs]
    x = torch.empty(sum(lengths), H, device='cuda:0')
    f0 = torch.empty(sum(lengths), device='cuda:0')
    o = 0
    for r in recs:
        x[o:o + len(r)].copy_(torch.from_numpy(r[:, :H]))
        f0[o:o + len(r)].copy_(torch.from_numpy(r[:, 1026]))
        o += len(r)
    return x, f0, lengths, [int(r[0, -1]) if len(r) else 0 for r in recs]


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--frames', type=int, default=1 << 20)
    p.add_argument('--iterations', type=int, default=10)
    p.add_argument('--train_file_pattern', default=None)
    p.add_argument('--no-host', action='store_true')
    args = p.parse_args()
    if args.train_file_pattern:
        x, f0, lengths, speakers = load_files(args.train_file_pattern)
    else:
        g = torch.Generator(device='cuda:0').manual_seed(0)
        F = args.frames
        x = torch.randn(F, H, device='cuda:0', generator=g) * 3 - 8
        f0 = torch.rand(F, device='cuda:0', generator=g) * 220 + 80
        f0[torch.rand(F, device='cuda:0', generator=g) < 0.3] = 0
        n = max(1, F // 680)
        lengths = [F // n + (1 if u < F % n else 0) for u in range(n)]
        speakers = [u % 10 for u in range(n)]
    F = x.shape[0]
    ranks = [r for lo, hi, _ in stats.percentile_ranks(F, [0.5, 99.5]) for r in (lo, hi)]
    vals = stats.column_select(x, ranks).cpu().numpy()
    passes = select_passes(vals)
    sec = timed(lambda: stats.column_select(x, ranks), args.iterations)
    nbytes = passes * F * H * 4
    print(json.dumps({'path': 'column_select', 'frames': F, 'ranks': ranks, 'seconds_per_call': sec, 'passes_over_x': passes,
                      'bytes_per_second': nbytes / sec, 'of_copy_rate': nbytes / sec / COPY_RATE}), flush=True)
    sec = timed(lambda: stats.speaker_stats(x, f0, lengths, speakers, 10), args.iterations)
    print(json.dumps({'path': 'speaker_stats', 'frames': F, 'utterances': len(lengths), 'seconds_per_call': sec,
                      'bytes_per_second': 2 * F * H * 4 / sec, 'of_copy_rate': 2 * F * H * 4 / sec / COPY_RATE}), flush=True)
    if not args.no_host:
        xh = x.cpu().numpy()
        t0 = time.perf_counter()
        lo = np.percentile(xh, 0.5, axis=0).astype(np.float32)
        hi = np.percentile(xh, 99.5, axis=0).astype(np.float32)
        host = time.perf_counter() - t0
        dev = stats.percentiles(x, [0.5, 99.5]).cpu().numpy()
        print(json.dumps({'path': 'host', 'frames': F, 'seconds_two_np_percentile': host,
                          'max_abs_host_minus_device': float(np.abs(np.stack([lo, hi]) - dev).max())}), flush=True)


if __name__ == '__main__':
    main()
