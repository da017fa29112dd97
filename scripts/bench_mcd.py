"""Time of the device MCD / DTW call (hipvae.metrics.mcd_dtw).
Usage: python scripts/bench_mcd.py [--sizes 54x700 8x4000] [--iterations 10] [--ref-frames 700]

Per size PxT: P pairs of about T frames per side (each side's length drawn within +-10 % of T, capped at 4096), smooth
random-walk spectra.  One JSON line per size: microseconds per call (one call evaluates the whole set), cells and
workspace bytes.  As a yardstick, the float64 NumPy restatement (tests/mcd_ref.py, written for clarity, not a tuned
baseline) is timed on the host on ONE pair of --ref-frames x --ref-frames frames.  Run under
`rocprofv3 --kernel-trace --stats` for the per-kernel split."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'vae-npvc_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from hipvae import metrics  # noqa: E402


def side(T, rng):
    k = np.arange(513) / 512.0
    c = 0.3 * rng.standard_normal(16) + np.cumsum(0.05 * rng.standard_normal((T, 16)), 0)
    sp = -6.0 - 2.5 * k[None] + sum(c[:, q:q + 1] * np.cos((q + 1) * np.pi * k)[None] / (1 + 0.3 * q) for q in range(16))
    f0 = np.where(rng.random(T) < 0.7, rng.uniform(80, 300, T), 0.0)
    return sp.astype(np.float32), rng.uniform(100.0, 2000.0, T).astype(np.float32), f0.astype(np.float32)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--sizes', nargs='+', default=['54x700', '8x4000'])
    p.add_argument('--iterations', type=int, default=10)
    p.add_argument('--ref-frames', type=int, default=700)
    args = p.parse_args()
    for size in args.sizes:
        P, T = (int(v) for v in size.split('x'))
        rng = np.random.default_rng(P * 10007 + T)
        draw = lambda: int(min(metrics.MAX_FRAMES, max(1, rng.integers(int(0.9 * T), int(1.1 * T) + 1))))   # noqa: E731
        la, lb = [draw() for _ in range(P)], [draw() for _ in range(P)]
        A, B = [side(t, rng) for t in la], [side(t, rng) for t in lb]
        a = [torch.from_numpy(np.concatenate([s[q] for s in A])).cuda() for q in range(3)]
        b = [torch.from_numpy(np.concatenate([s[q] for s in B])).cuda() for q in range(3)]
        call = lambda: metrics.mcd_dtw(a[0], a[1], a[2], la, b[0], b[1], b[2], lb)   # noqa: E731
        res = call()
        torch.cuda.synchronize()
        cells = sum(x * y for x, y in zip(la, lb))
        ws = int(metrics.layout(P, sum(la), sum(lb), cells, 24)['bytes'])
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(3):
            call()
        start.record()
        for _ in range(args.iterations):
            call()
        end.record()
        torch.cuda.synchronize()
        us = start.elapsed_time(end) * 1e3 / args.iterations
        r = res.cpu().numpy()
        print(json.dumps({'path': 'mcd_dtw', 'pairs': P, 'frames_a': sum(la), 'frames_b': sum(lb), 'cells': cells,
                          'us_per_call': us, 'cells_per_us': cells / us, 'workspace_bytes': ws,
                          'mean_mcd_db': float(r[:, 0].mean()), 'mean_path': float(r[:, 1].mean())}), flush=True)
    if args.ref_frames > 0:
        import mcd_ref as R
        rng = np.random.default_rng(1)
        sa, sb = side(args.ref_frames, rng), side(args.ref_frames, rng)
        W = R.mcep_matrix()
        t0 = time.perf_counter()
        R.mcd_pair(*sa, *sb, W=W)
        print(json.dumps({'path': 'numpy_restatement_one_pair', 'frames': args.ref_frames,
                          'seconds': time.perf_counter() - t0}), flush=True)


if __name__ == '__main__':
    main()
