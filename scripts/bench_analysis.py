"""Device analysis throughput (vaenpvc_analyze): audio-seconds per second for one call at about
80 s and 160 s of speech-like synthetic audio (utterances synthesised with Engine.synthesize from varied f0 / sp / ap).
Per-kernel split: run this script under `rocprofv3 --kernel-trace --stats -- python scripts/bench_analysis.py`.

    python scripts/bench_analysis.py [--seconds 80 160] [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'vae-npvc_amd'), ROOT]

from hipvae import world  # noqa: E402
from hipvae.engine import Engine  # noqa: E402

FS, UTT_FRAMES = 16000, 800          # 4 s utterances


def features(T, rng):
    """f0 with voiced runs and pauses, a formant-like envelope that drifts, ap low below 3 kHz in voiced frames."""
    t = np.arange(T)
    f0 = 120 + 60 * np.sin(2 * np.pi * t / rng.uniform(150, 400)) + rng.uniform(-20, 40)
    f0[(t // rng.integers(60, 120)) % 4 == 3] = 0.0
    fr = np.arange(513) * FS / 1024.0
    c1 = 500 + 200 * np.sin(2 * np.pi * t / 90)[:, None]
    c2 = 1500 + 400 * np.sin(2 * np.pi * t / 130)[:, None]
    sp = np.exp(-((fr - c1) / 250) ** 2) + 0.5 * np.exp(-((fr - c2) / 350) ** 2) + 1e-3
    en = sp.sum(1)
    ap = np.tile(np.clip(10 ** ((-40 + 40 * fr / 8000) / 20), 0.001, 1), (T, 1))
    ap[f0 == 0] = 1.0
    return (f0.astype(np.float32), np.log10(sp / en[:, None]).astype(np.float32), en.astype(np.float32),
            ap.astype(np.float32))


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--seconds', type=float, nargs='+', default=[80.0, 160.0])
    p.add_argument('--reps', type=int, default=5)
    a = p.parse_args()
    with open(os.path.join(ROOT, 'vae-npvc_amd', 'architecture-vae-vcc2016.json')) as fp:
        eng = Engine(json.load(fp), device='cuda:0')
    rng = np.random.default_rng(0)
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()   # noqa: E731
    for secs in a.seconds:
        n = max(1, int(round(secs * FS / (UTT_FRAMES * 80))))
        f0, sp, en, ap = (np.concatenate(z) for z in zip(*[features(UTT_FRAMES, rng) for _ in range(n)]))
        y, samples = eng.synthesize(dev(f0), dev(sp), dev(en), dev(ap), [UTT_FRAMES] * n)
        torch.cuda.synchronize()
        world.analyze(y, samples)                                      # warm-up (workspace allocation)
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            world.analyze(y, samples)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        audio = sum(samples) / FS
        med = float(np.median(ms))
        print(json.dumps({'utterances': n, 'audio_s': round(audio, 2), 'frames': sum(world.n_frames(s) for s in samples),
                          'ms_median': round(med, 3), 'ms_min': round(min(ms), 3),
                          'audio_s_per_s': round(audio / (med / 1000.0), 1)}))


if __name__ == '__main__':
    main()
