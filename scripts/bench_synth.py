"""Throughput of the device vocoder (Engine.synthesize) at 16 kHz, 5 ms frames.
Usage: python scripts/bench_synth.py [--frames 16384 32768] [--iterations 20] [--ref-frames 2048]

Per size: utterances of 300 to 1 100 frames (20 to 50 of them) with voiced runs (80-300 Hz, vibrato, octave jumps) and
unvoiced runs, envelopes and aperiodicities of .bin-like ranges.  One JSON line per size: microseconds per call (one
call synthesises the whole batch), seconds of audio per second, pulses and workspace bytes.  As a yardstick, the float64
NumPy restatement (tests/world_ref.py) is timed on the host over the first utterances of the batch (at least
--ref-frames frames) and reported in seconds of audio per second as well."""
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
from hipvae.engine import Engine  # noqa: E402

FS, FP = 16000, 5.0


def make_batch(F, rng):
    lengths = []
    while sum(lengths) < F:
        lengths.append(int(rng.integers(300, 1100)))
    lengths[-1] -= sum(lengths) - F
    if lengths[-1] < 1:
        lengths[-2] += lengths.pop()
    f0 = np.zeros(F)
    t = 0
    while t < F:
        n = min(int(rng.integers(10, 80)), F - t)
        if rng.random() < 0.65:
            s = np.arange(n)
            f0[t:t + n] = rng.uniform(80, 300) * (1 + 0.04 * np.sin(s / 6.0)) * np.where(rng.random() < 0.1, 2.0, 1.0)
        t += n
    k = np.arange(513) / 513
    sp = rng.uniform(-8.0, -6.0, (F, 1)) - 2.5 * k[None, :] + 0.4 * np.sin(2 * np.pi * k[None, :] * rng.uniform(2, 6, (F, 1)))
    en = rng.uniform(200.0, 3000.0, F)
    ap = np.clip(k[None, :] ** 0.5 * np.where(f0[:, None] > 0, rng.uniform(0.1, 0.8, (F, 1)), 1.0), 0, 1)
    return lengths, [a.astype(np.float32) for a in (f0, sp, en, ap)]


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--frames', type=int, nargs='+', default=[16384, 32768])
    p.add_argument('--iterations', type=int, default=20)
    p.add_argument('--ref-frames', type=int, default=2048)
    args = p.parse_args()
    with open(os.path.join(ROOT, 'vae-npvc_amd', 'architecture-vae-vcc2016.json')) as fp:
        eng = Engine(json.load(fp))
    for F in args.frames:
        rng = np.random.default_rng(F)
        lengths, host = make_batch(F, rng)
        f0, sp, en, ap = (torch.from_numpy(a).cuda() for a in host)
        call = lambda: eng.synthesize(f0, sp, en, ap, lengths, fs=FS, frame_period=FP)   # noqa: E731
        y, samples = call()
        torch.cuda.synchronize()
        n_seg = len(lengths)
        pulses = int(eng._synth_ws[:4 * n_seg].view(torch.int32).sum())    # workspace head: pulses kept per utterance
        ws = int(eng.lib.vaenpvc_synth_workspace_bytes(n_seg, sum(samples), 513, FS))
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(3):
            call()
        start.record()
        for _ in range(args.iterations):
            call()
        end.record()
        torch.cuda.synchronize()
        us = start.elapsed_time(end) * 1e3 / args.iterations
        audio = sum(samples) / FS
        # host float64 restatement on the first utterances (at least --ref-frames frames)
        import world_ref as W
        n_ref, fr = 0, 0
        while fr < min(args.ref_frames, F):
            fr += lengths[n_ref]
            n_ref += 1
        t0 = time.perf_counter()
        W.batch(*(a[:fr] for a in host), lengths[:n_ref], fs=FS, frame_period=FP)
        ref_s = time.perf_counter() - t0
        print(json.dumps({'path': 'synthesize', 'frames': F, 'utterances': n_seg, 'audio_s': audio, 'us_per_call': us,
                          'audio_s_per_s': audio / (us * 1e-6), 'pulses': pulses, 'workspace_bytes': ws,
                          'ref_host_frames': fr, 'ref_host_audio_s_per_s': fr * FP / 1000.0 / ref_s}), flush=True)


if __name__ == '__main__':
    main()
