"""Time of the device resampler (hipvae.resample) with the waveforms resident in HBM.
Usage: python scripts/bench_resample.py [--seconds 600] [--utterance_seconds 3.5] [--iterations 9] [--host_seconds 10]

Synthetic corpus: --seconds of audio per rate in utterances of about --utterance_seconds (uniform noise in [-1, 1); the
kernel's work does not depend on the data), resampled 48 000 -> 16 000 and 44 100 -> 16 000 in one call each.  One JSON
line per rate:
  seconds_per_call     median of --iterations calls, each timed with device events after two warm-up calls (min and max too)
  fma_per_second       the float64 fused multiply-adds the definition needs, n_out * 2K, over that time, and of_fp64_vector
                       = that rate against the chip's vector FP64 rate (78.6 TFLOP/s in the data sheet = 39.3e12 FMA/s)
  bytes_compulsory     x read once, y written once, the table read once; lanes_table_bytes = n_out * 2K * 8, what the
                       lanes ask the cache for
  host                 the same definition in NumPy (tests/resample_ref.py) on the first --host_seconds of the corpus:
                       seconds, audio seconds per second, and the device's largest distance from it in float32 ulp
Run under `rocprofv3 --kernel-trace --stats` for the kernel's own time."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'vae-npvc_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402
import resample_ref  # noqa: E402
from hipvae import resample as RS  # noqa: E402

FP64_FMA_RATE = 78.6e12 / 2      # vector FP64, data sheet
FS = 16000


def device_times(fn, iterations):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(iterations):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e-3)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--seconds', type=float, default=600.0)
    p.add_argument('--utterance_seconds', type=float, default=3.5)
    p.add_argument('--iterations', type=int, default=9)
    p.add_argument('--host_seconds', type=float, default=10.0)
    p.add_argument('--rates', type=int, nargs='+', default=[48000, 44100])
    args = p.parse_args()
    for rate in args.rates:
        up, down, half = RS.plan(rate, FS)
        n_utt = max(1, int(round(args.seconds / args.utterance_seconds)))
        rng = np.random.default_rng(rate)
        lengths = [int(v) for v in rng.integers(int(0.6 * args.utterance_seconds * rate),
                                                int(1.4 * args.utterance_seconds * rate) + 1, n_utt)]
        g = torch.Generator(device='cuda:0').manual_seed(rate)
        x = torch.rand(sum(lengths), device='cuda:0', generator=g) * 2 - 1
        y, outs = RS.resample(x, lengths, rate, FS)
        torch.cuda.synchronize()
        t = device_times(lambda: RS.resample(x, lengths, rate, FS), args.iterations)
        sec = float(np.median(t))
        n_out = sum(outs)
        fma = n_out * 2 * half
        nbytes = 4 * x.numel() + 4 * n_out + 8 * 2 * half * up
        res = {'path': 'resample', 'rate_in': rate, 'rate_out': FS, 'L': up, 'M': down, 'taps': 2 * half,
               'utterances': n_utt, 'audio_seconds': x.numel() / rate, 'samples_in': x.numel(), 'samples_out': n_out,
               'seconds_per_call': sec, 'seconds_min': min(t), 'seconds_max': max(t),
               'audio_seconds_per_second': x.numel() / rate / sec, 'fma': fma, 'fma_per_second': fma / sec,
               'of_fp64_vector': fma / sec / FP64_FMA_RATE, 'bytes_compulsory': nbytes,
               'bytes_compulsory_per_second': nbytes / sec, 'lanes_table_bytes': fma * 8}
        if args.host_seconds > 0:
            k, s = 0, 0
            while k < len(lengths) and (k == 0 or s + lengths[k] <= args.host_seconds * rate):
                s += lengths[k]
                k += 1
            xs = np.split(x[:s].cpu().numpy(), np.cumsum(lengths[:k])[:-1])
            t0 = time.perf_counter()
            ref = resample_ref.resample(xs, rate, FS)
            host = time.perf_counter() - t0
            got = y[:sum(outs[:k])].cpu().numpy()
            want = np.concatenate(ref)
            ulp = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
            res['host'] = {'audio_seconds': s / rate, 'seconds_numpy_restatement': host,
                           'audio_seconds_per_second': s / rate / host, 'device_max_ulp_from_it': float(ulp.max())}
        print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
