"""Throughput of the conversion path (convert.py:60-63,79-89): encode(x) -> z_mu, decode(z_mu, target speaker)
on frames resident in HBM.  Usage: python scripts/bench_convert.py [frames] [iterations] [--gv N_UTT]

--gv N_UTT adds the output stage in the same process: the inverse Tanhize (what convert.py runs by default) against the
global-variance post-filter (convert.py --gv) over N_UTT utterances of frames / N_UTT frames each, alone and behind
encode + decode."""
import argparse
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'vae-npvc_amd'))
import torch
from hipvae.engine import Engine

ap = argparse.ArgumentParser()
ap.add_argument('frames', nargs='?', type=int, default=32768)
ap.add_argument('iterations', nargs='?', type=int, default=20)
ap.add_argument('--gv', type=int, default=None, metavar='N_UTT')
args = ap.parse_args()
arch = json.load(open(os.path.join(ROOT, 'vae-npvc_amd', 'architecture-vae-vcc2016.json')))
F, iters = args.frames, args.iterations
eng = Engine(arch)
eng.init_params(0)
g = torch.Generator().manual_seed(0)
x = (torch.rand(F, 513, generator=g) * 2 - 1).cuda()
y = torch.full((F,), 9, dtype=torch.int64).cuda()


def timed(fn, n):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


dt = timed(lambda: eng.decode(eng.encode(x), y), iters)
print(json.dumps({'path': 'encode+decode (conversion)', 'frames': F, 'ms': dt * 1e3, 'frames_per_s': F / dt,
                  'algorithmic_tflops': F * 9.419e6 / dt / 1e12}))

if args.gv:
    n_utt = args.gv
    lengths = [F // n_utt + (1 if i < F % n_utt else 0) for i in range(n_utt)]
    xmin = (torch.rand(513, generator=g) * 4 - 12).cuda()
    xmax = xmin + (torch.rand(513, generator=g) * 5 + 2).cuda()
    gv = (torch.rand(513, generator=g) * 0.3 + 0.05).cuda() ** 2
    stages = {'tanhize_bwd': lambda t: eng.tanhize(t, xmin, xmax, forward=False),
              'gv_postfilter': lambda t: eng.gv_postfilter(t, lengths, xmin, xmax, gv)}
    xh = eng.decode(eng.encode(x), y)
    passes = {'tanhize_bwd': 2, 'gv_postfilter': 3}      # passes over F x 513 x 4 B: read x (twice for GV), write sp
    for name, stage in stages.items():
        ds = timed(lambda: stage(xh), max(iters, 100))
        dc = timed(lambda: stage(eng.decode(eng.encode(x), y)), iters)
        print(json.dumps({'path': 'encode+decode+' + name, 'frames': F, 'utterances': n_utt, 'stage_us': ds * 1e6,
                          'stage_GBps': passes[name] * F * 513 * 4 / ds / 1e9, 'ms': dc * 1e3, 'frames_per_s': F / dc}))
