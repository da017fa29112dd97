"""Statistics builder (the reference's build.py:15-65, plus the global-variance statistics it lacks):

    python build.py --train_file_pattern './dataset/vcc2016/bin/Training Set/*/*.bin' [--device]

writes under ./etc
    <spk>.npf      log-F0 mean and std over the speaker's frames with f0 > 2 (float32 [2], build.py:41-51)
    xmin.npf       per-bin 0.5 / 99.5 percentiles of sp over every training frame (build.py:57-65), float32 [513] on
    xmax.npf       disk whatever NumPy's percentile returns (the reference writes that dtype as is; SURVEY trap T4)
    <spk>_gv.npf   (not in the reference) global variance: per bin, the mean over the speaker's utterances of N >= 2
                   frames of the utterance's biased sp variance; computed in float64, stored float32 [513]
                   (read by `convert.py --gv`)

Default: one-shot host NumPy, which imports neither torch nor the HIP library.  Differences
from the reference: the files are read in sorted order (the reference's queue shuffles them); a file whose speaker
column is not constant is an error; a speaker without training files gets no files and a printed note (the reference
writes NaN statistics for it).

--device: the same files, checks, messages and outputs, computed on the GPU (hipvae.stats).  The
frame count comes from the file sizes, the frames go file by file into one device tensor, and the statistics are float64
on the device, rounded once to float32.  Two differences from the host path: a NaN or Inf in sp raises (the non-finite
flag of the select; the host path writes NaN percentiles), and the percentiles are the float64 interpolation
a + (b - a) g between the two bracketing order statistics (NumPy interpolates float32 input with a float32 fraction,
whose error grows with the frame count).
"""
import argparse
import glob
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, _HERE)

SP_DIM = 513
FEAT_DIM = SP_DIM + SP_DIM + 1 + 1 + 1      # [sp, ap, f0, en, s]: analyzer.FEAT_DIM


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--train_file_pattern', default='./dataset/vcc2016/bin/Training Set/*/*.bin',
                   help='training dir (to *.bin)')
    p.add_argument('--device', action='store_true',
                   help='compute the statistics on the GPU (float64 percentiles; non-finite sp is an error)')
    return p.parse_args(argv)


def load_speakers():
    """etc/speakers.tsv, as analyzer.SPEAKERS (read here so that the host path does not import torch through analyzer)."""
    with open(os.path.join(_HERE, 'etc', 'speakers.tsv')) as fp:
        return [s.strip() for s in fp.readlines() if s.strip()]


def read_whole_features(file_pattern):
    """analyzer.read_whole_features for one epoch: one dict per utterance file, in sorted order."""
    files = sorted(glob.glob(file_pattern))
    print('{} files found'.format(len(files)))
    for f in files:
        print('Processing {}'.format(f), flush=True)
        v = np.fromfile(f, '<f4').reshape(-1, FEAT_DIM)
        yield {
            'sp': v[:, :SP_DIM],
            'f0': v[:, SP_DIM * 2],
            'speaker': v[:, SP_DIM * 2 + 2].astype(np.int64),
            'filename': f.encode('utf8'),
        }


def check_speaker_column(name, spk, n_speakers):
    if spk.size and np.any(spk != spk[0]):
        raise ValueError('%s: speaker column is not constant (%s)' % (name, sorted(set(spk.tolist()))))
    if spk.size and not 0 <= spk[0] < n_speakers:
        raise ValueError('%s: speaker id %d outside [0, %d)' % (name, spk[0], n_speakers))


def utterance_variance(sp):
    """Biased per-bin variance of one utterance's sp [N, H], in float64."""
    s = np.asarray(sp, np.float64)
    return ((s - s.mean(axis=0)) ** 2).mean(axis=0)


def main_device(args, SPEAKERS):
    import torch
    from hipvae import stats

    files = sorted(glob.glob(args.train_file_pattern))
    print('{} files found'.format(len(files)))
    if not files:
        raise FileNotFoundError('no training files match %s' % args.train_file_pattern)
    sizes = [os.path.getsize(f) for f in files]
    for f, n in zip(files, sizes):
        if n % (FEAT_DIM * 4):
            raise ValueError('%s: %d bytes is not a whole number of %d-float records' % (f, n, FEAT_DIM))
    lengths = [n // (FEAT_DIM * 4) for n in sizes]
    F = sum(lengths)
    dev = torch.device('cuda:0')
    x = torch.empty(F, SP_DIM, dtype=torch.float32, device=dev)
    f0 = torch.empty(F, dtype=torch.float32, device=dev)
    speakers, frames, o = [], [0] * len(SPEAKERS), 0
    for f, n in zip(files, lengths):
        print('Processing {}'.format(f), flush=True)
        v = np.fromfile(f, '<f4').reshape(-1, FEAT_DIM)
        if len(v) != n:
            raise ValueError('%s changed size while it was read' % f)
        spk = v[:, SP_DIM * 2 + 2].astype(np.int64)
        check_speaker_column(f, spk, len(SPEAKERS))
        x[o:o + n].copy_(torch.from_numpy(v[:, :SP_DIM]))
        f0[o:o + n].copy_(torch.from_numpy(v[:, SP_DIM * 2]))
        speakers.append(int(spk[0]) if n else 0)       # an empty file adds nothing to any statistic
        frames[speakers[-1]] += n
        o += n
    if F == 0:
        raise ValueError('the training files hold no frame')

    # first, so that non-finite sp raises (ValueError naming the select's non-finite flag) before any file is written
    lo_hi = stats.percentiles(x, [0.5, 99.5]).cpu().numpy()
    lf0, gv, n_utt = stats.speaker_stats(x, f0, lengths, speakers, len(SPEAKERS))
    lf0, gv, n_utt = lf0.cpu().numpy(), gv.cpu().numpy(), n_utt.cpu().numpy()
    # ==== F0 stats ====
    for i, s in enumerate(SPEAKERS):
        print('Speaker {}'.format(s), flush=True)
        print('  len: {}'.format(frames[i]))
        if frames[i] == 0:
            print('  no training frames: no ./etc/{}.npf or ./etc/{}_gv.npf written'.format(s, s))
            continue
        lf0[i, 1:].astype(np.float32).tofile('./etc/{}.npf'.format(s))
        if n_utt[i] > 0:
            gv[i].astype(np.float32).tofile('./etc/{}_gv.npf'.format(s))
        else:
            print('  no utterance of 2 frames or more: no ./etc/{}_gv.npf written'.format(s))

    # ==== Min/Max value ====
    lo_hi[0].tofile('./etc/xmin.npf')
    lo_hi[1].tofile('./etc/xmax.npf')


def main(argv=None):
    args = parse_args(argv)
    SPEAKERS = load_speakers()
    os.makedirs('./etc', exist_ok=True)
    if args.device:
        return main_device(args, SPEAKERS)
    x_all, y_all, f0_all, gv_parts = [], [], [], {}
    for features in read_whole_features(args.train_file_pattern):
        spk = features['speaker']
        check_speaker_column(features['filename'].decode('utf8'), spk, len(SPEAKERS))
        x_all.append(features['sp'])
        y_all.append(spk)
        f0_all.append(features['f0'])
        if spk.size >= 2:
            gv_parts.setdefault(int(spk[0]), []).append(utterance_variance(features['sp']))
    if not x_all:
        raise FileNotFoundError('no training files match %s' % args.train_file_pattern)
    x_all = np.concatenate(x_all, axis=0)
    y_all = np.concatenate(y_all, axis=0)
    f0_all = np.concatenate(f0_all, axis=0)

    # ==== F0 stats ====
    for i, s in enumerate(SPEAKERS):
        print('Speaker {}'.format(s), flush=True)
        f0 = f0_all[y_all == i]
        print('  len: {}'.format(len(f0)))
        if len(f0) == 0:
            print('  no training frames: no ./etc/{}.npf or ./etc/{}_gv.npf written'.format(s, s))
            continue
        f0 = np.log(f0[f0 > 2.])
        np.asarray([f0.mean(), f0.std()], np.float32).tofile('./etc/{}.npf'.format(s))
        if i in gv_parts:
            np.mean(np.stack(gv_parts[i]), axis=0).astype(np.float32).tofile('./etc/{}_gv.npf'.format(s))
        else:
            print('  no utterance of 2 frames or more: no ./etc/{}_gv.npf written'.format(s))

    # ==== Min/Max value ====
    np.percentile(x_all, 0.5, axis=0).astype(np.float32).tofile('./etc/xmin.npf')
    np.percentile(x_all, 99.5, axis=0).astype(np.float32).tofile('./etc/xmax.npf')


if __name__ == '__main__':
    main()
