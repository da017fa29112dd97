"""Statistics builder (the reference's build.py:15-65, plus the global-variance statistics it lacks):

    python build.py --train_file_pattern './dataset/vcc2016/bin/Training Set/*/*.bin'

writes under ./etc
    <spk>.npf      log-F0 mean and std over the speaker's frames with f0 > 2 (float32 [2], build.py:41-51)
    xmin.npf       per-bin 0.5 / 99.5 percentiles of sp over every training frame (build.py:57-65), float32 [513] on
    xmax.npf       disk whatever NumPy's percentile returns (the reference writes that dtype as is; SURVEY trap T4)
    <spk>_gv.npf   (not in the reference) global variance: per bin, the mean over the speaker's utterances of N >= 2
                   frames of the utterance's biased sp variance; computed in float64, stored float32 [513]
                   (read by `convert.py --gv`)

One-shot host NumPy.  Differences from the reference: the files are read in sorted order
(the reference's queue shuffles them); a file whose speaker column is not constant is an error; a speaker without
training files gets no files and a printed note (the reference writes NaN statistics for it).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--train_file_pattern', default='./dataset/vcc2016/bin/Training Set/*/*.bin',
                   help='training dir (to *.bin)')
    return p.parse_args(argv)


def utterance_variance(sp):
    """Biased per-bin variance of one utterance's sp [N, H], in float64."""
    s = np.asarray(sp, np.float64)
    return ((s - s.mean(axis=0)) ** 2).mean(axis=0)


def main(argv=None):
    from analyzer import SPEAKERS, read_whole_features

    args = parse_args(argv)
    os.makedirs('./etc', exist_ok=True)
    x_all, y_all, f0_all, gv_parts = [], [], [], {}
    for features in read_whole_features(args.train_file_pattern):
        spk = features['speaker']
        name = features['filename'].decode('utf8')
        if spk.size and np.any(spk != spk[0]):
            raise ValueError('%s: speaker column is not constant (%s)' % (name, sorted(set(spk.tolist()))))
        if spk.size and not 0 <= spk[0] < len(SPEAKERS):
            raise ValueError('%s: speaker id %d outside [0, %d)' % (name, spk[0], len(SPEAKERS)))
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
