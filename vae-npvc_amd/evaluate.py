"""Objective evaluation CLI (not in the reference, whose validate.py only plots spectrograms):

    python evaluate.py --src SF1 --trg TM3 --model ConvVAE \
        --checkpoint logdir/train/<stamp>/model.ckpt-<N>

VCC2016 is a parallel corpus: the same basenames exist under every speaker.  Every source `.bin` is paired with the target
speaker's `.bin` of the same basename, converted like convert.py does (`convert.convert_utterances`, `convert.convert_f0`),
and compared with the target recording: mel-cepstral distortion (MCD) in dB along the dynamic-time-warping path between
the two, with the log-F0 RMSE and the voicing mismatch on the same path (hipvae.metrics.mcd_dtw on the GPU, DESIGN.md
section 16).  The unconverted source is compared with the target as well, so the report shows what the model gained.
Without `--checkpoint` only that second comparison is made (model-free: useful for checking an analysis setup).
Output: `<output_dir>/mcd-<src>-<trg>.tsv`, one row per utterance and two rows of means.
"""
import argparse
import glob
import json
import os
import sys
from importlib import import_module

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

COLUMNS = ('basename', 'src_frames', 'trg_frames', 'path_conv', 'mcd_conv_db', 'path_src', 'mcd_src_db', 'lf0_rmse_conv',
           'lf0_rmse_src', 'voicing_mismatch_conv', 'voicing_mismatch_src')
# the column whose path length weights a column in the MEAN_WEIGHTED_BY_PATH row (frame and path counts: plain means)
WEIGHT = {'mcd_conv_db': 'path_conv', 'lf0_rmse_conv': 'path_conv', 'voicing_mismatch_conv': 'path_conv',
          'mcd_src_db': 'path_src', 'lf0_rmse_src': 'path_src', 'voicing_mismatch_src': 'path_src'}


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--checkpoint', default=None, help='root of log dir; omit to compare source and target only')
    p.add_argument('--src', default='SF1', help='source speaker [SF1 - TM3]')
    p.add_argument('--trg', default='TM3', help='target speaker [SF1 - TM3]')
    p.add_argument('--output_dir', default='./logdir', help='where mcd-<src>-<trg>.tsv goes')
    p.add_argument('--module', default='model.vae', help='Module')
    p.add_argument('--model', default=None, help='Model (needed with --checkpoint)')
    p.add_argument('--file_pattern', default='./dataset/vcc2016/bin/Testing Set/{}/*.bin',
                   help='file pattern of the source speaker ({} = speaker)')
    p.add_argument('--trg_pattern', default=None,
                   help='file pattern of the target speaker\'s recordings ({} = speaker); default: --file_pattern')
    p.add_argument('--batch_frames', type=int, default=16384,
                   help='source frames gathered from consecutive utterances into one device call (convert.py\'s flag); '
                        '0 = one call per utterance')
    p.add_argument('--gv', action='store_true', help='convert with the global-variance post-filter (convert.py --gv)')
    p.add_argument('--order', type=int, default=24, help='mel-cepstral order M (the distortion uses coefficients 1 .. M)')
    p.add_argument('--alpha', type=float, default=0.42, help='all-pass constant of the mel warp (0.42 at 16 kHz)')
    p.add_argument('--energy_floor_db', type=float, default=40.0,
                   help='a setting of this tool, not part of the metric: frames whose energy `en` is more than this many dB '
                        'under the utterance\'s largest `en` (silence) are dropped from both sides before the alignment; '
                        '0 or negative keeps every frame')
    args = p.parse_args(argv)
    if args.checkpoint is not None and args.model is None:
        raise ValueError('\n  You MUST specify `model` with `checkpoint`.'
                         '\n    Use `python evaluate.py --help` to see applicable options.')
    return args


def basename(path):
    return os.path.splitext(os.path.basename(path))[0]


def pair_files(src_files, trg_files):
    """Pairs by basename -> ([(basename, src path, trg path)] sorted by basename, source files without a partner, target
    files without a partner)."""
    src = {basename(f): f for f in src_files}
    trg = {basename(f): f for f in trg_files}
    both = sorted(set(src) & set(trg))
    return ([(b, src[b], trg[b]) for b in both], [src[b] for b in sorted(set(src) - set(trg))],
            [trg[b] for b in sorted(set(trg) - set(src))])


def energy_keep(en, floor_db):
    """The frames that stay: 10 log10(en / max en) >= -floor_db (float64); floor_db <= 0 keeps all."""
    en = np.asarray(en, np.float64)
    if not floor_db > 0:
        return np.ones(en.shape, bool)
    return en >= en.max() * 10.0 ** (-float(floor_db) / 10.0)


def read_features(path):
    """One `.bin` file as analyzer.read_whole_features yields it."""
    from analyzer import FEAT_DIM, SP_DIM
    v = np.fromfile(path, '<f4').reshape(-1, FEAT_DIM)
    return {'sp': v[:, :SP_DIM], 'ap': v[:, SP_DIM:2 * SP_DIM], 'f0': v[:, SP_DIM * 2], 'en': v[:, SP_DIM * 2 + 1],
            'speaker': v[:, SP_DIM * 2 + 2].astype(np.int64), 'filename': path.encode('utf8')}


def _upload(arrays, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.concatenate(arrays).astype(np.float32))).to(device)


def default_device():
    import torch
    return torch.device('cuda', torch.cuda.current_device())


def evaluate_group(group, device, order=24, alpha=0.42, floor_db=40.0, convert_fn=None, f0_fn=None):
    """One group of (basename, source features, target features): one mcd_dtw call source against target and, with
    convert_fn (list of source sp -> list of converted sp tensors on the device) and f0_fn (source f0 -> converted f0),
    one call converted against target.  -> one row dict per utterance."""
    import torch
    from hipvae import metrics
    keep_s = [energy_keep(s['en'], floor_db) for _, s, _ in group]
    keep_t = [energy_keep(t['en'], floor_db) for _, _, t in group]
    len_s = [int(k.sum()) for k in keep_s]
    len_t = [int(k.sum()) for k in keep_t]
    side = lambda feats, keeps, key: _upload([f[key][k] for f, k in zip(feats, keeps)], device)   # noqa: E731
    src, trg = [s for _, s, _ in group], [t for _, _, t in group]
    sp_t, en_t, f0_t = (side(trg, keep_t, k) for k in ('sp', 'en', 'f0'))
    sp_s, en_s, f0_s = (side(src, keep_s, k) for k in ('sp', 'en', 'f0'))
    base = metrics.mcd_dtw(sp_s, en_s, f0_s, len_s, sp_t, en_t, f0_t, len_t, order=order, alpha=alpha)
    conv = None
    if convert_fn is not None:
        converted = convert_fn([s['sp'] for s in src])
        sp_c = torch.cat([c[torch.from_numpy(k).to(c.device)] for c, k in zip(converted, keep_s)], dim=0)
        f0_c = _upload([np.asarray(f0_fn(s['f0']), np.float32)[k] for s, k in zip(src, keep_s)], device)
        conv = metrics.mcd_dtw(sp_c.contiguous(), en_s, f0_c, len_s, sp_t, en_t, f0_t, len_t, order=order, alpha=alpha)
        conv = conv.cpu().numpy()
    base = base.cpu().numpy()
    rows = []
    nan = float('nan')
    for u, (name, _, _) in enumerate(group):
        b = base[u]
        c = conv[u] if conv is not None else [nan] * 8
        rows.append({'basename': name, 'src_frames': len_s[u], 'trg_frames': len_t[u],
                     'path_conv': c[1], 'mcd_conv_db': c[0], 'path_src': b[1], 'mcd_src_db': b[0],
                     'lf0_rmse_conv': c[3], 'lf0_rmse_src': b[3],
                     'voicing_mismatch_conv': c[5] / c[1], 'voicing_mismatch_src': b[5] / b[1]})
    return rows


def mean_rows(rows):
    """-> (means weighted by the path length of the comparison, plain means); NaN entries (no voiced cell, no model)
    are left out of a column's mean."""
    def mean(col, wcol):
        v = np.array([r[col] for r in rows], np.float64)
        w = np.array([r[wcol] for r in rows], np.float64) if wcol else np.ones(len(rows))
        ok = np.isfinite(v) & np.isfinite(w)
        return float((v[ok] * w[ok]).sum() / w[ok].sum()) if ok.any() else float('nan')
    out = []
    for label, weighted in (('MEAN_WEIGHTED_BY_PATH', True), ('MEAN', False)):
        r = {'basename': label}
        for col in COLUMNS[1:]:
            r[col] = mean(col, WEIGHT.get(col) if weighted else None)
        out.append(r)
    return out


def fmt(v):
    if isinstance(v, str):
        return v
    if isinstance(v, (int, np.integer)):
        return '%d' % v
    v = float(v)
    return 'nan' if not np.isfinite(v) else ('%d' % v if v == int(v) and abs(v) < 1e15 else '%.6f' % v)


def write_tsv(path, rows):
    with open(path, 'w') as fp:
        fp.write('\t'.join(COLUMNS) + '\n')
        for r in rows + mean_rows(rows):
            fp.write('\t'.join(fmt(r[c]) for c in COLUMNS) + '\n')


def main(argv=None):
    import torch
    import convert as conv_cli

    args = parse_args(argv)
    trg_pattern = args.trg_pattern or args.file_pattern
    pairs, only_src, only_trg = pair_files(sorted(glob.glob(args.file_pattern.format(args.src))),
                                           sorted(glob.glob(trg_pattern.format(args.trg))))
    print('{} pairs; {} source and {} target files without a partner'.format(len(pairs), len(only_src), len(only_trg)))
    for f in only_src + only_trg:
        print('No partner: {}'.format(f))
    if not pairs:
        raise ValueError('no source file of `{}` has a target file of the same basename under `{}`'.format(
            args.file_pattern.format(args.src), trg_pattern.format(args.trg)))
    convert_fn = f0_fn = None
    device = default_device()
    if args.checkpoint is not None:
        from analyzer import SPEAKERS, Tanhize, load_npf
        from util.wrapper import load
        MODEL = getattr(import_module(args.module), args.model)
        logdir, ckpt = os.path.split(args.checkpoint)
        with open(glob.glob(os.path.join(logdir, 'architecture*.json'))[0]) as fp:
            arch = json.load(fp)
        gv = conv_cli.load_gv(args.trg, int(arch['hwc'][0])) if args.gv else None
        normalizer = Tanhize(xmax=load_npf('./etc/xmax.npf'), xmin=load_npf('./etc/xmin.npf'))
        if gv is not None:
            gv = torch.as_tensor(gv).to(normalizer.xmin.device)
        machine = MODEL(arch)
        load(machine.engine, logdir, ckpt=ckpt)
        trg_id = SPEAKERS.index(args.trg)
        machine.engine.validate_ids(torch.full((1,), trg_id, dtype=torch.int64, device=machine.engine.device))
        device = machine.engine.device
        convert_fn = lambda sps: conv_cli.convert_utterances(machine, normalizer, sps, trg_id, gv=gv)   # noqa: E731
        f0_fn = lambda f0: conv_cli.convert_f0(f0, args.src, args.trg)                                   # noqa: E731
    feats = []
    for name, fs, ft in pairs:
        s = read_features(fs)
        s['pair'] = (name, s, read_features(ft))
        feats.append(s)
    rows = []
    for group in conv_cli.batched(feats, args.batch_frames):
        rows += evaluate_group([s['pair'] for s in group], device, order=args.order, alpha=args.alpha,
                               floor_db=args.energy_floor_db, convert_fn=convert_fn, f0_fn=f0_fn)
    os.makedirs(args.output_dir, exist_ok=True)
    out = os.path.join(args.output_dir, 'mcd-{}-{}.tsv'.format(args.src, args.trg))
    write_tsv(out, rows)
    w, m = mean_rows(rows)
    print('MCD [dB] converted vs target: {} (weighted by path length), {} (mean of utterances)'.format(
        fmt(w['mcd_conv_db']), fmt(m['mcd_conv_db'])))
    print('MCD [dB] source vs target:    {} (weighted by path length), {} (mean of utterances)'.format(
        fmt(w['mcd_src_db']), fmt(m['mcd_src_db'])))
    print('Wrote {}'.format(out))
    return out


if __name__ == '__main__':
    main()
