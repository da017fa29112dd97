"""Conversion CLI with the reference's flag names (convert.py:14-30):

    python convert.py --src SF1 --trg TM3 --model ConvVAE \
        --checkpoint logdir/train/<stamp>/model.ckpt-<N>

Device path per utterance (convert.py:79-89): Tanhize -> encode (z_mu) -> decode with the
target speaker id -> inverse Tanhize (with `--gv`: the global-variance post-filter fused with
it).  The log-F0 transform (convert.py:51-57) runs on the host.  `--vocoder pyworld` (the default)
synthesises with pyworld when it is importable and writes a wav, otherwise it saves the converted
features as `<src>-<trg>-<basename>.npz`.  `--vocoder device` synthesises every group of utterances
on the GPU (Engine.synthesize) and writes 16-bit PCM wavs.
"""
import argparse
import glob
import json
import os
import sys
import wave
from datetime import datetime
from importlib import import_module

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

FS = 16000
FRAME_PERIOD = 5.0          # ms: pyworld's default, used by the reference's analysis and synthesis


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--checkpoint', default=None, help='root of log dir')
    p.add_argument('--src', default='SF1', help='source speaker [SF1 - TM3]')
    p.add_argument('--trg', default='TM3', help='target speaker [SF1 - TM3]')
    p.add_argument('--output_dir', default='./logdir', help='root of output dir')
    p.add_argument('--module', default='model.vae', help='Module')
    p.add_argument('--model', default=None, help='Model')
    p.add_argument('--file_pattern', default='./dataset/vcc2016/bin/Testing Set/{}/*.bin', help='file pattern')
    p.add_argument('--batch_frames', type=int, default=16384,
                   help='(not in the reference) frames gathered from consecutive utterances into one device launch; '
                        '0 = REFERENCE-PARITY mode: one launch per utterance, like the reference\'s sess.run per file -- an '
                        'utterance of <= 512 frames then runs on the fp32-exact whole-frame kernels and its output does not '
                        'depend on its neighbours in the glob order.  The default gathers files onto the large-batch kernels '
                        '(2-term bf16 operands: within the 1e-4 relative parity bar, not bit-reproducible per file)')
    p.add_argument('--gv', action='store_true',
                   help='(not in the reference) global-variance post-filter: every bin of a converted utterance keeps its '
                        'mean and takes the target speaker\'s mean utterance variance, ./etc/<trg>_gv.npf (written by '
                        'build.py).  Off by default: the output is then the unfiltered conversion')
    p.add_argument('--vocoder', choices=['pyworld', 'device'], default='pyworld',
                   help='(not in the reference) pyworld (default, the reference\'s path): a wav through pyworld when it '
                        'imports, otherwise the converted features as .npz; device: WORLD-style synthesis on the GPU, one '
                        'call per group of utterances, 16-bit PCM wavs (no pyworld / soundfile import)')
    args = p.parse_args(argv)
    if args.model is None:                                               # convert.py:23-27
        raise ValueError('\n  You MUST specify `model`.'
                         '\n    Use `python convert.py --help` to see applicable options.')
    return args


def make_output_name(output_dir, filename, src, trg, ext):              # convert.py:35-43
    basename = os.path.splitext(os.path.split(str(filename, 'utf8'))[-1])[0]
    print('Processing {}'.format(basename))
    return os.path.join(output_dir, '{}-{}-{}.{}'.format(src, trg, basename, ext))


def get_default_output(logdir_root):                                     # convert.py:45-49
    stamp = datetime.now().strftime('%m%d-%H%M-%S-%Y')
    logdir = os.path.join(logdir_root, 'output', stamp)
    print('Using default logdir: {}'.format(logdir))
    return logdir


def convert_f0(f0, src, trg, etc_dir='./etc'):
    """convert.py:51-57 -- note the thresholds apply to the TRANSFORMED value (quirk kept)."""
    mu_s, std_s = np.fromfile(os.path.join(etc_dir, '{}.npf'.format(src)), np.float32)
    mu_t, std_t = np.fromfile(os.path.join(etc_dir, '{}.npf'.format(trg)), np.float32)
    f0 = np.asarray(f0, np.float32)
    lf0 = np.where(f0 > 1., np.log(np.where(f0 > 1., f0, 1.)), f0).astype(np.float32)
    lf0 = np.where(lf0 > 1., (lf0 - mu_s) / std_s * std_t + mu_t, lf0).astype(np.float32)
    lf0 = np.where(lf0 > 1., np.exp(lf0), lf0).astype(np.float32)
    return lf0


def load_gv(trg, H, etc_dir='./etc'):
    """The target speaker's global variance (build.py: `<spk>_gv.npf`, H float32), checked before any device work."""
    from analyzer import load_npf
    path = os.path.join(etc_dir, '{}_gv.npf'.format(trg))
    if not os.path.isfile(path):
        raise FileNotFoundError('%s: no global-variance statistics for speaker %s (written by build.py)' % (path, trg))
    gv = load_npf(path, count=H)
    if not np.all(np.isfinite(gv)) or np.any(gv < 0):
        raise ValueError('%s: global variances must be finite and >= 0' % path)
    return gv


def convert_utterance(machine, normalizer, sp, trg_id, gv=None, lengths=None):
    """The device tensor path of convert.py:79-89 for one utterance: sp [N,513] -> converted sp.  gv (target speaker's
    global variance, [513]): the GV post-filter replaces the inverse Tanhize; `lengths` then splits the rows into
    utterances stored back to back (default: one utterance)."""
    import torch
    x = normalizer.forward_process(sp)                                    # [N,513] in [-1,1]
    x = x.view(x.shape[0], 1, x.shape[1], 1)                              # nh_to_nchw (convert.py:60-63)
    y_t = torch.full((x.shape[0],), int(trg_id), dtype=torch.int64, device=x.device)
    z = machine.encode(x)
    x_t = machine.decode(z, y_t)                                          # NHWC [N,513,1,1]
    x_t = x_t.reshape(x_t.shape[0], -1)                                   # tf.squeeze
    if gv is None:
        return normalizer.backward_process(x_t)
    gv = torch.as_tensor(gv, dtype=torch.float32).to(x_t.device)
    return machine.engine.gv_postfilter(x_t, [x_t.shape[0]] if lengths is None else lengths, normalizer.xmin,
                                        normalizer.xmax, gv)


def convert_utterances(machine, normalizer, sps, trg_id, gv=None):
    """The same tensor path for SEVERAL utterances in one launch.  The model is frame-wise (W = 1: every frame is an independent
    sample of the network, model/vae.py:72-103), so the frames of consecutive files can share one encode -> decode call and the
    result is cut back at the file boundaries.  One utterance is a few hundred to ~2 000 frames, a size at which a launch
    sequence is latency-bound (0.4 ms for 1 024 frames against 2.5 ms for 32 768); the reference runs one sess.run per file
    (convert.py:105-116).  With `gv` the post-filter takes its statistics per file (one call for the group).  Returns the
    converted sp of every utterance, in order."""
    import torch
    sps = [np.ascontiguousarray(sp, np.float32) for sp in sps]
    if not sps:
        return []
    if len(sps) == 1:
        return [convert_utterance(machine, normalizer, sps[0], trg_id, gv=gv)]
    lengths = [sp.shape[0] for sp in sps]
    out = convert_utterance(machine, normalizer, np.concatenate(sps, axis=0), trg_id, gv=gv, lengths=lengths)
    return list(torch.split(out, lengths, dim=0))


def write_wav(path, y, fs=FS):
    """Mono 16-bit PCM through the standard library: rint(clip(y, -1, 1) * 32767)."""
    pcm = np.rint(np.clip(np.asarray(y, np.float64), -1.0, 1.0) * 32767.0).astype('<i2')
    with wave.open(path, 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(int(fs))
        w.writeframes(pcm.tobytes())


def synthesize_group(machine, group, converted, src, trg, etc_dir='./etc'):
    """Device vocoder for one group of utterances: the converted sp stays on the device, the converted f0, en and ap are
    uploaded, one Engine.synthesize call.  Returns the waveforms (host float32), one per utterance."""
    import torch
    dev = machine.engine.device
    lengths = [int(feat['sp'].shape[0]) for feat in group]
    sp = converted[0] if len(converted) == 1 else torch.cat(converted, dim=0)
    f0 = np.concatenate([convert_f0(feat['f0'], src, trg, etc_dir) for feat in group])
    en = np.concatenate([np.asarray(feat['en'], np.float32) for feat in group])
    ap = np.concatenate([np.asarray(feat['ap'], np.float32) for feat in group])
    up = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (f0, en, ap)]
    y, samples = machine.engine.synthesize(up[0], sp.contiguous(), up[1], up[2], lengths, fs=FS,
                                           frame_period=FRAME_PERIOD)
    y = y.cpu().numpy()
    return np.split(y, np.cumsum(samples)[:-1])


def batched(features, batch_frames):
    """Groups the utterance stream: consecutive feature dicts whose frame counts add up to at most `batch_frames` (an utterance
    longer than that goes alone; batch_frames <= 0: every utterance alone).  Order is preserved."""
    group, n = [], 0
    for feat in features:
        k = int(feat['sp'].shape[0])
        if group and (batch_frames <= 0 or n + k > batch_frames):
            yield group
            group, n = [], 0
        group.append(feat)
        n += k
    if group:
        yield group


def main(argv=None):
    from analyzer import read_whole_features, SPEAKERS, Tanhize, load_npf
    from util.wrapper import load

    args = parse_args(argv)
    MODEL = getattr(import_module(args.module), args.model)
    logdir, ckpt = os.path.split(args.checkpoint)
    arch_file = glob.glob(os.path.join(logdir, 'architecture*.json'))[0]  # should only be 1 file
    with open(arch_file) as fp:
        arch = json.load(fp)
    gv = None
    if args.gv:
        gv = load_gv(args.trg, int(arch['hwc'][0]))
    normalizer = Tanhize(xmax=load_npf('./etc/xmax.npf'), xmin=load_npf('./etc/xmin.npf'))
    if gv is not None:
        import torch
        gv = torch.as_tensor(gv).to(normalizer.xmin.device)                # once: no host-to-device copy per group
    machine = MODEL(arch)
    load(machine.engine, logdir, ckpt=ckpt)
    output_dir = get_default_output(args.output_dir)
    os.makedirs(output_dir, exist_ok=True)
    trg_id = SPEAKERS.index(args.trg)
    machine.engine.validate_ids(_ids(machine, 1, trg_id))
    if args.vocoder == 'device':
        for group in batched(read_whole_features(args.file_pattern.format(args.src)), args.batch_frames):
            converted = convert_utterances(machine, normalizer, [feat['sp'] for feat in group], trg_id, gv=gv)
            for feat, y in zip(group, synthesize_group(machine, group, converted, args.src, args.trg)):
                write_wav(make_output_name(output_dir, feat['filename'], args.src, args.trg, 'wav'), y, FS)
        return output_dir
    try:
        import pyworld  # noqa: F401  (absent in this image: the features are saved instead of a wav)
        import soundfile as sf
        have_world = True
    except ImportError:
        sf, have_world = None, False
    from analyzer import pw2wav
    for group in batched(read_whole_features(args.file_pattern.format(args.src)), args.batch_frames):
        converted = convert_utterances(machine, normalizer, [feat['sp'] for feat in group], trg_id, gv=gv)
        for feat, sp_t in zip(group, converted):
            sp = sp_t.cpu().numpy()
            f0 = convert_f0(feat['f0'], args.src, args.trg)
            feat.update({'sp': sp, 'f0': f0})
            if have_world:
                y = pw2wav(feat)                                           # convert.py:110-112
                sf.write(make_output_name(output_dir, feat['filename'], args.src, args.trg, 'wav'), y, FS)
            else:
                np.savez(make_output_name(output_dir, feat['filename'], args.src, args.trg, 'npz'),
                         sp=sp, f0=f0, ap=feat['ap'], en=feat['en'])
    return output_dir


def _ids(machine, n, trg_id):
    import torch
    return torch.full((max(1, n),), int(trg_id), dtype=torch.int64, device=machine.engine.device)


if __name__ == '__main__':
    main()
