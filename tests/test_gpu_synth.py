"""Device vocoder (vaenpvc_synthesize, csrc/gfx950_synth.hip): against the float64 restatement (tests/world_ref.py) at
two geometries, its defining properties, bit-for-bit batch invariance, and `convert.py --vocoder device` end to end."""
import importlib.abc
import json
import os
import sys
import wave

import numpy as np
import pytest
import torch

import world_ref as W
from helpers import load_arch

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 3, 57, 400, 6000]
# bars per utterance, at most 3x the largest value measured on an MI355X (8.9e-7 and 8.4e-7)
REL_L2 = 2.5e-6
MAX_OVER_PEAK = 2.5e-6


@pytest.fixture(scope='module')
def eng():
    from hipvae.engine import Engine
    return Engine(load_arch(), device='cuda:0')


def make_case(lengths, fs, seed):
    """Voiced and unvoiced runs, f0 jumps, f0 below fs/N + 1 and above the ceiling, one NaN and one inf f0; smooth
    log10 envelopes; aperiodicity runs at exactly 0, exactly 1 and in between."""
    rng = np.random.default_rng(seed)
    F = sum(lengths)
    f0 = np.zeros(F)
    t = 0
    while t < F:
        n = min(int(rng.integers(4, 60)), F - t)
        kind = rng.choice(['voiced', 'voiced', 'unvoiced', 'low', 'high', 'jump'])
        seg = np.arange(n)
        if kind == 'voiced':
            f0[t:t + n] = rng.uniform(80, 300) * (1 + 0.05 * np.sin(seg / 7.0))
        elif kind == 'low':
            f0[t:t + n] = rng.uniform(1, fs / W.N)                    # below fs/N + 1: unvoiced
        elif kind == 'high':
            f0[t:t + n] = rng.uniform(1100, 3000)                    # above the ceiling
        elif kind == 'jump':
            f0[t:t + n] = np.where(seg % 6 < 3, rng.uniform(90, 140), rng.uniform(200, 400))
        t += n
    if F > 100:
        f0[F // 2] = np.nan
        f0[F // 3] = np.inf
    k = np.arange(W.H) / W.H
    base = rng.uniform(-8.0, -6.0, (F, 1)) + np.cumsum(rng.normal(0, 0.05, (F, 1)), axis=0) * 0.1
    sp = base - 2.5 * k[None, :] + 0.4 * np.sin(2 * np.pi * k[None, :] * rng.uniform(2, 6, (F, 1)))
    en = rng.uniform(200.0, 3000.0, F)
    ap = np.empty((F, W.H))
    t = 0
    while t < F:
        n = min(int(rng.integers(3, 40)), F - t)
        kind = rng.integers(0, 3)
        if kind == 0:
            ap[t:t + n] = 0.0
        elif kind == 1:
            ap[t:t + n] = 1.0
        else:
            ap[t:t + n] = np.clip(rng.uniform(0, 1, (1, W.H)) * k[None, :] ** 0.3 + rng.uniform(0, 0.2, (n, 1)),
                                  0, 1)
            ap[t:t + n, 0] = rng.uniform(0.0, 0.9)
        t += n
    return (f0.astype(np.float32), sp.astype(np.float32), en.astype(np.float32), ap.astype(np.float32))


def run(eng, case, lengths, fs=16000, frame_period=5.0, seed=0):
    dev = eng.device
    f0, sp, en, ap = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in case)
    y, samples = eng.synthesize(f0, sp, en, ap, lengths, fs=fs, frame_period=frame_period, seed=seed)
    y = y.cpu().numpy()
    assert samples == [W.n_samples(T, frame_period, fs) for T in lengths] and len(y) == sum(samples)
    return np.split(y, np.cumsum(samples)[:-1])


def errors(got, want):
    got = np.asarray(got, np.float64)
    nw = np.linalg.norm(want)
    return np.linalg.norm(got - want) / nw, np.abs(got - want).max() / np.abs(want).max()


def check_against(got, want, what):
    worst = (0.0, 0.0)
    for T, g, r in zip(LENGTHS, got, want):
        assert g.shape == r.shape
        if not r.any():
            assert not g.any(), (what, T)
            continue
        e2, em = errors(g, r)
        print('%s T=%d rel_l2 %.3e max/peak %.3e' % (what, T, e2, em))
        assert e2 <= REL_L2 and em <= MAX_OVER_PEAK, (what, T, e2, em)
        worst = max(worst[0], e2), max(worst[1], em)
    return worst


@pytest.mark.parametrize('fs,frame_period', [(16000, 5.0), (22050, 5.8)])
def test_synth_against_float64(eng, fs, frame_period):
    case = make_case(LENGTHS, fs, seed=fs)
    got = run(eng, case, LENGTHS, fs, frame_period, seed=7)
    want = W.batch(*case, LENGTHS, fs=fs, frame_period=frame_period, seed=7)
    assert any(r.any() for r in want[:3])                             # a short utterance that does sound
    check_against(got, want, 'fs=%d' % fs)


def test_synth_seed(eng):
    lengths = [57, 400]
    case = make_case(lengths, 16000, seed=3)
    a = run(eng, case, lengths, seed=11)
    b = run(eng, case, lengths, seed=11)
    c = run(eng, case, lengths, seed=12)
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x, y)
        assert not np.array_equal(x, z)


def test_synth_ap_one_is_noise_only(eng):
    lengths = [400, 57]
    f0, sp, en, ap = make_case(lengths, 16000, seed=5)
    ap = np.ones_like(ap)
    f0 = np.full_like(f0, 150.0)                                        # voiced throughout
    got = run(eng, (f0, sp, en, ap), lengths, seed=1)
    other = run(eng, (f0, sp, en, ap), lengths, seed=2)
    want = W.batch(f0, sp, en, ap, lengths, seed=1, parts=('aper',))
    for g, o, r in zip(got, other, want):
        e2, em = errors(g, r)
        assert e2 <= REL_L2 and em <= MAX_OVER_PEAK, (e2, em)
        assert abs(np.corrcoef(g, o)[0, 1]) < 0.1                       # no deterministic (periodic) component


def test_synth_constant_f0_peak_spacing(eng):
    fs, f0v = 16000, 161.3
    T = 300
    f0, sp, en, ap = make_case([T], fs, seed=9)
    f0 = np.full(T, f0v, np.float32)
    ap = np.full_like(ap, 0.0)
    (y,) = run(eng, (f0, sp, en, ap), [T])
    y = y[2000:-2000].astype(np.float64)
    lags = np.arange(40, 400)
    ac = np.array([np.dot(y[:-L], y[L:]) for L in lags])
    assert abs(lags[np.argmax(ac)] - fs / f0v) <= 1.0
    # the strongest sample of each period sits a period after the previous one
    per = fs / f0v
    peaks = [int(np.argmax(np.abs(y[:int(per)])))]
    while peaks[-1] + per + 12 < len(y):
        lo = int(peaks[-1] + per) - 12
        peaks.append(lo + int(np.argmax(np.abs(y[lo:lo + 25]))))
    d = np.diff(peaks)
    assert len(d) > 30 and np.all(np.abs(d - per) <= 1.0), d


def test_synth_energy_scaling(eng):
    """Four times en -> twice the amplitude.  Exact up to the floors of the log-amplitudes: the inputs keep
    E (1 - R) far above the periodic part's 1e-12 (ap <= 0.9, en ~ 1e5), where the floor is below the bar."""
    lengths = [400, 57]
    f0, sp, en, ap = make_case(lengths, 16000, seed=13)
    en = (en * 100.0).astype(np.float32)
    ap = np.minimum(ap, 0.9).astype(np.float32)
    a = run(eng, (f0, sp, en, ap), lengths, seed=4)
    b = run(eng, (f0, sp, (4 * en).astype(np.float32), ap), lengths, seed=4)
    for x, y in zip(a, b):
        e2, em = errors(y, 2.0 * x.astype(np.float64))
        print('energy x4: rel_l2 %.3e max/peak %.3e' % (e2, em))
        assert e2 <= REL_L2 and em <= MAX_OVER_PEAK, (e2, em)


def test_synth_batch_invariance(eng):
    case = make_case(LENGTHS, 16000, seed=17)
    full = run(eng, case, LENGTHS, seed=5)
    starts = np.concatenate([[0], np.cumsum(LENGTHS)[:-1]])
    sl = lambda a, i: np.ascontiguousarray(a[starts[i]:starts[i] + LENGTHS[i]])   # noqa: E731
    for i, T in enumerate(LENGTHS):
        (alone,) = run(eng, tuple(sl(a, i) for a in case), [T], seed=5)
        assert np.array_equal(alone, full[i]), T
    # other neighbours and offsets: a foreign utterance in front, the order reversed
    extra = make_case([33], 16000, seed=99)
    order = list(range(len(LENGTHS)))[::-1]
    case2 = tuple(np.concatenate([e] + [sl(a, i) for i in order]) for e, a in zip(extra, case))
    out2 = run(eng, case2, [33] + [LENGTHS[i] for i in order], seed=5)
    for k, i in enumerate(order):
        assert np.array_equal(out2[k + 1], full[i]), LENGTHS[i]


# ---- convert.py --vocoder device end to end -------------------------------------------------------------------------

def make_dataset(root, n_utt, seed):
    rng = np.random.default_rng(seed)
    recs = []
    for spk_id, spk in [(0, 'SF1'), (9, 'TM3')]:
        d = os.path.join(root, 'bin', 'Training Set', spk)
        os.makedirs(d)
        for u in range(n_utt):
            n = int(rng.integers(40, 80))
            r = rng.standard_normal((n, 1029)).astype(np.float32)
            r[:, :513] = rng.uniform(-9, -5, (n, 513))
            r[:, 513:1026] = rng.uniform(0, 1, (n, 513))
            r[:, 1026] = np.where(rng.random(n) > 0.3, rng.uniform(80, 300, n), 0.0)
            r[:, 1027] = rng.uniform(100, 2000, n)
            r[:, -1] = spk_id
            r.tofile(os.path.join(d, '1000%02d.bin' % u))
            recs.append(r)
    allr = np.concatenate(recs)
    xmin = np.percentile(allr[:, :513], 0.5, axis=0).astype(np.float32)
    xmax = np.percentile(allr[:, :513], 99.5, axis=0).astype(np.float32)
    return xmin, xmax


class _ImportSpy(importlib.abc.MetaPathFinder):
    def __init__(self):
        self.seen = []

    def find_spec(self, name, path=None, target=None):
        if name.split('.')[0] in ('pyworld', 'soundfile'):
            self.seen.append(name)
        return None


@pytest.mark.parametrize('batch_frames,gv', [(None, False), (0, False), (None, True)])
def test_convert_cli_device_vocoder(tmp_path, monkeypatch, batch_frames, gv):
    import analyzer
    import convert as conv_cli
    from model.vae import ConvVAE
    arch = load_arch()
    root = str(tmp_path)
    xmin, xmax = make_dataset(root, n_utt=3, seed=31)
    etc = os.path.join(root, 'etc')
    os.makedirs(etc)
    xmin.tofile(os.path.join(etc, 'xmin.npf'))
    xmax.tofile(os.path.join(etc, 'xmax.npf'))
    np.array([5.0, 0.25], np.float32).tofile(os.path.join(etc, 'SF1.npf'))
    np.array([4.7, 0.30], np.float32).tofile(os.path.join(etc, 'TM3.npf'))
    np.full(513, 0.05, np.float32).tofile(os.path.join(etc, 'TM3_gv.npf'))
    logdir = os.path.join(root, 'logdir', 'train', 'stamp')
    os.makedirs(logdir)
    with open(os.path.join(logdir, 'architecture-vae-vcc2016.json'), 'w') as fp:
        json.dump(arch, fp)
    machine = ConvVAE(arch, seed=8)
    torch.save({'params': machine.engine.params.cpu(), 'step': 7}, os.path.join(logdir, 'model.ckpt-7'))
    for name in ('pyworld', 'soundfile'):
        monkeypatch.delitem(sys.modules, name, raising=False)
    spy = _ImportSpy()
    monkeypatch.setattr(sys, 'meta_path', [spy] + sys.meta_path)
    monkeypatch.chdir(root)
    argv = ['--src', 'SF1', '--trg', 'TM3', '--model', 'ConvVAE', '--checkpoint', os.path.join(logdir, 'model.ckpt-7'),
            '--output_dir', os.path.join(root, 'logdir'), '--vocoder', 'device',
            '--file_pattern', os.path.join(root, 'bin', 'Training Set', '{}', '*.bin')]
    if batch_frames is not None:
        argv += ['--batch_frames', str(batch_frames)]
    if gv:
        argv += ['--gv']
    out_dir = conv_cli.main(argv)
    assert spy.seen == []
    names = sorted(os.listdir(out_dir))
    src_dir = os.path.join(root, 'bin', 'Training Set', 'SF1')
    files = sorted(os.listdir(src_dir))
    assert names == ['SF1-TM3-%s.wav' % os.path.splitext(f)[0] for f in files]   # no .npz
    # the device-converted features of the same groups, synthesised utterance by utterance (batch invariant)
    feats = list(analyzer.read_whole_features(os.path.join(src_dir, '*.bin')))
    normalizer = analyzer.Tanhize(xmax=xmax, xmin=xmin)
    g = torch.from_numpy(np.full(513, 0.05, np.float32)).to(normalizer.xmin.device) if gv else None
    trg = analyzer.SPEAKERS.index('TM3')
    k = 0
    for group in conv_cli.batched(feats, 16384 if batch_frames is None else batch_frames):
        converted = conv_cli.convert_utterances(machine, normalizer, [f['sp'] for f in group], trg, gv=g)
        for feat, sp_t in zip(group, converted):
            f0 = conv_cli.convert_f0(feat['f0'], 'SF1', 'TM3')
            dev = machine.engine.device
            y, (S,) = machine.engine.synthesize(torch.from_numpy(f0).to(dev), sp_t.contiguous(),
                                                torch.from_numpy(np.ascontiguousarray(feat['en'])).to(dev),
                                                torch.from_numpy(np.ascontiguousarray(feat['ap'])).to(dev),
                                                [len(f0)], fs=16000, frame_period=5.0)
            want = np.rint(np.clip(y.cpu().numpy().astype(np.float64), -1, 1) * 32767).astype(np.int16)
            with wave.open(os.path.join(out_dir, names[k]), 'rb') as w:
                assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 16000)
                assert w.getnframes() == S == 80 * len(f0)
                got = np.frombuffer(w.readframes(S), '<i2')
            assert np.array_equal(got, want), names[k]
            assert np.abs(want).max() > 0
            k += 1
    assert k == len(files)
