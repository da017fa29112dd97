"""Global-variance post-filter on the device (vaenpvc_gv_postfilter, csrc/gfx950_gv.hip): against the float64
restatement (tests/gv_ref.py), its defining properties, bit-for-bit batch invariance, and `convert.py --gv` end to end."""
import json
import os

import numpy as np
import pytest
import torch

import gv_ref
from helpers import SMALL_ARCH, load_arch
from oracle import convvae_oracle as O

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 37, 700, 1500, 40000]


@pytest.fixture(scope='module')
def eng():
    from hipvae.engine import Engine
    return Engine(load_arch(), device='cuda:0')


def make_case(lengths, H, seed):
    """Decoder-like output in the Tanhize domain (per utterance and bin: its own mean and spread), real-looking
    sp ranges; at H > 2 one bin with xmax == xmin and one constant bin."""
    rng = np.random.default_rng(seed)
    xmin = rng.uniform(-12, -6, H).astype(np.float32)
    xmax = (xmin + rng.uniform(2, 7, H)).astype(np.float32)
    parts = [rng.uniform(-0.6, 0.6, H) + rng.uniform(0.02, 0.3, H) * rng.standard_normal((n, H)) for n in lengths]
    x = np.concatenate(parts).astype(np.float32)
    if H > 2:
        xmax[H // 3] = xmin[H // 3]
        x[:, H // 2] = 0.25
    g = (rng.uniform(0.05, 0.5, H) ** 2).astype(np.float32)
    return x, xmin, xmax, g


def run(eng, x, lengths, xmin, xmax, g):
    dev = eng.device
    out = eng.gv_postfilter(torch.from_numpy(x).to(dev), lengths, torch.from_numpy(xmin).to(dev),
                            torch.from_numpy(xmax).to(dev), torch.from_numpy(g).to(dev))
    return out.cpu().numpy()


@pytest.mark.parametrize('H', [513, SMALL_ARCH['hwc'][0], 1])
def test_gv_against_float64(eng, H):
    x, xmin, xmax, g = make_case(LENGTHS, H, seed=H)
    out = run(eng, x, LENGTHS, xmin, xmax, g)
    ref, _ = gv_ref.batch(x, LENGTHS, xmin, xmax, g)
    o = 0
    for n in LENGTHS:
        r = ref[o:o + n]
        scale = np.ptp(r) if np.ptp(r) > 0 else np.abs(r).max()      # (one value: its magnitude)
        err = np.abs(out[o:o + n] - r).max()
        assert err <= 1e-5 * scale, (H, n, err, scale)
        o += n


def test_gv_properties(eng):
    H = 513
    x, xmin, xmax, g = make_case(LENGTHS, H, seed=7)
    out = run(eng, x, LENGTHS, xmin, xmax, g)
    dev = eng.device
    plain = eng.tanhize(torch.from_numpy(x).to(dev), torch.from_numpy(xmin).to(dev), torch.from_numpy(xmax).to(dev),
                        forward=False).cpu().numpy()
    _, masks = gv_ref.batch(x, LENGTHS, xmin, xmax, g)
    o = 0
    for n, on in zip(LENGTHS, masks):
        c = gv_ref.tanhize_backward(x[o:o + n], xmin, xmax)
        y = out[o:o + n].astype(np.float64)
        if n == 1:
            assert not on.any()
        else:
            assert on.sum() == H - 2 and not on[H // 3] and not on[H // 2]
            assert np.abs(y[:, on].mean(0) - c[:, on].mean(0)).max() <= 2e-6
            v = ((y[:, on] - y[:, on].mean(0)) ** 2).mean(0)
            assert np.abs(v / g[on] - 1).max() <= 1e-4, n
        # pass-through bins: the bytes of the inverse Tanhize (same fp32 expression)
        assert np.array_equal(out[o:o + n][:, ~on], plain[o:o + n][:, ~on])
        o += n


def test_gv_batch_invariance(eng):
    H = 513
    x, xmin, xmax, g = make_case(LENGTHS, H, seed=11)
    full = run(eng, x, LENGTHS, xmin, xmax, g)
    starts = np.concatenate([[0], np.cumsum(LENGTHS)[:-1]])
    # each utterance alone (offset 0, no neighbours)
    for s, n in zip(starts, LENGTHS):
        alone = run(eng, np.ascontiguousarray(x[s:s + n]), [n], xmin, xmax, g)
        assert np.array_equal(alone, full[s:s + n]), n
    # other neighbours, other offsets (13 foreign frames in front, order reversed)
    extra = np.random.default_rng(3).uniform(-1, 1, (13, H)).astype(np.float32)
    order = list(range(len(LENGTHS)))[::-1]
    x2 = np.concatenate([extra] + [x[starts[i]:starts[i] + LENGTHS[i]] for i in order])
    out2 = run(eng, x2, [13] + [LENGTHS[i] for i in order], xmin, xmax, g)
    o = 13
    for i in order:
        n = LENGTHS[i]
        assert np.array_equal(out2[o:o + n], full[starts[i]:starts[i] + n]), n
        o += n


def make_dataset(root, n_utt, seed):
    rng = np.random.default_rng(seed)
    recs = []
    for spk_id, spk in [(0, 'SF1'), (9, 'TM3')]:
        d = os.path.join(root, 'bin', 'Training Set', spk)
        os.makedirs(d)
        for u in range(n_utt):
            n = int(rng.integers(40, 80))
            r = rng.standard_normal((n, 1029)).astype(np.float32)
            r[:, :513] = rng.uniform(-12, -3, (n, 513))
            r[:, 1026] = np.where(rng.random(n) > 0.3, rng.uniform(80, 300, n), 0.0)
            r[:, -1] = spk_id
            r.tofile(os.path.join(d, '1000%02d.bin' % u))
            recs.append(r)
    allr = np.concatenate(recs)
    xmin = np.percentile(allr[:, :513], 0.5, axis=0).astype(np.float32)
    xmax = np.percentile(allr[:, :513], 99.5, axis=0).astype(np.float32)
    return xmin, xmax


@pytest.mark.parametrize('batch_frames', [None, 0])
def test_convert_cli_gv_end_to_end(tmp_path, monkeypatch, batch_frames):
    """convert.main(['--gv', ...]) against the float64 pipeline O.np_forward -> O.tanhize_backward -> gv_ref, with the
    default grouping of files into one launch and with one launch per file."""
    import sys
    import types
    import analyzer
    import convert as conv_cli
    from model.vae import ConvVAE
    arch = load_arch()
    root = str(tmp_path)
    xmin, xmax = make_dataset(root, n_utt=3, seed=21)
    os.makedirs(os.path.join(root, 'etc'))
    xmin.tofile(os.path.join(root, 'etc', 'xmin.npf'))
    xmax.tofile(os.path.join(root, 'etc', 'xmax.npf'))
    np.array([5.0, 0.25], np.float32).tofile(os.path.join(root, 'etc', 'SF1.npf'))
    np.array([4.7, 0.30], np.float32).tofile(os.path.join(root, 'etc', 'TM3.npf'))
    logdir = os.path.join(root, 'logdir', 'train', 'stamp')
    os.makedirs(logdir)
    with open(os.path.join(logdir, 'architecture-vae-vcc2016.json'), 'w') as fp:
        json.dump(arch, fp)
    machine = ConvVAE(arch, seed=8)
    torch.save({'params': machine.engine.params.cpu(), 'step': 7}, os.path.join(logdir, 'model.ckpt-7'))
    P = O.unflatten_params(arch, machine.engine.params.cpu().numpy())
    trg = analyzer.SPEAKERS.index('TM3')
    src_dir = os.path.join(root, 'bin', 'Training Set', 'SF1')
    files = sorted(os.listdir(src_dir))
    raws, convs = [], []
    for f in files:
        raw = O.parse_records(open(os.path.join(src_dir, f), 'rb').read())
        x = O.tanhize_forward(raw['sp'].astype(np.float64), xmin.astype(np.float64), xmax.astype(np.float64))
        R = O.np_forward(arch, P, x, np.full(len(x), trg), None)
        raws.append(raw)
        convs.append(O.tanhize_backward(R['xh'], xmin.astype(np.float64), xmax.astype(np.float64)))
    # the target's GV: twice the std of what the decoder produces (the filter widens, as on over-smoothed output)
    g = (4.0 * np.mean([gv_ref.utterance_variance(c) for c in convs], axis=0)).astype(np.float32)
    g.tofile(os.path.join(root, 'etc', 'TM3_gv.npf'))
    calls = []
    fake_pw = types.ModuleType('pyworld')
    fake_pw.synthesize = lambda f0, sp, ap, fs: (calls.append((f0, sp, ap, fs)) or np.zeros(8))
    fake_sf = types.ModuleType('soundfile')
    fake_sf.write = lambda name, y, fs: None
    monkeypatch.setitem(sys.modules, 'pyworld', fake_pw)
    monkeypatch.setitem(sys.modules, 'soundfile', fake_sf)
    monkeypatch.chdir(root)
    argv = ['--src', 'SF1', '--trg', 'TM3', '--model', 'ConvVAE', '--checkpoint', os.path.join(logdir, 'model.ckpt-7'),
            '--output_dir', os.path.join(root, 'logdir'), '--gv',
            '--file_pattern', os.path.join(root, 'bin', 'Training Set', '{}', '*.bin')]
    if batch_frames is not None:
        argv += ['--batch_frames', str(batch_frames)]
    conv_cli.main(argv)
    assert len(calls) == len(files)
    for (f0, sp, ap, fs), raw, c in zip(calls, raws, convs):
        filtered, on = gv_ref.postfilter(c, g)
        assert on.all()
        want_f0, want_sp, want_ap = O.pw2wav_inputs(filtered.astype(np.float32), raw['ap'],
                                                    O.convert_f0(raw['f0'], 5.0, 0.25, 4.7, 0.30), raw['en'])
        assert np.allclose(f0, want_f0, rtol=1e-6) and np.array_equal(ap, want_ap)
        assert np.array_equal(np.sign(sp), np.sign(want_sp))
        la, lb = np.log10(np.abs(sp)), np.log10(np.abs(want_sp))
        assert np.abs(la - lb).max() < 1e-4 * np.abs(lb).max()
