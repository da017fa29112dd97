"""Device resampling (vaenpvc_resample, csrc/gfx950_resample.hip) against the float64 restatement
(tests/resample_ref.py): every output within one float32 ulp of the float32-rounded restatement, tile boundaries,
segment edges, bit-for-bit batch invariance and determinism, and `analyzer.py --resample` end to end.

The one-ulp bar: both sides sum at most 384 float64 products with sum |h| <= 2.6 and |x| <= 1, so they differ by less
than 1e-12 before the one rounding to float32, whose half-ulp at these magnitudes is about 3e-8: they can differ only
across a rounding boundary, by one ulp."""
import os
import re
import wave

import numpy as np
import pytest
import torch

import resample_ref as R
from helpers import ROOT

pytestmark = pytest.mark.gpu

FS = 16000
RATES = [48000, 44100, 22050, 11025, 8000]
TILE = int(re.search(r'#define\s+VAENPVC_RESAMPLE_TILE\s+(\d+)',
                     open(os.path.join(ROOT, 'include', 'vaenpvc.h')).read()).group(1))


def run(xs, rate_in):
    """-> list of float32 arrays, one per segment"""
    from hipvae import resample as RS
    x = torch.from_numpy(np.concatenate(xs).astype(np.float32)).cuda()
    y, outs = RS.resample(x, [len(v) for v in xs], rate_in, FS)
    torch.cuda.synchronize()
    y = y.cpu().numpy()
    assert y.dtype == np.float32 and len(y) == sum(outs)
    o = np.concatenate([[0], np.cumsum(outs)])
    return [y[o[i]:o[i + 1]] for i in range(len(xs))]


def check(got, xs, rate_in):
    want = R.resample(xs, rate_in, FS)
    assert len(got) == len(want)
    for u, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape, (rate_in, u)
        assert np.isfinite(g).all(), (rate_in, u)
        d = np.abs(g.astype(np.float64) - w.astype(np.float64)) / np.spacing(np.abs(w)).astype(np.float64)
        print('rate %d segment %d (%d -> %d samples): max distance %.3g ulp, %d of %d differ'
              % (rate_in, u, len(xs[u]), len(w), d.max(), int((d > 0).sum()), len(w)))
        assert R.within_one_ulp32(g, w), (rate_in, u, d.max())


@pytest.fixture(scope='module')
def batches():
    """Per rate: four segments of [1, K - 1, 2053, 3001] uniform samples, their device result (one call)."""
    out = {}
    for rate in RATES:
        K = R.plan(rate, FS)[2]
        rng = np.random.default_rng(rate)
        xs = [rng.uniform(-1, 1, n).astype(np.float32) for n in (1, K - 1, 2053, 3001)]
        out[rate] = (xs, run(xs, rate))
    return out


@pytest.mark.parametrize('rate_in', RATES)
def test_parity(batches, rate_in):
    xs, got = batches[rate_in]
    Lr, Mr, Kr = R.plan(rate_in, FS)
    assert [len(g) for g in got] == [R.out_length(len(x), Lr, Mr) for x in xs]
    check(got, xs, rate_in)


@pytest.mark.parametrize('rate_in', [22050, 48000])
@pytest.mark.parametrize('n_out', [TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_tiles(rate_in, n_out):
    """One segment whose output count sits on either side of a tile boundary (at 22 050 Hz, L = 320: r = m mod L wraps
    inside the second tile when TILE = 256)."""
    Lr, Mr, Kr = R.plan(rate_in, FS)
    n = (n_out * Mr) // Lr                     # the largest n with out_length(n) == n_out
    assert R.out_length(n, Lr, Mr) == n_out and R.out_length(n + 1, Lr, Mr) == n_out + 1
    x = np.random.default_rng(n_out).uniform(-1, 1, n).astype(np.float32)
    got = run([x], rate_in)
    assert len(got[0]) == n_out
    check(got, [x], rate_in)


@pytest.mark.parametrize('rate_in', RATES)
def test_edges(rate_in):
    """An impulse at the first and at the last input sample and a constant 1.0: zero padding at both ends."""
    n = 1500
    first, last = np.zeros(n, np.float32), np.zeros(n, np.float32)
    first[0], last[-1] = 1.0, 1.0
    xs = [first, last, np.ones(n, np.float32)]
    got = run(xs, rate_in)
    check(got, xs, rate_in)
    Lr, Mr, Kr = R.plan(rate_in, FS)
    T = R.table(rate_in, FS)
    assert got[0][0] == np.float32(T[Kr - 1, 0])            # h(0) = s R
    far = int((Kr + 2) * Lr / Mr) + 2                        # outputs whose window is past the impulse
    assert np.all(got[0][far:] == 0) and np.all(got[1][:len(got[1]) - far - 1] == 0)
    mid = got[2][len(got[2]) // 2 - 50:len(got[2]) // 2 + 50]
    assert np.abs(mid - 1.0).max() < 1e-6                    # DC gain of the pass band
    # output 0 keeps the taps j >= 0 of a symmetric filter whose taps add up to 1: (1 + h(0)) / 2
    assert abs(got[2][0] - 0.5 * (1.0 + T[Kr - 1, 0])) < 1e-5


def test_independence_and_determinism(batches):
    for rate_in in (44100, 8000):
        xs, got = batches[rate_in]
        for u in range(len(xs)):
            alone = run([xs[u]], rate_in)[0]
            assert np.array_equal(alone, got[u]), (rate_in, u)
        for order in ([3, 0, 2, 1], [2, 3, 1, 0]):
            again = run([xs[u] for u in order], rate_in)
            for j, u in enumerate(order):
                assert again[j].tobytes() == got[u].tobytes(), (rate_in, order, u)
        twice = run(xs, rate_in)
        assert b''.join(a.tobytes() for a in twice) == b''.join(a.tobytes() for a in got)


def harmonic(f0, fs, amp=0.3, nh=40):
    """Harmonic complex with instantaneous f0 track `f0` [S] (1/k amplitudes, below 7.8 kHz)."""
    ph = 2 * np.pi * np.cumsum(f0) / fs
    x = np.zeros(len(f0))
    for k in range(1, nh + 1):
        x += np.where(k * f0 < 7800, np.cos(k * ph) / k, 0.0)
    return amp * x / max(np.abs(x).max(), 1e-9)


def write_wav(path, pcm, fs):
    with wave.open(path, 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(fs)
        w.writeframes(np.asarray(pcm).astype('<i2').tobytes())


def test_analyzer_end_to_end(tmp_path):
    import analyzer
    from hipvae import resample as RS
    from hipvae import world
    wav = tmp_path / 'wav' / 'Training Set' / 'SF1'
    wav.mkdir(parents=True)
    pcm = {}
    for name, fs, f0 in (('10000', 48000, (140, 200)), ('10001', 22050, (220, 180))):
        x = harmonic(np.linspace(f0[0], f0[1], int(0.3 * fs)), fs)
        pcm[name] = (fs, np.round(x * 20000).astype(np.int16))
        write_wav(str(wav / (name + '.wav')), pcm[name][1], fs)

    def expect(name):
        fs, p = pcm[name]
        x = torch.from_numpy((p.astype(np.float64) / 32768.0).astype(np.float32)).cuda()
        y, outs = RS.resample(x, [len(p)], fs, FS)
        f0, sp, ap, en, frames = world.analyze(y, outs)
        assert frames == [world.n_frames(outs[0])] and outs[0] == R.out_length(len(p), *R.plan(fs, FS)[:2])
        ref = tmp_path / ('ref_' + name + '.bin')
        analyzer.write_bin(str(ref), sp.cpu().numpy(), ap.cpu().numpy(), f0.cpu().numpy(), en.cpu().numpy(), 'SF1')
        return ref.read_bytes(), frames[0], f0.cpu().numpy()

    want = {name: expect(name) for name in pcm}
    assert (want['10000'][2] > 0).mean() > 0.5                           # the resampled harmonic signal is voiced
    out = tmp_path / 'bin'
    written = analyzer.extract_and_save_bin_to(str(out), str(tmp_path / 'wav'), resample=True)
    assert [os.path.basename(p) for p in written] == ['10000.bin', '10001.bin']
    out2 = tmp_path / 'bin2'
    analyzer.main(['--dir_to_wav', str(tmp_path / 'wav'), '--dir_to_bin', str(out2), '--resample'])
    for name in pcm:
        for o in (out, out2):
            got = (o / 'Training Set' / 'SF1' / (name + '.bin')).read_bytes()
            assert len(got) == want[name][1] * analyzer.RECORD_BYTES, name
            assert got == want[name][0], name
    with pytest.raises(ValueError, match='48000'):
        analyzer.extract_and_save_bin_to(str(tmp_path / 'bin3'), str(tmp_path / 'wav'))
