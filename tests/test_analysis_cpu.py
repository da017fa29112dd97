"""Device analysis, host side: the C entry points' argument checks and workspace formula (no device is touched: every
rejection happens before a launch), the binding's host checks, the float64 restatement (tests/world_analysis_ref.py)
against ground truth on synthetic signals, and analyzer.py's host logic with the device call replaced."""
import math
import os
import wave

import numpy as np
import pytest

import world_analysis_ref as R
from hipvae import lib as L
from hipvae import world

E_ARG, E_WS = -1, -2
FS = 16000
# bars: about 3x the restatement's own error measured on these signals
F0_CONST = 1.5e-3      # interior frames, constant f0 (measured 4.6e-4)
F0_GLIDE = 6e-3        # interior voiced frames of a 100 -> 300 Hz glide (measured 2.0e-3)
ENV_DB = 4.0           # CheapTrick log envelope vs truth, shape within [f0, 7 kHz] (measured 1.26 / 1.72 dB)


def test_analysis_symbols_exported():
    lib = L.load_library()
    assert lib.vaenpvc_abi_version() == L.ABI_VERSION == 4
    for n in ('vaenpvc_analysis_workspace_bytes', 'vaenpvc_analyze'):
        assert hasattr(lib, n) and n in L.SIGNATURES


@pytest.mark.parametrize('S', [1, 79, 80, 81, 300, 16000, 123457])
def test_frame_count_formula(S):
    T = int(1000.0 * S / FS / 5.0) + 1
    assert R.n_frames(S) == world.n_frames(S) == T == S // 80 + 1


def _ws_formula(n_seg, S, F, nb):
    a = lambda b: (b + 255) // 256 * 256                                 # noqa: E731
    NBS, NES = S + n_seg, S // 2 + 2 * n_seg
    return (a(8 * n_seg) + a(8 * nb * 1281) + a(8 * nb * NBS) + a(8 * nb * 4 * NES) + a(4 * nb * 4 * n_seg) +
            2 * a(8 * nb * F) + 7 * a(8 * F) + a(4 * F))


@pytest.mark.parametrize('n_seg,S,lo,hi', [(1, 1, 71.0, 500.0), (2, 32000, 71.0, 500.0), (5, 531200, 71.0, 800.0),
                                           (3, 12345, 100.0, 400.0), (40, 2621440, 71.0, 72.0)])
def test_analysis_workspace_formula(n_seg, S, lo, hi):
    lib = L.load_library()
    F = S // 80 + n_seg
    nb = R.n_bands(lo, hi)
    assert nb == world.n_bands(lo, hi)
    got = lib.vaenpvc_analysis_workspace_bytes(n_seg, S, F, FS, 5.0, lo, hi)
    assert got == _ws_formula(n_seg, S, F, nb) == world.layout(n_seg, S, F, nb)['bytes']


def test_analysis_workspace_rejections():
    lib = L.load_library()
    ok = (2, 32000, 402, FS, 5.0, 71.0, 500.0)
    assert lib.vaenpvc_analysis_workspace_bytes(*ok) > 0
    for i, v in ((0, 0), (0, -1), (1, 1), (2, 403), (2, 1), (3, 22050), (3, 8000), (4, 0.5), (4, float('nan')),
                 (5, 70.9), (5, 500.0), (6, 800.1), (6, 71.0), (6, float('inf')), (1, 1 << 31)):
        bad = list(ok)
        bad[i] = v
        assert lib.vaenpvc_analysis_workspace_bytes(*bad) == E_ARG, (i, v)


def test_analyze_argument_checks_without_device():
    lib = L.load_library()
    n, S = 3, 80000
    F = S // 80 + n
    need = lib.vaenpvc_analysis_workspace_bytes(n, S, F, FS, 5.0, 71.0, 500.0)
    # fake device addresses, far apart and aligned: every rejection happens before a launch
    x, so, fo, f0, sp, ap, en, ws = (k << 30 for k in range(1, 9))

    def call(**kw):
        a = dict(x=x, so=so, fo=fo, n=n, S=S, F=F, fs=FS, fp=5.0, lo=71.0, hi=500.0, f0=f0, sp=sp, ap=ap, en=en, ws=ws,
                 nb=need)
        a.update(kw)
        return lib.vaenpvc_analyze(a['x'], a['so'], a['fo'], a['n'], a['S'], a['F'], a['fs'], a['fp'], a['lo'],
                                   a['hi'], a['f0'], a['sp'], a['ap'], a['en'], a['ws'], a['nb'], None)
    for kw in ({'fs': 22050}, {'fs': 8000}, {'lo': 70.0}, {'lo': 500.0}, {'hi': 801.0}, {'lo': float('nan')},
               {'n': 0}, {'n': -2}, {'S': 2}, {'F': 2}, {'F': F + 1}, {'fp': 0.0}, {'fp': float('inf')},
               {'x': None}, {'so': None}, {'fo': None}, {'f0': None}, {'sp': None}, {'ap': None}, {'en': None},
               {'sp': x}, {'ap': sp}, {'en': f0}, {'ws': ws + 16}, {'sp': ws}):
        assert call(**kw) == E_ARG, kw
    for kw in ({'ws': None}, {'nb': need - 1}, {'nb': 0}):
        assert call(**kw) == E_WS, kw
    assert b'workspace' in lib.vaenpvc_last_error()


def test_binding_host_checks():
    for args in (([], 16000), ([100, 0], 16000), ([100], 22050)):
        with pytest.raises(ValueError):
            world.check_args(args[0], args[1], 5.0, 71.0, 500.0)
    for lo, hi in ((70.0, 500.0), (300.0, 300.0), (71.0, 900.0)):
        with pytest.raises(ValueError):
            world.check_args([100], 16000, 5.0, lo, hi)
    with pytest.raises(ValueError):
        world.check_args([100], 16000, 0.0, 71.0, 500.0)
    assert world.check_args([5, 7], 16000, 5, 71, 500) == ([5, 7], 5.0, 71.0, 500.0)


def test_fft_sizes_bounded():
    """Every FFT a stage derives from the allowed f0 limits stays <= 2048 points at 16 kHz."""
    for lo in (71.0, 80.0, 200.0):
        for hi in (lo + 1.0, 500.0, 800.0):
            if hi > lo:
                assert R.max_fft_size(lo, hi) <= 2048
    assert R.stonemask_fft_size(71.0) == 2048 and R.stonemask_fft_size(46.0) == 4096
    assert R.n_bands(71.0, 800.0) == 7 and R.n_bands(71.0, 500.0) == 6
    assert 2 * (R.mround(FS / 50.0) + R.mround(FS / R.boundaries(71.0, 500.0)[0] * 2.0)) + 1 <= 1281


# ---------------------------------------------------------------------------------------------- restatement truth
def harmonic(f0, dur=0.6):
    f0 = np.full(int(dur * FS), float(f0)) if np.ndim(f0) == 0 else np.asarray(f0, np.float64)
    ph = 2 * np.pi * np.cumsum(f0) / FS
    x = sum(np.where(k * f0 < 7800, np.cos(k * ph) / k, 0.0) for k in range(1, 60))
    return 0.3 * x / np.abs(x).max()


@pytest.mark.parametrize('f0', [80.0, 150.0, 300.0, 450.0])
def test_restatement_constant_f0(f0):
    d = R.analyze(harmonic(f0))
    v = d['f0'][12:-12]
    assert (v > 0).all()
    assert np.abs(v / f0 - 1).max() <= F0_CONST
    assert np.isfinite(d['sp']).all() and np.isfinite(d['ap']).all()


def test_restatement_glide():
    g = np.linspace(100, 300, int(0.8 * FS))
    d = R.analyze(harmonic(g))
    T = len(d['f0'])
    tr = g[np.minimum(np.arange(T) * 80, len(g) - 1)][12:-12]
    v = d['f0'][12:-12]
    assert (v > 0).mean() >= 0.9
    assert np.abs(v[v > 0] / tr[v > 0] - 1).max() <= F0_GLIDE


def test_restatement_noise_and_silence():
    d = R.analyze(0.1 * np.random.default_rng(3).standard_normal(FS // 2))
    assert (d['f0'] == 0).mean() >= 0.95
    assert np.all(d['ap'][d['f0'] == 0] == R.AP_UNVOICED)
    s = R.analyze(np.zeros(4000))
    assert (s['f0'] == 0).all() and np.all(s['ap'] == R.AP_UNVOICED)
    for k in ('sp', 'en', 'ap'):
        assert np.isfinite(d[k]).all() and np.isfinite(s[k]).all()
    # the deterministic floor: silence has a flat envelope at kEps, en = 513 (kEps + 1e-10)
    assert np.allclose(s['sp_lin'], R.EPS, rtol=1e-9)
    assert np.allclose(s['sp'], math.log10(R.EPS / (513 * (R.EPS + 1e-10))), atol=1e-9)


def _allpole(x, poles):
    a = np.poly(np.concatenate([poles, np.conj(poles)])).real
    y = np.zeros(len(x))
    for n in range(len(x)):
        acc = x[n]
        for k in range(1, min(len(a), n + 1)):
            acc -= a[k] * y[n - k]
        y[n] = acc
    return y, a


@pytest.mark.parametrize('P', [128, 80])
def test_restatement_cheaptrick_envelope(P):
    """A pulse train through a known minimum-phase (all-pole) envelope: CheapTrick's log envelope follows it."""
    x = np.zeros(FS // 2)
    x[::P] = 1.0
    poles = np.array([0.97 * np.exp(2j * np.pi * 600 / FS), 0.95 * np.exp(2j * np.pi * 1800 / FS),
                      0.9 * np.exp(2j * np.pi * 3000 / FS)])
    y, a = _allpole(x, poles)
    d = R.analyze(0.1 * y / np.abs(y).max())
    fr = np.arange(513) * FS / 1024.0
    truth = 10 * np.log10(np.abs(1.0 / np.polyval(a[::-1], np.exp(-2j * np.pi * fr / FS))) ** 2)
    band = (fr >= FS / P) & (fr <= 7000)
    T = len(d['f0'])
    assert np.abs(d['f0'][20:T - 20] / (FS / P) - 1).max() < F0_CONST
    for i in range(20, T - 20):
        got = 10 * np.log10(d['sp_lin'][i][band])
        err = (got - got.mean()) - (truth[band] - truth[band].mean())
        assert np.abs(err).max() <= ENV_DB, i
    # periodic frames: D4C says periodic (low ap below 3 kHz), against ~1 on noise
    mid = slice(20, T - 20)
    assert (d['ap0'][mid] > R.THRESHOLD).all()
    assert (d['ap'][mid][:, fr < 3000] < 0.05).all()


# ---------------------------------------------------------------------------------------------- analyzer host logic
def _wav(path, pcm, fs=FS, channels=1, width=2):
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(channels)
        w.setsampwidth(width)
        w.setframerate(fs)
        w.writeframes(np.ascontiguousarray(pcm).tobytes())


def test_read_wav(tmp_path):
    import analyzer
    m = np.array([0, 16384, -32768, 32767], np.int16)
    _wav(tmp_path / 'm.wav', m)
    assert np.array_equal(analyzer.read_wav(str(tmp_path / 'm.wav')), (m / 32768.0).astype(np.float32))
    st = np.array([[100, 300], [-32768, 0], [5, 6]], np.int16)
    _wav(tmp_path / 's.wav', st, channels=2)
    assert np.array_equal(analyzer.read_wav(str(tmp_path / 's.wav')), (st / 32768.0).mean(1).astype(np.float32))
    _wav(tmp_path / 'r.wav', m, fs=22050)
    with pytest.raises(ValueError, match='22050'):
        analyzer.read_wav(str(tmp_path / 'r.wav'))
    _wav(tmp_path / 'w.wav', np.zeros(8, np.uint8), width=1)
    with pytest.raises(ValueError, match='16-bit'):
        analyzer.read_wav(str(tmp_path / 'w.wav'))


def test_group_by_seconds_keeps_order():
    import analyzer
    items = [('a', 8000), ('b', 8000), ('c', 20000), ('d', 100), ('e', 16000)]
    assert analyzer.group_by_seconds(items, 1.0) == [['a', 'b'], ['c'], ['d'], ['e']]
    assert analyzer.group_by_seconds(items, 0) == [['a'], ['b'], ['c'], ['d'], ['e']]
    assert analyzer.group_by_seconds(items, 100.0) == [['a', 'b', 'c', 'd', 'e']]
    assert analyzer.group_by_seconds([], 1.0) == []


def test_extract_and_save_bin_to_host_logic(tmp_path, monkeypatch):
    import analyzer
    calls = []

    def fake(xs, fs, f0_ceil):
        calls.append([len(x) for x in xs])
        out = []
        for x in xs:
            T = R.n_frames(len(x))
            ft = np.zeros((T, 1028), np.float32)
            ft[:, 0] = len(x)
            ft[:, 1026] = np.arange(T)
            out.append(ft)
        return out
    monkeypatch.setattr(analyzer, '_analyze', fake)
    src = tmp_path / 'wav'
    for d, s, files in (('Training Set', 'SF1', ['b.wav', 'a.wav']), ('Training Set', 'TM3', ['c.wav']),
                        ('Training Set', 'NOPE', ['z.wav']), ('Other', 'SF1', ['y.wav']),
                        ('Testing Set', 'SM1', ['d.wav'])):
        (src / d / s).mkdir(parents=True)
        for i, f in enumerate(files):
            _wav(src / d / s / f, np.zeros(4000 + 1000 * i + len(f) * 0, np.int16))
    (src / 'Training Set' / 'SF1' / 'sub').mkdir()
    out = tmp_path / 'bin'
    written = analyzer.extract_and_save_bin_to(str(out), str(src), batch_seconds=0.5)
    rel = [os.path.relpath(p, str(out)) for p in written]
    assert rel == [os.path.join('Testing Set', 'SM1', 'd.bin'), os.path.join('Training Set', 'SF1', 'a.bin'),
                   os.path.join('Training Set', 'SF1', 'b.bin'), os.path.join('Training Set', 'TM3', 'c.bin')]
    assert sum(calls, []) == [4000, 5000, 4000, 4000] and max(sum(c) for c in calls) <= 8000
    for p in written:
        assert os.path.getsize(p) % 4116 == 0
    feats = list(analyzer.read_whole_features(str(out / '*' / '*' / '*.bin')))
    spk = {os.path.basename(os.path.dirname(d['filename'].decode())): d for d in feats}
    assert spk['TM3']['speaker'].tolist() == [analyzer.SPEAKERS.index('TM3')] * R.n_frames(4000)
    assert spk['SM1']['f0'].tolist() == list(range(R.n_frames(4000)))
    a = [d for d in feats if d['filename'].decode().endswith('a.bin')][0]
    assert a['sp'][:, 0].tolist() == [5000.0] * R.n_frames(5000) and a['ap'].shape == (R.n_frames(5000), 513)


def test_cli_flags(monkeypatch):
    import analyzer
    seen = {}
    monkeypatch.setattr(analyzer, 'extract_and_save_bin_to', lambda *a: seen.setdefault('a', a))
    analyzer.main(['--dir_to_wav', 'w', '--dir_to_bin', 'b', '--f0_ceil', '400', '--batch_seconds', '3'])
    assert seen['a'] == ('b', 'w', 16000, 400.0, 3.0)
    for bad in (['--fs', '22050'], ['--f0_ceil', '900']):
        with pytest.raises(SystemExit):
            analyzer.main(bad)
