"""Device vocoder, host side: the C entry points' argument checks and workspace formula (no device is touched: every
rejection happens before a launch), the float64 restatement's own properties (tests/world_ref.py), the PCM16 writer and
the `--vocoder` flag of convert.py."""
import wave

import numpy as np
import pytest

import world_ref as W
from hipvae import lib as L

E_ARG, E_WS = -1, -2


def test_synth_symbols_exported():
    lib = L.load_library()
    assert lib.vaenpvc_abi_version() == L.ABI_VERSION == 4
    for n in ('vaenpvc_synth_workspace_bytes', 'vaenpvc_synthesize'):
        assert hasattr(lib, n) and n in L.SIGNATURES


def _ws_formula(n_seg, S, fs):
    a = lambda b: (b + 255) // 256 * 256                                 # noqa: E731
    slots = S * 1000 // fs + n_seg
    return a(4 * n_seg) + a(4 * (n_seg + 1)) + a(4 * slots) + a(8 * slots) + 4096 * slots


@pytest.mark.parametrize('n_seg,S,fs', [(1, 0, 16000), (1, 1, 8000), (6, 531200, 16000), (3, 12345, 22050),
                                        (40, 2621440, 48000)])
def test_synth_workspace_formula(n_seg, S, fs):
    lib = L.load_library()
    got = lib.vaenpvc_synth_workspace_bytes(n_seg, S, 513, fs)
    assert got == _ws_formula(n_seg, S, fs)
    assert got >= 4096 * (S * 1000 // fs + n_seg)                       # 4 KiB per pulse slot


def test_synth_workspace_rejections():
    lib = L.load_library()
    for bad in ((0, 100, 513, 16000), (-1, 100, 513, 16000), (1, -1, 513, 16000), (1, 100, 512, 16000),
                (1, 100, 1, 16000), (1, 100, 513, 7999), (1, 100, 513, 48001), (1, 1 << 31, 513, 16000)):
        assert lib.vaenpvc_synth_workspace_bytes(*bad) == E_ARG, bad


def test_synth_argument_checks_without_device():
    lib = L.load_library()
    n, F, S, H, fs = 3, 1000, 80000, 513, 16000
    need = lib.vaenpvc_synth_workspace_bytes(n, S, H, fs)
    # fake device addresses, far apart: every rejection happens before a launch
    f0, sp, en, ap, fo, so = 1 << 30, 2 << 30, 3 << 30, 4 << 30, 5 << 30, 6 << 30
    y, ws = 7 << 30, 8 << 30

    def call(**kw):
        a = dict(f0=f0, sp=sp, en=en, ap=ap, fo=fo, so=so, n=n, F=F, S=S, H=H, fs=fs, fp=5.0, seed=0, y=y, ws=ws,
                 nb=need)
        a.update(kw)
        return lib.vaenpvc_synthesize(a['f0'], a['sp'], a['en'], a['ap'], a['fo'], a['so'], a['n'], a['F'], a['S'],
                                      a['H'], a['fs'], a['fp'], a['seed'], a['y'], a['ws'], a['nb'], None)
    for kw in ({'n': 0}, {'n': -1}, {'H': 512}, {'H': 1024}, {'fs': 7999}, {'fs': 48001}, {'fp': 0.0}, {'fp': -5.0},
               {'fp': float('nan')}, {'fp': float('inf')}, {'f0': None}, {'sp': None}, {'en': None}, {'ap': None},
               {'fo': None}, {'so': None}, {'y': None}, {'S': -1}, {'F': 0},
               # d_y overlapping each input
               {'y': f0 + 4}, {'y': sp + 513 * 4 * 10}, {'y': en}, {'y': ap + 8}, {'y': fo}, {'y': so + 8},
               {'f0': y + 4 * (S - 1)}, {'y': ws + 64}):
        assert call(**kw) == E_ARG, kw
    assert call(nb=need - 1) == E_WS
    assert b'workspace too small' in lib.vaenpvc_last_error()
    assert call(ws=None) == E_WS
    assert call(ws=ws + 4) == E_ARG                                       # workspace alignment


# ---- the restatement's own properties -------------------------------------------------------------------------------

def test_min_phase_magnitude_and_causal_cepstrum():
    rng = np.random.default_rng(1)
    a = rng.uniform(-12, -2, (3, 1)) + np.cumsum(rng.normal(0, 0.05, (3, W.H)), axis=1)   # smooth: phase unwraps
    M = W.min_phase(a)
    assert np.allclose(np.abs(M), np.exp(a), rtol=1e-9)
    # log M = log|M| + i arg M (phase unwrapped over the bins) is the spectrum of a causal sequence: its cepstrum
    # vanishes above N/2
    lm = np.log(np.abs(M)) + 1j * np.unwrap(np.angle(M), axis=1)
    full = np.concatenate([lm, np.conj(lm[:, -2:0:-1])], axis=1)
    c = np.fft.ifft(full, axis=1)
    assert np.abs(c[:, W.N // 2 + 1:]).max() < 1e-9 * np.abs(c).max()
    assert np.abs(c.imag).max() < 1e-9 * np.abs(c).max()


@pytest.mark.parametrize('fs,f0', [(16000, 123.0), (16000, 207.3), (22050, 98.6)])
def test_constant_f0_pulse_spacing(fs, f0):
    T = 200
    S = W.n_samples(T, 5.0, fs)
    _, vuv, i, x = W.time_base(np.full(T, f0, np.float32), S, fs, 5.0)
    assert vuv.all()
    period = fs / float(np.float32(f0))
    d = np.diff(i)
    assert set(d) <= {int(np.floor(period)), int(np.ceil(period))}
    assert abs(d.mean() - period) < 2.0 / len(d) * period
    assert np.all((x > 0) & (x <= 1))


def test_unvoiced_and_ceiling_rates():
    fs, T = 16000, 100
    S = W.n_samples(T, 5.0, fs)
    for f0, want in ((0.0, 500.0), (3.0, 500.0), (np.nan, 500.0), (np.inf, 500.0), (4000.0, W.F0_CEIL)):
        _, _, i, _ = W.time_base(np.full(T, f0, np.float32), S, fs, 5.0)
        assert abs(np.diff(i).mean() - fs / want) < 0.05, f0
        assert len(i) <= W.capacity(S, fs)


def test_last_pulse_is_silent_and_segments_bounded():
    rng = np.random.default_rng(2)
    T = 57
    f0 = np.where(np.arange(T) < 30, 180.0, 0.0).astype(np.float32)
    sp = rng.uniform(-9, -5, (T, W.H)).astype(np.float32)
    en = np.full(T, 300.0, np.float32)
    ap = rng.uniform(0, 1, (T, W.H)).astype(np.float32)
    i, ns, r = W.segments(f0, sp, en, ap)
    assert len(i) > 2 and ns[-1] == 0 and not r[-1].any()
    assert np.all(ns[:-1] == np.minimum(np.diff(i), W.N)) and r[:-1].any(axis=1).all()


def test_one_frame_rule():
    f0 = np.array([150.0], np.float32)
    cf0, cvuv = W.coarse(f0, 16000)
    assert np.array_equal(cf0, [150.0, 150.0]) and np.array_equal(cvuv, [1.0, 1.0])
    cf0, cvuv = W.coarse(np.array([150.0, 120.0], np.float32), 16000)
    assert np.array_equal(cf0, [150.0, 120.0, 90.0]) and np.array_equal(cvuv, [1.0, 1.0, 1.0])


# ---- PCM writer and the CLI flag -------------------------------------------------------------------------------------

def test_pcm16_writer_roundtrip(tmp_path):
    import convert as conv_cli
    y = np.array([0.0, 0.5, -0.5, 1.0, -1.0, 1.7, -3.0, 1e-5, -0.49999 / 32767, np.float32(0.25)], np.float32)
    path = str(tmp_path / 'a.wav')
    conv_cli.write_wav(path, y, 16000)
    with wave.open(path, 'rb') as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, 2, 16000, len(y))
        got = np.frombuffer(w.readframes(len(y)), '<i2')
    assert np.array_equal(got, [0, 16384, -16384, 32767, -32767, 32767, -32767, 0, 0, 8192])


def test_convert_vocoder_flag():
    import convert as conv_cli
    assert conv_cli.parse_args(['--model', 'ConvVAE']).vocoder == 'pyworld'
    assert conv_cli.parse_args(['--model', 'ConvVAE', '--vocoder', 'device']).vocoder == 'device'
    assert conv_cli.parse_args(['--model', 'ConvVAE', '--vocoder', 'pyworld']).vocoder == 'pyworld'
    with pytest.raises(SystemExit):
        conv_cli.parse_args(['--model', 'ConvVAE', '--vocoder', 'griffin'])
    args = conv_cli.parse_args(['--model', 'ConvVAE'])
    assert (args.gv, args.batch_frames) == (False, 16384)               # the other defaults are untouched
