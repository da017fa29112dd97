"""Device resampling, host side: the exports, the host-only plan and filter entries against the float64 restatement
(tests/resample_ref.py), vaenpvc_resample's argument checks (no device is touched: every rejection happens before a
launch), the restatement against an independent formulation and against ideal sines, and analyzer.py's host logic with
the device calls replaced."""
import ctypes as C
import os
import re
import wave

import numpy as np
import pytest

import resample_ref as R
from helpers import ROOT
from hipvae import lib as L

E_ARG = -1
RATES = [8000, 11025, 22050, 24000, 32000, 44100, 48000, 96000]
PLANS = {48000: (1, 3, 192), 44100: (160, 441, 177), 32000: (1, 2, 128), 24000: (2, 3, 96), 22050: (320, 441, 89),
         11025: (640, 441, 64), 8000: (2, 1, 64), 96000: (1, 6, 384)}


def lib_plan(rate_in, rate_out=16000):
    lib = L.load_library()
    up, down, half = C.c_int32(-7), C.c_int32(-7), C.c_int32(-7)
    rc = lib.vaenpvc_resample_plan(rate_in, rate_out, C.byref(up), C.byref(down), C.byref(half))
    return rc, (up.value, down.value, half.value)


def lib_table(rate_in, rate_out=16000):
    rc, (up, down, half) = lib_plan(rate_in, rate_out)
    assert rc == 0
    t = np.full((2 * half, up), np.nan)
    assert L.load_library().vaenpvc_resample_filter(rate_in, rate_out, t.ctypes.data) == 0
    return t


def header_define(name):
    src = open(os.path.join(ROOT, 'include', 'vaenpvc.h')).read()
    return int(re.search(r'#define\s+%s\s+(\d+)' % name, src).group(1))


def test_resample_symbols_exported():
    lib = L.load_library()
    assert lib.vaenpvc_abi_version() == L.ABI_VERSION == 4
    for n in ('vaenpvc_resample_plan', 'vaenpvc_resample_filter', 'vaenpvc_resample'):
        assert hasattr(lib, n) and n in L.SIGNATURES


@pytest.mark.parametrize('rate_in', RATES + [15999])
def test_plan_matches_restatement(rate_in):
    rc, got = lib_plan(rate_in)
    assert rc == 0 and got == R.plan(rate_in, 16000)
    if rate_in in PLANS:
        assert got == PLANS[rate_in]                       # the table of DESIGN.md section 18
    else:
        assert got == (16000, 15999, 64)
    from hipvae import resample as RS
    assert RS.plan(rate_in, 16000) == got
    assert RS.out_length(1000, got[0], got[1]) == R.out_length(1000, got[0], got[1])


def test_plan_rejections():
    lib = L.load_library()
    for a, b in ((999, 16000), (16000, 999), (384001, 16000), (16000, 384001), (16000, 16000), (48000, 48000),
                 (0, 16000), (-48000, 16000)):
        rc, got = lib_plan(a, b)
        assert rc == E_ARG and got == (-7, -7, -7), (a, b)
        assert lib.vaenpvc_last_error()
    # 2 K L = 128 * 384000 entries > 2^24
    assert 2 * R.plan(383999, 384000)[2] * R.plan(383999, 384000)[0] > R.MAX_TABLE
    assert lib_plan(383999, 384000)[0] == E_ARG
    # a window one workgroup cannot stage: ceil(TILE M / L) + 2 K
    Lr, Mr, Kr = R.plan(384000, 1000)
    assert 2 * Kr * Lr <= R.MAX_TABLE
    assert -(-header_define('VAENPVC_RESAMPLE_TILE') * Mr // Lr) + 2 * Kr > header_define('VAENPVC_RESAMPLE_MAX_WINDOW')
    assert lib_plan(384000, 1000)[0] == E_ARG
    v = C.c_int32()
    for args in ((None, C.byref(v), C.byref(v)), (C.byref(v), None, C.byref(v)), (C.byref(v), C.byref(v), None)):
        assert lib.vaenpvc_resample_plan(48000, 16000, *args) == E_ARG
    assert lib.vaenpvc_resample_filter(48000, 16000, None) == E_ARG
    buf = np.zeros(4)
    assert lib.vaenpvc_resample_filter(16000, 16000, buf.ctypes.data) == E_ARG
    from hipvae import resample as RS
    for a, b in ((999, 16000), (16000, 16000), (383999, 384000), (1 << 40, 16000)):
        with pytest.raises(ValueError):
            RS.plan(a, b)
    for lengths in ([], [100, 0], [-1]):
        with pytest.raises(ValueError):
            RS.check_args(lengths, 48000, 16000)
    assert RS.check_args([5, 7], 48000, 16000) == ([5, 7], (1, 3, 192))


@pytest.mark.parametrize('rate_in', [48000, 44100, 22050, 11025, 8000])
def test_filter_matches_restatement(rate_in):
    """Both sides are float64 evaluations of values in [-1, 1]; the sinc argument reaches about 60 (its sine carries
    about 2e-14) and np.i0 agrees with scipy.special.i0 to 4.4e-16 relative on [0, BETA]: 1e-12 is two orders above
    that and eight below a float32 ulp."""
    got, want = lib_table(rate_in), R.table(rate_in, 16000)
    assert got.shape == want.shape == (2 * PLANS[rate_in][2], PLANS[rate_in][0])
    err = np.abs(got - want).max()
    print('rate %d: max |table - restatement| = %.3g' % (rate_in, err))
    assert err <= 1e-12
    from hipvae import resample as RS
    t = RS.filter_table(rate_in, 16000)
    assert t is RS.filter_table(rate_in, 16000) and np.array_equal(t, got) and not t.flags.writeable


def test_resample_argument_checks_without_device():
    lib = L.load_library()
    n, S_in = 3, 30000
    S_out = sum(R.out_length(k, 1, 3) for k in (10000, 10000, 10000))
    # fake device addresses, far apart: every rejection happens before a launch
    x, io, oo, tb, y = (k << 30 for k in range(1, 6))

    def call(**kw):
        a = dict(x=x, io=io, oo=oo, n=n, S_in=S_in, S_out=S_out, ri=48000, ro=16000, tb=tb, y=y)
        a.update(kw)
        return lib.vaenpvc_resample(a['x'], a['io'], a['oo'], a['n'], a['S_in'], a['S_out'], a['ri'], a['ro'], a['tb'],
                                    a['y'], None)
    for kw in ({'x': None}, {'io': None}, {'oo': None}, {'tb': None}, {'y': None}, {'n': 0}, {'n': -1}, {'n': 1 << 24},
               {'S_in': 2}, {'S_in': 1 << 31}, {'S_out': 2}, {'S_out': 10000 + n + 1}, {'S_out': 1 << 31},
               {'ri': 999}, {'ro': 999}, {'ri': 16000}, {'ri': 384001}, {'ri': 383999, 'ro': 384000},
               {'y': x}, {'y': x + 4 * S_in - 4}, {'y': tb}, {'y': tb + 8 * 384 - 8}, {'y': io}, {'y': oo},
               {'x': y + 4 * S_out - 4}):
        assert call(**kw) == E_ARG, kw
        assert lib.vaenpvc_last_error()
    # the largest S_out the samples allow passes the shape check and is then stopped by the overlap check
    assert call(S_out=10000 + n, y=x) == E_ARG and b'overlap' in lib.vaenpvc_last_error()


@pytest.mark.parametrize('rate_in', [48000, 32000])
def test_restatement_against_convolution(rate_in):
    """L = 1: y[m] = (x * h_full)[m M + K - 1] with h_full[i] = h(K - 1 - i), i = 0 .. 2K - 1."""
    Lr, Mr, Kr = R.plan(rate_in, 16000)
    assert Lr == 1
    x = np.random.default_rng(rate_in).uniform(-1, 1, 1501)
    h_full = R.h(Kr - 1 - np.arange(2 * Kr, dtype=np.float64), Lr, Mr)
    full = np.convolve(x, h_full)
    n_out = R.out_length(len(x), Lr, Mr)
    want = full[np.arange(n_out) * Mr + Kr - 1]
    got = R.resample_segment(x, rate_in, 16000, as_float32=False)
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12


def _sine(f, rate, dur=0.25):
    return np.sin(2 * np.pi * f * np.arange(int(dur * rate)) / rate)


@pytest.mark.parametrize('rate_in', [48000, 44100, 22050, 11025, 8000])
def test_restatement_quality(rate_in):
    """Pass band within 1e-6 of the ideal 16 kHz sine, stop band at most 1e-6, 800 samples in from each end (the
    restatement measures 3.9e-7 and 5.9e-8)."""
    T = R.table(rate_in, 16000)
    worst = 0.0
    for f in (100, 1000, 3000, 6000, 7000):
        if f >= rate_in / 2:
            continue
        y = R.resample_segment(_sine(f, rate_in), rate_in, 16000, T, as_float32=False)
        ideal = np.sin(2 * np.pi * f * np.arange(len(y)) / 16000.0)
        err = np.abs(y - ideal)[800:-800].max()
        worst = max(worst, err)
        assert err <= 1e-6, (rate_in, f, err)
    print('rate %d: pass band max error %.3g' % (rate_in, worst))
    if rate_in > 16000:
        worst = 0.0
        for f in (8450, 9000, 10000, 10900, 15000, 20000, 23000):
            if f >= rate_in / 2:
                continue
            y = R.resample_segment(_sine(f, rate_in), rate_in, 16000, T, as_float32=False)
            lev = np.abs(y)[800:-800].max()
            worst = max(worst, lev)
            assert lev <= 1e-6, (rate_in, f, lev)
        print('rate %d: stop band max level %.3g' % (rate_in, worst))


@pytest.mark.parametrize('rate_in', RATES)
def test_output_lengths(rate_in):
    from hipvae import resample as RS
    Lr, Mr, Kr = R.plan(rate_in, 16000)
    T = R.table(rate_in, 16000)
    for n in range(1, 51):
        want = (n * Lr + Mr - 1) // Mr
        assert want == int(np.ceil(n * 16000 / rate_in - 1e-9)) >= 1
        assert R.out_length(n, Lr, Mr) == RS.out_length(n, Lr, Mr) == want
        if n in (1, 2, 17, 50):
            assert len(R.resample_segment(np.ones(n), rate_in, 16000, T)) == want


# ---------------------------------------------------------------------------------------------- analyzer host logic
def _wav(path, pcm, fs, channels=1, width=2):
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(channels)
        w.setsampwidth(width)
        w.setframerate(fs)
        w.writeframes(np.ascontiguousarray(pcm).tobytes())


def test_cli_resample_flag(monkeypatch):
    import analyzer
    seen = []
    monkeypatch.setattr(analyzer, 'extract_and_save_bin_to', lambda *a, **kw: seen.append((a, kw)))
    analyzer.main(['--dir_to_wav', 'w', '--dir_to_bin', 'b', '--f0_ceil', '400', '--batch_seconds', '3', '--resample'])
    analyzer.main(['--dir_to_wav', 'w', '--dir_to_bin', 'b', '--f0_ceil', '400', '--batch_seconds', '3'])
    assert seen == [(('b', 'w', 16000, 400.0, 3.0), {'resample': True}), (('b', 'w', 16000, 400.0, 3.0), {})]
    for bad in (['--fs', '22050', '--resample'], ['--fs', '22050']):
        with pytest.raises(SystemExit):
            analyzer.main(bad)
    assert len(seen) == 2


def _fake_tree(tmp_path):
    """Training Set/SF1 with, in listing order, a 16 kHz, two 48 kHz and a 22.05 kHz file."""
    src = tmp_path / 'wav' / 'Training Set' / 'SF1'
    src.mkdir(parents=True)
    rng = np.random.default_rng(2)
    pcm = {}
    for name, fs, n in (('a.wav', 16000, 4000), ('b.wav', 48000, 12001), ('c.wav', 48000, 9000), ('d.wav', 22050, 5000)):
        pcm[name] = (fs, rng.integers(-20000, 20000, n).astype(np.int16))
        _wav(src / name, pcm[name][1], fs)
    return tmp_path / 'wav', pcm


def _fakes(monkeypatch, analyzer):
    rs_calls, an_calls = [], []

    def fake_resample(xs, rate_in, fs):
        rs_calls.append((rate_in, fs, [len(x) for x in xs]))
        Lr, Mr, _ = R.plan(rate_in, fs)
        return [np.full(R.out_length(len(x), Lr, Mr), 0.5, np.float32) for x in xs]

    def fake_analyze(xs, fs, f0_ceil):
        an_calls.append([np.array(x) for x in xs])
        out = []
        for x in xs:
            ft = np.zeros((len(x) // 80 + 1, 1028), np.float32)
            ft[:, 0] = len(x)
            out.append(ft)
        return out
    monkeypatch.setattr(analyzer, 'resample_group', fake_resample)
    monkeypatch.setattr(analyzer, '_analyze', fake_analyze)
    return rs_calls, an_calls


def test_extract_with_resample_host_logic(tmp_path, monkeypatch):
    import analyzer
    src, pcm = _fake_tree(tmp_path)
    rs_calls, an_calls = _fakes(monkeypatch, analyzer)
    out = tmp_path / 'bin'
    written = analyzer.extract_and_save_bin_to(str(out), str(src), resample=True)
    assert [os.path.basename(p) for p in written] == ['a.bin', 'b.bin', 'c.bin', 'd.bin']
    # one call per run of one rate; the 16 kHz file takes no part
    assert rs_calls == [(48000, 16000, [12001, 9000]), (22050, 16000, [5000])]
    fed = [x for call in an_calls for x in call]
    assert fed[0].dtype == np.float32
    assert np.array_equal(fed[0], (pcm['a.wav'][1] / 32768.0).astype(np.float32))       # untouched
    assert np.array_equal(fed[0], analyzer.read_wav(str(src / 'Training Set' / 'SF1' / 'a.wav')))
    want_len = [4000, R.out_length(12001, 1, 3), 3000, R.out_length(5000, 320, 441)]
    assert [len(x) for x in fed] == want_len == [4000, 4001, 3000, 3629]
    assert all(np.all(x == 0.5) for x in fed[1:])
    for p, n in zip(written, want_len):
        assert os.path.getsize(p) == (n // 80 + 1) * 4116                               # the resampled lengths
        rec = np.fromfile(p, '<f4').reshape(-1, 1029)
        assert np.all(rec[:, 0] == n)
    # without the flag the first file of another rate still stops the run
    with pytest.raises(ValueError, match='48000'):
        analyzer.extract_and_save_bin_to(str(tmp_path / 'bin2'), str(src))
    with pytest.raises(ValueError, match='22050'):
        analyzer.read_wav(str(src / 'Training Set' / 'SF1' / 'd.wav'))
    x, rate = analyzer.read_wav_native(str(src / 'Training Set' / 'SF1' / 'd.wav'))
    assert rate == 22050 and np.array_equal(x, (pcm['d.wav'][1] / 32768.0).astype(np.float32))
    _wav(tmp_path / 'w.wav', np.zeros(8, np.uint8), 48000, width=1)
    with pytest.raises(ValueError, match='16-bit'):
        analyzer.read_wav_native(str(tmp_path / 'w.wav'))
    # extract: one file, with and without the flag
    rs_calls.clear()
    ft = analyzer.extract(str(src / 'Training Set' / 'SF1' / 'b.wav'), resample=True)
    assert rs_calls == [(48000, 16000, [12001])] and ft.shape == (4001 // 80 + 1, 1028)
    ft = analyzer.extract(str(src / 'Training Set' / 'SF1' / 'a.wav'), resample=True)
    assert len(rs_calls) == 1 and ft.shape == (51, 1028)
    with pytest.raises(ValueError, match='48000'):
        analyzer.extract(str(src / 'Training Set' / 'SF1' / 'b.wav'))


def test_batch_seconds_caps_a_resample_run(tmp_path, monkeypatch):
    import analyzer
    src, pcm = _fake_tree(tmp_path)
    rs_calls, an_calls = _fakes(monkeypatch, analyzer)
    # 0.4 s of 48 kHz input is 19200 samples: b (12001) and c (9000) no longer share a call
    analyzer.extract_and_save_bin_to(str(tmp_path / 'bin'), str(src), batch_seconds=0.4, resample=True)
    assert rs_calls == [(48000, 16000, [12001]), (48000, 16000, [9000]), (22050, 16000, [5000])]
    assert max(sum(len(x) for x in call) for call in an_calls) <= max(int(0.4 * 16000), 4001)
    rs_calls.clear()
    analyzer.extract_and_save_bin_to(str(tmp_path / 'bin'), str(src), batch_seconds=0.0, resample=True)
    assert [c[2] for c in rs_calls] == [[12001], [9000], [5000]]
    rs_calls.clear()
    analyzer.extract_and_save_bin_to(str(tmp_path / 'bin'), str(src), batch_seconds=0.5, resample=True)
    assert rs_calls == [(48000, 16000, [12001, 9000]), (22050, 16000, [5000])]
