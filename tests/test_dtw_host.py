"""CPU checks of the DTW / mel-cepstral-distortion feature: the numpy oracle against brute force and its tie rule, the exported symbols
and the workspace size, the argument checks of ops.dtw (they fire before any device is touched), MCD_SCALE, the --mcd-wav-dir parser
rules and the pairing of synthesised files with recordings."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tests'))
import dtw_oracle as O  # noqa: E402


# ---------------------------------------------------------------- the oracle
@pytest.mark.parametrize('n', [1, 2, 3, 4])
@pytest.mark.parametrize('m', [1, 2, 3, 4])
def test_oracle_equals_brute_force(n, m):
    """every monotone path of the grid, enumerated: the oracle's total is the cheapest cost, its path is a path of that cost, and the
    path itself wherever the optimum is unique"""
    for seed in range(6):
        rs = np.random.RandomState(100 * n + 10 * m + seed)
        D = 1 + seed % 3
        x, y = rs.randn(n, D), rs.randn(m, D)
        bf = O.brute_force(x, y, 1.5)
        for dtype, tol in ((np.float64, 1e-12), (np.float32, 1e-5)):
            total, path = O.dtw(x.astype(dtype), y.astype(dtype), 1.5, dtype)
            assert total.dtype == dtype and abs(float(total) - bf[0][0]) <= tol * max(1.0, bf[0][0])
            assert O.is_path(path, n, m) and path.dtype == np.int32
            assert abs(O.path_cost(x.astype(dtype), y.astype(dtype), path, 1.5) - bf[0][0]) <= tol * max(1.0, bf[0][0])
            if len(bf) == 1 or bf[1][0] - bf[0][0] > 1e-4:
                assert tuple(map(tuple, path.tolist())) == bf[0][1]
    # the number of monotone paths of an n x m grid is the Delannoy number D(n-1, m-1)
    delannoy = {(0, 0): 1, (1, 1): 3, (2, 2): 13, (3, 3): 63, (1, 3): 7, (2, 3): 25}
    if (min(n, m) - 1, max(n, m) - 1) in delannoy:
        assert len(bf) == delannoy[(min(n, m) - 1, max(n, m) - 1)]


def test_oracle_tie_rule_on_constant_inputs():
    for n in (1, 2, 5, 17):
        x = np.ones((n, 2))
        total, path = O.dtw(x, x, 1.0)
        assert total == 0.0 and path.tolist() == [[k, k] for k in range(n)]             # square: the pure diagonal
        total, path = O.dtw(x, 3.0 * np.ones((1, 2)), 1.0)
        assert path.tolist() == [[k, 0] for k in range(n)]                              # m = 1: the only path
        assert abs(total - n * 2.0 * math.sqrt(2.0)) < 1e-12
        assert O.dtw(np.ones((1, 2)), x, 1.0)[1].tolist() == [[0, k] for k in range(n)]  # n = 1
    # every cost equal, n != m: the diagonal wins every tie on the way back from the corner, then (i-1, j), then (i, j-1)
    assert O.dtw(np.ones((4, 1)), np.zeros((2, 1)))[1].tolist() == [[0, 0], [1, 0], [2, 0], [3, 1]]
    assert O.dtw(np.ones((2, 1)), np.zeros((4, 1)))[1].tolist() == [[0, 0], [0, 1], [0, 2], [1, 3]]
    # degenerate pairs
    for x, y in ((np.zeros((0, 2)), np.ones((3, 2))), (np.ones((3, 2)), np.zeros((0, 2))), (np.array([[1.0], [np.nan]]), np.ones((2, 1)))):
        total, path = O.dtw(x, y)
        assert np.isnan(total) and path.shape == (0, 2)
    assert not O.is_path(np.zeros((0, 2)), 1, 1) and O.is_path([[0, 0]], 1, 1)
    assert not O.is_path([[0, 0], [2, 1]], 3, 2) and not O.is_path([[0, 0], [1, 1]], 3, 2) and not O.is_path([[0, 1], [1, 1]], 2, 2)
    assert O.eps(300, 333, 12) == (300 + 333 - 1 + 12 + 4) * 2.0 ** -24


def test_integer_inputs_have_integer_distances():
    rs = np.random.RandomState(0)
    for D in (1, 3):
        for _ in range(8):
            x, y = O.integer_pair(rs, 9, 7, D)
            assert x.dtype == np.float32 and x.shape == (9, D) and y.shape == (7, D)
            d32, d64 = O.distances(x, y, 1.0, np.float32), O.distances(x, y, 1.0, np.float64)
            assert np.array_equal(d32.astype(np.float64), d64) and np.array_equal(d64, np.round(d64))


# ---------------------------------------------------------------- the library
def test_library_exports_and_workspace():
    from semi_tts_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, 'st_dtw_batch') and hasattr(lib, 'st_dtw_workspace_bytes')
    assert 'st_dtw_batch' in _lib.SIGNATURES and len(_lib.SIGNATURES['st_dtw_batch']) == 19
    ws = lib.st_dtw_workspace_bytes
    ws.argtypes, ws.restype = [ctypes.c_int] * 3, ctypes.c_size_t
    assert ws(32, 300, 330) == 0                                    # a few seconds at the 10 ms hop: the back-pointers fit LDS
    top = ws(64, 4096, 4096)
    assert 64 * 4096 * 8191 // 4 <= top <= 2 * 64 * 4096 * 8191 // 4        # 2 bits per cell, (diagonal, position) indexing at most doubles it
    prev = 0
    for T in (1, 64, 300, 500, 600, 1000, 2048, 4096):
        for B in (1, 2, 64):
            cur = ws(B, T, T)
            assert 0 <= cur <= top and (cur == 0 or cur >= prev)
            assert ws(B, T, 4096) >= cur and ws(B, 4096, T) >= cur                 # monotone in every argument
            if B > 1:
                assert cur == B * ws(1, T, T)
        prev = ws(1, T, T)
    assert ws(1, 600, 600) > 0
    assert ws(0, 600, 600) == 0 and ws(1, 0, 5) == 0 and ws(1, 5, 4097) == 0    # outside the limits: nothing to hold


def test_c_entry_refuses_each_limit_without_a_device():
    """the limit checks precede the launch: -22 and a message naming the entry point, with pointers that are never dereferenced"""
    from semi_tts_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)

    def call(Tx=4, Ty=4, B=1, d0=0, d1=2, scale=1.0, x_st=2, y_st=2, x=p, ws=None):
        return lib.st_dtw_batch(x, 8, x_st, None, Tx, p, 8, y_st, None, Ty, B, d0, d1, scale, p, p, None, ws, None)
    for kw in (dict(B=0), dict(Tx=0), dict(Ty=0), dict(Tx=4097), dict(Ty=4097), dict(d0=-1), dict(d0=2), dict(d0=0, d1=65, x_st=65, y_st=65),
               dict(x_st=1), dict(y_st=1), dict(scale=0.0), dict(scale=-1.0), dict(scale=float('inf')), dict(scale=float('nan')),
               dict(x=None), dict(Tx=600, Ty=600)):                     # (the last: a table that needs the workspace, none given)
        assert call(**kw) == -22, kw
        assert b'st_dtw_batch' in lib.st_last_error()


# ---------------------------------------------------------------- ops argument checks
def _no_device(monkeypatch):
    from semi_tts_amd import _lib

    def no_device(*a, **k):
        raise AssertionError('reached the device')
    monkeypatch.setattr(_lib, 'load', no_device)


def test_dtw_argument_checks_fire_before_the_device(monkeypatch):
    from semi_tts_amd import ops, metrics
    _no_device(monkeypatch)
    x, y = torch.rand(2, 5, 4), torch.rand(2, 6, 4)
    for kw in (dict(x=x, y=y), dict(x=[[1.0]], y=y)):                  # CPU tensors, not tensors
        with pytest.raises(ValueError, match='GPU tensor'):
            ops.dtw(**kw)
    # the remaining checks read .is_cuda / .device / .shape / .dtype / .stride() only: a meta tensor stands in for a device tensor
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: self.device.type in ('cuda', 'meta')))
    mx, my = x.to('meta'), y.to('meta')
    wide = torch.rand(1, 3, 70).to('meta')
    cases = [
        (dict(x=mx, y=y), 'y must be'),
        (dict(x=mx.double(), y=my), 'float32'),
        (dict(x=mx[0], y=my), 'x must be'),
        (dict(x=mx, y=my[:1]), 'must match'),
        (dict(x=mx, y=my[:, :, :3]), 'must match'),
        (dict(x=mx[:0], y=my[:0]), 'B=0'),
        (dict(x=mx[:, :0], y=my), 'Tx=0'),
        (dict(x=mx, y=my[:, :0]), 'Ty=0'),
        (dict(x=torch.empty(1, 4097, 2, device='meta'), y=my[:1, :, :2]), 'Tx=4097'),
        (dict(x=mx[:1, :, :2], y=torch.empty(1, 4097, 2, device='meta')), 'Ty=4097'),
        (dict(x=mx, y=my, cols=(2, 2)), 'cols'),
        (dict(x=mx, y=my, cols=(-1, 2)), 'cols'),
        (dict(x=mx, y=my, cols=(0, 5)), 'cols'),
        (dict(x=mx, y=my, cols=3), 'cols'),
        (dict(x=wide, y=wide), 'at most 64'),
        (dict(x=wide, y=wide, cols=(2, 67)), 'at most 64'),
        (dict(x=mx, y=my, scale=0.0), 'scale'),
        (dict(x=mx, y=my, scale=-2.0), 'scale'),
        (dict(x=mx, y=my, scale=float('inf')), 'scale'),
        (dict(x=mx, y=my, scale=float('nan')), 'scale'),
        (dict(x=mx.transpose(1, 2), y=my.transpose(1, 2)[:, :, :5]), 'strides'),          # the last dimension is not contiguous
        (dict(x=mx[:, :, :1].expand(2, 5, 4), y=my[:, :, :4]), 'strides'),
        (dict(x=mx[:, :1].expand(2, 5, 4), y=my), 'strides'),                            # rows 0 floats apart
        (dict(x=mx, y=my, x_len=[1, 6]), 'x_len'),
        (dict(x=mx, y=my, x_len=[1, -1]), 'x_len'),
        (dict(x=mx, y=my, x_len=[1]), 'x_len'),
        (dict(x=mx, y=my, x_len=torch.tensor([1.0, 2.0])), 'x_len'),
        (dict(x=mx, y=my, x_len=torch.tensor([1, 2, 3]).to('meta')), 'x_len'),
        (dict(x=mx, y=my, y_len=[7, 1]), 'y_len'),
        (dict(x=mx, y=my, y_len=torch.tensor([1.0, 2.0]).to('meta')), 'y_len'),
    ]
    for kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            ops.dtw(**kw)
    with pytest.raises(ValueError, match='scale'):
        metrics.dtw(mx, my, scale=0.0)
    for n_cep in (1, 0, 5):
        with pytest.raises(ValueError, match='n_cep'):
            metrics.mcd(mx, None, my, None, n_cep=n_cep)
    # arguments the kernel takes get as far as the library (and no further here)
    for kw in (dict(x_len=[5, 0], y_len=[0, 6]), dict(cols=(1, 3), scale=2.5, want_path=False), dict(x_len=torch.tensor([1, 2]).to('meta'))):
        with pytest.raises(AssertionError, match='reached the device'):
            ops.dtw(mx, my, **kw)
    with pytest.raises(AssertionError, match='reached the device'):
        ops.dtw(wide[:, :, 3:67], wide[:, :, 3:67])                    # a column slice keeps its row stride
    with pytest.raises(AssertionError, match='reached the device'):
        metrics.mcd(mx, [5, 5], my, [6, 6], n_cep=4)


def test_mcd_scale():
    from semi_tts_amd.metrics import MCD_SCALE
    assert abs(MCD_SCALE - (10.0 / math.log(10.0)) * math.sqrt(2.0) * 5.0 * math.log(10.0)) <= 1e-12
    assert abs(MCD_SCALE - 50.0 * math.sqrt(2.0)) <= 1e-12


# ---------------------------------------------------------------- main.py flags
def _entry():
    sys.path.insert(0, REPO)
    import main as entry
    return entry


CFG = ['--config', 'config/supervised.yaml']


def test_mcd_flags_parse():
    entry = _entry()
    p = entry.parse_args(CFG + ['--mcd-wav-dir', 'syn', '--mcd-ref-dir', 'ref', '--mcd-path', '--batch-size', '4'])
    assert (p.mcd_wav_dir, p.mcd_ref_dir, p.mcd_path, p.batch_size) == ('syn', 'ref', True, 4)
    p = entry.parse_args(CFG + ['--mcd-wav-dir', 'syn', '--mcd-ref-dir', 'ref'])
    assert p.mcd_path is False and p.feat_wav_dir is None
    p = entry.parse_args(CFG)
    assert p.mcd_wav_dir is None and p.mcd_ref_dir is None and p.mcd_path is False


_NO_COMBINE = '--mcd-wav-dir does not combine with --'
_MCD = ['--mcd-wav-dir', 'syn', '--mcd-ref-dir', 'ref']


@pytest.mark.parametrize('argv,msg', [
    (CFG + _MCD + ['--gen-specgram'], _NO_COMBINE + 'gen-specgram'),
    (CFG + _MCD + ['--tts-only'], _NO_COMBINE + 'tts-only'),
    (CFG + _MCD + ['--dev-batches', '2'], _NO_COMBINE + 'dev-batches'),
    (CFG + _MCD + ['--unpair-wav-dir', 'u'], _NO_COMBINE + 'unpair-wav-dir'),
    (CFG + _MCD + ['--transcribe-wav-dir', 't'], _NO_COMBINE + 'transcribe-wav-dir'),
    (CFG + _MCD + ['--align-wav-dir', 'a'], _NO_COMBINE + 'align-wav-dir'),
    (CFG + _MCD + ['--vocode-dir', 'v'], _NO_COMBINE + 'vocode-dir'),
    (CFG + _MCD + ['--resample-wav-dir', 'r', '--resample-out', 'o'], _NO_COMBINE + 'resample-wav-dir'),
    (CFG + _MCD + ['--feat-wav-dir', 'f', '--feat', 'mfcc'], _NO_COMBINE + 'feat-wav-dir'),
    (CFG + _MCD + ['--build-lm-phn-dir', 'p', '--lm', 'x.npy', '--lm-order', '2'], _NO_COMBINE + 'build-lm-phn-dir'),
    (CFG + ['--mcd-wav-dir', 'syn'], '--mcd-wav-dir needs --config (its data.audio) and --mcd-ref-dir DIR'),
    (_MCD, '--mcd-wav-dir needs --config (its data.audio) and --mcd-ref-dir DIR'),
    (CFG + ['--mcd-ref-dir', 'ref'], '--mcd-ref-dir and --mcd-path belong to --mcd-wav-dir'),
    (CFG + ['--mcd-path'], '--mcd-ref-dir and --mcd-path belong to --mcd-wav-dir'),
    (CFG + ['--feat-wav-dir', 'f', '--feat', 'mfcc', '--mcd-path'], '--mcd-ref-dir and --mcd-path belong to --mcd-wav-dir'),
    # --resample with this mode is out of scope: that flag's own check and message answer
    (CFG + _MCD + ['--resample'], '--resample converts the files of --unpair-wav-dir, --transcribe-wav-dir or --align-wav-dir'),
])
def test_mcd_flag_refusals(argv, msg, capsys):
    entry = _entry()
    with pytest.raises(SystemExit):
        entry.parse_args(argv)
    assert msg in capsys.readouterr().err


# ---------------------------------------------------------------- pairing
def test_pairing_maps_pred_files_and_names_a_missing_partner(tmp_path):
    from semi_tts_amd.solver import mcd_key, mcd_pairs
    assert [mcd_key(f) for f in ('a-pred.wav', 'dir/a.wav', 'p225_001-pred.mic1.wav', 'b-pred-pred.wav', 'c-predx.wav', '-pred.wav')] == \
        ['a', 'a', 'p225_001', 'b-pred', 'c-predx', '']
    syn, ref = tmp_path / 'syn', tmp_path / 'ref'
    syn.mkdir()
    ref.mkdir()
    with pytest.raises(ValueError, match='no .wav files'):
        mcd_pairs(str(syn), str(ref))
    for f in ('b.wav', 'a-pred.wav', 'c-pred.x.WAV', 'notes.txt'):
        (syn / f).write_bytes(b'')
    for f in ('a.wav', 'c.wav'):
        (ref / f).write_bytes(b'')
    with pytest.raises(ValueError, match=r'b\.wav has no recording .*ref.b\.wav'):
        mcd_pairs(str(syn), str(ref))
    (ref / 'b.wav').write_bytes(b'')
    assert mcd_pairs(str(syn), str(ref)) == [('a-pred.wav', 'a', 'a.wav'), ('b.wav', 'b', 'b.wav'), ('c-pred.x.WAV', 'c', 'c.wav')]
    (syn / 'b-pred.wav').write_bytes(b'')
    with pytest.raises(ValueError, match=r'b-pred\.wav and b\.wav share'):
        mcd_pairs(str(syn), str(ref))


def test_scorer_checks_every_file_before_any_device_work(tmp_path, monkeypatch):
    """McdScorer.load_data names an unreadable file, a foreign sample rate and an utterance too short for the MFCC (no GPU needed)"""
    import yaml
    from semi_tts_amd import solver, audio
    from semi_tts_amd.audio import write_wav
    monkeypatch.setattr(audio, '_device', lambda: (_ for _ in ()).throw(AssertionError('reached the device')))
    config = yaml.load(open(os.path.join(REPO, 'config', 'supervised.yaml')), Loader=yaml.FullLoader)
    sr = config['data']['audio']['sample_rate']
    syn, ref = tmp_path / 'syn', tmp_path / 'ref'
    syn.mkdir()
    ref.mkdir()
    rs = np.random.RandomState(0)

    class P:
        mcd_wav_dir, mcd_ref_dir, mcd_path, name, logdir, batch_size = str(syn), str(ref), False, 'mcd', str(tmp_path / 'log'), 4
    write_wav(str(syn / 'a-pred.wav'), 0.1 * rs.randn(sr // 2), sr)
    write_wav(str(ref / 'a.wav'), 0.1 * rs.randn(sr // 2), sr)
    write_wav(str(syn / 'b.wav'), 0.1 * rs.randn(sr // 2), sr)
    sc = solver.McdScorer(config, P(), 'test')
    with pytest.raises(ValueError, match=r'b\.wav has no recording'):
        sc.load_data()
    (ref / 'b.wav').write_bytes(b'not a wav file')
    with pytest.raises(ValueError, match=r'ref.b\.wav is not a readable'):
        sc.load_data()
    write_wav(str(ref / 'b.wav'), 0.1 * rs.randn(sr // 2), sr // 2)
    with pytest.raises(ValueError, match=r'Expected %d but get %d .*ref.b\.wav' % (sr, sr // 2)):
        sc.load_data()
    write_wav(str(ref / 'b.wav'), 0.1 * rs.randn(sr // 50), sr)             # 20 ms: fewer than 9 MFCC frames
    with pytest.raises(ValueError, match=r'ref.b\.wav.*(too short|fewer than 9|n_fft)'):
        sc.load_data()
    write_wav(str(ref / 'b.wav'), 0.1 * rs.randn(42 * sr), sr)              # 42 s: more frames than the warp takes
    with pytest.raises(ValueError, match=r'ref.b\.wav has %d MFCC frames' % (1 + 42 * sr // audio.mfcc_dims(sr)[1])):
        sc.load_data()
    write_wav(str(ref / 'b.wav'), 0.1 * rs.randn(sr // 3), sr)
    assert sc.load_data() is sc and [p[1] for p in sc.pairs] == ['a', 'b']
    assert not os.path.exists(P.logdir)                                     # nothing is written before exec
