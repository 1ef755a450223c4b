"""CPU checks that pin what the directory tools of main.py say in load_data, word for word, before any device work: the messages of the
tools differ in small ways (bare file name or path, the flag named, the widths and channels refused) that shared helpers must keep.
Every tool is addressed through semi_tts_amd.solver.  Also the 16-bit writer against write_wav and WaveBatch.inverse against argsort."""
import os
import types
import wave

import numpy as np
import pytest
import yaml

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUDIO = dict(num_freq=257, num_mels=40, frame_length_ms=25, frame_shift_ms=10, preemphasis_coeff=0.97, sample_rate=16000)
CONFIG = dict(data=dict(audio=AUDIO))


def _wav(path, frames=100, rate=16000, width=2, channels=1):
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(channels)
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(b'\0' * (frames * width * channels))


def _truncated(path):
    """a .wav cut after its format chunk, before the samples: -> what `wave` says when it refuses the file"""
    _wav(path)
    data = open(str(path), 'rb').read()
    open(str(path), 'wb').write(data[:36])
    with pytest.raises((OSError, EOFError, wave.Error)) as e:
        wave.open(str(path), 'rb')
    assert str(e.value)
    return str(e.value)


def _message(tool):
    with pytest.raises(ValueError) as e:
        tool.load_data()
    return str(e.value)


# ---------------------------------------------------------------- Resampler, LoudnessWriter, Trimmer: the bare file name
WRITERS = {
    'resample': ('Resampler', dict(resample_rate=16000)),
    'loudness': ('LoudnessWriter', dict(loudness_target=-23.0, loudness_peak=-1.0, loudness_max_gain=30.0)),
    'trim': ('Trimmer', dict(trim_top_db=60.0, trim_frame_length=2048, trim_hop=512, trim_pad_ms=0.0)),
}


def _writer(kind, src, dst):
    from semi_tts_amd import solver
    name, extra = WRITERS[kind]
    paras = types.SimpleNamespace(batch_size=4, verbose=False, **extra)
    setattr(paras, kind + '_wav_dir', str(src))
    setattr(paras, kind + '_out', str(dst))
    return getattr(solver, name)(CONFIG, paras, 'test')


@pytest.mark.parametrize('kind', sorted(WRITERS))
def test_writers_name_the_bare_file_and_their_flag(kind, tmp_path):
    src, dst = tmp_path / 'in', tmp_path / 'out'
    src.mkdir()
    assert _message(_writer(kind, src, dst)) == '--%s-wav-dir %s: no .wav files' % (kind, src)
    (src / 'notes.txt').write_bytes(b'')
    assert _message(_writer(kind, src, dst)) == '--%s-wav-dir %s: no .wav files' % (kind, src)
    _wav(src / 'a.wav', width=1)
    assert _message(_writer(kind, src, dst)) == '--%s-wav-dir: a.wav is 8-bit; only 16-bit PCM is read' % kind
    _wav(src / 'a.wav', frames=0)
    assert _message(_writer(kind, src, dst)) == '--%s-wav-dir: a.wav holds no samples' % kind
    _wav(src / 'a.wav', rate=22050)
    if kind == 'resample':
        assert _writer(kind, src, dst).load_data().files == ['a.wav']
    else:
        assert _message(_writer(kind, src, dst)) == 'Sample rate mismatch. Expected 16000 but get 22050 (a.wav)'
    same = str(tmp_path) + '/./in/'
    assert _message(_writer(kind, src, same)) == '--%s-out %s is the directory --%s-wav-dir reads' % (kind, same, kind)
    (src / 'a.wav').write_bytes(b'not a wav')                          # an unreadable file is wave's own error, not a ValueError
    with pytest.raises((EOFError, wave.Error)):
        _writer(kind, src, dst).load_data()
    assert not dst.exists()


# ---------------------------------------------------------------- FeatureWriter, Transcriber, Aligner: the empty directory
def test_an_empty_directory_names_the_flag_of_each_tool(tmp_path, monkeypatch):
    from semi_tts_amd import audio, solver

    class Conv:
        n_mels = 80
    monkeypatch.setattr(audio, 'load_audio_transform', lambda **kw: Conv())
    (tmp_path / 'notes.txt').write_bytes(b'')
    paras = types.SimpleNamespace(feat_wav_dir=str(tmp_path), feat='mfcc', batch_size=4, verbose=False)
    assert _message(solver.FeatureWriter(CONFIG, paras, 'test')) == '--feat-wav-dir %s: no .wav files' % tmp_path
    for cls, attr, flag in ((solver.Transcriber, 'transcribe_wav_dir', '--transcribe-wav-dir'), (solver.Aligner, 'align_wav_dir', '--align-wav-dir')):
        tool = cls.__new__(cls)                                          # (no GPU needed: the solver's constructor is bypassed)
        tool.config, tool.n_mels = {'data': {'audio': {}}}, 80
        tool.paras = types.SimpleNamespace(phn_dir=None, vocab=None, **{attr: str(tmp_path)})
        assert _message(tool) == '%s %s: no .wav files' % (flag, tmp_path)


# ---------------------------------------------------------------- McdScorer, StoiScorer, AbxScorer: the path, a ValueError for an unreadable file
@pytest.fixture
def no_device(monkeypatch):
    from semi_tts_amd import audio
    monkeypatch.setattr(audio, '_device', lambda: (_ for _ in ()).throw(AssertionError('reached the device')))


def _supervised():
    return yaml.load(open(os.path.join(REPO, 'config', 'supervised.yaml')), Loader=yaml.FullLoader)


def test_mcd_scorer_names_the_path(tmp_path, no_device):
    from semi_tts_amd import solver
    config = _supervised()
    sr = config['data']['audio']['sample_rate']
    syn, ref = tmp_path / 'syn', tmp_path / 'ref'
    syn.mkdir()
    ref.mkdir()
    paras = types.SimpleNamespace(mcd_wav_dir=str(syn), mcd_ref_dir=str(ref), mcd_path=False, name='mcd', logdir=str(tmp_path / 'log'), batch_size=4)
    assert _message(solver.McdScorer(config, paras, 'test')) == '--mcd-wav-dir %s: no .wav files' % syn
    _wav(ref / 'a.wav', frames=sr // 2, rate=sr)
    path = str(syn / 'a.wav')
    why = _truncated(path)
    assert _message(solver.McdScorer(config, paras, 'test')) == '--mcd-wav-dir: %s is not a readable .wav file (%s)' % (path, why)
    _wav(path, frames=sr // 2, rate=sr, width=1)
    assert _message(solver.McdScorer(config, paras, 'test')) == '--mcd-wav-dir: %s is 8-bit; only 16-bit PCM is read' % path
    _wav(path, frames=sr // 2, rate=sr // 2)
    assert _message(solver.McdScorer(config, paras, 'test')) == '--mcd-wav-dir: sample rate mismatch. Expected %d but get %d (%s)' % (sr, sr // 2, path)
    assert not (tmp_path / 'log').exists()


def test_stoi_scorer_names_the_path_and_refuses_stereo(tmp_path, no_device):
    from semi_tts_amd import solver
    syn, ref = tmp_path / 'syn', tmp_path / 'ref'
    syn.mkdir()
    ref.mkdir()
    paras = types.SimpleNamespace(stoi_wav_dir=str(syn), stoi_ref_dir=str(ref), stoi_max_len_diff=0.05, batch_size=2, name='run',
                                  logdir=str(tmp_path / 'log'), verbose=False)
    assert _message(solver.StoiScorer(None, paras, 'test')) == '--stoi-wav-dir %s: no .wav files' % syn
    _wav(ref / 'a.wav', frames=4000, rate=10000)
    path = str(syn / 'a.wav')
    why = _truncated(path)
    assert _message(solver.StoiScorer(None, paras, 'test')) == '--stoi-wav-dir: %s is not a readable .wav file (%s)' % (path, why)
    _wav(path, frames=4000, rate=10000, channels=2)
    assert _message(solver.StoiScorer(None, paras, 'test')) == '--stoi-wav-dir: %s is 16-bit with 2 channels; only 16-bit mono PCM is read' % path
    _wav(path, frames=4000, rate=10000, width=1)
    assert _message(solver.StoiScorer(None, paras, 'test')) == '--stoi-wav-dir: %s is 8-bit with 1 channels; only 16-bit mono PCM is read' % path
    _wav(path, frames=0, rate=10000)
    assert _message(solver.StoiScorer(None, paras, 'test')) == '--stoi-wav-dir: %s holds no samples' % path
    assert not (tmp_path / 'log').exists()


def test_abx_scorer_names_the_path(tmp_path, no_device):
    from semi_tts_amd import solver
    config = _supervised()
    sr = config['data']['audio']['sample_rate']
    ali, wav = tmp_path / 'ali', tmp_path / 'wav'
    ali.mkdir()
    wav.mkdir()
    (ali / 'a.ali').write_text('# score=-12.500000 frames=20 frame_s=0.050000\nAA\t0\t20\n')
    paras = types.SimpleNamespace(abx_ali_dir=str(ali), abx_wav_dir=str(wav), name='abx', logdir=str(tmp_path / 'log'), batch_size=4, abx_spk_map=None,
                                  resample=False)
    path = str(wav / 'a.wav')
    why = _truncated(path)
    assert _message(solver.AbxScorer(config, paras, 'test')) == '--abx-wav-dir: %s is not a readable .wav file (%s)' % (path, why)
    _wav(path, frames=sr // 2, rate=sr // 2)
    assert _message(solver.AbxScorer(config, paras, 'test')) == \
        '--abx-wav-dir: sample rate mismatch. Expected %d but get %d (%s); --resample converts it' % (sr, sr // 2, path)
    _wav(path, frames=sr // 2, rate=sr, width=1)                        # no sample width is checked here
    assert solver.AbxScorer(config, paras, 'test').load_data().pairs[0][2] == 'a.wav'
    assert not (tmp_path / 'log').exists()


# ---------------------------------------------------------------- the 16-bit writer and the inverse of a batch's order
@pytest.mark.parametrize('x', [[0.25, -0.5], [1.0], [1.5, -2.0, 0.99999, -1.0, 0.0]])
def test_write_pcm16_writes_what_write_wav_writes(x, tmp_path):
    from semi_tts_amd import audio
    audio.write_wav(str(tmp_path / 'a.wav'), x, 22050)
    pcm = np.rint(np.clip(np.asarray(x, np.float64), -1.0, 1.0) * 32767.0).astype(np.int16)
    audio.write_pcm16(str(tmp_path / 'b.wav'), pcm, 22050)
    audio.write_pcm16(str(tmp_path / 'c.wav'), pcm.astype(np.int64)[::-1][::-1], 22050.0)        # (any integer array, any layout)
    want = (tmp_path / 'a.wav').read_bytes()
    assert (tmp_path / 'b.wav').read_bytes() == want and (tmp_path / 'c.wav').read_bytes() == want
    got, sr = audio._read_pcm(str(tmp_path / 'b.wav'))
    assert sr == 22050 and got[:, 0].tolist() == pcm.tolist()


@pytest.mark.parametrize('lens', [[5, 5, 3, 5, 1], [7]])
def test_wave_batch_inverse_is_the_argsort_of_its_order(lens):
    import torch
    from semi_tts_amd.audio import WaveBatch
    wb = WaveBatch([torch.zeros(n) for n in lens])
    inv = wb.inverse()
    assert inv.tolist() == np.argsort(wb.order).tolist() == np.argsort(wb.order, kind='stable').tolist()
    assert wb.order[inv].tolist() == list(range(len(lens))) and wb.lens[inv].tolist() == lens
