"""semi_tts_amd.corpus on the host: the four readers, encode, every refusal, the drop counts, the sampler against restatements of
VCTKDataset.__getitem__ (corpus/vctk.py:41-47) and the DataLoader settings of src/data.py:35-63, and main.py's flag refusals.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import corpus_cases as CC   # noqa: E402
from semi_tts_amd import corpus as C   # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = ['--config', os.path.join(REPO, 'config', 'semi-single-spkr-paired-data.yaml')]


@pytest.fixture(scope='module')
def toy(tmp_path_factory):
    return CC.write_toy_corpus(tmp_path_factory.mktemp('corpus'))


# ------------------------------------------------------------------------------------------------------------------ readers, encode
def test_the_four_readers(toy):
    cfg, rows = toy
    table = C.read_partition_table(cfg['partition_table'])
    assert [(r['id'], r['speaker'], r['split']) for r in table] == [(r['id'], r['speaker'], r['split']) for r in rows]
    assert all(abs(t['duration'] - r['samples'] / CC.SR) < 1e-3 for t, r in zip(table, rows))
    assert C.read_spkr_map(cfg['spkr_map']) == CC.SPEAKERS
    mt = C.read_map_table(cfg['map_table'])
    assert {k: (v['phn_seq'], v['spkr']) for k, v in mt.items()} == {r['id']: (r['phn_seq'], r['speaker']) for r in rows}
    assert any('  ' in v['phn_seq'] for v in mt.values())
    co = C.Corpus(**cfg)
    assert co.vocab_size == 3 + len(CC.VOCAB) == 9 and co.n_spkr == 2 and co.vocab[3:] == CC.VOCAB
    assert {s: len(co.rows[s]) for s in C.USED_SPLITS} == dict(CC.N_SPLIT)
    for u, r in zip([u for s in C.USED_SPLITS for u in co.rows[s]], rows):
        assert u.id == r['id'] and u.sid == CC.SPEAKERS[r['speaker']] and u.text == r['tokens']
        assert u.path == os.path.join(cfg['path'], r['speaker'], r['id'] + '.wav')
    got = co.measure('paired', CC.SR)
    assert [u.samples for u in got] == [r['samples'] for r in rows if r['split'] == 'paired']


def test_encode_is_the_reference_encoder():
    v2i = {v: 3 + i for i, v in enumerate(CC.VOCAB)}
    assert C.encode('AA B', v2i) == [3, 4, 0]
    assert C.encode('AA  B', v2i) == [3, 1, 4, 0]                       # a double space: one empty piece -> <space>
    assert C.encode(' AA   F \r\n', v2i) == [3, 1, 1, 8, 0]             # stripped first; two empty pieces inside
    assert C.encode('', v2i) == [1, 0]                                  # ''.split(' ') == ['']
    with pytest.raises(ValueError, match=r"pa_007.*'ZH'"):
        C.encode('AA ZH', v2i, 'pa_007')


# ------------------------------------------------------------------------------------------------------------------ refusals
def _broken(tmp_path, mutate, waves=True, **kw):
    rows = CC.toy_rows()
    extra = mutate(rows) or {}
    cfg = CC.write_tables(tmp_path, rows, **extra)
    if waves:
        CC.write_waves(cfg, [r for r in rows if not r.get('no_wav')])
    return cfg


def test_refusals_name_the_offenders(tmp_path):
    def unknown_speaker(rows):
        rows[1]['speaker'] = rows[12]['speaker'] = 'p999'
    with pytest.raises(ValueError, match=r'speaker not in spkr_map.*pa_001 \(p999\).*un_002'):
        C.Corpus(**_broken(tmp_path / 'a', unknown_speaker, waves=False))

    def no_transcript(rows):
        rows[3]['phn_seq'] = rows[17]['phn_seq'] = None
    with pytest.raises(ValueError, match=r'no transcript for: pa_003, de_001'):
        C.Corpus(**_broken(tmp_path / 'b', no_transcript, waves=False))

    def unknown_symbol(rows):
        rows[11]['phn_seq'] = 'AA QQ B'
    with pytest.raises(ValueError, match=r"un_001.*'QQ'"):
        C.Corpus(**_broken(tmp_path / 'c', unknown_symbol, waves=False))

    def no_wav(rows):
        for i in range(0, 14, 2):
            rows[i]['no_wav'] = True
    with pytest.raises(ValueError, match=r'no such \.wav: .*pa_000\.wav.*pa_008\.wav \.\.\. \(7 in all\)') as e:
        C.Corpus(**_broken(tmp_path / 'd', no_wav))
    assert 'un_000' not in str(e.value)                                   # the first few only

    def bad_split(rows):
        rows[0]['split'] = 'train'
    with pytest.raises(ValueError, match=r'split must be one of.*pa_000 \(train\)'):
        C.Corpus(**_broken(tmp_path / 'e', bad_split, waves=False))

    def twice(rows):
        rows[5]['id'] = rows[4]['id']
    with pytest.raises(ValueError, match='more than once: pa_004'):
        C.Corpus(**_broken(tmp_path / 'f', twice, waves=False))


def test_table_without_a_column_and_bad_speaker_map(tmp_path, toy):
    cfg, _ = toy
    p = tmp_path / 'part.csv'
    p.write_text(',speaker,split\nx,lj,paired\n')
    with pytest.raises(ValueError, match='lacks the column.*duration'):
        C.read_partition_table(str(p))
    m = tmp_path / 'map.tsv'
    m.write_text('file,phn_seq,spkr\nx,AA,lj\n')                          # commas: not the tab-separated layout
    with pytest.raises(ValueError, match='lacks the column'):
        C.read_map_table(str(m))
    j = tmp_path / 's.json'
    j.write_text('{"lj": 0, "p225": 5}')
    with pytest.raises(ValueError, match=r'ids must lie in \[0, 2\).*p225'):
        C.read_spkr_map(str(j))


def test_foreign_rate_raises_unless_resampled(tmp_path):
    rows = CC.toy_rows()
    cfg = CC.write_tables(tmp_path, rows)
    CC.write_waves(cfg, rows[:1], sr=16000)
    CC.write_waves(cfg, rows[1:])
    co = C.Corpus(**cfg)
    with pytest.raises(ValueError, match='Sample rate mismatch. Expected 22050 but get 16000'):
        co.measure('paired', CC.SR)
    got = co.measure('paired', CC.SR, resample=True)
    assert got[0].rate == 16000 and got[0].samples == -(-rows[0]['samples'] * 22050 // 16000)       # ceil(L new / orig)


# ------------------------------------------------------------------------------------------------------------------ drops
def test_drop_counts_and_report():
    mk = lambda n, toks: type('U', (), dict(samples=n, text=[3] * toks + [0]))()   # noqa: E731
    rows = [mk(512, 2), mk(513, 2), mk(20000, 126), mk(20000, 127), mk(275 * 99, 3), mk(275 * 100, 3), mk(100, 200)]
    kept, counts = C.select(rows, n_fft=1024, hop=275, max_tokens=127, max_frames=100)
    assert counts == dict(short=2, tokens=1, frames=1)                    # (the last row is short first: one rule per utterance)
    assert kept == [rows[1], rows[2], rows[4]]
    kept, counts = C.select(rows, n_fft=1024, hop=275, max_tokens=127)
    assert counts == dict(short=2, tokens=1, frames=0) and len(kept) == 4
    line = C.drop_report('paired', len(rows), dict(short=2, tokens=1, frames=1), 1024, 127, 100)
    assert '\n' not in line and line.startswith('paired: 3 of 7 utterances kept')
    assert '2 of 512 samples or fewer' in line and '1 over 127 tokens' in line and '1 over 100 frames' in line


def test_the_token_limit_is_the_ctc_kernels():
    from semi_tts_amd import ops
    assert ops.CTC_MAX_TOKENS == 127 and ops.CTC_TC == 16


# ------------------------------------------------------------------------------------------------------------------ sampler
LENS = [50, 90, 70, 90, 10, 30, 80, 20, 60, 40, 75]                       # N = 11; a tie (90, 90): stable


def _sorted_rows(lens):
    return sorted(range(len(lens)), key=lambda i: -lens[i])               # Python's sort is stable


def test_sampler_bucketing_windows_as_vctk_getitem():
    B = 4
    s = C.Sampler(LENS, B, bucketing=True, train=True, seed=3)
    table = _sorted_rows(LENS)
    assert table[:2] == [1, 3] and list(s.rows) == table
    ep = s.epoch(0)
    perm = np.random.RandomState([3, 0, 0]).permutation(len(LENS))
    assert len(ep) == len(LENS) == s.n_batches()
    for index, batch in zip(perm, ep):
        index = min(len(table) - B, int(index))                           # corpus/vctk.py:44-45
        assert list(batch) == table[index:index + B]
    assert sorted(int(b[0]) for b in ep) != [int(b[0]) for b in ep]       # shuffled
    assert sum(list(b) == table[-B:] for b in ep) == B                    # the starts N - B .. N - 1 clamp to the last window


def test_sampler_without_bucketing_permutes_and_drops_the_remainder():
    B = 4
    s = C.Sampler(LENS, B, bucketing=False, train=True, seed=3)
    table = np.array(_sorted_rows(LENS))
    ep = s.epoch(2)
    perm = np.random.RandomState([3, 0, 2]).permutation(len(LENS))
    assert len(ep) == len(LENS) // B == s.n_batches() == 2
    assert [list(b) for b in ep] == [list(table[perm[0:4]]), list(table[perm[4:8]])]
    assert len({int(i) for b in ep for i in b}) == 8


def test_sampler_dev_in_order_with_the_remainder():
    s = C.Sampler(LENS, 4, bucketing=True, train=False, seed=3)           # bucketing does not apply to dev (corpus/vctk.py:21)
    table = _sorted_rows(LENS)
    assert [list(b) for b in s.epoch(0)] == [table[0:4], table[4:8], table[8:11]] == [list(b) for b in s.epoch(5)]
    assert s.n_batches() == 3
    walked = [list(s.next()) for _ in range(4)]
    assert walked[3] == walked[0] == table[0:4]                           # restarts
    s.next()
    s.rewind()
    assert list(s.next()) == table[0:4]


def test_sampler_small_split_gives_one_batch_of_all_rows():
    for train, bucket in ((True, True), (True, False), (False, False)):
        s = C.Sampler(LENS[:3], 4, bucketing=bucket, train=train)
        assert [list(b) for b in s.epoch(0)] == [[1, 2, 0]] and s.n_batches() == 1
        assert list(s.next()) == list(s.next()) == [1, 2, 0]


def test_sampler_repeats_for_the_same_seed_rank_epoch_and_differs_otherwise():
    key = lambda s, e: [tuple(b) for b in s.epoch(e)]      # noqa: E731
    a, b = C.Sampler(LENS, 4, seed=7, rank=1, world=2), C.Sampler(LENS, 4, seed=7, rank=1, world=2)
    np.random.seed(0)
    first = key(a, 0)
    np.random.rand(10)                                                    # the global generator is not the sampler's
    assert first == key(b, 0) and key(a, 3) == key(b, 3)
    assert key(a, 0) != key(a, 1)
    assert key(a, 0) != key(C.Sampler(LENS, 4, seed=8, rank=1, world=2), 0)
    it = [tuple(a.next()) for _ in range(3)]                              # N = 5 on this rank: one batch per epoch
    assert it == [key(b, 0)[0], key(b, 1)[0], key(b, 2)[0]]


def test_sampler_ranks_are_disjoint_and_complete():
    table = _sorted_rows(LENS)
    shards = [C.Sampler(LENS, 2, train=False, rank=k, world=3) for k in range(3)]
    for k, s in enumerate(shards):
        assert list(s.rows) == table[k::3]
    rows = [int(i) for s in shards for b in s.epoch(0) for i in b]
    assert sorted(rows) == list(range(len(LENS)))
    with pytest.raises(ValueError, match='no utterance for rank 2 of 3'):
        C.Sampler(LENS[:2], 2, rank=2, world=3)


# ------------------------------------------------------------------------------------------------------------------ main.py
@pytest.mark.parametrize('extra,msg', [
    (['--corpus', '--unpair-wav-dir', 'x'], '--corpus trains on the splits of data.corpus'),
    (['--corpus', '--gen-specgram'], 'does not combine with --gen-specgram'),
    (['--corpus', '--transcribe-wav-dir', 'x'], 'does not combine with --transcribe-wav-dir'),
    (['--corpus-max-gb', '2'], 'belong to --corpus'),
    (['--max-frames', '400'], 'belong to --corpus'),
    (['--corpus', '--corpus-max-gb', '0'], 'finite and positive'),
    (['--corpus', '--max-frames', '0'], '--max-frames must be >= 1'),
    (['--dev-batches', '-1'], '--dev-batches must be >= 0'),
    (['--corpus', '--dev-batches', '-2'], '--dev-batches must be >= 0'),
    (['--corpus', '--tts-only', '--dev-batches', '-1'], 'does not combine with --tts-only'),
])
def test_main_refuses(extra, msg, capsys):
    sys.path.insert(0, REPO)
    import main as entry
    with pytest.raises(SystemExit):
        entry.parse_args(CFG + extra)
    assert msg in capsys.readouterr().err


def test_main_accepts_the_corpus_flags(capsys):
    sys.path.insert(0, REPO)
    import main as entry
    p = entry.parse_args(CFG + ['--corpus', '--dev-batches', '-1', '--actual-len', '--max-frames', '800', '--corpus-max-gb', '1.5', '--resample'])
    assert p.corpus and p.dev_batches == -1 and p.actual_len and p.max_frames == 800 and p.corpus_max_gb == 1.5
    p = entry.parse_args(CFG + ['--corpus', '--tts-only'])
    assert p.corpus and p.tts_only and p.corpus_max_gb is None and p.max_frames is None
    assert 'actual-len' not in capsys.readouterr().out                    # no longer announced as having no effect
    assert 'no effect' not in entry.parser.format_help().split('--actual-len')[1].split('--store-best-per')[0]
