"""Which GRU kernel a hidden size takes and how the BatchNorm column reductions cut their rows -- host arithmetic only, no GPU:
st_gru_seq_variant looks at H alone, st_colreduce_workspace_floats at (M, N).  Every row of the case tables (norm_rnn_cases.py) reaches
the variant / chunking named in it, and together the rows reach every GRU kernel, the refusal, and every chunking regime of the merge
kernels -- the GPU tests run the rows against float64 references."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import norm_rnn_cases as R   # noqa: E402
from semi_tts_amd import _lib   # noqa: E402


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libsemitts_hip.so is not built (python -m semi_tts_amd.build)')
    return _lib.load()


@pytest.mark.parametrize('c', R.GRU, ids=[c['id'] for c in R.GRU])
def test_gru_row_reaches_its_variant(lib, c):
    assert R.gru_name(lib.st_gru_seq_variant(c['H'], 0)) == c['fwd']
    assert R.gru_name(lib.st_gru_seq_variant(c['H'], 1)) == c['bwd']


def test_gru_rows_cover_every_variant_and_the_refusal(lib):
    fwd = {R.gru_name(lib.st_gru_seq_variant(c['H'], 0)) for c in R.GRU}
    bwd = {R.gru_name(lib.st_gru_seq_variant(c['H'], 1)) for c in R.GRU}
    assert fwd == {'tri', 'quad', 'general', 'refused'}, fwd
    assert bwd == {'tri', 'reg32', 'general', 'refused'}, bwd


def test_gru_variant_edges(lib):
    """every H from 1 to the refusal: the kernels hand over at 84 / 128 in both directions, nothing above 341, nothing below 1; the
    rows of the table sit on both sides of every edge"""
    def edges(bwd):
        names = [R.gru_name(lib.st_gru_seq_variant(H, bwd)) for H in range(0, R.GRU_MAX_H + 3)]
        return [(H, names[H]) for H in range(1, len(names)) if names[H] != names[H - 1]]
    assert edges(0) == [(1, 'tri'), (85, 'quad'), (129, 'general'), (342, 'refused')]
    assert edges(1) == [(1, 'tri'), (85, 'reg32'), (129, 'general'), (342, 'refused')]
    assert R.gru_name(lib.st_gru_seq_variant(0, 0)) == 'refused' and R.gru_name(lib.st_gru_seq_variant(-3, 1)) == 'refused'
    Hs = {c['H'] for c in R.GRU}
    for H, _ in edges(0) + edges(1):
        assert {H - 1, H} <= Hs | {0}, H


@pytest.mark.parametrize('c', R.BN_ROWS, ids=[c['id'] for c in R.BN_ROWS])
def test_bn_row_chunking(lib, c):
    for N in R.BN_N:
        ws = int(lib.st_colreduce_workspace_floats(c['M'], N))
        assert ws == 2 * c['chunks'] * N + 2 * N, (c['M'], N, ws)          # (chunks) x (2, N) records + the 2N sums
    assert R.chunking(c['M']) == (c['chunks'], c['rpc'], c['empty'], c['last'])
    assert (c['chunks'] - c['empty'] - 1) * c['rpc'] + c['last'] == c['M']


def test_bn_rows_cover_every_chunking_regime(lib):
    rows = R.BN_ROWS
    assert any(c['chunks'] == 1 and c['M'] < R.CHUNK_ROWS for c in rows)                 # fewer rows than one chunk's worth
    assert any(1 < c['chunks'] < R.MERGE_LANES for c in rows)                            # every chunk in register slot 0
    assert any(R.MERGE_LANES < c['chunks'] < R.MAX_CHUNKS for c in rows)                 # slots j >= 1, partly filled
    assert any(c['chunks'] == R.MAX_CHUNKS and c['rpc'] == R.CHUNK_ROWS for c in rows)   # all 8 slots of all lanes, no cap reached
    assert any(c['chunks'] == R.MAX_CHUNKS and c['M'] > R.MAX_CHUNKS * R.CHUNK_ROWS for c in rows)    # the 128-chunk cap
    assert any(c['empty'] >= 1 and c['chunks'] < R.MAX_CHUNKS for c in rows)
    assert any(c['empty'] >= 2 and c['chunks'] == R.MAX_CHUNKS for c in rows)           # trailing empty chunks at the cap
    assert any(c['last'] == 1 and c['chunks'] > 1 for c in rows)                         # a one-row last chunk
    assert any(c['M'] == 1 for c in rows)
    assert {c['M'] for c in rows} >= {2064, 4128, 8256, 16512}                           # the production row counts
    # the statistics test's (M, N, layout) rows reach every M, every N and both column windows
    st = R.bn_stat_rows()
    assert {m for m, _, _ in st} == {c['M'] for c in rows}
    assert {n for _, n, _ in st} == set(R.BN_N) and {lay for _, _, lay in st} == set(R.BN_LAYOUTS)
