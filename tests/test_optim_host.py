"""The multi-tensor optimiser's host arithmetic and the references of its GPU test -- no GPU: st_mt_launch_plan and st_mt_blocks look at
sizes only and never touch memory, and mt_run / st_mt_copy (optim.hip) cut a list into launches through the code the query runs.  Every
row of the split tables (optim_cases.py) reaches the split named in it, the rule restated there agrees with the library over a sweep,
the float64 Adam reference is float64 torch.optim.Adam, and an fp32 emulation of the kernel's operation sequence stays inside the
derived bounds -- the GPU test (test_gpu_optim.py) runs the kernels against those references and bounds."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_cases as OC   # noqa: E402
from semi_tts_amd import _lib   # noqa: E402


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libsemitts_hip.so is not built (python -m semi_tts_amd.build)')
    return _lib.load()


def lib_plan(lib, sizes, kind=0, cap=64):
    """[(tensor slots, blocks)] per launch as the library reports it, None for a refusal"""
    n = (C.c_long * len(sizes))(*sizes)
    b, t = (C.c_int * cap)(), (C.c_int * cap)()
    k = lib.st_mt_launch_plan(n, len(sizes), kind, b, t, cap)
    if k < 0:
        return None
    assert k <= cap
    return [(t[i], b[i]) for i in range(k)]


def lib_blocks(lib, sizes):
    return int(lib.st_mt_blocks((C.c_long * len(sizes))(*sizes), len(sizes)))


# ------------------------------------------------------------------------------------------------ rows reach their splits
@pytest.mark.parametrize('c', OC.SPLIT_ROWS, ids=[c['id'] for c in OC.SPLIT_ROWS])
def test_split_row_reaches_its_launches(lib, c):
    assert lib_plan(lib, c['sizes']) == c['want'] == OC.plan(c['sizes'])
    assert c['reach'] in OC.reaches(c['want'], c['sizes'])
    assert sum(b for _, b in c['want']) == lib_blocks(lib, c['sizes']) == OC.blocks(c['sizes'])


@pytest.mark.parametrize('c', OC.COPY_SPLIT_ROWS, ids=[c['id'] for c in OC.COPY_SPLIT_ROWS])
def test_copy_split_row_reaches_its_launches(lib, c):
    assert lib_plan(lib, c['sizes'], kind=1) == c['want'] == OC.plan(c['sizes'], kind=1)


def test_rows_reach_every_split_case():
    """a launch filled by tensors, a launch filled by blocks, a tensor cut across launches, the single launch -- and the row that fills
    slots and blocks of one launch at once and starts the next at slot 0 with the rest of the same tensor"""
    got = set()
    for c in OC.SPLIT_ROWS:
        got |= OC.reaches(c['want'], c['sizes'])
    assert got == {'single', 'tensors', 'blocks', 'cut'}
    assert {len(c['sizes']) for c in OC.SPLIT_ROWS} >= {24, 25, 48, 49}
    assert (OC.MT_T, OC.MT_NB) in [c['want'][0] for c in OC.SPLIT_ROWS]
    got = set()
    for c in OC.COPY_SPLIT_ROWS:
        got |= OC.reaches(c['want'], c['sizes'], kind=1)
    assert got == {'single', 'tensors', 'blocks', 'cut'}


def test_size_table_has_every_loop_round_and_chunk_edge():
    want = {1, 2, 3, 4, 5, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 32767, 32768, 32769, 65535, 65536,
            65537, 3 * 32768 + 5}
    assert set(OC.SIZES) == want and len(OC.SIZES) == len(want) and OC.OFFSETS == (0, 1, 2, 3)
    assert len({name for _, name in OC.SIZE_ROWS}) == len(OC.SIZE_ROWS)


# ------------------------------------------------------------------------------------------------ the rule itself
def test_python_rule_agrees_with_the_library_on_a_sweep(lib):
    rng = random.Random(7)
    bad = []
    for trial in range(1500):
        kind = trial % 2
        T, NB, chunk, _ = OC.LIMITS[kind]
        nt = rng.choice([1, 2, 5, T - 1, T, T + 1, 2 * T, 2 * T + 1, 130])
        pick = [0, -3, 1, chunk - 1, chunk, chunk + 1, 7 * chunk + 3, (NB - T) * chunk, NB * chunk, NB * chunk + 1, (2 * NB + 5) * chunk]
        sizes = [rng.choice(pick) if rng.random() < 0.5 else rng.randrange(0, 3 * chunk) for _ in range(nt)]
        got = lib_plan(lib, sizes, kind, cap=512)
        if got != OC.plan(sizes, kind):
            bad.append((kind, sizes))
        elif kind == 0:
            assert sum(b for _, b in got) == lib_blocks(lib, sizes)
            assert all(1 <= t <= T and 1 <= b <= NB and t <= b for t, b in got)
    assert not bad, bad[:3]


def test_blocks_and_refusals(lib):
    ch = OC.MT_CHUNK
    for sizes, want in (([0], 0), ([-1], 0), ([-ch], 0), ([1], 1), ([ch - 1], 1), ([ch], 1), ([ch + 1], 2), ([2 * ch], 2), ([2 * ch + 1], 3),
                        ([0, ch, -5, ch + 1, 0], 3), ([65535 * ch], 65535), ([65535 * ch + 1], 65536)):
        assert lib_blocks(lib, sizes) == want == OC.blocks(sizes), sizes
    # a list of empty tensors: no launch; the chunk index has 16 bits: 65535 chunks are taken (103 launches), one more float is refused
    assert lib_plan(lib, [0, -4, 0]) == [] == OC.plan([0, -4, 0])
    top = lib_plan(lib, [65535 * ch], cap=128)
    assert top == OC.plan([65535 * ch]) and len(top) == 103 and sum(b for _, b in top) == 65535
    assert lib_plan(lib, [5, 65535 * ch + 1]) is None and OC.plan([5, 65535 * ch + 1]) is None
    assert lib_plan(lib, [65535 * OC.MC_CHUNK - 1], kind=1, cap=128) == OC.plan([65535 * OC.MC_CHUNK - 1], kind=1)
    assert lib_plan(lib, [65535 * OC.MC_CHUNK], kind=1) is None and OC.plan([65535 * OC.MC_CHUNK], kind=1) is None
    # bad arguments; more launches than the caller's arrays hold are counted, not written
    n = (C.c_long * 3)(ch, 641 * ch, 1)
    b, t = (C.c_int * 2)(-7, -7), (C.c_int * 2)(-7, -7)
    assert lib.st_mt_launch_plan(None, 3, 0, b, t, 2) < 0 and lib.st_mt_launch_plan(n, 0, 0, b, t, 2) < 0
    assert lib.st_mt_launch_plan(n, 3, 2, b, t, 2) < 0 and lib.st_mt_launch_plan(n, 3, 0, None, None, 2) < 0
    assert lib.st_mt_launch_plan(n, 3, 0, b, t, 1) == 2 and (b[0], t[0], b[1], t[1]) == (640, 2, -7, -7)
    assert lib.st_mt_launch_plan(n, 3, 0, None, None, 0) == 2


def test_table_lru_model():
    lru = OC.TableLru(primed=range(100, 116))
    assert [lru.use(k) for k in (115, 100, 1, 101, 100)] == [False, False, True, True, False]        # 1 evicted 101
    assert len(lru.order) == OC.MT_TABS and lru.order[-3:] == [1, 101, 100] and 102 not in lru.order


# ------------------------------------------------------------------------------------------------ references and bounds
def test_adam_ref_is_float64_torch_adam():
    g0 = torch.Generator().manual_seed(1)
    p = torch.randn(257, generator=g0, dtype=torch.float64)
    ref = p.clone().requires_grad_()
    opt = torch.optim.Adam([ref], lr=1e-3)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for step in range(1, 6):
        lr = 1e-3 * step
        opt.param_groups[0]['lr'] = lr
        grad = torch.randn(257, generator=g0, dtype=torch.float64) * 10.0 ** (step - 3)
        ref.grad = grad.clone()
        opt.step()
        p, m, v, denom, q = OC.adam_ref(p, grad, m, v, *OC.adam_scalars(step, lr), exact_scalars=True)
        assert torch.allclose(p, ref.detach(), rtol=0, atol=1e-15) and bool((denom > 0).all())
        st = opt.state[ref]
        # (a few float64 roundings in another association: 1e-14 of each moment's own scale)
        for mine, theirs in ((m, st['exp_avg']), (v, st['exp_avg_sq'])):
            assert torch.allclose(mine, theirs, rtol=0, atol=1e-14 * float(theirs.abs().max()))


def test_fp32_emulation_stays_inside_adam_bound():
    """the kernel's sequence with every operation correctly rounded, over 6 x 8192 elements of adam_operands and the scalar sets of the
    GPU test: the worst error / bound ratio per output is below 1 (and above 0.5: the bounds are not slack by more than the 2x the GPU
    test allows on top)"""
    worst = dict(p=0.0, m=0.0, v=0.0)
    for i, (step, lr) in enumerate([(1, 1e-3), (2, 1e-3), (10000, 1e-3), (1, 1.0), (2, 1.0), (10000, 1.0)]):
        p, g, m, v = OC.adam_operands(8192, seed=20 + i)
        sc = OC.adam_scalars(step, lr)
        ref = OC.adam_ref(p, g, m, v, *sc)
        bound = OC.adam_bound(p, g, m, v, *sc)
        got = OC.adam_emulate_f32(p.numpy(), g.numpy(), m.numpy(), v.numpy(), *sc)
        for k, r, e, x in zip('pmv', ref[:3], bound, got):
            assert bool(np.isfinite(x).all())
            err = (torch.from_numpy(x).double() - r).abs()
            assert bool((err[e == 0] == 0).all())
            ratio = float((err[e > 0] / e[e > 0]).max())
            worst[k] = max(worst[k], ratio)
    assert all(0.5 < r <= 1.0 for r in worst.values()), worst


def test_adam_operands_cover_the_zero_patterns():
    p, g, m, v = OC.adam_operands(4096, seed=3)
    assert bool(((g == 0) & (m == 0) & (v == 0)).any()) and bool(((g == 0) & (m != 0)).any()) and bool(((g != 0) & (v == 0)).any())
    assert bool((v >= 0).all()) and float(g.abs().max()) > 1e3 and float(g[g != 0].abs().min()) < 1e-10


def test_norm_emulation_stays_inside_norm_bound():
    """the fixed summation order restated in numpy (the GPU test asks the device for its bits): inside norm_bound of float64 at every
    size of the table, one-tensor and ragged, and exact where the sum is"""
    g = torch.Generator().manual_seed(2)
    datas = [torch.randn(n, generator=g) * 10.0 ** (i % 6 - 3) for i, n in enumerate(OC.SIZES)]
    for n, d in zip(OC.SIZES, datas):
        ref = OC.norm_ref([d])
        assert abs(float(OC.norm_emulate_f32([d])) - ref) <= OC.norm_bound(OC.blocks([n])) * ref, n
    for pre in (1.0, 1.0 / 3.0):
        ref = OC.norm_ref(datas, pre)
        assert abs(float(OC.norm_emulate_f32(datas, pre)) - ref) <= OC.norm_bound(OC.blocks(OC.SIZES), scaled=pre != 1.0) * ref
    assert float(OC.norm_emulate_f32([torch.tensor([3.0]), torch.zeros(0), torch.tensor([4.0, 0.0, 0.0, 0.0, 0.0])], 0.25)) == 1.25
    assert float(OC.norm_emulate_f32([torch.full((4 * 65536,), 0.5)])) == 256.0


def test_norm_sizes_mix_the_loop_rounds_and_the_probes_are_exact():
    """the norm's own sizes send EVERY thread of a block through an eight-piece round and then a two-piece round and / or a single
    piece (the edge table sends at most one thread through a mixed sequence); the order probes give 4096 exactly in the restated
    order, the tail's probe one ulp more"""
    def rounds(npc, t):              # (eight-piece, two-piece, single) rounds of thread t over npc pieces: the loop conditions of mt_body<0>
        i, r = t, [0, 0, 0]
        for width, k in ((8, 0), (2, 1), (1, 2)):
            while i + (width - 1) * OC.MT_THREADS < npc:
                r[k] += 1
                i += width * OC.MT_THREADS
        return tuple(r)
    want = {11267: (1, 1, 1), 43009: (1, 1, 0), 9218: (1, 0, 1), 3072: (0, 1, 1)}
    for (n, _), last in zip(OC.NORM_EXTRA_ROWS, (11267, 10241, 9218, 3072)):
        assert {rounds(last // 4, t) for t in range(OC.MT_THREADS)} == {want[n]}, n
    assert [n % 4 for n, _ in OC.NORM_EXTRA_ROWS] == [3, 1, 2, 0]
    assert all(len({rounds((n % OC.MT_CHUNK or OC.MT_CHUNK) // 4, t) for t in range(OC.MT_THREADS)}) <= 2 for n in OC.SIZES)
    for n in OC.NORM_SIZES:
        for lab, x in OC.order_probes(n):
            assert float(OC.norm_emulate_f32([x])) == (4096.0 + 2.0 ** -11 if lab.endswith('tail') else 4096.0), (n, lab)
    assert len(OC.order_probes(11267)) == 5 and OC.order_probes(3) == []


def test_norm_bound_and_clip_coef():
    assert OC.norm_bound(1) == 42.5 * OC.U and OC.norm_bound(64) == 42.5 * OC.U and OC.norm_bound(65) == 43 * OC.U
    assert OC.norm_bound(701, scaled=True) == (42 + 5.5 + 1) * OC.U
    assert OC.clip_coef(10.0, 5.0) == float(np.float32(5.0) / (np.float32(10.0) + np.float32(1e-6)))
    assert OC.clip_coef(1.0, 5.0) == 1.0 and OC.clip_coef(1.0, 5.0, 0.25) == 0.25 and OC.clip_coef(0.0, 5.0) == 1.0
    assert OC.clip_coef(float('inf'), 5.0) == 0.0 and OC.clip_coef(float('nan'), 5.0, 0.25) == 0.25      # NaN < 1 is false: no clip
    t = [torch.tensor([3.0]), torch.tensor([4.0, 0.0])]
    assert OC.norm_ref(t) == 5.0 and OC.norm_ref(t, 0.25) == 1.25
