"""Builds libsemitts_hip.so (gfx950 only) in-tree with hipcc.  `python -m semi_tts_amd.build`"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
LIBDIR = os.path.join(HERE, 'lib')
LIB = os.path.join(LIBDIR, 'libsemitts_hip.so')
SOURCES = ['skinny.hip', 'skinny_packed.hip', 'attention.hip', 'gemm.hip', 'rnn.hip', 'vq.hip', 'runtime.hip', 'decoder.hip', 'grad.hip', 'attention_bwd.hip', 'decoder_bwd.hip', 'loss.hip', 'optim.hip', 'norm.hip', 'audio.hip', 'ctc_decode.hip', 'ctc_align.hip', 'resample.hip', 'dtw.hip',
           'attn_stats.hip']
# the pitch kernels (st_f0_yin, st_f0_path_scores), listed apart: tests/test_synth_host.py pins the twenty entries above
PITCH_SOURCES = ['f0.hip']
# the silence-trimming kernels (st_trim_silence), listed apart for the same reason
TRIM_SOURCES = ['trim.hip']
# the transcript-scoring kernel (st_edit_align), listed apart for the same reason
SCORE_SOURCES = ['edit_align.hip']
# the loudness kernels (st_loudness_batch, st_wave_gain), listed apart for the same reason
LOUDNESS_SOURCES = ['loudness.hip']
# the ABX kernels (st_dtw_pairs, st_abx_count, st_abx_across), listed apart for the same reason
ABX_SOURCES = ['abx.hip']
# the intelligibility kernels (st_stoi_batch), listed apart for the same reason
STOI_SOURCES = ['stoi.hip']
# the alignment kernels (st_xcorr_delay, st_sisdr_batch, st_wave_gather), listed apart for the same reason
ALIGN_SOURCES = ['xcorr.hip']
# the BatchNorm kernels (st_bn_*, st_bn_bank_*), taken out of gemm.hip and grad.hip, listed apart for the same reason
BATCHNORM_SOURCES = ['batchnorm.hip']
# the k-means kernels (st_kmeans_assign, st_kmeans_update, st_kmeans_relocate, st_kmeans_pp_*), listed apart for the same reason
KMEANS_SOURCES = ['kmeans.hip']


def _hipcc():
    for c in (os.environ.get('HIPCC'), '/opt/rocm/bin/hipcc', 'hipcc'):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    return 'hipcc'


def needs_build():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [os.path.join(os.path.dirname(HERE), 'include', 'semitts.h')]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=True):
    """hipcc --offload-arch=gfx950 -> semi_tts_amd/lib/libsemitts_hip.so (cross-compiles without a GPU)."""
    if not force and not needs_build():
        return LIB
    os.makedirs(LIBDIR, exist_ok=True)
    objs = []
    procs = []
    for src in SOURCES + PITCH_SOURCES + TRIM_SOURCES + SCORE_SOURCES + LOUDNESS_SOURCES + ABX_SOURCES + STOI_SOURCES + ALIGN_SOURCES + BATCHNORM_SOURCES + KMEANS_SOURCES:
        obj = os.path.join(LIBDIR, src.replace('.hip', '.o'))
        cmd = [_hipcc(), '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-mllvm', '-amdgpu-kernarg-preload-count=16', '-c', os.path.join(CSRC, src), '-o', obj]
        procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
        objs.append(obj)
    for src, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError('hipcc failed on %s:\n%s' % (src, out))
        if verbose and out.strip():
            print(out)
    cmd = [_hipcc(), '--offload-arch=gfx950', '-shared', '-fPIC', '-o', LIB] + objs
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError('link failed:\n' + r.stdout)
    if verbose:
        print('built', LIB)
    return LIB


if __name__ == '__main__':
    build(force='--force' in sys.argv)
