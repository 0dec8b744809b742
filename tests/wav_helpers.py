"""Helpers the GPU tests of waveform I/O share (test_gpu_stream_wav_ragged, _resample, _out_rate, test_gpu_sample_format): test
signals, references, blocking feed loops, sentinel-checked vocoder runs, launch counts.  Where two tests need different behaviour under
one idea, both versions live here under their own names."""
import numpy as np
import torch

from conan_amd import synth
from tests.test_gpu_stream_wav import HOP, L, SEG, ctx  # noqa: F401  (ctx: module fixture, re-exported to the importing tests)

SENTINEL = 7.0      # float sentinel of _voc_run's buffers
SENT = 0xA5         # byte sentinel of _voc_run_bytes' buffers


def _sig(B, N, rate, seed):
    """Speech-band tones plus noise at `rate` Hz, [B, N] cuda float32."""
    rng = np.random.default_rng(seed)
    t = np.arange(N) / float(rate)
    w = [0.3 * np.sin(2 * np.pi * (150 + 70 * i) * t) + 0.1 * np.sin(2 * np.pi * 2300 * t) + 0.05 * rng.standard_normal(N) for i in range(B)]
    return torch.from_numpy(np.stack(w).astype(np.float32)).cuda()


def _ref(B, seed=3):
    return torch.from_numpy(synth.mel(40, seed, B)).cuda()


def _lin(rate):
    return L * rate // 16000


def _equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _mel(B, T, seed):
    return torch.from_numpy(np.stack([synth.mel(T, seed + i)[0] for i in range(B)])).cuda()


def _profiled(st, fn):
    st.profile_begin()
    out = fn()
    st.profile_end()
    return out, {k[0]: k[3] for k in st.profile_kernels()}


def _voc_run(st, slots, mel, sizes, ld=None):
    """conan_hifigan_step over `mel` in steps of sizes[k % len] frames into sentinel-filled buffers -> (rows per call, counts per call)."""
    n, T = mel.shape[0], mel.shape[1]
    pos, k, rows, counts = 0, 0, [], []
    while pos < T:
        f = min(sizes[k % len(sizes)], T - pos)
        buf = torch.full((n, ld or f * HOP), SENTINEL, device="cuda")
        st.hifigan_step(slots, mel[:, pos:pos + f], out=buf)
        cnt = st.output_samples()
        torch.cuda.synchronize()
        for i in range(n):
            assert bool((buf[i, cnt[i]:] == SENTINEL).all()), (pos, i, cnt)      # nothing past the count is touched
        rows.append([buf[i, :cnt[i]].clone() for i in range(n)])
        counts.append((f, cnt))
        pos, k = pos + f, k + 1
    return rows, counts


def _voc_run_bytes(st, slots, mel, sizes, ld=None):
    """conan_hifigan_step over `mel` in steps of sizes[k % len] frames into sentinel-filled byte buffers -> (rows per call in the
    slots' dtypes, (frames, counts) per call).  Every byte past a row's count must keep the sentinel."""
    n, T = mel.shape[0], mel.shape[1]
    pos, k, rows, counts = 0, 0, [], []
    while pos < T:
        f = min(sizes[k % len(sizes)], T - pos)
        raw = torch.full((n, (ld or f * HOP) * 4), SENT, dtype=torch.uint8, device="cuda")
        got = st.hifigan_step(slots, mel[:, pos:pos + f], out=raw.view(torch.float32))
        cnt = st.output_samples()
        torch.cuda.synchronize()
        if not isinstance(got, (list, tuple)):
            got = [got[i, :cnt[i]] for i in range(n)]
        for i in range(n):
            nb = cnt[i] * got[i].element_size()
            assert got[i].shape[0] == cnt[i] and bool((raw[i, nb:] == SENT).all()), (pos, i, cnt)
        rows.append([g.clone() for g in got])
        counts.append((f, cnt))
        pos, k = pos + f, k + 1
    return rows, counts


def _staggered_in_rates(U, seed):
    rng = np.random.default_rng(seed)
    pool = [8000, 11025, 22050, 24000, 32000, 44100, 48000, 96000]
    rates = [16000 if u % 4 == 0 else int(rng.choice(pool)) for u in range(U)]
    srcs = [_sig(1, int(rng.integers(r // 10, r // 2 + 2 * _lin(r))), r, 100 + u)[0] for u, r in enumerate(rates)]
    starts = sorted(int(v) for v in rng.integers(0, 12, U))
    return rates, srcs, starts


def _staggered_in_out_rates(U, seed):
    rng = np.random.default_rng(seed)
    pool = [8000, 11025, 22050, 24000, 32000, 44100, 48000]
    rates = [None if u % 4 == 0 else int(rng.choice(pool)) for u in range(U)]
    orates = [None if u % 3 == 1 else int(rng.choice(pool + [96000])) for u in range(U)]
    srcs = [_sig(1, int(rng.integers((r or 16000) // 10, (r or 16000) // 2 + 2 * _lin(r or 16000))), r or 16000, 100 + u)[0] for u, r in enumerate(rates)]
    starts = sorted(int(v) for v in rng.integers(0, 10, U))
    return rates, orates, srcs, starts


def _run_manual_at_rate(eng, src, rate, preset, hook=None):
    """Blocking feed loop of one utterance on eng.slots (the rate already set); hook(call_index) runs before each call."""
    Li = _lin(rate)
    N = src.shape[1]
    last = (N - 1) // Li * Li
    outs, pos, fin, i = [], 0, False, 0
    while True:
        if hook:
            hook(i)
        i += 1
        if pos < last:
            e, c, m, w = eng.st.step_wav(eng.slots, src[:, pos:pos + Li])
            pos += Li
        else:
            e, c, m, w = eng.st.step_wav(eng.slots, src[:, pos:] if not fin else src[:, :0], final=True)
            pos, done, fin = N, fin and e == 0, True
            if done:
                break
        if e:
            outs.append((w.clone(), m.clone(), c[:, :e].clone()))
    torch.cuda.synchronize()
    return [torch.cat(t, 1) for t in zip(*outs)]


def _run_manual(eng, src, Li, hook=None):
    """Blocking step_wav loop of one utterance on eng.slots (rates and formats already set); hook(call index) runs before each call."""
    N = src.shape[1]
    last = (N - 1) // Li * Li
    outs, pos, fin, i = [], 0, False, 0
    while True:
        if hook:
            hook(i)
        i += 1
        if pos < last:
            e, c, m, w = eng.st.step_wav(eng.slots, src[:, pos:pos + Li])
            pos += Li
        else:
            e, c, m, w = eng.st.step_wav(eng.slots, src[:, pos:] if not fin else src[:, :0], final=True)
            pos, done, fin = N, fin and e == 0, True
            if done:
                break
        if e:
            w = torch.stack(list(w)) if isinstance(w, (list, tuple)) else w
            outs.append((w.clone(), m.clone(), c[:, :e].clone()))
    torch.cuda.synchronize()
    return [torch.cat(t, 1) for t in zip(*outs)]
