"""Slot snapshots on the GPU (conan_streams_export_slots / _import_slots): a stream that is exported, carried through the host and a
pickle, and imported into a dirtied slot of another stream-set continues bit for bit as if it had never moved - across the ring sets
of build_vocoder (stream-sets of 2, 4 and 16 slots), both arithmetics, fixed and default plans, the waveform path with rates and
formats, the Emformer memory bank, another max_frames, the pipelined step and a second device.  Every comparison is torch.equal."""
import pickle

import numpy as np
import pytest
import torch

from conan_amd import _lib, configs, synth
from conan_amd.engine import StreamingVoiceConversionEngine
from conan_amd.runtime import Context
from tests.conftest import ARITHS

pytestmark = pytest.mark.gpu

SEG, RC, HOP = 4, 2, 320
NCHUNK = 18
FIXED = _lib.STREAMS_FIXED_PLAN


def _make_ctx(device=0, chp=None, **models):
    chp, vhp = chp or configs.conan_hparams(), configs.hifigan_hparams()
    c = Context(chp, vhp, device, **models)
    c.load_state_dict("emformer", synth.emformer_state_dict(chp, 0))
    if models.get("conan", True):
        c.load_state_dict("conan", synth.conan_state_dict(chp, 0))
    if models.get("hifigan", True):
        c.load_state_dict("hifigan", synth.hifigan_state_dict(vhp, 0))
    c.finalize()
    return c


@pytest.fixture(scope="module")
def ctx():
    c = _make_ctx()
    assert c.hop == HOP and c.cfg.emf_segment == SEG and c.cfg.emf_right_context == RC
    yield c
    c.close()


def _chunks(seed, n=NCHUNK):
    """The chunks [1, seg + rc, 80] of a synthetic utterance of n * seg (+ rc) frames."""
    mel = torch.from_numpy(synth.mel(n * SEG + RC, seed)).cuda()
    return [mel[:, j * SEG:j * SEG + SEG + RC].contiguous() for j in range(n)]


def _ref(seed, frames=40):
    return torch.from_numpy(synth.mel(frames, seed)).cuda()


def _start(st, slots, ref):
    st.reset(slots)
    st.set_reference(slots, ref.expand(len(slots), -1, -1).contiguous() if ref.shape[0] == 1 else ref)


def _steps(st, slots, chunks):
    """Blocking chunk steps of `slots` (each fed the same chunk) -> [(codes, mel, wav)] per chunk, cloned."""
    out = []
    for ch in chunks:
        c, m, w = st.step(slots, ch.expand(len(slots), -1, -1).contiguous())
        out.append((c.clone(), m.clone(), w.clone()))
    return out


def _same(got, want, row=0, wrow=0):
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        for k, name in enumerate(("codes", "mel", "wav")):
            assert torch.equal(g[k][row], w[k][wrow]), (j, name)


def _carry(snap, device="cuda"):
    """export -> host -> pickle round trip -> device"""
    return pickle.loads(pickle.dumps(snap.cpu())).to(device)


_REFS = {}


def _reference_run(ctx, size, arith, flags, src_seed=11, ref_seed=21, max_frames=SEG, change=None):
    """One stream alone in slot 0 of a stream-set of these arguments, NCHUNK chunks (computed once per argument set; never modified).
    change = (chunk, reference seed): set_reference again before that chunk."""
    key = (size, arith, flags, src_seed, ref_seed, max_frames, change)
    if key not in _REFS:
        st = ctx.streams(size, max_frames=max_frames, max_ref_frames=64, arith=arith, flags=flags)
        _start(st, [0], _ref(ref_seed))
        ch = _chunks(src_seed)
        if change is None:
            _REFS[key] = _steps(st, [0], ch)
        else:
            out = _steps(st, [0], ch[:change[0]])
            st.set_reference([0], _ref(change[1]))
            _REFS[key] = out + _steps(st, [0], ch[change[0]:])
        st.close()
    return _REFS[key]


def _dirty(st, slot):
    """Three chunks of another utterance with another reference in `slot`."""
    _start(st, [slot], _ref(77, 52))
    _steps(st, [slot], _chunks(99, 3))


# ------------------------------------------------------------------------------------------------------------------ 1. migration, mel in

@pytest.mark.parametrize("flags", [FIXED, 0], ids=["fixed", "default"])
@pytest.mark.parametrize("size", [2, 4, 16])
@pytest.mark.parametrize("arith", ARITHS)
def test_migration_continues_bitwise(ctx, arith, size, flags):
    want = _reference_run(ctx, size, arith, flags)
    ch = _chunks(11)
    A = ctx.streams(size, max_frames=SEG, max_ref_frames=64, arith=arith, flags=flags)
    B = ctx.streams(size, max_frames=SEG, max_ref_frames=64, arith=arith, flags=flags)
    assert A.layout_id == B.layout_id and A.snapshot_bytes == B.snapshot_bytes
    dst = min(2, size - 1)
    # cuts: 1 - the history still holds start-of-utterance zeros; 4; 14 - Emformer left context saturated, every vocoder ring wrapped
    for cut in (1, 4, 14):
        _start(A, [0], _ref(21))
        head = _steps(A, [0], ch[:cut])
        _same(head, want[:cut])
        _dirty(B, dst)
        B.import_slots([dst], _carry(A.export_slots([0])))
        _same(_steps(B, [dst], ch[cut:]), want[cut:])
    A.close(); B.close()


# ------------------------------------------------------------------------------------------------------------------ 2. source and neighbours

@pytest.mark.parametrize("arith", ARITHS)
def test_source_and_neighbours_untouched(ctx, arith):
    size, cut = 4, 6
    want = _reference_run(ctx, size, arith, FIXED)
    solo = [_reference_run(ctx, size, arith, FIXED, src_seed=31 + k, ref_seed=41 + k) for k in range(2)]
    ch = _chunks(11)
    nb = [_chunks(31), _chunks(32)]
    A = ctx.streams(size, max_frames=SEG, max_ref_frames=64, arith=arith, flags=FIXED)
    B = ctx.streams(size, max_frames=SEG, max_ref_frames=64, arith=arith, flags=FIXED)
    _start(A, [0], _ref(21))
    _steps(A, [0], ch[:cut])
    _dirty(B, 2)
    _start(B, [0, 1], torch.cat([_ref(41), _ref(42)]))
    got = [[], []]
    for j in range(NCHUNK):
        if j == cut:
            B.import_slots([2], _carry(A.export_slots([0])))
            moved = []
        slots = [0, 1] if j < cut else [0, 1, 2]
        chunk = torch.cat([nb[0][j], nb[1][j]] + ([ch[j]] if j >= cut else []))
        c, m, w = B.step(slots, chunk)
        for k in range(2):
            got[k].append((c[k:k + 1].clone(), m[k:k + 1].clone(), w[k:k + 1].clone()))
        if j >= cut:
            moved.append((c[2:3].clone(), m[2:3].clone(), w[2:3].clone()))
    _same(got[0], solo[0]); _same(got[1], solo[1])
    _same(moved, want[cut:])
    _same(_steps(A, [0], ch[cut:]), want[cut:])      # the source goes on after the export
    A.close(); B.close()


# ------------------------------------------------------------------------------------------------------------------ 3. fork

@pytest.mark.parametrize("arith", ARITHS)
def test_fork(ctx, arith):
    size, cut, change = 4, 5, 9
    want = _reference_run(ctx, size, arith, FIXED)
    want2 = _reference_run(ctx, size, arith, FIXED, change=(change, 55))
    ch = _chunks(11)
    st = ctx.streams(size, max_frames=SEG, max_ref_frames=64, arith=arith, flags=FIXED)
    _dirty(st, 3)
    _start(st, [0], _ref(21))
    _steps(st, [0], ch[:cut])
    st.import_slots([1, 3], _carry(st.export_slots([0])).select([0, 0]))
    got = _steps(st, [0, 1, 3], ch[cut:change])
    for row in range(3):
        _same(got, want[cut:change], row=row)
    st.set_reference([3], _ref(55))
    got = _steps(st, [0, 1, 3], ch[change:])
    _same(got, want[change:], row=0); _same(got, want[change:], row=1)
    _same(got, want2[change:], row=2)
    st.close()


# ------------------------------------------------------------------------------------------------------------------ 4. waveform path

def _wav16(N, rate, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(N) / float(rate)
    return (0.3 * np.sin(2 * np.pi * 190 * t) + 0.1 * np.sin(2 * np.pi * 2300 * t) + 0.03 * rng.standard_normal(N)).astype(np.float32)


def _wav_run(ctx, migrate_after=None):
    """Two staggered-path streams - slot 0 at 48 kHz s16 in, 8 kHz mu-law out; slot 1 at the model rate in f32 - fed to the end, drained
    and flushed.  migrate_after = k: after the k-th call both streams move to a fresh engine.  -> (per call rows, flush rows, infos, grow)"""
    x0 = torch.from_numpy(np.round(_wav16(9 * 3840 + 1700, 48000, 5) * 32767).astype(np.int16)).cuda()
    x1 = torch.from_numpy(_wav16(9 * 1280 + 500, 16000, 6)).cuda()
    xs, Ls = [x0, x1], [3840, 1280]
    eng = StreamingVoiceConversionEngine(ctx, 2, max_ref_frames=64)
    eng.open_slots([0, 1], torch.cat([_ref(21), _ref(22)]), in_rate=[48000, None], out_rate=[8000, None], in_format=["s16", None],
                   out_format=["ulaw", None])
    live, pos, fin = [0, 1], [0, 0], [False, False]
    calls, flushed, infos, grow, ncall = [], {}, None, None, 0
    while live:
        rows, samples, final = [], [], []
        for s in live:
            N, L = xs[s].shape[0], Ls[s]
            last = (N - 1) // L * L
            if pos[s] < last:
                piece, pos[s] = xs[s][pos[s]:pos[s] + L], pos[s] + L
                final.append(0)
            else:
                piece, pos[s] = (xs[s][pos[s]:] if not fin[s] else xs[s][:0]), N
                final.append(1)
            rows.append(piece); samples.append(piece.shape[0])
        was_final = [fin[s] for s in live]
        for s, f in zip(live, final):
            fin[s] = fin[s] or bool(f)
        res = eng.feed_ragged(live, rows, samples, final)
        counts = eng.st.output_samples()
        calls.append([(s, int(counts[i]), w.clone(), m.clone(), c.clone()) for i, (s, (w, m, c)) in enumerate(zip(live, res))])
        for s, wf, (w, m, c) in zip(list(live), was_final, res):
            if wf and m.shape[0] == 0:
                flushed[s] = eng.finish([s])[0].clone()
                live.remove(s)
        ncall += 1
        if migrate_after == ncall:
            snap = _carry(eng.export_streams([0, 1]))
            infos = [snap.info(0), snap.info(1)]
            fresh = StreamingVoiceConversionEngine(ctx, 2, max_ref_frames=64)      # its stream-set never had a rate or a format
            before = fresh.st.state_bytes
            fresh.import_streams([0, 1], snap)
            grow = fresh.st.state_bytes - before
            eng.st.close()
            eng = fresh
    eng.st.close()
    return calls, flushed, infos, grow


def test_waveform_path_with_rates_and_formats(ctx):
    want_calls, want_flush, _, _ = _wav_run(ctx)
    calls, flush, infos, grow = _wav_run(ctx, migrate_after=3)
    assert len(calls) == len(want_calls) and len(calls) > 10
    for got, want in zip(calls, want_calls):
        assert [(g[0], g[1]) for g in got] == [(w[0], w[1]) for w in want]
        for g, w in zip(got, want):
            assert g[2].dtype == w[2].dtype and all(torch.equal(a, b) for a, b in zip(g[2:], w[2:]))
    assert sorted(flush) == sorted(want_flush) == [0, 1]
    for s in (0, 1):
        assert flush[s].dtype == want_flush[s].dtype and torch.equal(flush[s], want_flush[s])
    assert flush[0].dtype == torch.uint8 and flush[0].numel() > 0
    # what the two setters document: 32768 floats per slot for the input ring, next_pow2(8192 + 8 + max_frames * hop) for the output ring
    out_ring = 1 << int(np.ceil(np.log2(_lib.RESAMPLE_MAX_TAPS + 8 + SEG * HOP)))
    assert grow == 2 * 4 * (32768 + out_ring)
    assert (infos[0]["in_rate"], infos[0]["out_rate"], infos[0]["in_format"], infos[0]["out_format"]) == (48000, 8000, "s16", "ulaw")
    assert (infos[1]["in_rate"], infos[1]["out_rate"], infos[1]["in_format"], infos[1]["out_format"]) == (None, None, "f32", "f32")
    assert infos[0]["has_ref"] and infos[1]["bytes"] < infos[0]["bytes"]


# ------------------------------------------------------------------------------------------------------------------ 5. Emformer memory bank

def test_emformer_memory_bank():
    M, cut, n = 4, 11, 16      # the bank (8 rows per layer) has wrapped by chunk 9
    chp = dict(configs.conan_hparams(), emformer_max_memory_size=M)
    c = _make_ctx(chp=chp, conan=False, hifigan=False)
    assert c.cfg.emf_max_memory_size == M
    ch = _chunks(13, n)
    A, B = c.streams(4, max_frames=SEG, max_ref_frames=16), c.streams(4, max_frames=SEG, max_ref_frames=16)
    A.reset([0])
    want = [tuple(t.clone() for t in A.emformer_step([0], x)) for x in ch]
    A.reset([1])
    for x in ch[:cut]:
        A.emformer_step([1], x)
    B.reset([3])
    for x in _chunks(14, 3):
        B.emformer_step([3], x)
    B.import_slots([3], _carry(A.export_slots([1])))
    for j in range(cut, n):
        got = B.emformer_step([3], ch[j])
        for g, w in zip(got, want[j]):
            assert torch.equal(g, w), j
    A.close(); B.close(); c.close()


# ------------------------------------------------------------------------------------------------------------------ 6. max_frames

@pytest.mark.parametrize("arith", ARITHS)
def test_max_frames_independence(ctx, arith):
    size, cut = 4, 7
    A = ctx.streams(size, max_frames=4, max_ref_frames=64, arith=arith, flags=FIXED)
    B = ctx.streams(size, max_frames=8, max_ref_frames=64, arith=arith, flags=FIXED)
    assert A.snapshot_bytes == B.snapshot_bytes and A.layout_id == B.layout_id
    assert A.state_bytes < B.state_bytes      # (longer rings, the same history)
    want = _reference_run(ctx, size, arith, FIXED, max_frames=8)
    ch = _chunks(11)
    _start(A, [0], _ref(21))
    _steps(A, [0], ch[:cut])
    _dirty(B, 2)
    B.import_slots([2], _carry(A.export_slots([0])))
    _same(_steps(B, [2], ch[cut:]), want[cut:])
    A.close(); B.close()


# ------------------------------------------------------------------------------------------------------------------ 7. bounds, determinism

def test_bounds_and_determinism(ctx):
    st = ctx.streams(4, max_frames=SEG, max_ref_frames=64)
    _start(st, [1], _ref(21))
    _steps(st, [1], _chunks(11, 5))
    nbytes = st.snapshot_bytes
    assert nbytes % 256 == 0
    bufs = [torch.full((1, nbytes + 4096), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2)]
    snaps = [st.export_slots([1], out=b) for b in bufs]
    used = snaps[0].info(0)["bytes"]
    assert 0 < used <= nbytes
    assert bool((bufs[0][0, used:] == 0xA5).all()) and bool((bufs[1][0, used:] == 0xA5).all())
    assert torch.equal(bufs[0], bufs[1]) and snaps[0].meta == snaps[1].meta
    assert snaps[0].info(0)["layout_id"] == st.layout_id
    assert nbytes * st.max_slots < st.state_bytes      # the history is smaller than the rings
    print("snapshot bytes per slot", nbytes, "used", used, "state bytes per slot", st.state_bytes // st.max_slots)
    st.close()


# ------------------------------------------------------------------------------------------------------------------ 8. errors

def test_errors_leave_everything_unchanged(ctx):
    size, cut = 4, 5
    arith = "limb"
    other = "f32"
    want = _reference_run(ctx, size, arith, FIXED)
    ch = _chunks(11)
    st = ctx.streams(size, max_frames=SEG, max_ref_frames=64, arith=arith, flags=FIXED)
    _start(st, [0, 1], _ref(21))
    _steps(st, [0, 1], ch[:cut])
    good = st.export_slots([0])
    foreign = []
    for kw in (dict(arith=other, max_ref_frames=64), dict(arith=arith, max_ref_frames=128)):
        o = ctx.streams(size, max_frames=SEG, flags=FIXED, **kw)
        _start(o, [0], _ref(33))
        _steps(o, [0], _chunks(34, 2))
        foreign.append((o.layout_id, o.export_slots([0])))
        o.close()

    def refused(slots, snap, *needles, ld=None):
        with pytest.raises(_lib.ConanError) as e:
            if ld is None:
                st.import_slots(slots, snap)
            else:
                a = np.asarray(slots, dtype=np.int32)
                meta = (_lib.SlotMeta * len(a)).from_buffer_copy(snap.meta)
                _lib.check(st.lib.conan_streams_import_slots(st.h, a.ctypes.data, len(a), snap.blob.data_ptr(), ld, meta, None))
        assert e.value.code == _lib.ERR_INVALID
        for n in needles:
            assert n in str(e.value), (n, str(e.value))

    for fid, snap in foreign:
        assert fid != st.layout_id
        refused([1], snap, "%016x" % fid, "%016x" % st.layout_id)
    used = good.info(0)["bytes"]
    refused([1], good, "blob_ld_bytes", ld=used - 16)                       # a truncated row
    refused([1, 1], good.select([0, 0]), "duplicate slot")
    refused([1, size], good.select([0, 0]), "out of range")
    meta = bytearray(good.meta); meta[40] ^= 0x10
    refused([1], type(good)(bytes(meta), good.blob), "corrupted")
    # a call with one good and one bad record changes neither slot
    mixed = type(good)(good.meta + bytes(meta), torch.cat([good.blob, good.blob]))
    refused([2, 1], mixed, "record 1")
    got = _steps(st, [0, 1], ch[cut:])
    _same(got, want[cut:], row=0); _same(got, want[cut:], row=1)
    st.close()


# ------------------------------------------------------------------------------------------------------------------ 9. pipelined

@pytest.mark.parametrize("arith", ARITHS)
def test_pipelined_export_import(ctx, arith):
    size, cut = 4, 6
    want = _reference_run(ctx, size, arith, FIXED)
    ch = _chunks(11)
    A = ctx.streams(size, max_frames=SEG, max_ref_frames=64, arith=arith, flags=FIXED)
    B = ctx.streams(size, max_frames=SEG, max_ref_frames=64, arith=arith, flags=FIXED)

    def run_async(st, slot, chunks):
        outs = []
        for x in chunks:
            w = torch.empty(1, SEG * HOP, device="cuda")
            c = torch.empty(1, SEG, dtype=torch.int32, device="cuda")
            m = torch.empty(1, SEG, 80, device="cuda")
            st.step_async([slot], x, w, codes=c, mel_out=m)
            outs.append((c, m, w))
        return outs

    _start(A, [0], _ref(21))
    head = run_async(A, 0, ch[:cut])
    snap = A.export_slots([0])                   # right behind step_async: the export joins the pipeline itself
    _dirty(B, 2)
    B.import_slots([2], snap)
    tail = run_async(B, 2, ch[cut:])
    B.join(); A.join()
    torch.cuda.synchronize()
    _same(head + tail, want)
    A.close(); B.close()


# ------------------------------------------------------------------------------------------------------------------ 10. two GPUs

@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_two_gpus(ctx):
    size, cut = 4, 6
    want = _reference_run(ctx, size, "auto", FIXED)
    ch = _chunks(11)
    A = ctx.streams(size, max_frames=SEG, max_ref_frames=64, flags=FIXED)
    _start(A, [0], _ref(21))
    _steps(A, [0], ch[:cut])
    snap = A.export_slots([0]).to("cuda:1")
    c1 = _make_ctx(device=1)
    with torch.cuda.device(1):
        B = c1.streams(size, max_frames=SEG, max_ref_frames=64, flags=FIXED)
        assert B.layout_id == A.layout_id
        B.import_slots([2], snap)
        got = _steps(B, [2], [x.to("cuda:1") for x in ch[cut:]])
        got = [tuple(t.to("cuda:0") for t in g) for g in got]
        B.close()
    _same(got, want[cut:])
    A.close(); c1.close()
