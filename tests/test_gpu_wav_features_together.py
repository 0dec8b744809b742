"""The per-slot source features of the wav-in step together in one stream-set (input level, pitch follow, pitch register, activity,
bypass): what a call interleaves - rows with and without each feature in the same emit group, two emit groups in one ragged call,
restarts travelling in a mixed call, a refused call between valid ones.  Every assertion is an equality between two runs of the same
code, bit for bit: pipelined against blocking, each slot against the same utterance alone, a run with a refused call against the run
without it.  A fixed-plan stream-set: a row's arithmetic does not depend on the rows it shares a launch with.

  slot 0   input level, pitch follow and register, activity mode 2, bypass with fill_gate and a half-and-half mix
  slot 1   activity mode 1 only; its first utterance ends early, the slot is reset (front-end included) and takes a second one
  slot 2   bypass only, no fill_gate
  slot 3   no setter ever called

  tick      0    1    2    3    4    5    6    7    8        (one ragged call per tick over the live slots; the frames a row emits)
  slot 0                   0    4    4    4    2    0
  slot 1    0    4    3    0 |  0    4    3    0             (| the reset)
  slot 2                   0    4    4    3    0
  slot 3                   0    4    4    4    1    0
"""
import pytest
import torch

from conan_amd import _lib
from tests.test_gpu_bypass import KW, _bursts, _noise
from tests.test_gpu_f0 import _ref
from tests.test_gpu_pitch import full  # noqa: F401  (module fixture: the small synthetic full model)

pytestmark = pytest.mark.gpu

HOP, SEG = 320, 4
L = SEG * HOP
SLOTS = [0, 1, 2, 3]
REFUSED_TICK = 5      # every slot is live and emits a full chunk; slot 1's chunk carries the restart of its reset


def _utterances():
    b = _bursts(3, 17)
    return [dict(slot=0, start=3, wav=b[0, :3 * L + 500]),                    # 4 chunks, the last of 2 frames
            dict(slot=1, start=0, wav=b[1, :L + 700]),                        # 2 chunks, the last of 3 frames
            dict(slot=1, start=4, wav=b[2, :L + 700], reuse=True),            # ... and the slot's second utterance
            dict(slot=2, start=3, wav=_noise(1, 2 * L + 650, 71)[0]),         # 3 chunks, the last of 3 frames
            dict(slot=3, start=3, wav=_noise(1, 3 * L + 100, 72)[0])]         # 4 chunks, the last of 1 frame


def _settings(st, slot):
    if slot == 0:
        st.set_input_level([0], target=-26.0)
        st.set_pitch_follow([0], True)
        st.set_pitch_register([0], target=7.5)
        st.set_activity([0], **KW)
        st.set_bypass([0], wet=0.5, dry=0.5, fill_gate=True)
    elif slot == 1:
        st.set_activity([1], gate=False, **KW)
    elif slot == 2:
        st.set_bypass([2], wet=0.25, dry=0.75)


def _open(full, slots, refs):
    st = full.streams(len(SLOTS), 4, 64, flags=_lib.STREAMS_FIXED_PLAN)
    st.reset(slots, which=15)
    st.set_reference(slots, refs[slots])
    for slot in slots:
        _settings(st, slot)
    return st


def _drive(st, utts, refs, pipelined=False, hooks=None, refuse_at=None):
    """One step_wav_ragged call per tick over the live utterances -> (per utterance (codes, mel, wav) over its emitted frames, per
    call dict(tick, slots, emit[, the hooks and state queries behind the call])).  hooks: the slots whose features' hooks and states
    are read behind every call (they join pipelined work).  refuse_at: that tick's call is first made with a mel configuration a
    following slot refuses."""
    U = len(utts)
    pos, fin, done, begun = [0] * U, [False] * U, [False] * U, [False] * U
    outs, calls = [[] for _ in range(U)], []
    step = st.step_wav_ragged_async if pipelined else st.step_wav_ragged
    tick = -1
    while not all(done):
        tick += 1
        live = [u for u in range(U) if utts[u]["start"] <= tick and not done[u]]
        if not live:
            continue
        slots = [utts[u]["slot"] for u in live]
        assert len(set(slots)) == len(slots), (tick, slots)      # a slot's earlier utterance has drained
        for u in live:
            if not begun[u] and utts[u].get("reuse"):
                st.reset([utts[u]["slot"]], which=15)            # (CONAN_MODEL_FRONTEND included: the features' restarts)
                st.set_reference([utts[u]["slot"]], refs[[utts[u]["slot"]]])
            begun[u] = True
        rows = torch.zeros(len(live), L, device="cuda")
        samples, final = [], []
        for r, u in enumerate(live):
            x = utts[u]["wav"]
            N = x.shape[0]
            last = (N - 1) // L * L
            k = L if pos[u] < last else N - pos[u]
            rows[r, :k] = x[pos[u]:pos[u] + k]
            samples.append(k); final.append(pos[u] >= last); pos[u] += k
        if refuse_at == tick:
            assert 0 in slots
            with pytest.raises(_lib.ConanError) as e:
                st.step_wav_ragged(slots, rows, samples, final, mel=dict(sample_rate=22050))
            assert e.value.code == _lib.ERR_INVALID and "follows the source pitch" in str(e.value)
        was_final = [fin[u] for u in live]
        emit, c, m, w = step(slots, rows, samples, final)
        call = dict(tick=tick, slots=slots, emit=list(emit))
        if hooks is not None:
            st.join()
            call["out"] = [(c[r, :e], m[r, :e], w[r, :e * HOP]) for r, e in enumerate(emit)]
            call["contour"], call["activity"], call["bypass"] = st.step_wav_contour(), st.step_wav_activity(), st.step_wav_bypass()
            if 0 in hooks:
                call["input_level"] = st.input_level([0])
                call["register"] = st.pitch_register([0])
            call["activity_state"] = st.activity_state([s for s in (0, 1) if s in hooks])
            call["bypass_state"] = st.bypass_state([s for s in (0, 2) if s in hooks])
        calls.append(call)
        for r, u in enumerate(live):
            e = emit[r]
            fin[u] = fin[u] or final[r]
            done[u] = was_final[r] and e == 0
            if e:
                outs[u].append((c[r, :e], m[r, :e], w[r, :e * HOP]))
    st.join()
    torch.cuda.synchronize()
    return [[torch.cat([o[i] for o in out]).clone() for i in range(3)] for out in outs], calls


def _bits(x):
    return x.view({4: torch.int32, 8: torch.int64}[x.element_size()]) if x.is_floating_point() else x


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return a.shape == b.shape and torch.equal(_bits(a), _bits(b))
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    return a == b


def _restart(st, refs):
    st.reset(SLOTS, which=15)
    st.set_reference(SLOTS, refs)


def test_features_together(full):
    utts, refs = _utterances(), _ref(len(SLOTS))
    st = _open(full, SLOTS, refs)
    # ---- the run, blocking, with every hook and state query behind every call
    blk, calls = _drive(st, utts, refs, hooks=SLOTS)
    emits = {c["tick"]: dict(zip(c["slots"], c["emit"])) for c in calls}
    assert emits[6] == {0: SEG, 3: SEG, 1: 3, 2: 3}      # two emit groups, each with rows with and without every feature
    assert emits[REFUSED_TICK] == {0: SEG, 1: SEG, 2: SEG, 3: SEG} and emits[4][1] == 0      # slot 1's first chunk after its reset
    assert emits[7] == {0: 2, 1: 0, 2: 0, 3: 1} and [len(o[0]) for o in blk] == [14, 7, 7, 11, 13]
    two = next(c for c in calls if c["tick"] == 6)      # (call row = slot there) the hooks read zeros where a row has no such feature
    (f0, uv), (_, lvl), (wet, dry) = two["contour"], two["activity"], two["bypass"]
    assert bool((f0[0] != 0).any() or (uv[0] != 0).any()) and bool(wet[0].any()) and bool(dry[2, :3].any()) and not wet[2, 3:].any()
    assert not f0[1:].any() and not uv[1:].any() and not lvl[2:].any() and not wet[[1, 3]].any() and not dry[[1, 3]].any()
    assert all(s["frames"] > 0 for s in two["activity_state"])
    # ---- pipelined against blocking: behind every call, then free running
    _restart(st, refs)
    pip, pcalls = _drive(st, utts, refs, pipelined=True, hooks=SLOTS)
    assert len(pcalls) == len(calls)
    for a, b in zip(pcalls, calls):
        for k in b:
            assert _same(a[k], b[k]), (b["tick"], k)
    assert _same(pip, blk)
    _restart(st, refs)
    free, fcalls = _drive(st, utts, refs, pipelined=True)
    assert [c["emit"] for c in fcalls] == [c["emit"] for c in calls] and _same(free, blk)
    # ---- errors change nothing: a refused call in mid-run, then the bits of the run without it
    _restart(st, refs)
    again, rcalls = _drive(st, utts, refs, hooks=SLOTS, refuse_at=REFUSED_TICK)
    for a, b in zip(rcalls, calls):
        for k in b:
            assert _same(a[k], b[k]), (b["tick"], k)
    assert _same(again, blk)
    st.close()
    # ---- each slot against itself alone, in a stream-set with that slot's settings only (slot 3: no setter ever called)
    for slot in SLOTS:
        solo = _open(full, [slot], refs)
        mine = [u for u in range(len(utts)) if utts[u]["slot"] == slot]
        got, _ = _drive(solo, [utts[u] for u in mine], refs)
        for u, g in zip(mine, got):
            assert _same(g, blk[u]), (slot, u)
        solo.close()
