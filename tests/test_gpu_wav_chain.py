"""The wav-in step with every per-slot feature on in one stream-set ("The chain as a whole"): the slot table, the utterances
and the tick schedule of tests/wav_chain_cases.py.  What a call shares between features - the source staging set that goes to the
resampler, the equaliser or the leveller according to the other rows of the call, the nine output stages on the caller's rows or on
the output staging, every stage's staging sets under pipelining, every plan() in front of a refusal - is held to runs of the same
slot alone, to the blocking run and to the run without the refusals.  Every comparison is bit for bit (raw bytes for coded rows);
nothing here has a tolerance.

The walks are over _lib.SLOT_FEATURES: a feature added to the table is read here (its hook behind every call, its states at the
end) as soon as tests/wav_chain_cases.py enables it, and tests/test_wav_chain_cpu.py fails until it does."""
import numpy as np
import pytest
import torch

from conan_amd import _lib
from tests import wav_chain_cases as W
from tests.test_gpu_f0 import _ref
from tests.test_gpu_pitch import full  # noqa: F401  (module fixture: the small synthetic full model)

pytestmark = pytest.mark.gpu

HOP, SEG, L = W.HOP, W.SEG, W.L
FULL = 1 << 20
QUIET = {"ulaw": 0xFF, "alaw": 0xD5}      # a format's silence: a far end that leaves the row's bytes alone
# the hooks of the last call, per keyword of _lib.SLOT_FEATURES with a `last` symbol
HOOKS = dict(follow=lambda st: st.step_wav_contour(), activity=lambda st: st.step_wav_activity(), bypass=lambda st: st.step_wav_bypass(),
             comfort=lambda st: (st.step_wav_comfort(),), tones=lambda st: st.step_wav_tones())
REFUSED_TICK = 4      # every slot is live; two emit groups; slot 5 delivers a full chunk at 24 kHz


def _bits(x):
    return x.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[x.element_size()]) if x.is_floating_point() else x


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    return a == b


def _diff(a, b, path=""):
    """The first place two records differ (for the assertion's message)."""
    if isinstance(a, dict) and isinstance(b, dict) and a.keys() == b.keys():
        for k in a:
            if not _same(a[k], b[k]):
                return _diff(a[k], b[k], f"{path}/{k}")
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)) and len(a) == len(b):
        for i, (x, y) in enumerate(zip(a, b)):
            if not _same(x, y):
                return _diff(x, y, f"{path}[{i}]")
    return path


def _conceal_cfg(slot):
    """The struct of the slot's concealment, for the stand-alone op."""
    return _lib.conceal_cfg(W.SETTINGS[slot]["conceal"]["rate"] or W.RATE)


def _echo_cfg(slot):
    kw = dict(W.SETTINGS[slot]["echo"])
    return _lib.echo_cfg(kw.pop("rate") or W.RATE, **kw)


@pytest.fixture(scope="module")
def refs():
    return _ref(W.MAX_SLOTS)


def _open(full, refs, slots, settings=None, max_slots=W.MAX_SLOTS, out_ld=W.OUT_LD):
    """A stream-set that holds the settings of `slots` only."""
    settings = W.SETTINGS if settings is None else settings
    st = full.streams(max_slots, W.MAX_FRAMES, W.MAX_REF, flags=_lib.STREAMS_FIXED_PLAN)
    st.reset(slots, which=15)
    st.set_reference(slots, refs[slots])
    if out_ld:
        st.set_output_ld(out_ld)
    for slot in slots:
        W.apply_settings(st, slot, settings[slot])
    return st


def _restart(st, refs, slots):
    st.reset(slots, which=15)
    st.set_reference(slots, refs[slots])


def _states(st, slot, settings):
    """Every state query of _lib.SLOT_FEATURES the slot's settings allow: keyword -> (the state rows, the seed rows)."""
    out = {}
    for key, f in _lib.SLOT_FEATURES.items():
        if key not in settings or settings[key].get("cfg", True) is None:      # (a feature the settings turn off has no state to query)
            continue
        state = st._feature_state(key, [slot]) if f.state else None
        seed = st._feature_seed_rows(key, [slot]) if f.seed_state else None
        cfg = st._get_feature(key, [slot]) if f.getter else None
        out[key] = (state.clone() if isinstance(state, torch.Tensor) else state, seed, cfg)
    return out


def _call_rows(utts, rows, settings, lost_on=True):
    """One call's input as the library takes it: (wav rows, samples, final, lost flags or None, far rows or None)."""
    wav, far, flags = [], [], torch.zeros(len(rows), 4, dtype=torch.int32)
    any_lost = any_far = False
    for i, r in enumerate(rows):
        u = utts[r["u"]]
        piece = torch.from_numpy(u["wav"][r["lo"]:r["hi"]].copy())
        wav.append(piece.cuda())
        fmt = settings[r["slot"]].get("in_format", "f32")
        if "far" in u and "echo" in settings[r["slot"]] and len(piece):
            far.append(torch.from_numpy(u["far"][r["lo"]:r["hi"]].copy()).cuda())
            any_far = True
        else:
            far.append(torch.full_like(piece, QUIET.get(fmt, 0)).cuda())
        if "lost" in u and "conceal" in settings[r["slot"]] and len(piece):
            p = u["packet"]
            assert r["lo"] % p == 0
            fl = u["lost"][r["lo"] // p:-(-r["hi"] // p)] if lost_on else []
            flags[i, :len(fl)] = torch.from_numpy(np.asarray(fl, dtype=np.int32))
            any_lost = True
    return wav, [r["hi"] - r["lo"] for r in rows], [r["final"] for r in rows], flags.cuda() if any_lost else None, far if any_far else None


def _run(st, refs, ticks, settings=None, pipelined=False, hooks=False, refuse_at=None, lost_on=True, first_tick=0, slot_of=None, utts=None):
    """The schedule on `st`, one step_wav_ragged call per tick -> dict(calls: per utterance its calls' records in order, tail: per
    utterance what flush_output gave, emit: per tick the call's emits, states: per slot every state query at the end).  A record is
    dict(emit, codes, mel, wav in the slot's output dtype[, hooks, states]); hooks=True reads every `last=` hook of
    _lib.SLOT_FEATURES and every state query behind every call (they join pipelined work).  refuse_at: that tick's call is first
    made twice in forms the library refuses.  first_tick: the ticks in front of it are left out; slot_of maps a slot of the
    schedule to the slot of `st` that plays it; utts: the utterances of `ticks` (default: the cases')."""
    utts = W.utterances() if utts is None else utts
    settings = W.SETTINGS if settings is None else settings
    slot_of = slot_of or {}
    step = st.step_wav_ragged_async if pipelined else st.step_wav_ragged
    out = dict(calls={}, tail={}, emit=[], states={})
    live_slots = set()
    for t in ticks:
        if t["tick"] < first_tick:
            continue
        rows = t["rows"]
        slots = [slot_of.get(r["slot"], r["slot"]) for r in rows]
        for slot in t["resets"]:
            s = slot_of.get(slot, slot)
            st.reset([s], which=15)      # (CONAN_MODEL_FRONTEND included: the features' restarts)
            st.set_reference([s], refs[[slot]])
        wav, samples, final, lost, far = _call_rows(utts, rows, settings, lost_on)
        if refuse_at == t["tick"]:
            assert len(rows) == len(W.SLOTS)
            # follow.plan is the last plan() whose refusal a call with slots 0 and 1 can reach: the sample-rate refusals of the
            # detector and the tone stage behind it are its own condition, which it meets first; the equaliser and the leveller
            # have planned their rows by then, and out_plan (the next refusal) has planned every group's output rows
            with pytest.raises(_lib.ConanError) as e:
                st.step_wav_ragged(slots, wav, samples, final, mel=dict(fft_size=256, win_length=256))
            assert e.value.code == _lib.ERR_INVALID and "fmin needs lags beyond half the frame" in str(e.value), str(e.value)
            st.set_output_ld(L)
            with pytest.raises(_lib.ConanError) as e:
                st.step_wav_ragged(slots, wav, samples, final)
            assert e.value.code == _lib.ERR_INVALID and "slot 5" in str(e.value) and "more than the row stride" in str(e.value), str(e.value)
            st.set_output_ld(W.OUT_LD)
        emit, c, m, w = step(slots, wav, samples, final, lost=lost, far=far)
        counts = st.output_samples()
        assert list(emit) == t["plan"]["emit"], (t["tick"], list(emit), t["plan"]["emit"])      # the host rules of the cases' replay
        out["emit"].append(list(emit))
        last = {}
        if hooks:
            st.join()
            last = {key: [x.clone() for x in HOOKS[key](st)] for key, f in _lib.SLOT_FEATURES.items() if f.last and any(key in settings[r["slot"]] for r in rows)}
        for i, (r, slot) in enumerate(zip(rows, slots)):
            e = emit[i]
            live_slots.add((r["slot"], slot))
            rec = dict(emit=e, codes=c[i, :e], mel=m[i, :e], wav=st.wav_row(w, i, slot, counts[i]))
            if hooks:
                rec["hooks"] = {}
                for key, got in last.items():
                    if key in settings[r["slot"]]:
                        rec["hooks"][key] = [x[i] for x in got]
                    else:
                        assert not any(bool(x[i].any()) for x in got), (t["tick"], slot, key)      # a row without the feature reads zeros
                rec["states"] = _states(st, slot, settings[r["slot"]])
            out["calls"].setdefault(r["u"], []).append(rec)
        for u in t["done"]:
            slot = slot_of.get(utts[u]["slot"], utts[u]["slot"])
            if "out_rate" in settings[utts[u]["slot"]]:
                out["tail"][u] = st.flush_output([slot])[0]      # (joins pipelined work)
    st.join()
    torch.cuda.synchronize()
    for sched, slot in sorted(live_slots):
        out["states"][sched] = _states(st, slot, settings[sched])
    return out


def _delivered(run, u):
    """An utterance's delivered audio, the flush included, as one row."""
    rows = [r["wav"] for r in run["calls"][u]] + ([run["tail"][u]] if u in run["tail"] else [])
    return torch.cat(rows)


def _frames(run, u, key, k):
    """Row k of a hook over an utterance's emitted frames."""
    return torch.cat([r["hooks"][key][k][:r["emit"]] for r in run["calls"][u]]).cpu().numpy()


@pytest.fixture(scope="module")
def blocking(full, refs):
    """The run every test compares with: blocking, with every hook and state query behind every call.  Left unchanged."""
    st = _open(full, refs, W.SLOTS)
    run = _run(st, refs, W.schedule(), hooks=True)
    st.close()
    return run


def _solo(full, refs, slot, settings=None, hooks=True, **kw):
    """The slot's utterances alone in a stream-set that holds its settings only (no output stride where no row needs one)."""
    settings = {**W.SETTINGS, slot: settings} if settings is not None else W.SETTINGS
    utts = W.utterances()
    mine = tuple(u for u in range(len(utts)) if utts[u]["slot"] == slot)
    st = _open(full, refs, [slot], settings, out_ld=W.OUT_LD if settings[slot].get("out_rate", 0) > W.RATE else 0)
    run = _run(st, refs, W.schedule(only=mine), settings, hooks=hooks, **kw)
    st.close()
    return run, mine


# ------------------------------------------------------------------------------------------------------------- a. each slot alone

@pytest.mark.parametrize("slot", W.SLOTS)
def test_each_slot_equals_itself_alone(full, refs, blocking, slot):
    solo, mine = _solo(full, refs, slot)
    for u in mine:
        assert len(solo["calls"][u]) == len(blocking["calls"][u])
        for k, (a, b) in enumerate(zip(solo["calls"][u], blocking["calls"][u])):
            assert _same(a, b), (slot, u, k, _diff(a, b))
        assert _same(solo["tail"].get(u), blocking["tail"].get(u)), (slot, u)
    assert _same(solo["states"][slot], blocking["states"][slot]), (slot, _diff(solo["states"][slot], blocking["states"][slot]))


# ------------------------------------------------------------------------------------------------------------- b. pipelined

def _assert_runs_equal(got, want, what):
    assert got["emit"] == want["emit"], what
    for u in want["calls"]:
        for k, (a, b) in enumerate(zip(got["calls"][u], want["calls"][u])):
            b = b if "hooks" in a else {x: b[x] for x in a}
            assert _same(a, b), (what, u, k, _diff(a, b))
    assert _same(got["tail"], want["tail"]), (what, _diff(got["tail"], want["tail"]))
    assert _same(got["states"], want["states"]), (what, _diff(got["states"], want["states"]))


def test_pipelined_equals_blocking(full, refs, blocking):
    ticks = W.schedule()
    st = _open(full, refs, W.SLOTS)
    _assert_runs_equal(_run(st, refs, ticks, pipelined=True, hooks=True), blocking, "hooked")
    # free running, twice back to back on one stream-set: between the joins of tick 0 (no row emits) and of the reset in front of
    # slot 1's second utterance more calls are in flight than a stage has staging sets
    for again in range(2):
        _restart(st, refs, W.SLOTS)
        _assert_runs_equal(_run(st, refs, ticks, pipelined=True), blocking, f"free {again}")
    st.close()


# ------------------------------------------------------------------------------------------------------------- c. refusals

def test_refused_calls_change_nothing(full, refs, blocking):
    st = _open(full, refs, W.SLOTS)
    _assert_runs_equal(_run(st, refs, W.schedule(), hooks=True, refuse_at=REFUSED_TICK), blocking, "refused")
    st.close()


# ------------------------------------------------------------------------------------------------------------- g. not vacuous

def test_every_stage_acted(full, refs, blocking):
    utts = W.utterances()
    for u, slot in ((0, 0), (1, 1)):
        gate = _frames(blocking, u, "activity", 1)
        assert gate.max() == FULL, (slot, gate)
        closed = np.nonzero(gate == 0)[0]
        closed = closed[closed > np.argmax(gate == FULL)]
        assert len(closed) and (gate[closed[-1]:] == FULL).any(), (slot, gate)      # open, closed, open again
        assert _frames(blocking, u, "comfort", 0)[closed].all(), slot      # the comfort level in the closed stretch
        digit, sound, level = (_frames(blocking, u, "tones", k) for k in range(3))
        assert [k for k, _, _ in _lib.tone_events(digit)] == [W.DIGIT], (slot, digit)
        assert (level[digit >= 0] > 0).all() and (sound[digit >= 0] == W.T.KEYS.index(W.DIGIT)).all(), slot      # ... and regenerated
        f0, uv = _frames(blocking, u, "follow", 0), _frames(blocking, u, "follow", 1)
        assert f0.any() and (uv == 0).any(), slot
        wet, dry = _frames(blocking, u, "bypass", 0), _frames(blocking, u, "bypass", 1)
        assert wet.any() and dry.any(), slot
    # a packet was repaired and an echo cancelled: the stand-alone ops change the rows the slots were fed
    for u, fmt in ((0, "ulaw"), (1, "f32")):
        src, far, lost = (torch.from_numpy(utts[u][k].copy()).cuda() for k in ("wav", "far", "lost"))
        fixed = full.conceal(src[None], lost[None], _conceal_cfg(utts[u]["slot"]), fmt)
        assert not torch.equal(fixed[0], src)
        cancelled, stats = full.echo(fixed, far[None], _echo_cfg(utts[u]["slot"]), fmt, stats=True)
        d2, e2, adapted, _ = (int(v) for v in stats[0].cpu())
        assert not torch.equal(cancelled[0], fixed[0]) and adapted > 0 and e2 < d2, (u, d2, e2, adapted)
    # the mark is found in what slots 0, 1 and 5 delivered, and not in slot 4's
    for u, present in ((0, True), (1, True), (6, True), (5, False)):
        slot = utts[u]["slot"]
        s = W.SETTINGS[slot]
        got = full.watermark_detect(_delivered(blocking, u), W.KEY, format=s.get("out_format", "f32"), rate=s.get("out_rate", W.RATE))[0]
        print("watermark", slot, got)
        assert got["present"] == present, (slot, got)      # (the id needs a whole word of 24 blocks: these rows hold two)


@pytest.mark.parametrize("stage", sorted(W.OUTPUT_STAGES_OFF))
def test_turning_one_output_stage_off_changes_the_delivered_bits(full, refs, blocking, stage):
    """... and nothing in front of the vocoder: the codes and the mel are the full run's."""
    settings = dict(W.SETTINGS[1])
    settings[stage] = W.OUTPUT_STAGES_OFF[stage]
    solo, mine = _solo(full, refs, 1, settings, hooks=False)
    for u in mine:
        assert _same([(r["codes"], r["mel"]) for r in solo["calls"][u]], [(r["codes"], r["mel"]) for r in blocking["calls"][u]]), (stage, u)
    assert not _same(_delivered(solo, mine[0]), _delivered(blocking, mine[0])), stage


def test_lost_packets_reach_the_model(full, refs, blocking):
    """The run without the lost flags (the silence stays in the rows) differs in slot 1's mel: the repair is in the chain."""
    solo, mine = _solo(full, refs, 1, hooks=False, lost_on=False)
    assert not _same(torch.cat([r["mel"] for r in solo["calls"][mine[0]]]), torch.cat([r["mel"] for r in blocking["calls"][mine[0]]]))


# ------------------------------------------------------------------------------------------------------------- d. the source side

SOURCE_SIDE = ("conceal", "echo", "in_format", "in_rate", "eq", "level")


@pytest.fixture(scope="module")
def prepared(full):
    """Per utterance of slots 0 and 1 the f32 model-rate audio its front-end reads, from the whole source signal by the stand-alone
    ops in the documented order: Context.conceal, echo, convert_samples, resample, eq, level, each from its zero state."""
    utts, out = W.utterances(), {}
    for u in (0, 1, 2):
        slot = utts[u]["slot"]
        s = W.SETTINGS[slot]
        fmt, rate = s.get("in_format", "f32"), s.get("in_rate", W.RATE)
        x, far, lost = (torch.from_numpy(utts[u][k].copy()).cuda()[None] for k in ("wav", "far", "lost"))
        x = full.conceal(x, lost, _conceal_cfg(slot), fmt)
        x = full.echo(x, far, _echo_cfg(slot), fmt)
        if fmt != "f32":
            x = full.convert_samples(x, fmt, "f32")
        if rate != W.RATE:
            x = full.resample(x, rate, W.RATE)
        x = full.eq(x, **s["eq"])
        out[u] = full.level(x, **s["level"])[0].clone()
    torch.cuda.synchronize()
    return out


def _whole(run, u, hooks=True):
    """An utterance's run over its emitted frames, whatever calls it was cut into: codes, mel, the delivered audio, the hooks' rows."""
    calls = run["calls"][u]
    out = dict(codes=torch.cat([r["codes"] for r in calls]), mel=torch.cat([r["mel"] for r in calls]), wav=_delivered(run, u))
    if hooks:
        out["hooks"] = {key: [torch.cat([r["hooks"][key][k][:r["emit"]] for r in calls]) for k in range(len(calls[0]["hooks"][key]))] for key in calls[0]["hooks"]}
    return out


def _variant(full, refs, slot, settings, wavs, hooks=True):
    """The slot's utterances with other settings and other audio (f32 at the model rate), alone -> (the run, its utterances)."""
    utts = [dict(slot=slot, start=30 * k, wav=w.cpu().numpy(), chunk=L, reuse=k > 0) for k, w in enumerate(wavs)]
    settings = {**W.SETTINGS, slot: settings}
    st = _open(full, refs, [slot], settings, out_ld=0)
    run = _run(st, refs, W.build_schedule(utts, settings), settings, hooks=hooks, utts=utts)
    st.close()
    return run


@pytest.mark.parametrize("slot", [0, 1])
def test_the_source_side_equals_the_stand_alone_ops(full, refs, blocking, prepared, slot):
    """Slots 0' and 1': the settings without conceal, echo, input format, input rate, input eq and input level, fed what the
    stand-alone ops make of the whole source.  Slot 1's span holds both staging paths (the equaliser's own and the resampler's)."""
    mine = [u for u in (0, 1, 2) if W.utterances()[u]["slot"] == slot]
    settings = {k: v for k, v in W.SETTINGS[slot].items() if k not in SOURCE_SIDE}
    run = _variant(full, refs, slot, settings, [prepared[u] for u in mine])
    for k, u in enumerate(mine):
        got, want = _whole(run, k), _whole(blocking, u)
        assert _same(got, want), (slot, u, _diff(got, want))


# ------------------------------------------------------------------------------------------------------------- e. the output side

def _padded(x, frames):
    """The source as the mix sees it: zeros beyond the samples received."""
    out = torch.zeros(frames * HOP, device=x.device)
    out[:len(x)] = x
    return out


@pytest.mark.parametrize("slot", [0, 1])
def test_the_output_side_equals_the_stand_alone_ops(full, refs, blocking, prepared, slot):
    """Slots 0'' and 1'': the source-side settings with every output stage off (activity and tones only detect) give the raw vocoder
    audio; the stand-alone ops in the order of hifigan_step, with the per-frame levels the full slot's own hooks report, give the
    delivered rows of the full slot, the flush included."""
    s = W.SETTINGS[slot]
    mine = [u for u in (0, 1, 2) if W.utterances()[u]["slot"] == slot]
    settings = {k: v for k, v in s.items() if k not in SOURCE_SIDE + ("bypass", "comfort", "out_eq", "out_level", "watermark", "out_rate", "out_format")}
    settings.update(activity=dict(s["activity"], gate=False), tones=dict(s["tones"], regenerate=False))
    raw = _variant(full, refs, slot, settings, [prepared[u] for u in mine])
    act, byp, cmf = _lib.activity_cfg(**s["activity"]), _lib.bypass_cfg(**s["bypass"]), _lib.comfort_cfg(**s["comfort"])
    for k, u in enumerate(mine):
        r, want = _whole(raw, k), _whole(blocking, u)
        assert _same(r["codes"], want["codes"]) and _same(r["mel"], want["mel"]), (slot, u)      # the output stages touch no model input
        h = want["hooks"]
        assert _same(r["hooks"]["activity"], h["activity"]) and _same(r["hooks"]["tones"][0], h["tones"][0]), (slot, u)
        frames = len(r["codes"])
        gate, (wet, dry), comfort, (_, sound, level) = h["activity"][1][None], (x[None] for x in h["bypass"]), h["comfort"][0][None], h["tones"]
        y = r["wav"][None]
        assert y.shape[1] == frames * HOP
        y = full.eq(y, **s["out_eq"])
        y = full.level(y, **s["out_level"])
        y = full.activity_gate(y, gate, start_level=int(act.seed.level))
        y = full.bypass_mix(y, _padded(prepared[u], frames)[None], wet, dry, start=(int(byp.seed_wet), (int(byp.seed_dry) * (FULL - int(act.seed.level))) >> 20))      # (bypass_ref.seed_state: the fill formula on the seed)
        y = full.comfort_fill(y, gate, comfort, cfg=cmf, seeds=[s["comfort"]["seed"]], start=(int(act.seed.level), cmf.seed_level))
        y = full.watermark_embed(y, **s["watermark"])
        y = full.tone_fill(y, sound[None], level[None], cfg=_lib.tone_cfg(**s["tones"]))
        if "out_rate" in s:
            y = full.resample(y, W.RATE, s["out_rate"])
        if "out_format" in s:
            y = full.convert_samples(y, "f32", s["out_format"])
        assert _same(y[0], want["wav"]), (slot, u, y.shape, want["wav"].shape, int((y[0] != want["wav"]).sum()) if y[0].shape == want["wav"].shape else -1)


# ------------------------------------------------------------------------------------------------------------- f. the hand-over

# keyword -> (the setter's keywords in the settings, the state rows, the seed rows, the getter's keywords) -> the setter's keywords on
# the importing side, as each feature's own documentation states the protocol ("The chain as a whole"); None: the slot
# snapshot carries the feature
HAND_OVER = dict(
    eq=lambda kw, state, rows, cfg: dict(cfg=cfg, seed=rows),
    level=None,
    pitch=None,
    follow=lambda kw, state, rows, cfg: dict(kw),
    register=lambda kw, state, rows, cfg: dict(kw, seed=tuple(int(v) for v in state[0].tolist()), reseed=True),
    activity=lambda kw, state, rows, cfg: dict(kw, seed=state[0], reseed=True),
    bypass=lambda kw, state, rows, cfg: dict(kw, start=(state[0]["wet"], state[0]["dry"]), reseed=True),
    conceal=lambda kw, state, rows, cfg: dict(kw, seed=rows),
    echo=lambda kw, state, rows, cfg: dict(kw, seed=rows),
    denoise=lambda kw, state, rows, cfg: dict(kw, seed=rows, reseed=True),
    comfort=lambda kw, state, rows, cfg: dict(kw, start=state[0]["level"], reseed=True),
    tones=lambda kw, state, rows, cfg: dict(kw, seed=state[0], reseed=True),
    out_eq=lambda kw, state, rows, cfg: dict(cfg=cfg, seed=rows),
    out_level=lambda kw, state, rows, cfg: dict(kw, seed=rows),
    watermark=lambda kw, state, rows, cfg: dict(kw, seed=rows, reseed=True),
)
def _no_cfg(states):
    """The state and seed rows without the getters' settings: a handed-over seed is part of the setting a getter reports."""
    return {k: v[:2] for k, v in states.items()}


CUT_TICK = 4      # slot 1 has taken three calls: 3840 samples in, 2560 out - off the leveller's grid of 100 ms blocks on both sides


def test_hand_over_of_everything_at_once(full, refs, blocking):
    """Slot 1 in mid-utterance: every state and seed_state of _lib.SLOT_FEATURES is queried, the slot exported, imported into
    another slot index of a stream-set of another size, every setter called again with the queried seeds; the run goes on as the
    uncut one - outputs, hooks and the states behind every call.  (A model-rate slot's calls are whole segments of the equaliser,
    whose pending tail is therefore empty here: its own test cuts off that grid.)"""
    ticks = W.schedule(only=(1,))
    settings = W.SETTINGS[1]
    a = _open(full, refs, [1])
    _run(a, refs, [t for t in ticks if t["tick"] < CUT_TICK])
    states = _states(a, 1, settings)
    snap = a.export_slots([1])
    b = full.streams(W.MAX_SLOTS + 2, W.MAX_FRAMES, W.MAX_REF, flags=_lib.STREAMS_FIXED_PLAN)
    b.import_slots([2], snap)
    assert b.layout_id == a.layout_id
    for key, f in W.CHAIN_FEATURES.items():      # (the walk is over the table: a feature without a protocol fails here)
        assert key in HAND_OVER, f"{key}: no hand-over protocol in this test"
        assert HAND_OVER[key] is not None or not f.seed_state, f"{key} has a seed_state and is not handed over"
        if HAND_OVER[key] is not None:
            state, rows, cfg = states[key]
            getattr(b, f.method)([2], **HAND_OVER[key](settings[key], state, rows, cfg[0] if cfg else None))
    # the opaque records are the slot's at once (the struct states report their seeds until the first chunk restarts from them)
    seeded = {k: v[1] for k, v in _states(b, 2, settings).items()}
    assert _same(seeded, {k: v[1] for k, v in states.items()}), _diff(seeded, {k: v[1] for k, v in states.items()})
    assert [b.input_eq([2])[0], b.output_eq([2])[0]] == [states["eq"][2][0], states["out_eq"][2][0]]      # (the grids' origins and positions)
    got = _run(b, refs, ticks, {**W.SETTINGS, 2: settings}, hooks=True, first_tick=CUT_TICK, slot_of={1: 2})
    a.close(); b.close()
    want = blocking["calls"][1]
    done = len(want) - len(got["calls"][1])
    assert done == CUT_TICK - W.utterances()[1]["start"]
    for k, (x, y) in enumerate(zip(got["calls"][1], want[done:])):
        x, y = dict(x, states=_no_cfg(x["states"])), dict(y, states=_no_cfg(y["states"]))
        assert _same(x, y), (k + done, _diff(x, y))


# ------------------------------------------------------------------------------------------------------------- the engine

def test_an_engine_utterance_with_every_feature_keyword(full, refs, blocking):
    """start_wav with every keyword of _lib.SLOT_FEATURES at once (through infer_wav, whose calls are same-position ones): the bytes of
    the Streams run of slot 1."""
    from conan_amd.engine import StreamingVoiceConversionEngine
    u = W.utterances()[1]
    kw = {k: (dict(v) or True) for k, v in W.SETTINGS[1].items()}
    kw.update(conceal=True, echo={k: v for k, v in W.SETTINGS[1]["echo"].items() if k != "rate"})      # (the engine names the slot's rate itself)
    assert set(kw) == set(W.CHAIN_FEATURES)
    n = W.MAX_SLOTS      # (a fixed plan follows max_slots: an engine of the stream-set's size, the utterance in every row)
    eng = StreamingVoiceConversionEngine(full, n, max_ref_frames=W.MAX_REF, flags=_lib.STREAMS_FIXED_PLAN)
    src, far, lost = (torch.from_numpy(u[k].copy()).cuda()[None].repeat(n, 1) for k in ("wav", "far", "lost"))
    want = _whole(blocking, 1, hooks=False)
    for pipelined in (False, True):
        w, m, c = eng.infer_wav(src, refs[[1] * n], pipelined=pipelined, lost=lost, far=far, **kw)
        torch.cuda.synchronize()
        for row in range(n):
            got = dict(codes=c[row], mel=m[row], wav=w[row])
            assert _same(got, want), (pipelined, row, _diff(got, want))
    eng.st.close()
