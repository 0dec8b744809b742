"""CPU checks of the chain test's cases (tests/wav_chain_cases.py; the GPU side is tests/test_gpu_wav_chain.py): the settings table
names every per-slot feature, the schedule holds every kind of tick the chain test is about - from the host rules alone, replayed in
Python - and the references say that the source signals make every source-side stage act."""
import numpy as np

from conan_amd import _lib
from tests import activity_ref as A
from tests import conceal_ref as CR
from tests import echo_ref as ER
from tests import resample_ref as rs
from tests import sample_format_ref as SF
from tests import tone_ref as TR
from tests import wav_chain_cases as W


def test_the_settings_name_every_feature():
    """A feature added to _lib.SLOT_FEATURES fails here until slots 0 and 1 of the chain test enable it (W.CHAIN_FEATURES: all of the
    table but what the engine applies by its own rules)."""
    assert set(_lib.SLOT_FEATURES) - set(W.CHAIN_FEATURES) == {"echo_delay"}
    for slot in (0, 1):
        assert set(W.SETTINGS[slot]) - set(W.RATES) == set(W.CHAIN_FEATURES), (slot, set(W.CHAIN_FEATURES) ^ (set(W.SETTINGS[slot]) - set(W.RATES)))
    assert set(W.RATES) <= set(W.SETTINGS[0]) and not set(W.RATES) & set(W.SETTINGS[1])      # input and output rate, input and output format
    assert W.OUT_LD > W.L and W.OUT_LD >= -(-W.L * W.SETTINGS[5]["out_rate"] // W.RATE)       # ... and the output stride
    assert (W.SETTINGS[0]["in_rate"], W.SETTINGS[0]["out_rate"], W.SETTINGS[0]["in_format"], W.SETTINGS[0]["out_format"]) == (8000, 8000, "ulaw", "ulaw")
    assert W.SETTINGS[0]["conceal"]["rate"] == W.SETTINGS[0]["echo"]["rate"] == 8000
    assert W.SETTINGS[0]["activity"]["gate"] and W.SETTINGS[0]["bypass"] == dict(wet=0.5, dry=0.5, fill_gate=True)
    assert W.SETTINGS[2] == dict(level=W.SETTINGS[1]["level"]) and W.SETTINGS[3] == dict(in_format="s16", out_format="s16") and W.SETTINGS[4] == {}
    assert set(W.SETTINGS[5]) == {"out_eq", "out_level", "watermark", "out_rate"} and W.SETTINGS[5]["out_rate"] == 24000
    # every struct builds on the host (the keywords are the setters')
    for slot, s in W.SETTINGS.items():
        for key, kw in s.items():
            if key in W.RATES:
                continue
            f, kw = _lib.SLOT_FEATURES[key], dict(kw)
            if key in ("eq", "out_eq"):
                kw["rate"] = W.RATE
            if key in ("conceal", "echo"):
                kw["rate"] = kw["rate"] or W.RATE
            assert getattr(f.build(**kw), f.on), (slot, key)
    # the output stages slot 1 loses one at a time are stages it has
    assert set(W.OUTPUT_STAGES_OFF) <= set(W.SETTINGS[1])


def test_the_schedule_holds_every_kind_of_tick():
    utts, ticks = W.utterances(), W.schedule()
    by = {t["tick"]: t for t in ticks}
    for u in utts:
        calls = -(-len(u["wav"]) // u["chunk"])
        assert 3 <= calls <= 5, (u["slot"], calls)      # utterances of 3 to 5 chunks
    first = {u: min(t["tick"] for t in ticks for r in t["rows"] if r["u"] == u) for u in range(len(utts))}
    a = [t for t in ticks if any(r["u"] == 1 for r in t["rows"])]      # the ticks of slot 1's first utterance

    def fed(t, slot):
        return any(s == slot and m > 0 for s, m in zip(t["plan"]["slots"], t["plan"]["model_samples"]))

    # the equaliser stages the call: slot 1 has samples, no row causes a resampler launch, slots 2 and 4 ride as its copy rows and
    # slot 2's leveller works in place behind it
    staged = [t for t in a if t["plan"]["eq_stages"]]
    assert staged and all(fed(t, 1) and fed(t, 2) and fed(t, 4) and not t["plan"]["launch"] and t["plan"]["lv_rows"] and not t["plan"]["lv_stages"] for t in staged)
    # later ticks of the same utterance: slot 0 or 3 is in the call, a launch writes the staging and both stages work in place
    later = [t for t in a if t["tick"] > staged[-1]["tick"] and fed(t, 1) and t["plan"]["launch"]]
    assert later and all((fed(t, 0) or fed(t, 3)) and t["plan"]["eq_rows"] and not t["plan"]["eq_stages"] and not t["plan"]["lv_stages"] for t in later)
    assert any(fed(t, 0) for t in later) and any(fed(t, 3) for t in later)
    # slots 2 and 4 only: the leveller stages
    assert any(t["plan"]["slots"] == [2, 4] and t["plan"]["lv_stages"] and not t["plan"]["eq_rows"] and not t["plan"]["launch"] for t in ticks)
    # two emit groups with a row that carries a rate or a format out: the groups' audio is routed
    assert any(len(t["plan"]["groups"]) == 2 and t["plan"]["outward"] and t["plan"]["route"] for t in ticks)
    # an all-features slot drains beside rows with samples
    assert any(any(r["slot"] in (0, 1) and r["hi"] == r["lo"] and r["final"] for r in t["rows"]) and any(r["hi"] > r["lo"] for r in t["rows"]) for t in ticks)
    # the first chunk after the reset of slot 1, with and without a launch in the calls of that utterance
    reset = next(t for t in ticks if t["resets"] == [1])
    assert reset["tick"] == first[2] and reset["plan"]["emit"][reset["plan"]["slots"].index(1)] == 0
    after = by[reset["tick"] + 1]
    assert after["plan"]["emit"][after["plan"]["slots"].index(1)] == W.SEG
    b = [t for t in ticks if any(r["u"] == 2 for r in t["rows"]) and fed(t, 1)]
    assert any(t["plan"]["eq_stages"] for t in b)
    # a tick where every slot is live and takes part in the output, directly usable for the refused calls
    full = [t for t in ticks if t["plan"]["slots"] == W.SLOTS]
    assert any(all(e > 0 for e in t["plan"]["emit"]) and len(t["plan"]["groups"]) == 2 for t in full)
    # more calls in flight than a stage has staging sets: a call without an emitting row joins, and so does a reset or a flush
    run, best = 0, 0
    for t in ticks:
        if t["resets"] or not t["plan"]["groups"]:
            run = 0
        run += bool(t["plan"]["groups"])
        best = max(best, run)
        if any("out_rate" in W.SETTINGS[utts[u]["slot"]] for u in t["done"]):
            run = 0
    assert best > W.STAGE_SETS, best
    # each slot alone takes the calls it takes in the full run
    for u in range(len(utts)):
        mine = tuple(v for v in range(len(utts)) if utts[v]["slot"] == utts[u]["slot"])
        solo = [(r["lo"], r["hi"], r["final"], t["plan"]["emit"][i]) for t in W.schedule(only=mine) for i, r in enumerate(t["rows"]) if r["u"] == u]
        full_run = [(r["lo"], r["hi"], r["final"], t["plan"]["emit"][i]) for t in ticks for i, r in enumerate(t["rows"]) if r["u"] == u]
        assert solo == full_run, u


def _prepared(name):
    """(the source as fed, lost flags, repaired, cancelled, the echo's stats, the model-rate f32 audio the front-end reads) through
    the references."""
    mic, far, lost = W.telephone() if name == "t" else W.wideband(name)
    slot, rate, fmt = (0, 8000, "ulaw") if name == "t" else (1, W.RATE, "f32")
    fixed = CR.conceal(mic, lost, fmt, **CR.defaults(rate))
    fixed = fixed[0] if isinstance(fixed, tuple) else fixed
    kw = {k: v for k, v in W.SETTINGS[slot]["echo"].items() if k != "rate"}
    out, stats, _ = ER.cancel(fixed, far, fmt, **dict(ER.defaults(rate), **kw))
    x = out if name != "t" else rs.resample(SF.decode(out, "ulaw")[None].astype(np.float64), 8000, W.RATE)[0][0].astype(np.float32)
    return mic, lost, fixed, out, stats, x


def test_the_source_signals_make_every_source_stage_act():
    for name in ("t", "a", "b"):
        mic, lost, fixed, out, stats, x = _prepared(name)
        packet = 160 if name == "t" else W.HOP
        for p in np.nonzero(lost)[0]:      # every lost packet was repaired
            assert np.any(fixed[p * packet:(p + 1) * packet] != mic[p * packet:(p + 1) * packet]), (name, p)
        assert stats[2] > 0 and ER.erle_db(stats[0], stats[1]) > 0.0, (name, stats)      # an echo reduction above zero
        assert [k for k, _, _ in TR.events(TR.detect(x)[0])] == [W.DIGIT], name          # the digit
        level = A.run(x, _lib.activity_cfg(**W.KW))["level"]
        if name != "b":                                                                   # the gate opens, closes and opens again
            closed = np.nonzero(level == 0)[0]
            closed = closed[closed > np.argmax(level == A.FULL)]
            assert len(closed) and (level[closed[-1]:] == A.FULL).any(), (name, level)
    # slot 0's two lost packets: one in the middle of a call, one at a call's end
    lost = np.nonzero(W.telephone()[2])[0]
    per_call = (W.L // 2) // 160
    assert len(lost) == 2 and sorted(int(p) % per_call for p in lost) == [2, per_call - 1]
