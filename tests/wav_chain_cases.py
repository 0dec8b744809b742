"""The cases the chain tests share (tests/test_gpu_wav_chain.py on the GPU, tests/test_wav_chain_cpu.py without one): the slot table,
the utterances, the tick schedule, and the host rules of a wav-in call restated in Python ("The chain as a whole").  Plain
data and numpy: importable without a GPU.

  slot 0   "telephone": mu-law in at 8 kHz, conceal and echo at that rate and format, every other row of _lib.SLOT_FEATURES (activity
           mode 2 with the gate, bypass fill_gate half and half), out at 8 kHz in mu-law
  slot 1   every row of _lib.SLOT_FEATURES at the model rate in f32; two utterances with a reset (which=15) between them
  slot 2   input level only
  slot 3   s16 in and s16 out only
  slot 4   no setter ever called
  slot 5   the output side only: output eq, output level, watermark, out at 24 kHz

  tick      0    1    2    3    4    5    6    7    8    9   10   11   12      (one ragged call per tick over the live slots; the
  slot 0                   0    4    4    4    4    4    0                      frames a row emits; | the reset of slot 1)
  slot 1         0    4    4    4    4    4    0 |  0    4    4    3    0
  slot 2    0    4    4    4    3    0
  slot 3                   0    4    4    2    0
  slot 4    0    4    4    4    4    1    0
  slot 5                   0    4    4    4    4    4    0

Ticks 1 and 2: no row causes a resampler launch and slot 1 has the equaliser, which stages the call (slots 2 and 4 ride as copy rows,
slot 2's leveller works in place).  Ticks 3 .. 5: slots 0 and 3 bring a launch, and both stages work in place.  Tick 0: the leveller
stages.  Tick 4: every slot is live, two emit groups, routed rows - the refused calls go in front of it.  Tick 6: slot 1 drains beside
rows with samples.  Tick 9: slot 1's first chunk behind its reset.  The rows last at most five chunks, which is less than the first
400 ms block of the levellers' meters and two blocks of the watermark's detector: the levellers act through their initial gain, and
the mark is loud enough for two blocks.
"""
import functools

import numpy as np

from conan_amd import _lib
from tests import activity_ref as A
from tests import resample_ref as rs
from tests import sample_format_ref as SF
from tests import tone_ref as T

HOP, SEG, RC, NFFT = 320, 4, 2, 1024      # the small synthetic full model: segment 4, right context 2, the default front-end
L = SEG * HOP
RATE = 50 * HOP
MAX_SLOTS, MAX_FRAMES, MAX_REF = 6, 4, 64
SLOTS = [0, 1, 2, 3, 4, 5]
STAGE_SETS = 4                            # kStageSets (csrc/streams.h): the depth of every stage's staging sets
OUT_LD = -(-L * 24000 // RATE) + 2        # the output stride: a full chunk of the fastest slot (slot 5 at 24 kHz)
KEY, ID = 0x0123456789ABCDEF, 0xBEEF
KW = dict(hold_frames=1, attack_frames=2, release_frames=3)      # the activity tests' detector: it opens and closes within a few chunks
RATES = ("in_rate", "out_rate", "in_format", "out_format")
DIGIT = "5"


# the chain's features: the table's rows that the engine applies as the table's keywords (the echo-delay estimator, which the engine
# steers by rules of its own and which changes no sample, has its own tests)
CHAIN_FEATURES = {k: f for k, f in _lib.SLOT_FEATURES.items() if not f.engine_own}


def every_feature(rate):
    """Every row of CHAIN_FEATURES, keyword -> the keywords of its Streams setter; conceal and echo at `rate` (None: the model's)."""
    return dict(
        eq=dict(sections=[dict(kind="highpass", f=120.0)]),
        level=dict(target=-26.0, initial_gain_db=-4.0),      # (the rows end before the meter's first block of 400 ms: the initial gain is what acts)
        pitch=dict(shift_semitones=2.0),
        follow={},
        register=dict(target=7.5),
        activity=dict(gate=True, **KW),
        bypass=dict(wet=0.5, dry=0.5, fill_gate=True),
        conceal=dict(rate=rate),
        echo=dict(rate=rate, mu_shift=1),
        denoise={},
        comfort=dict(seed=0x5EED),
        tones=dict(gain=0.05),      # (quiet: the regenerated pair is unmarked audio in a row of two detector blocks)
        out_eq=dict(sections=[dict(kind="peak", f=1800.0, q=1.5, gain_db=4.0)]),
        out_level=dict(target=-24.0, initial_gain_db=-3.0),
        watermark=dict(key=KEY, id=ID, gain=1.0, floor=0.05),      # (loud, and alive in the closed gate: the rows are two detector blocks long)
    )


# slot -> keyword -> the setter's keywords; the keywords are _lib.SLOT_FEATURES's plus RATES
SETTINGS = {
    0: dict(every_feature(8000), in_rate=8000, out_rate=8000, in_format="ulaw", out_format="ulaw"),
    1: every_feature(None),
    2: dict(level=dict(target=-26.0, initial_gain_db=-4.0)),
    3: dict(in_format="s16", out_format="s16"),
    4: {},
    5: dict(out_eq=dict(sections=[dict(kind="lowshelf", f=300.0, q=0.7, gain_db=-6.0)]), out_level=dict(target=-20.0, initial_gain_db=5.0), watermark=dict(key=KEY, id=ID + 1, gain=0.25),
            out_rate=24000),
}
# the nine output stages of hifigan_step a slot can lose one at a time: keyword -> the setter's keywords that turn the stage off
# (the detectors stay: the gate and the regeneration are their mode 2)
OUTPUT_STAGES_OFF = dict(out_eq=dict(cfg=None), out_level=dict(cfg=None), activity=dict(gate=False, **KW), bypass=dict(cfg=None), comfort=dict(cfg=None),
                         watermark=dict(cfg=None), tones=dict(regenerate=False))


def apply_settings(st, slot, settings=None):
    """The slot's setters, in the order the engine's open_slots applies them: output rate, formats, input rate, then _lib.SLOT_FEATURES."""
    s = SETTINGS[slot] if settings is None else settings
    assert set(s) <= set(_lib.SLOT_FEATURES) | set(RATES), sorted(s)
    if "out_rate" in s:
        st.set_output_rate([slot], s["out_rate"])
    if "in_format" in s:
        st.set_input_format([slot], s["in_format"])
    if "out_format" in s:
        st.set_output_format([slot], s["out_format"])
    if "in_rate" in s:
        st.set_input_rate([slot], s["in_rate"])
    for key, f in _lib.SLOT_FEATURES.items():
        if key in s:
            getattr(st, f.method)([slot], **s[key])


# ---------------------------------------------------------------------------------------------------------------- the source signals

GAP = 5400      # where the second burst begins: five quiet frames behind the first, enough for the hang-over and the whole release


def _speech(N, seed, digit_frame):
    """N samples cut out of the activity tests' burst signal - noise, the 210 Hz burst over [800, 2720), noise, the 120 Hz burst from
    GAP on: the gate opens, closes and reopens inside five chunks - with one DTMF digit of four frames in the first burst, off the
    frame grid."""
    b = A.burst_signal(noise=1e-3, seed=seed).astype(np.float64)
    x = np.concatenate([b[20000:23200], b[32000 - (GAP - 3200):]])[:N].copy()
    pos = digit_frame * HOP + 37
    x[pos:pos + 4 * HOP] = T.pair(DIGIT, 4 * HOP, (-12.0, -14.0), start=pos)
    return x


def _far(N, seed, lo, hi, delay, gain):
    """(far [N], its echo [N]): an independent noise that is on in [lo, hi), and the delayed, attenuated copy the microphone hears."""
    rng = np.random.default_rng(seed)
    far = 0.2 * rng.standard_normal(N)
    far[:lo] = 0.0
    far[hi:] = 0.0
    echo = np.zeros(N)
    echo[delay:] = gain * far[:N - delay]
    return far, echo


@functools.lru_cache(maxsize=None)
def telephone():
    """Slot 0's utterance: (mic mu-law [N8], far mu-law [N8], lost [packets of 160]) at 8 kHz.  Packets 6 and 11 never arrived: 11 is
    the last packet of the third call, so its fade back into received audio lies in the fourth."""
    N8 = 4 * (L // 2) + 600
    x16 = _speech(2 * N8, 17, 3)
    x8 = rs.resample(x16[None], RATE, 8000)[0][0]
    far, echo = _far(N8, 5, 0, 1300, 9, 0.25)
    mic = SF.encode((x8 + echo).astype(np.float32), "ulaw")
    lost = np.zeros(-(-N8 // 160), dtype=np.int32)
    lost[[6, 11]] = 1
    for p in np.nonzero(lost)[0]:
        mic[p * 160:(p + 1) * 160] = 0xFF      # (mu-law silence: what a receiver puts where nothing arrived)
    return mic, SF.encode(far.astype(np.float32), "ulaw"), lost


@functools.lru_cache(maxsize=None)
def wideband(which):
    """Slot 1's utterances 'a' and 'b': (mic f32 [N], far f32 [N], lost [packets of 320]) at the model rate."""
    N, seed, frame = (4 * L + 1200, 23, 3) if which == "a" else (2 * L + 700, 29, 4)
    far, echo = _far(N, 7 if which == "a" else 8, 0, 2600, 21, 0.25)
    mic = (_speech(N, seed, frame) + echo).astype(np.float32)
    lost = np.zeros(-(-N // HOP), dtype=np.int32)
    lost[5] = 1
    mic[5 * HOP:6 * HOP] = 0.0
    return mic, far.astype(np.float32), lost


def _noise(N, seed, amp=0.1):
    return (amp * np.random.default_rng(seed).standard_normal(N)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def utterances():
    """dict(slot, start tick, wav in the slot's input dtype, chunk = the samples of a non-final call[, far, lost, reuse])."""
    t, a, b = telephone(), wideband("a"), wideband("b")
    return [dict(slot=0, start=3, wav=t[0], far=t[1], lost=t[2], packet=160, chunk=L // 2),                          # 5 calls with samples
            dict(slot=1, start=1, wav=a[0], far=a[1], lost=a[2], packet=HOP, chunk=L),                               # 5
            dict(slot=1, start=8, wav=b[0], far=b[1], lost=b[2], packet=HOP, chunk=L, reuse=True),                   # 3, behind the reset
            dict(slot=2, start=0, wav=_noise(3 * L + 650, 71), chunk=L),                                              # 4
            dict(slot=3, start=3, wav=SF.encode(_noise(2 * L + 400, 72), "s16"), chunk=L),                           # 3
            dict(slot=4, start=0, wav=_noise(4 * L + 100, 73), chunk=L),                                              # 5
            dict(slot=5, start=3, wav=_noise(4 * L + 1200, 74), chunk=L)]                                              # 5


# ---------------------------------------------------------------------------------------------------------------- the host rules

class Rate:
    """length() and ready() of ch::RsTable (csrc/host_common.h) for the default filter."""

    def __init__(self, in_rate, out_rate):
        self.orig, self.new, self.w, ph = rs.filt(in_rate, out_rate)
        self.ph = [(klo, len(h)) for klo, h in ph]

    def length(self, n):
        return -(-self.new * n // self.orig)

    def ready(self, n):
        best = self.length(n)
        for p, (klo, cnt) in enumerate(self.ph):
            c = klo + cnt - 1 - self.w
            q = 0 if n - c <= 0 else -(-(n - c) // self.orig)
            best = min(best, p + self.new * q)
        return best


class Host:
    """What wavio::step_wav keeps and decides on the host for a stream-set with `settings` (slot -> keywords) and an output stride:
    rs_plan, fe_plan, the emit groups, direct / scatter / route, and which stage gets the resampler's staging set."""

    def __init__(self, settings=None, out_ld=OUT_LD):
        self.settings = SETTINGS if settings is None else settings
        self.out_ld = out_ld
        self.tables = {s: Rate(c["in_rate"], RATE) for s, c in self.settings.items() if c.get("in_rate", RATE) != RATE}
        self.fe, self.rs = {}, {}
        for s in self.settings:
            self.reset(s)

    def reset(self, slot):
        self.fe[slot] = dict(recv=0, frames=0, chunks=0)
        self.rs[slot] = dict(inp=0, out=0)

    def call(self, slots, samples, final):
        mm, ff, launch = [], [], False
        for slot, sm, fin in zip(slots, samples, final):
            c = self.settings[slot]
            if slot in self.tables:
                t, r = self.tables[slot], self.rs[slot]
                I = r["inp"] + sm
                if fin:
                    J = min(t.length(I), r["out"] + L)
                    f = int(J == t.length(I))
                else:
                    J, f = min(max(t.ready(I), r["out"]), r["out"] + L), 0
                m = J - r["out"]
                r["inp"], r["out"] = I, J
                launch = launch or sm > 0 or m > 0
            else:
                m, f = sm, fin
                launch = launch or (c.get("in_format", "f32") != "f32" and sm > 0)
            mm.append(m); ff.append(f)
        emit = []
        for slot, m, f in zip(slots, mm, ff):
            o = self.fe[slot]
            R = o["recv"] + m
            fc = 1 + R // HOP if f else ((R - NFFT // 2) // HOP + 1 if R >= NFFT // 2 else 0)
            pos, e = o["chunks"] * SEG, 0
            if f:
                e = min(SEG, fc - pos) if pos < fc else 0
            elif pos + SEG + RC <= fc:
                e = SEG
            o["recv"], o["frames"], o["chunks"] = R, max(o["frames"], fc), o["chunks"] + (e > 0)
            emit.append(e)
        groups = [[i for i, e in enumerate(emit) if e == g] for g in range(SEG, 0, -1)]
        groups = [g for g in groups if g]
        direct = len(groups) == 1 and len(groups[0]) == len(slots) and emit[0] == SEG
        scatter = not direct and bool(groups)
        outward = [i for g in groups for i in g if self.settings[slots[i]].get("out_rate", RATE) != RATE or self.settings[slots[i]].get("out_format", "f32") != "f32"]
        eq_any = any("eq" in self.settings[s] and m > 0 for s, m in zip(slots, mm))
        lv_any = any("level" in self.settings[s] and m > 0 for s, m in zip(slots, mm))
        eq_stages = eq_any and not launch
        lv_stages = lv_any and not launch and not eq_stages
        return dict(slots=list(slots), samples=list(samples), final=list(final), model_samples=mm, emit=emit, groups=groups, launch=launch, eq_rows=eq_any,
                    eq_stages=eq_stages, lv_rows=lv_any, lv_stages=lv_stages, scatter=scatter, route=scatter and (self.out_ld != 0 or bool(outward)), outward=outward)


def build_schedule(utts, settings=None, only=None):
    """A run of `utts` from the host rules alone: per tick dict(tick, resets = the slots reset in front of the call, rows = per call
    row dict(u, slot, lo, hi, final, drain), plan = Host.call's answer, done = the utterances whose drain answered with no frame).
    only: the utterances (indices) of a run that holds those alone."""
    us = list(range(len(utts))) if only is None else list(only)
    host = Host(settings)
    pos, fin, done = {u: 0 for u in us}, {u: False for u in us}, {u: False for u in us}
    begun, ticks, tick = set(), [], -1
    while not all(done.values()):
        tick += 1
        live = [u for u in us if utts[u]["start"] <= tick and not done[u]]
        if not live:
            continue
        assert len({utts[u]["slot"] for u in live}) == len(live), (tick, live)      # a slot's earlier utterance has drained
        resets = [utts[u]["slot"] for u in live if u not in begun and utts[u].get("reuse")]
        begun.update(live)
        for s in resets:
            host.reset(s)
        rows = []
        for u in live:
            N, step = len(utts[u]["wav"]), utts[u]["chunk"]
            last = (N - 1) // step * step
            k = step if pos[u] < last else N - pos[u]
            rows.append(dict(u=u, slot=utts[u]["slot"], lo=pos[u], hi=pos[u] + k, final=int(pos[u] >= last), drain=fin[u]))
            pos[u] += k
        plan = host.call([r["slot"] for r in rows], [r["hi"] - r["lo"] for r in rows], [r["final"] for r in rows])
        ended = []
        for r, e in zip(rows, plan["emit"]):
            if r["drain"] and e == 0:
                done[r["u"]] = True
                ended.append(r["u"])
            fin[r["u"]] = fin[r["u"]] or bool(r["final"])
        ticks.append(dict(tick=tick, resets=resets, rows=rows, plan=plan, done=ended))
    return ticks


@functools.lru_cache(maxsize=None)
def schedule(only=None):
    """The chain test's run (build_schedule of utterances() under SETTINGS); only: a tuple of utterance indices."""
    return build_schedule(utterances(), None, only)
