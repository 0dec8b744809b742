"""Batched multi-stream serving engine: B independent utterance streams on one GPU, sharded by
slot range over the ranks of a torch.distributed job (one process per GPU).

Streams are independent units (private conv/KV state, no cross-stream arithmetic),
so the compute path has no collective.  The only exchange is the gather of finished audio to
rank 0 (RCCL `gather` over xGMI on GPUs, gloo in the CPU tests)."""
import functools
import os
import types

import numpy as np
import torch
import torch.distributed as dist

from . import _lib


def shard_range(total, rank, world):
    """Contiguous slot range [lo, hi) of `rank`: GPU g owns streams [g*B/W, (g+1)*B/W)."""
    base, rem = divmod(total, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def init_distributed(backend=None):
    """Read RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from the environment (torch.distributed.run)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        if backend is None:
            backend = "nccl" if torch.cuda.is_available() else "gloo"
        if backend == "nccl":
            torch.cuda.set_device(local)
        dist.init_process_group(backend=backend, rank=rank, world_size=world)
    return rank, local, world


def gather_audio(wav_local, world, rank, dst=0):
    """Gather per-rank audio [b_r, samples] to `dst` (ragged b_r allowed); returns the concatenated
    [B, samples] tensor on dst, None elsewhere."""
    if world == 1:
        return wav_local
    counts = [torch.zeros(1, dtype=torch.int64, device=wav_local.device) for _ in range(world)]
    dist.all_gather(counts, torch.tensor([wav_local.shape[0]], dtype=torch.int64, device=wav_local.device))
    counts = [int(c.item()) for c in counts]
    mx = max(counts)
    pad = wav_local
    if wav_local.shape[0] < mx:
        pad = torch.cat([wav_local, wav_local.new_zeros(mx - wav_local.shape[0], wav_local.shape[1])])
    bufs = [torch.empty_like(pad) for _ in range(world)] if rank == dst else None
    dist.gather(pad.contiguous(), bufs, dst=dst)
    if rank != dst:
        return None
    return torch.cat([b[:c] for b, c in zip(bufs, counts)])


def gather_audio_equal(wav_local, world, rank, bufs=None, dst=0):
    """Fast path when every rank holds the same number of streams (the benchmark's weak scaling)."""
    if world == 1:
        return wav_local
    if rank == dst and bufs is None:
        bufs = [torch.empty_like(wav_local) for _ in range(world)]
    dist.gather(wav_local, bufs if rank == dst else None, dst=dst)
    return bufs


class _HostStream:
    """Stand-in for torch.cuda.Stream / Event on a host-only process group (gloo): everything is synchronous, so
    waits and records are no-ops.  Lets the CPU tests drive the very choreography the GPU benchmark runs."""

    def wait_event(self, ev):
        pass

    def wait_stream(self, s):
        pass

    def synchronize(self):
        pass

    def record(self, stream=None):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


class AudioGatherRing:
    """Collection of finished audio on rank 0 (the path's only exchange) without serialising the chunk
    pipeline: audio of step j goes to buffer j % nb; gathers (RCCL on GPUs, gloo on CPU) are enqueued on a side stream
    behind `join()` (= "the audio of every step enqueued so far is complete"), and a buffer is handed out again only after
    the gather that read it has finished.

        ring = AudioGatherRing(lambda: torch.empty(B, samples, device=dev), world, rank, every=4)
        for j in range(steps):
            buf, fence = ring.acquire(j, fence=True)   # fence: the side stream, when a gather that read buf may be pending
            ... enqueue the step that writes buf (Streams.step_async(..., out_fence=fence)) ...
            ring.submit(j, join)                        # every `every`-th step: side stream: join(); gather(group); record
        ring.flush(steps - 1); ring.drain()

    `every` = steps per gather (SURVEY.md §8e allows per step or per utterance).  With every = 1 each step's buffer is gathered
    by itself (nb buffers).  With every = E > 1 the ring is 2 groups of E step buffers, contiguous in one allocation: the E
    buffers of a group travel in ONE collective after the group's last step while the next group's steps already write the
    other group, and the side stream is touched - one join, one gather, one event record, one output fence for the step that
    re-opens the group - once per E steps instead of once per step.  (Measured on one MI355X, world 1, where the gather itself
    is a no-op: the per-step form costs the 64-stream pipelined step 6.5 %)

    Pipelined steps should not take the wait on the current stream: it holds back the step's Emformer and decoder stages,
    which never touch the buffer, and drains the three-stage pipeline (measured: 1.81 -> 2.6 ms per step).  `acquire(j,
    fence=True)` returns the event recorded behind the gather that last read the buffer's group instead (None while no gather
    can be pending, and for every step but the first of a group) for `Streams.step_async(..., out_fence=fence)`: only the
    stage that writes the audio waits, and only for that gather.
    """

    def __init__(self, make_buffer, world, rank, nb=4, always=False, on_gathered=None, every=1):
        self.world, self.rank = world, rank
        self.every = max(1, int(every))
        self.nb = nb if self.every == 1 else 2 * self.every
        proto = make_buffer()
        self.pool = proto.new_zeros((self.nb,) + tuple(proto.shape))          # group g = pool[g * every : (g + 1) * every]
        self.bufs = [self.pool[i] for i in range(self.nb)]
        self.active = world > 1 or always
        self.cuda = proto.is_cuda
        self.on_gathered = on_gathered
        self._g = [proto.new_zeros((self.every,) + tuple(proto.shape)) for _ in range(world)] if (world > 1 and rank == 0) else None
        self.gbufs = None if self._g is None else [g[0] if self.every == 1 else g for g in self._g]   # what rank 0 last gathered, per rank
        ngroups = self.nb // self.every
        if self.active and self.cuda:
            self.comm = torch.cuda.Stream()
            self.done = [torch.cuda.Event() for _ in range(ngroups)]
        else:
            self.comm = _HostStream()
            self.done = [_HostStream() for _ in range(ngroups)]
        self.recorded = [False] * ngroups   # done[g] has been recorded at least once (an unrecorded event is no fence)
        self.submitted = 0            # gathers enqueued
        self.last_gathered = None     # last step whose audio has been handed to a gather
        self.last_sent = None         # the local tensor of that gather (a group of step buffers)
        self._next = 0                # first step not yet covered by a gather

    def acquire(self, j, fence=False):
        k = j % self.nb
        first = j % self.every == 0                       # the step that re-opens a group is the one that may collide with its gather
        # (a group whose gather was skipped - no submit() for it - has no recorded event: nothing to wait for)
        pending = self.active and j >= self.nb and first and self.recorded[k // self.every]
        if fence:       # the event recorded right behind the gather that read this group (NOT the side stream's tail: a later gather's
                        # join is already enqueued there, and it waits for the newest step)
            return self.bufs[k], (self.done[k // self.every] if (pending and self.cuda) else None)
        if pending:
            (torch.cuda.current_stream() if self.cuda else _HostStream()).wait_event(self.done[k // self.every])
        return self.bufs[k]

    def _gather(self, j, join, wait_current):
        """One collective for the steps self._next .. j (all in one group).  Only THEIR buffers travel: a flush() in the middle
        of a group must not read the buffers of the group's later steps, which may be written while the collective runs, and a
        group's remainder after a flush travels without the buffers the flush already sent."""
        g = (j % self.nb) // self.every
        lo, hi = max(0, self._next - (j - j % self.every)), j % self.every + 1
        grp = self.pool[g * self.every + lo:g * self.every + hi]
        dst = None if self._g is None else [b[lo:hi] for b in self._g]
        cur = torch.cuda.current_stream() if self.cuda else None
        ctxm = torch.cuda.stream(self.comm) if self.cuda else self.comm
        with ctxm:
            if wait_current and self.cuda:
                self.comm.wait_stream(cur)
            if join is not None:
                join()
            out = gather_audio_equal(grp, self.world, self.rank, dst)
            if self.on_gathered is not None and self.rank == 0:
                src = out if self.world > 1 else [grp]
                for js in range(self._next, j + 1):
                    self.on_gathered(js, [b[js % self.every - lo] for b in src])
            self.done[g].record(self.comm) if self.cuda else None
            self.recorded[g] = True
        if dst is not None:
            self.gbufs = [b[0] if self.every == 1 else b for b in dst]        # what rank 0 gathered last, per rank
        self.submitted += 1
        self.last_gathered, self.last_sent, self._next = j, grp, j + 1

    def submit(self, j, join=None, wait_current=False):
        """join: callable making the CURRENT stream wait for the audio of every step enqueued so far (Streams.join);
        wait_current: the audio was produced on the stream that is current now (blocking steps) - the side stream waits for
        it.  A gather is enqueued when step j completes a group."""
        if not self.active:
            self.last_gathered = j
            return
        self._join, self._wait_current = join, wait_current
        if (j + 1) % self.every == 0:
            self._gather(j, join, wait_current)

    def flush(self, j):
        """Gather the steps up to j that no gather has covered yet (a timed region that ends inside a group)."""
        if self.active and j >= self._next:
            self._gather(j, getattr(self, "_join", None), getattr(self, "_wait_current", False))

    def drain(self):
        if self.active:
            self.comm.synchronize()


def _per_slot(value, n):
    """One value per slot: a list or tuple as it is, anything else for all n."""
    return list(value) if isinstance(value, (list, tuple)) else [value] * n


def _by_value(slots, values):
    """[(value, the slots that have it)], values in order of first appearance."""
    return [(v, [s for s, x in zip(slots, values) if x == v]) for v in dict.fromkeys(values)]


_FOLLOW_KEYS = ("lead", "hyst", "max_age")      # the follow rule's keywords inside echo_delay= (_lib.echo_delay_follow)

# what True means to a feature's Streams setter, by engine keyword (register= has no True: a scalar is its target)
_TRUE = dict(level=True, pitch=True, follow=True, out_level=True, activity=dict(gate=True), bypass={}, conceal={}, echo={}, denoise={}, comfort={}, watermark={}, tones={})


def _accept(keyword, v, k, n, voice):
    """What value v (not None / False) of keyword= means for the k-th of n slots: the cfg of the feature's Streams setter.  A dict is
    the setter's keywords; True, a string and a scalar are the feature's own.  Host only: register="voice" is looked up in
    bank.registers of voice = (bank, ids) and is a ValueError where that has nothing to give."""
    forms = f"True, a dict of {_lib.SLOT_FEATURES[keyword].method}'s keywords"
    if isinstance(v, dict):
        return dict(v)
    if keyword == "register":
        if not isinstance(v, str):
            return dict(target=float(v))
        if v != "voice":
            raise ValueError(f"register: {v!r} (a target in log2 Hz, 'voice', a dict of set_pitch_register's keywords or None)")
        if voice is None:
            raise ValueError("register='voice' needs voice=(bank, ids)")
        bank, ids = voice
        if len(ids) != n:
            raise ValueError(f"register='voice': {len(ids)} voice ids for {n} slots")
        target = bank.registers.get(int(ids[k]))
        if target is None:
            raise ValueError(f"register='voice': voice {int(ids[k])} has no register (VoiceBank.enroll_wav(register=True))")
        return dict(target=target)
    if keyword in ("eq", "out_eq"):      # (no True: there is no default cascade, and a bare list would read as one value per slot)
        raise ValueError(f"{keyword}: {v!r} (a dict(sections=[...]) of {_lib.SLOT_FEATURES[keyword].method}'s keywords, a list with one per slot, or None)")
    if v is True:
        return dict(_TRUE[keyword]) if isinstance(_TRUE[keyword], dict) else True
    if keyword == "activity":
        if isinstance(v, str) and v == "detect":
            return dict(gate=False)
        forms = "True, 'detect', a dict of set_activity's keywords"
    if keyword == "conceal":
        if isinstance(v, _lib.ConcealCfg):
            return v
        forms = "True, a dict of conan_conceal_cfg's fields, an _lib.ConcealCfg"
    if keyword == "echo":
        if isinstance(v, _lib.EchoCfg):
            return v
        forms = "True, a dict of conan_echo_cfg's fields, an _lib.EchoCfg"
    raise ValueError(f"{keyword}: {v!r} ({forms} or None)")


class StreamingVoiceConversionEngine:
    """The chunk loop of StreamingVoiceConversion.infer_once (inference/Conan.py:72-166) for many
    streams at once: mel in -> (wav, mel, codes) out, state carried in a conan_streams handle."""

    def __init__(self, ctx, n_streams, max_ref_frames=256, max_frames=None, arith="auto", flags=0, dev_plan=None):
        self.ctx = ctx
        self.n = n_streams
        self.arith = arith          # conan_streams_opts.arith of the stream-set: 'auto' | 'f32' | 'limb'
        self.flags, self.dev_plan = flags, dev_plan      # conan_streams_opts.flags (_lib.STREAMS_*) / .dev_plan
        self.st = ctx.streams(n_streams, max_frames=max(ctx.cfg.emf_segment, max_frames or 0), max_ref_frames=max_ref_frames, arith=arith,
                              flags=flags, dev_plan=dev_plan)
        self.slots = list(range(n_streams))
        self.seg, self.rc = ctx.cfg.emf_segment, ctx.cfg.emf_right_context
        self._used = set()          # the keywords of _lib.SLOT_FEATURES whose setter has been called on the stream-set (_apply)
        # the echo-delay estimator (echo_delay=): whether its setter has been called, per slot the follow rule's keywords and the
        # last report read (est, age), and the report of the last far= call on its way to the host (_note_report)
        self._ed = types.SimpleNamespace(used=False, follow={}, last={}, pending=None)

    @staticmethod
    def _check_voice(ref_mel, voice):
        """Exactly one of ref_mel and voice = (bank, ids) names the target voices; -> (bank, ids) or None.  Host only."""
        if (ref_mel is None) == (voice is None):
            raise ValueError("give either ref_mel (a style pass per slot: Streams.set_reference) or voice=(bank, ids) (enrolled voices: "
                             "Streams.set_voice), not both and not neither")
        if voice is None:
            return None
        bank, ids = voice
        return bank, [int(i) for i in ids]

    def _reference(self, slots, ref_mel, ref_len, voice):
        """The slots' target voices: a style pass of ref_mel, or voice = (bank, ids), one enrolled id per slot."""
        voice = self._check_voice(ref_mel, voice)
        if voice is None:
            self.st.set_reference(slots, ref_mel, ref_len)
        else:
            self.st.set_voice(slots, voice[0], voice[1])

    def set_voice(self, slots=None, bank=None, ids=None):
        """A live change of the slots' target voice (all slots by default) to the enrolled voices `ids` of `bank`, between feed /
        feed_ragged calls, also mid-utterance and with pipelined steps in flight (Streams.set_voice: one launch, no style pass).
        Steps already enqueued keep the old voice; in force from the next call."""
        if bank is None or ids is None:
            raise ValueError("set_voice: bank= and ids= are required")
        self.st.set_voice(self.slots if slots is None else slots, bank, ids)

    def start(self, ref_mel, ref_len=None, which=7, out_rate=None, out_filter=None, out_format=None, pitch=None, voice=None, out_level=None, watermark=None, out_eq=None,
              drift=None):
        """drift: the far device's clock error in ppm (> 0: it runs fast; None: no compensation) - the audio then leaves through the
        drift resampler (Streams.set_output_drift) at out_rate, also at the model rate; set_drift changes it between steps.
        voice: (bank, ids) - enrolled voices of a runtime.VoiceBank, one id per slot, in place of ref_mel (then None).
        pitch: the slots' pitch control in the decoder step (Streams.set_pitch) - None / False: none; a dict of its keywords
        (shift_semitones, range, pivot, uv_threshold), or a list with one per slot.
        out_rate: the sample rate the audio leaves at (None: the model rate), resampled on the GPU behind the vocoder; out_filter:
        dict of Context.resample's filter keywords.  The steps then deliver what the filter has the inputs for, finish() the tail.
        out_format: the sample format the audio leaves in ('f32' | 's16' | 'ulaw' | 'alaw'; None: float32), encoded on the GPU.
        out_level: the output leveller (Streams.set_output_level) - None / False: none; True: Context.level's defaults; a dict: its
        keywords.  The same causal BS.1770 leveller as start_wav(level=...), on the converted voice: on the GPU between the vocoder
        and the gate, the mix, the output resampler and the encoders, without look-ahead or added latency.
        out_eq: the output equaliser (Streams.set_output_eq) - None / False: none; a dict(sections=[...]) of 1 .. 4 biquad sections
        (raw 5-tuples or dict(kind=, f=, q=, gain_db=) designed at the model rate), or a list with one dict per slot.  It runs on the
        GPU directly behind the vocoder, in front of the output leveller: the returned model-rate wav is ctx.eq of the unfiltered one,
        bit for bit.  Any cascade is the caller's choice: the library ships no preset, and nobody has listened to one.
        watermark: the output watermark (Streams.set_watermark) - None / False: none; a dict of its keywords (key, id, gain, floor),
        or a list with one per slot; True: the defaults, key 0 and id 0.  The mark goes into the audio on the GPU behind the last
        in-place stage, in front of the output resampler and the encoders: the returned model-rate wav is ctx.watermark_embed of the
        unmarked one, bit for bit, and Context.watermark_detect finds it again."""
        if isinstance(out_level, (list, tuple)):
            raise ValueError("out_level: one value for all slots here; open_slots and infer_wav_staggered take one per slot / utterance")
        if isinstance(out_rate, (list, tuple)) or isinstance(out_format, (list, tuple)):
            raise ValueError("out_rate / out_format: one value for all slots here (feed / infer return one [B, count] block); open_slots and "
                             "infer_wav_staggered take one per slot / utterance")
        self._check_voice(ref_mel, voice)
        if isinstance(drift, (list, tuple)):
            raise ValueError("drift: one value for all slots here; open_slots and infer_wav_staggered take one per slot / utterance")
        drifts = self._drift_values(drift, len(self.slots))
        values = self._host_checks(len(self.slots), pitch=pitch, out_level=out_level, watermark=watermark, out_eq=out_eq)
        self.st.reset(self.slots, which=which)
        self._reference(self.slots, ref_mel, ref_len, voice)
        self._set_out_rate(self.slots, out_rate, out_filter)
        self._set_drift(self.slots, drifts, out=(out_rate, out_filter))
        self._set_format(self.slots, out_format, self.st.output_formats, self.st.set_output_format)
        for keyword in values:      # (pitch, out_level, watermark)
            self._apply(keyword, self.slots, values[keyword])

    def start_wav(self, ref_mel, ref_len=None, in_rate=None, out_rate=None, out_filter=None, in_format=None, out_format=None, level=None,
                  pitch=None, voice=None, follow=None, register=None, activity=None, bypass=None, out_level=None, conceal=None, echo=None, echo_delay=None, comfort=None, denoise=None, watermark=None, tones=None, eq=None, out_eq=None,
                  drift=None, **filter):
        """start() plus a fresh streaming front-end (CONAN_MODEL_FRONTEND): the next feed() is the utterance's first audio.
        drift: the far device's clock error in ppm (start), on both sides of the slots: the input goes through the drift resampler
        too (Streams.set_input_drift, at in_rate or the model rate).  feed() then takes 0 .. 2 x 80 ms of samples per call and may
        emit nothing in a call; set_drift changes the value between calls.
        in_rate: the input's sample rate (None: the model rate), resampled on the GPU; filter: Context.resample's filter keywords.
        in_format: the input's sample format (None: float32; 's16' takes int16 rows, 'ulaw' / 'alaw' uint8), decoded on the GPU.
        out_rate / out_filter / out_format / out_level / watermark: as in start().
        level: the input leveller (Streams.set_input_level) - None / False: none; True: Context.level's defaults; a dict: its
        keywords.  It runs on the GPU on the decoded, resampled samples in front of the front-end, causally: feed() gains no latency.
        pitch, voice: as in start().
        follow: source-pitch following (Streams.set_pitch_follow) - None / False: none; True: the tracker's defaults; a dict of its
        keywords (fmin, fmax, threshold, floor_db).  The decoder steps then take f0 / uv from the input's own contour, tracked on the
        GPU on the samples the front-end reads; `pitch` applies on top.
        register: register matching for following slots (Streams.set_pitch_register) - None / False: none; a float: the target in
        log2 Hz; "voice": bank.registers[id] of the slot's voice=(bank, ids) (VoiceBank.enroll_wav(register=True)); a dict of
        set_pitch_register's keywords.  The followed contour is then moved to the target's register by a causal log-f0 mean.
        activity: the source-activity detector (Streams.set_activity) - None / False: none; True: detect and gate the output with
        the defaults; "detect": detect only; a dict of set_activity's keywords (gate=False: detect only).  chunk_activity() reads
        the last call's flags.  bypass: the wet/dry mix with the slot's own source audio (Streams.set_bypass) - None / False: none;
        True: enabled at full wet (a later set_bypass toggles it); a dict of set_bypass's keywords.  chunk_bypass() reads
        the last call's levels.  conceal: loss concealment of the input rows (Streams.set_conceal) - None / False: none; True: the
        defaults of the slot's input rate; a dict of conan_conceal_cfg's fields over them.  feed(lost=...) then repairs the packets
        that never arrived, on the GPU in front of the step.  echo: echo cancellation of the input rows (Streams.set_echo) - None /
        False: none; True: the defaults of the slot's input rate; a dict of conan_echo_cfg's fields over them.  feed(far=...) then
        cancels what the far end's audio left in the rows, on the GPU behind the repair and in front of the step.
        echo_delay: the echo-delay estimator beside the canceller (Streams.set_echo_delay; it needs echo=) - None / False: none;
        True: the defaults of the slot's input rate; a dict of conan_echo_delay_cfg's fields over them and of the follow rule's
        keywords lead, hyst, max_age (_lib.echo_delay_follow_keywords: 8 ms, 4 ms, 64 frames - choices).  feed(far=...) then runs
        the estimator in front of the canceller, and between calls the engine moves the canceller's delay where the rule
        (_lib.echo_delay_follow) says; echo_delays() reads the result.
        comfort: comfort noise in the closed activity gate
        (Streams.set_comfort; activity= beside it) - None / False: none; True: the defaults; a dict of set_comfort's keywords; the
        seed defaults to one derived from the slot's index.  chunk_comfort() reads the last call's levels.
        denoise: noise suppression of the input's log-mel frames (Streams.set_denoise) - None / False: none; True: the defaults for
        the default mel front-end (log10, vmin -6, eps 1e-6); a dict of _lib.denoise_cfg's keywords (a feed(mel=...) with another
        log base or floor names it there: natural_log, mel_vmin, eps).  The Emformer then sees the suppressed frames.
        tones: DTMF detection and regeneration (Streams.set_tones) - None / False: none; True: detect and regenerate with the
        defaults; a dict of set_tones's keywords (regenerate=False only detects).  chunk_tones() reads the last call's rows.
        eq: the source-side equaliser (Streams.set_input_eq) - None / False: none; a dict(sections=[...]) as out_eq's (start).  It
        filters the decoded, resampled samples in front of the leveller and the front-end: everything that reads the slot's audio
        sees ctx.eq of the source.
        There is no trim= here: silence trimming (infer_wav(trim=True)) moves audio forward over pauses it has seen whole, and a
        stream cannot drop time it has not heard yet; activity= is what a live call has in its place."""
        self._check_voice(ref_mel, voice)
        if isinstance(drift, (list, tuple)):
            raise ValueError("drift: one value for all slots here; open_slots and infer_wav_staggered take one per slot / utterance")
        self._drift_values(drift, len(self.slots))
        if isinstance(in_format, (list, tuple)) or isinstance(level, (list, tuple)):
            raise ValueError("in_format / level: one value for all slots here; open_slots and infer_wav_staggered take one per slot / utterance")
        values = self._host_checks(len(self.slots), voice, level=level, follow=follow, register=register, activity=activity, bypass=bypass,
                                   conceal=conceal, echo=echo, comfort=comfort, denoise=denoise, tones=tones, eq=eq)
        delays = self._echo_delay_values(echo_delay, echo, len(self.slots))
        self.start(ref_mel, ref_len, which=7 | 8, out_rate=out_rate, out_filter=out_filter, out_format=out_format, pitch=pitch, voice=voice,
                   out_level=out_level, watermark=watermark, out_eq=out_eq, drift=drift)
        self._set_rate(self.slots, in_rate, filter)
        self._set_drift(self.slots, self._drift_values(drift, len(self.slots)), inp=(in_rate, filter))
        self._set_format(self.slots, in_format, self.st.input_formats, self.st.set_input_format)
        for keyword in values:      # (pitch and out_level went in with start(), in front of the input rate)
            self._apply(keyword, self.slots, values[keyword], [in_rate] * len(self.slots))
        self._apply_echo_delay(self.slots, delays, [in_rate] * len(self.slots))

    @staticmethod
    def _values(keyword, value, n, what="slots", voice=None):
        """keyword= (one value or one per slot) -> per slot None (None / False: none) or the cfg of the feature's Streams setter
        (_accept).  Host only."""
        values = list(value) if isinstance(value, (list, tuple)) else [value] * n
        if len(values) != n:
            raise ValueError(f"{keyword}: {len(values)} values for {n} {what}")
        return [None if v is None or v is False else _accept(keyword, v, k, n, voice) for k, v in enumerate(values)]

    @classmethod
    def _host_checks(cls, n, voice=None, utterances=(), **given):
        """The host checks of the given per-slot keywords, before anything runs: keyword -> _values' list, in the order of
        _lib.SLOT_FEATURES.  utterances: the keywords whose n counts utterances in the error's text."""
        return {k: cls._values(k, given[k], n, "utterances" if k in utterances else "slots", voice) for k in _lib.SLOT_FEATURES if k in given}

    def _apply(self, keyword, slots, values, rates=None):
        """The slots' feature from _values' list, one setter call per slot, behind the slots' reset (states restart from their seeds at
        the first emitted chunk).  A feature with a Streams dict (level, pitch, out_level): a slot that never had one is left alone.
        The others: a stream-set that never used the feature gets no setter call at all; once used, None turns a slot off.  rates:
        the slots' input rates (None: the model rate), for the concealment's and the canceller's defaults.  A comfort seed defaults to
        _lib.comfort_seed(slot)."""
        f = _lib.SLOT_FEATURES[keyword]
        if not f.mirror:
            if all(v is None for v in values) and keyword not in self._used:
                return
            self._used.add(keyword)
        for k, (slot, v) in enumerate(zip(slots, values)):
            if v is None and f.mirror and int(slot) not in getattr(self.st, f.mirror):
                continue
            kw = {}
            if keyword in ("conceal", "echo"):
                v, kw = None if v is None else (v or True), dict(rate=rates[k])      # ({}: True, the defaults of the slot's rate)
            elif keyword == "comfort" and v is not None:
                v = dict(dict(seed=_lib.comfort_seed(slot)), **v)
            getattr(self.st, f.method)([slot], cfg=v, **kw)

    def _live(self, keyword, slots, *args, **kw):
        """A live setter: the feature's Streams setter on `slots` (all slots by default), which counts as use of the feature."""
        f = _lib.SLOT_FEATURES[keyword]
        if not f.mirror:
            self._used.add(keyword)
        getattr(self.st, f.method)(self.slots if slots is None else slots, *args, **kw)

    @staticmethod
    def _echo_delay_values(echo_delay, echo, n, what="slots"):
        """echo_delay= (one value or one per slot) -> per slot None (None / False: none) or a dict of conan_echo_delay_cfg's fields
        and the follow rule's keywords.  A slot with one needs echo=: the estimate steers the canceller's delay.  Host only."""
        values, echoes = _per_slot(echo_delay, n), _per_slot(echo, n)
        if len(values) != n:
            raise ValueError(f"echo_delay: {len(values)} values for {n} {what}")
        known = set(_lib._ECHO_DELAY_FIELDS) | set(_FOLLOW_KEYS)
        out = []
        for k, v in enumerate(values):
            if v is None or v is False:
                out.append(None)
                continue
            if k >= len(echoes) or echoes[k] is None or echoes[k] is False:
                raise ValueError("echo_delay: the estimate steers the canceller's delay and needs echo= (True, or conan_echo_cfg's fields)")
            if isinstance(v, _lib.EchoDelayCfg):
                v = _lib.echo_delay_keywords(v)
            elif v is True:
                v = {}
            elif not isinstance(v, dict):
                raise ValueError(f"echo_delay: {v!r} (True, a dict of conan_echo_delay_cfg's fields and lead / hyst / max_age, an _lib.EchoDelayCfg or None)")
            if set(v) - known:
                raise ValueError(f"echo_delay: unknown fields {sorted(set(v) - known)}")
            out.append(dict(v))
        return out

    def _apply_echo_delay(self, slots, values, rates, live=False):
        """The slots' estimator from _echo_delay_values' list, behind the slots' reset.  A stream-set that never used it gets no
        setter call at all; once used, None turns a slot off.  rates: the slots' input rates (None: the model rate), for the
        defaults.  live: a change between calls - an enabled slot keeps its last report."""
        if all(v is None for v in values) and not self._ed.used:
            return
        self._ed.used = True
        if self._ed.pending is not None and not live:      # (a report of the slots' earlier utterances says nothing about the new ones)
            self._ed.pending[0][:] = [None if s in slots else s for s in self._ed.pending[0]]
        for slot, v, rate in zip(slots, values, rates):
            rate = int(rate or self.st.model_rate)
            if v is None:
                self.st.set_echo_delay([slot], None)
                self._ed.follow.pop(slot, None)
                self._ed.last.pop(slot, None)
                continue
            self.st.set_echo_delay([slot], {k: x for k, x in v.items() if k not in _FOLLOW_KEYS} or True, rate=rate)
            self._ed.follow[slot] = dict(_lib.echo_delay_follow_keywords(rate), **{k: int(v[k]) for k in _FOLLOW_KEYS if k in v})
            if not live or slot not in self._ed.last:
                self._ed.last[slot] = (-1, 0)

    def set_echo_delay(self, slots=None, cfg=True, rate=None, **kw):
        """A live change of the slots' echo-delay estimator (all slots by default) between feed / feed_ragged calls, also
        mid-utterance: start_wav's echo_delay= values, keywords on top (cfg=None turns it off; an enabled slot keeps its state, and a
        changed n_lags the sums that still exist).  rate: the slots' input rate, for the defaults (None: the model rate)."""
        slots = self.slots if slots is None else list(slots)
        v = self._echo_delay_values(cfg, True, 1)[0]
        self._follow_pending()
        self._apply_echo_delay(slots, [None if v is None else dict(v, **kw)] * len(slots), [rate] * len(slots), live=True)

    def _far_report(self, slots):
        """The report tensor of a far= call: int64 [n, 6] on the device when a slot of the call follows its estimate, else None."""
        if not any(s in self._ed.follow for s in slots):
            return None
        return torch.zeros(len(slots), 6, dtype=torch.int64, device=self.st.dev)

    def _note_report(self, slots, samples, rep):
        """The call's report starts for the host (pinned, behind the estimator on the current stream); _follow_pending reads it."""
        host = torch.empty(tuple(rep.shape), dtype=rep.dtype, pin_memory=True)
        host.copy_(rep, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._ed.pending = ([s if m > 0 else None for s, m in zip(slots, samples)], host, ev, rep)

    def _follow_pending(self):
        """The follow rule on the last far= call's report, between calls: it waits for that call's estimator launch - work on the
        caller's stream in front of the call's step, not the pipelined steps themselves - and moves a canceller's delay
        (Streams.set_echo, fields only: the canceller's own guard deals with the stale weights) where the rule says."""
        if self._ed.pending is None:
            return
        slots, host, ev, _ = self._ed.pending
        self._ed.pending = None
        ev.synchronize()
        for slot, row in zip(slots, host.tolist()):
            f = self._ed.follow.get(slot)
            if slot is None or f is None:      # (a row without samples reports zeros, not an estimate)
                continue
            self._ed.last[slot] = (row[0], row[1])
            cfg = self.st.echo_cfg([slot])[0]
            d = None if cfg is None else _lib.echo_delay_follow(row[0], row[1], cfg["delay"], **f)
            if d is not None:
                self.st.set_echo([slot], dict(cfg, delay=d))

    def echo_delays(self, slots=None):
        """Per slot (all slots by default) (est, age, delay in force): the estimator's confirmed lag in samples (-1: none yet) and
        its age in frames as of the last far= call, and the canceller's bulk delay after the follow rule has seen them (None for a
        slot without a canceller).  It waits for the last call's report."""
        self._follow_pending()
        out = []
        for slot in (self.slots if slots is None else slots):
            cfg = self.st.echo_cfg([slot])[0]
            out.append(self._ed.last.get(slot, (-1, 0)) + (None if cfg is None else cfg["delay"],))
        return out

    def set_bypass(self, slots=None, cfg=True, **kw):
        """A live change of the slots' bypass (all slots by default) between feed / feed_ragged calls, also mid-utterance and with
        pipelined steps in flight: Streams.set_bypass's arguments (cfg=None turns it off; without reseed=True an enabled slot keeps
        its levels and slews to the new targets - the toggle).  In force from the next emitted chunk."""
        self._live("bypass", slots, cfg, **kw)

    def set_comfort(self, slots=None, cfg=True, **kw):
        """A live change of the slots' comfort noise (all slots by default) between feed / feed_ragged calls, also mid-utterance and
        with pipelined steps in flight: Streams.set_comfort's arguments (cfg=None turns it off; without reseed=True an enabled slot
        keeps its level).  In force from the next emitted chunk."""
        self._live("comfort", slots, cfg, **kw)

    def chunk_comfort(self):
        """The frame-end comfort levels of the last feed / feed_ragged call (Streams.step_wav_comfort; joins pipelined work): [n, seg]
        int32 in the call's row order, zeros for rows without the feature and past a row's frames; _lib.comfort_dbov(level) is the
        RFC 3389 noise level byte of a frame."""
        return self.st.step_wav_comfort()

    def set_tones(self, slots=None, cfg=True, **kw):
        """A live change of the slots' DTMF detection and regeneration (all slots by default) between feed / feed_ragged calls, also
        mid-utterance and with pipelined steps in flight: Streams.set_tones's arguments (cfg=None turns it off; without reseed=True
        an enabled slot keeps its state).  In force from the next emitted chunk."""
        self._live("tones", slots, cfg, **kw)

    def chunk_tones(self):
        """The tone rows of the last feed / feed_ragged call (Streams.step_wav_tones; joins pipelined work): (digit, sound, level),
        each [n, seg] int32 in the call's row order; digit is the confirmed key of each 20 ms frame (-1: none) and
        _lib.tone_events(rows) lists the presses a host sends as RFC 4733 events."""
        return self.st.step_wav_tones()

    def set_eq(self, slots=None, cfg=True, seed=None, **kw):
        """A live change of the slots' source-side equaliser (all slots by default) between feed / feed_ragged calls, also
        mid-utterance and with pipelined steps in flight: Streams.set_input_eq's arguments (sections=[...]; cfg=None turns it off).
        An enabled slot's pending tail closes with the old coefficients and the sections keep their state words: the change does
        not click.  In force from the next call."""
        self._live("eq", slots, cfg, seed=seed, **kw)

    def set_out_eq(self, slots=None, cfg=True, seed=None, **kw):
        """A live change of the slots' output equaliser - the tone control - as set_eq: Streams.set_output_eq's arguments.  In force
        from the next vocoder step."""
        self._live("out_eq", slots, cfg, seed=seed, **kw)

    def set_denoise(self, slots=None, cfg=True, **kw):
        """A live change of the slots' noise suppression (all slots by default) between feed / feed_ragged calls, also mid-utterance
        and with pipelined steps in flight: Streams.set_denoise's arguments (cfg=None turns it off; without reseed=True an enabled
        slot keeps its noise floor).  In force from the slot's next frame."""
        self._live("denoise", slots, cfg, **kw)

    def set_conceal(self, slots=None, cfg=True, **kw):
        """A live change of the slots' loss concealment (all slots by default) between feed / feed_ragged calls, also mid-utterance:
        Streams.set_conceal's arguments (cfg=None turns it off; an enabled slot keeps its state)."""
        self._live("conceal", slots, cfg, **kw)

    def set_echo(self, slots=None, cfg=True, **kw):
        """A live change of the slots' echo canceller (all slots by default) between feed / feed_ragged calls, also mid-utterance:
        Streams.set_echo's arguments (cfg=None turns it off; an enabled slot keeps its state, and a changed taps the weights that
        still exist)."""
        self._live("echo", slots, cfg, **kw)

    def _lost_rows(self, slots, lost, pos, counts):
        """The flags of one call's rows cut from whole-utterance flags: row i takes lost[i] from sample position pos[i] on, counts[i]
        samples -> int32 [n, packets] (zeros for a row without flags or without the feature), or None when no row has any."""
        cfgs = self.st.conceal_cfg(slots)
        rows = []
        for c, fl, p, m in zip(cfgs, lost, pos, counts):
            if fl is None or c is None or m == 0:
                rows.append(None)
                continue
            if p % c["packet"]:
                raise ValueError(f"lost: a call begins at sample {p}, off the packets of {c['packet']} samples: the calls' rows must be whole packets long")
            rows.append(fl[p // c["packet"]:(p + m + c["packet"] - 1) // c["packet"]].to(torch.int32))
        if all(r is None for r in rows):
            return None
        width = max(r.shape[0] for r in rows if r is not None)
        out = torch.zeros(len(rows), width, dtype=torch.int32, device=self.st.dev)
        for i, r in enumerate(rows):
            if r is not None:
                out[i, :r.shape[0]] = r
        return out

    def chunk_bypass(self):
        """The frame-end wet and effective dry levels of the last feed / feed_ragged call (Streams.step_wav_bypass; joins pipelined
        work): (wet [n, seg], dry [n, seg]) int32 in the call's row order, zeros for rows without the feature and past a row's frames."""
        return self.st.step_wav_bypass()

    def set_activity(self, slots=None, cfg=True, **kw):
        """A live change of the slots' activity detector (all slots by default) between feed / feed_ragged calls, also mid-utterance
        and with pipelined steps in flight: Streams.set_activity's arguments (cfg=None turns it off; without reseed=True an enabled
        slot keeps its state).  In force from the next emitted chunk."""
        self._live("activity", slots, cfg, **kw)

    def chunk_activity(self):
        """The flags and frame-end gate levels of the last feed / feed_ragged call (Streams.step_wav_activity; joins pipelined work):
        (act [n, seg], level [n, seg]) int32 in the call's row order, zeros for rows without the detector and past a row's frames."""
        return self.st.step_wav_activity()

    def set_pitch_register(self, slots=None, **kw):
        """A live change of the slots' register matching (all slots by default) between feed / feed_ragged calls, also mid-utterance
        and with pipelined steps in flight: Streams.set_pitch_register's keywords (cfg=None turns it off; without reseed=True an
        enabled slot keeps its estimate: the voice change in the middle of a call).  In force from the next emitted chunk."""
        self._live("register", slots, **kw)

    def set_pitch_follow(self, slots=None, cfg=True, **kw):
        """A live change of the slots' source-pitch following (all slots by default) between feed / feed_ragged calls, also
        mid-utterance and with pipelined steps in flight: Streams.set_pitch_follow's arguments (cfg=None turns it off).  In force
        from the next emitted chunk."""
        self._live("follow", slots, cfg, **kw)

    def set_output_level(self, slots=None, cfg=True, seed=None, **kw):
        """The slots' output leveller (all slots by default) between utterances, or mid-utterance with seed= (a hand-over):
        Streams.set_output_level's arguments (cfg=None turns it off).  Joins pipelined steps in flight."""
        self._live("out_level", slots, cfg, seed=seed, **kw)

    def set_watermark(self, slots=None, cfg=True, seed=None, **kw):
        """A live change of the slots' output watermark (all slots by default) between calls, also mid-utterance and with pipelined
        steps in flight: Streams.set_watermark's arguments (cfg=None turns it off; without reseed=True an enabled slot keeps its
        position and envelope; seed= is a hand-over).  In force from the next vocoder step."""
        self._live("watermark", slots, cfg, seed=seed, **kw)

    def set_pitch(self, slots=None, **kw):
        """A live change of the slots' pitch control (all slots by default) between feed / feed_ragged calls, also mid-utterance and
        with pipelined steps in flight: Streams.set_pitch's keywords; no keyword at all turns it off.  In force from the next call."""
        self._live("pitch", slots, dict(kw) if kw else None)

    @staticmethod
    def _set_format(slots, fmt, table, setter):
        """The slots' sample format (None: float32), one value or one per slot.  Slots that never had another format are left alone."""
        for f, group in _by_value(slots, _per_slot(fmt, len(slots))):
            group = [s for s in group if (f or "f32") != "f32" or s in table]
            if group:
                setter(group, f or "f32")

    def _set_out_rate(self, slots, out_rate, out_filter):
        """The slots' output rate (None: the model rate), one value or one per slot, and the stream-set's output stride: wide enough
        for a full chunk of the fastest slot.  Slots that never had another rate are left alone."""
        st = self.st
        for r, group in _by_value(slots, _per_slot(out_rate, len(slots))):
            group = [s for s in group if r is not None or s in st.output_rates]
            if group:
                if self.ctx.cfg.voc_upsample == 2 and r is not None:
                    raise ValueError("out_rate with an upsample 'nn' vocoder: run Streams.hifigan_step over the mel prefix and Streams.flush_output instead")
                st.set_output_rate(group, r or st.model_rate, **(out_filter or {}))
        self._fit_output_ld()

    def _fit_output_ld(self):
        """The stream-set's output stride: wide enough for a full chunk of the fastest slot (0 without output rates)."""
        st = self.st
        L = self.seg * self.ctx.hop
        ld = max([L] + [-(-L * r // st.model_rate) + 2 for r in st.output_rates.values()]) if st.output_rates else 0
        # (a drift slot's sink may run fast by _lib.DRIFT_MAX_PPB: its chunk is that much longer)
        ld = max([ld] + [-(-L * st.output_rates[s] * (10 ** 9 + _lib.DRIFT_MAX_PPB) // (st.model_rate * 10 ** 9)) + 3 for s in getattr(st, "output_drifts", ())])      # (a Streams stand-in that predates drift has no such set)
        if ld != st.output_ld:
            st.set_output_ld(ld)

    @staticmethod
    def _drift_values(drift, n, what="slots"):
        """drift= (ppm: one value or one per slot; None / False: none) -> per slot None or the ppm as a float.  Host only."""
        values = _per_slot(drift, n)
        if len(values) != n:
            raise ValueError(f"drift: {len(values)} values for {n} {what}")
        out = []
        for v in values:
            if v is None or v is False:
                out.append(None)
                continue
            if isinstance(v, bool) or not isinstance(v, (int, float)):
                raise ValueError(f"drift: {v!r} (the far device's clock error in ppm, > 0: it runs fast; or None)")
            _lib.drift_ppb(v)      # (the range check)
            out.append(float(v))
        return out

    def _set_drift(self, slots, values, out=None, inp=None):
        """The slots' drift resamplers from _drift_values' list, behind the rate setters (which remove them).  out = (out_rate,
        out_filter): the output side at the slots' output rate; inp = (in_rate, filter): the input side at their input rate
        (None in either: the model rate)."""
        st = self.st
        if all(v is None for v in values):
            return
        outs, ins = _per_slot(out[0] if out else None, len(slots)), _per_slot(inp[0] if inp else None, len(slots))
        for slot, v, ro, ri in zip(slots, values, outs, ins):
            if v is None:
                continue
            if out is not None:
                st.set_output_drift([slot], v, rate=ro or st.model_rate, **(out[1] or {}))
            if inp is not None:
                st.set_input_drift([slot], v, rate=ri or st.model_rate, **(inp[1] or {}))
        self._fit_output_ld()

    def set_drift(self, slots=None, ppm=0.0):
        """A live change of the slots' clock drift (all slots by default) between feed / feed_ragged / step calls, on both sides
        where the slot has a drift resampler (start / start_wav / open_slots(drift=...)): in force from the slot's next output."""
        st = self.st
        slots = [int(s) for s in (self.slots if slots is None else slots)]
        ins, outs = [s for s in slots if s in st.input_drifts], [s for s in slots if s in st.output_drifts]
        if len(set(ins) | set(outs)) != len(slots):
            raise ValueError("set_drift: a slot without drift (give drift= when the utterance starts)")
        _lib.drift_ppb(ppm)
        if ins:
            st.set_input_drift(ins, ppm)
        if outs:
            st.set_output_drift(outs, ppm)

    def export_streams(self, slots):
        """The streams in `slots` as a runtime.SlotSnapshot (Streams.export_slots): park them, move them to another engine, rank or
        process, or fork them.  The slots are left as they are."""
        return self.st.export_slots(slots)

    def import_streams(self, slots, snap):
        """Continue the streams of `snap` in `slots` of this engine (Streams.import_slots): feed, feed_ragged and finish go on where
        the exporting engine stopped.  Rates, formats, the input leveller and the pitch control travel with the streams; the output
        stride follows them."""
        st = self.st
        st.import_slots(slots, snap)
        self._fit_output_ld()

    def finish(self, slots=None):
        """End of utterance on a stream-set with output rates: the slots' remaining output samples (Streams.flush_output), one 1-D
        tensor per slot (empty for a slot without a rate)."""
        return self.st.flush_output(self.slots if slots is None else slots)

    @staticmethod
    def _rows(w):
        """A step's wav rows (a list on a stream-set with output rates; all slots of these calls deliver the same count) as [B, count]."""
        return torch.stack(list(w)) if isinstance(w, (list, tuple)) else w

    def _set_rate(self, slots, in_rate, filter):
        """The slots' input rate (None: the model rate).  A stream-set that never had another rate is left alone."""
        if in_rate is None and not self.st.input_rate_set:
            return
        self.st.set_input_rate(slots, in_rate or self.st.model_rate, **filter)

    def _in_len(self, in_rate):
        """Input samples of one non-final feed at `in_rate` (80 ms: seg*hop at the model rate)."""
        L = self.seg * self.ctx.hop
        return L if in_rate is None else L * int(in_rate) // self.st.model_rate

    @torch.no_grad()
    def feed(self, wav_chunk, final=False, pipelined=False, mel=None, lost=None, far=None, echo_stats=None):
        """Streaming waveform input (conan_step_wav): wav_chunk [B, seg*hop] (cuda; 0 .. seg*hop samples when final; at an input
        rate set by start_wav, seg*hop*in_rate/model_rate) ->
        (wav [B, emit*hop], mel [B, emit, 80], codes [B, emit]) of the chunk this call emitted (emit = 0 on the first call: one
        chunk of algorithmic latency).  After final=True keep calling feed(empty, final=True) until it returns 0 frames.
        pipelined: conan_step_wav_async - the tensors are complete after self.st.join().
        The reference's whole-utterance loud_norm still cannot run here: that loudness is a property of the whole utterance, which a
        streaming call has not seen yet (infer_wav(loud_norm=True) normalises an utterance it holds whole).  What can stream is the
        input leveller, start_wav(level=...): a causal BS.1770 meter of the audio so far steers a ramped gain towards the same
        target, on the GPU in front of the front-end, without look-ahead or added latency (Context.level is its whole-signal form).
        Silence trimming (infer_wav(trim=True)) cannot run here either: a live call cannot drop time.  What serves there is the
        activity detector, start_wav(activity=...): per-frame flags and an output gate, and a server that recorded the call can cut
        the recording afterwards with those flags (Context.trim_silence(flags=...)) without detecting again.
        lost: [B, packets] integer or bool (cuda), non-zero = that packet of the row never arrived: the slots with start_wav(conceal=...)
        repair them on the GPU in front of the step (Streams.conceal; packets count from the start of the row).  The chunk is
        copied first: the caller's tensor keeps its samples.
        far: [B, samples] in wav_chunk's dtype, what went to each caller's earpiece while the row was recorded: the slots with
        start_wav(echo=...) cancel its echo on the GPU behind the repair and in front of the step (Streams.echo).  The chunk is
        copied first here too.  Slots with start_wav(echo_delay=...) run their estimator in front of the canceller, and the call
        first applies the follow rule to the previous far= call's report (_follow_pending).  echo_stats: Streams.echo's stats tensor
        for this call's rows (int64 [B, 4] on the device) or None."""
        fn = self.st.step_wav_async if pipelined else self.st.step_wav
        st = self.st
        if lost is not None:
            wav_chunk, fn = wav_chunk.clone(), functools.partial(fn, lost=lost)
        rep = None
        if far is not None:
            self._follow_pending()
            rep = self._far_report(self.slots)
            wav_chunk, fn = (wav_chunk if lost is not None else wav_chunk.clone()), functools.partial(fn, far=far, **({} if rep is None else dict(echo_delay_report=rep)), **({} if echo_stats is None else dict(echo_stats=echo_stats)))
        if not (st.output_ld or st.output_formats):
            emit, c, m, w = fn(self.slots, wav_chunk, final=final, mel=mel)
            if rep is not None:
                self._note_report(self.slots, [wav_chunk.shape[1]] * len(self.slots), rep)
            return w, m, c[:, :emit]
        # output rates / formats: rows at the stride in force, all slots at one position, rate and format here (a view: pipelined
        # steps complete at join())
        buf = torch.empty(len(self.slots), st.output_ld or self.seg * self.ctx.hop, device=wav_chunk.device)
        emit, c, m, _ = fn(self.slots, wav_chunk, final=final, mel=mel, wav_out=buf)
        if rep is not None:
            self._note_report(self.slots, [wav_chunk.shape[1]] * len(self.slots), rep)
        w = st.wav_block(buf, self.slots, st.output_samples()[0] if emit else 0, st.output_ld or (emit or self.seg) * self.ctx.hop)
        return w, m, c[:, :emit]

    @staticmethod
    def _check_lost(lost, conceal, loud_norm, trim):
        """lost= of the whole-utterance calls: it needs conceal=, and cannot go with loud_norm or trim.  Host only."""
        if lost is None:
            return
        if conceal is None or conceal is False:
            raise ValueError("lost: the flags need conceal= (True, or conan_conceal_cfg's fields)")
        if loud_norm or (trim is not None and trim is not False):
            raise ValueError("lost: loud_norm and trim hold the utterance whole, in front of the streaming repair: repair it whole first "
                             "(Context.conceal) and pass the repaired utterance without lost=")

    @staticmethod
    def _check_far(far, echo, loud_norm, trim):
        """far= of the whole-utterance calls: it needs echo=, and cannot go with loud_norm or trim.  Host only."""
        if far is None:
            return
        if echo is None or echo is False:
            raise ValueError("far: the far end needs echo= (True, or conan_echo_cfg's fields)")
        if loud_norm or (trim is not None and trim is not False):
            raise ValueError("far: loud_norm and trim hold the utterance whole, in front of the streaming canceller: cancel it whole first "
                             "(Context.echo) and pass the cancelled utterance without far=")

    @torch.no_grad()
    def _loud_norm(self, wav, in_rate, in_format):
        """The reference's loud_norm (Context.loud_norm: -22 LUFS, peak limit) of whole float32 utterances [..., N] at their input rate."""
        if in_format not in (None, "f32"):
            raise ValueError("loud_norm takes float32 rows: decode the utterance first (Context.convert_samples) or pass in_format=None")
        return self.ctx.loud_norm(wav, in_rate or self.st.model_rate)

    @staticmethod
    def _trim_keywords(trim):
        """trim= of the whole-utterance calls -> None (off) or Context.trim_silence's keywords: False / None, True, or a dict."""
        if trim is None or trim is False:
            return None
        if trim is True:
            return {}
        if isinstance(trim, dict):
            return dict(trim)
        raise ValueError(f"trim: {trim!r} is neither True, False nor a dict of Context.trim_silence's keywords")

    @torch.no_grad()
    def _trim(self, wav, in_rate, in_format, kw):
        """Context.trim_silence of whole float32 utterances [..., N] at their input rate -> (rows, kept samples per row)."""
        if in_format not in (None, "f32"):
            raise ValueError("trim takes float32 rows: decode the utterance first (Context.convert_samples) or pass in_format=None")
        rate = int(in_rate or self.st.model_rate)
        if rate % 50:
            raise ValueError(f"trim: the input rate {rate} must be a multiple of 50 (the detector's frames are 20 ms)")
        out, kept = self.ctx.trim_silence(wav, hop_size=rate // 50, **kw)
        if int(np.min(kept)) < 1:
            raise ValueError("trim: an utterance has no activity, nothing is left of it")
        return out, kept

    @torch.no_grad()
    def infer_wav(self, src_wav, ref_mel, ref_len=None, pipelined=True, mel=None, in_rate=None, out_rate=None, out_filter=None, in_format=None,
                  out_format=None, loud_norm=False, trim=False, level=None, pitch=None, voice=None, follow=None, register=None, activity=None,
                  activity_log=None, bypass=None, out_level=None, conceal=None, lost=None, echo=None, far=None, echo_delay=None, comfort=None, denoise=None, watermark=None, tones=None, eq=None, out_eq=None,
                  drift=None, **filter):
        """drift: the far device's clock error in ppm on both sides of the slots (start_wav), one value: the results are those of
        infer_wav(ctx.resample_drift(x, in_rate, model_rate, drift), ...), x the decoded utterance, and the returned wav is
        ctx.resample_drift(model-rate wav, model_rate, out_rate, drift, side='sink'), bit for bit.
        src_wav [B, N] (cuda), ref_mel [B, Tr, 80] (or None with voice = (bank, ids): start) -> (wav, mel, codes) of the utterance fed 80 ms at a time and drained:
        the results of infer(ctx.wav2mel(src_wav), ref_mel) bit for bit.  in_rate (+ filter keywords): src_wav's sample rate,
        resampled on the GPU; the results are those of infer_wav(ctx.resample(src_wav, in_rate, **filter), ref_mel) bit for bit.
        out_rate (+ out_filter): the returned wav is the whole utterance at that rate, ctx.resample of the model-rate wav bit for bit.
        in_format: src_wav's sample format (int16 / uint8 samples; the results are those of the decoded floats, ctx.convert_samples,
        bit for bit); out_format: the returned wav's format (ctx.convert_samples of the float wav bit for bit).
        loud_norm: each whole source utterance is loudness-normalised at its input rate before it is fed (the reference's loud_norm;
        float32 rows only); the results are those of infer_wav(ctx.loud_norm(src_wav, rate), ...) bit for bit.
        trim: True, or a dict of Context.trim_silence's keywords: the long pauses are cut out of each whole utterance at its input rate
        (a multiple of 50; float32 rows only) before loud_norm and before anything is fed - every trimmed second is a second of
        Emformer, decoder and vocoder work not done.  The rows of one call are fed together, so they come back as long as the longest
        kept one, the shorter ones with zeros behind their audio: the results are those of infer_wav(ctx.trim_silence(src_wav,
        hop_size=rate // 50)[0], ...) bit for bit (infer_wav_staggered trims every utterance to its own length).
        level: the streaming input leveller (start_wav); the results are those of infer_wav(ctx.level(x, **level), ...) bit for bit,
        x = the decoded, resampled utterance.  pitch: the slots' pitch control in the decoder step (start).  follow: source-pitch
        following (start_wav): the decoder steps take ctx.f0 of the samples the front-end reads instead of the predictor's contour.
        register: register matching of the followed contour (start_wav): the steps take ctx.f0_register of that contour.
        activity: the source-activity detector (start_wav): ctx.activity of the samples the front-end reads, and with the gate the
        returned wav is ctx.activity_gate of the ungated one, bit for bit.  activity_log: a list that receives (act [B, emit],
        level [B, emit]) per emitted chunk (chunk_activity after each call, which joins pipelined work).
        bypass: the wet/dry mix (start_wav): the returned wav is ctx.bypass_mix of the unmixed one and of the samples the front-end
        reads, bit for bit.  out_level: the output leveller (start): the returned model-rate wav is ctx.level of the unlevelled
        one, bit for bit, and gate, mix, output rate and format apply to the levelled audio.
        conceal + lost: loss concealment (start_wav) with lost [B, packets], the flags of the whole utterance: the results are those
        of infer_wav(ctx.conceal(src_wav, lost, cfg, in_format), ...) bit for bit.  Not with loud_norm or trim, which hold the
        utterance whole: repair it whole first (Context.conceal).  denoise: the noise suppressor (start_wav): the results are those of
        infer(ctx.mel_denoise(ctx.wav2mel(x)), ...) bit for bit, x = the samples the front-end reads.  watermark: the output watermark
        (start): the returned model-rate wav is ctx.watermark_embed of the unmarked one, bit for bit.
        echo + far: echo cancellation (start_wav) with far [B, N], the far end of the whole utterance in src_wav's format: the
        results are those of infer_wav(ctx.echo(src_wav, far, cfg, in_format), ...) bit for bit.  Not with loud_norm or trim.
        echo_delay: the estimator beside the canceller (start_wav): the canceller's delay then follows the estimate from call to
        call, so the results are those of the whole-signal canceller only until the first change."""
        self._check_voice(ref_mel, voice)
        self._host_checks(len(self.slots), voice, level=level, pitch=pitch, follow=follow, register=register, activity=activity, bypass=bypass,
                          conceal=conceal, echo=echo, comfort=comfort, denoise=denoise, out_level=out_level, watermark=watermark, tones=tones, eq=eq, out_eq=out_eq)      # (before anything runs)
        self._check_lost(lost, conceal, loud_norm, trim)
        self._check_far(far, echo, loud_norm, trim)
        self._echo_delay_values(echo_delay, echo, len(self.slots))
        if far is not None and tuple(far.shape) != tuple(src_wav.shape):
            raise ValueError(f"far: {tuple(far.shape)} for a src_wav of {tuple(src_wav.shape)}: the far end is the utterance's, sample for sample")
        trim = self._trim_keywords(trim)
        if trim is not None:
            src_wav = self._trim(src_wav, in_rate, in_format, trim)[0]
        if loud_norm:
            src_wav = self._loud_norm(src_wav, in_rate, in_format)
        self.start_wav(ref_mel, ref_len, in_rate, out_rate=out_rate, out_filter=out_filter, in_format=in_format, out_format=out_format, level=level,
                       pitch=pitch, voice=voice, follow=follow, register=register, activity=activity, bypass=bypass, out_level=out_level, conceal=conceal,
                       echo=echo, echo_delay=echo_delay, comfort=comfort, denoise=denoise, watermark=watermark, tones=tones, eq=eq, out_eq=out_eq, drift=drift, **filter)
        B, N = src_wav.shape
        L = self._in_len(in_rate)
        last = (N - 1) // L * L                       # the final call takes the remaining 1 .. L samples
        empty = src_wav.new_zeros(B, 0)
        cut = lambda p, m: None if lost is None else self._lost_rows(self.slots, list(lost), [p] * B, [m] * B)      # noqa: E731
        wavs, mels, codes = [], [], []
        pos, final = 0, False
        while True:
            if pos < last:
                w, m, c = self.feed(src_wav[:, pos:pos + L], pipelined=pipelined, mel=mel, lost=cut(pos, L), far=None if far is None else far[:, pos:pos + L])
                pos += L
            else:
                w, m, c = self.feed(src_wav[:, pos:] if not final else empty, final=True, pipelined=pipelined, mel=mel,
                                    lost=None if final else cut(pos, N - pos), far=None if final or far is None else far[:, pos:])
                pos, done, final = N, final and m.shape[1] == 0, True
                if done:
                    break
            if m.shape[1]:
                wavs.append(w)
                mels.append(m)
                codes.append(c)
                if activity_log is not None:
                    a, l = self.chunk_activity()
                    activity_log.append((a[:, :m.shape[1]].clone(), l[:, :m.shape[1]].clone()))
        if pipelined:
            self.st.join()
        if self.st.output_rates:
            wavs.append(torch.stack(self.finish()))
        return torch.cat(wavs, 1), torch.cat(mels, 1), torch.cat(codes, 1)

    def open_slots(self, slots, ref_mel, ref_len=None, in_rate=None, out_rate=None, out_filter=None, in_format=None, out_format=None, level=None,
                   pitch=None, voice=None, follow=None, register=None, activity=None, bypass=None, out_level=None, conceal=None, echo=None, echo_delay=None, comfort=None, denoise=None, watermark=None, tones=None, eq=None, out_eq=None,
                   drift=None, **filter):
        """drift: the slots' clock drift in ppm (start_wav), one value or a list with one per slot, on both sides of each slot.
        Start new utterances in `slots` while the other slots are mid-utterance: a full reset (models and streaming front-end,
        which = 7 | 8) and their references (ref_mel [len(slots), Tr, 80]).  in_rate: the slots' input rate (None: the model
        rate), one value or one per slot; filter: Context.resample's filter keywords.  out_rate / out_filter: the slots' output rate
        (None: the model rate), one value or one per slot.  in_format / out_format: the slots' sample formats (None: float32), one
        value or one per slot.  level: the slots' input leveller (start_wav), one value or a list with one per slot.  pitch: the
        slots' pitch control (start), one value or a list with one per slot.  voice: (bank, ids) - enrolled voices, one id per slot, in
        place of ref_mel (then None): one launch instead of a style pass per slot.  follow: the slots' source-pitch following
        (start_wav), one value or a list with one per slot.  register: the slots' register matching (start_wav), one value or a list
        with one per slot.  activity: the slots' activity detector (start_wav), one value or a list with one per slot.  bypass: the
        slots' wet/dry mix (start_wav), one value or a list with one per slot.  out_level: the slots' output leveller (start), one
        value or a list with one per slot.  conceal: the slots' loss concealment (start_wav), one value or a list with one per slot.
        denoise: the slots' noise suppression (start_wav), one value or a list with one per slot.
        watermark: the slots' output watermark (start), one value or a list with one per slot.
        echo_delay: the slots' echo-delay estimator (start_wav; it needs echo= on the same slot), one value or a list with one per slot.
        No trim=, as in start_wav: the slots stream, and a stream cannot drop time (infer_wav_staggered(trim=True) trims utterances
        it holds whole)."""
        self._check_voice(ref_mel, voice)
        drifts = self._drift_values(drift, len(slots))
        values = self._host_checks(len(slots), voice, level=level, pitch=pitch, follow=follow, register=register, activity=activity, bypass=bypass,
                                   conceal=conceal, echo=echo, comfort=comfort, denoise=denoise, out_level=out_level, watermark=watermark, tones=tones, eq=eq, out_eq=out_eq)
        delays = self._echo_delay_values(echo_delay, echo, len(slots))
        self.st.reset(slots, which=7 | 8)
        self._reference(slots, ref_mel, ref_len, voice)
        self._set_out_rate(slots, out_rate, out_filter)
        self._set_format(slots, in_format, self.st.input_formats, self.st.set_input_format)
        self._set_format(slots, out_format, self.st.output_formats, self.st.set_output_format)
        for r, group in _by_value(slots, _per_slot(in_rate, len(slots))):
            self._set_rate(group, r, filter)
        self._set_drift(slots, drifts, out=(out_rate, out_filter), inp=(in_rate, filter))
        for keyword in values:      # (the order of _lib.SLOT_FEATURES: pitch behind level, out_level and watermark last)
            self._apply(keyword, slots, values[keyword], _per_slot(in_rate, len(slots)))
        self._apply_echo_delay(slots, delays, _per_slot(in_rate, len(slots)))

    @torch.no_grad()
    def feed_ragged(self, slots, wav, samples, final, pipelined=False, mel=None, lost=None, far=None, echo_stats=None):
        """Streaming waveform input for slots at different positions of their utterances (conan_step_wav_ragged): slot i takes the
        first samples[i] samples of wav row i (wav [n, <= seg*hop] cuda, or a list of 1-D rows, each in its slot's input format's
        dtype) with its own final flag; the rules per slot are feed()'s.
        -> one (wav [emit*hop], mel [emit, 80], codes [emit]) per slot, of the chunk it emitted (emit = 0: empty).
        pipelined: conan_step_wav_ragged_async - the tensors are complete after self.st.join().
        As in feed(), the reference's whole-utterance loud_norm cannot run here (infer_wav_staggered(loud_norm=True) holds the
        utterances whole); open_slots(level=...) gives a slot the causal input leveller, which can, and a call may mix levelled
        and unlevelled slots.  lost: [n, packets] integer or bool (cuda), as feed()'s: the rows of slots with the concealment are
        repaired in front of the step, the others keep their bytes.  far: the rows' far end in wav's form (feed()'s): the rows
        of slots with the canceller are cancelled behind the repair, the others keep their bytes.  echo_stats: as feed()'s."""
        fn = self.st.step_wav_ragged_async if pipelined else self.st.step_wav_ragged
        if (lost is not None or far is not None) and isinstance(wav, torch.Tensor):
            wav = wav.clone()      # (a list of rows is packed into a buffer of its own anyway)
        rep = None
        if far is not None:
            self._follow_pending()
            rep = self._far_report(slots)
        emit, c, m, w = fn(slots, wav, samples, final, mel=mel, lost=lost, far=far, **({} if rep is None else dict(echo_delay_report=rep)),
                        **({} if echo_stats is None else dict(echo_stats=echo_stats)))
        if rep is not None:
            self._note_report(slots, samples, rep)
        counts = self.st.output_samples()        # (emit * hop for a slot without an output rate)
        return [(self.st.wav_row(w, i, slots[i], counts[i]), m[i, :e], c[i, :e]) for i, e in enumerate(emit)]

    @torch.no_grad()
    def infer_wav_staggered(self, src_wavs, starts, ref_mel, pipelined=True, mel=None, in_rates=None, out_rates=None, out_filter=None,
                            in_formats=None, out_formats=None, loud_norm=False, trim=False, level=None, pitch=None, voice=None, follow=None,
                            register=None, activity=None, activity_log=None, bypass=None, out_level=None, conceal=None, lost=None, echo=None, far=None, echo_delay=None, comfort=None, denoise=None, watermark=None, tones=None, eq=None, out_eq=None, **filter):
        """Utterances that start at different times, served together: src_wavs = list of 1-D cuda waveforms, starts[u] = the tick
        (one feed_ragged call, 80 ms of audio) at which utterance u's first audio arrives, ref_mel [U, Tr, 80] (one reference each).
        Utterance u takes the lowest free slot of self.slots at its start tick (a slot is free again once its drain has emitted 0
        frames; with no slot free the utterance waits for one); every tick is one feed_ragged over the slots live in it.
        -> one (wav, mel [T, 80], codes [T]) per utterance: what infer_wav would give for it alone.  The slot each utterance used is
        left in self.staggered_slots.  in_rates[u] (+ filter keywords): utterance u's sample rate (None: the model rate); one call
        then mixes rates, with rows as wide as the widest input of the call.  out_rates[u] (+ out_filter): the rate utterance u's
        wav is returned at (None: the model rate).  in_formats[u] / out_formats[u]: the sample format utterance u arrives / is
        returned in (None: float32); one call then mixes formats, each row packed in its own.  loud_norm: every utterance is
        loudness-normalised whole, at its own input rate, before its first audio is fed (float32 utterances only).  trim: True, or a
        dict of Context.trim_silence's keywords: the long pauses are cut out of every utterance, whole, at its own input rate (a
        multiple of 50; float32 utterances only) before loud_norm; each keeps its own trimmed length.  level: the
        streaming input leveller (start_wav), one value for every utterance or a list with one per utterance.  pitch: the pitch
        control (start), one value for every utterance or a list with one per utterance.  voice: (bank, ids) - one enrolled id per
        utterance, in place of ref_mel (then None).  follow: source-pitch following (start_wav), one value for every
        utterance or a list with one per utterance.  register: register matching (start_wav), one value for every utterance or a list
        with one per utterance.  activity: the activity detector (start_wav), one value for every utterance or a list with one per
        utterance.  activity_log: a list that receives, per utterance, a list of (act [emit], level [emit]) per emitted chunk
        (chunk_activity after each call, which joins pipelined work).  bypass: the wet/dry mix (start_wav), one value for every
        utterance or a list with one per utterance.  out_level: the output leveller (start), one value for every utterance or a
        list with one per utterance.  conceal: loss concealment (start_wav), one value for every utterance or a list with one per
        utterance; lost: per utterance its whole flags (a 1-D tensor) or None.  Not with loud_norm or trim (Context.conceal repairs an
        utterance whole).  denoise: the noise suppression (start_wav), one value for every utterance or a list with one per utterance.
        watermark: the output watermark (start), one value for every utterance or a list with one per utterance.
        echo: echo cancellation (start_wav), one value for every utterance or a list with one per utterance; far: per utterance its
        whole far end (a 1-D tensor as long as the utterance, in its format) or None, which stands for a silent far end.  Not with
        loud_norm or trim.  echo_delay: the estimator beside the canceller (start_wav), one value for every utterance or a list with
        one per utterance."""
        voice = self._check_voice(ref_mel, voice)
        U = len(src_wavs)
        # (host checks before anything runs; per utterance, in the form open_slots takes back)
        values = self._host_checks(U, voice, ("out_level",), level=level, pitch=pitch, follow=follow, register=register, activity=activity,
                                   bypass=bypass, conceal=conceal, echo=echo, comfort=comfort, denoise=denoise, out_level=out_level, watermark=watermark, tones=tones, eq=eq, out_eq=out_eq)
        self._check_lost(lost, conceal, loud_norm, trim)
        if lost is not None and len(lost) != U:
            raise ValueError(f"lost: {len(lost)} values for {U} utterances")
        self._check_far(far, echo, loud_norm, trim)
        if far is not None and len(far) != U:
            raise ValueError(f"far: {len(far)} values for {U} utterances")
        delays = self._echo_delay_values(echo_delay, echo, U, "utterances")
        if activity_log is not None:
            activity_log[:] = [[] for _ in range(U)]
        ifmts, ofmts, orates, rates = (list(v) if v is not None else [None] * U for v in (in_formats, out_formats, out_rates, in_rates))
        trim = self._trim_keywords(trim)
        if trim is not None:
            src_wavs = [self._trim(x, rates[u], ifmts[u], trim)[0] for u, x in enumerate(src_wavs)]      # (one row: cut to its kept length)
        if loud_norm:
            src_wavs = [self._loud_norm(x, rates[u], ifmts[u]) for u, x in enumerate(src_wavs)]
        assert len(starts) == U and len(ref_mel if voice is None else voice[1]) == U
        Ls = [self._in_len(r) for r in rates]
        pending = sorted(range(U), key=lambda u: (starts[u], u))
        free = sorted(self.slots)
        live = {}                                         # utterance -> [slot, samples fed, final fed]
        outs = [[] for _ in range(U)]
        self.staggered_slots = [None] * U
        tick = 0
        while pending or live:
            new = []
            while pending and starts[pending[0]] <= tick and free:
                u = pending.pop(0)
                live[u] = [free.pop(0), 0, False]
                self.staggered_slots[u] = live[u][0]
                new.append(u)
            if new:
                self.open_slots([live[u][0] for u in new], torch.stack([ref_mel[u] for u in new]) if voice is None else None,
                                voice=None if voice is None else (voice[0], [voice[1][u] for u in new]), in_rate=[rates[u] for u in new],
                                out_rate=[orates[u] for u in new], out_filter=out_filter, in_format=[ifmts[u] for u in new],
                                out_format=[ofmts[u] for u in new], echo_delay=[delays[u] for u in new],
                                **{k: [v[u] for u in new] for k, v in values.items()}, **filter)
            if not live:
                tick += 1
                continue
            us = list(live)
            rows, samples, final, draining, first, frows = [], [], [], [], [], []
            width = max(Ls[u] for u in us)
            for u in us:
                x, (slot, pos, fin) = src_wavs[u], live[u]
                N, L = x.shape[0], Ls[u]
                last = (N - 1) // L * L                   # the final call takes the remaining 1 .. L samples
                draining.append(fin)
                first.append(pos)
                if pos < last:
                    piece, live[u][1] = x[pos:pos + L], pos + L
                    final.append(0)
                elif not fin:
                    piece, live[u][1], live[u][2] = x[pos:], N, True
                    final.append(1)
                else:
                    piece = x[:0]
                    final.append(1)
                samples.append(piece.shape[0])
                rows.append(piece if self.st.input_formats else torch.nn.functional.pad(piece, (0, width - piece.shape[0])))
                if far is not None:      # (the far end of the same samples; none: the format's silence, which leaves the row's bytes alone)
                    quiet = {"ulaw": 0xFF, "alaw": 0xD5}.get(ifmts[u], 0)
                    fpiece = torch.full_like(piece, quiet) if far[u] is None else far[u][first[-1]:first[-1] + piece.shape[0]]
                    frows.append(fpiece if self.st.input_formats else torch.nn.functional.pad(fpiece, (0, width - fpiece.shape[0])))
            # (rows of several dtypes travel as a list, each packed in its slot's format)
            flags = None if lost is None else self._lost_rows([live[u][0] for u in us], [lost[u] for u in us], first, samples)
            res = self.feed_ragged([live[u][0] for u in us], rows if self.st.input_formats else torch.stack(rows), samples, final, pipelined=pipelined, mel=mel,
                                   lost=flags, far=None if far is None else (frows if self.st.input_formats else torch.stack(frows)))
            if activity_log is not None and any(m.shape[0] for _, m, _ in res):
                fl, lv = self.chunk_activity()
                for r, (u, (_, m, _)) in enumerate(zip(us, res)):
                    if m.shape[0]:
                        activity_log[u].append((fl[r, :m.shape[0]].clone(), lv[r, :m.shape[0]].clone()))
            for u, was_final, (w, m, c) in zip(us, draining, res):
                if m.shape[0]:
                    outs[u].append((w, m, c))
                elif was_final:                           # the drain's empty answer: the slot is free again
                    if orates[u] is not None and live[u][0] in self.st.output_rates:      # (the flush joins pipelined work)
                        tail = self.finish([live[u][0]])[0]
                        outs[u].append((tail, m[:0], c[:0]))
                    free.append(live.pop(u)[0])
                    free.sort()
            tick += 1
        if pipelined:
            self.st.join()
        return [tuple(torch.cat(t, 0) for t in zip(*o)) for o in outs]

    def chunks(self, src_mel):
        """inference/Conan.py:95-110: (pos, emit, chunk[B, seg+rc, 80]) with repeat-last padding."""
        B, T, F = src_mel.shape
        pos = 0
        while pos < T:
            emit = min(self.seg, T - pos)
            look = min(self.rc, T - (pos + emit))
            real = emit + look
            chunk = src_mel[:, pos:pos + real]
            need = self.seg + self.rc - real
            if need > 0:
                chunk = torch.cat([chunk, chunk[:, -1:].expand(B, need, F)], 1)
            yield pos, emit, chunk.contiguous()
            pos += emit

    @torch.no_grad()
    def windowed_step(self, chunk, ctx_codes, return_mel=False):
        """One chunk in the bounded-window mode of BASELINE.json configs[1] / configs[4] ("80 ms chunk + 160 ms context",
        "40 ms chunk / 320 ms context window"): the Emformer stays stateful (its left context is its own
        K/V cache); the Conan decoder and the vocoder are reset and fed `ctx_codes` ([B, ctx] int32, the codes of the
        preceding frames, possibly fewer at the start of an utterance) + this chunk's codes in one step; only the last
        `seg` frames are kept.  The oracle of this mode is the reference module fed the same window.
        Returns (codes [B, seg], wav [B, seg*hop]) (+ mel [B, seg, 80])."""
        st, seg, hop = self.st, self.seg, self.ctx.hop
        if st.output_rates or st.output_ld or st.output_formats:
            raise ValueError("windowed_step keeps the last seg * hop model-rate samples of a window: not available on a stream-set whose slots have "
                             "an output rate or format (start(..., out_rate=None, out_format=None) restores the model rate and float32)")
        _, _, codes = st.emformer_step(self.slots, chunk, want_out=False, want_logits=False)
        win = torch.cat([ctx_codes.to(codes.dtype), codes], 1) if ctx_codes is not None and ctx_codes.shape[1] else codes
        st.reset(self.slots, which=2 | 4)
        mel = st.decoder_step(self.slots, win)
        wav = st.hifigan_step(self.slots, mel)
        out = (codes, wav[:, -seg * hop:])
        return out + (mel[:, -seg:],) if return_mel else out

    @torch.no_grad()
    def infer(self, src_mel, ref_mel, ref_len=None, pipelined=True, out_rate=None, out_filter=None, out_format=None, pitch=None, voice=None,
              out_level=None, watermark=None, out_eq=None, drift=None):
        """src_mel [B,T,80], ref_mel [B,Tr,80] (cuda) -> wav [B, T*hop], mel [B,T,80], codes [B,T].
        drift: the far device's clock error in ppm on the output side (start): the returned wav is ctx.resample_drift(side='sink') of
        the model-rate wav at out_rate, bit for bit.

        The whole source is available here, so by default the chunks are issued as pipelined steps
        (conan_step_async): the Emformer + decoder of chunk t+1 overlap the vocoder of chunk t.  The
        results are bit-identical to the blocking loop (pipelined=False).  out_rate (+ out_filter): the returned wav is the
        whole utterance at that rate, ctx.resample of the model-rate wav bit for bit.  out_format: the returned wav's sample format.
        pitch: the slots' pitch control in the decoder step (start).  voice: (bank, ids) in place of ref_mel (then None; start).
        out_level: the output leveller (start): the returned model-rate wav is ctx.level of the unlevelled one, bit for bit.
        watermark: the output watermark (start): the returned model-rate wav is ctx.watermark_embed of the unmarked one, bit for bit."""
        self._check_voice(ref_mel, voice)
        if self.ctx.cfg.voc_upsample == 2:
            if drift not in (None, False):
                raise ValueError("drift with an upsample 'nn' vocoder: its steps are whole prefixes; run Context.resample_drift(side='sink') over the "
                                 "returned wav instead")
            if out_eq not in (None, False):
                raise ValueError("out_eq with an upsample 'nn' vocoder: its steps are whole prefixes, not update intervals; filter the returned wav "
                                 "with Context.eq instead")
            if watermark not in (None, False):
                raise ValueError("watermark with an upsample 'nn' vocoder: its steps are whole prefixes, not update intervals; mark the returned wav "
                                 "with Context.watermark_embed instead")
            if out_level not in (None, False):
                raise ValueError("out_level with an upsample 'nn' vocoder: its steps are whole prefixes, not update intervals; level the returned wav "
                                 "with Context.level instead")
            if out_format not in (None, "f32"):
                raise ValueError("out_format with an upsample 'nn' vocoder: convert the returned wav with Context.convert_samples instead")
            self._set_out_rate(self.slots, out_rate, out_filter)      # (refuses a rate; restores the model rate)
            return self._infer_prefix_vocoder(src_mel, ref_mel, ref_len, pitch, voice)
        self.start(ref_mel, ref_len, out_rate=out_rate, out_filter=out_filter, out_format=out_format, pitch=pitch, voice=voice, out_level=out_level, watermark=watermark, out_eq=out_eq,
                   drift=drift)
        B = src_mel.shape[0]
        hop, nm = self.ctx.hop, self.ctx.cfg.num_mels
        wavs, mels, codes = [], [], []
        for pos, emit, chunk in self.chunks(src_mel):
            if pipelined:
                c = torch.empty(B, self.seg, dtype=torch.int32, device=src_mel.device)
                m = torch.empty(B, emit, nm, device=src_mel.device)
                w = torch.empty(B, self.st.output_ld or emit * hop, device=src_mel.device)
                self.st.step_async(self.slots, chunk, w, emit=emit, codes=c, mel_out=m)
                if self.st.output_ld or self.st.output_formats:
                    w = self.st.wav_block(w, self.slots, self.st.output_samples()[0])
            else:
                c, m, w = self.st.step(self.slots, chunk, emit=emit)
            wavs.append(self._rows(w))
            mels.append(m)
            codes.append(c[:, :emit])
        if pipelined:
            self.st.join()
        if self.st.output_rates:
            wavs.append(torch.stack(self.finish()))
        return torch.cat(wavs, 1), torch.cat(mels, 1), torch.cat(codes, 1)

    @torch.no_grad()
    def _infer_prefix_vocoder(self, src_mel, ref_mel, ref_len=None, pitch=None, voice=None):
        """Vocoders that look ahead (`upsample: nn`, CausalUpsampleBlock1) cannot carry state from chunk to chunk; the
        reference loop does not need them to: it runs the vocoder on ALL mel frames so far and keeps the samples of the
        current chunk (inference/Conan.py:147-155).  Same here: Emformer and decoder step statefully, the vocoder is reset
        and run over the prefix (O(T^2) like the reference; rings sized for the whole utterance)."""
        B, T, _ = src_mel.shape
        if self.st.max_frames < T:
            mr = self.st.max_ref_frames
            self.st.close()
            self.st = self.ctx.streams(self.n, max_frames=T, max_ref_frames=mr, arith=self.arith, flags=self.flags, dev_plan=self.dev_plan)
        self.start(ref_mel, ref_len, pitch=pitch, voice=voice)
        hop = self.ctx.hop
        wavs, mels, codes = [], [], []
        for pos, emit, chunk in self.chunks(src_mel):
            _, _, c = self.st.emformer_step(self.slots, chunk, want_out=False, want_logits=False)
            m = self.st.decoder_step(self.slots, c[:, :emit].contiguous())
            mels.append(m)
            codes.append(c[:, :emit])
            self.st.reset(self.slots, which=4)
            w = self.st.hifigan_step(self.slots, torch.cat(mels, 1))
            wavs.append(w[:, pos * hop:(pos + emit) * hop])
        return torch.cat(wavs, 1), torch.cat(mels, 1), torch.cat(codes, 1)
