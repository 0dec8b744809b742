"""What a target voice costs (python3 tools/voice_time.py [max_slots]; default a 64-slot stream-set of the full configuration with
256-frame references): conan_set_reference - the style pass - against conan_streams_set_voice from a bank, and how long a
pipelined step sequence stalls around each.

Call times: device events around one call (set_reference) or around windows of back-to-back calls (set_voice) after a warm-up, so a
call's host side is inside the figure; medians with the range.  Stall: 60 pipelined steps with the step clock on (one completion
stamp per step on the vocoder stream); at step 30 nothing / set_reference / set_voice of all slots is called; printed are the median
interval between completions, the largest interval among the ten around the call, and their difference."""
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from conan_amd import configs, synth  # noqa: E402
from conan_amd.runtime import Context  # noqa: E402

S = int(sys.argv[1]) if len(sys.argv) > 1 else 64
REF = 256
chp, vhp = configs.conan_hparams(), configs.hifigan_hparams()
ctx = Context(chp, vhp, 0)
ctx.load_state_dict("emformer", synth.emformer_state_dict(chp, 0))
ctx.load_state_dict("conan", synth.conan_state_dict(chp, 0))
ctx.load_state_dict("hifigan", synth.hifigan_state_dict(vhp, 0))
ctx.finalize()
st = ctx.streams(S, max_frames=4, max_ref_frames=REF)
slots = list(range(S))
ref = torch.from_numpy(synth.mel(REF, 3, S)).cuda()
bank = ctx.voices(S, REF)
bank.enroll(slots, ref, via=st)
st.reset(slots)
print("stream-set of %d slots (arith %s), references of %d frames; a voice is %d bytes" % (S, st.arith, REF, bank.info(0)["bytes"]))


def timed(fn, windows, calls):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        us.append(1e3 * a.elapsed_time(b) / calls)
    return float(np.median(us)), float(min(us)), float(max(us))


r = timed(lambda: st.set_reference(slots, ref), 7, 1)
v = timed(lambda: st.set_voice(slots, bank, slots), 15, 20)
print("set_reference of %d slots: %.1f us (%.1f-%.1f) | set_voice of the same slots: %.1f us (%.1f-%.1f) | ratio %.0f"
      % (S, r[0], r[1], r[2], v[0], v[1], v[2], r[0] / v[0]))

seg, rc, hop = st.seg, st.rc, ctx.hop
STEPS, AT = 60, 30
mel = torch.from_numpy(synth.mel(STEPS * seg + rc, 7, S)).cuda()
chunks = [mel[:, j * seg:j * seg + seg + rc].contiguous() for j in range(STEPS)]
wav = torch.empty(S, seg * hop, device="cuda")


def sequence(call):
    st.reset(slots)
    st.set_voice(slots, bank, slots)
    st.step_clock(STEPS + 4)
    for j, ch in enumerate(chunks):
        if j == AT and call is not None:
            call()
        st.step_async(slots, ch, wav)
    st.join()
    torch.cuda.synchronize()
    ms = np.array(st.step_clock_read())
    st.step_clock(0)
    near = ms[AT - 4:AT + 6]      # (interval i lies between the completions of steps i and i + 1; the first ones fill the pipeline)
    return float(np.median(ms)), float(near.max()), AT - 4 + int(near.argmax())


sequence(None)      # warm-up
for name, call in (("no call", None), ("set_reference", lambda: st.set_reference(slots, ref)), ("set_voice", lambda: st.set_voice(slots, bank, slots)),
                   ("no call", None), ("set_reference", lambda: st.set_reference(slots, ref)), ("set_voice", lambda: st.set_voice(slots, bank, slots))):
    med, worst, at = sequence(call)
    print("%-13s at step %d of %d pipelined steps: median interval %.3f ms, largest %.3f ms (interval %d): stall %.3f ms" % (name, AT, STEPS, med, worst, at, worst - med))
bank.close()
st.close()
ctx.close()
