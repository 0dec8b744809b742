"""Cost of the equaliser (conan_streams_set_input_eq / conan_streams_set_output_eq) on 64 pipelined same-position wav-in streams, full
model, synthetic weights: `python tools/eq_time.py [steps] [repeats] [legs]` prints one JSON line.
  ms_per_step   the legs (default off,in,out; at most three stream-sets in one process, so `both` takes a second run: off,both)
                alternated within the run - off: never called a setter; in: the source-side filter on every slot; out: the output
                filter on every slot; both - four sections each: the mean interval between consecutive step completions
                (conan_step_clock), one figure per repeat;
  kernels       blocking calls under the profile hooks, per case: eq_stream_kernel's time per launch (64 rows of 1280 samples).
The cascade (high-pass 80 Hz, notch 50 Hz Q 30, peak +6 dB at 2.5 kHz, low-pass 3.4 kHz) is a choice for timing: nobody has listened
to it."""
import json
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
import bench
from conan_amd import synth
from conan_amd.engine import StreamingVoiceConversionEngine

B = 64
K = int(sys.argv[1]) if len(sys.argv) > 1 else 60
REP = int(sys.argv[2]) if len(sys.argv) > 2 else 3
W = 10
ctx, chp, vhp = bench.build_context(0)
hop, seg = ctx.hop, ctx.cfg.emf_segment
L = seg * hop
rng = np.random.default_rng(0)
ref = torch.from_numpy(synth.mel(256, 4321, B)).cuda()
N = (W + K + 2) * L
t = np.arange(N) / 16000.0
voice = np.stack([0.2 * np.sin(2 * np.pi * (120 + 5 * i) * t) + 0.1 * np.sin(2 * np.pi * 3 * (120 + 5 * i) * t) for i in range(B)])
voice = voice + 0.05 + 0.02 * np.sin(2 * np.pi * 50.0 * t) + 1e-3 * rng.standard_normal((B, N))
ps = [torch.from_numpy(voice[:, j * L:(j + 1) * L].astype(np.float32)).cuda().contiguous() for j in range(W + K + 2)]
EQ = dict(sections=[dict(kind="highpass", f=80.0), dict(kind="notch", f=50.0, q=30.0), dict(kind="peak", f=2500.0, q=1.0, gain_db=6.0),
                    dict(kind="lowpass", f=3400.0)])
LEGS = sys.argv[3].split(",") if len(sys.argv) > 3 else ["off", "in", "out"]
ALL = {"off": {}, "in": dict(eq=EQ), "out": dict(out_eq=EQ), "both": dict(eq=EQ, out_eq=EQ)}
assert 1 <= len(LEGS) <= 3 and all(k in ALL for k in LEGS), LEGS
START = {k: ALL[k] for k in LEGS}
engines = {k: StreamingVoiceConversionEngine(ctx, B, max_ref_frames=257) for k in START}


def run(mode):
    eng = engines[mode]
    eng.start_wav(ref, **START[mode])
    st = eng.st
    outs = [(torch.empty(B, seg, dtype=torch.int32, device="cuda"), torch.empty(B, seg, 80, device="cuda"), torch.empty(B, L, device="cuda")) for _ in range(8)]
    st.step_wav_async(eng.slots, ps[0])          # first call: no chunk
    for j in range(1, W + K + 1):
        if j == W + 1:
            st.join(); torch.cuda.synchronize()
            st.step_clock(K + 1)
        c, m, w = outs[j % 8]
        e, _, _, _ = st.step_wav_async(eng.slots, ps[j], codes=c, mel_out=m, wav_out=w)
        assert e == seg
    st.join(); torch.cuda.synchronize()
    iv = st.step_clock_read()
    st.step_clock(0)
    return statistics.fmean(iv)


def kernel_times(mode):
    eng = engines[mode]
    eng.start_wav(ref, **START[mode])
    st = eng.st
    for j in range(W):
        st.step_wav(eng.slots, ps[j])
    st.profile_begin()
    for j in range(W, W + 20):
        st.step_wav(eng.slots, ps[j])
    st.profile_end()
    return {k[0]: {"us_per_launch": k[1] * 1e3 / k[3], "launches": k[3]} for k in st.profile_kernels() if k[0] == "eq_stream_kernel"}


res = {k: [] for k in engines}
for r in range(REP):
    for k in engines:
        res[k].append(run(k))
print(json.dumps({"streams": B, "steps": K, "repeats": REP, "ms_per_step": res, "median": {k: float(np.median(v)) for k, v in res.items()},
                  "spread": {k: [min(v), max(v)] for k, v in res.items()}, "kernels": {k: kernel_times(k) for k in engines}}))
