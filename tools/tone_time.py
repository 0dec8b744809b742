"""Cost of the signalling tones (conan_streams_set_tones) on 64 pipelined same-position wav-in streams, full model, synthetic weights:
`python tools/tone_time.py [steps] [repeats]` prints one JSON line.
  ms_per_step   off / idle / keyed alternated within the run (three stream-sets: never called the setter; mode 2 on every slot, fed
                speech-like audio without a key, so the fill finds level 0; mode 2 on every slot, fed 100 ms key presses 100 ms apart,
                so the fill sounds half of the time): the mean interval between consecutive step completions (conan_step_clock), one
                figure per repeat;
  kernels       blocking calls under the profile hooks, per case: tone_kernel's and tone_fill_kernel's time per launch (64 rows of 4
                frames; 64 rows of 1280 samples)."""
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
line = 1e-3 * rng.standard_normal((B, N))
voice = np.stack([0.2 * np.sin(2 * np.pi * (120 + 5 * i) * t) + 0.1 * np.sin(2 * np.pi * 3 * (120 + 5 * i) * t) for i in range(B)]) + line
keys = np.stack([0.25 * (np.sin(2 * np.pi * (697, 770, 852, 941)[i % 4] * t) + np.sin(2 * np.pi * (1209, 1336, 1477, 1633)[i // 4 % 4] * t)) for i in range(B)])
press = (np.arange(N) // 1600) % 2 == 1
SIGNAL = {"off": voice, "idle": voice, "keyed": np.where(press, keys, voice)}
ps = {k: [torch.from_numpy(v[:, j * L:(j + 1) * L].astype(np.float32)).cuda().contiguous() for j in range(W + K + 2)] for k, v in SIGNAL.items()}
engines = {k: StreamingVoiceConversionEngine(ctx, B, max_ref_frames=257) for k in SIGNAL}
START = {"off": {}, "idle": dict(tones=True), "keyed": dict(tones=True)}


def run(mode):
    eng = engines[mode]
    eng.start_wav(ref, **START[mode])
    st = eng.st
    outs = [(torch.empty(B, seg, dtype=torch.int32, device="cuda"), torch.empty(B, seg, 80, device="cuda"), torch.empty(B, L, device="cuda")) for _ in range(8)]
    st.step_wav_async(eng.slots, ps[mode][0])          # first call: no chunk
    for j in range(1, W + K + 1):
        if j == W + 1:
            st.join(); torch.cuda.synchronize()
            st.step_clock(K + 1)
        c, m, w = outs[j % 8]
        e, _, _, _ = st.step_wav_async(eng.slots, ps[mode][j], codes=c, mel_out=m, wav_out=w)
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
        st.step_wav(eng.slots, ps[mode][j])
    st.profile_begin()
    for j in range(W, W + 20):
        st.step_wav(eng.slots, ps[mode][j])
    st.profile_end()
    names = ("tone_kernel", "tone_fill_kernel")
    return {k[0]: {"us_per_launch": k[1] * 1e3 / k[3], "launches": k[3]} for k in st.profile_kernels() if k[0] in names}


res = {k: [] for k in engines}
for r in range(REP):
    for k in engines:
        res[k].append(run(k))
print(json.dumps({"streams": B, "steps": K, "repeats": REP, "ms_per_step": res, "median": {k: float(np.median(v)) for k, v in res.items()},
                  "spread": {k: [min(v), max(v)] for k, v in res.items()}, "kernels": {k: kernel_times(k) for k in engines}}))
