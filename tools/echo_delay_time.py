"""Cost of the echo-delay estimator (conan_streams_set_echo_delay, conan_streams_echo_delay) on 64 pipelined same-position wav-in
streams, full model, synthetic weights: `python tools/echo_delay_time.py [steps] [repeats]` prints one JSON line.
  ms_per_step   the legs alternated within the run - echo: the canceller on every slot with the 16 kHz defaults, the yardstick (its
                launches are the ones the stream-set ran before the estimator existed); echo_delay: the estimator beside it with the
                16 kHz defaults (6144 lags), its launch in front of the canceller's on the caller's stream: the mean interval
                between consecutive step completions (conan_step_clock), one figure per repeat;
  kernel_us     the kernel alone, blocking calls under the profile hooks: echo_delay_kernel's time per launch on 64 rows of 1280
                samples for n_lags 1024 / 3072 / 6144 (a white far end, its echo in the mic).
The echo path (a 3-sample delay at half level) is a choice for timing: no measured room is in the repository.  The legs drive
Streams directly, so the canceller's delay stays where it is: the engine's follow rule is host arithmetic between calls."""
import json
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
import bench
from conan_amd import _lib, synth
from conan_amd.engine import StreamingVoiceConversionEngine

B = 64
K = int(sys.argv[1]) if len(sys.argv) > 1 else 60
REP = int(sys.argv[2]) if len(sys.argv) > 2 else 5
W = 10
ctx, chp, vhp = bench.build_context(0)
hop, seg = ctx.hop, ctx.cfg.emf_segment
L = seg * hop
rng = np.random.default_rng(0)
ref = torch.from_numpy(synth.mel(256, 4321, B)).cuda()
N = (W + K + 2) * L
t = np.arange(N) / 16000.0
far = 0.1 * rng.standard_normal((B, N))
voice = np.stack([0.1 * np.sin(2 * np.pi * (120 + 5 * i) * t) for i in range(B)]) + 0.5 * np.roll(far, 3, 1) + 1e-3 * rng.standard_normal((B, N))
ps = [torch.from_numpy(voice[:, j * L:(j + 1) * L].astype(np.float32)).cuda().contiguous() for j in range(W + K + 2)]
fs = [torch.from_numpy(far[:, j * L:(j + 1) * L].astype(np.float32)).cuda().contiguous() for j in range(W + K + 2)]
START = {"echo": dict(echo=True), "echo_delay": dict(echo=True, echo_delay=True)}
engines = {k: StreamingVoiceConversionEngine(ctx, B, max_ref_frames=257) for k in START}


def run(mode):
    eng = engines[mode]
    eng.start_wav(ref, **START[mode])
    st = eng.st
    outs = [(torch.empty(B, seg, dtype=torch.int32, device="cuda"), torch.empty(B, seg, 80, device="cuda"), torch.empty(B, L, device="cuda")) for _ in range(8)]
    ins = [torch.empty(B, L, device="cuda") for _ in range(8)]      # (the canceller works in place: each step takes a copy of its chunk)
    st.step_wav_async(eng.slots, ins[0].copy_(ps[0]), far=fs[0])          # first call: no chunk
    for j in range(1, W + K + 1):
        if j == W + 1:
            st.join(); torch.cuda.synchronize()
            st.step_clock(K + 1)
        c, m, w = outs[j % 8]
        e, _, _, _ = st.step_wav_async(eng.slots, ins[j % 8].copy_(ps[j]), codes=c, mel_out=m, wav_out=w, far=fs[j])
        assert e == seg
    st.join(); torch.cuda.synchronize()
    iv = st.step_clock_read()
    st.step_clock(0)
    return statistics.fmean(iv)


def kernel_time(n_lags):
    st = engines["echo_delay"].st
    st.set_echo_delay(list(range(B)), None)
    st.set_echo_delay(list(range(B)), _lib.echo_delay_cfg(16000, n_lags=n_lags))
    for j in range(W):
        st.echo_delay(list(range(B)), ps[j], L, fs[j])
    st.profile_begin()
    for j in range(W, W + 20):
        st.echo_delay(list(range(B)), ps[j], L, fs[j])
    st.profile_end()
    k = [k for k in st.profile_kernels() if k[0] == "echo_delay_kernel"][0]
    state = st.echo_delay_state([0])[0].cpu().numpy()
    est = int(np.frombuffer(state[8:12].tobytes(), dtype=np.int32)[0])
    return {"us_per_launch": k[1] * 1e3 / k[3], "launches": k[3], "est_slot0": est}


res = {k: [] for k in engines}
for r in range(REP):
    for k in engines:
        res[k].append(run(k))
print(json.dumps({"streams": B, "steps": K, "repeats": REP, "ms_per_step": res, "median": {k: float(np.median(v)) for k, v in res.items()},
                  "spread": {k: [min(v), max(v)] for k, v in res.items()}, "state_bytes_per_slot": int(_lib.lib().conan_echo_delay_state_bytes()),
                  "kernel_us": {str(n): kernel_time(n) for n in (1024, 3072, 6144)}}))
