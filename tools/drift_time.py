"""Cost of drift rows in the two resampler launches (resample_stream_kernel, resample_out_kernel) at 64 slots, full model,
synthetic weights: `python tools/drift_time.py [calls]` prints one JSON line.
  stream_us     resample_stream_kernel's time per launch under the profile hooks (conan_profile_*), 64 rows of one 80 ms chunk at
                48 kHz and at 8 kHz: every row rational (set_input_rate: the parent commit's launch), every row a drift row
                (set_input_drift at +300 ppm), and 32 of each in one call;
  out_us        resample_out_kernel's time per launch, 64 rows of one vocoder step to 48 kHz and to 8 kHz, the same three cases
                (set_output_rate / set_output_drift).
The rational cases run the code the parent commit ran plus one uniform branch per row; run the parent's library with the same
script (its drift cases fail on the missing symbols) for the parent's own numbers."""
import json
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
import bench
from conan_amd import synth
from conan_amd.engine import StreamingVoiceConversionEngine

B = 64
K = int(sys.argv[1]) if len(sys.argv) > 1 else 20
ctx, chp, vhp = bench.build_context(0)
hop, seg = ctx.hop, ctx.cfg.emf_segment
L = seg * hop
rng = np.random.default_rng(0)
ref = torch.from_numpy(synth.mel(256, 4321, B)).cuda()
eng = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=257)
st = eng.st
HALF = list(range(0, B, 2))


def tone(n, rate):
    t = np.arange(n) / float(rate)
    return torch.from_numpy(np.stack([0.3 * np.sin(2 * np.pi * (110 + 3 * i) * t) + 1e-3 * rng.standard_normal(n) for i in range(B)]).astype(np.float32)).cuda()


def per_launch(name):
    k = [k for k in st.profile_kernels() if k[0] == name]
    assert len(k) == 1 and k[0][3] == K, k
    return k[0][1] * 1e3 / K


def stream_case(rate, drift_slots):
    eng.start_wav(ref)
    st.set_input_rate(eng.slots, rate)
    if drift_slots:
        st.set_input_drift(drift_slots, 300.0, rate=rate)
    s_in = L * rate // 16000
    x = tone(s_in * (K + 2), rate)
    common = len(drift_slots) in (0, B)
    call = (lambda w: st.step_wav(eng.slots, w)) if common else (lambda w: st.step_wav_ragged(eng.slots, w, [s_in] * B, [0] * B))
    for j in range(2):
        call(x[:, j * s_in:(j + 1) * s_in].contiguous())
    st.profile_begin()
    for j in range(2, K + 2):
        call(x[:, j * s_in:(j + 1) * s_in].contiguous())
    st.profile_end()
    return per_launch("resample_stream_kernel")


def out_case(rate, drift_slots):
    eng.start(ref)
    st.set_output_rate(eng.slots, rate)
    if drift_slots:
        st.set_output_drift(drift_slots, 300.0, rate=rate)
    st.set_output_ld(L * rate // 16000 + 64)
    mel = torch.from_numpy(synth.mel(seg * (K + 2), 77, B)).cuda()
    for j in range(2):
        st.hifigan_step(eng.slots, mel[:, j * seg:(j + 1) * seg])
    st.profile_begin()
    for j in range(2, K + 2):
        st.hifigan_step(eng.slots, mel[:, j * seg:(j + 1) * seg])
    st.profile_end()
    us = per_launch("resample_out_kernel")
    st.set_output_rate(eng.slots, 16000)
    st.set_output_ld(0)
    return us


cases = {"rational": [], "drift": list(range(B)), "half": HALF}
stream = {f"{r // 1000}k": {name: stream_case(r, sl) for name, sl in cases.items()} for r in (48000, 8000)}
out = {f"{r // 1000}k": {name: out_case(r, sl) for name, sl in cases.items()} for r in (48000, 8000)}
print(json.dumps({"slots": B, "launches": K, "stream_us": stream, "out_us": out}))
