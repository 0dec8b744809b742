"""Cost of the loss concealment's repair launch (conan_streams_conceal) at 64 slots, full model, synthetic weights:
`python tools/conceal_time.py [launches]` prints one JSON line.
  repair_us     cnk::conceal_kernel's time per launch under the profile hooks (conan_profile_*), 64 rows of one 80 ms chunk, per case:
                the rate's defaults at 16 kHz f32 and at 48 kHz s16; no packet lost (the rows are decoded and the state moves on,
                nothing is written), one packet of four lost in every row (one lag search, one packet synthesised, one fade), every
                packet lost (a run that goes on: no search after the first call);
  wav_in_ms     the blocking wav-in call the repair stands in front of (conan_step_wav, 64 slots at the model rate, f32): device
                events around 20 calls, the median of 5 such groups."""
import json
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
import bench
from conan_amd import _lib, synth
from conan_amd.engine import StreamingVoiceConversionEngine

B = 64
K = int(sys.argv[1]) if len(sys.argv) > 1 else 40
ctx, chp, vhp = bench.build_context(0)
hop, seg = ctx.hop, ctx.cfg.emf_segment
L = seg * hop
rng = np.random.default_rng(0)
ref = torch.from_numpy(synth.mel(256, 4321, B)).cuda()
eng = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=257)
st = eng.st


def tone(n, rate):
    t = np.arange(n) / float(rate)
    return np.stack([0.3 * np.sin(2 * np.pi * (110 + 3 * i) * t) + 1e-3 * rng.standard_normal(n) for i in range(B)]).astype(np.float32)


def repair_case(rate, fmt, flags):
    """us per launch over K launches on consecutive chunks; the first call of a case (the restart) is left out."""
    n = rate // 50 * 4
    x = torch.from_numpy(tone(n * (K + 1), rate)).cuda()
    if fmt != "f32":
        x = ctx.convert_samples(x, "f32", fmt)
    st.set_input_format(eng.slots, fmt)
    st.set_conceal(eng.slots, None)
    st.set_conceal(eng.slots, True, rate=rate)
    lost = torch.tensor([flags] * B, dtype=torch.int32, device="cuda")
    rows = [x[:, j * n:(j + 1) * n].contiguous() for j in range(K + 1)]
    st.conceal(eng.slots, rows[0], n, lost)
    st.profile_begin()
    for j in range(1, K + 1):
        st.conceal(eng.slots, rows[j], n, lost)
    st.profile_end()
    k = [k for k in st.profile_kernels() if k[0] == "conceal_kernel"]
    assert len(k) == 1 and k[0][3] == K, k
    return k[0][1] * 1e3 / K


def wav_in_call():
    st.set_input_format(eng.slots, "f32")
    eng.start_wav(ref)
    x = torch.from_numpy(tone(L * 128, 16000)).cuda()
    ps = [x[:, j * L:(j + 1) * L].contiguous() for j in range(128)]
    for j in range(8):
        st.step_wav(eng.slots, ps[j])
    groups, j = [], 8
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(20):
            st.step_wav(eng.slots, ps[j])
            j += 1
        b.record()
        torch.cuda.synchronize()
        groups.append(a.elapsed_time(b) / 20)
    return float(np.median(groups)), groups


eng.start_wav(ref)
cases = {"none": [0, 0, 0, 0], "one_of_four": [0, 1, 0, 0], "all": [1, 1, 1, 1]}
repair = {f"{rate // 1000}k_{fmt}": {name: repair_case(rate, fmt, fl) for name, fl in cases.items()} for rate, fmt in ((16000, "f32"), (48000, "s16"))}
ms, groups = wav_in_call()
print(json.dumps({"slots": B, "launches": K, "state_bytes_per_slot": int(_lib.lib().conan_conceal_state_bytes()), "repair_us": repair,
                  "wav_in_ms": ms, "wav_in_ms_groups": groups}))
