"""64 pipelined same-position streams fed audio at other sample rates, full model, synthetic weights:
`python tools/stream_wav_rate_ab.py [steps] [repeats] [mode]` prints one JSON line (ms per 80 ms tick, medians, ratios against
16 kHz input).  Modes: 16000 (the model rate, no resampler), 48000_hann and 44100_kaiser_best (conan_streams_set_input_rate, one
resample_stream_kernel launch per conan_step_wav_async call in front of mel_stream_kernel); `all` (default) alternates the three
within the run.  A single mode is what to run under `rocprofv3 --kernel-trace --stats` for resample_stream_kernel's time per call
(profiles/stream_wav_resample_b64_*)."""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
import bench
from conan_amd import synth
from conan_amd.engine import StreamingVoiceConversionEngine

B = 64
K = int(sys.argv[1]) if len(sys.argv) > 1 else 60
REP = int(sys.argv[2]) if len(sys.argv) > 2 else 3
MODE = sys.argv[3] if len(sys.argv) > 3 else "all"
W = 10
MODES = {"16000": (16000, None), "48000_hann": (48000, "hann"), "44100_kaiser_best": (44100, "kaiser_best")}
ctx, chp, vhp = bench.build_context(0)
eng = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=257)
hop, seg = ctx.hop, ctx.cfg.emf_segment
L = seg * hop
rng = np.random.default_rng(0)
ref = torch.from_numpy(synth.mel(256, 4321, B)).cuda()
outs = [(torch.empty(B, seg, dtype=torch.int32, device="cuda"), torch.empty(B, seg, 80, device="cuda"), torch.empty(B, L, device="cuda")) for _ in range(8)]


def pieces(rate):
    Li = L * rate // 16000
    N = (W + K + 2) * Li
    t = np.arange(N) / float(rate)
    x = np.stack([0.3 * np.sin(2 * np.pi * (120 + 5 * i) * t) + 0.05 * rng.standard_normal(N) for i in range(B)]).astype(np.float32)
    x = torch.from_numpy(x).cuda()
    return [x[:, j * Li:(j + 1) * Li].contiguous() for j in range(W + K + 2)]


def run(rate, preset, ps):
    eng.start_wav(ref, in_rate=rate if preset else None, preset=preset or "hann")
    eng.st.step_wav_async(eng.slots, ps[0])          # first call: no chunk
    for j in range(1, W + K + 1):
        if j == W + 1:
            eng.st.join(); torch.cuda.synchronize(); t0 = time.perf_counter()
        c, m, w = outs[j % 8]
        e, _, _, _ = eng.st.step_wav_async(eng.slots, ps[j], codes=c, mel_out=m, wav_out=w)
        assert e == seg
    eng.st.join(); torch.cuda.synchronize()
    return (time.perf_counter() - t0) / K * 1e3


modes = list(MODES) if MODE == "all" else [MODE]
data = {k: pieces(MODES[k][0]) for k in modes}
res = {k: [] for k in modes}
for r in range(REP):
    for k in modes:
        res[k].append(run(*MODES[k], data[k]))
med = {k: float(np.median(v)) for k, v in res.items()}
out = {"streams": B, "steps": K, "ms_per_tick": res, "median": med}
if "16000" in med:
    out["over_16k"] = {k: med[k] / med["16000"] - 1 for k in med if k != "16000"}
print(json.dumps(out))
