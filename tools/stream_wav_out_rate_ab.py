"""64 pipelined same-position streams whose audio leaves at other sample rates, full model, synthetic weights:
`python tools/stream_wav_out_rate_ab.py [steps] [repeats] [mode]` prints one JSON line (ms per 80 ms tick, medians, ratios against
the run without an output rate).  Modes: none (the model rate, no output resampler), 48000_hann, 44100_kaiser_best and 8000_hann
(conan_streams_set_output_rate, one resample_out_kernel launch per conan_step_wav_async call behind conv_post_kernel, on the vocoder
stream); `all` (default) alternates the four within the run.  A single mode is what to run under `rocprofv3 --kernel-trace --stats`
for resample_out_kernel's time per launch (profiles/stream_wav_out_rate_b64_*).  On a shared machine give every GPU step its own
time limit and chain them:
  timeout -k 10 300 python tools/stream_wav_out_rate_ab.py 60 3 all && \\
  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d profiles/stream_wav_out_rate_b64_48000_hann -- python tools/stream_wav_out_rate_ab.py 60 1 48000_hann && ..."""
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
MODES = {"none": (None, None), "48000_hann": (48000, "hann"), "44100_kaiser_best": (44100, "kaiser_best"), "8000_hann": (8000, "hann")}
ctx, chp, vhp = bench.build_context(0)
eng = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=257)
hop, seg = ctx.hop, ctx.cfg.emf_segment
L = seg * hop
rng = np.random.default_rng(0)
ref = torch.from_numpy(synth.mel(256, 4321, B)).cuda()
N = (W + K + 2) * L
t = np.arange(N) / 16000.0
x = torch.from_numpy(np.stack([0.3 * np.sin(2 * np.pi * (120 + 5 * i) * t) + 0.05 * rng.standard_normal(N) for i in range(B)]).astype(np.float32)).cuda()
ps = [x[:, j * L:(j + 1) * L].contiguous() for j in range(W + K + 2)]


def run(rate, preset):
    eng.start_wav(ref, out_rate=rate, out_filter={"preset": preset or "hann"})
    ld = eng.st.output_ld or L
    outs = [(torch.empty(B, seg, dtype=torch.int32, device="cuda"), torch.empty(B, seg, 80, device="cuda"), torch.empty(B, ld, device="cuda")) for _ in range(8)]
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
res = {k: [] for k in modes}
for r in range(REP):
    for k in modes:
        res[k].append(run(*MODES[k]))
med = {k: float(np.median(v)) for k, v in res.items()}
out = {"streams": B, "steps": K, "ms_per_tick": res, "median": med}
if "none" in med:
    out["over_none"] = {k: med[k] / med["none"] - 1 for k in med if k != "none"}
print(json.dumps(out))
