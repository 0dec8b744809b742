"""64 pipelined same-position streams whose audio arrives and leaves in other sample formats, full model, synthetic weights:
`python tools/stream_wav_format_ab.py [steps] [repeats] [mode]` prints one JSON line (ms per 80 ms tick per run, medians).
Modes, alternated within the run when `all` (default):
  f32_8k, f32_8k_again   8 kHz hann in and out as float32, twice: the yardstick and its own spread (A/A in the same alternation);
  ulaw_8k                the same with mu-law in and out (conan_streams_set_input_format / _output_format): the same launches as
                         f32_8k, so the formats should cost nothing outside that spread;
  f32_16k                the model rate as float32: no I/O launch at all;
  s16_16k                the model rate as 16-bit PCM in and out: adds the two copy-row launches (resample_stream_kernel in front of
                         the front-end launch, resample_out_kernel behind conv_post_kernel).
The JSON reports (a) ulaw_8k against f32_8k beside the A/A spread and (b) the time s16_16k adds per tick and per added launch.
A single mode is what to run under `rocprofv3 --kernel-trace --stats` for the kernels' time per launch
(profiles/stream_wav_format_b64_*).  On a shared machine give every GPU step its own time limit and chain them:
  timeout -k 10 300 python tools/stream_wav_format_ab.py 60 5 all && \\
  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d profiles/stream_wav_format_b64_s16_16k -- python tools/stream_wav_format_ab.py 60 1 s16_16k"""
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
REP = int(sys.argv[2]) if len(sys.argv) > 2 else 5
MODE = sys.argv[3] if len(sys.argv) > 3 else "all"
W = 10
# mode -> (rate in and out, format in and out)
MODES = {"f32_8k": (8000, None), "ulaw_8k": (8000, "ulaw"), "f32_8k_again": (8000, None), "f32_16k": (None, None), "s16_16k": (None, "s16")}
ctx, chp, vhp = bench.build_context(0)
eng = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=257)
hop, seg = ctx.hop, ctx.cfg.emf_segment
L = seg * hop
rng = np.random.default_rng(0)
ref = torch.from_numpy(synth.mel(256, 4321, B)).cuda()


def signal(rate):
    N = (W + K + 2) * L * rate // 16000
    t = np.arange(N) / float(rate)
    return torch.from_numpy(np.stack([0.3 * np.sin(2 * np.pi * (120 + 5 * i) * t) + 0.05 * rng.standard_normal(N) for i in range(B)]).astype(np.float32)).cuda()


PIECES = {}


def pieces(rate, fmt):
    """The calls' input rows in `fmt`, converted once (the callers' side of the wire is not what is timed)."""
    key = (rate, fmt)
    if key not in PIECES:
        x = signal(rate or 16000)
        if fmt:
            x = ctx.convert_samples(x, "f32", fmt)
        Li = L * (rate or 16000) // 16000
        PIECES[key] = [x[:, j * Li:(j + 1) * Li].contiguous() for j in range(W + K + 2)]
    return PIECES[key]


def run(rate, fmt):
    ps = pieces(rate, fmt)
    eng.start_wav(ref, in_rate=rate, out_rate=rate, in_format=fmt, out_format=fmt)
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
out = {"streams": B, "steps": K, "repeats": REP, "ms_per_tick": res, "median": med}
if MODE == "all":
    out["a_8k"] = {"ulaw_over_f32": med["ulaw_8k"] / med["f32_8k"] - 1, "f32_again_over_f32": med["f32_8k_again"] / med["f32_8k"] - 1,
                   "f32_spread": [min(res["f32_8k"] + res["f32_8k_again"]), max(res["f32_8k"] + res["f32_8k_again"])]}
    added = med["s16_16k"] - med["f32_16k"]
    out["b_16k"] = {"added_ms_per_tick": added, "added_us_per_launch": added * 1e3 / 2, "s16_over_f32": med["s16_16k"] / med["f32_16k"] - 1,
                    "f32_spread": [min(res["f32_16k"]), max(res["f32_16k"])]}
print(json.dumps(out))
