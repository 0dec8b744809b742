"""Pipelined 64-stream chunk steps fed precomputed mel (conan_step_async) against the same steps fed audio (conan_step_wav_async),
full model, synthetic weights: `python tools/stream_wav_ab.py [steps] [repeats]` prints one JSON line (ms per step, medians, ratio).
Under `rocprofv3 --kernel-trace --stats` it gives mel_stream_kernel's time per call (profiles/stream_wav_b64_kernel_stats.csv)."""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
import bench
from conan_amd.engine import StreamingVoiceConversionEngine
from conan_amd import synth

B, W, K, REP = 64, 10, int(sys.argv[1]) if len(sys.argv) > 1 else 60, int(sys.argv[2]) if len(sys.argv) > 2 else 3
ctx, chp, vhp = bench.build_context(0)
eng = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=257)
hop, seg = ctx.hop, ctx.cfg.emf_segment
L = seg * hop
N = (W + K + 2) * L
rng = np.random.default_rng(0)
t = np.arange(N) / 16000.0
wav = torch.from_numpy(np.stack([0.3 * np.sin(2 * np.pi * (120 + 5 * i) * t) + 0.05 * rng.standard_normal(N) for i in range(B)]).astype(np.float32)).cuda()
ref = torch.from_numpy(synth.mel(256, 4321, B)).cuda()
whole = ctx.wav2mel(wav)
chunks = [c for _, _, c in eng.chunks(whole)]
outs = [(torch.empty(B, seg, dtype=torch.int32, device="cuda"), torch.empty(B, seg, 80, device="cuda"), torch.empty(B, L, device="cuda")) for _ in range(8)]


def run_mel():
    eng.start(ref)
    for j in range(W + K):
        if j == W:
            eng.st.join(); torch.cuda.synchronize(); t0 = time.perf_counter()
        c, m, w = outs[j % 8]
        eng.st.step_async(eng.slots, chunks[j], w, codes=c, mel_out=m)
    eng.st.join(); torch.cuda.synchronize()
    return (time.perf_counter() - t0) / K * 1e3


def run_wav():
    eng.start_wav(ref)
    eng.st.step_wav_async(eng.slots, wav[:, :L].contiguous())        # first call: no chunk
    pieces = [wav[:, (j + 1) * L:(j + 2) * L].contiguous() for j in range(W + K)]
    for j in range(W + K):
        if j == W:
            eng.st.join(); torch.cuda.synchronize(); t0 = time.perf_counter()
        c, m, w = outs[j % 8]
        e, _, _, _ = eng.st.step_wav_async(eng.slots, pieces[j], codes=c, mel_out=m, wav_out=w)
        assert e == seg
    eng.st.join(); torch.cuda.synchronize()
    return (time.perf_counter() - t0) / K * 1e3


res = {"mel": [], "wav": []}
for r in range(REP):
    res["mel"].append(run_mel())
    res["wav"].append(run_wav())
med = {k: float(np.median(v)) for k, v in res.items()}
print(json.dumps({"ms_per_step": res, "median": med, "wav_over_mel": med["wav"] / med["mel"] - 1}))
