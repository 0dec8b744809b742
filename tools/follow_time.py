"""64 pipelined same-position wav-in streams with and without source-pitch following (conan_streams_set_pitch_follow), full model,
synthetic weights: `python tools/follow_time.py [steps] [repeats] [mode]` prints one JSON line.
Modes, alternated within the run when `all` (default):
  off, off_again   no slot ever followed (the stream-set never calls the setter): the yardstick and its own spread;
  follow           a second stream-set with every slot following: one f0_yin_kernel per emitting call behind the front-end launch
                   (256 frames per 64-stream step), and the decoder step reads the tracked contour.
Per mode: the mean interval between consecutive step completions (device events on the library's vocoder stream, conan_step_clock),
one figure per repeat.  `kernel` (part of `all`) runs blocking calls under the profile hooks and reports f0_yin_kernel's time per
launch beside the front-end's (mel_stream_kernel).  A library without the feature (an older commit's tree on sys.path) runs the `off`
modes only, which is how the figures of two commits are compared: alternate the two trees' runs on one machine."""
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
REP = int(sys.argv[2]) if len(sys.argv) > 2 else 5
MODE = sys.argv[3] if len(sys.argv) > 3 else "all"
W = 10
ctx, chp, vhp = bench.build_context(0)
HAS = hasattr(ctx, "f0")
hop, seg = ctx.hop, ctx.cfg.emf_segment
L = seg * hop
rng = np.random.default_rng(0)
ref = torch.from_numpy(synth.mel(256, 4321, B)).cuda()
N = (W + K + 2) * L
t = np.arange(N) / 16000.0
x = torch.from_numpy(np.stack([0.3 * np.sin(2 * np.pi * (120 + 5 * i) * t) + 0.1 * np.sin(2 * np.pi * (240 + 10 * i) * t) + 0.02 * rng.standard_normal(N) for i in range(B)]).astype(np.float32)).cuda()
ps = [x[:, j * L:(j + 1) * L].contiguous() for j in range(W + K + 2)]
engines = {"off": StreamingVoiceConversionEngine(ctx, B, max_ref_frames=257)}
if HAS:
    engines["follow"] = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=257)


def run(mode):
    eng = engines["follow" if mode == "follow" else "off"]
    if mode == "follow":
        eng.start_wav(ref, follow=True)
    else:
        eng.start_wav(ref)
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


def kernel_times():
    """Blocking calls under the profile hooks -> {kernel: us per launch} of the launch following adds and of the front-end's."""
    eng = engines["follow"]
    eng.start_wav(ref, follow=True)
    st = eng.st
    for j in range(W):
        st.step_wav(eng.slots, ps[j])
    st.profile_begin()
    for j in range(W, W + 20):
        st.step_wav(eng.slots, ps[j])
    st.profile_end()
    return {k[0]: {"us_per_launch": k[1] * 1e3 / k[3], "launches": k[3]} for k in st.profile_kernels() if k[0] in ("f0_yin_kernel", "mel_stream_kernel")}


modes = [m for m in (["off", "follow", "off_again"] if MODE == "all" else [MODE]) if m != "kernel" and (HAS or m != "follow")]
res = {k: [] for k in modes}
for r in range(REP):
    for k in modes:
        res[k].append(run(k))
out = {"streams": B, "steps": K, "repeats": REP, "following": HAS, "ms_per_step": res, "median": {k: float(np.median(v)) for k, v in res.items()},
       "spread": {k: [min(v), max(v)] for k, v in res.items()}}
if HAS and MODE in ("all", "kernel"):
    out["kernels"] = kernel_times()
print(json.dumps(out))
