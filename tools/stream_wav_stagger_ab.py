"""64 pipelined streams at 64 DIFFERENT positions of their utterances, full model, synthetic weights:
`python tools/stream_wav_stagger_ab.py [steps] [repeats] [mode]` prints one JSON line (ms per 80 ms tick, medians, ratios).
  steady     one conan_step_wav_ragged_async call per tick (staggered) against 64 same-position slots through conan_step_wav_async
             (same), alternated within the run
  status_quo the same staggered streams served as one conan_step_wav_async call per distinct position (64 one-slot calls per tick)
  churn      one stream ending and one starting every tick (ragged calls; the slot list changes: pipeline drains)
mode = all (default) or steady (the ragged steady state alone: run it under `rocprofv3 --kernel-trace --stats` for
mel_stream_ragged_kernel's time per call, profiles/stream_wav_ragged_b64_kernel_stats.csv).  Each schedule is run once blocking to
record its calls, then replayed pipelined from a reset; only the ticks of the measured window are timed."""
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
ctx, chp, vhp = bench.build_context(0)
eng = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=257)
hop, seg = ctx.hop, ctx.cfg.emf_segment
L = seg * hop
rng = np.random.default_rng(0)
ref = torch.from_numpy(synth.mel(256, 4321, B)).cuda()


def tone(N, i):
    t = np.arange(N) / 16000.0
    return 0.3 * np.sin(2 * np.pi * (120 + 5 * i) * t) + 0.05 * rng.standard_normal(N)


def record(utts):
    """utts: list of (start tick, samples).  Runs the schedule blocking (lowest free slot per start, as infer_wav_staggered) and
    returns its ticks: (slots started, slots, wav [n, L] cuda, samples, final)."""
    eng.st.reset(eng.slots, which=15)
    eng.st.set_reference(eng.slots, ref)
    wavs = [torch.from_numpy(tone(n, u).astype(np.float32)) for u, (_, n) in enumerate(utts)]
    pending, free, live, ticks, tick = list(range(len(utts))), list(range(B)), {}, [], 0
    while pending or live:
        started = []
        while pending and utts[pending[0]][0] <= tick and free:
            u = pending.pop(0)
            live[u] = [free.pop(0), 0, False]
            started.append(live[u][0])
        if started:
            eng.st.reset(started, which=15)
        us = list(live)
        rows, sm, fi, was = torch.zeros(len(us), L), [], [], []
        for r, u in enumerate(us):
            slot, pos, fin = live[u]
            N = utts[u][1]
            last = (N - 1) // L * L
            was.append(fin)
            if pos < last:
                rows[r] = wavs[u][pos:pos + L]
                live[u][1] = pos + L
                sm.append(L), fi.append(0)
            elif not fin:
                rows[r, :N - pos] = wavs[u][pos:]
                live[u][1], live[u][2] = N, True
                sm.append(N - pos), fi.append(1)
            else:
                sm.append(0), fi.append(1)
        slots = [live[u][0] for u in us]
        rows = rows.cuda()
        if us:
            emit, _, _, _ = eng.st.step_wav_ragged(slots, rows, sm, fi)
            for u, e, f in zip(us, emit, was):
                if f and e == 0:
                    free.append(live.pop(u)[0])
                    free.sort()
        ticks.append((started, slots, rows, sm, fi))
        tick += 1
    torch.cuda.synchronize()
    return ticks


outs = [(torch.empty(B, seg, dtype=torch.int32, device="cuda"), torch.empty(B, seg, 80, device="cuda"), torch.empty(B, L, device="cuda")) for _ in range(8)]


def replay(ticks, lo, hi, per_position=False):
    """ms per tick over ticks [lo, hi) of a recorded schedule, pipelined, from a reset."""
    eng.st.reset(eng.slots, which=15)
    eng.st.set_reference(eng.slots, ref)
    t0 = None
    for j in range(hi):
        if j == lo:
            eng.st.join(); torch.cuda.synchronize(); t0 = time.perf_counter()
        started, slots, rows, sm, fi = ticks[j]
        if started:
            eng.st.reset(started, which=15)
        c, m, w = outs[j % 8]
        if per_position:
            for i, s in enumerate(slots):
                eng.st.step_wav_async([s], rows[i:i + 1, :sm[i]], final=bool(fi[i]), codes=c[i:i + 1], mel_out=m[i:i + 1], wav_out=w[i:i + 1])
        else:
            eng.st.step_wav_ragged_async(slots, rows, sm, fi, codes=c, mel_out=m, wav_out=w)
    eng.st.join(); torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (hi - lo) * 1e3


def run_same(pieces):
    eng.start_wav(ref)
    eng.st.step_wav_async(eng.slots, pieces[0])          # first call: no chunk
    for j in range(1, W + K + 1):
        if j == W + 1:
            eng.st.join(); torch.cuda.synchronize(); t0 = time.perf_counter()
        c, m, w = outs[j % 8]
        e, _, _, _ = eng.st.step_wav_async(eng.slots, pieces[j], codes=c, mel_out=m, wav_out=w)
        assert e == seg
    eng.st.join(); torch.cuda.synchronize()
    return (time.perf_counter() - t0) / K * 1e3


# staggered: slot i starts at tick i; the window starts when all 64 are in steady state
span = B + W + K + 2
stag = record([(i, span * L) for i in range(B)])
lo, hi = B + W, B + W + K
same = torch.from_numpy(np.stack([tone((W + K + 2) * L, i) for i in range(B)]).astype(np.float32)).cuda()
same_pieces = [same[:, j * L:(j + 1) * L].contiguous() for j in range(W + K + 2)]
res = {"ragged_staggered": [], "same_position": []}
if MODE == "all":
    res.update({"status_quo_per_position": [], "churn": []})
    # churn: utterances of 60 ticks, one starting every tick (one ending every tick once the first have drained)
    churn = record([(j, 60 * L - 100) for j in range(B + W + K + 70)])
    clo = 70
for r in range(REP):
    res["same_position"].append(run_same(same_pieces))
    res["ragged_staggered"].append(replay(stag, lo, hi))
    if MODE == "all":
        res["status_quo_per_position"].append(replay(stag, lo, lo + max(10, K // 4), per_position=True))
        res["churn"].append(replay(churn, clo, clo + K))
med = {k: float(np.median(v)) for k, v in res.items()}
out = {"streams": B, "steps": K, "ms_per_tick": res, "median": med, "ragged_over_same": med["ragged_staggered"] / med["same_position"] - 1}
if MODE == "all":
    out["status_quo_over_ragged"] = med["status_quo_per_position"] / med["ragged_staggered"]
    out["churn_over_ragged"] = med["churn"] / med["ragged_staggered"] - 1
print(json.dumps(out))
