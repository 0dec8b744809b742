"""Cost of the output watermark (conan_streams_set_watermark) on 64 pipelined same-position wav-in streams, full model, synthetic
weights, and of its detector: `python tools/watermark_time.py [steps] [repeats] [--parent DIR]` prints one JSON line.
  ms_per_step   never / on / parent alternated within the run: a stream-set that never called the setter, one with the mark on every
                slot, and - with --parent DIR, a built checkout of the parent commit - the parent's library on the same input.  Each
                leg of each repeat is a child process of its own (the parent's tree needs its own libconan_hip.so and Python
                package, which one process cannot load beside this tree's), run one after the other: the mean interval between
                consecutive step completions (conan_step_clock), one figure per repeat;
  kernels       blocking calls under the profile hooks with the mark, the gate and the comfort fill on: watermark_embed_kernel's
                time per launch (64 rows of 1280 samples) beside comfort_fill_kernel's and resample_out_kernel's;
  detect        conan_watermark_detect on 64 rows of 10 s (s16), HIP events around the call's two launches (watermark_corr_kernel,
                watermark_peak_kernel), and on 64 rows of 4095 samples, which leaves the peak kernel's launch alone; and
                conan_watermark_embed on the same 64 rows of 10 s."""
import json
import os
import statistics
import subprocess
import sys

B = 64
W = 10


def leg(mode, K):
    """One leg in this process, with the tree in the working directory: -> dict(ms=..., kernels=..., detect=...)."""
    import numpy as np
    import torch

    sys.path.insert(0, ".")
    import bench
    from conan_amd import synth
    from conan_amd.engine import StreamingVoiceConversionEngine

    ctx, chp, vhp = bench.build_context(0)
    hop, seg = ctx.hop, ctx.cfg.emf_segment
    L = seg * hop
    rng = np.random.default_rng(0)
    ref = torch.from_numpy(synth.mel(256, 4321, B)).cuda()
    N = (W + K + 2) * L
    t = np.arange(N) / 16000.0
    x = np.stack([0.3 * np.sin(2 * np.pi * (120 + 5 * i) * t) * (np.sin(2 * np.pi * 3.0 * t + i) > 0) for i in range(B)]) + 1e-2 * rng.standard_normal((B, N))
    ps = [torch.from_numpy(x[:, j * L:(j + 1) * L].astype(np.float32)).cuda().contiguous() for j in range(W + K + 2)]
    eng = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=257)
    start = dict(watermark=dict(key=0x0123456789ABCDEF, id=0xBEEF)) if mode == "on" else {}
    st = eng.st
    eng.start_wav(ref, **start)
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
    out = dict(ms=statistics.fmean(iv))
    if mode == "on":
        out.update(blocking_legs(ctx, eng, st, ref, ps, start, rng))
    return out


def blocking_legs(ctx, eng, st, ref, ps, start, rng):
    """The kernels' blocking times: the step's launches under the profile hooks, the whole-signal calls under HIP events."""
    import ctypes as C

    import numpy as np
    import torch

    from conan_amd import _lib
    from conan_amd.runtime import _ptr, _stream

    out = {}
    eng.start_wav(ref, activity=True, comfort=True, out_rate=8000, out_format="ulaw", **start)
    for j in range(W):
        st.step_wav(eng.slots, ps[j])
    st.profile_begin()
    for j in range(W, W + 20):
        st.step_wav(eng.slots, ps[j])
    st.profile_end()
    names = ("watermark_embed_kernel", "comfort_fill_kernel", "activity_gate_kernel", "resample_out_kernel")
    out["kernels"] = {k[0]: {"us_per_launch": k[1] * 1e3 / k[3], "launches": k[3]} for k in st.profile_kernels() if k[0] in names}

    def timed(fn, reps=10):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))

    long = torch.from_numpy((0.2 * rng.standard_normal((B, 160000))).astype(np.float32)).cuda()
    marked = ctx.watermark_embed(long, key=1, id=2)
    s16 = ctx.convert_samples(marked, "f32", "s16")

    def detector(rows, n):
        sm = np.full(B, n, dtype=np.int64)
        kmax = max(n // 2048 - 1, 1)
        score = torch.empty(B, 2048, dtype=torch.int64, device="cuda")
        soft = torch.empty(B, kmax, dtype=torch.int64, device="cuda")
        hit = torch.empty(B, 16, dtype=torch.uint8, device="cuda")
        ld = rows.shape[1] // 2
        return lambda: _lib.check(ctx.lib.conan_watermark_detect(ctx.h, 1, 1, _ptr(rows), ld, B, sm.ctypes.data_as(C.c_void_p), _ptr(score), _ptr(soft), kmax,
                                                                 _ptr(hit), _stream()))

    out["detect"] = dict(rows=B, seconds=10, corr_and_peak=timed(detector(s16, 160000)), peak_alone_no_blocks=timed(detector(s16, 4095)),
                         embed_whole=timed(lambda: ctx.watermark_embed(long, out=marked, key=1, id=2)))
    out["detect"]["z"] = [r["z"] for r in ctx.watermark_detect(s16[:2], 1, format="s16")]
    return out


def child(mode, K, cwd):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", mode, str(K)], cwd=cwd, check=True, capture_output=True, text=True)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    args = sys.argv[1:]
    if args[:1] == ["--leg"]:
        print(json.dumps(leg(args[1], int(args[2]))))
        return
    parent = None
    if "--parent" in args:
        i = args.index("--parent")
        parent = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    K = int(args[0]) if len(args) > 0 else 60
    REP = int(args[1]) if len(args) > 1 else 3
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    legs = {"parent": ("never", parent)} if parent else {}
    legs.update(never=("never", here), on=("on", here))
    res, kernels, detect = {k: [] for k in legs}, None, None
    for _ in range(REP):
        for name, (mode, cwd) in legs.items():
            r = child(mode, K, cwd)
            res[name].append(r["ms"])
            kernels, detect = r.get("kernels", kernels), r.get("detect", detect)
    print(json.dumps({"streams": B, "steps": K, "repeats": REP, "ms_per_step": res, "median": {k: statistics.median(v) for k, v in res.items()},
                      "spread": {k: [min(v), max(v)] for k, v in res.items()}, "kernels": kernels, "detect": detect}))


if __name__ == "__main__":
    main()
