"""Cost of silence trimming (conan_trim_silence) on whole signals: `python tools/trim_time.py [rows] [seconds]` prints one JSON line.
64 rows of 60 s at 16 kHz by default (3001 frames per row), speech-like on / off signals so that the cuts fall inside the rows.
  forms       us per call (device events around 20 calls, the median of 5 such groups) of the three forms of the call on the same rows
              and the same flags: plan only with the caller's flags (the table upload and trim_plan_kernel), the caller's flags with
              audio (+ trim_gather_kernel), and the detector form (+ activity_kernel);
  launches    the differences between the forms: us per launch of trim_gather_kernel and of activity_kernel beside trim_plan_kernel's
              call;
  gather      the bytes trim_gather_kernel moves - every sample of a row read once, every sample of it written once (the kept
              frames' samples, zeros behind them) - per second, and that as a fraction of `hbm_copy_gbs`, the float4 copy rate
              measured on this part (6.29 TB/s of the 8 TB/s peak)."""
import ctypes as C
import json
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
import bench
from conan_amd import _lib
from conan_amd.runtime import mel_cfg

ROWS = int(sys.argv[1]) if len(sys.argv) > 1 else 64
SECONDS = float(sys.argv[2]) if len(sys.argv) > 2 else 60.0
HBM_COPY_GBS = 6290.0      # MI355X: measured float4 copy rate
HOP, FFT = 320, 1024
ctx, _, _ = bench.build_context(0)
N = int(SECONDS * 50 * HOP)
F = 1 + N // HOP
rng = np.random.default_rng(0)
t = np.arange(N) / (50.0 * HOP)
# a tone that a 0.4 Hz square wave switches, over line noise: pauses of 1.25 s, which the default widths cut down to 0.36 s
x = torch.from_numpy(np.stack([(0.3 * np.sin(2 * np.pi * (120 + 5 * i) * t) * (np.sin(2 * np.pi * 0.4 * t + i) > 0) + 1e-3 * rng.standard_normal(N))
                               for i in range(ROWS)]).astype(np.float32)).cuda()
out = torch.empty_like(x)
mask = torch.empty(ROWS, F, dtype=torch.int32, device="cuda")
off = torch.empty(ROWS, F, dtype=torch.int64, device="cuda")
out_len = torch.empty(ROWS, dtype=torch.int64, device="cuda")
mc = mel_cfg(fft_size=FFT, hop_size=HOP, win_length=FFT, sample_rate=50 * HOP)
ac, tc = _lib.activity_cfg(), _lib.trim_cfg()
flags = ctx.activity(x, cfg=ac, fft_size=FFT, hop_size=HOP, state=False)[0].contiguous()


def call(detector, audio):
    _lib.check(ctx.lib.conan_trim_silence(ctx.h, C.byref(mc), C.byref(ac) if detector else None, C.byref(tc), C.c_void_p(x.data_ptr()), N, ROWS, N, None,
                                          None if detector else C.c_void_p(flags.data_ptr()), 0 if detector else F,
                                          C.c_void_p(out.data_ptr()) if audio else None, N, C.c_void_p(mask.data_ptr()), C.c_void_p(off.data_ptr()), F,
                                          C.c_void_p(out_len.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))


def timed(fn):
    for _ in range(3):
        fn()
    groups = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(20):
            fn()
        b.record()
        torch.cuda.synchronize()
        groups.append(a.elapsed_time(b) * 1e3 / 20)
    return float(np.median(groups)), groups


call(True, True)      # (the workspace grows to its largest form once, outside the timed groups)
forms = {}
for name, det, audio in (("plan_only_caller_flags", False, False), ("caller_flags", False, True), ("detector", True, True)):
    us, groups = timed(lambda: call(det, audio))
    forms[name] = {"us_per_call": us, "us_groups": groups}
call(False, True)
kept_f = int(out_len.sum().item())
call(True, True)
kept_d = int(out_len.sum().item())
assert kept_f == kept_d      # the detector form runs the same kernel as Context.activity: the same flags, the same cuts
gather_us = forms["caller_flags"]["us_per_call"] - forms["plan_only_caller_flags"]["us_per_call"]
moved = 2 * ROWS * N * 4
print(json.dumps({"rows": ROWS, "seconds": SECONDS, "frames": F, "kept_fraction": kept_f / (ROWS * N), "forms": forms,
                  "launches": {"trim_plan_kernel_call_us": forms["plan_only_caller_flags"]["us_per_call"], "trim_gather_kernel_us": gather_us,
                               "activity_kernel_us": forms["detector"]["us_per_call"] - forms["caller_flags"]["us_per_call"]},
                  "gather": {"bytes": moved, "gbs": moved / (gather_us * 1e-6) / 1e9, "hbm_copy_gbs": HBM_COPY_GBS,
                             "fraction_of_hbm_copy_rate": moved / (gather_us * 1e-6) / (HBM_COPY_GBS * 1e9)}}))
