"""Time of one conan_loud_norm call (python3 tools/loud_norm_time.py [rows] [seconds] [rate]; default 64 rows of 10 s at 16 kHz).

Device events around windows of back-to-back calls after a warm-up; prints the median window per call, the spread, and the time
of reading the input twice and writing it once at the HBM rate a float4 copy reaches on this part (6.29 TB/s) and at its
specification (8 TB/s).  Run it under `rocprofv3 --kernel-trace --stats -d <dir> -- python3 tools/loud_norm_time.py` for the
time per kernel."""
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from conan_amd import configs  # noqa: E402
from conan_amd.runtime import Context  # noqa: E402

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 64
secs = float(sys.argv[2]) if len(sys.argv) > 2 else 10.0
rate = int(sys.argv[3]) if len(sys.argv) > 3 else 16000
N = int(secs * rate)
ctx = Context(configs.conan_hparams(True), None, 0, False, True, False)
g = torch.Generator(device="cuda").manual_seed(0)
x = 0.05 * torch.randn(rows, N, device="cuda", generator=g)
x[:, N // 3:N // 2] *= 1e-3                                  # a quiet stretch: both gates have work
y = torch.empty_like(x)
for _ in range(5):
    ctx.loud_norm(x, rate, out=y)
torch.cuda.synchronize()
WIN, CALLS = 20, 25
ms = []
for _ in range(WIN):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        ctx.loud_norm(x, rate, out=y)
    b.record()
    b.synchronize()
    ms.append(a.elapsed_time(b) / CALLS)
ms = np.array(ms)
mb = rows * N * 4 * 3 / 1e6
print("conan_loud_norm, %d rows of %d samples at %d Hz: median %.1f us per call (min %.1f, max %.1f over %d windows of %d calls)"
      % (rows, N, rate, 1e3 * np.median(ms), 1e3 * ms.min(), 1e3 * ms.max(), WIN, CALLS))
print("two reads and one write of the input: %.1f MB = %.1f us at 6.29 TB/s (measured copy rate), %.1f us at 8 TB/s (specification)"
      % (mb, mb / 6.29, mb / 8.0))
print("LUFS of row 0: %.4f -> %.4f" % (ctx.loudness(x[0], rate).item(), ctx.loudness(y[0], rate).item()))
ctx.close()
