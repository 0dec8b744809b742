"""Time of slot snapshots (python3 tools/snapshot_time.py [max_slots]; default a 64-slot stream-set of the full configuration).

Exports and imports 1, 16 and 64 slots that are a few chunks into an utterance and prints, per count: bytes per slot, the median
microseconds of one export and of one import (device events around windows of back-to-back calls after a warm-up, so a call's host
side - checks, the call rows' upload - is inside the figure), the GB/s that is (blob bytes moved per second; each byte is read once and
written once) and, in the same run, the time of one device-to-device hipMemcpyAsync (a contiguous uint8 Tensor.copy_) of a buffer of
the same total bytes.  Expectation to check: pack / unpack within 2x of the plain copy."""
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from conan_amd import configs, synth  # noqa: E402
from conan_amd.runtime import Context  # noqa: E402

S = int(sys.argv[1]) if len(sys.argv) > 1 else 64
chp, vhp = configs.conan_hparams(), configs.hifigan_hparams()
ctx = Context(chp, vhp, 0)
ctx.load_state_dict("emformer", synth.emformer_state_dict(chp, 0))
ctx.load_state_dict("conan", synth.conan_state_dict(chp, 0))
ctx.load_state_dict("hifigan", synth.hifigan_state_dict(vhp, 0))
ctx.finalize()
st = ctx.streams(S, max_frames=4, max_ref_frames=256)
slots = list(range(S))
st.reset(slots)
st.set_reference(slots, torch.from_numpy(synth.mel(40, 3, S)).cuda())
mel = torch.from_numpy(synth.mel(6 * 4 + 2, 7, S)).cuda()
for j in range(6):
    st.step(slots, mel[:, 4 * j:4 * j + 6].contiguous())
per = st.snapshot_bytes
print("stream-set of %d slots: state %.2f MB per slot, snapshot %d bytes per slot (%.1f %% of the state), layout id %016x"
      % (S, st.state_bytes / S / 1e6, per, 100.0 * per * S / st.state_bytes, st.layout_id))
WIN, CALLS = 15, 20


def timed(fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(WIN):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            fn()
        b.record()
        b.synchronize()
        us.append(1e3 * a.elapsed_time(b) / CALLS)
    return float(np.median(us)), float(min(us)), float(max(us))


for n in (1, 16, 64):
    if n > S:
        continue
    sl = slots[:n]
    blob = torch.empty(n, per, dtype=torch.uint8, device="cuda")
    snap = st.export_slots(sl, out=blob)
    used = sum(snap.info(i)["bytes"] for i in range(n))
    other = torch.empty(used, dtype=torch.uint8, device="cuda")
    src = torch.empty(used, dtype=torch.uint8, device="cuda")
    ex = timed(lambda: st.export_slots(sl, out=blob))
    im = timed(lambda: st.import_slots(sl, snap))
    cp = timed(lambda: other.copy_(src, non_blocking=True))
    print("%2d slots, %d bytes used per slot: export %.1f us (%.1f-%.1f) %.0f GB/s | import %.1f us (%.1f-%.1f) %.0f GB/s | memcpy of %d bytes %.1f us "
          "(%.1f-%.1f) %.0f GB/s | export / memcpy %.2f, import / memcpy %.2f"
          % (n, used // n, ex[0], ex[1], ex[2], used / ex[0] / 1e3, im[0], im[1], im[2], used / im[0] / 1e3, used, cp[0], cp[1], cp[2], used / cp[0] / 1e3,
             ex[0] / cp[0], im[0] / cp[0]))
st.close()
ctx.close()
