"""The five features whose per-slot state is an opaque device record that the setter takes back as seed rows - loss concealment, echo
cancellation, the echo-delay estimator, noise suppression, the watermark - share one host path for the seed rows and the state query.
One table, one test: the query on a slot that is off, the row checks of the query and of the setter's seed (pointer, stride), the
fresh record of a slot just enabled, and a record handed to a second slot through rows wider than a record.  No kernel runs here: the
records are read as the setters and the queries leave them."""
import numpy as np
import pytest
import torch

from conan_amd import _lib
from conan_amd.runtime import _i32, _ptr, _stream
from tests import echo_delay_ref as ED
from tests import echo_ref as EC
from tests.test_gpu_pitch import full  # noqa: F401  (module fixture: the small synthetic full model)

pytestmark = pytest.mark.gpu

ECHO = dict(taps=128, delay=3, mu_shift=2, dt_num=1, dt_den=2, hang=2, reg=4096, far_min=1024)
DELAY = dict(n_lags=320, thr=16, leak=3, ratio=4, min_peak=8, hold=2, tol=2)
# name (conan_streams_set_<name>, conan_streams_<name>_state, conan_<name>_state_bytes), the reader's Streams method, a minimal enabled
# cfg, the fresh record (None: zeros), and the bytes of a seeded record that the setter clears (echo delay: A[n_lags ..])
FEATURES = [
    ("conceal", "conceal_state", lambda: _lib.conceal_cfg(16000), None, None),
    ("echo", "echo_state", lambda: _lib.echo_cfg(**ECHO), lambda: EC.Canceller("f32", **ECHO).record(), None),
    ("echo_delay", "echo_delay_state", lambda: _lib.echo_delay_cfg(**DELAY), lambda: ED.Estimator("f32", **DELAY).record(),
     slice(64 + 4 * DELAY["n_lags"], 64 + 4 * ED.MAX_LAGS)),
    ("denoise", "denoise_state", lambda: _lib.denoise_cfg(), None, None),
    ("watermark", "watermark_state", lambda: _lib.watermark_cfg(key=0x1234567, id=7), None, None),
]


def _refused(call, code):
    with pytest.raises(_lib.ConanError) as e:
        call()
    assert e.value.code == code, (e.value.code, code)


@pytest.mark.parametrize("name,reader,cfg,fresh,cleared", FEATURES, ids=[f[0] for f in FEATURES])
def test_seed_rows_and_state_query(full, name, reader, cfg, fresh, cleared):
    st = full.streams(8, 4, 64)
    st.reset(list(range(8)))
    setter, read = getattr(st, "set_" + name), getattr(st, reader)
    query = getattr(st.lib, "conan_streams_%s_state" % name)
    nbytes = int(getattr(st.lib, "conan_%s_state_bytes" % name)())
    _refused(lambda: read([2]), _lib.ERR_STATE)      # a stream-set that never had the feature
    setter([2], cfg())
    _refused(lambda: read([2, 3]), _lib.ERR_STATE)      # ... and a slot that is off beside one that is on
    want = np.zeros(nbytes, dtype=np.uint8) if fresh is None else fresh()
    assert want.shape == (nbytes,) and np.array_equal(read([2])[0].cpu().numpy(), want)      # the fresh record of a slot just enabled

    # two different records of arbitrary bytes go into slots 5 and 7 from rows bytes + 64 apart, and read back as they went in -
    # each alone, and both in one query, in either order and beside the fresh one (the rows' strides are used on both sides)
    rng = np.random.default_rng(len(name))
    recs = rng.integers(0, 256, (2, nbytes), dtype=np.uint8)
    recs[:, :8] = 0      # (the canceller and the estimator read their position here: a multiple of every block)
    if cleared is not None:
        recs[:, cleared] = 0
    assert not np.array_equal(recs[0], recs[1])
    rec = recs[0]
    seed = torch.zeros(3, nbytes + 64, dtype=torch.uint8, device="cuda")
    seed[1:, :nbytes] = torch.from_numpy(recs).cuda()
    setter([5, 7], cfg(), seed=seed[1:])
    assert seed[1:].stride(0) == nbytes + 64
    assert np.array_equal(read([5])[0].cpu().numpy(), recs[0]) and np.array_equal(read([7])[0].cpu().numpy(), recs[1])
    assert np.array_equal(read([7, 2, 5]).cpu().numpy(), np.stack([recs[1], want, recs[0]]))
    assert np.array_equal(read([2])[0].cpu().numpy(), want)

    # refused rows change nothing: a pointer off by 4 bytes, a stride smaller than the record, a stride that is no multiple of 8
    a, p = _i32([5])
    flat = torch.zeros(2 * nbytes + 64, dtype=torch.uint8, device="cuda")
    assert flat.data_ptr() % 8 == 0
    for rows, ld in ((flat[4:], nbytes), (flat, nbytes - 8), (flat, nbytes + 4)):
        _refused(lambda: _lib.check(query(st.h, p, 1, _ptr(rows), ld, _stream())), _lib.ERR_INVALID)
        bad = torch.as_strided(rows, (1, max(ld, 1)), (ld, 1))      # the setter reads the stride off the tensor
        _refused(lambda: setter([5], cfg(), seed=bad), _lib.ERR_INVALID)
        _refused(lambda: setter([6], cfg(), seed=bad), _lib.ERR_INVALID)
    torch.cuda.synchronize()
    assert not flat.any()      # no refused query wrote a row
    assert np.array_equal(read([5])[0].cpu().numpy(), rec) and np.array_equal(read([2])[0].cpu().numpy(), want)
    _refused(lambda: read([6]), _lib.ERR_STATE)      # the refused setter enabled nothing
    st.close()
