"""Signals of the echo-delay tests (tests/test_echo_delay_ref_cpu.py, tests/test_gpu_echo_delay.py): far ends, an echo path, and the
composed case in which the follow rule steers tests/echo_ref.py's canceller from tests/echo_delay_ref.py's reports.  numpy only,
fixed seeds; everything is generated here and nothing is read from a file."""
import numpy as np

from tests import echo_delay_ref as ER
from tests import echo_ref as CR

F32 = np.float32
RATE, SECONDS, PATH_TAPS = 16000, 6, 600
N = RATE * SECONDS


def white(seed, n=N, rms=0.1):
    return (np.random.default_rng(seed).standard_normal(n) * rms).astype(F32)


def speech_like(seed, n=N, rms=0.1):
    """Low-passed noise (a 16-tap moving average: most energy under 1 kHz) under a slow syllable-rate envelope with pauses."""
    rng = np.random.default_rng(seed)
    x = np.convolve(rng.standard_normal(n + 15), np.ones(16) / 16.0, "valid")
    t = np.arange(n) / RATE
    env = np.clip(np.sin(2 * np.pi * 3.1 * t + rng.uniform(0, 6.28)) + 0.3 * np.sin(2 * np.pi * 0.7 * t + rng.uniform(0, 6.28)), 0, None)
    x = x * env
    return (x * (rms / np.sqrt(np.mean(x ** 2)))).astype(F32)


def tone(freq=300.0, n=N, amp=0.1):
    return (amp * np.sin(2 * np.pi * freq * np.arange(n) / RATE)).astype(F32)


def path(seed, taps=PATH_TAPS, gain_db=-6.0):
    """A decaying random path of `taps` taps whose energy gain is gain_db."""
    rng = np.random.default_rng(seed)
    h = rng.standard_normal(taps) * np.exp(-np.arange(taps) / (taps / 6.0))
    return h * (10 ** (gain_db / 20.0) / np.sqrt(np.sum(h ** 2)))


def echo(far, h, bulk):
    """What the far end leaves in the microphone: far delayed by `bulk` samples (an int, or per sample an array) through h."""
    n = len(far)
    y = np.convolve(far.astype(np.float64), h)[:n]
    idx = np.arange(n) - bulk
    return np.where(idx >= 0, y[np.clip(idx, 0, n - 1)], 0.0).astype(F32)


def first_confirmed(track):
    """The index of the first frame whose report holds an estimate, or -1."""
    hit = np.nonzero(track[:, 0] >= 0)[0]
    return int(hit[0]) if len(hit) else -1


def peak_ratio(rep, n_lags):
    """pk * n_lags / s of a report row."""
    return rep[4] * n_lags / max(rep[5], 1)


# ---- the composed case: a path at bulk delay 3000 under a canceller of 1024 taps, calls of 1280 samples
COMPOSED = dict(seed=7, bulk=3000, taps=1024, call=1280, seconds=6)


def composed_signals():
    c = COMPOSED
    far = white(c["seed"], RATE * c["seconds"])
    mic = echo(far, path(c["seed"] + 100), c["bulk"])
    return mic, far


def composed_run(mic, far, follow, n_calls=None):
    """The numpy references call by call.  follow: apply the rule between calls (else the canceller keeps delay 0).
    -> (per call the canceller's stats [4], per call the delay in force AFTER the call, per call the estimator's report)"""
    c = COMPOSED
    can = CR.Canceller("f32", **dict(CR.defaults(RATE), taps=c["taps"]))
    est = ER.Estimator("f32", **ER.defaults(RATE))
    fk = dict(lead=RATE * 8 // 1000, hyst=RATE * 4 // 1000, max_age=64)
    stats, delays, reports = [], [], []
    calls = len(mic) // c["call"] if n_calls is None else n_calls
    for i in range(calls):
        lo, hi = i * c["call"], (i + 1) * c["call"]
        _, rep = est.apply(mic[lo:hi], far[lo:hi])
        _, _, st = can.apply(mic[lo:hi], far[lo:hi])
        if follow:
            d = ER.follow(rep[0], rep[1], can.delay, **fk)
            if d is not None:
                can.configure(**dict({f: getattr(can, f) for f in CR.FIELDS}, delay=d))
        stats.append(st)
        delays.append(can.delay)
        reports.append(rep)
    return np.asarray(stats, dtype=np.int64), delays, np.asarray(reports, dtype=np.int64)


def last_second_erle(stats):
    """ERLE in dB over the calls of the last second."""
    k = RATE // COMPOSED["call"]
    return CR.erle_db(stats[-k:, 0].sum(), stats[-k:, 1].sum())
