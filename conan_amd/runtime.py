"""Thin Python handles over the C-ABI: Context (weights) and Streams (per-slot state).

PyTorch-ROCm is used only as the device-memory / stream plumbing: every tensor argument is a
CUDA(=HIP) torch tensor whose data_ptr() is handed to libconan_hip.so, and work is enqueued on
torch's current HIP stream.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib


def _require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError("conan_amd needs a HIP device (MI355X); there is no CPU fallback")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _i32(a):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.int32))
    return a, a.ctypes.data_as(C.c_void_p)


def _struct_rows(buf, State):
    """uint8 [n, sizeof(State)] on the device -> a list of dicts of the State struct's fields but `reserved` (synchronises)."""
    raw = buf.cpu().numpy().tobytes()
    size = C.sizeof(State)
    states = [State.from_buffer_copy(raw[i * size:(i + 1) * size]) for i in range(buf.shape[0])]
    return [{name: getattr(s, name) for name, _ in State._fields_ if name != "reserved"} for s in states]


def _feature_cfg(f, cfg, kw, defaults=()):
    """The Cfg struct of a setter of feature f (an _lib.SlotFeature) from its (cfg, **kw): None is the zeroed struct, "off", and takes
    no keywords; a struct passes; True, a dict and the keywords go to the feature's builder over the method's own `defaults`, a dict's
    entries over those and the keywords over the dict's."""
    if cfg is None:
        if kw and f.noun:
            raise ValueError(f"{f.method}: cfg=None turns {f.noun} off and takes no keywords")
        return f.cfg()
    if isinstance(cfg, f.cfg):
        return cfg
    return f.build(**dict(defaults, **dict({} if cfg is True else cfg, **kw)))


# torch dtype of a row in each sample format (conan_streams_set_input_format / _output_format, conan_convert_samples)
SAMPLE_DTYPES = {"f32": torch.float32, "s16": torch.int16, "ulaw": torch.uint8, "alaw": torch.uint8}


def _row_bytes(rows, n, ld, device):
    """Rows of samples (1-D tensors, or one 2-D tensor) packed from the start of rows `ld` * 4 bytes apart: uint8 [n, ld * 4]."""
    buf = torch.zeros(n, ld * 4, dtype=torch.uint8, device=device)
    if isinstance(rows, torch.Tensor):
        if rows.shape[1]:
            buf.view(rows.dtype)[:, :rows.shape[1]] = rows
    else:
        for i, r in enumerate(rows):
            if r.numel():
                buf[i].view(r.dtype)[:r.numel()] = r
    return buf


def _rate_cfg(key, cfg, rate=None):
    """An enabled Cfg struct of a feature of _lib.SLOT_FEATURES whose defaults follow the input rate (conceal, echo, echo_delay), of:
    one itself; True (the defaults of `rate`); an integer rate; a dict of fields over the defaults of `rate` (without a rate every
    field must be given)."""
    f = _lib.SLOT_FEATURES[key]
    if isinstance(cfg, f.cfg):
        return cfg
    if cfg is True:
        if rate is None:
            raise ValueError(f"{key}: True stands for a rate's defaults, and no rate is known here")
        return f.build(rate)
    if isinstance(cfg, dict):
        return f.build(rate, **cfg)
    if isinstance(cfg, (int, np.integer)) and not isinstance(cfg, bool):
        return f.build(int(cfg))
    raise ValueError(f"{key}: {cfg!r} is neither an _lib.{f.cfg.__name__}, a dict of its fields, a rate nor True")


def _pack_signals(who, fmt, dev, lengths, **rows):
    """The whole-signal calls' rows (keyword -> [..., N] samples of format `fmt`, all of one shape) packed for the library ->
    (the format's code, the packed uint8 buffers in the keywords' order, the leading shape, n, N, the row stride in dwords, the
    int64 lengths: `lengths` per row, default N)."""
    f = _lib.sample_format(fmt)
    rows = {k: v.to(dev) for k, v in rows.items()}
    first = next(iter(rows.values()))
    if any(v.dtype != SAMPLE_DTYPES[fmt] or v.shape != first.shape for v in rows.values()):
        got = " and ".join(f"{v.dtype} {tuple(v.shape)}" for v in rows.values())
        raise ValueError(f"{who}: format {fmt!r} takes {SAMPLE_DTYPES[fmt]} samples in {' and '.join(rows)} rows of one shape, got {got}")
    lead, N = first.shape[:-1], first.shape[-1]
    n = int(np.prod(lead)) if len(lead) else 1
    ld = max((N * _lib.SAMPLE_BYTES[fmt] + 3) // 4, 1)
    bufs = [_row_bytes(v.reshape(n, N), n, ld, dev) for v in rows.values()]
    sm = np.full(n, N, dtype=np.int64) if lengths is None else np.ascontiguousarray(np.asarray(lengths, dtype=np.int64).reshape(n))
    return f, bufs, lead, n, N, ld, sm


def mel_cfg(fft_size=1024, hop_size=320, win_length=1024, num_mels=80, fmin=80, fmax=7600, sample_rate=16000, eps=1e-6,
            mel_vmin=-6.0, mel_vmax=1.5, framing=0, natural_log=False, mag_eps=0.0):
    """conan_mel_cfg with Context.wav2mel's defaults (inference/Conan.py:57-70)."""
    return _lib.MelCfg(fft_size, hop_size, win_length, num_mels, sample_rate, float(fmin), float(fmax), eps, mel_vmin, mel_vmax,
                       int(framing), int(bool(natural_log)), float(mag_eps))


class Context:
    """conan_ctx: packed weights of up to three models on one device."""

    def __init__(self, conan_hp=None, hifigan_hp=None, device=0, emformer=True, conan=True, hifigan=True):
        _require_gpu()
        self.lib = _lib.lib()
        self.cfg = _lib.make_cfg(conan_hp, hifigan_hp, emformer, conan, hifigan)
        self.device = int(device)
        self.conan_hp, self.hifigan_hp = conan_hp, hifigan_hp
        h = C.c_void_p()
        _lib.check(self.lib.conan_ctx_create(self.device, C.byref(self.cfg), C.byref(h)))
        self.h = h
        self.finalized = False

    def load_state_dict(self, model, sd):
        """model in {'emformer','conan','hifigan'}; sd maps the reference's state_dict keys to
        numpy arrays / torch tensors (utils/commons/ckpt_utils.py:26-66)."""
        for k, v in sd.items():
            a = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
            if a.dtype.kind != "f":
                continue
            a = np.ascontiguousarray(a, dtype=np.float32)
            shape = (C.c_int64 * max(1, a.ndim))(*a.shape)
            _lib.check(self.lib.conan_ctx_load_tensor(self.h, f"{model}.{k}".encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim))
        return self

    def finalize(self):
        _lib.check(self.lib.conan_ctx_finalize(self.h))
        self.finalized = True
        return self

    @property
    def hop(self):
        return self.lib.conan_hop_size(self.h)

    @property
    def weight_bytes(self):
        return self.lib.conan_ctx_weight_bytes(self.h)

    def wav2mel(self, wav, fft_size=1024, hop_size=320, win_length=1024, num_mels=80, fmin=80, fmax=7600, sample_rate=16000,
                eps=1e-6, mel_vmin=-6.0, mel_vmax=1.5, framing=0, natural_log=False, mag_eps=0.0):
        """Mel front-end on the GPU (conan_wav2mel): wav cuda float32 [n, samples] -> mel [n, frames, num_mels].
        Defaults: clip(librosa_wav2spec(wav)['mel'], mel_vmin, mel_vmax) of inference/Conan.py:57-70 (its loud_norm branch is
        Context.loud_norm, run on the waveform first),
        frames = 1 + samples // hop.  framing=1, natural_log=True, mag_eps=1e-9: the torch.stft front-end of
        inference/Conan_previous.py:100-121 (reflect padding, center=False), frames = samples // hop."""
        wav = wav.to(torch.device("cuda", self.device), torch.float32).contiguous()
        if wav.dim() == 1:
            wav = wav[None]
        n, samples = wav.shape
        mc = _lib.MelCfg(fft_size, hop_size, win_length, num_mels, sample_rate, float(fmin), float(fmax), eps, mel_vmin, mel_vmax,
                         int(framing), int(bool(natural_log)), float(mag_eps))
        if framing == 0:
            frames = 1 + samples // hop_size
        else:
            frames = max(0, (samples + 2 * ((fft_size - hop_size) // 2) - fft_size) // hop_size + 1)
        mel = torch.empty(n, frames, num_mels, device=wav.device)
        got = C.c_int32(0)
        _lib.check(self.lib.conan_wav2mel(self.h, C.byref(mc), _ptr(wav), n, samples, _ptr(mel), C.byref(got), _stream()))
        assert got.value == frames
        return mel

    def resample(self, x, orig_freq, new_freq=16000, lowpass_filter_width=6, rolloff=0.99, resampling_method="sinc_interp_hann", beta=None,
                 preset=None):
        """torchaudio.functional.resample on the GPU (conan_resample): x [..., N] float32 -> [..., ceil(new * N / orig)] with
        new / orig = new_freq / orig_freq reduced.  preset='hann' (torchaudio's defaults) or 'kaiser_best' (resampy's kaiser_best
        as torchaudio documents it) replaces the filter keywords.  orig_freq == new_freq returns a copy."""
        cfg = _lib.resample_cfg(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, beta, preset)
        x = x.to(torch.device("cuda", self.device), torch.float32).contiguous()
        lead, N = x.shape[:-1], x.shape[-1]
        n = int(np.prod(lead)) if len(lead) else 1
        nout = _lib.check(self.lib.conan_resample_length(C.byref(cfg), N))
        y = torch.empty(*lead, nout, device=x.device)
        if n and N:
            got = C.c_int64(0)
            _lib.check(self.lib.conan_resample(self.h, C.byref(cfg), _ptr(x), n, N, _ptr(y), C.byref(got), _stream()))
            assert got.value == nout
        return y

    def resample_drift(self, x, orig_freq, new_freq, drift, side="source", **filter):
        """conan_resample_drift: x [..., N] float32 resampled from orig_freq to new_freq with the far device's clock drift taken out -
        a windowed sinc at an arbitrary position (the law of include/conan_hip.h).  drift: ppm (> 0: the device runs fast), or a
        list of (output_index, ppm) that starts at output 0; ppm becomes the law's ppb by round(ppm * 1000).  side: 'source' (the
        device sampled x) or 'sink' (the device plays the result).  filter: Context.resample's filter keywords.  The filter runs at
        equal rates too, and drift 0 is not bit-equal to Context.resample."""
        cfg = _lib.resample_cfg(orig_freq, new_freq, **filter)
        sd = _lib.drift_side(side)
        at, ppb = _lib.drift_schedule(drift)
        x = x.to(torch.device("cuda", self.device), torch.float32).contiguous()
        lead, N = x.shape[:-1], x.shape[-1]
        n = int(np.prod(lead)) if len(lead) else 1
        nout = self.lib.conan_resample_drift_length(C.byref(cfg), sd, N, at.ctypes.data, ppb.ctypes.data, len(at))
        if nout < 0:
            raise ValueError("resample_drift: the library refuses this configuration or schedule")
        y = torch.empty(*lead, nout, device=x.device)
        if n and N:
            got = C.c_int64(0)
            _lib.check(self.lib.conan_resample_drift(self.h, C.byref(cfg), sd, _ptr(x), n, N, at.ctypes.data, ppb.ctypes.data, len(at), _ptr(y),
                                                     nout, C.byref(got), _stream()))
            assert got.value == nout
        return y

    def resample_drift_table(self, orig_freq, new_freq, **filter):
        """conan_resample_drift_table (host only): the law's f32 table as numpy [1025, 2W] - row p holds the taps at phase p / 1024."""
        return _lib.resample_drift_table(orig_freq, new_freq, **filter)

    def _loud_call(self, x, sample_rate, target, peak_limit, lengths, out, measure_only):
        """One conan_loud_norm call over the rows of x -> (y or None, stats float64 [n, 4], the leading shape)."""
        dev = torch.device("cuda", self.device)
        x = x.to(dev, torch.float32)
        lead, N = x.shape[:-1], x.shape[-1]
        n = int(np.prod(lead)) if len(lead) else 1
        if not (x.dim() == 2 and x.stride(1) == 1 and x.stride(0) >= N):      # (a 2-D view with a row stride is read in place)
            x = x.reshape(n, N).contiguous()
        lens = np.full(n, N, dtype=np.int64) if lengths is None else np.ascontiguousarray(np.asarray(lengths, dtype=np.int64).reshape(-1))
        if lens.shape[0] != n:
            raise ValueError(f"loud_norm: {lens.shape[0]} lengths for {n} rows")
        y = None
        if not measure_only:
            if out is not None:
                if not (out.is_cuda and out.dtype == torch.float32 and out.dim() == 2 and out.shape[0] == n and out.stride(1) == 1):
                    raise ValueError("loud_norm: out must be a cuda float32 [n, ld] buffer with unit column stride")
                y = out
            else:
                y = x.clone() if lengths is not None else torch.empty(n, N, device=dev)      # (the floats past a row's length stay x's)
        stats = torch.empty(n, 4, dtype=torch.float64, device=dev)
        cfg = _lib.LoudnessCfg(int(sample_rate), float(target), int(bool(peak_limit)), (C.c_int32 * 3)(0, 0, 0))
        _lib.check(self.lib.conan_loud_norm(self.h, C.byref(cfg), _ptr(x), x.stride(0), n, lens.ctypes.data_as(C.c_void_p), _ptr(y),
                                            y.stride(0) if y is not None else 0, _ptr(stats), _stream()))
        return y, stats, lead

    def loud_norm(self, x, sample_rate, target=-22.0, peak_limit=True, lengths=None, return_stats=False, out=None):
        """The reference's loud_norm (librosa_wav2spec, utils/audio/__init__.py:58-63) on the GPU (conan_loud_norm): x [..., N] float32
        at `sample_rate` -> the rows measured with a BS.1770 meter, scaled to `target` LUFS and, with peak_limit, divided by their
        peak where that exceeds 1.  lengths: samples per row (default N; the floats past a row's length come back as x's).  A row
        without a loudness (silence, or nothing above the meter's absolute gate) comes back unchanged; a row shorter than 0.4 s is an
        error.  return_stats: also the float64 [..., 4] stats (LUFS, gain applied, peak before limiting, blocks in the gated set).
        out: a cuda float32 [n, ld] buffer to write the rows into (it may be x itself: in place); only the first lengths[i] floats
        of a row are written."""
        y, stats, lead = self._loud_call(x, sample_rate, target, peak_limit, lengths, out, False)
        if out is None:
            y = y.reshape(*lead, y.shape[-1])
        return (y, stats.reshape(*lead, 4)) if return_stats else y

    def loudness(self, x, sample_rate, lengths=None):
        """Integrated loudness (BS.1770, as pyloudnorm's Meter.integrated_loudness) of the rows of x [..., N] -> float64 [...] LUFS
        (-inf for a row with nothing above the absolute gate).  A measure-only conan_loud_norm call."""
        _, stats, lead = self._loud_call(x, sample_rate, -22.0, True, lengths, None, True)
        return stats[:, 0].reshape(*lead) if len(lead) else stats[0, 0]

    def level(self, x, target=-22.0, max_boost_db=20.0, max_cut_db=40.0, initial_gain_db=0.0, window_blocks=_lib.LEVEL_MAX_BLOCKS,
              peak_limit=True, clip=False, lengths=None, return_trace=False, out=None):
        """The streaming leveller's law on whole signals (conan_level; include/conan_hip.h, conan_level_cfg): x [..., N] float32 at
        the model rate (hop * 50) -> the rows as a wav-in slot with Streams.set_input_level(**cfg) hands them to its front-end, bit
        for bit.  A causal BS.1770 meter read every segment * hop samples steers a gain towards `target` LUFS within
        [-max_cut_db, +max_boost_db], from initial_gain_db, over the last window_blocks 100 ms blocks; peak_limit keeps the gain
        times the peak so far at or under 1, clip clamps the samples to [-1, 1].  The defaults are a choice, not a measurement.
        lengths: samples per row (default N; the floats past a row's length come back as x's).  return_trace: also the float64
        [..., ceil(N / U), 2] rows (L_k, G_k) of the update instants (rows past a shorter row's last instant are NaN).  out: a cuda
        float32 [n, ld] buffer to write the rows into (it may be x itself: in place)."""
        dev = torch.device("cuda", self.device)
        x = x.to(dev, torch.float32)
        lead, N = x.shape[:-1], x.shape[-1]
        n = int(np.prod(lead)) if len(lead) else 1
        if not (x.dim() == 2 and x.stride(1) == 1 and x.stride(0) >= N):
            x = x.reshape(n, N).contiguous()
        lens = np.full(n, N, dtype=np.int64) if lengths is None else np.ascontiguousarray(np.asarray(lengths, dtype=np.int64).reshape(-1))
        if lens.shape[0] != n:
            raise ValueError(f"level: {lens.shape[0]} lengths for {n} rows")
        if out is not None:
            if not (out.is_cuda and out.dtype == torch.float32 and out.dim() == 2 and out.shape[0] == n and out.stride(1) == 1):
                raise ValueError("level: out must be a cuda float32 [n, ld] buffer with unit column stride")
            y = out
        else:
            y = x.clone() if lengths is not None else torch.empty(n, N, device=dev)
        U = self.cfg.emf_segment * self.hop
        K = max(1, -(-N // U)) if U > 0 else 1
        trace = torch.full((n, K, 2), float("nan"), dtype=torch.float64, device=dev) if return_trace else None
        cfg = _lib.level_cfg(target, max_boost_db, max_cut_db, initial_gain_db, window_blocks, peak_limit, clip)
        _lib.check(self.lib.conan_level(self.h, C.byref(cfg), _ptr(x), x.stride(0), n, lens.ctypes.data_as(C.c_void_p), _ptr(y), y.stride(0),
                                        _ptr(trace), K, _stream()))
        if out is None:
            y = y.reshape(*lead, y.shape[-1])
        return (y, trace.reshape(*lead, K, 2)) if return_trace else y

    def eq(self, x, sections=None, cfg=None, lengths=None, rate=None, seed=None, return_state=False, out=None):
        """The equaliser on whole signals (conan_eq; include/conan_hip.h, conan_eq_cfg), one launch: x [n, N] (or [N]) float32 -> the
        rows through a cascade of 1 .. 4 biquad sections in f64.  sections: raw 5-tuples (b0, b1, b2, a1, a2) or dicts
        (kind=, f=, q=, gain_db=) designed at `rate` Hz (default: the model rate, 50 * hop); or cfg: an _lib.EqCfg.  A 2-D view whose
        rows are contiguous keeps its row stride.  lengths: samples per row (default N; the floats behind a row's length come back
        as x's).  seed: uint8 [n, 592] (cuda) rows of conan_eq_state the rows continue from, with the cfg's origin and pos naming
        their origin and position (eq_cfg(..., origin=, pos=)); None: every row starts from zero.  out: a cuda float32 [n, ld]
        buffer (it may be x itself: in place).  -> y, and with return_state=True (y, states uint8 [n, 592]): a signal cut anywhere and
        chained through the state gives the whole signal's bits."""
        dev = torch.device("cuda", self.device)
        c = cfg if cfg is not None else _lib.eq_cfg(sections, rate=float(self.hop * 50 if rate is None else rate))
        v = x.to(dev, torch.float32)
        one = v.dim() == 1
        if one:
            v = v[None]
        if v.dim() != 2:
            raise ValueError(f"eq: x must be [n, N] or [N], got {tuple(x.shape)}")
        n, N = v.shape
        if not (v.stride(1) == 1 and v.stride(0) >= N) and n * N:
            v = v.contiguous()
        x_ld = v.stride(0) if n > 1 else max(N, 1)
        lens = np.full(n, N, dtype=np.int64) if lengths is None else np.ascontiguousarray(np.asarray(lengths, dtype=np.int64).reshape(-1))
        if lens.shape[0] != n or lens.min(initial=0) < 0 or lens.max(initial=0) > N:
            raise ValueError(f"eq: lengths must be {n} values in 0 .. {N}")
        if out is not None:
            y = out if out.dim() == 2 else out[None]
            if not (y.is_cuda and y.dtype == torch.float32 and y.shape[0] == n and y.shape[1] >= N and (y.stride(1) == 1 or y.shape[1] <= 1)):
                raise ValueError("eq: out must be a cuda float32 [n, >= N] buffer with unit column stride")
        else:
            y = v.clone() if lengths is not None else torch.empty(n, N, dtype=torch.float32, device=dev)
        y_ld = y.stride(0) if n > 1 else max(y.shape[1], 1)
        size = C.sizeof(_lib.EqState)
        if seed is not None and (seed.dtype != torch.uint8 or not seed.is_cuda or tuple(seed.shape) != (n, size) or not seed.is_contiguous()):
            raise ValueError(f"eq: seed must be a contiguous cuda uint8 [{n}, {size}] tensor, as return_state=True returns it")
        st = torch.empty(n, size, dtype=torch.uint8, device=dev) if return_state else None
        if n:
            _lib.check(self.lib.conan_eq(self.h, C.byref(c), _ptr(v), x_ld, n, lens.ctypes.data_as(C.c_void_p), _ptr(y), y_ld, _ptr(st), _ptr(seed), _stream()))
        if out is None and one:
            y = y[0]
        return (y, st) if return_state else y

    def f0(self, wav, fmin=50.0, fmax=900.0, threshold=0.15, floor_db=-60.0, fft_size=1024, hop_size=None):
        """The source-pitch tracker on whole signals (conan_f0; include/conan_hip.h, conan_f0_cfg): wav [..., N] float32 at the model
        rate (50 * hop_size; hop_size defaults to the vocoder's hop) -> (f0 [..., 1 + N // hop_size] in log2 Hz, 0 where unvoiced;
        uv [..., frames] 0 | 1): YIN on the mel front-end's centred frames of fft_size samples.  It is what a following wav-in slot
        (Streams.set_pitch_follow) hands its decoder steps, bit for bit."""
        dev = torch.device("cuda", self.device)
        x = wav.to(dev, torch.float32).contiguous()
        lead, N = x.shape[:-1], x.shape[-1]
        n = int(np.prod(lead)) if len(lead) else 1
        hop = int(hop_size or self.hop)
        mc = mel_cfg(fft_size=fft_size, hop_size=hop, win_length=fft_size, sample_rate=50 * hop)
        cfg = _lib.f0_cfg(fmin, fmax, threshold, floor_db)
        frames = 1 + N // hop
        f0 = torch.empty(n, frames, device=dev)
        uv = torch.empty(n, frames, device=dev)
        got = C.c_int32(0)
        _lib.check(self.lib.conan_f0(self.h, C.byref(mc), C.byref(cfg), _ptr(x), n, N, _ptr(f0), _ptr(uv), C.byref(got), _stream()))
        assert got.value == frames
        return f0.reshape(*lead, frames), uv.reshape(*lead, frames)

    def f0_register(self, f0, uv, target=None, max_shift=2.0, prior=None, prior_frames=50, seed=None, lengths=None):
        """Register matching on whole contours (conan_f0_register; include/conan_hip.h, conan_register_cfg): f0 / uv [..., T] as
        Context.f0 returns them -> (matched [..., T], state [..., 2] int64 = (n, S) after each row): the causal log-f0 mean transform
        that moves each row's mean log-f0 towards `target` (log2 Hz).  The estimate starts from seed = (count, sum) or from
        prior_frames frames at `prior` (default: the target).  target=None is the pure measurement: no contour comes back (None) and
        the estimate starts from (0, 0) unless a seed or a prior is given; a row's mean is S / (n * 2^22).  lengths: frames per row
        (default T).  It is what a following wav-in slot with Streams.set_pitch_register hands its decoder steps, bit for bit."""
        dev = torch.device("cuda", self.device)
        x = f0.to(dev, torch.float32).contiguous()
        u = uv.to(dev, torch.float32).contiguous()
        if u.shape != x.shape:
            raise ValueError(f"f0_register: f0 {tuple(x.shape)} and uv {tuple(u.shape)} differ in shape")
        lead, T = x.shape[:-1], x.shape[-1]
        n = int(np.prod(lead)) if len(lead) else 1
        lens = np.full(n, T, dtype=np.int32) if lengths is None else np.ascontiguousarray(np.asarray(lengths, dtype=np.int32).reshape(-1))
        if lens.shape[0] != n:
            raise ValueError(f"f0_register: {lens.shape[0]} lengths for {n} rows")
        if target is None:
            cfg = _lib.register_cfg(0.0, max_shift, prior=prior, prior_frames=0 if prior is None else prior_frames, seed=seed)
        else:
            cfg = _lib.register_cfg(target, max_shift, prior=prior, prior_frames=prior_frames, seed=seed)
        out = torch.empty_like(x) if target is not None else None
        state = torch.empty(n, 2, dtype=torch.int64, device=dev)
        _lib.check(self.lib.conan_f0_register(self.h, C.byref(cfg), _ptr(x), _ptr(u), n, lens.ctypes.data_as(C.c_void_p), T, _ptr(out), _ptr(state),
                                              _stream()))
        return out, state.reshape(*lead, 2)

    def activity(self, wav, cfg=None, power=False, fft_size=1024, hop_size=None, state=True, **kw):
        """The source-activity detector on whole signals (conan_activity; include/conan_hip.h, conan_activity_cfg): wav [..., N] float32
        at the model rate (50 * hop_size; hop_size defaults to the vocoder's hop) -> (act [..., frames] int32 0 | 1, level [..., frames]
        int32 - the gate level after each frame, 2^20 = open -, state: a list with one dict per row (active, hang, level, floor, frames,
        active_frames) after the row), frames = 1 + N // hop_size; power=True appends the frame powers [..., frames] float64.  cfg: an
        _lib.ActivityCfg, or **kw = _lib.activity_cfg's keywords.  state=False: no state is fetched (None in its place), and the call
        does not synchronise.  It is what a wav-in slot with Streams.set_activity computes, bit
        for bit."""
        dev = torch.device("cuda", self.device)
        x = wav.to(dev, torch.float32).contiguous()
        lead, N = x.shape[:-1], x.shape[-1]
        n = int(np.prod(lead)) if len(lead) else 1
        hop = int(hop_size or self.hop)
        mc = mel_cfg(fft_size=fft_size, hop_size=hop, win_length=fft_size, sample_rate=50 * hop)
        c = cfg if cfg is not None else _lib.activity_cfg(**kw)
        frames = 1 + N // hop
        act = torch.empty(n, frames, dtype=torch.int32, device=dev)
        lvl = torch.empty(n, frames, dtype=torch.int32, device=dev)
        pw = torch.empty(n, frames, dtype=torch.float64, device=dev) if power else None
        sbuf = torch.empty(n, C.sizeof(_lib.ActivityState), dtype=torch.uint8, device=dev) if state else None
        got = C.c_int32(0)
        _lib.check(self.lib.conan_activity(self.h, C.byref(mc), C.byref(c), _ptr(x), n, N, _ptr(act), _ptr(lvl), _ptr(pw), _ptr(sbuf), C.byref(got),
                                           _stream()))
        assert got.value == frames
        out = (act.reshape(*lead, frames), lvl.reshape(*lead, frames), _struct_rows(sbuf, _lib.ActivityState) if state else None)
        return out + (pw.reshape(*lead, frames),) if power else out

    def activity_gate(self, wav, level, start_level=0, hop_size=None, out=None):
        """The gate's gain law on whole signals (conan_activity_gate): wav [..., N] float32 times the gain of level [..., >= ceil(N / hop)]
        int32 (the level after each frame, as Context.activity returns it; start_level: the level before frame 0) -> [..., N]; the
        level moves linearly inside a frame and 2^20 at both ends leaves the samples' bits alone.  out=wav gates in place."""
        dev = torch.device("cuda", self.device)
        x = wav.to(dev, torch.float32).contiguous()
        lv = level.to(dev, torch.int32).contiguous()
        lead, N = x.shape[:-1], x.shape[-1]
        n = int(np.prod(lead)) if len(lead) else 1
        if lv.shape[:-1] != lead:
            raise ValueError(f"activity_gate: wav {tuple(x.shape)} and level {tuple(lv.shape)} differ in their leading shape")
        y = torch.empty_like(x) if out is None else out
        if y.shape != x.shape or y.dtype != torch.float32 or not y.is_contiguous():
            raise ValueError("activity_gate: out must be a contiguous float32 tensor of wav's shape")
        _lib.check(self.lib.conan_activity_gate(self.h, int(hop_size or self.hop), _ptr(x), n, N, N, _ptr(lv), lv.shape[-1], int(start_level), _ptr(y),
                                                _stream()))
        return y

    def trim_silence(self, wav, lengths=None, flags=None, cfg=None, smooth_frames=12, max_silence_frames=18, norm=False, return_mask=False,
                     fft_size=1024, hop_size=None, activity_cfg=None, **activity_kw):
        """The reference's trim_long_sil on the GPU (conan_trim_silence; include/conan_hip.h, conan_trim_cfg): wav [..., N] float32 at
        the model rate (50 * hop_size; hop_size defaults to the vocoder's hop) -> (out [..., max(out_lengths)] float32: each row's
        kept frames moved together, zeros behind them; out_lengths: int64 numpy [...], the one host read of the call).  The frames
        are the detector's (1 + len // hop_size per row, 20 ms each); a frame is kept where the moving average of the flags over
        smooth_frames frames rounds to 1, or within a pause of at most max_silence_frames frames between such frames.  flags:
        int32 [..., >= frames] (any non-zero: active) - e.g. what a live call collected from Streams.step_wav_activity - instead of
        running the detector; else activity_cfg (an _lib.ActivityCfg) or **activity_kw (_lib.activity_cfg's keywords) configure
        Context.activity's detector, whose flags these then are bit for bit.  cfg: an _lib.TrimCfg instead of the two widths.
        lengths: samples per row (default N).  norm=True: the rows first go through loud_norm(target=-20.0, peak_limit=True), as the
        reference's trim_long_silences(norm=True) does, and the normalised, trimmed audio comes back.  return_mask=True appends
        the kept-frame mask int32 [..., frames] and the offsets int64 [..., frames] (where a kept frame's samples start in `out`;
        -1 for a dropped frame)."""
        dev = torch.device("cuda", self.device)
        x = wav.to(dev, torch.float32)
        lead, N = x.shape[:-1], x.shape[-1]
        n = int(np.prod(lead)) if len(lead) else 1
        if not (x.dim() == 2 and x.stride(1) == 1 and x.stride(0) >= N):      # (a 2-D view with a row stride is read in place)
            x = x.reshape(n, N).contiguous()
        hop = int(hop_size or self.hop)
        lens = None
        if lengths is not None:
            lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.int64).reshape(-1))
            if lens.shape[0] != n:
                raise ValueError(f"trim_silence: {lens.shape[0]} lengths for {n} rows")
        if flags is not None and (activity_cfg is not None or activity_kw):
            raise ValueError("trim_silence: flags= replaces the detector; its keywords make no sense beside them")
        if norm:
            x = self.loud_norm(x, 50 * hop, target=-20.0, peak_limit=True, lengths=lens)
        mc = mel_cfg(fft_size=fft_size, hop_size=hop, win_length=fft_size, sample_rate=50 * hop)
        tc = cfg if cfg is not None else _lib.trim_cfg(smooth_frames, max_silence_frames)
        frames = 1 + N // hop
        fl, ac = None, None
        if flags is not None:
            fl = flags.to(dev, torch.int32)
            if fl.shape[:-1] != lead:
                raise ValueError(f"trim_silence: wav {tuple(wav.shape)} and flags {tuple(fl.shape)} differ in their leading shape")
            fl = fl.reshape(n, fl.shape[-1]).contiguous()
        else:
            ac = activity_cfg if activity_cfg is not None else _lib.activity_cfg(**activity_kw)
        out = torch.zeros(n, N, device=dev)
        mask = torch.zeros(n, frames, dtype=torch.int32, device=dev) if return_mask else None
        off = torch.full((n, frames), -1, dtype=torch.int64, device=dev) if return_mask else None
        out_len = torch.empty(n, dtype=torch.int64, device=dev)
        _lib.check(self.lib.conan_trim_silence(self.h, C.byref(mc), C.byref(ac) if ac is not None else None, C.byref(tc), _ptr(x), x.stride(0), n, N,
                                               lens.ctypes.data_as(C.c_void_p) if lens is not None else None, _ptr(fl),
                                               fl.shape[1] if fl is not None else 0, _ptr(out), N, _ptr(mask), _ptr(off), frames, _ptr(out_len),
                                               _stream()))
        got = out_len.cpu().numpy()
        res = (out[:, :int(got.max())].reshape(*lead, -1), got.reshape(*lead) if len(lead) else got[0])
        return res + (mask.reshape(*lead, frames), off.reshape(*lead, frames)) if return_mask else res

    def bypass_mix(self, wet, dry, wet_levels, dry_levels, start=(_lib.ACTIVITY_FULL, 0), hop_size=None, out=None):
        """The bypass mix on whole signals (conan_bypass_mix; include/conan_hip.h, conan_bypass_cfg): wet [..., N] (the converted
        audio) and dry [..., N] (the source) float32, with the frame-end levels wet_levels / dry_levels [..., >= ceil(N / hop)] int32 in
        0 .. 2^20 (the dry ones are the effective levels, as Streams.step_wav_bypass returns them) and start = (wet0, dry0), the levels
        before frame 0 -> [..., N].  The levels move linearly inside a frame; full wet and no dry leaves wet's bits alone.  A 2-D
        operand whose rows are contiguous keeps its row stride (a view of a wider buffer is read in place); out=wet mixes in place.
        It is what a wav-in slot with Streams.set_bypass computes, bit for bit."""
        dev = torch.device("cuda", self.device)

        def rows(t, dtype):
            t = t.to(dev, dtype)
            if t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1]:
                return t, t.stride(0)
            t = t.contiguous()
            return t, t.shape[-1]

        x, x_ld = rows(wet, torch.float32)
        d, d_ld = rows(dry, torch.float32)
        lw, lw_ld = rows(wet_levels, torch.int32)
        ldv, ld_ld = rows(dry_levels, torch.int32)
        lead, N = x.shape[:-1], x.shape[-1]
        n = int(np.prod(lead)) if len(lead) else 1
        if d.shape != x.shape:
            raise ValueError(f"bypass_mix: wet {tuple(x.shape)} and dry {tuple(d.shape)} differ in shape")
        if lw.shape[:-1] != lead or ldv.shape != lw.shape:
            raise ValueError(f"bypass_mix: wet {tuple(x.shape)}, wet_levels {tuple(lw.shape)} and dry_levels {tuple(ldv.shape)} do not match")
        if ld_ld != lw_ld:
            ldv, lw = ldv.contiguous(), lw.contiguous()
            lw_ld = ld_ld = lw.shape[-1]
        if out is None:
            y, y_ld = torch.empty(x.shape, dtype=torch.float32, device=dev), N
        else:
            y, y_ld = (out, out.stride(0)) if out.dim() == 2 and out.stride(1) == 1 else (out, N)
            if y.shape != x.shape or y.dtype != torch.float32 or y.device != dev or not (y.is_contiguous() or (y.dim() == 2 and y.stride(1) == 1 and y_ld >= N)):
                raise ValueError("bypass_mix: out must be a float32 tensor of wet's shape on the device, contiguous or a 2-D view with contiguous rows")
        _lib.check(self.lib.conan_bypass_mix(self.h, int(hop_size or self.hop), _ptr(x), x_ld, _ptr(d), d_ld, n, N, _ptr(lw), _ptr(ldv), lw_ld,
                                             int(start[0]), int(start[1]), _ptr(y), y_ld, _stream()))
        return y

    def comfort_track(self, act, power, cfg=None, return_state=False, **kw):
        """The comfort noise's tracker on whole signals (conan_comfort_track; include/conan_hip.h, conan_comfort_cfg): act [..., F]
        int32 and power [..., F] float64 as Context.activity returns them -> the frame-end comfort levels [..., F] int32, every row
        from the cfg's start level.  cfg: an _lib.ComfortCfg, or **kw: _lib.comfort_cfg's keywords.  return_state=True appends the
        rows' states, a list of dict(level, idle_frames).  It is what a wav-in slot with Streams.set_comfort tracks, bit for bit."""
        dev = torch.device("cuda", self.device)
        c = cfg if cfg is not None else _lib.comfort_cfg(**kw)
        a = act.to(dev, torch.int32).contiguous()
        lead, F = a.shape[:-1], a.shape[-1]
        n = int(np.prod(lead)) if len(lead) else 1
        p = None
        if power is not None:
            p = power.to(dev, torch.float64).contiguous()
            if p.shape != a.shape:
                raise ValueError(f"comfort_track: act {tuple(a.shape)} and power {tuple(p.shape)} differ in shape")
        out = torch.empty(a.shape, dtype=torch.int32, device=dev)
        st = torch.empty(n, 16, dtype=torch.uint8, device=dev) if return_state else None
        _lib.check(self.lib.conan_comfort_track(self.h, C.byref(c), _ptr(a), _ptr(p), n, F, F, _ptr(out), _ptr(st), _stream()))
        if not return_state:
            return out
        return out, _struct_rows(st, _lib.ComfortState)

    def comfort_fill(self, wav, gate_levels, comfort_levels, cfg=None, seeds=None, start=(_lib.ACTIVITY_FULL, 0), pos0=0, hop_size=None, out=None, **kw):
        """The comfort noise's fill on whole signals (conan_comfort_fill): wav [..., N] float32 (the audio behind the gate and the
        mix) with the frame-end gate levels gate_levels [..., >= ceil(N / hop)] int32 in 0 .. 2^20 (Streams.step_wav_activity's) and
        comfort levels comfort_levels (Streams.step_wav_comfort's, or comfort_track's); start = (gate level, comfort level) before
        frame 0 -> [..., N].  Sample s of a row is sample pos0 + s of the white source.  cfg: an _lib.ComfortCfg, or **kw:
        _lib.comfort_cfg's keywords (colour, norm and seed are read); seeds: one seed per row instead of the cfg's.  A 2-D operand
        whose rows are contiguous keeps its row stride; out=wav fills in place.  An open gate keeps wav's bits.  It is what a wav-in
        slot with Streams.set_comfort computes, bit for bit."""
        dev = torch.device("cuda", self.device)
        c = cfg if cfg is not None else _lib.comfort_cfg(**kw)

        def rows(t, dtype):
            t = t.to(dev, dtype)
            if t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1]:
                return t, t.stride(0)
            t = t.contiguous()
            return t, t.shape[-1]

        x, x_ld = rows(wav, torch.float32)
        lg, lg_ld = rows(gate_levels, torch.int32)
        lc, lc_ld = rows(comfort_levels, torch.int32)
        lead, N = x.shape[:-1], x.shape[-1]
        n = int(np.prod(lead)) if len(lead) else 1
        if lg.shape[:-1] != lead or lc.shape != lg.shape:
            raise ValueError(f"comfort_fill: wav {tuple(x.shape)}, gate_levels {tuple(lg.shape)} and comfort_levels {tuple(lc.shape)} do not match")
        if lc_ld != lg_ld:
            lg, lc = lg.contiguous(), lc.contiguous()
            lg_ld = lc_ld = lg.shape[-1]
        sd = None
        if seeds is not None:
            sd = np.ascontiguousarray(np.asarray([int(v) & ((1 << 64) - 1) for v in seeds], dtype=np.uint64))
            if sd.shape[0] != n:
                raise ValueError(f"comfort_fill: {sd.shape[0]} seeds for {n} rows")
        if out is None:
            y, y_ld = torch.empty(x.shape, dtype=torch.float32, device=dev), N
        else:
            y, y_ld = (out, out.stride(0)) if out.dim() == 2 and out.stride(1) == 1 else (out, N)
            if y.shape != x.shape or y.dtype != torch.float32 or y.device != dev or not (y.is_contiguous() or (y.dim() == 2 and y.stride(1) == 1 and y_ld >= N)):
                raise ValueError("comfort_fill: out must be a float32 tensor of wav's shape on the device, contiguous or a 2-D view with contiguous rows")
        _lib.check(self.lib.conan_comfort_fill(self.h, int(hop_size or self.hop), C.byref(c), sd.ctypes.data_as(C.c_void_p) if sd is not None else None,
                                               _ptr(x), x_ld, n, N, int(pos0), _ptr(lg), _ptr(lc), lg_ld, int(start[0]), int(start[1]), _ptr(y), y_ld,
                                               _stream()))
        return y

    def tone_table(self, sample_rate=None):
        """conan_tone_table: the tone table of `sample_rate` (default: the model rate), W[m] = rint(2^14 cos(2 pi m / M)) -> int16 numpy
        [sample_rate].  Host only."""
        M = self.hop * 50 if sample_rate is None else int(sample_rate)
        out = np.zeros(max(M, 1), dtype=np.int16)
        _lib.check(self.lib.conan_tone_table(M, out.ctypes.data_as(C.c_void_p)))
        return out

    def tones(self, wav, lens=None, cfg=None, seed=None, hop_size=None, return_state=False, **kw):
        """conan_tones: the DTMF detector (include/conan_hip.h, conan_tone_cfg) on whole signals at 50 * hop Hz, one launch.  wav [n, N]
        (or [N]) float32; a 2-D view whose rows are contiguous keeps its row stride.  lens: per row the samples to read (default N).
        cfg: an _lib.ToneCfg, or **kw: _lib.tone_cfg's keywords.  seed: uint8 [n, 48] (cuda) rows of conan_tone_state the rows start
        from (tones(return_state=True)'s second form below), None: the cfg's seed; a row's first frame has index seed.frames, so a
        signal cut at frame boundaries and chained through the state gives the whole signal's rows.  -> (digit, sound, level) int32
        [n, F] with F = the longest row's ceil(len / hop) frames, -1 / -1 / 0 behind a shorter row's frames; with return_state=True
        also (states, rows): a list of dict(cand, run, cur, miss, held, sound, level, events, frames) (synchronises) and the same
        states as uint8 [n, 48].  _lib.tone_events(digit) lists the key presses.  It is what a wav-in slot with Streams.set_tones
        detects, bit for bit."""
        dev = torch.device("cuda", self.device)
        hop = int(hop_size or self.hop)
        c = cfg if cfg is not None else _lib.tone_cfg(**dict(dict(hop=hop), **kw))
        v = wav.to(dev, torch.float32)
        if v.dim() == 1:
            v = v[None]
        if v.dim() != 2:
            raise ValueError(f"tones: wav must be [n, N] or [N], got {tuple(wav.shape)}")
        n, N = v.shape
        if not (v.stride(1) == 1 and v.stride(0) >= N) and n * N:
            v = v.contiguous()
        ld = v.stride(0) if n > 1 else max(N, 1)
        sm = np.full(n, N, dtype=np.int64) if lens is None else np.ascontiguousarray(np.asarray(lens, dtype=np.int64).reshape(n))
        if sm.min(initial=0) < 0 or sm.max(initial=0) > N:
            raise ValueError(f"tones: lens must be in 0 .. {N}")
        size = C.sizeof(_lib.ToneState)
        if seed is not None and (seed.dtype != torch.uint8 or not seed.is_cuda or tuple(seed.shape) != (n, size) or not seed.is_contiguous()):
            raise ValueError(f"tones: seed must be a contiguous cuda uint8 [{n}, {size}] tensor, as return_state=True returns it")
        F = max(int((int(sm.max(initial=0)) + hop - 1) // hop), 1)
        digit = torch.full((n, F), -1, dtype=torch.int32, device=dev)
        sound = torch.full((n, F), -1, dtype=torch.int32, device=dev)
        level = torch.zeros(n, F, dtype=torch.int32, device=dev)
        st = torch.empty(n, size, dtype=torch.uint8, device=dev) if return_state else None
        frames = np.zeros(n, dtype=np.int64)
        if n:
            _lib.check(self.lib.conan_tones(self.h, hop, C.byref(c), _ptr(v), ld, n, sm.ctypes.data_as(C.c_void_p), _ptr(seed), _ptr(digit), _ptr(sound),
                                            _ptr(level), F, _ptr(st), frames.ctypes.data_as(C.c_void_p), _stream()))
        if not return_state:
            return digit, sound, level
        return digit, sound, level, (_struct_rows(st, _lib.ToneState), st)

    def tone_fill(self, wav, sound, level, cfg=None, start=(0, -1), pos0=0, hop_size=None, out=None, **kw):
        """conan_tone_fill: the regeneration on whole signals.  wav [..., N] float32 (the audio behind every other in-place stage) with
        sound [..., >= ceil(N / hop)] and level (int32; Streams.step_wav_tones' or Context.tones'); start = (level, sound) before
        frame 0; pos0: the utterance index of a row's first sample, one value or one per row -> [..., N].  cfg: an _lib.ToneCfg, or
        **kw: _lib.tone_cfg's keywords (gain is read).  A 2-D operand whose rows are contiguous keeps its row stride; out=wav fills in
        place.  Frames with level 0 at both ends keep wav's bits.  It is what a wav-in slot with Streams.set_tones (mode 2) puts out,
        bit for bit."""
        dev = torch.device("cuda", self.device)
        hop = int(hop_size or self.hop)
        c = cfg if cfg is not None else _lib.tone_cfg(**dict(dict(hop=hop), **kw))

        def rows(t, dtype):
            t = t.to(dev, dtype)
            if t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1]:
                return t, t.stride(0)
            t = t.contiguous()
            return t, t.shape[-1]

        x, x_ld = rows(wav, torch.float32)
        sd, sd_ld = rows(sound, torch.int32)
        lv, lv_ld = rows(level, torch.int32)
        lead, N = x.shape[:-1], x.shape[-1]
        n = int(np.prod(lead)) if len(lead) else 1
        if sd.shape[:-1] != lead or lv.shape != sd.shape:
            raise ValueError(f"tone_fill: wav {tuple(x.shape)}, sound {tuple(sd.shape)} and level {tuple(lv.shape)} do not match")
        if sd_ld != lv_ld:
            sd, lv = sd.contiguous(), lv.contiguous()
            sd_ld = lv_ld = sd.shape[-1]
        ps = np.ascontiguousarray(np.broadcast_to(np.asarray(pos0, dtype=np.int64), (n,)))
        if out is None:
            y, y_ld = torch.empty(x.shape, dtype=torch.float32, device=dev), N
        else:
            y, y_ld = (out, out.stride(0)) if out.dim() == 2 and out.stride(1) == 1 else (out, N)
            if y.shape != x.shape or y.dtype != torch.float32 or y.device != dev or not (y.is_contiguous() or (y.dim() == 2 and y.stride(1) == 1 and y_ld >= N)):
                raise ValueError("tone_fill: out must be a float32 tensor of wav's shape on the device, contiguous or a 2-D view with contiguous rows")
        _lib.check(self.lib.conan_tone_fill(self.h, hop, C.byref(c), _ptr(x), x_ld, n, N, ps.ctypes.data_as(C.c_void_p), _ptr(sd), _ptr(lv), sd_ld,
                                            int(start[0]), int(start[1]), _ptr(y), y_ld, _stream()))
        return y

    def register_of(self, wav, **f0_keywords):
        """The register of wav [n, N] (or [N]) at the model rate: per row the mean log2 Hz of its voiced frames - Context.f0 followed
        by the measurement of f0_register - or None for a row without a counted frame.  **f0_keywords: Context.f0's."""
        f0, uv = self.f0(wav, **f0_keywords)
        _, state = self.f0_register(f0, uv)
        return [int(S) / (int(k) * float(_lib.REGISTER_UNIT)) if k else None for k, S in state.reshape(-1, 2).cpu().tolist()]

    def convert_samples(self, x, src, dst, out=None):
        """conan_convert_samples: x [..., N] of format `src` ('f32' float32, 's16' int16, 'ulaw' / 'alaw' uint8) -> [..., N] of
        format `dst`, by the library's one conversion rule (decode exactly, encode with round-to-nearest-even and saturation).
        out: a contiguous 2-D cuda buffer with one row per signal whose rows are a multiple of 4 bytes; the samples are written
        from the start of each row, the bytes past them are left alone, and the rows come back as views in dst's dtype."""
        fs, fd = _lib.sample_format(src), _lib.sample_format(dst)
        dev = torch.device("cuda", self.device)
        x = x.to(dev)
        if x.dtype != SAMPLE_DTYPES[src]:
            raise ValueError(f"convert_samples: format {src!r} takes {SAMPLE_DTYPES[src]} samples, got {x.dtype}")
        lead, N = x.shape[:-1], x.shape[-1]
        n = int(np.prod(lead)) if len(lead) else 1
        bs, bd = _lib.SAMPLE_BYTES[src], _lib.SAMPLE_BYTES[dst]
        src_ld = (N * bs + 3) // 4
        xin = x.reshape(n, N).contiguous() if N * bs % 4 == 0 else _row_bytes(x.reshape(n, N), n, src_ld, dev)
        if out is None:
            out = torch.empty(n, 4 * ((N * bd + 3) // 4), dtype=torch.uint8, device=dev)
        assert out.is_cuda and out.is_contiguous() and out.dim() == 2 and out.shape[0] == n and out.shape[1] * out.element_size() % 4 == 0
        dst_ld = out.shape[1] * out.element_size() // 4
        if n and N:
            _lib.check(self.lib.conan_convert_samples(self.h, fs, _ptr(xin), src_ld, fd, _ptr(out), dst_ld, n, N, _stream()))
        return out.view(SAMPLE_DTYPES[dst])[:, :N].reshape(*lead, N)

    def conceal(self, x, lost, cfg, fmt="f32", lengths=None):
        """conan_conceal: the loss concealment's law (include/conan_hip.h, conan_conceal_cfg) on whole signals from the zero state.
        x [..., N] of format `fmt` ('f32' float32, 's16' int16, 'ulaw' / 'alaw' uint8); lost [..., >= ceil(N / packet)] integer or
        bool, non-zero = the packet never arrived; cfg: an _lib.ConcealCfg, a dict of its fields, or an input rate, which stands for
        that rate's defaults (_lib.conceal_keywords); lengths: per row the samples to repair (default N).  -> the repaired signals
        [..., N] in fmt's dtype (x itself is left alone: the rows are packed into a buffer of the library's row stride first).  It
        is what a slot with Streams.set_conceal computes over its rows, bit for bit."""
        c = _rate_cfg("conceal", cfg)
        dev = torch.device("cuda", self.device)
        f, (buf,), lead, n, N, ld, sm = _pack_signals("conceal", fmt, dev, lengths, x=x)
        flags = lost.to(dev).reshape(n, -1).to(torch.int32).contiguous()
        if n and N:
            _lib.check(self.lib.conan_conceal(self.h, C.byref(c), f, _ptr(buf), ld, n, sm.ctypes.data_as(C.c_void_p), _ptr(flags), flags.shape[1], _stream()))
        return buf.view(SAMPLE_DTYPES[fmt])[:, :N].reshape(*lead, N)

    def echo(self, mic, far, cfg, fmt="f32", lengths=None, stats=False):
        """conan_echo: the echo canceller's law (include/conan_hip.h, conan_echo_cfg) on whole signals from the zero state.  mic, far
        [..., N] of format `fmt` ('f32' float32, 's16' int16, 'ulaw' / 'alaw' uint8): the microphone rows and what went to the
        earpiece, sample for sample; cfg: an _lib.EchoCfg, a dict of its fields, or an input rate, which stands for that rate's
        defaults (_lib.echo_keywords); lengths: per row the samples to cancel (default N).  -> the cancelled signals [..., N] in
        fmt's dtype (mic itself is left alone), and with stats=True also int64 [n, 4] (cuda): per row sum d^2, sum e^2, blocks
        adapted, blocks frozen.  It is what a slot with Streams.set_echo computes over its rows, bit for bit."""
        c = _rate_cfg("echo", cfg)
        dev = torch.device("cuda", self.device)
        f, (buf, fbuf), lead, n, N, ld, sm = _pack_signals("echo", fmt, dev, lengths, mic=mic, far=far)
        st = torch.zeros(n, 4, dtype=torch.int64, device=dev)
        if n and N:
            _lib.check(self.lib.conan_echo(self.h, C.byref(c), f, _ptr(buf), ld, _ptr(fbuf), ld, n, sm.ctypes.data_as(C.c_void_p), _ptr(st), _stream()))
        out = buf.view(SAMPLE_DTYPES[fmt])[:, :N].reshape(*lead, N)
        return (out, st) if stats else out

    def echo_delay(self, mic, far, cfg, fmt="f32", lengths=None):
        """conan_echo_delay: the echo-delay estimator's law (include/conan_hip.h, conan_echo_delay_cfg) on whole signals from the zero
        state.  mic, far [..., N] of format `fmt`, as Context.echo takes them (both are only read); cfg: an _lib.EchoDelayCfg, a dict
        of its fields, or an input rate, which stands for that rate's defaults (_lib.echo_delay_keywords); lengths: per row the
        samples to take (default N).  -> (track int64 [n, N // 1024, 6] (cuda): per row the report after each frame end, zeros
        behind a shorter row's frames; report int64 [n, 6]: est, age, cand, run, last_pk, last_s after the last sample).  It is
        what a slot with Streams.set_echo_delay computes over its rows, bit for bit."""
        c = _rate_cfg("echo_delay", cfg)
        dev = torch.device("cuda", self.device)
        f, (buf, fbuf), lead, n, N, ld, sm = _pack_signals("echo_delay", fmt, dev, lengths, mic=mic, far=far)
        frames = N // _lib.ECHO_DELAY_FRAME
        track = torch.zeros(n, frames, 6, dtype=torch.int64, device=dev)
        report = torch.zeros(n, 6, dtype=torch.int64, device=dev)
        if n and N:
            _lib.check(self.lib.conan_echo_delay(self.h, C.byref(c), f, _ptr(buf), ld, _ptr(fbuf), ld, n, sm.ctypes.data_as(C.c_void_p),
                                                 _ptr(track) if frames else None, frames * 6, _ptr(report), _stream()))
        return track, report

    def mel_denoise(self, mel, lens=None, cfg=None, seed=None, out=None, state=False, **kw):
        """conan_mel_denoise: the noise suppressor's law (include/conan_hip.h, conan_denoise_cfg) on whole log-mel rows, one launch.
        mel [n, T, num_mels] (or [T, num_mels]) float32; a 3-D view whose rows are contiguous keeps its row stride.  lens: per row
        the frames to take (default T; the frames behind them come back as they came).  cfg: an _lib.DenoiseCfg, or **kw:
        _lib.denoise_cfg's keywords (natural_log, mel_vmin and eps are the mel's own).  seed: uint8 [n, bytes] (cuda) rows of conan_denoise_state the rows start from (mel_denoise(state=True)
        or Streams.denoise_state); None: every row starts before its first frame.  out: a tensor of mel's shape and strides (out=mel:
        in place).  -> the suppressed mel, and with state=True also the rows' states uint8 [n, bytes] (_lib.DenoiseState reads one).
        It is what a wav-in slot with Streams.set_denoise computes on its frames, bit for bit, and what a caller with mel-in slots
        streams through seed and state."""
        dev = torch.device("cuda", self.device)
        c = cfg if cfg is not None else _lib.denoise_cfg(**kw)
        x = mel.to(dev, torch.float32)
        if x.dim() == 2:
            x = x[None]
        if x.dim() != 3:
            raise ValueError(f"mel_denoise: mel must be [n, T, num_mels] or [T, num_mels], got {tuple(mel.shape)}")
        n, T, nm = x.shape
        if not (x.stride(2) == 1 and x.stride(1) == nm and x.stride(0) >= T * nm) and n * T * nm:
            x = x.contiguous()
        ld = x.stride(0) if n > 1 else max(T * nm, 1)
        if out is None:
            y = torch.empty_strided(x.shape, (ld, nm, 1), dtype=torch.float32, device=dev) if n > 1 else torch.empty_like(x)
            if lens is not None:
                y.copy_(x)      # (the frames past a row's length come back as they came)
        else:
            y = out if out.dim() == 3 else out[None]
            if y.shape != x.shape or y.dtype != torch.float32 or y.device != dev or (n * T * nm and (y.stride(2) != 1 or y.stride(1) != nm or (n > 1 and y.stride(0) != ld))):
                raise ValueError("mel_denoise: out must be a float32 tensor of mel's shape and strides on the device")
        fr = np.full(n, T, dtype=np.int32) if lens is None else np.ascontiguousarray(np.asarray(lens, dtype=np.int32).reshape(n))
        if fr.min(initial=0) < 0 or fr.max(initial=0) > T:
            raise ValueError(f"mel_denoise: lens must be in 0 .. {T}")
        size = C.sizeof(_lib.DenoiseState)
        if seed is not None and (seed.dtype != torch.uint8 or not seed.is_cuda or tuple(seed.shape) != (n, size) or not seed.is_contiguous()):
            raise ValueError(f"mel_denoise: seed must be a contiguous cuda uint8 [{n}, {size}] tensor, as state=True returns it")
        st = torch.empty(n, size, dtype=torch.uint8, device=dev) if state else None
        if n * T * nm == 0 and state:      # (no frame anywhere: the states are the seeds, or the record before the first frame)
            st = seed.clone() if seed is not None else torch.zeros_like(st)
        if n * T * nm:
            _lib.check(self.lib.conan_mel_denoise(self.h, C.byref(c), _ptr(x), n, fr.ctypes.data_as(C.c_void_p), ld, nm, _ptr(seed), _ptr(y), _ptr(st),
                                                  _stream()))
        y = out if out is not None else (y[0] if mel.dim() == 2 else y)
        return (y, st) if state else y

    def watermark_embed(self, x, lens=None, cfg=None, seed=None, out=None, state=False, **kw):
        """conan_watermark_embed: the watermark's embedder (include/conan_hip.h, conan_watermark_cfg) on whole signals at 16 kHz, one
        launch.  x [n, N] (or [N]) float32; a 2-D view whose rows are contiguous keeps its row stride.  lens: per row the samples to
        mark (default N; the samples behind them come back as they came).  cfg: an _lib.WatermarkCfg, or **kw: _lib.watermark_cfg's
        keywords (key, id, gain, floor).  seed: uint8 [n, 16] (cuda) rows of conan_watermark_state the rows start from
        (watermark_embed(state=True) or Streams.watermark_state); None: every row starts at position 0.  out: a tensor of x's shape
        and strides (out=x: in place).  -> the marked audio, and with state=True also the rows' states uint8 [n, 16]
        (_lib.WatermarkState reads one).  It is what a slot with Streams.set_watermark adds to its vocoder audio, bit for bit."""
        dev = torch.device("cuda", self.device)
        c = cfg if cfg is not None else _lib.watermark_cfg(**kw)
        v = x.to(dev, torch.float32)
        if v.dim() == 1:
            v = v[None]
        if v.dim() != 2:
            raise ValueError(f"watermark_embed: x must be [n, N] or [N], got {tuple(x.shape)}")
        n, N = v.shape
        if not (v.stride(1) == 1 and v.stride(0) >= N) and n * N:
            v = v.contiguous()
        ld = v.stride(0) if n > 1 else max(N, 1)
        if out is None:
            y = torch.empty_strided(v.shape, (ld, 1), dtype=torch.float32, device=dev) if n > 1 else torch.empty_like(v)
            if lens is not None:
                y.copy_(v)
        else:
            y = out if out.dim() == 2 else out[None]
            if y.shape != v.shape or y.dtype != torch.float32 or y.device != dev or (n * N and (y.stride(1) != 1 or (n > 1 and y.stride(0) != ld))):
                raise ValueError("watermark_embed: out must be a float32 tensor of x's shape and strides on the device")
        sm = np.full(n, N, dtype=np.int64) if lens is None else np.ascontiguousarray(np.asarray(lens, dtype=np.int64).reshape(n))
        if sm.min(initial=0) < 0 or sm.max(initial=0) > N:
            raise ValueError(f"watermark_embed: lens must be in 0 .. {N}")
        size = C.sizeof(_lib.WatermarkState)
        if seed is not None and (seed.dtype != torch.uint8 or not seed.is_cuda or tuple(seed.shape) != (n, size) or not seed.is_contiguous()):
            raise ValueError(f"watermark_embed: seed must be a contiguous cuda uint8 [{n}, {size}] tensor, as state=True returns it")
        st = torch.empty(n, size, dtype=torch.uint8, device=dev) if state else None
        if n:
            _lib.check(self.lib.conan_watermark_embed(self.h, C.byref(c), _ptr(v), n, sm.ctypes.data_as(C.c_void_p), ld, _ptr(seed), _ptr(y), _ptr(st),
                                                      _stream()))
        y = out if out is not None else (y[0] if x.dim() == 1 else y)
        return (y, st) if state else y

    def watermark_detect(self, x, key, format="f32", rate=16000, threshold=None, lens=None, raw=False):
        """conan_watermark_detect and conan_watermark_decide: the watermark's detector on x [n, N] (or [N]) of `format` ('f32' float32,
        's16' int16, 'ulaw' / 'alaw' uint8) at `rate` Hz; audio at another rate is decoded and brought to 16 kHz with the library's
        own resampler first (the offset search absorbs the filter's delay).  key: the embedder's; threshold: None is the library's
        default (_lib.WATERMARK_THRESHOLD); lens: per row the samples to read (default N).  -> one dict per row: present, z, id,
        offset, rotation, marker_score, blocks; with raw=True also S (int64 [2048]), soft (int64 [blocks]) and peak, the detector's
        integers.  Rows under two blocks (4096 samples) report present = 0, blocks = 0.  Synchronises."""
        f = _lib.sample_format(format)
        dev = torch.device("cuda", self.device)
        v = x.to(dev)
        if v.dtype != SAMPLE_DTYPES[format]:
            raise ValueError(f"watermark_detect: format {format!r} takes {SAMPLE_DTYPES[format]} samples, got {v.dtype}")
        if v.dim() == 1:
            v = v[None]
        if v.dim() != 2:
            raise ValueError(f"watermark_detect: x must be [n, N] or [N], got {tuple(x.shape)}")
        n, N = v.shape
        sm = np.full(n, N, dtype=np.int64) if lens is None else np.ascontiguousarray(np.asarray(lens, dtype=np.int64).reshape(n))
        if sm.min(initial=0) < 0 or sm.max(initial=0) > N:
            raise ValueError(f"watermark_detect: lens must be in 0 .. {N}")
        if int(rate) != 16000:
            if lens is not None:
                raise ValueError("watermark_detect: lens needs rate=16000 (resample the rows one by one)")
            v = self.resample(v if format == "f32" else self.convert_samples(v, format, "f32"), int(rate), 16000)
            f, format, N = _lib.sample_format("f32"), "f32", v.shape[1]
            sm = np.full(n, N, dtype=np.int64)
        ld = max((N * _lib.SAMPLE_BYTES[format] + 3) // 4, 1)
        buf = _row_bytes(v.reshape(n, N), n, ld, dev)
        kmax = max(int(sm.max(initial=0)) // _lib.WATERMARK_BLOCK - 1, 0)
        score = torch.empty(n, _lib.WATERMARK_BLOCK, dtype=torch.int64, device=dev)
        soft = torch.empty(n, max(kmax, 1), dtype=torch.int64, device=dev)
        hit = torch.empty(n, C.sizeof(_lib.WatermarkHit), dtype=torch.uint8, device=dev)
        results = []
        if n:
            _lib.check(self.lib.conan_watermark_detect(self.h, int(key) & ((1 << 64) - 1), f, _ptr(buf), ld, n, sm.ctypes.data_as(C.c_void_p), _ptr(score),
                                                       _ptr(soft), soft.shape[1], _ptr(hit), _stream()))
        S, sf, hits = score.cpu().numpy(), soft.cpu().numpy(), hit.cpu().numpy().tobytes()
        th = _lib.WATERMARK_THRESHOLD if threshold is None else float(threshold)
        for i in range(n):
            h = _lib.WatermarkHit.from_buffer_copy(hits[i * 16:(i + 1) * 16])
            r = _lib.WatermarkResult()
            s_row, f_row = np.ascontiguousarray(S[i]), np.ascontiguousarray(sf[i])
            _lib.check(self.lib.conan_watermark_decide(s_row.ctypes.data_as(C.c_void_p), f_row.ctypes.data_as(C.c_void_p), C.byref(h), th, C.byref(r)))
            d = dict(present=bool(r.present), z=float(r.z), id=int(r.id), offset=int(r.offset), rotation=int(r.rotation), marker_score=int(r.marker_score),
                     blocks=int(r.blocks))
            if raw:
                d.update(S=s_row, soft=f_row[:h.blocks].copy(), peak=int(h.peak))
            results.append(d)
        return results

    def streams(self, max_slots, max_frames=4, max_ref_frames=256, arith="auto", flags=0, dev_plan=None):
        """A stream-set.  arith: 'auto' (library default), 'f32' (f32-input MFMA everywhere) or 'limb' (fp32 products of the
        vocoder's matrix kernels as bf16 limb products) - conan_streams_opts.arith; flags: _lib.STREAMS_*; dev_plan: developer /
        test switches of the launch plan, "NAME=value;..." (conan_streams_opts.dev_plan; None in deployments)."""
        return Streams(self, max_slots, max_frames, max_ref_frames, arith, flags, dev_plan)

    def voices(self, capacity, max_ref_frames=256):
        """A voice bank (conan_voices_create): up to `capacity` enrolled target voices of up to max_ref_frames reference frames, kept
        on the device outside any slot; Streams.set_voice assigns them to slots in one launch."""
        return VoiceBank(self, capacity, max_ref_frames)

    def close(self):
        if getattr(self, "h", None):
            self.lib.conan_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SlotSnapshot:
    """Exported streams (Streams.export_slots): `meta` - the host records, 256 bytes per stream - and `blob` - a uint8 tensor
    [n, bytes], one row of device state per stream.  Position independent: it holds no pointers, slot numbers or ring indices, so it
    may be moved to the host (cpu), to another device (to), pickled, and imported by another process into a stream-set of the same
    layout_id."""

    def __init__(self, meta, blob):
        assert len(meta) == blob.shape[0] * _lib.SLOT_META_BYTES and blob.dtype == torch.uint8 and blob.dim() == 2
        self.meta, self.blob = bytes(meta), blob

    def __len__(self):
        return self.blob.shape[0]

    def info(self, i):
        """conan_slot_meta_info of stream i: dict(layout_id, bytes, has_ref, in_format, out_format, in_rate, out_rate, level, pitch); a
        rate is None for a stream without one; level (conan_slot_meta_level) is the input leveller's keywords as
        Streams.set_input_level takes them, pitch (conan_slot_meta_pitch) the pitch control's as Streams.set_pitch takes them; each
        None for a stream without one."""
        rec = _lib.SlotMeta.from_buffer_copy(self.meta[i * _lib.SLOT_META_BYTES:(i + 1) * _lib.SLOT_META_BYTES])
        out = _lib.SlotInfo()
        _lib.check(_lib.lib().conan_slot_meta_info(C.byref(rec), C.byref(out)))
        names = {v: k for k, v in _lib.SAMPLE_FORMATS.items()}

        def setting(f):
            c = f.cfg()
            return f.keywords(c) if _lib.check(getattr(_lib.lib(), f.meta)(C.byref(rec), C.byref(c))) else None

        return dict(level=setting(_lib.SLOT_FEATURES["level"]), pitch=setting(_lib.SLOT_FEATURES["pitch"]), layout_id=int(out.layout_id), bytes=int(out.bytes), has_ref=bool(out.has_ref), in_format=names[out.in_format],
                    out_format=names[out.out_format],
                    in_rate=out.in_rate.in_rate if out.in_rate.in_rate != out.in_rate.out_rate else None,
                    out_rate=out.out_rate.out_rate if out.out_rate.in_rate != out.out_rate.out_rate else None,
                    in_cfg=out.in_rate, out_cfg=out.out_rate)

    def cpu(self):
        return SlotSnapshot(self.meta, self.blob.cpu())

    def to(self, device):
        return SlotSnapshot(self.meta, self.blob.to(device))

    def select(self, rows):
        """The snapshot of the streams `rows` (indices into this one), in that order; a row may repeat (a fork)."""
        rows = [int(r) for r in rows]
        M = _lib.SLOT_META_BYTES
        return SlotSnapshot(b"".join(self.meta[r * M:(r + 1) * M] for r in rows), self.blob[rows])

    def __getstate__(self):
        b = self.blob.cpu().contiguous()
        return {"meta": self.meta, "shape": tuple(b.shape), "blob": b.numpy().tobytes()}

    def __setstate__(self, state):
        self.meta = state["meta"]
        self.blob = torch.frombuffer(bytearray(state["blob"]), dtype=torch.uint8).reshape(state["shape"])


class VoiceSet:
    """Exported voices (VoiceBank.export): `meta` - the host records, 256 bytes per voice - and `blob` - a uint8 tensor [n, bytes],
    one row per voice.  A row is sized by the voice's tokens alone and holds no pointers or indices: it may be moved to the host
    (cpu), to another device (to), pickled, written to a file, and imported into any bank of the same model shape whose
    max_ref_frames holds the voice."""

    def __init__(self, meta, blob):
        assert len(meta) == blob.shape[0] * _lib.VOICE_META_BYTES and blob.dtype == torch.uint8 and blob.dim() == 2
        self.meta, self.blob = bytes(meta), blob

    def __len__(self):
        return self.blob.shape[0]

    def info(self, i):
        """conan_voice_meta_info of voice i: dict(layout_id, bytes, ref_frames, tokens)."""
        M = _lib.VOICE_META_BYTES
        rec = _lib.VoiceMeta.from_buffer_copy(self.meta[i * M:(i + 1) * M])
        out = _lib.VoiceInfo()
        _lib.check(_lib.lib().conan_voice_meta_info(C.byref(rec), C.byref(out)))
        return dict(layout_id=int(out.layout_id), bytes=int(out.bytes), ref_frames=int(out.ref_frames), tokens=int(out.tokens))

    def cpu(self):
        return VoiceSet(self.meta, self.blob.cpu())

    def to(self, device):
        return VoiceSet(self.meta, self.blob.to(device))

    def select(self, rows):
        """The set of the voices `rows` (indices into this one), in that order; a row may repeat."""
        rows = [int(r) for r in rows]
        M = _lib.VOICE_META_BYTES
        return VoiceSet(b"".join(self.meta[r * M:(r + 1) * M] for r in rows), self.blob[rows])

    def __getstate__(self):
        b = self.blob.cpu().contiguous()
        return {"meta": self.meta, "shape": tuple(b.shape), "blob": b.numpy().tobytes()}

    def __setstate__(self, state):
        self.meta = state["meta"]
        self.blob = torch.frombuffer(bytearray(state["blob"]), dtype=torch.uint8).reshape(state["shape"])


class VoiceBank:
    """conan_voices: enrolled target voices - the cached result of set_reference's style pass - on the device, outside any slot."""

    def __init__(self, ctx, capacity, max_ref_frames=256):
        self.ctx, self.lib = ctx, ctx.lib
        self.capacity, self.max_ref_frames = int(capacity), int(max_ref_frames)
        h = C.c_void_p()
        _lib.check(self.lib.conan_voices_create(ctx.h, self.capacity, self.max_ref_frames, C.byref(h)))
        self.h = h
        self.dev = torch.device("cuda", ctx.device)
        self.registers = {}      # id -> mean log2 Hz of the enrolled waveform (enroll_wav(register=True)); host only

    def enroll(self, ids, ref_mel, ref_len=None, via=None):
        """conan_voices_enroll: the style pass of ref_mel [n, Tr, num_mels] (as Streams.set_reference) into entries `ids`, one voice
        per pass on the workspace of the stream-set `via`."""
        if via is None:
            raise ValueError("VoiceBank.enroll: via= (a Streams of this context, whose workspace the style pass runs on) is required")
        a, p = _i32(ids)
        ref_mel = ref_mel.to(self.dev, torch.float32).contiguous()
        if ref_mel.dim() == 2:
            ref_mel = ref_mel[None]
        n, tr = ref_mel.shape[0], ref_mel.shape[1]
        if n != len(a):
            raise ValueError(f"VoiceBank.enroll: {len(a)} ids for {n} reference mels")
        if ref_len is None:
            ref_len = [tr] * n
        l, lp = _i32(ref_len)
        if len(l) != n:
            raise ValueError(f"VoiceBank.enroll: {len(l)} lengths for {n} reference mels")
        _lib.check(self.lib.conan_voices_enroll(self.h, via.h, p, n, _ptr(ref_mel), lp, tr, _stream()))
        via._release()
        for i in a:
            self.registers.pop(int(i), None)      # (the id holds another voice now; enroll_wav(register=True) measures it)

    def enroll_wav(self, ids, wav, via=None, sample_rate=None, loud_norm=False, register=False, trim=False, denoise=False, eq=None, **mel):
        """Context.wav2mel of wav [n, samples] - resampled from sample_rate to the mel front-end's rate, loudness-normalised and
        trimmed first where asked - then enroll.  **mel: wav2mel's keywords.  trim: True, or a dict of Context.trim_silence's
        keywords: the long pauses of each clip are cut out (behind resampling and loud_norm) so that they neither dilute the style
        vector nor spend prosody tokens; the rows then differ in length, each is enrolled with its own frame count, and the result
        is that of enroll(ids, wav2mel(trimmed rows), ref_len) bit for bit.  The front-end's rate must be 50 * hop_size, and a clip
        without any activity is an error.  register=True also measures each voice's register
        (Context.register_of of the same prepared wav, which must then be at the model rate) into the host dict self.registers[id] -
        what register="voice" of the engine's wav-in calls looks up; export / import_voices do not carry it.  denoise: True, or a
        dict of _lib.denoise_cfg's keywords: the noise suppressor (Context.mel_denoise, with the mel's own log base, vmin and eps)
        runs on each clip's mel, over its own frames, in front of enroll.  eq: a dict(sections=[...]) of _lib.eq_cfg's keywords: the
        equaliser's whole-signal form (Context.eq, sections designed at the front-end's rate) on each clip behind the resampling and
        in front of loud_norm - where a wav-in slot's source-side equaliser stands."""
        rate = int(mel.get("sample_rate", 16000))
        wav = wav.to(self.dev, torch.float32)
        if wav.dim() == 1:
            wav = wav[None]
        if sample_rate is not None and int(sample_rate) != rate:
            wav = self.ctx.resample(wav, int(sample_rate), rate)
        if eq:
            wav = self.ctx.eq(wav, cfg=_lib.eq_cfg(**dict(dict(rate=float(rate)), **dict(eq))))
        if loud_norm:
            wav = self.ctx.loud_norm(wav, rate)
        ref_len = None
        if trim:
            hop = int(mel.get("hop_size", 320))
            if rate != 50 * hop:
                raise ValueError(f"enroll_wav(trim=): the front-end's sample_rate {rate} must be 50 * hop_size {hop}")
            wav, kept = self.ctx.trim_silence(wav, hop_size=hop, **({} if trim is True else dict(trim)))
            if int(kept.min()) < 1:
                raise ValueError("enroll_wav(trim=): a clip has no activity, nothing is left of it")
            ref_len = [1 + int(k) // hop for k in kept]
        ref_mel = self.ctx.wav2mel(wav, **mel)
        if denoise:
            own = dict(natural_log=bool(mel.get("natural_log", False)), mel_vmin=mel.get("mel_vmin", -6.0), eps=mel.get("eps", 1e-6))
            ref_mel = self.ctx.mel_denoise(ref_mel, lens=ref_len, out=ref_mel, **dict(own, **({} if denoise is True else dict(denoise))))
        self.enroll(ids, ref_mel, ref_len, via=via)
        if register:
            for i, r in zip(ids, self.ctx.register_of(wav, hop_size=mel.get("hop_size"))):
                self.registers[int(i)] = r

    def remove(self, ids):
        a, p = _i32(ids)
        _lib.check(self.lib.conan_voices_remove(self.h, p, len(a)))
        for i in a:
            self.registers.pop(int(i), None)

    def info(self, id):
        """conan_voices_info: dict(ref_frames, tokens, bytes) of an enrolled id, None for one that holds no voice."""
        out = _lib.VoiceInfo()
        _lib.check(self.lib.conan_voices_info(self.h, int(id), C.byref(out)))
        return dict(ref_frames=int(out.ref_frames), tokens=int(out.tokens), bytes=int(out.bytes)) if out.enrolled else None

    @property
    def blob_bytes(self):
        """Bytes a row of this bank can need (conan_voices_blob_bytes), a multiple of 256."""
        return _lib.check(self.lib.conan_voices_blob_bytes(self.h))

    def export(self, ids):
        """conan_voices_export: the voices `ids` -> VoiceSet (blob on this device, complete in stream order)."""
        a, p = _i32(ids)
        n = len(a)
        blob = torch.zeros(n, self.blob_bytes, dtype=torch.uint8, device=self.dev)
        meta = (_lib.VoiceMeta * n)()
        _lib.check(self.lib.conan_voices_export(self.h, p, n, _ptr(blob), blob.stride(0), meta, _stream()))
        return VoiceSet(bytes(meta), blob)

    def import_voices(self, ids, voice_set):
        """conan_voices_import: entry ids[i] becomes voice i of `voice_set`.  Every record is checked before anything changes."""
        a, p = _i32(ids)
        n = len(a)
        if len(voice_set) != n:
            raise ValueError(f"import_voices: {n} ids for a set of {len(voice_set)} voices")
        blob = voice_set.blob.to(self.dev)
        if blob.stride(1) != 1 or blob.stride(0) % 16 or blob.data_ptr() % 16:
            blob = blob.contiguous()
        meta = (_lib.VoiceMeta * n).from_buffer_copy(voice_set.meta)
        _lib.check(self.lib.conan_voices_import(self.h, p, n, _ptr(blob), blob.stride(0), meta, _stream()))
        blob.record_stream(torch.cuda.current_stream())

    def close(self):
        if getattr(self, "h", None):
            self.lib.conan_voices_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Streams:
    """conan_streams: per-slot streaming state + the step functions."""

    def __init__(self, ctx, max_slots, max_frames=4, max_ref_frames=256, arith="auto", flags=0, dev_plan=None):
        self.ctx, self.lib = ctx, ctx.lib
        self.max_slots, self.max_frames, self.max_ref_frames = max_slots, max_frames, max_ref_frames
        if arith not in _lib.ARITH_NAMES:
            raise ValueError(f"arith must be one of {sorted(_lib.ARITH_NAMES)}, got {arith!r}")
        opts = _lib.StreamsOpts(_lib.ABI_VERSION, _lib.ARITH_NAMES[arith], int(flags), 0, dev_plan.encode() if dev_plan else None)
        h = C.c_void_p()
        _lib.check(self.lib.conan_streams_create_opts(ctx.h, max_slots, max_frames, max_ref_frames, C.byref(opts), C.byref(h)))
        self._keep = []   # buffers of pipelined steps in flight (released by join())
        self.h = h
        self.dev = torch.device("cuda", ctx.device)
        c = ctx.cfg
        self.seg, self.rc = c.emf_segment, c.emf_right_context
        self.input_rate_set = False      # set_input_rate has run on this stream-set (its history ring exists)
        self.output_rates = {}           # slot -> output rate, for the slots whose audio leaves at another rate than the model's
        self.input_drifts, self.output_drifts = set(), set()      # the slots with a drift resampler (set_input_drift / set_output_drift)
        self.echo_delays = set()                                  # the slots with an echo-delay estimator (set_echo_delay)
        self.output_ld = 0               # set_output_ld: row stride of every step's wav (0: each step's own)
        self.input_formats = {}          # slot -> 's16' | 'ulaw' | 'alaw', for the slots whose wav-in rows are not float32
        self.output_formats = {}         # slot -> the same, for the slots whose audio leaves in another format
        self.input_levels = {}           # slot -> dict of set_input_level's keywords, for the slots with an input leveller
        self.output_levels = {}          # slot -> dict of set_output_level's keywords, for the slots with an output leveller
        self.pitch_cfgs = {}             # slot -> dict of set_pitch's keywords, for the slots with a pitch control
        self._last_wav_n = 0             # rows of the most recent wav-in call (step_wav_contour)

    @property
    def state_bytes(self):
        return self.lib.conan_streams_state_bytes(self.h)

    @property
    def arith(self):
        """'f32' or 'limb': the arithmetic this stream-set's vocoder launches use where both forms exist ('auto' resolved)."""
        return {_lib.ARITH_F32: "f32", _lib.ARITH_LIMB: "limb"}[_lib.check(self.lib.conan_streams_arith(self.h))]

    @property
    def snapshot_bytes(self):
        """Bytes of one stream's blob row (conan_streams_snapshot_bytes): an upper bound over the slots, a multiple of 256."""
        return _lib.check(self.lib.conan_streams_snapshot_bytes(self.h))

    @property
    def layout_id(self):
        """conan_streams_layout_id: equal for stream-sets a snapshot can move between."""
        return int(self.lib.conan_streams_layout_id(self.h))

    def export_slots(self, slots, out=None):
        """conan_streams_export_slots: the streams in `slots` -> SlotSnapshot (blob on this device; complete in stream order, the
        host records at once).  Joins pipelined work; changes nothing in the slots.  out: a cuda uint8 [n, >= snapshot_bytes] buffer."""
        a, p = _i32(slots)
        n = len(a)
        blob = out if out is not None else torch.empty(n, self.snapshot_bytes, dtype=torch.uint8, device=self.dev)
        assert blob.is_cuda and blob.dtype == torch.uint8 and blob.dim() == 2 and blob.shape[0] == n and blob.stride(1) == 1
        meta = (_lib.SlotMeta * n)()
        _lib.check(self.lib.conan_streams_export_slots(self.h, p, n, _ptr(blob), blob.stride(0), meta, _stream()))
        self._release()
        return SlotSnapshot(bytes(meta), blob)

    def import_slots(self, slots, snap):
        """conan_streams_import_slots: slot slots[i] becomes stream i of `snap` (history, positions, style cache, rates, formats,
        input leveller).  Every record is checked before anything changes.  The blob is moved to this device if it is elsewhere."""
        a, p = _i32(slots)
        n = len(a)
        if len(snap) != n:
            raise ValueError(f"import_slots: {n} slots for a snapshot of {len(snap)} streams")
        blob = snap.blob.to(self.dev)
        if blob.stride(1) != 1 or blob.stride(0) % 16 or blob.data_ptr() % 16:
            blob = blob.contiguous()
        meta = (_lib.SlotMeta * n).from_buffer_copy(snap.meta)
        _lib.check(self.lib.conan_streams_import_slots(self.h, p, n, _ptr(blob), blob.stride(0), meta, _stream()))
        blob.record_stream(torch.cuda.current_stream())
        self._release()
        for i, slot in enumerate(a):      # the Python-side mirrors of the slot configuration that travelled
            info = snap.info(i)
            self._drift_slots("input").discard(int(slot))      # (a snapshot carries no drift resampler: the import replaces the slot's)
            self._drift_slots("output").discard(int(slot))
            self._note_format(self.input_formats, [slot], info["in_format"])
            self._note_format(self.output_formats, [slot], info["out_format"])
            if info["in_rate"] is not None:
                self.input_rate_set = True
            if info["out_rate"] is not None:
                self.output_rates[int(slot)] = int(info["out_rate"])
            else:
                self.output_rates.pop(int(slot), None)
            for key in ("level", "pitch"):
                self._note_cfg(_lib.SLOT_FEATURES[key], slot, info[key])

    def _note_cfg(self, f, slot, keywords):
        """The slot's entry in the dict slot -> keywords of a feature that keeps one: the keywords, or none for a slot without it."""
        if keywords is not None:
            getattr(self, f.mirror)[int(slot)] = keywords
        else:
            getattr(self, f.mirror).pop(int(slot), None)

    def _set_feature(self, key, slots, cfg, kw, defaults=(), seed=None):
        """A feature's setter: the struct of (cfg, **kw) over `defaults` (_feature_cfg) goes to the slots, with the seed rows where
        the feature takes them; pipelined buffers are released where the call joined them; the slots' keywords are noted."""
        f = _lib.SLOT_FEATURES[key]
        a, p = _i32(slots)
        c = _feature_cfg(f, cfg, kw, defaults)
        args = [self.h, p, len(a), C.byref(c)]
        if f.seed_state:
            reader = f.seed_state[len("conan_streams_"):]
            if seed is not None and (seed.dtype != torch.uint8 or seed.dim() != 2 or seed.shape[0] != len(a) or not seed.is_cuda or seed.stride(1) != 1):
                raise ValueError(f"{f.method}: seed must be a cuda uint8 [n, bytes] tensor, as {reader} returns it")
            args += [_ptr(seed), int(seed.stride(0))] if seed is not None else [None, 0]
        _lib.check(getattr(self.lib, f.setter)(*args, *([_stream()] if f.stream else [])))
        if f.release:
            self._release()
        if f.mirror:
            for slot in a:
                self._note_cfg(f, slot, f.keywords(c) if getattr(c, f.on) else None)
        return c

    def _call_rows(self, who, slots, samples, report=None, width=0, **rows):
        """The arguments of a pre-step row call (conceal, echo, echo_delay): rows (keyword -> a 2-D cuda tensor with one row per
        slot, contiguous rows a multiple of 4 bytes apart), samples (an int or one per row) and the optional int64 [n, width] report
        tensor -> (the slot array's pointer, n, the samples' pointer, per row tensor its pointer and its stride in dwords)."""
        a, p = _i32(slots)
        n = len(a)
        for name, t in rows.items():
            if not (t.is_cuda and t.dim() == 2 and t.shape[0] == n and (t.shape[1] < 2 or t.stride(1) == 1)
                    and t.stride(0) * t.element_size() % 4 == 0 and t.data_ptr() % 4 == 0):
                raise ValueError(f"{who}: {name} must be a 2-D cuda tensor [n, .] with contiguous rows a multiple of 4 bytes apart")
        if report is not None and not (report.is_cuda and report.dtype == torch.int64 and report.is_contiguous() and tuple(report.shape) == (n, width)):
            raise ValueError(f"{who}: the report must be a contiguous int64 cuda tensor [n, {width}]")
        sm, sp = _i32([int(samples)] * n if isinstance(samples, (int, np.integer)) else samples)
        assert len(sm) == n, (n, len(sm))
        return (p, n, sp) + tuple(x for t in rows.values() for x in (_ptr(t), t.stride(0) * t.element_size() // 4))

    def _get_feature(self, key, slots, report=None):
        """A feature's cfg getter: per slot what `report` (default: the feature's keywords) makes of the struct, None for a slot
        without the feature."""
        f = _lib.SLOT_FEATURES[key]
        out = []
        for slot in slots:
            c = f.cfg()
            _lib.check(getattr(self.lib, f.getter)(self.h, int(slot), C.byref(c)))
            out.append((report or f.keywords)(c) if getattr(c, f.on) else None)
        return out

    def _feature_state(self, key, slots):
        """A feature's state rows (joins pipelined work): a numeric tensor [n, columns] (cuda), or for struct rows a list of dicts
        (synchronises)."""
        f = _lib.SLOT_FEATURES[key]
        a, p = _i32(slots)
        struct = isinstance(f.rows, type)
        buf = torch.empty(len(a), C.sizeof(f.rows) if struct else f.rows[1], dtype=torch.uint8 if struct else getattr(torch, f.rows[0]), device=self.dev)
        _lib.check(getattr(self.lib, f.state)(self.h, p, len(a), _ptr(buf), _stream()))
        self._release()
        return _struct_rows(buf, f.rows) if struct else buf

    def _feature_seed_rows(self, key, slots):
        """A feature's opaque state rows uint8 [n, bytes] (cuda), which its setter takes back as seed=.  Joins pipelined work."""
        f = _lib.SLOT_FEATURES[key]
        a, p = _i32(slots)
        nbytes = int(_lib.check(getattr(self.lib, f.seed_bytes)(*([self.h] if _lib._PROTOS[f.seed_bytes][1] else []))))
        out = torch.empty(len(a), nbytes, dtype=torch.uint8, device=self.dev)
        _lib.check(getattr(self.lib, f.seed_state)(self.h, p, len(a), _ptr(out), nbytes, _stream()))
        self._release()
        return out

    def _last_rows(self, key, k, dtype=torch.int32):
        """What the last wav-in call left for a feature (joins pipelined work): k tensors [n, seg] in call order."""
        n = self._last_wav_n
        bufs = [torch.empty(max(n, 1), self.seg, dtype=dtype, device=self.dev) for _ in range(k)]      # (before any wav-in call the library answers CONAN_ERR_STATE)
        _lib.check(getattr(self.lib, _lib.SLOT_FEATURES[key].last)(self.h, *[_ptr(b) for b in bufs], _stream()))
        self._release()
        return tuple(b[:n] for b in bufs)

    def _release(self):
        """Buffers of pipelined steps may be dropped once the current torch stream waits for the library's internal
        streams (every stream-ordered entry point joins them in C).  Those streams are invisible to torch's caching
        allocator, so each buffer is first marked as in use on the current stream: its block then returns to the
        pool only after work enqueued here - which sits behind the join - has completed."""
        if self._keep:
            cur = torch.cuda.current_stream()
            for group in self._keep:
                for t in group:
                    if t is not None and t.is_cuda:
                        t.record_stream(cur)
            self._keep.clear()

    def reset(self, slots, which=7):
        a, p = _i32(slots)
        _lib.check(self.lib.conan_streams_reset(self.h, p, len(a), which, _stream()))
        self._release()

    def set_input_rate(self, slots, rate, **filter):
        """conan_streams_set_input_rate: the slots' wav-in input arrives at `rate` Hz and is resampled on the GPU to the model rate
        (hop * 50) in front of the streaming front-end.  filter: Context.resample's filter keywords (lowpass_filter_width, rolloff,
        resampling_method, beta, or preset='hann' / 'kaiser_best'; default hann).  The slots must be at the start of an utterance;
        the rate survives CONAN_MODEL_FRONTEND resets; rate == the model rate restores the model-rate path."""
        a, p = _i32(slots)
        cfg = _lib.resample_cfg(rate, self.model_rate, **filter)
        _lib.check(self.lib.conan_streams_set_input_rate(self.h, p, len(a), C.byref(cfg)))
        self.input_rate_set = True
        self._drift_slots("input").difference_update(int(s) for s in a)

    def set_output_rate(self, slots, rate, **filter):
        """conan_streams_set_output_rate: the slots' audio leaves every step at `rate` Hz, resampled on the GPU behind the vocoder.
        filter: Context.resample's filter keywords (default hann).  The slots must be at the start of their vocoder stream; the rate
        survives resets; rate == the model rate restores the model-rate path.  A step then delivers what the filter has the inputs
        for (output_samples) and flush_output the tail; rows above the model rate need set_output_ld."""
        a, p = _i32(slots)
        cfg = _lib.resample_cfg(self.model_rate, rate, **filter)
        _lib.check(self.lib.conan_streams_set_output_rate(self.h, p, len(a), C.byref(cfg)))
        self._drift_slots("output").difference_update(int(s) for s in a)
        for slot in a:
            if int(rate) != self.model_rate:
                self.output_rates[int(slot)] = int(rate)
            else:
                self.output_rates.pop(int(slot), None)

    def _drift_slots(self, side):
        """The set of slots with a drift resampler on `side` ('input' / 'output'): the attributes input_drifts / output_drifts."""
        return self.__dict__.setdefault(side + "_drifts", set())

    def set_input_drift(self, slots, ppm, rate=None, **filter):
        """conan_streams_set_input_drift: clock-drift compensation of the slots' wav-in input.  ppm: the far device's clock error
        (> 0: it runs fast; one value or one per slot; round(ppm * 1000) ppb).  rate given: configure - the input arrives at `rate`
        Hz (the model rate is allowed) and goes through the drift resampler (filter: Context.resample's keywords) in place of the
        rational one; the slots must be at the start of an utterance.  rate=None: a live change between calls, taking effect at the
        slot's next output.  A configured slot takes 0 .. 2 * (80 ms) samples per call and may emit no frame in a call."""
        a, p = _i32(slots)
        ppb = _lib.drift_ppb_rows(ppm, len(a))
        cfg = _lib.resample_cfg(rate, self.model_rate, **filter) if rate is not None else None
        _lib.check(self.lib.conan_streams_set_input_drift(self.h, p, len(a), C.byref(cfg) if cfg is not None else None, ppb.ctypes.data))
        if rate is not None:
            self.input_rate_set = True
            self._drift_slots("input").update(int(s) for s in a)

    def _drift_query(self, fn, slots):
        a, p = _i32(slots)
        ppb, i, o = np.zeros(len(a), dtype=np.int32), np.zeros(len(a), dtype=np.int64), np.zeros(len(a), dtype=np.int64)
        _lib.check(fn(self.h, p, len(a), ppb.ctypes.data, i.ctypes.data, o.ctypes.data))
        return [(int(ppb[k]) / 1000.0, int(i[k]), int(o[k])) for k in range(len(a))]

    def input_drift(self, slots):
        """conan_streams_input_drift: per slot (ppm in force, input samples received, model-rate samples handed to the front-end)."""
        return self._drift_query(self.lib.conan_streams_input_drift, slots)

    def set_output_drift(self, slots, ppm, rate=None, **filter):
        """conan_streams_set_output_drift: clock-drift compensation of the slots' audio output, as set_input_drift: rate given
        configures (the slots at the start of their vocoder stream; the audio leaves at `rate` Hz through the drift resampler),
        rate=None changes ppm between steps.  A step delivers what is ready (output_samples) and flush_output the tail; a fast
        sink takes more than frames * hop samples per step: set_output_ld."""
        a, p = _i32(slots)
        ppb = _lib.drift_ppb_rows(ppm, len(a))
        cfg = _lib.resample_cfg(self.model_rate, rate, **filter) if rate is not None else None
        _lib.check(self.lib.conan_streams_set_output_drift(self.h, p, len(a), C.byref(cfg) if cfg is not None else None, ppb.ctypes.data))
        if rate is not None:
            for slot in a:
                self.output_rates[int(slot)] = int(rate)      # (the steps' wav is then a list of rows trimmed to their counts)
                self._drift_slots("output").add(int(slot))

    def output_drift(self, slots):
        """conan_streams_output_drift: per slot (ppm in force, model-rate samples produced, output samples delivered)."""
        return self._drift_query(self.lib.conan_streams_output_drift, slots)

    def set_input_format(self, slots, fmt):
        """conan_streams_set_input_format: the slots' wav-in rows arrive as 'f32' (float32), 's16' (int16), 'ulaw' or 'alaw' (uint8,
        G.711) and are decoded on the GPU.  Stateless: takes effect from the next call, survives resets; 'f32' restores the default."""
        a, p = _i32(slots)
        _lib.check(self.lib.conan_streams_set_input_format(self.h, p, len(a), _lib.sample_format(fmt)))
        self._note_format(self.input_formats, a, fmt)

    def set_input_level(self, slots, cfg=True, **kw):
        """conan_streams_set_input_level: a causal BS.1770 leveller on the slots' model-rate samples, behind format decoding and the
        input resampler, in front of the streaming front-end.  Context.level's keywords (target, max_boost_db, max_cut_db,
        initial_gain_db, window_blocks, peak_limit, clip) set it, as keywords or as a dict in cfg; those not given keep
        Context.level's defaults, so set_input_level(slots) is the default leveller.  Only cfg=None turns it off.
        The slots must be at the start of an utterance; the setting survives resets, which clear the meter.
        input_levels[slot] holds every keyword of a levelled slot, as SlotSnapshot.info reports them."""
        self._set_feature("level", slots, cfg, kw)

    def set_pitch(self, slots, cfg=True, **kw):
        """conan_streams_set_pitch: the slots' pitch control in the decoder step - shift_semitones (a key change), range (the
        contour's excursion around `pivot`, log2 Hz: 1 unchanged, 0 monotone), uv_threshold (a frame is unvoiced when the head's d0
        exceeds it: +inf voices every frame whose code is not the silent token, -inf whispers) - as keywords or as a dict in cfg;
        those not given keep _lib.pitch_cfg's defaults.  Only cfg=None turns it off.  It may be called at any time, also
        mid-utterance (it joins pipelined work); the change takes effect from the next step and survives resets."""
        self._set_feature("pitch", slots, cfg, kw)

    def set_pitch_follow(self, slots, cfg=True, **kw):
        """conan_streams_set_pitch_follow: the slots' decoder steps take f0 / uv from the YIN contour of their own input (wav-in steps
        only), so the converted voice keeps the source's melody; the slots' pitch control (set_pitch) applies on top.  Context.f0's
        tracker keywords (fmin, fmax, threshold, floor_db) as keywords or as a dict in cfg; those not given keep the defaults.  Only
        cfg=None turns it off.  It may be called at any time, also mid-utterance (it joins pipelined work); the change takes effect
        from the next emitted chunk and survives resets.  Slot snapshots do not carry it."""
        self._set_feature("follow", slots, cfg, kw)

    def pitch_follow(self, slots):
        """conan_streams_pitch_follow: per slot the tracker's keywords as set_pitch_follow takes them, None for a slot that does not
        follow."""
        return self._get_feature("follow", slots)

    def set_pitch_register(self, slots, target=None, cfg=True, max_shift=2.0, prior=None, prior_frames=50, seed=None, reseed=False):
        """conan_streams_set_pitch_register: register matching for slots that follow (set_pitch_follow) - the causal log-f0 mean
        transform moves each slot's mean log-f0 to `target` (log2 Hz; VoiceBank.registers / Context.register_of of the target voice)
        by at most max_shift octaves, so a converted voice sits in the target's register, not the source's.  The estimate starts
        from seed = (count, sum) - a state queried with pitch_register: the hand-over - or from prior_frames frames at `prior`
        (default: the target).  cfg: a dict of these keywords instead; cfg=None turns it off.  It restarts from the seed when a slot
        is enabled, after reseed=True and at the first chunk after a reset of the front-end; a call with reseed=False on an enabled
        slot changes target / max_shift from the next emitted chunk and keeps the estimate.  Slot snapshots do not carry it."""
        self._set_feature("register", slots, cfg, {}, dict(target=target, max_shift=max_shift, prior=prior, prior_frames=prior_frames, seed=seed, reseed=reseed))

    def pitch_register(self, slots):
        """Per slot dict(target, max_shift, count, sum, mean, shift) - the setting (conan_streams_pitch_register) and the estimate
        (conan_streams_pitch_register_state; joins pipelined work, synchronises): (count, sum) = the state, mean = sum / (count * 2^22)
        in log2 Hz and shift = the clamped target - mean in octaves (None while count is 0) - or None for a slot without the register."""
        slots = [int(x) for x in slots]
        cfgs = self._get_feature("register", slots, report=lambda c: c)
        on = [slot for slot, c in zip(slots, cfgs) if c is not None]
        states = dict(zip(on, self._feature_state("register", on).cpu().tolist())) if on else {}
        out = []
        for slot, c in zip(slots, cfgs):
            if c is None:
                out.append(None)
                continue
            k, S = states[slot]
            mean = S / (k * float(_lib.REGISTER_UNIT)) if k else None
            shift = None if mean is None else min(max(c.target - mean, -c.max_shift), c.max_shift)
            out.append(dict(target=c.target, max_shift=c.max_shift, count=k, sum=S, mean=mean, shift=shift))
        return out

    def set_activity(self, slots, cfg=True, gate=True, **kw):
        """conan_streams_set_activity: a causal voice-activity detector on the slots' own input (wav-in steps only), on the frames
        the front-end reads, one more launch per call; gate=True (mode 2) also gates the vocoder's audio of the slots, click-free,
        in front of the output resampler and encoder; gate=False (mode 1) only detects.  **kw / a dict in cfg: _lib.activity_cfg's
        keywords (thresholds, hangover, attack / release, seed=, reseed=); cfg may also be an _lib.ActivityCfg; only cfg=None turns it
        off.  It may be called at any time (it joins pipelined work); the change takes effect from the next emitted chunk and
        survives resets.  The state restarts from the seed when a slot is enabled, after reseed=True and at the first chunk after a
        reset of the front-end; reseed=False on an enabled slot replaces the parameters and keeps the state.  Slot snapshots do not
        carry it: query activity_state, export, import, then set_activity(seed=state, reseed=True)."""
        self._set_feature("activity", slots, cfg, kw, dict(gate=gate))

    def activity(self, slots):
        """conan_streams_activity: per slot the setting as _lib.activity_keywords reports it (set_activity takes it back), None for a
        slot without the detector."""
        return self._get_feature("activity", slots)

    def activity_state(self, slots):
        """conan_streams_activity_state (joins pipelined work, synchronises): per slot dict(active, hang, level, floor, frames,
        active_frames); a slot whose state is about to restart reports its seed.  A slot without the detector is an error."""
        return self._feature_state("activity", slots)

    def step_wav_activity(self):
        """The flags and frame-end gate levels the last wav-in call produced (conan_step_wav_activity; joins pipelined work) ->
        (act [n, seg] int32, level [n, seg] int32) in call order; rows without the detector, rows that emitted nothing and entries
        past a row's emitted frames are 0."""
        return self._last_rows("activity", 2)

    def set_bypass(self, slots, cfg=True, wet=1.0, dry=0.0, ramp_ms=40.0, fill_gate=False, start=None, reseed=False, **kw):
        """conan_streams_set_bypass: a latency-matched dry path and a wet/dry mix on the slots' output (wav-in steps only).  The chunk's
        source samples - at the model rate, behind decoding, the input resampler and the leveller - are mixed with the vocoder's audio
        behind the activity gate and in front of the output resampler and encoder: out = wet * converted + dry * source, sample for
        sample aligned.  wet / dry: the targets as linear shares (wet_db= / dry_db=: in decibels); ramp_ms: the time a full-scale
        change takes, in steps of one 20 ms frame, linear inside a frame (step=: levels per frame directly); fill_gate: the dry share is
        scaled by the closed part of the slot's activity gate (room tone in pauses: set_activity(gate=True) beside it); start: the
        (wet, dry) integer levels a restart begins from (default: the targets).  cfg: True, a dict of these keywords, an
        _lib.BypassCfg, or None, which turns the feature off.  The defaults are choices, not measurements.
        It may be called at any time (it joins pipelined work); the change takes effect from the next emitted chunk and survives
        resets.  The levels restart from `start` when a slot is enabled, after reseed=True and at the first chunk after a reset of the
        front-end; reseed=False on an enabled slot replaces targets, ramp and fill_gate and keeps the levels - the toggle.  Slot
        snapshots do not carry it: query bypass_state, export, import, then set_bypass(start=(wet, dry), reseed=True)."""
        self._set_feature("bypass", slots, cfg, kw, dict(wet=wet, dry=dry, ramp_ms=ramp_ms, fill_gate=fill_gate, start=start, reseed=reseed))

    def bypass(self, slots):
        """conan_streams_bypass: per slot the setting as _lib.bypass_keywords reports it (set_bypass takes it back), None for a slot
        without the feature."""
        return self._get_feature("bypass", slots)

    def bypass_state(self, slots):
        """conan_streams_bypass_state (joins pipelined work, synchronises): per slot dict(wet, dry, dry_eff), the levels after the
        slot's last emitted frame; a slot whose levels are about to restart reports its seed.  A slot without the feature is an error."""
        return self._feature_state("bypass", slots)

    def step_wav_bypass(self):
        """The frame-end wet and effective dry levels the last wav-in call produced (conan_step_wav_bypass; joins pipelined work) ->
        (wet [n, seg] int32, dry [n, seg] int32) in call order; rows without the feature, rows that emitted nothing and entries past a
        row's emitted frames are 0."""
        return self._last_rows("bypass", 2)

    def set_comfort(self, slots, cfg=True, **kw):
        """conan_streams_set_comfort: comfort noise in place of the silence of a closed activity gate (wav-in steps only; the slot needs
        set_activity beside it, and is filled where that gates the output).  Synthetic noise at the level of the source's background
        - tracked per frame from the detector's flags and frame powers - is cross-faded against the gate's ramp, behind the wet/dry
        mix and in front of the output resampler and encoder; nothing of the caller's room passes.  **kw / a dict in cfg:
        _lib.comfort_cfg's keywords (follow, level_db, offset_db, min_db, max_db, rise_db, fall_db, colour, start_db, seed, reseed);
        cfg may also be an _lib.ComfortCfg; only cfg=None turns it off.  The defaults are choices, not measurements.
        It may be called at any time (it joins pipelined work); the change takes effect from the next emitted chunk and survives
        resets.  The level restarts from the start level when a slot is enabled, after reseed=True and at the first chunk after a
        reset of the front-end; reseed=False on an enabled slot replaces the parameters and keeps the level.  Slot snapshots do not
        carry it: query comfort_state, export, import, then set_comfort(start=level, reseed=True)."""
        self._set_feature("comfort", slots, cfg, kw)

    def comfort(self, slots):
        """conan_streams_comfort: per slot the setting as _lib.comfort_keywords reports it (set_comfort takes it back), None for a slot
        without the feature."""
        return self._get_feature("comfort", slots)

    def comfort_state(self, slots):
        """conan_streams_comfort_state (joins pipelined work, synchronises): per slot dict(level, idle_frames), the comfort level after
        the slot's last emitted frame; a slot whose level is about to restart reports its start level.  A slot without the feature
        is an error."""
        return self._feature_state("comfort", slots)

    def step_wav_comfort(self):
        """The frame-end comfort levels the last wav-in call produced (conan_step_wav_comfort; joins pipelined work) -> [n, seg] int32
        in call order; rows without the feature (or without a detector), rows that emitted nothing and entries past a row's emitted
        frames are 0.  _lib.comfort_dbov turns a level into the RFC 3389 noise level byte."""
        return self._last_rows("comfort", 1)[0]

    def set_tones(self, slots, cfg=True, **kw):
        """conan_streams_set_tones: a DTMF detector on the slots' own input (wav-in steps only), on the audio the activity detector
        reads, one more launch per call; regenerate=True (mode 2, the default) also replaces the slots' output, while a digit is
        confirmed, by a tone pair synthesised from a table, behind every other in-place stage and in front of the output resampler
        and encoder, so that a DTMF receiver behind the engine hears the key; regenerate=False (mode 1) only detects.  Nothing of the
        source audio passes.  **kw / a dict in cfg: _lib.tone_cfg's keywords (level_db, twist_db, sel, share, on_frames, off_frames,
        min_frames, ramp_ms, gain, seed=, reseed=); cfg may also be an _lib.ToneCfg; only cfg=None turns it off.  The defaults are
        choices: talk-off against real speech has not been measured.
        It may be called at any time (it joins pipelined work); the change takes effect from the next emitted chunk and survives
        resets.  The state restarts from the seed when a slot is enabled, after reseed=True and at the first chunk after a reset of the
        front-end; reseed=False on an enabled slot replaces the parameters and keeps the state.  Slot snapshots do not carry it:
        query tone_state, export, import, then set_tones(seed=state, reseed=True)."""
        self._set_feature("tones", slots, cfg, kw, dict(hop=self.model_rate // 50))

    def tones(self, slots):
        """conan_streams_tones: per slot the setting as _lib.tone_keywords reports it (set_tones takes it back), None for a slot
        without the detector."""
        return self._get_feature("tones", slots)

    def tone_state(self, slots):
        """conan_streams_tone_state (joins pipelined work, synchronises): per slot dict(cand, run, cur, miss, held, sound, level, events,
        frames); a slot whose state is about to restart reports its seed.  A slot without the detector is an error."""
        return self._feature_state("tones", slots)

    def step_wav_tones(self):
        """The frame rows the last wav-in call produced (conan_step_wav_tones; joins pipelined work) -> (digit [n, seg], sound [n, seg],
        level [n, seg]) int32 in call order: the confirmed digit of each frame (-1: none; _lib.TONE_KEYS[d] is its key and
        _lib.tone_events lists the presses), the pair the regeneration sounds and its level.  Rows without the detector, rows that
        emitted nothing and entries past a row's emitted frames are 0."""
        return self._last_rows("tones", 3)

    def step_wav_contour(self):
        """The contour the last wav-in call handed the decoder (conan_step_wav_contour; joins pipelined work) -> (f0 [n, seg] log2 Hz,
        uv [n, seg]) in call order; rows that do not follow, and entries past a row's emitted frames, are 0."""
        return self._last_rows("follow", 2, torch.float32)

    def pitch(self, slots):
        """conan_streams_pitch: per slot the pitch control's keywords as set_pitch takes them, None for a slot without one."""
        return self._get_feature("pitch", slots)

    def input_level(self, slots):
        """conan_streams_input_level: float64 [n, 4] (cuda) rows (L_k, G_k, P_k, J_k) of the slots' latest update instants - the
        loudness read, the gain the current ramp ends at, the peak so far, the complete blocks.  Joins pipelined work."""
        return self._feature_state("level", slots)

    def set_output_level(self, slots, cfg=True, seed=None, **kw):
        """conan_streams_set_output_level: the same causal BS.1770 leveller on the slots' own vocoder audio, between conv_post and the
        activity gate, the wet/dry mix, the output resampler and the encoders.  set_input_level's keyword rules: Context.level's
        keywords as keywords or as a dict in cfg, the rest at their defaults; only cfg=None turns it off.  Without a seed the slots
        must be at the start of their vocoder streams; seed: uint8 [n, bytes] (cuda) rows of output_level_state from a stream at the
        same position (a hand-over).  The setting survives resets, which restart the meter.  output_levels[slot] holds every keyword
        of a levelled slot."""
        self._set_feature("out_level", slots, cfg, kw, seed=seed)

    def output_level(self, slots):
        """conan_streams_output_level: float64 [n, 4] (cuda) rows (L_k, G_k, P_k, J_k) of the instant the slots' latest ramps end at.
        Joins pipelined work."""
        return self._feature_state("out_level", slots)

    def output_level_state(self, slots):
        """conan_streams_output_level_state: uint8 [n, bytes] (cuda), the slots' leveller states for set_output_level(seed=).  Joins
        pipelined work."""
        return self._feature_seed_rows("out_level", slots)

    def set_conceal(self, slots, cfg=True, rate=None, seed=None, **kw):
        """conan_streams_set_conceal: loss concealment on the slots' wav-in rows (include/conan_hip.h, conan_conceal_cfg).  cfg: True
        (the defaults of `rate`, the slots' input rate; None: the model rate), a dict of fields over those defaults, an
        _lib.ConcealCfg, or None, which turns the feature off; keywords are fields too.  seed: uint8 [n, bytes] (cuda) rows of
        conceal_state (a hand-over).  It may be called at any time (it joins pipelined work) and survives resets; the state restarts
        when a slot that was off is enabled and at the first repair after a reset of the front-end.  Slot snapshots do not carry it.
        The repair itself is conceal(), or lost= on the wav-in steps."""
        self._set_feature("conceal", slots, cfg, kw, dict(rate=self.model_rate if rate is None else int(rate)), seed=seed)

    def conceal_cfg(self, slots):
        """conan_streams_conceal_cfg: per slot the dict of its fields (set_conceal takes it back), None for a slot without the feature."""
        return self._get_feature("conceal", slots)

    def conceal(self, slots, wav, samples, lost):
        """conan_streams_conceal: repairs the lost packets of the rows IN PLACE, in front of the step call that takes them.  wav: a
        2-D cuda tensor with one row per slot, contiguous rows a multiple of 4 bytes apart, row i in the format of slots[i] (a
        float32 tensor for f32 slots; for other or mixed formats the packed uint8 rows the steps build); samples: an int or one per
        row; lost [n, >= ceil(samples / packet)] integer or bool, non-zero = lost.  Rows of slots without the feature and rows
        without samples keep their bytes.  -> wav"""
        args = self._call_rows("conceal", slots, samples, wav=wav)
        flags = lost.to(self.dev).reshape(args[1], -1).to(torch.int32).contiguous()
        _lib.check(self.lib.conan_streams_conceal(self.h, *args, _ptr(flags), flags.shape[1], _stream()))
        return wav

    def conceal_state(self, slots):
        """conan_streams_conceal_state: uint8 [n, bytes] (cuda), the slots' concealment states for set_conceal(seed=).  Joins pipelined
        work."""
        return self._feature_seed_rows("conceal", slots)

    def set_echo(self, slots, cfg=True, rate=None, seed=None, **kw):
        """conan_streams_set_echo: echo cancellation on the slots' wav-in rows (include/conan_hip.h, conan_echo_cfg).  cfg: True (the
        defaults of `rate`, the slots' input rate; None: the model rate), a dict of fields over those defaults, an _lib.EchoCfg, or
        None, which turns the feature off; keywords are fields too.  seed: uint8 [n, bytes] (cuda) rows of echo_state (a
        hand-over).  It may be called at any time (it joins pipelined work) and survives resets; an enabled slot keeps its state (a
        changed taps keeps the weights that still exist), which restarts when a slot that was off is enabled and at the first echo
        call after a reset of the front-end.  Slot snapshots do not carry it.  The cancellation itself is echo(), or far= on the
        wav-in steps."""
        self._set_feature("echo", slots, cfg, kw, dict(rate=self.model_rate if rate is None else int(rate)), seed=seed)

    def echo_cfg(self, slots):
        """conan_streams_echo_cfg: per slot the dict of its fields (set_echo takes it back), None for a slot without the feature."""
        return self._get_feature("echo", slots)

    def echo(self, slots, wav, samples, far, stats=None):
        """conan_streams_echo: cancels the far end's echo in the rows IN PLACE, in front of the step call that takes them and behind
        conceal().  wav, far: 2-D cuda tensors with one row per slot, contiguous rows a multiple of 4 bytes apart, row i in the
        format of slots[i] (as conceal()'s wav); samples: an int or one per row; stats: an int64 cuda tensor [n, 4] to fill (per row
        sum d^2, sum e^2, blocks adapted and frozen in this call) or None.  Rows of slots without the feature and rows without
        samples keep their bytes.  -> wav"""
        args = self._call_rows("echo", slots, samples, stats, 4, wav=wav, far=far)
        _lib.check(self.lib.conan_streams_echo(self.h, *args, _ptr(stats), _stream()))
        return wav

    def echo_state(self, slots):
        """conan_streams_echo_state: uint8 [n, bytes] (cuda), the slots' canceller states for set_echo(seed=).  Joins pipelined work."""
        return self._feature_seed_rows("echo", slots)

    def set_echo_delay(self, slots, cfg=True, rate=None, seed=None, **fields):
        """conan_streams_set_echo_delay: the echo-delay estimator on the slots' wav-in rows (include/conan_hip.h,
        conan_echo_delay_cfg).  cfg: True (the defaults of `rate`, the slots' input rate; None: the model rate), a dict of fields
        over those defaults, an _lib.EchoDelayCfg, or None, which turns the feature off; keywords are fields too.  seed: uint8
        [n, bytes] (cuda) rows of echo_delay_state (a hand-over).  It may be called at any time (it joins pipelined work) and
        survives resets; an enabled slot keeps its state (a changed n_lags keeps the sums that still exist), which restarts when a
        slot that was off is enabled and at the first estimator call after a reset of the front-end.  Slot snapshots do not carry
        it, and the slot needs no canceller.  The estimate itself is echo_delay(), or far= on the wav-in steps."""
        slots = [int(s) for s in slots]
        if cfg is None or cfg is False:      # (False: the engine's "none")
            cfg = None
        else:      # a struct from every form _rate_cfg takes; keywords go over a struct's fields as over a dict's
            if fields:
                cfg = dict(_lib.echo_delay_keywords(cfg) if isinstance(cfg, _lib.EchoDelayCfg) else cfg if isinstance(cfg, dict) else {}, **fields)
            cfg, fields = _rate_cfg("echo_delay", cfg, self.model_rate if rate is None else int(rate)), {}
        c = self._set_feature("echo_delay", slots, cfg, fields, seed=seed)
        (self.echo_delays.update if c.enabled else self.echo_delays.difference_update)(slots)

    def echo_delay_cfg(self, slots):
        """conan_streams_echo_delay_cfg: per slot the dict of its fields (set_echo_delay takes it back), None for a slot without."""
        return self._get_feature("echo_delay", slots)

    def echo_delay(self, slots, wav, samples, far, report=None):
        """conan_streams_echo_delay: the estimator READS the rows and the far rows - in front of echo(), which rewrites wav, and
        behind conceal() - and updates the slots' states.  wav, far, samples: as echo()'s; report: an int64 cuda tensor [n, 6] to
        fill (per row est, age, cand, run, last_pk, last_s after the call; _lib.ECHO_DELAY_REPORT) or None.  Rows of slots without
        the feature and rows without samples are skipped and report zeros.  -> report"""
        args = self._call_rows("echo_delay", slots, samples, report, 6, wav=wav, far=far)
        _lib.check(self.lib.conan_streams_echo_delay(self.h, *args, _ptr(report), _stream()))
        return report

    def echo_delay_state(self, slots):
        """conan_streams_echo_delay_state: uint8 [n, bytes] (cuda), the slots' estimator states for set_echo_delay(seed=).  Joins
        pipelined work."""
        return self._feature_seed_rows("echo_delay", slots)

    def _far_stages(self, a, wav, samples, far_rows, echo_stats, echo_delay_report):
        """far= of a wav-in step: the delay estimator of the slots that have one reads the rows, then the canceller rewrites them."""
        if self.echo_delays:
            self.echo_delay(a, wav, samples, far_rows, echo_delay_report)
        self.echo(a, wav, samples, far_rows, echo_stats)

    def set_denoise(self, slots, cfg=True, seed=None, **kw):
        """conan_streams_set_denoise: noise suppression on the slots' wav-in frames (include/conan_hip.h, conan_denoise_cfg): a causal
        spectral gate on the log-mel frames the front-end has just computed, under a per-band noise floor tracked per frame, in place
        in the slot's mel ring and in the chunk the step consumes.  No latency, no second spectral pipeline; the audio ring, and with
        it the f0 tracker, the detector, the dry path and the leveller, is untouched.  **kw / a dict in cfg: _lib.denoise_cfg's
        keywords; cfg may also be an _lib.DenoiseCfg; only cfg=None turns it off.  The defaults are choices, not measurements.
        It may be called at any time (it joins pipelined work) and survives resets.  The state restarts at the slot's next frame
        when a slot is enabled, after reseed=True and after a reset of the front-end - from its row of seed (uint8 [n, bytes] cuda
        rows of denoise_state) where one is given; reseed=False on an enabled slot replaces the parameters and keeps the state.
        Slot snapshots do not carry it: query denoise_state, export, import, then set_denoise(seed=rows, reseed=True)."""
        self._set_feature("denoise", slots, cfg, kw, seed=seed)

    def denoise(self, slots):
        """conan_streams_denoise: per slot the setting as _lib.denoise_keywords reports it (set_denoise takes it back), None for a slot
        without the feature."""
        return self._get_feature("denoise", slots)

    def denoise_state(self, slots):
        """conan_streams_denoise_state: uint8 [n, bytes] (cuda), the slots' conan_denoise_state records (_lib.DenoiseState reads one:
        frames, bins, the noise floor and the attenuation per bin) for set_denoise(seed=) and Context.mel_denoise(seed=).  Joins
        pipelined work."""
        return self._feature_seed_rows("denoise", slots)

    def set_input_eq(self, slots, cfg=True, seed=None, **kw):
        """conan_streams_set_input_eq: an equaliser on the slots' SOURCE audio (wav-in steps only; include/conan_hip.h, conan_eq_cfg):
        a cascade of 1 .. 4 biquad sections in f64 on the model-rate samples the front-end is about to read, one more launch per
        call, in front of the leveller - so the audio ring and everything that reads it see the filtered source.  **kw / a dict in
        cfg: _lib.eq_cfg's keywords (sections=[...]: raw 5-tuples or dict(kind=, f=, q=, gain_db=) designed at the model rate); cfg
        may also be an _lib.EqCfg; only cfg=None turns it off.  No cascade is a default: any example is a choice nobody has
        listened to.  It may be called at any time (it joins pipelined work) and survives resets.  Enabling starts from zero at the
        current position; changing an enabled slot closes its pending tail with the old coefficients and keeps the sections' state
        words - the live tone control, no click.  seed: uint8 [n, 592] cuda rows of input_eq_state with origin= and pos= as
        input_eq reports them: the slot continues that stream.  Slot snapshots do not carry it: query input_eq and input_eq_state,
        export, import, then set_input_eq(cfg=the keywords, seed=rows)."""
        self._set_feature("eq", slots, cfg, kw, dict(rate=self.model_rate), seed=seed)

    def input_eq(self, slots):
        """conan_streams_input_eq: per slot the setting as _lib.eq_keywords reports it - the sections as raw 5-tuples, the grid's
        origin and the slot's position (set_input_eq takes it back) - None for a slot without the feature."""
        return self._get_feature("eq", slots)

    def input_eq_state(self, slots):
        """conan_streams_input_eq_state: uint8 [n, 592] (cuda), the slots' conan_eq_state records (_lib.EqState reads one) for
        set_input_eq(seed=) and Context.eq(seed=).  Joins pipelined work."""
        return self._feature_seed_rows("eq", slots)

    def set_output_eq(self, slots, cfg=True, seed=None, **kw):
        """conan_streams_set_output_eq: the same equaliser on the audio the slots emit - a tone control, a telephone band, a
        de-emphasis - in place directly behind the vocoder and in front of the output leveller, the gate, the mix, the output
        resampler and the encoders: one more launch per vocoder step with a filtered row, in every step entry point.  Arguments,
        live changes, seed and hand-over as set_input_eq (output_eq, output_eq_state)."""
        self._set_feature("out_eq", slots, cfg, kw, dict(rate=self.model_rate), seed=seed)

    def output_eq(self, slots):
        """conan_streams_output_eq: as input_eq."""
        return self._get_feature("out_eq", slots)

    def output_eq_state(self, slots):
        """conan_streams_output_eq_state: as input_eq_state."""
        return self._feature_seed_rows("out_eq", slots)

    def set_watermark(self, slots, cfg=True, seed=None, **kw):
        """conan_streams_set_watermark: a keyed mark in the audio the slots emit (include/conan_hip.h, conan_watermark_cfg): a +-1
        chip sequence under a causal peak envelope, added on the GPU behind the comfort fill and in front of the output resampler and
        the encoders, one more launch per vocoder step that carries a marked row, in every step entry point.  Context.watermark_detect
        finds it again.  **kw / a dict in cfg: _lib.watermark_cfg's keywords (key, id, gain, floor); cfg may also be an
        _lib.WatermarkCfg; only cfg=None turns it off.  The defaults are choices, not measurements.  It may be called at any time
        (it joins pipelined work) and survives resets.  The state (position and envelope) restarts when a slot that was off is
        enabled, after reseed=True and after a reset with the vocoder - from seed (uint8 [n, 16] cuda: rows of watermark_state) where
        one is given; reseed=False on an enabled slot replaces key, id, gain and floor and keeps the state.  Slot snapshots do not
        carry it: query watermark_state, export, import, then set_watermark(seed=rows, reseed=True)."""
        self._set_feature("watermark", slots, cfg, kw, seed=seed)

    def watermark(self, slots):
        """conan_streams_watermark: per slot the setting as _lib.watermark_keywords reports it (set_watermark takes it back), None for
        a slot without the mark."""
        return self._get_feature("watermark", slots)

    def watermark_state(self, slots):
        """conan_streams_watermark_state: uint8 [n, 16] (cuda), the slots' conan_watermark_state records (_lib.WatermarkState reads
        one: pos, env) for set_watermark(seed=) and Context.watermark_embed(seed=).  Joins pipelined work."""
        return self._feature_seed_rows("watermark", slots)

    def set_output_format(self, slots, fmt):
        """conan_streams_set_output_format: the slots' audio leaves every step (and flush_output) as 'f32', 's16', 'ulaw' or 'alaw',
        encoded on the GPU behind the vocoder and the output resampler.  Row strides stay in 4-byte units; counts stay in samples."""
        a, p = _i32(slots)
        _lib.check(self.lib.conan_streams_set_output_format(self.h, p, len(a), _lib.sample_format(fmt)))
        self._note_format(self.output_formats, a, fmt)

    @staticmethod
    def _note_format(table, slots, fmt):
        for slot in slots:
            if fmt in (None, "f32"):
                table.pop(int(slot), None)
            else:
                table[int(slot)] = fmt

    def _out_dtype(self, slot):
        return SAMPLE_DTYPES[self.output_formats.get(int(slot), "f32")]

    def wav_row(self, wav, i, slot, count):
        """Row i of a step's 2-D wav buffer in its slot's output dtype, its first `count` samples."""
        return wav[i].view(self._out_dtype(slot))[:count]

    def wav_block(self, wav, slots, count, ld=None):
        """A step's wav buffer (rows `ld` floats apart) as one [n, count] view in the slots' common output dtype."""
        dts = {self._out_dtype(s) for s in slots}
        if len(dts) != 1:
            raise ValueError("the slots deliver different sample formats: take the rows one by one (wav_row)")
        n = len(slots)
        ld = ld or wav.numel() // n
        return wav.view(-1)[:n * ld].view(n, ld).view(dts.pop())[:, :count]

    def _in_rows(self, slots, wav, min_ld):
        """The wav-in rows as the library takes them: (buffer, row stride in 4-byte units, samples per row).  wav: one 2-D tensor
        (rows of one dtype) or a list of 1-D tensors, each in its slot's dtype (float32, int16 for 's16', uint8 for G.711)."""
        n = len(slots)
        rows = list(wav) if isinstance(wav, (list, tuple)) else None
        if rows is None and wav.dtype not in (torch.int16, torch.uint8):
            wav = wav.to(self.dev, torch.float32)
        for i, slot in enumerate(slots):
            want = SAMPLE_DTYPES[self.input_formats.get(int(slot), "f32")]
            got = rows[i].dtype if rows is not None else wav.dtype
            if got != want:
                raise ValueError(f"slot {int(slot)} takes {want} samples (set_input_format), row {i} holds {got}")
        if rows is None:
            assert wav.dim() == 2 and wav.shape[0] == n, wav.shape
            samples = [wav.shape[1]] * n
            if wav.dtype == torch.float32:
                if wav.shape[1] < min_ld:
                    wav = torch.nn.functional.pad(wav, (0, min_ld - wav.shape[1]))
                return wav.to(self.dev).contiguous(), wav.shape[1], samples
            ld = max(min_ld, (wav.shape[1] * wav.element_size() + 3) // 4)
            return _row_bytes(wav.to(self.dev), n, ld, self.dev), ld, samples
        assert len(rows) == n, (n, len(rows))
        ld = max([min_ld] + [(r.numel() * r.element_size() + 3) // 4 for r in rows])
        return _row_bytes([r.to(self.dev) for r in rows], n, ld, self.dev), ld, [r.numel() for r in rows]

    def set_output_ld(self, ld):
        """conan_streams_set_output_ld: row stride (floats) of wav in every step from now on; 0 = each step's own."""
        _lib.check(self.lib.conan_streams_set_output_ld(self.h, int(ld)))
        self.output_ld = int(ld)

    def output_samples(self):
        """Samples the most recent step call wrote to each row of its wav, in call order (known at once, also for pipelined calls)."""
        n = _lib.check(self.lib.conan_streams_output_samples(self.h, None, 0))
        buf = (C.c_int32 * max(n, 1))()
        _lib.check(self.lib.conan_streams_output_samples(self.h, buf, n))
        return [buf[i] for i in range(n)]

    def output_pending(self, slots):
        """What flush_output would deliver for these slots now (0 for a slot without a rate)."""
        a, p = _i32(slots)
        buf = (C.c_int32 * len(a))()
        _lib.check(self.lib.conan_streams_output_pending(self.h, p, len(a), buf))
        return list(buf)

    def flush_output(self, slots, out=None):
        """conan_streams_flush_output: end of utterance -> one 1-D tensor per slot, its remaining output samples (empty without a
        rate).  Joins pipelined work.  The slots refuse further steps until a reset that includes the vocoder."""
        a, p = _i32(slots)
        counts = self.output_pending(slots)
        ld = max(counts + [1])
        wav = out if out is not None else torch.empty(len(a), ld, device=self.dev)
        assert wav.is_cuda and wav.is_contiguous() and wav.dim() == 2 and wav.shape[0] == len(a) and wav.dtype == torch.float32
        _lib.check(self.lib.conan_streams_flush_output(self.h, p, len(a), _ptr(wav), wav.shape[1], _stream()))
        self._release()
        return [self.wav_row(wav, i, a[i], c) for i, c in enumerate(counts)]

    def _wav_rows(self, wav, slots, ld=None):
        """A step's wav as the caller sees it: unchanged on a stream-set without output rate, stride or format, else one 1-D tensor
        per row (rows `ld` floats apart) in its slot's dtype, trimmed to the count the step reported."""
        if not (self.output_rates or self.output_ld or self.output_formats):
            return wav
        n = len(slots)
        counts = self.output_samples()
        ld = ld or wav.numel() // n
        rows = wav.view(-1)[:n * ld].view(n, ld)
        return [self.wav_row(rows, i, slots[i], counts[i]) for i in range(n)]

    @property
    def model_rate(self):
        """The wav-in steps' model rate: hop * 50 (20 ms frames)."""
        return self.ctx.hop * 50

    def set_reference(self, slots, ref_mel, ref_len=None):
        """ref_mel: cuda float32 [n, Tr, 80]."""
        a, p = _i32(slots)
        ref_mel = ref_mel.to(self.dev, torch.float32).contiguous()
        n, tr = ref_mel.shape[0], ref_mel.shape[1]
        if ref_len is None:
            ref_len = [tr] * n
        l, lp = _i32(ref_len)
        _lib.check(self.lib.conan_set_reference(self.h, p, len(a), _ptr(ref_mel), lp, tr, _stream()))
        self._release()

    def set_voice(self, slots, bank, ids):
        """conan_streams_set_voice: slot slots[i] gets voice ids[i] of `bank` (a VoiceBank) - one launch instead of a style pass.
        In the order of the current stream: steps already enqueued keep the old voice, the next one uses the new."""
        a, p = _i32(slots)
        v, vp = _i32(ids)
        if len(v) != len(a):
            raise ValueError(f"set_voice: {len(a)} slots for {len(v)} voice ids")
        _lib.check(self.lib.conan_streams_set_voice(self.h, p, len(a), bank.h, vp, _stream()))
        self._release()

    def set_voice_mix(self, slots, bank, ids, weights):
        """conan_streams_set_voice_mix: ids / weights [n, k] (k <= 4): slot i gets the prosody side of ids[i][0] and the style vector
        sum_k weights[i][k] * style[ids[i][k]] (an fp32 fma chain in k order; the weights are not normalised)."""
        a, p = _i32(slots)
        v = np.ascontiguousarray(np.asarray(ids, dtype=np.int32).reshape(len(a), -1))
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float32).reshape(len(a), -1))
        if v.shape != w.shape:
            raise ValueError(f"set_voice_mix: ids {v.shape} and weights {w.shape} differ")
        _lib.check(self.lib.conan_streams_set_voice_mix(self.h, p, len(a), bank.h, v.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p),
                                                        v.shape[1], _stream()))
        self._release()

    def voice(self, slots):
        """conan_streams_voice: per slot the voice id last assigned whole by set_voice, -1 otherwise."""
        out = []
        for slot in np.atleast_1d(np.asarray(slots, dtype=np.int32)):
            r = C.c_int32(0)
            _lib.check(self.lib.conan_streams_voice(self.h, int(slot), C.byref(r)))
            out.append(int(r.value))
        return out

    def emformer_step(self, slots, chunk, want_out=True, want_logits=True, want_codes=True):
        a, p = _i32(slots)
        n = len(a)
        c = self.ctx.cfg
        chunk = chunk.to(self.dev, torch.float32).contiguous()
        assert chunk.shape == (n, self.seg + self.rc, c.emf_input_dim), chunk.shape
        out = torch.empty(n, self.seg, c.emf_input_dim, device=self.dev) if want_out else None
        logits = torch.empty(n, self.seg, c.emf_output_dim, device=self.dev) if want_logits else None
        codes = torch.empty(n, self.seg, dtype=torch.int32, device=self.dev) if want_codes else None
        _lib.check(self.lib.conan_emformer_step(self.h, p, n, _ptr(chunk), _ptr(out), _ptr(logits), _ptr(codes), _stream()))
        self._release()
        return out, logits, codes

    def emformer_project(self, head, x):
        """x [..., D] (cuda float32) through the checkpoint's output head `head` ('proj' / 'proj1' / 'proj2'):
        conan_emformer_project, a k = 1 conv on the MFMA path."""
        D = self.ctx.cfg.emf_input_dim
        x2 = x.to(self.dev, torch.float32).reshape(-1, D).contiguous()
        K = int(self.lib.conan_emformer_head_dim(self.h, head.encode()))
        if K <= 0:
            raise _lib.ConanError(_lib.ERR_MISSING, f"no Emformer output head '{head}'")
        y = torch.empty(x2.shape[0], K, device=self.dev)
        _lib.check(self.lib.conan_emformer_project(self.h, head.encode(), _ptr(x2), x2.shape[0], _ptr(y), _stream()))
        self._release()
        return y.reshape(*x.shape[:-1], K)

    def decoder_step(self, slots, codes, taps=False, f0=None, uv=None):
        """codes [n, T] -> mel [n, T, 80] (+ the taps dict).  f0 [n, T] (log2 Hz, the reference's norm_f0) / uv [n, T] (> 0: unvoiced;
        None: voiced): the caller's contour instead of the predictor's (conan_decoder_step_pitch; Conan.forward(f0=, uv=,
        infer=False)); the slots' pitch control (set_pitch) applies on top of it."""
        a, p = _i32(slots)
        n = len(a)
        c = self.ctx.cfg
        codes = codes.to(self.dev, torch.int32).contiguous()
        T = codes.shape[1]
        mel = torch.empty(n, T, c.num_mels, device=self.dev)
        if f0 is None and uv is not None:
            raise ValueError("decoder_step: uv without f0 (the reference ignores both unless f0 is given)")
        if f0 is not None:
            f0 = f0.to(self.dev, torch.float32).reshape(n, T).contiguous()
            uv = uv.to(self.dev, torch.float32).reshape(n, T).contiguous() if uv is not None else None
        if not taps:
            if f0 is not None:
                _lib.check(self.lib.conan_decoder_step_pitch(self.h, p, n, T, _ptr(codes), _ptr(f0), _ptr(uv), _ptr(mel), None, _stream()))
            else:
                _lib.check(self.lib.conan_decoder_step(self.h, p, n, T, _ptr(codes), _ptr(mel), None, None, None, None, _stream()))
            self._release()
            return mel
        S = (self.max_ref_frames + 3) // 4 if self.max_ref_frames >= 4 else 1
        out = {"uv_pred": torch.empty(n, T, 2, device=self.dev), "f0_denorm_pred": torch.empty(n, T, device=self.dev),
               "pitch_bins": torch.empty(n, T, dtype=torch.int32, device=self.dev),
               "decoder_inp": torch.empty(n, T, c.hidden_size, device=self.dev),
               "content_embed_proj": torch.empty(n, T, c.hidden_size, device=self.dev),
               "attn": [torch.empty(n, T, S, device=self.dev) for _ in range(2)]}
        t = _lib.DecoderTaps()
        t.uv_pred, t.f0_denorm_pred, t.pitch_bins = out["uv_pred"].data_ptr(), out["f0_denorm_pred"].data_ptr(), out["pitch_bins"].data_ptr()
        t.decoder_inp, t.content_embed_proj = out["decoder_inp"].data_ptr(), out["content_embed_proj"].data_ptr()
        t.attn[0], t.attn[1] = out["attn"][0].data_ptr(), out["attn"][1].data_ptr()
        if f0 is not None:
            _lib.check(self.lib.conan_decoder_step_pitch(self.h, p, n, T, _ptr(codes), _ptr(f0), _ptr(uv), _ptr(mel), C.byref(t), _stream()))
        else:
            _lib.check(self.lib.conan_decoder_step_taps(self.h, p, n, T, _ptr(codes), _ptr(mel), C.byref(t), _stream()))
        self._release()
        return mel, out

    def style_embed(self, slots):
        """style_embed [n, H] of the slots' current reference (Conan.encode_spk_embed, cached by set_reference)."""
        a, p = _i32(slots)
        out = torch.empty(len(a), self.ctx.cfg.hidden_size, device=self.dev)
        _lib.check(self.lib.conan_get_style(self.h, p, len(a), _ptr(out), None, _stream()))
        self._release()
        return out

    def set_style(self, slots, style):
        """Conan.forward(spk_embed=...): override the cached global style vector, style [n, H] (cuda)."""
        a, p = _i32(slots)
        style = style.to(self.dev, torch.float32).reshape(len(a), self.ctx.cfg.hidden_size).contiguous()
        _lib.check(self.lib.conan_set_style(self.h, p, len(a), _ptr(style), _stream()))
        self._release()

    def prosody_ids(self, slots):
        """VQ indices of the slots' prosody tokens: (ids int32 [n, max_tokens] (-1 padded), counts int32 [n])."""
        a, p = _i32(slots)
        S = (self.max_ref_frames + 3) // 4 if self.max_ref_frames >= 4 else 1
        ids = torch.empty(len(a), S, dtype=torch.int32, device=self.dev)
        cnt = torch.empty(len(a), dtype=torch.int32, device=self.dev)
        _lib.check(self.lib.conan_get_prosody_ids(self.h, p, len(a), _ptr(ids), _ptr(cnt), _stream()))
        self._release()
        return ids, cnt

    def hifigan_step_taps(self, slots, mel, stage_out=False):
        """hifigan_step plus the generator's intermediate tensors: (wav, pre_tanh, conv_pre_act [n,T,C0], [ups_i [n,T*rate_i,C_i]]);
        stage_out=True appends [stage_out_i [n,T*rate_i,C_i]] = leaky_relu(mean of the stage's ResBlocks)."""
        a, p = _i32(slots)
        n = len(a)
        c = self.ctx.cfg
        mel = mel.to(self.dev, torch.float32).contiguous()
        T = mel.shape[1]
        hop = self.ctx.hop
        wav = torch.empty(n, self.output_ld or T * hop, device=self.dev)
        pre = torch.empty(n, T * hop, device=self.dev)
        cpre = torch.empty(n, T, c.voc_initial_channel, device=self.dev)
        ups, outs, ch_, rate = [], [], c.voc_initial_channel, 1
        t = _lib.HifiganTaps()
        t.conv_pre_act = cpre.data_ptr()
        for i in range(c.voc_num_ups):
            ch_ //= 2
            rate *= c.voc_up_rates[i]
            ups.append(torch.empty(n, T * rate, ch_, device=self.dev))
            t.ups[i] = ups[-1].data_ptr()
            if stage_out:
                outs.append(torch.empty(n, T * rate, ch_, device=self.dev))
                t.stage_out[i] = outs[-1].data_ptr()
        _lib.check(self.lib.conan_hifigan_step_taps(self.h, p, n, T, _ptr(mel), _ptr(wav), _ptr(pre), C.byref(t), _stream()))
        self._release()
        wav = self._wav_rows(wav, a)
        return (wav, pre, cpre, ups, outs) if stage_out else (wav, pre, cpre, ups)

    def hifigan_step(self, slots, mel, want_pre_tanh=False, out=None):
        """mel: cuda float32 [n, frames, 80] -> wav [n, frames*hop]."""
        a, p = _i32(slots)
        n = len(a)
        mel = mel.to(self.dev, torch.float32).contiguous()
        T = mel.shape[1]
        hop = self.ctx.hop
        wav = out if out is not None else torch.empty(n, self.output_ld or T * hop, device=self.dev)
        pre = torch.empty(n, T * hop, device=self.dev) if want_pre_tanh else None
        _lib.check(self.lib.conan_hifigan_step(self.h, p, n, T, _ptr(mel), _ptr(wav), _ptr(pre), _stream()))
        self._release()
        wav = self._wav_rows(wav, a)
        return (wav, pre) if want_pre_tanh else wav

    def step(self, slots, mel_chunk, emit=None, codes=None, mel_out=None, wav_out=None):
        """Fused chunk step (one iteration of inference/Conan.py:95-156 for all slots)."""
        a, p = _i32(slots)
        n = len(a)
        emit = self.seg if emit is None else emit
        hop = self.ctx.hop
        if codes is None:
            codes = torch.empty(n, self.seg, dtype=torch.int32, device=self.dev)
        if mel_out is None:
            mel_out = torch.empty(n, emit, self.ctx.cfg.num_mels, device=self.dev)
        if wav_out is None:
            wav_out = torch.empty(n, self.output_ld or emit * hop, device=self.dev)
        _lib.check(self.lib.conan_step(self.h, p, n, emit, _ptr(mel_chunk), _ptr(codes), _ptr(mel_out), _ptr(wav_out), _stream()))
        self._release()
        return codes, mel_out, self._wav_rows(wav_out, a)

    def step_async(self, slots, mel_chunk, wav_out, emit=None, codes=None, mel_out=None, out_fence=None):
        """Pipelined chunk step (conan_step_async): returns at once; the front-end of the next call overlaps this
        call's vocoder.  `wav_out` (and the optional outputs) must be caller-owned tensors kept alive until join().
        out_fence: a torch.cuda.Stream whose work enqueued so far - or a recorded torch.cuda.Event that - must finish before this
        step's vocoder writes `wav_out` (conan_streams_output_fence / _event: e.g. the collective that still reads the buffer)."""
        a, p = _i32(slots)
        n = len(a)
        emit = self.seg if emit is None else int(emit)
        mel_chunk = mel_chunk.to(self.dev, torch.float32).contiguous()
        assert mel_chunk.shape == (n, self.seg + self.rc, self.ctx.cfg.emf_input_dim), mel_chunk.shape
        assert wav_out.is_cuda and wav_out.is_contiguous() and wav_out.numel() >= n * (self.output_ld or emit * self.ctx.hop)
        self._keep.append((mel_chunk, wav_out, codes, mel_out))
        if out_fence is not None:
            if isinstance(out_fence, torch.cuda.Event):      # an event recorded behind the one operation that read wav_out
                _lib.check(self.lib.conan_streams_output_fence_event(self.h, C.c_void_p(out_fence.cuda_event)))
            else:
                _lib.check(self.lib.conan_streams_output_fence(self.h, C.c_void_p(out_fence.cuda_stream)))
        _lib.check(self.lib.conan_step_async(self.h, p, n, emit, _ptr(mel_chunk), _ptr(codes), _ptr(mel_out), _ptr(wav_out), _stream()))

    def step_wav(self, slots, wav, final=False, codes=None, mel_out=None, wav_out=None, mel=None, lost=None, far=None, echo_stats=None, echo_delay_report=None):
        """Waveform-in chunk step (conan_step_wav): wav [n, samples] cuda float32, samples = seg*hop (0 .. seg*hop when final);
        slots with an input rate (set_input_rate) take seg*hop*rate/model_rate samples instead.
        -> (emit, codes [n, seg], mel [n, emit, 80], wav [n, emit*hop]); emit = 0: no chunk this call (the first call, the end of a
        drain).  mel: dict of Context.wav2mel's front-end keywords (framing 0 only).  Slots with an input format (set_input_format)
        take int16 ('s16') or uint8 ('ulaw' / 'alaw') rows; with an output rate, stride or format wav is a list of 1-D rows, each
        in its slot's dtype.  lost: the packet flags of the rows [n, packets] (conceal(), on the rows as packed for the library, in
        front of the step; a contiguous float32 wav on the device is its own packed form and is repaired in place).  far: the far
        end of the rows, shaped and typed as wav (echo_delay() for the slots with an estimator, then echo(), behind the repair and in
        front of the step); echo_stats: echo()'s stats; echo_delay_report: echo_delay()'s report."""
        return self._step_wav(slots, wav, final, codes, mel_out, wav_out, mel, False, lost, far, echo_stats, echo_delay_report)

    def step_wav_async(self, slots, wav, final=False, codes=None, mel_out=None, wav_out=None, mel=None, lost=None, far=None, echo_stats=None, echo_delay_report=None):
        """Pipelined step_wav (conan_step_wav_async): the outputs are complete after join(); same return value."""
        return self._step_wav(slots, wav, final, codes, mel_out, wav_out, mel, True, lost, far, echo_stats, echo_delay_report)

    def _wav_in_call(self, n, wav, codes, mel_out, wav_out, mel, pipelined, call):
        """What the wav-in steps share: the default output buffers and their lifetime (a pipelined call's are kept until the next
        join, a blocking call releases the kept ones) around call(mel_cfg, codes, mel_out, wav_out).  -> (codes, mel_out, wav_out)"""
        if codes is None:
            codes = torch.empty(n, self.seg, dtype=torch.int32, device=self.dev)
        if mel_out is None:
            mel_out = torch.empty(n, self.seg, self.ctx.cfg.num_mels, device=self.dev)
        if wav_out is None:
            wav_out = torch.empty(n, self.output_ld or self.seg * self.ctx.hop, device=self.dev)
        mc = mel_cfg(**(mel or {}))
        self._last_wav_n = n
        if pipelined:
            self._keep.append((wav, wav_out, codes, mel_out))
        call(mc, codes, mel_out, wav_out)
        if not pipelined:
            self._release()
        return codes, mel_out, wav_out

    def _step_wav(self, slots, wav, final, codes, mel_out, wav_out, mel, pipelined, lost=None, far=None, echo_stats=None, echo_delay_report=None):
        a, p = _i32(slots)
        n = len(a)
        hop, nm = self.ctx.hop, self.ctx.cfg.num_mels
        assert wav.dim() == 2 and wav.shape[0] == n, wav.shape
        samples = wav.shape[1]
        wav, _, _ = self._in_rows(a, wav, samples)      # (rows samples * 4 bytes apart, whatever the format)
        if lost is not None and samples:
            self.conceal(a, wav, samples, lost)
        if far is not None and samples:
            assert far.dim() == 2 and tuple(far.shape) == (n, samples), far.shape
            self._far_stages(a, wav, samples, self._in_rows(a, far, samples)[0], echo_stats, echo_delay_report)
        emit = C.c_int32(0)
        fn = self.lib.conan_step_wav_async if pipelined else self.lib.conan_step_wav
        codes, mel_out, wav_out = self._wav_in_call(n, wav, codes, mel_out, wav_out, mel, pipelined, lambda mc, c, m, w: _lib.check(
            fn(self.h, p, n, samples, int(bool(final)), _ptr(wav), C.byref(mc), _ptr(c), _ptr(m), _ptr(w), C.byref(emit), _stream())))
        e = emit.value
        if self.output_rates or self.output_ld or self.output_formats:
            w = self._wav_rows(wav_out, a, self.output_ld or e * hop) if e else [wav_out.view(-1)[:0].view(self._out_dtype(s)) for s in a]
        else:
            w = wav_out.view(-1)[:n * e * hop].view(n, e * hop)
        return e, codes, mel_out.view(-1)[:n * e * nm].view(n, e, nm), w

    def step_wav_ragged(self, slots, wav, samples, final, codes=None, mel_out=None, wav_out=None, mel=None, lost=None, far=None, echo_stats=None, echo_delay_report=None):
        """Waveform-in chunk step for slots at different positions of their utterances (conan_step_wav_ragged): slot i takes the
        first samples[i] samples of wav row i (wav [n, <= seg*hop] cuda float32, or None when every samples[i] is 0) and is stepped
        as step_wav([slot], samples[i], final[i]) alone would step it.  Rows wider than seg*hop (slots with an input rate above the
        model rate) go through conan_step_wav_ragged_ld with the row width as stride.  wav may also be a list of n 1-D rows, each in the
        dtype of its slot's input format (float32, int16, uint8): they are packed from the start of rows a whole number of 4-byte
        units apart.  -> (emit: list of n ints, codes [n, seg], mel [n, seg, 80], wav [n, seg*hop] float32 storage): row i holds
        emit[i] frames (wav_row(wav, i, slot, count) gives it in the slot's output dtype); the rest of the row is left as it was.
        lost, far, echo_stats, echo_delay_report: as step_wav's (far in wav's form: one tensor or a list of rows)."""
        return self._step_wav_ragged(slots, wav, samples, final, codes, mel_out, wav_out, mel, False, lost, far, echo_stats, echo_delay_report)

    def step_wav_ragged_async(self, slots, wav, samples, final, codes=None, mel_out=None, wav_out=None, mel=None, lost=None, far=None, echo_stats=None, echo_delay_report=None):
        """Pipelined step_wav_ragged (conan_step_wav_ragged_async): the outputs are complete after join(); same return value."""
        return self._step_wav_ragged(slots, wav, samples, final, codes, mel_out, wav_out, mel, True, lost, far, echo_stats, echo_delay_report)

    def _step_wav_ragged(self, slots, wav, samples, final, codes, mel_out, wav_out, mel, pipelined, lost=None, far=None, echo_stats=None, echo_delay_report=None):
        a, p = _i32(slots)
        n = len(a)
        L = self.seg * self.ctx.hop
        sm, sp = _i32(samples)
        fi, fp = _i32([int(bool(f)) for f in final])
        assert len(sm) == n and len(fi) == n, (n, len(sm), len(fi))
        ld = L
        if wav is not None:                           # rows are seg*hop floats apart in conan_step_wav_ragged, wider ones go through _ld
            wav, ld, _ = self._in_rows(a, wav, L)
            if lost is not None:
                self.conceal(a, wav, sm, lost)
            if far is not None:
                self._far_stages(a, wav, sm, self._in_rows(a, far, ld)[0], echo_stats, echo_delay_report)
        emit = (C.c_int32 * n)()
        if ld == L:
            fn, stride = self.lib.conan_step_wav_ragged_async if pipelined else self.lib.conan_step_wav_ragged, ()
        else:
            fn, stride = self.lib.conan_step_wav_ragged_ld_async if pipelined else self.lib.conan_step_wav_ragged_ld, (ld,)
        codes, mel_out, wav_out = self._wav_in_call(n, wav, codes, mel_out, wav_out, mel, pipelined, lambda mc, c, m, w: _lib.check(
            fn(self.h, p, n, sp, fp, _ptr(wav), *stride, C.byref(mc), _ptr(c), _ptr(m), _ptr(w), emit, _stream())))
        return list(emit), codes, mel_out, wav_out

    def wav_chunk(self, n):
        """The [n, seg+rc, 80] mel chunk the last step_wav call assembled (conan_step_wav_chunk; joins pipelined work)."""
        out = torch.empty(n, self.seg + self.rc, self.ctx.cfg.emf_input_dim, device=self.dev)
        _lib.check(self.lib.conan_step_wav_chunk(self.h, _ptr(out), _stream()))
        self._release()
        return out

    def join(self):
        """Make the current torch stream wait for every pipelined step enqueued so far."""
        _lib.check(self.lib.conan_streams_join(self.h, _stream()))
        self._release()

    def profile_mark(self):
        """One cnk::profile_mark_kernel dispatch on the current stream (marker for rocprofv3 post-processing)."""
        _lib.check(self.lib.conan_profile_mark(self.h, _stream()))

    def step_clock(self, capacity):
        """Record a completion stamp per pipelined step on the internal vocoder stream (conan_step_clock); 0 = off."""
        _lib.check(self.lib.conan_step_clock(self.h, int(capacity)))

    def step_clock_read(self, cap=4096):
        """Intervals (ms) between the completions of consecutive pipelined steps since step_clock()."""
        buf = (C.c_double * cap)()
        n = _lib.check(self.lib.conan_step_clock_read(self.h, buf, cap))
        return [buf[i] for i in range(n)]

    def step_timeline(self, capacity):
        """Record start / end events of the three stages of every following pipelined step (conan_step_timeline); 0 = off."""
        _lib.check(self.lib.conan_step_timeline(self.h, int(capacity)))

    def step_timeline_read(self, cap=1024):
        """Per recorded step [emf start, emf end, dec start, dec end, voc start, voc end] in ms since the first event."""
        buf = (C.c_double * (cap * 6))()
        n = _lib.check(self.lib.conan_step_timeline_read(self.h, buf, cap))
        return [[buf[i * 6 + e] for e in range(6)] for i in range(n)]

    def profile_begin(self):
        _lib.check(self.lib.conan_profile_begin(self.h))

    def profile_end(self):
        """-> (conv kernel ms, algorithmic conv FLOPs, conv launches) since profile_begin()."""
        ms, fl, nl = C.c_double(), C.c_double(), C.c_int64()
        _lib.check(self.lib.conan_profile_end(self.h, C.byref(ms), C.byref(fl), C.byref(nl)))
        return ms.value, fl.value, nl.value

    def profile_kernels(self):
        """Per kernel instantiation after profile_end(): list of (name, ms, flops, launches)."""
        out, i = [], 0
        while True:
            buf = C.create_string_buffer(128)
            ms, fl, nl = C.c_double(), C.c_double(), C.c_int64()
            rc = _lib.check(self.lib.conan_profile_kernel(self.h, i, buf, 128, C.byref(ms), C.byref(fl), C.byref(nl)))
            if rc == 0:
                return out
            out.append((buf.value.decode(), ms.value, fl.value, nl.value))
            i += 1

    def close(self):
        if getattr(self, "h", None):
            self.lib.conan_streams_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
