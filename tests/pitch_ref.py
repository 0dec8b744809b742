"""The per-slot pitch control of the decoder step (include/conan_hip.h, conan_pitch_cfg), restated: the law in numpy float64 and a
decoder built from oracle.conan's public pieces that applies it.  Test infrastructure only.

The law, per frame row; (d0, d1) is the uv / f0 head's output:
  source   with a caller contour v = f0_in, uv = uv_in > 0 (uv_in None: voiced), no silent-token forcing;
           otherwise v = d1, uv = (d0 > thr) or code == silent_token, thr = uv_threshold of an enabled cfg, 0 without one
  enabled  if range != 1: v = range * (v - pivot) + pivot; then v = v + shift_oct, shift_oct = float32(shift_semitones / 12)
  then     f0 = min(max(2 ** v, 50), 900) with a NaN going to 50; uv -> f0 = 0; the mel-scale bin of f0_to_coarse.
A cfg is a dict of conan_amd._lib.pitch_cfg's keywords (shift_semitones, range, pivot, uv_threshold), None for a disabled slot."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import conan as oconan

PIVOT = 7.5
MEL_MIN = 1127.0 * np.log(1.0 + 50.0 / 700.0)
MEL_MAX = 1127.0 * np.log(1.0 + 900.0 / 700.0)
BAND = 1e-3      # a row is unsafe when its mel-scale value is this close to a rounding boundary, or d0 this close to the threshold


def full_cfg(cfg):
    """Every keyword of a cfg (those not given: pitch_cfg's defaults), None for None."""
    if cfg is None:
        return None
    return dict(dict(shift_semitones=0.0, range=1.0, pivot=PIVOT, uv_threshold=0.0), **cfg)


def f32_cfg(cfg):
    """full_cfg with every value rounded to float32: what the library stores and reports."""
    return None if cfg is None else {k: float(np.float32(v)) for k, v in full_cfg(cfg).items()}


def law_v(d0, d1, codes, silent_token, cfg=None, f0=None, uv=None):
    """-> (v float64, uv bool): the contour value in front of denorm_f0 and the unvoiced flag."""
    d0, d1 = np.asarray(d0, np.float64), np.asarray(d1, np.float64)
    cfg = full_cfg(cfg)
    if f0 is not None:
        v = np.asarray(f0, np.float64).copy()
        unv = np.asarray(uv, np.float64) > 0 if uv is not None else np.zeros(v.shape, bool)
    else:
        v = d1.copy()
        thr = np.float64(np.float32(cfg["uv_threshold"])) if cfg is not None else 0.0
        unv = (d0 > thr) | (np.asarray(codes) == silent_token)
    if cfg is not None:
        rg, pv = np.float64(np.float32(cfg["range"])), np.float64(np.float32(cfg["pivot"]))
        if rg != 1.0:
            with np.errstate(invalid="ignore"):
                v = rg * (v - pv) + pv
        v = v + np.float64(np.float32(np.float64(np.float32(cfg["shift_semitones"])) / 12.0))
    return v, unv


def law(d0, d1, codes, silent_token, cfg=None, f0=None, uv=None, thr_band=True):
    """-> dict(v, uv, f0 (Hz, 0 where unvoiced), f0_voiced (Hz before the uv zeroing), mel (the mel-scale value in front of the
    rounding), bins int64, unsafe bool)."""
    v, unv = law_v(d0, d1, codes, silent_token, cfg, f0, uv)
    with np.errstate(over="ignore", invalid="ignore"):
        hz = np.exp2(v)
    hz = np.where(np.isnan(hz), 50.0, np.minimum(np.maximum(hz, 50.0), 900.0))      # fminf(fmaxf(x, 50), 900): a NaN goes to 50
    out_hz = np.where(unv, 0.0, hz)
    mel = 1127.0 * np.log(1.0 + out_hz / 700.0)
    mel = np.where(mel > 0, (mel - MEL_MIN) * 254.0 / (MEL_MAX - MEL_MIN) + 1.0, mel)
    mel = np.minimum(np.maximum(mel, 1.0), 255.0)
    bins = (mel + 0.5).astype(np.int64)
    frac = mel + 0.5 - np.floor(mel + 0.5)
    unsafe = (np.minimum(frac, 1.0 - frac) < BAND) & (mel > 1.0) & (mel < 255.0)
    if f0 is None and thr_band:
        thr = np.float64(np.float32(full_cfg(cfg)["uv_threshold"])) if cfg is not None else 0.0
        if np.isfinite(thr):
            unsafe = unsafe | (np.abs(np.asarray(d0, np.float64) - thr) < BAND)
    return dict(v=v, uv=unv, f0=out_hz, f0_voiced=hz, mel=mel, bins=bins, unsafe=unsafe)


@torch.no_grad()
def decode_frames_pitch(sd, hp, content, cache, st=None, cfg=None, f0=None, uv=None, bins_override=None):
    """oracle.conan.decode_frames with the pitch control: content [B, T] int64, cfg a dict / None for all rows or a list with one per
    batch row, f0 / uv [B, T] the caller's contour, bins_override [B, T] the bins to embed instead of the law's (the tensors that
    follow the embedding then do not depend on a row that sits on a rounding boundary).  With all four None it is decode_frames."""
    content = torch.as_tensor(content).long()
    ret = {"content": content}
    emb = F.embedding(content, sd["content_embedding.weight"])
    ce = oconan.causal_conv1d(emb.transpose(1, 2), sd["content_proj.0.conv.weight"], sd["content_proj.0.conv.bias"], 1, st, "content_proj.0.conv")
    ce = F.leaky_relu(ce, 0.01).transpose(1, 2)
    ret["content_embed_proj"] = ce
    ret["style_embed"] = style_embed = cache["style_embed"]
    pitch_inp = ce + style_embed
    out = pitch_inp.transpose(0, 1)
    mem = cache["tokens"].transpose(0, 1)
    attns = []
    for l in range(2):
        out, a = oconan.cross_atten_layer(sd, f"align.layers.{l}", out, mem, cache["key_padding_mask"])
        attns.append(a.unsqueeze(1))
    ret["attn"] = attns
    ret["pitch_embed"] = pitch_inp = pitch_inp + out.transpose(0, 1)
    ret["uv_pred"] = uv_pred = oconan.pitch_predictor(sd, "uv_predictor", pitch_inp, 5, st)
    B = content.shape[0]
    cfgs = list(cfg) if isinstance(cfg, (list, tuple)) else [cfg] * B
    d0, d1 = uv_pred[:, :, 0].numpy(), uv_pred[:, :, 1].numpy()
    rows = [law(d0[b], d1[b], content[b].numpy(), hp["silent_token"], cfgs[b], None if f0 is None else np.asarray(f0)[b],
                None if uv is None else np.asarray(uv)[b]) for b in range(B)]
    # (v in float32, then the oracle's own denorm_f0 / f0_to_coarse: with nothing set, v is d1 and this is decode_frames bit for bit)
    with np.errstate(over="ignore", invalid="ignore"):
        v32 = torch.from_numpy(np.stack([r["v"] for r in rows]).astype(np.float32))
    unv = torch.from_numpy(np.stack([r["uv"] for r in rows]))
    f0_denorm = oconan.denorm_f0(v32.clone(), unv)
    f0_denorm = torch.where(torch.isnan(f0_denorm), torch.full_like(f0_denorm, 50.0), f0_denorm)
    pitch = oconan.f0_to_coarse(f0_denorm)
    ret["fdiff"] = 0.0
    ret["f0_denorm_pred"], ret["uv"], ret["pitch_bins"] = f0_denorm, unv, pitch
    ret["unsafe"] = torch.from_numpy(np.stack([r["unsafe"] for r in rows]))
    ret["law"] = rows
    if bins_override is not None:
        pitch = torch.as_tensor(bins_override).long()
    pitch_embed = F.embedding(pitch, sd["pitch_embed.weight"], padding_idx=0)
    ret["decoder_inp"] = decoder_inp = pitch_inp + pitch_embed
    x = oconan.causal_conv_blocks(sd, "decoder", decoder_inp.transpose(1, 2), hp["dec_kernel_size"], hp["dec_dilations"], hp["layers_in_block"],
                                  hp.get("dec_post_net_kernel", 3), st)
    ret["decoder_out"] = x.transpose(1, 2)
    ret["mel_out"] = F.linear(x.transpose(1, 2), sd["mel_out.weight"], sd["mel_out.bias"])
    ret["tgt_nonpadding"] = (content != -1).float()[:, :, None]
    return ret


# ------------------------------------------------------------------------------------------------ the cases the GPU tests run
# (tests/test_pitch_cpu.py holds the reference alone to the boundary band on every one of them; tests/test_gpu_pitch.py runs them)

FRAMES = 16
SLOT_LISTS = {1: [3], 2: [4, 1], 6: [5, 0, 3, 1, 4, 2]}      # never the identity; stream-sets of 6 slots
ROW_CFGS = [None, dict(shift_semitones=5.0), dict(range=0.5, shift_semitones=-2.0), None, dict(uv_threshold=float("inf"), shift_semitones=12.0),
            dict(range=0.0, pivot=7.9)]
ALT_CFGS = [dict(shift_semitones=-7.0), None, dict(range=1.5, pivot=7.3), dict(uv_threshold=-0.05), None, dict(shift_semitones=3.0)]
# name -> (call rows, frames per step, cfg per call row)
LAW_CASES = {"n1_T4_taps": (1, 4, [ROW_CFGS[1]]), "n2_T4_xcd": (2, 4, ROW_CFGS[:2]), "n6_T4_tiles": (6, 4, ROW_CFGS), "n6_T3_ragged": (6, 3, ROW_CFGS)}
SWITCH_FRAME = 8


def inputs(n, seed=0):
    """(reference mel [n, 40, 80] float32, codes [n, FRAMES] int64) of a case; the codes hold the silent token at frame 0."""
    from conan_amd import synth
    return synth.mel(40, 21 + seed, n), synth.codes(FRAMES, n, seed=7 + seed)


def contour(n, seed=0):
    """A caller contour (f0 log2 Hz, uv 0 / 1) [n, FRAMES]: a slow wave around 2^7.4 Hz; frame 0 - the silent token - is marked voiced."""
    r = np.random.default_rng(100 + seed)
    t = np.arange(FRAMES)[None, :]
    f0 = (7.4 + 0.5 * np.sin(0.45 * t + r.uniform(0, 6, (n, 1))) + 0.05 * r.standard_normal((n, FRAMES))).astype(np.float32)
    uv = (r.uniform(size=(n, FRAMES)) < 0.25).astype(np.float32)
    uv[:, 0] = 0.0
    return f0, uv


_MODEL, _STYLE = {}, {}


def model():
    """(hparams, numpy state dict, torch state dict) of the synthetic full-size Conan the cases run on."""
    if not _MODEL:
        from conan_amd import configs, synth
        from oracle.common import to_torch_sd
        hp = configs.conan_hparams()
        sd_np = synth.conan_state_dict(hp, 0)
        _MODEL.update(hp=hp, sd_np=sd_np, sd=to_torch_sd(sd_np))
    return _MODEL["hp"], _MODEL["sd_np"], _MODEL["sd"]


def reference_rows(n, seed, segments, f0=None, uv=None, bins=None, frames=FRAMES):
    """The oracle per call row: segments = [(first frame, cfg per row), ...] (the cfg in force from that frame on), f0 / uv the
    caller's contour [n, frames], bins [n, frames] the bins to embed.  -> per row a dict of numpy arrays over the frames
    (uv_pred, pitch_bins, f0_denorm_pred, unsafe, uv, mel_out).  The style pass of a (seed, row) is computed once."""
    hp, _, sd = model()
    ref, codes = inputs(n, seed)
    out = []
    for b in range(n):
        if (n, seed, b) not in _STYLE:
            _STYLE[(n, seed, b)] = oconan.style_pass(sd, hp, torch.from_numpy(ref[b:b + 1]))
        st, parts = {}, []
        for k, (lo, cfgs) in enumerate(segments):
            hi = segments[k + 1][0] if k + 1 < len(segments) else frames
            sl = slice(lo, hi)
            parts.append(decode_frames_pitch(sd, hp, codes[b:b + 1, sl], _STYLE[(n, seed, b)], st, cfgs[b], None if f0 is None else f0[b:b + 1, sl],
                                             None if uv is None else uv[b:b + 1, sl], None if bins is None else bins[b:b + 1, sl]))
        out.append({k: np.concatenate([np.asarray(p[k][0]) for p in parts], 0) for k in ("uv_pred", "pitch_bins", "f0_denorm_pred", "unsafe", "uv", "mel_out")})
    return out
