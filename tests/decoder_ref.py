"""The decoder step (conan_decoder_step; csrc/decoder.hip, decoder_mega.hip, rowops.h, rowconv.hip) against FLOAT64 per slot: the runs
and cases the GPU sweep steps through (tests/test_gpu_decoder_f64.py), their float64 reference, the pitch-bin band, and the launch
plan of decoder.hip:116-140, 166-171 restated.  Plain helpers, no fixtures: tests/test_decoder_ref_cpu.py pins the reference to
oracle/conan.py, recomputes the yardsticks and the band and shows that the bounds reject deliberate changes.

The reference is tests.pitch_ref.decode_frames_pitch on the checkpoint widened to float64 (tests.style_ref.sd64), with per-slot state
carried over the whole run.  Every run draws its slots' voices round-robin from FOUR references (VOICE_LENS frames of synth.mel): the
neighbouring rows of a tile never share a voice, and the float64 style side runs once per voice - the GPU test puts the voices in
through the voice bank (enrol once, assign), so every slot of a voice holds bit-equal rows.  The slots of one voice that are active
in a step go through one call (their states concatenated along the batch axis); test_decoder_ref_cpu shows batched == alone.

A RUN is the inputs: max_slots, max_frames, the slot list (a non-identity permutation inside a larger max_slots), per slot a voice
and a synth.codes seed, and the steps [(slots of the step, frames)], with resets (decoder state only) in front of a step.  A CASE is
a run on a stream-set (arithmetic, flags, dev_plan, taps): several cases share a run - its reference and its yardstick.

Pitch bins.  A tapped step returns its bins: the reference embeds them, and they are asserted equal to the float64 law's on safe
rows.  A persistent launch returns none: the reference embeds the float64 law's own bins, and a slot's rows from its first unsafe
row to the end of its run (the next reset) are left out of the comparison - the decoder is causal, a wrong bin reaches every later
row.  A row is unsafe when its mel-scale value lies within BAND_MEL of a rounding boundary or its d0 within BAND_D0 of the voicing
threshold; a band is 16 x the largest difference of that quantity between the fp32 oracle and float64 over all runs (MAX_MEL_ERR,
MAX_D0_ERR, recomputed by the CPU test: the rule of style_ref.BAND).  The code seeds are drawn from SEEDS, per voice the seeds whose
first SEED_FRAMES frames hold no unsafe row in float64 (find_seeds; the CPU test asserts the 2 % cap with the reference alone).
Contour runs (decoder_step(f0=, uv=)) put every f0 at the centre of a bin: no row of theirs is unsafe."""
import contextlib
import math

import numpy as np
import torch

from tests import pitch_ref as P
from tests import style_ref as S

H = 256
VOICE_LENS = (5, 40, 64, 131)      # 2, 10, 16, 33 tokens
VOICE_SEED = 900
NV = len(VOICE_LENS)
MAX_REF = 132                      # max_ref_frames of every stream-set and of the bank: 33 tokens
CODE_FRAMES = 96                   # a slot's code stream; a run consumes a prefix
SEED_FRAMES = 96

# fp32 oracle against float64, the largest difference over all runs (measured on the CPU; test_decoder_ref_cpu recomputes them)
MAX_MEL_ERR = 1.7e-4               # of the mel-scale value in front of the rounding (values 1 .. 255)
MAX_D0_ERR = 3.0e-6                # of d0, the voicing head's output
BAND_MEL, BAND_D0 = 16 * MAX_MEL_ERR, 16 * MAX_D0_ERR
MAX_LEFT_OUT = 0.02

# per voice: code seeds (1000 * voice + k, k ascending) whose first SEED_FRAMES frames hold no unsafe row in float64 (find_seeds)
SEEDS = {
    0: [0, 1, 5, 6, 7, 8, 9, 11, 12, 13, 14, 16, 17, 18, 19, 20, 23, 24, 26, 29],
    1: [1000, 1002, 1003, 1005, 1006, 1008, 1009, 1010, 1011, 1013, 1016, 1017, 1018, 1019, 1020, 1021, 1022, 1024, 1025, 1026],
    2: [2000, 2001, 2002, 2005, 2006, 2007, 2008, 2009, 2012, 2013, 2014, 2016, 2018, 2019, 2021, 2023, 2024, 2025, 2026, 2027],
    3: [3000, 3006, 3007, 3008, 3011, 3014, 3015, 3016, 3017, 3018, 3021, 3023, 3026, 3028, 3029, 3030, 3031, 3032, 3034, 3038],
}

FUSED, SEPARATE_SMALL, FIXED_PLAN = 1, 2, 8      # conan_amd._lib.STREAMS_*
TAPS = ("content_embed_proj", "attn0", "attn1", "uv_pred", "decoder_inp", "mel_out")


def voice_mels():
    from conan_amd import synth
    return [synth.mel(L, VOICE_SEED + 10 * v, 1)[0].copy() for v, L in enumerate(VOICE_LENS)]


def slot_codes(seed):
    """A slot's code stream [CODE_FRAMES] int64 (the silent token at frames 0, 17, ...)."""
    from conan_amd import synth
    return synth.codes(CODE_FRAMES, 1, seed=seed)[0]


def centre_v(bins):
    """log2 Hz (float32) at the centre of mel-scale bin `bins` (2 .. 254): the inverse of f0_to_coarse in float64."""
    mel = (np.asarray(bins, np.float64) - 1.0) * (P.MEL_MAX - P.MEL_MIN) / 254.0 + P.MEL_MIN
    return np.log2(700.0 * (np.exp(mel / 1127.0) - 1.0)).astype(np.float32)


def slot_contour(seed):
    """(f0 log2 Hz float32, uv float32, bins int64) [CODE_FRAMES] of a contour slot: a random bin per frame, a fifth unvoiced."""
    r = np.random.default_rng(5000 + seed)
    bins = r.integers(2, 255, CODE_FRAMES)
    uv = (r.uniform(size=CODE_FRAMES) < 0.2).astype(np.float32)
    return centre_v(bins), uv, np.where(uv > 0, 1, bins)


# ------------------------------------------------------------------------------------------------------------ the runs
def _perm(n, max_slots):
    p = np.random.default_rng(1000 * max_slots + n).permutation(max_slots)[:n].tolist()
    if p == list(range(n)):
        p = p[::-1] if n > 1 else [max_slots - 1]
    return [int(x) for x in p]


def _run(n, max_slots, T, steps=3, max_frames=None, contour=False):
    slots = _perm(n, max_slots)
    assert slots != list(range(n))
    return dict(max_slots=max_slots, max_frames=max_frames or max(4, T), slots=slots, voice={s: i % NV for i, s in enumerate(slots)},
                steps=[(list(slots), T)] * steps, resets={}, contour=contour)


def _staggered(frames, max_frames):
    """n = 5: slot k joins at step k, slot 1 is reset in front of step 8; `frames`: the per-step frame counts."""
    r = _run(5, 8, 4, max_frames=max_frames)
    r["steps"] = [(r["slots"][:min(k + 1, 5)], T) for k, T in enumerate(frames)]
    r["resets"] = {8: [r["slots"][1]]}
    return r


def _cache_run():
    """14 steps over 13 distinct (active count, frames) pairs, then the first pair again: the 12-entry program cache evicts it."""
    r = _run(7, 9, 4, max_frames=4)
    pairs = [(n, 4) for n in range(1, 8)] + [(n, 2) for n in (1, 2, 3, 5, 6, 7)]
    assert len(set(pairs)) == 13
    r["steps"] = [(r["slots"][:n], T) for n, T in pairs + pairs[:1]]
    return r


def _fixed2():
    """Two slots of `fp33` - the same slots, voices and codes - alone on a set of 33."""
    r = dict(RUNS["fp33"])
    pick = [r["slots"][20], r["slots"][3]]
    r["steps"] = [(pick, 4)] * 3
    return r


RUNS = {
    # 1. geometry, T = 4
    "g5": _run(5, 8, 4), "g32": _run(32, 40, 4), "g33": _run(33, 40, 4), "g65": _run(65, 68, 4),
    # 2. frames per step
    "t1n17": _run(17, 20, 1), "t1n16": _run(16, 20, 1), "t2n9": _run(9, 12, 2), "t8n3": _run(3, 5, 8), "t16n2": _run(2, 4, 16),
    "t3n6": _run(6, 8, 3),
    "x1t2": _run(1, 3, 2), "x4t4": _run(4, 6, 4), "x1t16": _run(1, 3, 16), "x2t8": _run(2, 4, 8), "x5t3": _run(5, 7, 3),
    # 3. long and staggered: 14 steps
    "long": _staggered([4] * 14, 4), "longmix": _staggered([4, 3, 1, 2, 8, 16, 4, 3, 1, 2, 8, 16, 4, 3], 16),
    # 4. flags
    "fp33": _run(33, 33, 4), "s2": _run(2, 4, 4),
    # 5. program cache
    "cache": _cache_run(),
    # 6. contour
    "c5t4": _run(5, 8, 4, contour=True), "c2t4": _run(2, 4, 4, contour=True), "c6t3": _run(6, 8, 3, contour=True),
}
RUNS["fp2"] = _fixed2()
# 7. pipelined steps (conan_step_async): the codes are the Emformer's own, recorded from the GPU (PIPE_GOLDEN; a step is judged with the
# codes it returned, the yardstick and the cap are computed on the recorded ones)
RUNS["p5"], RUNS["p2"] = dict(_run(5, 8, 4), pipelined=True), dict(_run(2, 4, 4), pipelined=True)
PIPE_RUNS = ("p5", "p2")
PIPE_GOLDEN = "decoder_f64_pipelined_codes.npz"
PIPE_MEL_SEED = {"p5": 31, "p2": 47}


def pipe_chunks(name, seg, rc):
    """The source mel chunks [n, seg + rc, 80] float32 of a pipelined run, one per step."""
    from conan_amd import synth
    run = RUNS[name]
    mel = synth.mel(len(run["steps"]) * seg + rc, PIPE_MEL_SEED[name], len(run["slots"]))
    return [np.ascontiguousarray(mel[:, j * seg:j * seg + seg + rc]) for j in range(len(run["steps"]))]


_PIPE = {}


def pipe_codes(name):
    """The recorded codes [n, frames] int64 of a pipelined run (tests/golden)."""
    if not _PIPE:
        from tests.conftest import load_golden
        _PIPE.update(load_golden(PIPE_GOLDEN))
    return _PIPE[name].astype(np.int64)


def slot_seed(run, slot):
    """The slot's code seed: the k-th good seed of its voice, k = the slot's rank among the run's slots of that voice."""
    v = run["voice"][slot]
    k = [s for s in run["slots"] if run["voice"][s] == v].index(slot)
    return SEEDS[v][k] if len(SEEDS[v]) > k else 1000 * v + k


def run_frames(run):
    """slot -> frames the run takes from its code stream."""
    out = {s: 0 for s in run["slots"]}
    for slots, T in run["steps"]:
        for s in slots:
            out[s] += T
    assert max(out.values()) <= CODE_FRAMES
    return out


def step_inputs(run):
    """Per step: dict(slots, T, codes [n, T] int64, f0 / uv [n, T] float32 or None, first {slot: first frame of the step})."""
    at = {s: 0 for s in run["slots"]}
    if run.get("pipelined"):
        rec = pipe_codes([k for k, v in RUNS.items() if v is run][0])
        streams = {s: rec[i] for i, s in enumerate(run["slots"])}
    else:
        streams = {s: slot_codes(slot_seed(run, s)) for s in run["slots"]}
    cont = {s: slot_contour(slot_seed(run, s)) for s in run["slots"]} if run["contour"] else None
    out = []
    for slots, T in run["steps"]:
        d = dict(slots=list(slots), T=T, codes=np.stack([streams[s][at[s]:at[s] + T] for s in slots]), f0=None, uv=None, first={s: at[s] for s in slots})
        if cont:
            d["f0"] = np.stack([cont[s][0][at[s]:at[s] + T] for s in slots])
            d["uv"] = np.stack([cont[s][1][at[s]:at[s] + T] for s in slots])
            d["cbins"] = np.stack([cont[s][2][at[s]:at[s] + T] for s in slots])
        for s in slots:
            at[s] += T
        out.append(d)
    return out


# ------------------------------------------------------------------------------------------------------------ the cases
def _case(run, arith="limb", flags=0, dev_plan=None, taps=False):
    return dict(run=run, arith=arith, flags=flags, dev_plan=dev_plan, taps=taps)


CASES = {}
for _r in ("g5", "g32", "g33", "g65"):
    CASES[_r + "_limb"] = _case(_r)
for _r in ("g5", "g33", "g65"):
    CASES[_r + "_f32"] = _case(_r, "f32")
CASES["g5_taps"] = _case("g5", "f32", taps=True)
CASES["g33_taps"] = _case("g33", taps=True)
for _r in ("t1n17", "t1n16", "t2n9", "t8n3", "t16n2", "t3n6", "x1t2", "x4t4", "x1t16", "x2t8", "x5t3", "long", "longmix", "cache", "c5t4", "c2t4", "c6t3"):
    CASES[_r] = _case(_r)
CASES["longmix_f32"] = _case("longmix", "f32")
CASES["fused_n33"] = _case("g33", flags=FUSED)
CASES["fused_n5"] = _case("g5", flags=FUSED)
CASES["fixed_n33"] = _case("fp33", flags=FIXED_PLAN)
CASES["fixed_n2"] = _case("fp2", flags=FIXED_PLAN)
CASES["sepsmall_n2"] = _case("s2", flags=SEPARATE_SMALL)
for _k, _p, _r in (("gs4", "MEGA_GS=4", "g33"), ("gs16", "MEGA_GS=16", "g33"), ("grid64", "MEGA_GRID=64", "g33"), ("grid256_n65", "MEGA_GRID=256", "g65"),
                   ("narrow0", "MEGA_NARROW=0", "g33"), ("nol2", "MEGA_NOL2", "g33"), ("rowconv0", "ROWCONV=0", "g33"), ("decmega0", "DEC_MEGA=0", "g33")):
    CASES[_k] = _case(_r, dev_plan=_p)


# ------------------------------------------------------------------------------------------------------------ the plan, restated
MEGA = "cnk::decoder_mega_kernel"


def _switches(dev_plan):
    sw = dict(DEC_MEGA=1, ROWCONV=1, MEGA_GRID=0, MEGA_GS=8, MEGA_NARROW=1, MEGA_NOL2=0)
    for item in (dev_plan or "").split(";"):
        if item.strip():
            k, _, v = item.strip().partition("=")
            assert k in sw, k
            sw[k] = 1 if k == "MEGA_NOL2" else int(v or "1")
    return sw


def plan(max_slots, n, T, arith, flags=0, dev_plan=None, taps=False, num_cu=256):
    """decoder.hip:116-140, 166-171 -> dict(form: 'separate' | 'xcd' | 'tiles', kernel, njobs, groups, group_size, rowconv).
    Not restated: the residency cap of line 137-139 (groups x group_size against the workgroups the device holds; every case here is
    far below it) and the shapes rowconv does not take (a recording that meets one keeps the separate launches)."""
    sw = _switches(dev_plan)
    prows = (max_slots if flags & FIXED_PLAN else n) * T
    # (rowconv takes T >= 2 - rowconv.hip rowconv_supported -: a step of one frame per slot records no program at any slot count and runs
    # conv_mfma + LayerNorm launches; the two 2048-wide 1x1 layers (ff2) take rowlin above 16 plan rows, split-K conv_mfma up to 16)
    sep = dict(form="separate", kernel=None, njobs=0, groups=0, group_size=0, rowconv=bool(sw["ROWCONV"]) and T >= 2, rowlin=bool(sw["ROWCONV"]) and prows > 16)
    if taps or not sw["DEC_MEGA"] or not sw["ROWCONV"] or T < 2:
        return sep
    tiles_ok = (16 % T == 0 and prows > 16) or (prows <= 16 and T >= 2 and not flags & SEPARATE_SMALL)
    if not tiles_ok:
        return sep
    if prows <= 16:
        return dict(form="xcd", kernel=MEGA + "<4, 2>", njobs=1, groups=1, group_size=num_cu, rowconv=True, rowlin=True)
    grid = min(sw["MEGA_GRID"], num_cu) if sw["MEGA_GRID"] > 0 else 128
    gs = sw["MEGA_GS"]
    njobs = -(-n * T // 16)
    groups = max(1, min(njobs, grid // gs))
    padded = -(-groups // 8) * 8
    if padded * gs <= max(grid, 64) and padded <= 32:
        groups = padded
    return dict(form="tiles", kernel=MEGA + ("<4, 3>" if arith == "limb" else "<6, 3>"), njobs=njobs, groups=groups, group_size=gs, rowconv=True, rowlin=True)


def case_plans(name, num_cu=256):
    c = CASES[name]
    r = RUNS[c["run"]]
    return [plan(r["max_slots"], len(slots), T, c["arith"], c["flags"], c["dev_plan"], c["taps"], num_cu) for slots, T in r["steps"]]


def check_launches(names, p):
    """The kernels of one step (conftest.kernels_of) against its restated plan."""
    mega = {k: v for k, v in names.items() if "decoder_mega_kernel" in k}
    rc = sum(v for k, v in names.items() if "rowconv_kernel" in k)
    rl = sum(v for k, v in names.items() if "rowlin_kernel" in k)
    mfma = sum(v for k, v in names.items() if "conv_mfma_kernel" in k)
    if p["form"] == "separate":
        assert not mega, (p, sorted(names.items()))
        assert (rc > 0) == p["rowconv"] and (rl > 0) == p["rowlin"], (p, sorted(names.items()))
        assert p["rowconv"] or mfma > 0, (p, sorted(names.items()))
    else:
        assert mega == {p["kernel"]: 1}, (p, sorted(names.items()))
        assert rc == 0 and rl == 0 and mfma == 0, (p, sorted(names.items()))


# ------------------------------------------------------------------------------------------------------------ the reference
@contextlib.contextmanager
def one_thread():
    """torch on one CPU thread: the fp32 oracle's last bits - and with them the yardsticks, whose smallest tensors hold a few values per
    slot and step - depend on how the BLAS splits a product over threads; the recorded figures are the single-threaded ones."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def voices(dtype=torch.float64, ids=None, exact_positions=False):
    """The four voices' style side in `dtype` (style_ref.style_reference, computed once per voice and dtype in front of the quantiser;
    fp32 on one thread).  ids: per voice the VQ ids to embed (the GPU's, or the fp32 oracle's)."""
    with (one_thread() if dtype == torch.float32 else contextlib.nullcontext()):
        return [S.style_reference(m, dtype, ids_override=None if ids is None else ids[v], key=("decoder_ref", v), exact_positions=exact_positions)
                for v, m in enumerate(voice_mels())]


def mel_scale32(f0_denorm):
    """The fp32 oracle's mel-scale value in front of the rounding: oracle.conan.f0_to_coarse's own steps on its f0_denorm_pred."""
    f0 = torch.as_tensor(f0_denorm)
    lo, hi = 1127 * np.log(1 + 50.0 / 700), 1127 * np.log(1 + 900.0 / 700)
    m = 1127 * (1 + f0 / 700).log()
    m[m > 0] = (m[m > 0] - lo) * 254 / (hi - lo) + 1
    m[m <= 1] = 1
    m[m > 255] = 255
    return m


def unsafe_rows(mel, d0, codes, silent_token, contour):
    """A row's bin could differ in another arithmetic: the mel-scale value within BAND_MEL of a rounding boundary, or - the predictor's
    contour, no silent token - d0 within BAND_D0 of the threshold 0."""
    mel, d0 = np.asarray(mel, np.float64), np.asarray(d0, np.float64)
    frac = mel + 0.5 - np.floor(mel + 0.5)
    u = (np.minimum(frac, 1.0 - frac) < BAND_MEL) & (mel > 1.0) & (mel < 255.0)
    if not contour:
        u = u | ((np.abs(d0) < BAND_D0) & (np.asarray(codes) != silent_token))
    return u


def _merge(states, rows):
    keys = sorted({k for s in rows for k in states[s]})
    if not keys:
        return {}
    out = {}
    for k in keys:
        tmpl = next(states[s][k] for s in rows if k in states[s])
        out[k] = torch.cat([states[s].get(k, torch.zeros_like(tmpl)) for s in rows], 0)
    return out


@torch.no_grad()
def run_reference(run, vo, dtype=torch.float64, bins=None, sd=None, alone=False, hooks=None):
    """The run in `dtype` -> per step dict(slots, T, content_embed_proj / uv_pred / decoder_inp / mel_out [n, T, .], attn0 / attn1: list
    per row [T, tokens], bins [n, T] (the law's own), mel_value / d0 [n, T], unsafe [n, T]).
    vo: voices(dtype, ...); bins: per step [n, T] to embed instead of the law's; sd: the checkpoint (default: the widened / the fp32
    one); alone: every slot in a call of its own.  hooks (the CPU test's deliberate changes, fp32 side): dict of
    codes(step index, codes) -> codes, state(step index, states), style(slot, voice index) -> the voice whose style vector the slot reads, bins(step index, rows of the call, bins) -> bins."""
    hp = P.model()[0]
    sd = sd or (S.sd64() if dtype == torch.float64 else P.model()[2])
    hooks = hooks or {}
    states = {s: {} for s in run["slots"]}
    out = []
    for k, si in enumerate(step_inputs(run)):
        for s in run["resets"].get(k, []):
            states[s] = {}
        if "state" in hooks:
            hooks["state"](k, states)
        slots, T, codes = si["slots"], si["T"], si["codes"]
        if "codes" in hooks:
            codes = hooks["codes"](k, codes.copy())
        n = len(slots)
        vof = [(run["voice"][s], hooks["style"](s, run["voice"][s]) if "style" in hooks else run["voice"][s]) for s in slots]      # (tokens of, style vector of)
        groups = [[i] for i in range(n)] if alone else [[i for i in range(n) if vof[i] == v] for v in sorted(set(vof))]
        res = dict(slots=slots, T=T, codes=codes, attn0=[None] * n, attn1=[None] * n)
        emb = None if bins is None else np.asarray(bins[k])
        if emb is None and "bins" in hooks:
            emb = "hook"
        parts = {}
        for g in groups:
            (v, vs), B = vof[g[0]], len(g)
            c = vo[v]["cache"]
            cache = {"style_embed": vo[vs]["cache"]["style_embed"], "tokens": c["tokens"].expand(B, -1, -1), "key_padding_mask": c["key_padding_mask"].expand(B, -1)}
            st = _merge(states, [slots[i] for i in g])
            kw = dict(f0=None if si["f0"] is None else si["f0"][g], uv=None if si["uv"] is None else si["uv"][g])
            if isinstance(emb, str):
                own = P.decode_frames_pitch(sd, hp, codes[g], cache, {kk: vv.clone() for kk, vv in st.items()}, **kw)["pitch_bins"].numpy()
                kw["bins_override"] = hooks["bins"](k, g, own.copy())
            elif emb is not None:
                kw["bins_override"] = emb[g]
            r = P.decode_frames_pitch(sd, hp, codes[g], cache, st, **kw)
            assert r["mel_out"].dtype == dtype
            for j, i in enumerate(g):
                states[slots[i]] = {kk: vv[j:j + 1].clone() for kk, vv in st.items()}
                parts[i] = (r, j)
                for l in range(2):
                    res[f"attn{l}"][i] = r["attn"][l][j, 0]
        for t in ("content_embed_proj", "uv_pred", "decoder_inp", "mel_out", "f0_denorm_pred"):
            res[t] = torch.stack([parts[i][0][t][parts[i][1]] for i in range(n)])
        res["bins"] = np.stack([np.asarray(parts[i][0]["pitch_bins"][parts[i][1]]) for i in range(n)])
        res["mel_value"] = np.stack([parts[i][0]["law"][parts[i][1]]["mel"] for i in range(n)])
        res["d0"] = res["uv_pred"][:, :, 0].double().numpy()
        res["unsafe"] = unsafe_rows(res["mel_value"], res["d0"], codes, hp["silent_token"], run["contour"])
        out.append(res)
    return out


def keep_rows(run, ref):
    """Per step {slot: leading rows of the step that are compared}: all of them up to the slot's first unsafe row of its run (a reset
    starts a new run), none behind it.  -> (per step dicts, rows left out, rows in all)"""
    dead = {s: False for s in run["slots"]}
    out, lost, rows = [], 0, 0
    for k, r in enumerate(ref):
        for s in run["resets"].get(k, []):
            dead[s] = False
        keep = {}
        for i, s in enumerate(r["slots"]):
            u = np.flatnonzero(r["unsafe"][i])
            keep[s] = 0 if dead[s] else (int(u[0]) if len(u) else r["T"])
            dead[s] = dead[s] or len(u) > 0
            lost += r["T"] - keep[s]
            rows += r["T"]
        out.append(keep)
    return out, lost, rows


def step_tensors(res, tensors):
    """{tensor: [one array per slot of the step]} of a run_reference step, or of a GPU step brought to the same layout."""
    return {t: [res[t][i] for i in range(len(res["slots"]))] for t in tensors}


def judge_steps(got, want, bounds, tensors, keep=None):
    """style_ref.judge per step over every active slot, on the rows `keep` leaves.  got / want: per step dicts as run_reference's.
    -> (ok, {tensor: (worst rms, worst max)}, list of (step, slot) that failed)"""
    worst, bad = {t: (0.0, 0.0) for t in tensors}, []
    for k, (g, w) in enumerate(zip(got, want)):
        n = len(w["slots"])
        idx = [i for i in range(n) if keep is None or keep[k][w["slots"][i]] > 0]
        if not idx:
            continue
        cut = lambda x, i: x[i] if keep is None else x[i][:keep[k][w["slots"][i]]]
        gg = {t: [cut(g[t], i) for i in idx] for t in tensors}
        ww = {t: [torch.as_tensor(cut(w[t], i)).double() for i in idx] for t in tensors}
        j = S.judge(gg, ww, bounds)
        for t, (r, m) in S.worst(j).items():
            worst[t] = (max(worst[t][0], r), max(worst[t][1], m))
        bad += [(k, w["slots"][i]) for q, i in enumerate(idx) if not j["ok"][q]]
    return not bad, worst, bad


def oracle_run(run, hooks=None, sd32=None, patch=None):
    """The fp32 oracle against the float64 reference on a run, the way the GPU test judges a tapped run: the float64 side embeds the
    fp32 side's VQ ids and pitch bins; the fp32 side runs on one CPU thread (one_thread).  hooks / sd32 / patch (a context manager around the fp32 computation): the deliberate changes.
    -> (fp32 steps, float64 steps)"""
    v32 = voices(torch.float32)
    v64 = voices(torch.float64, ids=[v["used"] for v in v32])
    with one_thread(), (patch() if patch else contextlib.nullcontext()):
        got = run_reference(run, v32, torch.float32, sd=sd32, hooks=hooks)
    want = run_reference(run, v64, torch.float64, bins=[g["bins"] for g in got])
    return got, want


def yardstick(got, want):
    """{tensor: (worst rms, worst max)} of the fp32 oracle over every slot and step of a run."""
    inf = {t: (math.inf, math.inf) for t in TAPS}
    return judge_steps(got, want, inf, TAPS)[1]


def find_seeds(count=20, candidates=64):
    """Per voice the first `count` seeds 1000 * voice + k whose SEED_FRAMES frames hold no unsafe row in float64."""
    out = {}
    v64 = voices(torch.float64)
    for v in range(NV):
        slots = list(range(candidates))
        run = dict(max_slots=candidates, max_frames=SEED_FRAMES, slots=slots, voice={s: v for s in slots}, steps=[(slots, SEED_FRAMES)], resets={}, contour=False)
        saved, SEEDS[v] = SEEDS[v], []      # (slot_seed then falls back to 1000 * voice + k)
        try:
            ref = run_reference(run, v64)[0]
        finally:
            SEEDS[v] = saved
        out[v] = [1000 * v + k for k in range(candidates) if not ref["unsafe"][k].any()][:count]
    return out
