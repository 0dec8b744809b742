"""Float64 reference of the style pass (conan_set_reference / conan_voices_enroll; conan_streams::style_pass in csrc/decoder.hip) and of
the prosody attention that reads its K/V rows, the cases the GPU sweep runs (tests/test_gpu_style_f64.py), the launch plan of those
cases restated, and the error statistics the sweep asserts (judge).  Plain helpers, no fixtures: tests/test_style_ref_cpu.py pins the
reference to oracle/conan.py, recomputes the yardsticks and shows that the bounds reject deliberate changes.

The arithmetic is oracle.conan.style_pass - dtype-generic - on the checkpoint widened to float64 with the reference mel widened to
float64: library and reference multiply the same bits.  A slot's reference runs ALONE on ref[:ref_len] (the library's per-slot
meaning: a slot's result does not depend on what shares its pass; the last group of four frames may be partial).  On top of the
oracle: the K/V rows of both aligner layers, formed from `tokens` with the in_proj rows oracle.conan.cross_atten_layer hands to
F.multi_head_attention_forward and laid out [S][K | V] as the library caches them; per token the margin between the two smallest
float64 VQ distances; `ids_override`, which embeds the ids the code under test chose, so that everything behind the quantiser is
compared even where a token sits on a decision boundary; the decoder step in float64 (tests.pitch_ref.decode_frames_pitch with
the widened checkpoint and bins_override); and position_table, the sinusoidal position table with its fp32 steps spelled out, which
the GPU test embeds instead of torch's fp32 table (whose last bits differ between machines - see there)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import conan as oconan
from tests import pitch_ref as P

STEP_FRAMES, STEPS = 4, 2          # the decoder steps behind the pass: two steps of four frames
NHEAD = 2

# ------------------------------------------------------------------------------------------------------------ the cases
# name -> max_ref_frames, max_slots, the calls (slot list - never the identity -, reference lengths), and what the case is there for.
# Every input is synth.mel(length, seed of the case + 10 * row): its own seed per slot.
_PERM8 = [5, 2, 7, 0, 3, 6, 1, 4]
C64, C32_64, C32 = "cnk::conv_mfma_kernel<64, 64, 2, 2, 1, 32>", "cnk::conv_mfma_kernel<32, 64, 1, 2, 2, 64>", "cnk::conv_mfma_kernel<32, 32, 1, 1, 4, 128>"
CONV_CFGS = ((C64, 64, 64), (C32_64, 32, 64), (C32, 32, 32))      # streams.hip:29 `wide`; conv_mfma.hip:782-793

CASES = {
    # references shorter than half the 31-tap kernel, 1 .. 8 tokens: the 5-tap prosody convs over one or two rows
    "short": dict(max_ref=32, max_slots=8, slots=_PERM8, lens=[1, 2, 3, 4, 5, 7, 8, 31], seed=100, reach={C32}),
    # 1992 rows: the 512-column layers in 64 x 64 tiles, the rest still in 32 x 32
    "edge_1992": dict(max_ref=256, max_slots=8, slots=_PERM8, lens=[249, 1, 17, 33, 64, 131, 150, 248], seed=200, reach={C64, C32}),
    # 2104 rows: 264 tiles of the 512-column layers on 256 CUs - the split-K tail -, the 256-column layers in 32 x 64
    "tail_2104": dict(max_ref=264, max_slots=8, slots=_PERM8, lens=[263, 263, 262, 261, 260, 257, 256, 255], seed=300, reach={C64, C32_64, C32}),
    # one slot, 250 tokens: the 512-column layers in 32 x 64
    "one_997": dict(max_ref=1000, max_slots=2, slots=[1], lens=[997], seed=400, reach={C32_64, C32}),
    # 4040 rows: the 256-column layers in 64 x 64, the 160-column layers in 32 x 64
    "wide_4040": dict(max_ref=512, max_slots=8, slots=_PERM8, lens=[505, 505, 504, 503, 502, 501, 500, 499], seed=500, reach={C64, C32_64, C32}),
    # tokens 512, 1, 16, 17, 63, 64, 65, 127 with last groups of 1, 1, 1, 2, 3, 4, 1, 1 frames; every frame-rate layer and the wide
    # token-rate layers in 64 x 64 (the 160- and 80-column token-rate layers, 4096 rows, in 32 x 64)
    "long": dict(max_ref=2048, max_slots=8, slots=_PERM8, lens=[2045, 1, 61, 66, 251, 256, 257, 505], seed=600, reach={C64, C32_64}),
    # 11 slots of 12 in one call: a pass of eight with lengths up to 64, then a pass of three on the workspace the longer pass used
    "passes": dict(max_ref=64, max_slots=12, slots=[9, 4, 11, 0, 7, 2, 10, 5, 8, 1, 6], lens=[64, 33, 12, 64, 50, 7, 41, 63, 5, 9, 2], seed=700, reach={C32}),
    # frames that are zero inside a reference (all bins: the conv blocks' masks and the style mean's count; the first bin alone: the
    # WaveNet's mask), and a reference given with ref_len 150 whose frames from 131 on are zero
    "zeros": dict(max_ref=264, max_slots=4, slots=[3, 1], lens=[263, 150], seed=800, reach={C32}),
}
LONG_VOICE = 2048                  # `long` also enrols a voice of exactly max_ref_frames, alone: 512 tokens, sp[h][512] exactly full
SP_BATCH = 8                       # streams.hip:853: slots per pass


def case_mels(name):
    """The case's references: a list of float32 arrays [length, 80], one per call row."""
    from conan_amd import synth
    c = CASES[name]
    mels = [synth.mel(L, c["seed"] + 10 * i, 1)[0].copy() for i, L in enumerate(c["lens"])]
    if name == "zeros":
        mels[0][[5, 6, 7, 8, 100, 262]] = 0.0
        mels[0][40:44, 0] = 0.0
        mels[1][131:] = 0.0
    return mels


def long_voice_mel():
    from conan_amd import synth
    return synth.mel(LONG_VOICE, CASES["long"]["seed"] + 99, 1)[0].copy()


def case_codes(name):
    """Content codes [rows, STEPS * STEP_FRAMES] int64 of the decoder steps that follow the case's pass."""
    from conan_amd import synth
    c = CASES[name]
    return synth.codes(STEPS * STEP_FRAMES, len(c["lens"]), seed=c["seed"] + 7)


def padded(mels, width=None):
    """The call's input: [rows, width, 80] float32 with every reference at the front of its row, and the lengths."""
    width = width or max(m.shape[0] for m in mels)
    out = np.zeros((len(mels), width, 80), np.float32)
    for i, m in enumerate(mels):
        out[i, :m.shape[0]] = m
    return out, [m.shape[0] for m in mels]


# ------------------------------------------------------------------------------------------------------------ the plan, restated
def _ceil(a, b):
    return -(-a // b)


def pick_cfg(rows, cols, cus):
    """streams.hip:24-51 pick_cfg for one problem of more than 32 columns: the first of 64 x 64, 32 x 64, 32 x 32 tiles with a tile
    for every CU, else the 32 x 32 tiles.  (conv_tall / conv_limb never take a style-pass layer: its tensors are not rings.)"""
    assert cols > 32
    for name, tm, tn in CONV_CFGS:
        if _ceil(rows, tm) * _ceil(cols, tn) >= cus:
            return name
    return CONV_CFGS[-1][0]


def tail_split(rows, cols, ktaps, cin, cus):
    """streams.hip:113-129: K slices of the tail tiles of a 64 x 64 launch whose tile count is above and no multiple of the CU count
    (1: no split).  The slab (8 Mi floats) and the tile counters (4096) of api.hip:264."""
    if pick_cfg(rows, cols, cus) != C64:
        return 1
    tiles = _ceil(rows, 64) * _ceil(cols, 64)
    nks = ktaps * _ceil(_ceil(cin, 32) * 32, 32)
    rem = tiles % cus
    if not (tiles > cus and rem > 0 and tiles <= 4096):
        return 1
    S = min(8, cus // rem, nks // 8)
    while S > 1 and rem * S * 64 * 64 > (8 << 20):
        S -= 1
    return S if S >= 2 else 1


def pass_layers(n, T, hp=None, nvq=None):
    """(name, rows, columns, taps, input channels) of every conan_streams::conv launch of one pass of n slots whose longest reference
    has T frames (decoder.hip style_pass), in launch order."""
    hp = hp or P.model()[0]
    nvq = nvq or int(P.model()[2]["prosody_extractor.vqvae.embedding"].shape[0])
    H, NM, S = hp["hidden_size"], 80, _ceil(T, 4)
    out = [("global_conv_in", n * T, H, 1, NM)]
    for _ in range(10):
        out += [("genc.c1", n * T, 2 * H, 31, H), ("genc.c2", n * T, H, 1, 2 * H)]
    out.append(("genc.post", n * T, H, 3, H))
    for i in range(4):
        out += [("wn.in", n * T, 2 * NM, 3, NM), ("wn.rs", n * T, 2 * NM if i < 3 else NM, 1, NM)]
    for _ in range(10):
        out += [("penc.c1", n * S, 2 * NM, 5, NM), ("penc.c2", n * S, NM, 1, 2 * NM)]
    out += [("penc.post", n * S, H, 3, NM), ("vq.dot", n * S, nvq, 1, H), ("l1", n * S, H, 1, 2 * H), ("kv", n * S, 2 * H, 1, H), ("kv", n * S, 2 * H, 1, H)]
    return out


def passes_of(lens, batch=SP_BATCH):
    """(slots in the pass, longest reference) per pass of one call."""
    return [(len(lens[i:i + batch]), max(lens[i:i + batch])) for i in range(0, len(lens), batch)]


def call_kernels(lens, cus, batch=SP_BATCH):
    """Kernel name -> launches of one set_reference call (batch = 1: an enrolment, one voice per pass)."""
    out = {}
    for n, T in passes_of(lens, batch):
        for _, rows, cols, _, _ in pass_layers(n, T):
            k = pick_cfg(rows, cols, cus)
            out[k] = out.get(k, 0) + 1
    return out


def layer_cfgs(lens, cus, batch=SP_BATCH):
    """{(layer name, columns): set of configurations} over the passes of a call."""
    out = {}
    for n, T in passes_of(lens, batch):
        for name, rows, cols, _, _ in pass_layers(n, T):
            out.setdefault((name, cols), set()).add(pick_cfg(rows, cols, cus))
    return out


# ------------------------------------------------------------------------------------------------------------ the reference
_SD64 = {}


def sd64():
    if not _SD64:
        _SD64.update({k: v.double() if v.is_floating_point() else v for k, v in P.model()[2].items()})
    return _SD64


def kv_rows(sd, tokens):
    """The K/V rows both aligner layers cache: per layer [S, 2H] = [K | V], K = tokens W_k^T + b_k and V alike with rows H .. 2H and
    2H .. 3H of in_proj (what F.multi_head_attention_forward forms from `mem` in oracle.conan.cross_atten_layer)."""
    H = tokens.shape[-1]
    out = []
    for l in range(2):
        w, b = sd[f"align.layers.{l}.multihead_attn.in_proj_weight"], sd[f"align.layers.{l}.multihead_attn.in_proj_bias"]
        out.append(F.linear(tokens, w[H:], b[H:]))
    return out


def position_table(n, dim):
    """SinusoidalPositionalEmbedding.get_embedding (oracle.conan.sinusoid_table) with its fp32 steps - the step of the exponent, the
    frequencies, the angles position x frequency - rounded to fp32 one by one in numpy, and the sine and cosine of those angles in
    float64.  -> float64 [n, dim].
    Why the GPU test does not take the oracle's table: torch forms it in fp32 with the CPU's vector exp, whose last bit differs
    between machines, and a frequency that is half an ulp off moves the angle of position p by p half-ulps. Measured on two
    machines: this table against torch's, max |d| over 2001 rows 7.6e-6 on one and 1.2e-4 on the other; the K/V rows of a 512-token
    voice - the same GPU bits - 2.5e-7 rms from a float64 reference built with the first machine's table and 1.46e-6 from one built
    with the second's, growing linearly with the token count: half of the bound from the reference alone. The library builds its
    table on the host by the same fp32 steps with libm's expf / sinf / cosf (csrc/ctx.hip); its formula compiled alone agrees with
    this table to 3.3e-8 over all 2002 rows, which is sinf's own rounding, and against this table the GPU's K/V rows sit at 2.4e-7
    at every length. tests/test_style_ref_cpu.py holds this table to torch's within two ulps of the angle."""
    half = dim // 2
    step = np.float32(math.log(10000.0) / (half - 1))
    arg = np.arange(half, dtype=np.float32) * -step
    freq = np.exp(arg.astype(np.float64)).astype(np.float32)             # the correctly rounded fp32 exponential
    angle = np.arange(n, dtype=np.float32)[:, None] * freq[None, :]
    assert arg.dtype == angle.dtype == np.float32
    angle = angle.astype(np.float64)
    t = np.concatenate([np.sin(angle), np.cos(angle)], 1)
    t[0] = 0.0
    return torch.from_numpy(t)


@torch.no_grad()
def behind_quantiser(sd, hp, enc, ids, exact_positions=False):
    """oracle.conan.style_pass from the VQ indices on (straight-through value, positions, l1), for enc [1, S, H], ids [1, S].
    exact_positions: position_table instead of the oracle's fp32 table (float64 only)."""
    H = hp["hidden_size"]
    q = F.embedding(ids, sd["prosody_extractor.vqvae.embedding"]).view_as(enc)
    z = enc + (q - enc)
    pos = oconan.make_positions(z[:, :, 0], 0)
    n = max(2000 + 1, int(pos.max()) + 1)
    assert not exact_positions or enc.dtype == torch.float64
    table = position_table(n, H) if exact_positions else oconan.sinusoid_table(n, H, 0)
    positions = table.index_select(0, pos.view(-1)).view(1, pos.shape[1], -1)
    tokens = F.linear(torch.cat([z, positions], dim=-1), sd["l1.weight"], sd["l1.bias"])
    return tokens, tokens[:, :, 0].eq(0)


_PASS = {}


@torch.no_grad()
def style_reference(mel, dtype=torch.float64, ids_override=None, key=None, exact_positions=False):
    """One slot's reference alone: mel [length, 80] float32 -> dict of style [H], ids [S] (the arg-min of the distances in `dtype`),
    top2 [S, 2] / margin [S] (the two nearest codes and the gap between their distances), dist [S, M], used [S] (the ids embedded:
    ids_override or ids), tokens [S, H], mask [S] (1: a key the attention reads), kv [2][S, 2H], cache (decode_frames' style cache).
    key: anything hashable that names the mel - the pass in front of the quantiser is then computed once per (key, dtype).
    exact_positions: see position_table (the GPU test's choice; the yardsticks - fp32 oracle against float64 - keep the oracle's table
    on both sides, where it cancels)."""
    hp = P.model()[0]
    sd = sd64() if dtype == torch.float64 else P.model()[2]
    if key is None or (key, dtype) not in _PASS:
        c = oconan.style_pass(sd, hp, torch.from_numpy(np.ascontiguousarray(mel))[None].to(dtype))
        assert c["style_embed"].dtype == dtype and c["tokens"].dtype == dtype
        if key is not None:
            _PASS[(key, dtype)] = c
    else:
        c = _PASS[(key, dtype)]
    S = c["enc"].shape[1]
    dist = c["vq_dist"].reshape(S, -1)
    top = dist.topk(2, -1, largest=False)
    ids = top.indices[:, 0]
    used = ids if ids_override is None else torch.as_tensor(np.asarray(ids_override)).long().reshape(S)
    tokens, kpm = behind_quantiser(sd, hp, c["enc"], used[None], exact_positions)
    return dict(style=c["style_embed"][0, 0], ids=ids, oracle_ids=c["vq_ids"][0], top2=top.indices, margin=top.values[:, 1] - top.values[:, 0], dist=dist,
                used=used, tokens=tokens[0], mask=(~kpm[0]).to(dtype), kv=kv_rows(sd, tokens[0]), oracle_tokens=c["tokens"][0],
                cache={"style_embed": c["style_embed"], "tokens": tokens, "key_padding_mask": kpm})


@torch.no_grad()
def decode_reference(ref, codes, dtype=torch.float64, bins_override=None):
    """STEPS decoder steps of STEP_FRAMES frames behind a slot's pass: codes [frames] int64 -> dict of attn [2][frames, S], mel
    [frames, 80], bins [frames] (the law's own), unsafe [frames]."""
    hp = P.model()[0]
    sd = sd64() if dtype == torch.float64 else P.model()[2]
    st, parts = {}, []
    codes = torch.as_tensor(np.asarray(codes)).long().reshape(1, -1)
    for p in range(0, codes.shape[1], STEP_FRAMES):
        q = slice(p, p + STEP_FRAMES)
        parts.append(P.decode_frames_pitch(sd, hp, codes[:, q], ref["cache"], st, bins_override=None if bins_override is None else np.asarray(bins_override).reshape(1, -1)[:, q]))
    assert parts[0]["mel_out"].dtype == dtype
    return dict(attn=[torch.cat([p["attn"][l][0, 0] for p in parts], 0) for l in range(2)], mel=torch.cat([p["mel_out"][0] for p in parts], 0),
                bins=torch.cat([p["pitch_bins"][0] for p in parts], 0), unsafe=torch.cat([p["unsafe"][0] for p in parts], 0))


# ------------------------------------------------------------------------------------------------------------ judging
TENSORS = ("style", "kv0", "kv1", "attn0", "attn1", "mel_out")


def errors(got, want):
    """(relative rms error |e|_2 / |want|_2, largest |e| over the rms of want, whether `got` is finite throughout) of one slot's
    tensor against float64."""
    want = torch.as_tensor(want)
    assert want.dtype == torch.float64, want.dtype
    got = torch.as_tensor(np.asarray(got)) if not torch.is_tensor(got) else got
    assert tuple(got.shape) == tuple(want.shape), (got.shape, want.shape)
    e = got.double().cpu() - want
    rms = want.pow(2).mean().sqrt()
    return float(e.pow(2).sum().sqrt() / want.pow(2).sum().sqrt()), float(e.abs().max() / rms), bool(torch.isfinite(got).all())


def judge(got, want, bounds):
    """Per slot and tensor.  got / want: {tensor: [one array per slot]} (want float64), bounds: {tensor: (rms bound, max bound)}.
    -> {"rms": {tensor: [per slot]}, "max": {tensor: [per slot]}, "ok": [per slot]}: a slot is ok when every tensor given for it is
    finite and within both of its bounds."""
    names = [t for t in want]
    n = len(want[names[0]])
    res = {"rms": {t: [] for t in names}, "max": {t: [] for t in names}, "ok": [True] * n}
    for t in names:
        assert len(got[t]) == len(want[t]) == n, t
        for i in range(n):
            r, m, fin = errors(got[t][i], want[t][i])
            res["rms"][t].append(r)
            res["max"][t].append(m)
            res["ok"][i] = res["ok"][i] and fin and r <= bounds[t][0] and m <= bounds[t][1]
    return res


def worst(j):
    """{tensor: (largest rms, largest max)} over the slots of a judge() result."""
    return {t: (max(j["rms"][t]), max(j["max"][t])) for t in j["rms"]}


def check_ids(got_ids, ref, band):
    """The ids a slot's pass chose against its float64 reference: exact on safe tokens (margin >= band); on unsafe tokens one of the
    two nearest codes in float64.  -> number of unsafe tokens."""
    got = torch.as_tensor(np.asarray(got_ids)).long().reshape(-1)
    assert got.shape == ref["ids"].shape, (got.shape, ref["ids"].shape)
    safe = ref["margin"] >= band
    assert bool((got[safe] == ref["ids"][safe]).all()), ("a safe token's id differs", got[safe].tolist(), ref["ids"][safe].tolist())
    near = (got[~safe] == ref["top2"][~safe][:, 0]) | (got[~safe] == ref["top2"][~safe][:, 1])
    assert bool(near.all()), "an unsafe token's id is not one of the two nearest"
    return int((~safe).sum())


def case_references(name):
    """The case's mels (for `long` with the 2048-frame voice appended) and their codes, row by row."""
    mels, codes = case_mels(name), case_codes(name)
    if name == "long":
        mels, codes = mels + [long_voice_mel()], np.concatenate([codes, codes[:1]], 0)
    return mels, codes


def oracle_run(name, mutate=None, tamper=None):
    """The fp32 oracle (oracle.conan.style_pass, the K/V rows, decode_frames) against the float64 reference over a case's references,
    on the CPU, the way the GPU test judges the library: the float64 side embeds the fp32 side's ids and bins.  mutate: a context
    manager entered around the ORACLE's computation only; tamper(row, result): changes the oracle's result of a slot in place
    (tests/test_style_ref_cpu.py's deliberate changes).
    -> (got, want: {tensor: [per row]}, ids_ok [per row]: check_ids passed, refs: the float64 references with their own ids)"""
    import contextlib
    mels, codes = case_references(name)
    got, want, ids_ok, refs = {t: [] for t in TENSORS}, {t: [] for t in TENSORS}, [], []
    for i, m in enumerate(mels):
        own = style_reference(m, torch.float64, key=(name, i))
        with (mutate() if mutate else contextlib.nullcontext()):
            g = style_reference(m, torch.float32, key=None if mutate else (name, i))
            if tamper:
                tamper(i, g)
            dg = decode_reference(g, codes[i], torch.float32)
        try:
            check_ids(g["used"], own, BAND)
            ids_ok.append(True)
        except AssertionError:
            ids_ok.append(False)
        w = style_reference(m, torch.float64, ids_override=g["used"], key=(name, i))
        dw = decode_reference(w, codes[i], torch.float64, bins_override=dg["bins"])
        for t, a, b in (("style", g["style"], w["style"]), ("kv0", g["kv"][0], w["kv"][0]), ("kv1", g["kv"][1], w["kv"][1]),
                        ("attn0", dg["attn"][0], dw["attn"][0]), ("attn1", dg["attn"][1], dw["attn"][1]), ("mel_out", dg["mel"], dw["mel"])):
            got[t].append(a)
            want[t].append(b)
        refs.append(own)
    return got, want, ids_ok, refs


# A token is unsafe when the gap between its two smallest float64 VQ distances is below BAND = 16 x the largest difference between an
# fp32-oracle distance and the float64 distance over all cases (measured: 1.59e-4 on distances around 280; tests/test_style_ref_cpu.py
# recomputes it).  At most MAX_UNSAFE of a case's tokens may be unsafe.
MAX_DIST_ERR = 1.6e-4
BAND = 16 * MAX_DIST_ERR
MAX_UNSAFE = 0.01


def tokens_of(length):
    return _ceil(length, 4)
