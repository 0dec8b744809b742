"""The style pass (conan_set_reference, conan_voices_enroll; conan_streams::style_pass) and the prosody attention that reads what it
caches against FLOAT64, per slot, at the launch shapes a real reference reaches: up to 8 references of 5 s in one pass (2000 rows and
more: every tile configuration of conan_streams::conv the pass can take - 64 x 64, 32 x 64, 32 x 32 -, the split-K tail), one
reference of 997 frames, 2045 and 2048 frames (512 tokens, the documented limit: sp[h][XA_MAX_S] of the attention and
spos[XA_MAX_S] of vq_pos_kernel exactly full), references shorter than half the 31-tap kernel, two passes of one call on one
workspace, zero frames inside a reference.

A Conan-only context with the full synthetic checkpoint; one stream-set per case (tests/style_ref.py holds the cases, the float64
reference and the judge).  Per case: (1) the batched pass - its launches against the plan restated from the device's CU count, the
style vector, the VQ ids and the token counts; (2) the K/V rows, the key mask and the rest of an enrolled voice, cut from an exported
bank row; (3) the attention that reads the rows - two decoder steps with taps (xattn_tile), then the persistent launch and the
DEC_MEGA=0 set; (4) a slot that had a longer voice.

Bounds.  Per slot and tensor the relative rms error and the largest error over the slot's rms, against
    rms bound = RMS_FACTOR (8) x the fp32 ORACLE's rms,   max bound = MAX_FACTOR (16) x the fp32 oracle's max
where the oracle's figures (ORACLE_FP32 below; tests/test_style_ref_cpu.py recomputes them) are oracle.conan.style_pass / decode_frames
in fp32 on the CPU against the float64 reference on the case's own inputs, the worst slot.  The factors and their reasons are the
project's own (tests/test_gpu_vocoder_f64.py): K-ordered MFMA accumulation differs from torch's blocked sums and the layers chain
through LayerNorm; 8 x 4e-7 still sits well below a product formed from two bf16 limbs (2^-16 = 1.5e-5).  No bound comes from the
kernels under test.  VQ ids are exact on safe tokens (float64 margin >= style_ref.BAND) and one of the two nearest codes in float64
on the others; everything behind the quantiser is compared with the reference that embeds the GPU's own ids (and, in the decoder
step, the GPU's own pitch bins) and style_ref.position_table - the position table by the fp32 steps the library and the oracle both
follow, sine and cosine in float64 - instead of the table torch's fp32 exp gives on the machine the test runs on.

The key mask is read where it can be read: inside an exported bank row, which holds a voice's tokens and nothing past them (every
entry +0.0).  The mask entries of a stream-set's slot past its token count are not visible through the API; what they and the K/V
rows past the count would do is: `attn` past a slot's tokens is asserted to be exactly +0.0, and the slot that had a longer voice is
compared bit for bit with a fresh one.

Not covered: the -inf branch of kmask_kernel.  tokens[:, :, 0] == 0 does not occur for any input that goes through the model (l1 has
a bias), so every key mask entry of a token is 0; nothing here fakes it."""
import numpy as np
import pytest
import torch

from tests import pitch_ref as P
from tests import style_ref as S
from tests.conftest import kernels_of
from tests.test_gpu_vocoder_f64 import MAX_FACTOR, RMS_FACTOR

pytestmark = pytest.mark.gpu

# case: {tensor: (oracle fp32 rms, oracle fp32 max)} as measured, the worst slot (for `long` including the 2048-frame voice)
ORACLE_FP32 = {
    "short": {"style": (2.672e-07, 1.054e-06), "kv0": (1.680e-07, 6.855e-07), "kv1": (1.753e-07, 7.533e-07),
              "attn0": (1.222e-07, 2.932e-07), "attn1": (1.238e-07, 3.457e-07), "mel_out": (5.940e-07, 2.847e-06)},
    "edge_1992": {"style": (1.703e-07, 4.951e-07), "kv0": (3.848e-07, 3.631e-06), "kv1": (3.999e-07, 2.700e-06),
                  "attn0": (3.012e-07, 1.255e-06), "attn1": (2.310e-07, 1.015e-06), "mel_out": (6.050e-07, 5.240e-06)},
    "tail_2104": {"style": (6.361e-08, 3.851e-07), "kv0": (3.857e-07, 3.348e-06), "kv1": (4.033e-07, 2.775e-06),
                  "attn0": (2.530e-07, 1.645e-06), "attn1": (2.334e-07, 1.621e-06), "mel_out": (5.656e-07, 2.946e-06)},
    "one_997": {"style": (5.951e-08, 3.181e-07), "kv0": (3.893e-07, 2.881e-06), "kv1": (4.059e-07, 2.884e-06),
                "attn0": (2.421e-07, 1.289e-06), "attn1": (2.121e-07, 1.198e-06), "mel_out": (5.224e-07, 1.992e-06)},
    "wide_4040": {"style": (6.682e-08, 4.045e-07), "kv0": (3.890e-07, 3.497e-06), "kv1": (4.071e-07, 3.391e-06),
                  "attn0": (2.922e-07, 2.133e-06), "attn1": (2.447e-07, 1.332e-06), "mel_out": (5.775e-07, 2.696e-06)},
    "long": {"style": (1.694e-07, 5.650e-07), "kv0": (3.937e-07, 3.502e-06), "kv1": (4.073e-07, 3.393e-06),
             "attn0": (2.538e-07, 2.726e-06), "attn1": (2.300e-07, 2.656e-06), "mel_out": (6.011e-07, 2.766e-06)},
    "passes": {"style": (3.122e-07, 1.008e-06), "kv0": (3.793e-07, 2.209e-06), "kv1": (3.981e-07, 2.267e-06),
               "attn0": (2.254e-07, 7.499e-07), "attn1": (2.071e-07, 6.936e-07), "mel_out": (5.780e-07, 2.637e-06)},
    "zeros": {"style": (6.573e-08, 3.690e-07), "kv0": (3.844e-07, 2.502e-06), "kv1": (4.035e-07, 2.605e-06),
              "attn0": (2.368e-07, 1.000e-06), "attn1": (2.147e-07, 8.558e-07), "mel_out": (5.218e-07, 2.156e-06)},
}
BOUNDS = {c: {t: (RMS_FACTOR * r, MAX_FACTOR * m) for t, (r, m) in v.items()} for c, v in ORACLE_FP32.items()}
MEGA_TOL = dict(atol=2e-5, rtol=1e-5)      # a persistent launch against the separate launches of the same step (tests/test_gpu_pitch.py)
H = 256


# ------------------------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def ctx():
    from conan_amd.runtime import Context
    hp, sd_np, _ = P.model()
    assert hp["hidden_size"] == H
    c = Context(hp, None, 0, emformer=False, conan=True, hifigan=False)
    c.load_state_dict("conan", sd_np)
    c.finalize()
    yield c
    c.close()


@pytest.fixture(scope="module")
def sets(ctx):
    """case -> its one stream-set, made on first use with every slot of the case reset, closed at the end of the module."""
    made = {}

    def get(name):
        if name not in made:
            c = S.CASES[name]
            made[name] = ctx.streams(c["max_slots"], S.STEP_FRAMES, c["max_ref"])
            made[name].reset(c["slots"])
        return made[name]
    yield get
    for st in made.values():
        st.close()


_REFS = {}


def _refs(name):
    """The case's inputs and float64 references (each slot alone, its own ids), computed once."""
    if name not in _REFS:
        mels, codes = S.case_mels(name), S.case_codes(name)
        _REFS[name] = dict(mels=mels, codes=codes, own=[S.style_reference(m, key=(name, i)) for i, m in enumerate(mels)])
    return _REFS[name]


def _num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _pass(st, name):
    """The case's one set_reference call -> the kernels it launched."""
    c, r = S.CASES[name], _refs(name)
    assert c["slots"] != list(range(len(c["slots"])))
    ref, lens = S.padded(r["mels"])
    ref = torch.from_numpy(ref).cuda()
    return kernels_of(st, lambda: st.set_reference(c["slots"], ref, lens))


def _assert_plan(names, name, lens, batch=S.SP_BATCH):
    """The launches are the restated plan's; on 256 CUs, the configurations the case is there to reach.
    The split-K tail of `tail_2104` is asserted through the restated rule alone (style_ref.tail_split): a launch carries the same kernel
    name with and without the split and the profile records hold no split factor, so a stream-set that did not split (the developer
    switch NO_TAILSPLIT of a developer build) would not be noticed here - what the test holds is that the numbers of that launch, split or not, meet the
    bounds."""
    cus = _num_cu()
    assert names == S.call_kernels(lens, cus, batch), (name, sorted(names.items()), sorted(S.call_kernels(lens, cus, batch).items()))
    if cus == 256 and batch == S.SP_BATCH:
        assert S.CASES[name]["reach"] == set(names), (name, sorted(names))
        lc = S.layer_cfgs(lens, cus)
        n, T = S.passes_of(lens)[0]
        if name == "edge_1992":
            assert lc[("genc.c1", 512)] == {S.C64} and lc[("genc.c2", 256)] == {S.C32}
        if name == "tail_2104":
            assert lc[("genc.c1", 512)] == {S.C64} and lc[("genc.c2", 256)] == {S.C32_64} and S.tail_split(n * T, 512, 31, 256, cus) == 8
        if name == "one_997":
            assert n == 1 and lc[("genc.c1", 512)] == {S.C32_64}
        if name == "wide_4040":
            assert lc[("genc.c2", 256)] == {S.C64} and lc[("wn.in", 160)] == {S.C32_64}
        if name == "long":
            assert all(v == {S.C64} for (layer, _), v in lc.items() if layer.split(".")[0] in ("global_conv_in", "genc", "wn"))
        if name == "passes":
            assert [p[0] for p in S.passes_of(lens)] == [8, 3]


def _judge(tag, got, want, bounds):
    j = S.judge(got, want, bounds)
    for t, (r, m) in S.worst(j).items():
        print(f"[style-vs-f64] {tag} {t:8s}: rms {min(j['rms'][t]):.3e} .. {r:.3e} (bound {bounds[t][0]:.3e}), max {m:.3e} (bound {bounds[t][1]:.3e})")
    assert all(j["ok"]), (tag, j)
    return j


def _check_pass(tag, name, style, ids, cnt, refs):
    """Style vector, ids and counts of the slots of a pass against their references."""
    style, ids, cnt = style.cpu(), ids.cpu(), cnt.cpu()
    unsafe, tokens = 0, 0
    for i, own in enumerate(refs):
        k = own["ids"].shape[0]
        assert int(cnt[i]) == k, (tag, i, int(cnt[i]), k)
        assert bool((ids[i, k:] == -1).all()), (tag, i, "ids past the slot's tokens")
        unsafe += S.check_ids(ids[i, :k], own, S.BAND)
        tokens += k
    print(f"[style-vs-f64] {tag}: {unsafe} unsafe of {tokens} tokens")
    _judge(tag, {"style": [style[i] for i in range(len(refs))]}, {"style": [own["style"] for own in refs]}, BOUNDS[name])


# ------------------------------------------------------------------------------------------------------------ 1. the batched pass
@pytest.mark.parametrize("name", list(S.CASES))
def test_batched_pass(sets, name):
    c, r = S.CASES[name], _refs(name)
    st = sets(name)
    names = _pass(st, name)
    _assert_plan(names, name, c["lens"])
    ids, cnt = st.prosody_ids(c["slots"])
    _check_pass(name, name, st.style_embed(c["slots"]), ids, cnt, r["own"])


def test_limb_stream_set_runs_no_limb_kernel():
    """A stream-set whose vocoder runs the bf16-limb kernels keeps the style pass on the fp32 MFMA: no limb (or conv_tall) launch, the same
    plan, the same bounds."""
    from conan_amd import configs, synth
    from conan_amd.runtime import Context
    hp, sd_np, _ = P.model()
    vhp = configs.hifigan_hparams()
    full = Context(hp, vhp, 0, emformer=False, conan=True, hifigan=True)
    full.load_state_dict("conan", sd_np)
    full.load_state_dict("hifigan", synth.hifigan_state_dict(vhp, 0))
    full.finalize()
    for name in ("short", "edge_1992"):
        c, r = S.CASES[name], _refs(name)
        st = full.streams(c["max_slots"], S.STEP_FRAMES, c["max_ref"], arith="limb")
        assert st.arith == "limb"
        st.reset(c["slots"])
        names = _pass(st, name)
        assert not [k for k in names if "limb" in k or "tall" in k], sorted(names)
        _assert_plan(names, name, c["lens"])
        ids, cnt = st.prosody_ids(c["slots"])
        _check_pass(name + " (limb set)", name, st.style_embed(c["slots"]), ids, cnt, r["own"])
        st.close()
    full.close()


# ------------------------------------------------------------------------------------------------------------ 2. K/V rows
def row_off(tokens, hidden=H):
    """voice::row_off (csrc/voice_layout.h), restated: byte offsets of a row's regions - style [H] f32, the count's 16-byte cell, ids
    and mask [tokens] padded to 16-byte cells, then per layer [tokens][K | V] f32."""
    pad = lambda b: (b + 15) // 16 * 16
    o = {"count": hidden * 4}
    o["ids"] = o["count"] + 16
    o["mask"] = o["ids"] + pad(tokens * 4)
    o["kv0"] = o["mask"] + pad(tokens * 4)
    o["kv1"] = o["kv0"] + tokens * 2 * hidden * 4
    o["bytes"] = o["kv1"] + tokens * 2 * hidden * 4
    return o


def _cut(row, tokens):
    """An exported row (uint8, cpu) -> dict(style [H], count, ids [tokens], mask [tokens], kv0 / kv1 [tokens, 2H])."""
    o = row_off(tokens)
    b = row.numpy().tobytes()
    f = lambda lo, n, dt: np.frombuffer(b, dt, n, lo).copy()
    return dict(style=f(0, H, np.float32), count=int(f(o["count"], 1, np.int32)[0]), ids=f(o["ids"], tokens, np.int32), mask=f(o["mask"], tokens, np.float32),
                kv0=f(o["kv0"], tokens * 2 * H, np.float32).reshape(tokens, 2 * H), kv1=f(o["kv1"], tokens * 2 * H, np.float32).reshape(tokens, 2 * H))


def _check_bank(tag, name, ctx, via, mels, refs, bank_max_ref, keys):
    """Enrol `mels` through `via` into a bank of bank_max_ref (one call, ids in reverse order), export it and judge every row."""
    n = len(mels)
    bank = ctx.voices(n, bank_max_ref)
    vids = list(range(n))[::-1]
    ref, lens = S.padded(mels)
    ref = torch.from_numpy(ref).cuda()
    names = kernels_of(via, lambda: bank.enroll(vids, ref, lens, via=via))
    assert names == S.call_kernels(lens, _num_cu(), 1), (tag, sorted(names.items()))      # one voice per pass
    vs = bank.export(vids)
    blob = vs.blob.cpu()
    got, want = {t: [] for t in ("style", "kv0", "kv1")}, {t: [] for t in ("style", "kv0", "kv1")}
    unsafe = 0
    for i, own in enumerate(refs):
        k = own["ids"].shape[0]
        info = vs.info(i)
        assert info["tokens"] == k == bank.info(vids[i])["tokens"] and info["ref_frames"] == lens[i] and info["bytes"] == row_off(k)["bytes"], (tag, i, info)
        row = _cut(blob[i], k)
        assert row["count"] == k
        assert not row["mask"].view(np.uint32).any(), (tag, i, "a token's key mask is not +0.0")
        unsafe += S.check_ids(row["ids"], own, S.BAND)
        w = S.style_reference(mels[i], ids_override=row["ids"], key=keys[i], exact_positions=True)
        for t, a, b in (("style", row["style"], w["style"]), ("kv0", row["kv0"], w["kv"][0]), ("kv1", row["kv1"], w["kv"][1])):
            got[t].append(a)
            want[t].append(b)
    print(f"[style-vs-f64] {tag}: {unsafe} unsafe of {sum(o['ids'].shape[0] for o in refs)} tokens")
    _judge(tag, got, want, BOUNDS[name])
    bank.close()


@pytest.mark.parametrize("name", list(S.CASES))
def test_kv_rows_of_enrolled_voices(ctx, sets, name):
    c, r = S.CASES[name], _refs(name)
    st = sets(name)
    keys = [(name, i) for i in range(len(r["mels"]))]
    _check_bank(name + " bank", name, ctx, st, r["mels"], r["own"], c["max_ref"], keys)
    if name == "long":
        # the voice of exactly max_ref_frames, alone: 512 tokens
        m = S.long_voice_mel()
        key = (name, len(r["mels"]))
        own = S.style_reference(m, key=key)
        assert own["ids"].shape[0] == 512
        _check_bank(name + " 2048-frame voice", name, ctx, st, [m], [own], c["max_ref"], [key])
        # a bank whose max_ref_frames differs from the stream-set's: the rows of a 505- and a 66-frame voice in a bank of 512
        pick = [7, 3]
        _check_bank(name + " bank of 512", name, ctx, st, [r["mels"][i] for i in pick], [r["own"][i] for i in pick], 512, [keys[i] for i in pick])


# ------------------------------------------------------------------------------------------------------------ 3. the attention that reads them
def _steps(st, slots, codes, taps):
    """STEPS decoder steps of STEP_FRAMES frames -> (mel [n, frames, 80] cpu, attn [2][n, frames, S_max] cpu or None, bins or None)."""
    mels, attn, bins = [], [[], []], []
    for p in range(0, codes.shape[1], S.STEP_FRAMES):
        out = st.decoder_step(slots, codes[:, p:p + S.STEP_FRAMES].contiguous(), taps=taps)
        if taps:
            mels.append(out[0].cpu())
            bins.append(out[1]["pitch_bins"].cpu())
            for l in range(2):
                attn[l].append(out[1]["attn"][l].cpu())
        else:
            mels.append(out.cpu())
    if not taps:
        return torch.cat(mels, 1), None, None
    return torch.cat(mels, 1), [torch.cat(a, 1) for a in attn], torch.cat(bins, 1)


@pytest.mark.parametrize("name", list(S.CASES))
def test_attention_reads_the_rows(ctx, sets, name):
    c, r = S.CASES[name], _refs(name)
    slots, n = c["slots"], len(c["slots"])
    st = sets(name)
    st.reset(slots)
    _pass(st, name)
    ids, cnt = st.prosody_ids(slots)
    ids = ids.cpu()
    codes = torch.from_numpy(r["codes"]).int().cuda()
    assert codes.shape[1] == S.STEPS * S.STEP_FRAMES
    mel_t, attn, bins = _steps(st, slots, codes, True)           # the separate launches: xattn_tile
    got, want = {t: [] for t in ("attn0", "attn1", "mel_out")}, {t: [] for t in ("attn0", "attn1", "mel_out")}
    for i, own in enumerate(r["own"]):
        k = own["ids"].shape[0]
        S.check_ids(ids[i, :k], own, S.BAND)
        w = S.style_reference(r["mels"][i], ids_override=ids[i, :k], key=(name, i), exact_positions=True)
        d = S.decode_reference(w, r["codes"][i], bins_override=bins[i])
        for l in range(2):
            assert not attn[l][i, :, k:].numpy().view(np.uint32).any(), (name, i, l, "attn past the slot's tokens is not +0.0")
            got[f"attn{l}"].append(attn[l][i, :, :k])
            want[f"attn{l}"].append(d["attn"][l])
        got["mel_out"].append(mel_t[i])
        want["mel_out"].append(d["mel"])
    _judge(name + " taps", got, want, BOUNDS[name])
    # without taps: the persistent launch (several row tiles at 8 slots, xcd mode at one and two) - mg_xattn_rows.  decoder_step falls
    # back to the separate launches without a word where the persistent launch declines, so the launches are asserted
    st.reset(slots, which=2)
    out = {}
    names = kernels_of(st, lambda: out.setdefault("m", _steps(st, slots, codes, False)))
    mel_m = out["m"][0]
    assert any("decoder_mega_kernel" in k for k in names) and not any("rowconv_kernel" in k or "rowlin_kernel" in k for k in names), (name, sorted(names))
    assert sum(v for k, v in names.items() if "decoder_mega_kernel" in k) == S.STEPS, (name, sorted(names.items()))
    form = ", 3>" if n * S.STEP_FRAMES > 16 else ", 2>"      # decoder_mega_kernel<OCC, CM>: CM = 3 several row tiles, CM = 2 xcd mode (one tile)
    assert all(k.endswith(form) for k in names if "decoder_mega_kernel" in k), (name, n, sorted(names))
    np.testing.assert_allclose(mel_m.numpy(), mel_t.numpy(), **MEGA_TOL)
    # ... and the separate launches of a DEC_MEGA=0 set
    sep = ctx.streams(c["max_slots"], S.STEP_FRAMES, c["max_ref"], dev_plan="DEC_MEGA=0")
    sep.reset(slots)
    ref, lens = S.padded(r["mels"])
    sep.set_reference(slots, torch.from_numpy(ref).cuda(), lens)
    names = kernels_of(sep, lambda: out.setdefault("s", _steps(sep, slots, codes, False)))
    mel_s = out["s"][0]
    sep.close()
    assert any("rowconv_kernel" in k for k in names) and not any("decoder_mega_kernel" in k for k in names), (name, sorted(names))
    np.testing.assert_allclose(mel_m.numpy(), mel_s.numpy(), **MEGA_TOL)
    np.testing.assert_allclose(mel_t.numpy(), mel_s.numpy(), **MEGA_TOL)
    print(f"[style-vs-f64] {name}: persistent against taps max |d| {float((mel_m - mel_t).abs().max()):.3e}, against DEC_MEGA=0 {float((mel_m - mel_s).abs().max()):.3e}")


# ------------------------------------------------------------------------------------------------------------ 4. a slot that had a longer voice
def test_slot_that_had_a_longer_voice(ctx, sets):
    """The 512-token slot of `long` is given a 5-frame reference (row 4 of `short`): its style, ids, count and the next decoder steps' mel are, bit for
    bit, those of a fresh stream-set's slot given the 5-frame reference alone - nothing of the 510 rows the longer voice left behind
    is read.  (Bitwise only because both passes launch the same shapes, which is asserted.)"""
    name = "long"
    c, r = S.CASES[name], _refs(name)
    slot = c["slots"][0]
    assert c["lens"][0] == 2045
    st = sets(name)
    st.reset(c["slots"])
    _pass(st, name)
    assert int(st.prosody_ids([slot])[1][0]) == 512
    assert S.CASES["short"]["lens"][4] == 5
    five = torch.from_numpy(_refs("short")["mels"][4][None]).cuda()
    codes = torch.from_numpy(r["codes"][:1]).int().cuda()
    na = kernels_of(st, lambda: st.set_reference([slot], five))
    fresh = ctx.streams(c["max_slots"], S.STEP_FRAMES, c["max_ref"])
    fresh.reset([slot])
    nb = kernels_of(fresh, lambda: fresh.set_reference([slot], five))
    assert na == nb == S.call_kernels([5], _num_cu()), (sorted(na.items()), sorted(nb.items()))
    ia, ca = st.prosody_ids([slot])
    ib, cb = fresh.prosody_ids([slot])
    assert int(ca[0]) == 2 and torch.equal(ca, cb) and torch.equal(ia, ib) and bool((ia[0, 2:] == -1).all())
    assert torch.equal(st.style_embed([slot]), fresh.style_embed([slot]))
    st.reset([slot], which=2)
    for taps in (False, True):
        ma, aa, _ = _steps(st, [slot], codes, taps)
        mb, ab, _ = _steps(fresh, [slot], codes, taps)
        assert torch.equal(ma, mb) and bool(torch.isfinite(ma).all()), taps
        if taps:
            assert torch.equal(aa[0], ab[0]) and torch.equal(aa[1], ab[1]) and not aa[0][0, :, 2:].numpy().view(np.uint32).any()
        st.reset([slot], which=2)
        fresh.reset([slot], which=2)
    # against float64 too: the slot is judged like any other
    own = _refs("short")["own"][4]
    S.check_ids(ia[0, :2].cpu(), own, S.BAND)
    _judge("long, then 5 frames", {"style": [st.style_embed([slot])[0].cpu()]}, {"style": [own["style"]]}, BOUNDS["short"])
    fresh.close()


# ------------------------------------------------------------------------------------------------------------ the table
def test_bounds_follow_the_rule():
    """The bounds are the stated rule applied to the recorded oracle figures, per case and tensor; every one stays below 1e-5 (rms), so
    a two-limb product (2^-16) still fails."""
    assert set(ORACLE_FP32) == set(S.CASES) and (RMS_FACTOR, MAX_FACTOR) == (8.0, 16.0)
    for c, v in ORACLE_FP32.items():
        assert set(v) == set(S.TENSORS)
        for t, (r, m) in v.items():
            assert BOUNDS[c][t] == (8 * r, 16 * m)
            assert 0 < BOUNDS[c][t][0] < 1e-5 and 0 < BOUNDS[c][t][1] < 1e-4
