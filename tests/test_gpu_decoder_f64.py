"""The decoder step (conan_decoder_step: csrc/decoder.hip, decoder_mega.hip, rowops.h, rowconv.hip) against FLOAT64, per slot and per
step, across its launch forms: the separate launches (rowconv_kernel / rowlin_kernel; conv_mfma with ROWCONV=0), the single-tile
persistent launch (xcd mode, decoder_mega_kernel<4, 2>) and the multi-tile persistent launch in both builds - <4, 3>, the 128-register
build of every limb stream-set, and <6, 3> of the f32 sets - with 8, 16 and 24 groups, more jobs than groups, ragged last tiles, 1 to
16 frames per slot, slots at different ring positions, CONAN_STREAMS_FUSED_DECODER_BLOCKS / _FIXED_PLAN / _SEPARATE_SMALL_STEPS, the
non-default MEGA_* switches of the shipped library, and a program re-recorded after the 12-entry cache evicted it.

tests/decoder_ref.py holds the runs, the cases, the float64 reference and the restated plan.  Two contexts with the full-size
synthetic checkpoint: Conan alone for the f32 sets, Conan + vocoder for the limb sets.  The four voices are enrolled once per context
into a voice bank and assigned; the float64 style side embeds the VQ ids the GPU chose and style_ref.position_table.  Per case one
stream-set; per step the launches are asserted against the restated plan (conftest.kernels_of) and every active slot's mel_out - in
tapped runs also content_embed_proj, both attention maps, uv_pred, decoder_inp and the bins - is judged with style_ref.judge.

Bounds: per slot, step and tensor the relative rms error <= RMS_FACTOR (8) x the fp32 oracle's, the largest error over the slot's rms
<= MAX_FACTOR (16) x the fp32 oracle's, where the oracle's figures (ORACLE_FP32, the worst slot and step of the run, measured on the
CPU against the float64 reference; tests/test_decoder_ref_cpu.py recomputes them) come from the run's own inputs.  No figure comes
from the kernels under test.  Pitch bins: see tests/decoder_ref.py - a tapped run's bins are embedded and asserted on safe rows; a
persistent launch is compared with the float64 law's own bins, a slot's rows from its first unsafe row on left out (none with the
recorded seeds).

What the cases found about the plan: a step of ONE frame per slot never takes the persistent launch - rowconv takes T >= 2
(rowconv.hip rowconv_supported), the recording meets a conv_mfma layer and the step keeps its separate launches at any slot count.
The case `t1n17` (17 slots of one frame) therefore asserts conv_mfma + rowlin launches, not two tiles of 16 slots, and holds those to
float64 like every other form.  Pipelined steps are not visible to the profile hooks: their launch assertion is that of a blocking
conan_step of the same shape on the same stream-set.  Nothing else is left out; no bound failed (profiles/decoder_vs_f64.txt)."""
import numpy as np
import pytest
import torch

from tests import decoder_ref as D
from tests import pitch_ref as P
from tests import style_ref as S
from tests.conftest import kernels_of
from tests.test_gpu_vocoder_f64 import MAX_FACTOR, RMS_FACTOR

pytestmark = pytest.mark.gpu

# run: {tensor: (oracle fp32 rms, oracle fp32 max)} as measured on the CPU (one thread: decoder_ref.one_thread), the worst slot and step
ORACLE_FP32 = {
    "g5": {"content_embed_proj": (3.749e-07, 2.551e-06), "attn0": (2.360e-07, 1.033e-06), "attn1": (2.285e-07, 7.873e-07), "uv_pred": (1.436e-07, 2.653e-07), "decoder_inp": (2.338e-07, 1.606e-06), "mel_out": (5.796e-07, 2.453e-06)},
    "g32": {"content_embed_proj": (1.648e-07, 1.055e-06), "attn0": (2.250e-07, 1.019e-06), "attn1": (2.273e-07, 1.255e-06), "uv_pred": (1.504e-07, 2.812e-07), "decoder_inp": (2.186e-07, 1.135e-06), "mel_out": (4.687e-07, 2.322e-06)},
    "g33": {"content_embed_proj": (1.648e-07, 1.055e-06), "attn0": (2.250e-07, 1.019e-06), "attn1": (2.273e-07, 1.255e-06), "uv_pred": (1.504e-07, 2.812e-07), "decoder_inp": (2.208e-07, 1.135e-06), "mel_out": (4.687e-07, 2.322e-06)},
    "g65": {"content_embed_proj": (1.656e-07, 1.306e-06), "attn0": (3.070e-07, 1.255e-06), "attn1": (2.654e-07, 1.570e-06), "uv_pred": (1.739e-07, 2.874e-07), "decoder_inp": (2.430e-07, 1.210e-06), "mel_out": (4.830e-07, 3.026e-06)},
    "t1n17": {"content_embed_proj": (1.827e-07, 1.112e-06), "attn0": (2.200e-07, 7.124e-07), "attn1": (2.043e-07, 8.337e-07), "uv_pred": (9.566e-08, 1.309e-07), "decoder_inp": (2.076e-07, 8.813e-07), "mel_out": (3.331e-07, 1.137e-06)},
    "t1n16": {"content_embed_proj": (1.827e-07, 1.112e-06), "attn0": (2.200e-07, 7.124e-07), "attn1": (2.043e-07, 8.337e-07), "uv_pred": (9.566e-08, 1.309e-07), "decoder_inp": (2.076e-07, 8.813e-07), "mel_out": (3.331e-07, 1.137e-06)},
    "t2n9": {"content_embed_proj": (1.662e-07, 9.732e-07), "attn0": (2.295e-07, 7.398e-07), "attn1": (1.817e-07, 6.240e-07), "uv_pred": (8.869e-08, 1.356e-07), "decoder_inp": (1.967e-07, 9.058e-07), "mel_out": (4.605e-07, 1.915e-06)},
    "t8n3": {"content_embed_proj": (3.687e-07, 2.805e-06), "attn0": (2.263e-07, 8.887e-07), "attn1": (2.407e-07, 8.866e-07), "uv_pred": (2.563e-07, 5.469e-07), "decoder_inp": (2.682e-07, 1.839e-06), "mel_out": (5.714e-07, 2.473e-06)},
    "t16n2": {"content_embed_proj": (3.722e-07, 2.910e-06), "attn0": (1.792e-07, 8.095e-07), "attn1": (1.581e-07, 6.823e-07), "uv_pred": (1.864e-07, 4.966e-07), "decoder_inp": (2.879e-07, 1.932e-06), "mel_out": (6.144e-07, 2.732e-06)},
    "t3n6": {"content_embed_proj": (3.782e-07, 2.350e-06), "attn0": (2.460e-07, 7.657e-07), "attn1": (2.420e-07, 7.929e-07), "uv_pred": (1.306e-07, 1.686e-07), "decoder_inp": (2.371e-07, 1.549e-06), "mel_out": (5.657e-07, 2.342e-06)},
    "x1t2": {"content_embed_proj": (3.693e-07, 1.724e-06), "attn0": (6.487e-08, 1.193e-07), "attn1": (6.747e-08, 1.193e-07), "uv_pred": (1.499e-07, 2.813e-07), "decoder_inp": (2.707e-07, 1.127e-06), "mel_out": (5.573e-07, 2.407e-06)},
    "x4t4": {"content_embed_proj": (3.749e-07, 2.551e-06), "attn0": (2.360e-07, 1.033e-06), "attn1": (2.285e-07, 7.873e-07), "uv_pred": (1.571e-07, 3.167e-07), "decoder_inp": (2.797e-07, 1.606e-06), "mel_out": (6.042e-07, 2.453e-06)},
    "x1t16": {"content_embed_proj": (3.722e-07, 2.784e-06), "attn0": (8.871e-08, 2.179e-07), "attn1": (1.337e-07, 3.145e-07), "uv_pred": (1.770e-07, 4.966e-07), "decoder_inp": (2.879e-07, 1.932e-06), "mel_out": (6.144e-07, 2.449e-06)},
    "x2t8": {"content_embed_proj": (3.687e-07, 2.805e-06), "attn0": (1.529e-07, 5.342e-07), "attn1": (1.597e-07, 6.673e-07), "uv_pred": (2.563e-07, 5.469e-07), "decoder_inp": (2.682e-07, 1.839e-06), "mel_out": (5.714e-07, 2.329e-06)},
    "x5t3": {"content_embed_proj": (3.880e-07, 2.350e-06), "attn0": (2.460e-07, 7.657e-07), "attn1": (2.420e-07, 7.929e-07), "uv_pred": (1.511e-07, 2.780e-07), "decoder_inp": (2.454e-07, 1.549e-06), "mel_out": (5.915e-07, 2.186e-06)},
    "long": {"content_embed_proj": (3.875e-07, 3.947e-06), "attn0": (2.554e-07, 1.033e-06), "attn1": (2.285e-07, 9.956e-07), "uv_pred": (2.668e-07, 4.282e-07), "decoder_inp": (2.797e-07, 2.241e-06), "mel_out": (6.042e-07, 2.453e-06)},
    "longmix": {"content_embed_proj": (3.935e-07, 3.911e-06), "attn0": (2.605e-07, 1.880e-06), "attn1": (2.533e-07, 1.280e-06), "uv_pred": (2.365e-07, 5.177e-07), "decoder_inp": (2.729e-07, 2.012e-06), "mel_out": (5.823e-07, 3.463e-06)},
    "fp33": {"content_embed_proj": (1.648e-07, 1.055e-06), "attn0": (2.250e-07, 1.019e-06), "attn1": (2.273e-07, 1.255e-06), "uv_pred": (1.504e-07, 2.812e-07), "decoder_inp": (2.208e-07, 1.135e-06), "mel_out": (4.687e-07, 2.322e-06)},
    "s2": {"content_embed_proj": (3.618e-07, 2.551e-06), "attn0": (1.283e-07, 3.140e-07), "attn1": (1.172e-07, 3.255e-07), "uv_pred": (1.571e-07, 3.167e-07), "decoder_inp": (2.797e-07, 1.376e-06), "mel_out": (6.042e-07, 2.339e-06)},
    "cache": {"content_embed_proj": (3.787e-07, 2.695e-06), "attn0": (2.554e-07, 1.033e-06), "attn1": (2.285e-07, 7.873e-07), "uv_pred": (2.707e-07, 4.633e-07), "decoder_inp": (2.867e-07, 1.672e-06), "mel_out": (6.215e-07, 2.498e-06)},
    "c5t4": {"content_embed_proj": (3.749e-07, 2.551e-06), "attn0": (2.360e-07, 1.033e-06), "attn1": (2.285e-07, 7.873e-07), "uv_pred": (1.436e-07, 2.653e-07), "decoder_inp": (2.351e-07, 1.605e-06), "mel_out": (5.565e-07, 2.468e-06)},
    "c2t4": {"content_embed_proj": (3.618e-07, 2.551e-06), "attn0": (1.283e-07, 3.140e-07), "attn1": (1.172e-07, 3.255e-07), "uv_pred": (1.571e-07, 3.167e-07), "decoder_inp": (2.721e-07, 1.355e-06), "mel_out": (5.580e-07, 2.436e-06)},
    "c6t3": {"content_embed_proj": (3.782e-07, 2.350e-06), "attn0": (2.460e-07, 7.657e-07), "attn1": (2.420e-07, 7.929e-07), "uv_pred": (1.306e-07, 1.686e-07), "decoder_inp": (2.327e-07, 1.580e-06), "mel_out": (5.981e-07, 2.408e-06)},
    "fp2": {"content_embed_proj": (3.630e-07, 2.282e-06), "attn0": (2.360e-07, 1.033e-06), "attn1": (2.285e-07, 7.631e-07), "uv_pred": (1.424e-07, 2.685e-07), "decoder_inp": (2.718e-07, 1.606e-06), "mel_out": (6.189e-07, 2.377e-06)},
    "p5": {"content_embed_proj": (3.453e-07, 2.109e-06), "attn0": (2.394e-07, 8.379e-07), "attn1": (2.195e-07, 7.014e-07), "uv_pred": (1.421e-07, 3.007e-07), "decoder_inp": (2.412e-07, 1.323e-06), "mel_out": (5.870e-07, 3.016e-06)},
    "p2": {"content_embed_proj": (3.457e-07, 2.251e-06), "attn0": (1.672e-07, 3.995e-07), "attn1": (1.288e-07, 5.443e-07), "uv_pred": (1.448e-07, 2.871e-07), "decoder_inp": (2.803e-07, 1.601e-06), "mel_out": (6.084e-07, 2.313e-06)},
}
BOUNDS = {r: {t: (RMS_FACTOR * a, MAX_FACTOR * b) for t, (a, b) in v.items()} for r, v in ORACLE_FP32.items()}


# ------------------------------------------------------------------------------------------------------------ fixtures
class _Side:
    """A context, the bank with the four voices, and the float64 style side that embeds the ids this context's pass chose."""

    def __init__(self, vocoder, emformer=False):
        from conan_amd import configs, synth
        from conan_amd.runtime import Context
        hp, sd_np, _ = P.model()
        vhp = configs.hifigan_hparams() if vocoder else None
        self.ctx = Context(hp, vhp, 0, emformer=emformer, conan=True, hifigan=vocoder)
        if emformer:
            self.ctx.load_state_dict("emformer", synth.emformer_state_dict(hp, 0))
        self.ctx.load_state_dict("conan", sd_np)
        if vocoder:
            self.ctx.load_state_dict("hifigan", synth.hifigan_state_dict(vhp, 0))
        self.ctx.finalize()
        self.bank = self.ctx.voices(D.NV, D.MAX_REF)
        via = self.ctx.streams(D.NV, 4, D.MAX_REF)
        mels = D.voice_mels()
        ref, lens = S.padded(mels)
        self.bank.enroll(list(range(D.NV)), torch.from_numpy(ref).cuda(), lens, via=via)
        slots = [2, 0, 3, 1]
        via.reset(slots)
        via.set_voice(slots, self.bank, list(range(D.NV)))
        ids, cnt = via.prosody_ids(slots)
        ids, cnt = ids.cpu(), cnt.cpu()
        own = D.voices(torch.float64)
        used = []
        for v in range(D.NV):
            k = own[v]["ids"].shape[0]
            assert int(cnt[v]) == k == S.tokens_of(D.VOICE_LENS[v])
            S.check_ids(ids[v, :k], own[v], S.BAND)
            used.append(ids[v, :k].clone())
        self.vo = D.voices(torch.float64, ids=used, exact_positions=True)
        self.tokens = [int(c) for c in cnt]
        via.close()
        self.refs = {}

    def close(self):
        self.bank.close()
        self.ctx.close()


@pytest.fixture(scope="module")
def sides():
    made = {}

    def get(arith):
        if arith not in made:
            made[arith] = _Side(vocoder=arith != "f32", emformer=arith == "full")      # ("full": Emformer, Conan and vocoder - the pipelined steps)
        return made[arith]
    yield get
    for s in made.values():
        s.close()


def _num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ------------------------------------------------------------------------------------------------------------ a case on the GPU
_GOT = {}


def _gpu_run(sides, name):
    """The case's steps on a stream-set of its own, each step's launches asserted -> per step dicts in run_reference's layout."""
    if name in _GOT:
        return _GOT[name]
    c = D.CASES[name]
    run = D.RUNS[c["run"]]
    side = sides(c["arith"])
    st = side.ctx.streams(run["max_slots"], run["max_frames"], D.MAX_REF, arith=c["arith"], flags=c["flags"], dev_plan=c["dev_plan"])
    assert st.arith == c["arith"]
    st.reset(run["slots"])
    st.set_voice(run["slots"], side.bank, [run["voice"][s] for s in run["slots"]])
    plans = D.case_plans(name, _num_cu())
    got = []
    for k, si in enumerate(D.step_inputs(run)):
        if k in run["resets"]:
            st.reset(run["resets"][k], which=2)
        codes = torch.from_numpy(si["codes"]).int().cuda()
        kw = {} if si["f0"] is None else dict(f0=torch.from_numpy(si["f0"]).cuda(), uv=torch.from_numpy(si["uv"]).cuda())
        out = {}
        names = kernels_of(st, lambda: out.setdefault("o", st.decoder_step(si["slots"], codes, taps=c["taps"], **kw)))
        D.check_launches(names, plans[k])
        g = dict(slots=si["slots"], T=si["T"])
        if c["taps"]:
            mel, taps = out["o"]
            g["mel_out"] = mel.cpu()
            for t in ("content_embed_proj", "uv_pred", "decoder_inp"):
                g[t] = taps[t].cpu()
            g["bins"] = taps["pitch_bins"].cpu().numpy().astype(np.int64)
            for l in range(2):
                a = taps["attn"][l].cpu()
                toks = [side.tokens[run["voice"][s]] for s in si["slots"]]
                for i, kt in enumerate(toks):
                    assert not a[i, :, kt:].numpy().view(np.uint32).any(), (name, k, i, l, "attn past the slot's tokens is not +0.0")
                g[f"attn{l}"] = [a[i, :, :kt] for i, kt in enumerate(toks)]
        else:
            g["mel_out"] = out["o"].cpu()
        got.append(g)
    st.close()
    _GOT[name] = got
    return got


def _reference(side, name, got):
    """The float64 steps the case is judged against, and the rows kept."""
    c = D.CASES[name]
    run = D.RUNS[c["run"]]
    if c["taps"]:
        ref = D.run_reference(run, side.vo, bins=[g["bins"] for g in got])
        for g, r in zip(got, ref):      # (r["bins"]: the float64 law's own)
            safe = ~r["unsafe"]
            assert (g["bins"][safe] == r["bins"][safe]).all(), (name, "a safe row's bin differs from the float64 law's")
        return ref, None, 0, sum(r["T"] * len(r["slots"]) for r in ref)
    if c["run"] not in side.refs:
        side.refs[c["run"]] = D.run_reference(run, side.vo)
    ref = side.refs[c["run"]]
    keep, lost, rows = D.keep_rows(run, ref)
    assert lost <= D.MAX_LEFT_OUT * rows, (name, lost, rows)
    return ref, keep, lost, rows


def _geometry(name):
    plans = D.case_plans(name, _num_cu())
    seen = []
    many = len(set(D.RUNS[D.CASES[name]["run"]]["steps"][k][1] for k in range(len(plans)))) > 1 or len({len(sl) for sl, _ in D.RUNS[D.CASES[name]["run"]]["steps"]}) > 1
    for p, (slots, T) in zip(plans, D.RUNS[D.CASES[name]["run"]]["steps"]):
        s = ("" if many else f"n={len(slots)} T={T} ") + ("separate" + ("" if p["rowconv"] else " (conv_mfma)") if p["form"] == "separate" else
                                        f"{p['kernel'][5:]} {p['njobs']} jobs on {p['groups']} x {p['group_size']}")
        if s not in seen:
            seen.append(s)
    return "; ".join(seen)


@pytest.mark.parametrize("name", list(D.CASES))
def test_decoder_step_against_float64(sides, name):
    c = D.CASES[name]
    side = sides(c["arith"])
    got = _gpu_run(sides, name)
    ref, keep, lost, rows = _reference(side, name, got)
    tensors = D.TAPS if c["taps"] else ("mel_out",)
    b = BOUNDS[c["run"]]
    ok, worst, bad = D.judge_steps(got, ref, b, tensors, keep)
    ratio = max(max(worst[t][0] / b[t][0], worst[t][1] / b[t][1]) for t in tensors)
    print(f"[decoder-vs-f64] {name} ({c['arith']}{', taps' if c['taps'] else ''}{', flags ' + str(c['flags']) if c['flags'] else ''}{', ' + c['dev_plan'] if c['dev_plan'] else ''}): "
          f"{_geometry(name)}; {rows - lost} of {rows} rows; mel_out rms {worst['mel_out'][0]:.3e} (bound {b['mel_out'][0]:.3e}) max {worst['mel_out'][1]:.3e} "
          f"(bound {b['mel_out'][1]:.3e}); worst ratio to a bound {ratio:.3f}")
    if c["taps"]:
        for t in tensors:
            print(f"[decoder-vs-f64]   {name} {t:18s}: rms {worst[t][0]:.3e} (bound {b[t][0]:.3e}), max {worst[t][1]:.3e} (bound {b[t][1]:.3e})")
    assert ok, (name, bad, worst)


@pytest.mark.parametrize("name", list(D.PIPE_RUNS))
def test_pipelined_steps_against_float64(sides, name):
    """conan_step_async on the full context (Emformer -> decoder -> vocoder on three internal streams): the decoder step's program
    carries the copy of the step's codes and the twin mel_out operator that writes the caller's mel.  Each step's returned mel is
    judged against the float64 reference fed the codes that step returned, with the float64 law's own bins.  Pipelined launches are
    not visible to the profile hooks; the launch assertion is that of a blocking conan_step of the same shape on the same set."""
    run = D.RUNS[name]
    side = sides("full")
    slots, n = run["slots"], len(run["slots"])
    st = side.ctx.streams(run["max_slots"], run["max_frames"], D.MAX_REF)
    assert st.arith == "limb"
    st.reset(slots)
    st.set_voice(slots, side.bank, [run["voice"][s] for s in slots])
    keep = []
    for ch in D.pipe_chunks(name, st.seg, st.rc):
        c, m = torch.empty(n, st.seg, dtype=torch.int32, device="cuda"), torch.empty(n, st.seg, 80, device="cuda")
        w = torch.empty(n, st.seg * side.ctx.hop, device="cuda")
        st.step_async(slots, torch.from_numpy(ch).cuda(), w, codes=c, mel_out=m)
        keep.append((c, m, w))
    st.join()
    torch.cuda.synchronize()
    codes = [k[0].cpu().numpy().astype(np.int64) for k in keep]
    got = [dict(slots=slots, T=st.seg, mel_out=k[1].cpu()) for k in keep]
    assert st.seg == run["steps"][0][1] and all(bool(torch.isfinite(k[2]).all()) for k in keep)
    differ = int((np.concatenate(codes, 1) != D.pipe_codes(name)).sum())
    ref = D.run_reference(run, side.vo, hooks=dict(codes=lambda k, c: codes[k]))
    rows_kept, lost, rows = D.keep_rows(run, ref)
    assert lost <= D.MAX_LEFT_OUT * rows, (name, lost, rows)
    b = BOUNDS[name]
    ok, worst, bad = D.judge_steps(got, ref, b, ("mel_out",), rows_kept)
    p = D.plan(run["max_slots"], n, st.seg, "limb", num_cu=_num_cu())
    st.reset(slots)
    st.set_voice(slots, side.bank, [run["voice"][s] for s in slots])
    ch = torch.from_numpy(D.pipe_chunks(name, st.seg, st.rc)[0]).cuda()
    names = kernels_of(st, lambda: st.step(slots, ch))
    st.close()
    print(f"[decoder-vs-f64] {name} (pipelined, full context): n={n} T={run['steps'][0][1]} {p['kernel'][5:]} {p['njobs']} jobs on {p['groups']} x {p['group_size']}; "
          f"{differ} codes differ from the recorded ones; {rows - lost} of {rows} rows; mel_out rms {worst['mel_out'][0]:.3e} (bound {b['mel_out'][0]:.3e}) "
          f"max {worst['mel_out'][1]:.3e} (bound {b['mel_out'][1]:.3e}); worst ratio to a bound {max(worst['mel_out'][0] / b['mel_out'][0], worst['mel_out'][1] / b['mel_out'][1]):.3f}")
    assert {k: v for k, v in names.items() if "decoder_mega_kernel" in k} == {p["kernel"]: 1} and not any("rowconv_kernel" in k or "rowlin_kernel" in k for k in names), sorted(names.items())
    assert ok, (name, bad, worst)


def test_fixed_plan_bits_do_not_depend_on_the_active_slots(sides):
    """CONAN_STREAMS_FIXED_PLAN: two slots alone on a set of 33 run decoder_mega_kernel<4, 3> (asserted by the case's launches) and give,
    bit for bit, what the same slots give among 33 active ones."""
    full, two = _gpu_run(sides, "fixed_n33"), _gpu_run(sides, "fixed_n2")
    assert all(p["form"] == "tiles" and p["kernel"].endswith("<4, 3>") for p in D.case_plans("fixed_n2", _num_cu()))
    for a, b in zip(full, two):
        for i, s in enumerate(b["slots"]):
            assert torch.equal(b["mel_out"][i], a["mel_out"][a["slots"].index(s)]), s


def test_bounds_follow_the_rule():
    """The bounds are the stated rule applied to the recorded oracle figures, per run and tensor; every rms bound stays below 1e-5, so a
    product formed from two bf16 limbs (2^-16) still fails."""
    assert set(ORACLE_FP32) == set(D.RUNS) and (RMS_FACTOR, MAX_FACTOR) == (8.0, 16.0)
    assert {c["run"] for c in D.CASES.values()} | set(D.PIPE_RUNS) == set(D.RUNS)
    for r, v in ORACLE_FP32.items():
        assert set(v) == set(D.TAPS)
        for t, (a, m) in v.items():
            assert BOUNDS[r][t] == (8 * a, 16 * m)
            assert 0 < BOUNDS[r][t][0] < 1e-5 and 0 < BOUNDS[r][t][1] < 1e-4
