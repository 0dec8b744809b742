"""tests/decoder_ref.py without a GPU: the float64 reference of the decoder step is pinned to oracle/conan.py (its fp32 instance is
decode_frames bit for bit), batched equals alone, the restated plan gives every case the form and the group count it is there for,
the recorded yardsticks (tests/test_gpu_decoder_f64.py ORACLE_FP32), the band (decoder_ref.MAX_MEL_ERR / MAX_D0_ERR) and the seed
table are recomputed, the share of rows left out is capped with the reference alone, and the judge with the GPU test's bounds
rejects deliberate changes to the fp32 oracle's side."""
import contextlib
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import conan as oconan
from tests import decoder_ref as D
from tests import pitch_ref as P
from tests import test_gpu_decoder_f64 as g


@functools.lru_cache(maxsize=None)
def _oracle_run(name):
    return D.oracle_run(D.RUNS[name])


# ------------------------------------------------------------------------------------------------------------ the reference is the oracle
@pytest.mark.parametrize("name", ["g5", "longmix"])
def test_reference_is_the_oracle(name):
    """run_reference in fp32, every slot alone, with nothing overridden IS oracle.conan.decode_frames carried step by step with the
    slot's own state: content_embed_proj, both attention maps, uv_pred, the bins, decoder_inp and mel_out bit for bit (what
    tests/pitch_ref.py claims for decode_frames_pitch with nothing set) - staggered joins, the reset and changing frame counts included."""
    hp, _, sd = P.model()
    run = D.RUNS[name]
    vo = D.voices(torch.float32)
    got = D.run_reference(run, vo, torch.float32, alone=True)
    states = {s: {} for s in run["slots"]}
    for k, (si, r) in enumerate(zip(D.step_inputs(run), got)):
        for s in run["resets"].get(k, []):
            states[s] = {}
        for i, s in enumerate(si["slots"]):
            o = oconan.decode_frames(sd, hp, torch.from_numpy(si["codes"][i:i + 1]), vo[run["voice"][s]]["cache"], states[s])
            for t in ("content_embed_proj", "uv_pred", "decoder_inp", "mel_out"):
                assert torch.equal(o[t][0], r[t][i]), (name, k, s, t)
            assert np.array_equal(o["pitch_bins"][0].numpy(), r["bins"][i]), (name, k, s)
            for l in range(2):
                assert torch.equal(o["attn"][l][0, 0], r[f"attn{l}"][i]), (name, k, s, l)


@pytest.mark.parametrize("name", ["g33", "long", "c6t3"])
def test_batched_equals_alone(name):
    """The slots of one voice in one call (states concatenated, zero state for a slot that joins or was reset) give what each slot
    gives in a call of its own: float64, every tensor within 1e-12 absolute, the bins and the unsafe rows equal."""
    run = D.RUNS[name]
    vo = D.voices()
    a, b = D.run_reference(run, vo), D.run_reference(run, vo, alone=True)
    worst = 0.0
    for x, y in zip(a, b):
        for t in D.TAPS:
            for i in range(len(x["slots"])):
                worst = max(worst, float((x[t][i] - y[t][i]).abs().max()))
        assert np.array_equal(x["bins"], y["bins"]) and np.array_equal(x["unsafe"], y["unsafe"])
    print(f"[decoder-vs-f64] {name}: batched against alone, max |d| {worst:.3e}")
    assert worst <= 1e-12


def test_contour_runs_sit_on_bin_centres():
    """Every f0 of a contour run rounds to its bin from the centre: the float64 law's bins are the ones the contour was built from, the
    mel-scale value is within 1e-3 of the bin (float32 rounding of the log2 Hz value), and no row is unsafe."""
    for name in ("c5t4", "c2t4", "c6t3"):
        run = D.RUNS[name]
        for si, r in zip(D.step_inputs(run), D.run_reference(run, D.voices())):
            assert np.array_equal(r["bins"], si["cbins"]) and not r["unsafe"].any()
            assert np.abs(r["mel_value"] - si["cbins"]).max() < 1e-3


# ------------------------------------------------------------------------------------------------------------ the plan
def _forms(name):
    return [(p["form"], (p["kernel"] or "")[-6:], p["njobs"], p["groups"], p["group_size"]) for p in D.case_plans(name, 256)]


def test_cases_reach_their_launch_forms():
    """On 256 CUs the restated plan gives every case the form, the build and the geometry it is there for."""
    L, F32 = "<4, 3>", "<6, 3>"
    tiles = lambda name, build, njobs, groups, gs=8: _forms(name) == [("tiles", build, njobs, groups, gs)] * 3
    # 1. geometry: two jobs and six idle groups; 8 on 8; 9 on 16; 17 on 16 (group 0 takes a second job, of one slot)
    assert tiles("g5_limb", L, 2, 8) and tiles("g32_limb", L, 8, 8) and tiles("g33_limb", L, 9, 16) and tiles("g65_limb", L, 17, 16)
    assert tiles("g5_f32", F32, 2, 8) and tiles("g33_f32", F32, 9, 16) and tiles("g65_f32", F32, 17, 16)
    assert 5 * 4 - 16 == 4 and 33 * 4 - 8 * 16 == 4 and 65 * 4 - 16 * 16 == 4      # the live rows of the last tile
    # 2. frames per step
    assert tiles("t2n9", L, 2, 8) and tiles("t8n3", L, 2, 8) and tiles("t16n2", L, 2, 8)
    for name in ("t1n17", "t1n16", "t3n6", "c6t3"):
        assert {f[0] for f in _forms(name)} == {"separate"}, name
    # (T = 1: rowconv takes T >= 2, so a one-frame step runs conv_mfma at any slot count - 17 slots are no two tiles of 16)
    assert not D.case_plans("t1n17")[0]["rowconv"] and D.case_plans("t1n17")[0]["rowlin"] and not D.case_plans("t1n16")[0]["rowlin"]
    assert D.case_plans("t3n6")[0]["rowconv"] and D.case_plans("t3n6")[0]["rowlin"]
    for name in ("x1t2", "x4t4", "x1t16", "x2t8", "x5t3", "c2t4"):
        assert _forms(name) == [("xcd", "<4, 2>", 1, 1, 256)] * 3, name
    assert 5 * 3 == 15
    # 3. long and staggered: xcd mode up to four slots, then two tiles; with changing frame counts all three forms
    assert [f[0] for f in _forms("long")] == ["xcd"] * 4 + ["tiles"] * 10
    assert {f[0] for f in _forms("longmix")} == {"xcd", "tiles", "separate"} and {f[1] for f in _forms("longmix_f32")} == {"<4, 2>", F32, ""}
    r = D.RUNS["long"]
    assert max(D.run_frames(r).values()) >= 48 and sum(T for _, T in r["steps"]) >= 48 and list(r["resets"]) == [8]
    # 4. flags and switches
    assert tiles("fused_n33", L, 9, 16) and tiles("fused_n5", L, 2, 8) and tiles("fixed_n33", L, 9, 16) and tiles("fixed_n2", L, 1, 8)
    assert {f[0] for f in _forms("sepsmall_n2")} == {"separate"} and D.plan(4, 2, 4, "limb")["form"] == "xcd"
    assert tiles("gs4", L, 9, 16, 4) and tiles("gs16", L, 9, 8, 16) and tiles("grid64", L, 9, 8) and tiles("grid256_n65", L, 17, 24)
    assert tiles("narrow0", L, 9, 16) and tiles("nol2", L, 9, 16)
    assert {f[0] for f in _forms("rowconv0")} == {"separate"} and not D.case_plans("rowconv0")[0]["rowconv"] and not D.case_plans("rowconv0")[0]["rowlin"]
    assert {f[0] for f in _forms("decmega0")} == {"separate"} and D.case_plans("decmega0")[0]["rowconv"]
    assert {f[0] for f in _forms("g33_taps")} == {"separate"}
    # 5. program cache: 13 distinct (active count, frames) pairs, then the first again - more than the 12 entries
    steps = [(len(s), T) for s, T in D.RUNS["cache"]["steps"]]
    assert len(set(steps[:13])) == 13 and steps[13] == steps[0] and all(f[0] != "separate" for f in _forms("cache"))
    # 6. contour runs in each form
    assert tiles("c5t4", L, 2, 8)
    # a MEGA_GRID above the CU count is clamped; the default grid of 128 is not
    assert D.plan(68, 65, 4, "limb", dev_plan="MEGA_GRID=256", num_cu=128)["groups"] == 16 and D.plan(68, 65, 4, "limb", num_cu=64)["groups"] == 16


def test_runs_are_what_they_claim():
    """Slot lists are non-identity permutations inside a larger max_slots (the fixed-plan pair fills its set by design), neighbouring
    call rows never share a voice, every slot of a run has its own code seed, and the fixed-plan pair are slots of `fp33`."""
    for name, r in D.RUNS.items():
        n = len(r["slots"])
        assert len(set(r["slots"])) == n and r["slots"] != list(range(n)) and max(r["slots"]) < r["max_slots"], name
        assert n < r["max_slots"] or name in ("fp33", "fp2"), name
        seeds = [D.slot_seed(r, s) for s in r["slots"]]
        assert len(set(seeds)) == n, name
        if name in D.PIPE_RUNS:      # (the Emformer's codes, recorded: one row per call row, the run's frames)
            assert D.pipe_codes(name).shape == (n, sum(T for _, T in r["steps"]))
        for slots, T in r["steps"]:
            assert T <= r["max_frames"] and all(r["voice"][a] != r["voice"][b] for a, b in zip(slots, slots[1:])), name
    a, b = D.RUNS["fp33"], D.RUNS["fp2"]
    assert all(D.slot_seed(a, s) == D.slot_seed(b, s) and a["voice"][s] == b["voice"][s] for s in b["steps"][0][0])


# ------------------------------------------------------------------------------------------------------------ yardsticks, band, cap
@pytest.mark.parametrize("name", list(D.RUNS))
def test_bounds_follow_the_oracle(name):
    """The recorded ORACLE_FP32 figures are what the fp32 oracle gives against the float64 reference on the run's inputs: each recorded
    rms within a factor 1.25 of the recomputed one, each recorded max within a factor 2 (the rule of tests/test_style_ref_cpu.py).  The
    clean oracle passes the bounds; its bins are the float64 law's on every safe row."""
    got, want = _oracle_run(name)
    y = D.yardstick(got, want)
    print()
    for t in D.TAPS:
        rec = g.ORACLE_FP32[name][t]
        print(f"[decoder-vs-f64] {name} {t:18s}: rms {y[t][0]:.3e} max {y[t][1]:.3e}   recorded {rec[0]:.3e} {rec[1]:.3e}")
        assert rec[0] / 1.25 <= y[t][0] <= rec[0] * 1.25, (name, t, y[t], rec)
        assert rec[1] / 2 <= y[t][1] <= rec[1] * 2, (name, t, y[t], rec)
    assert D.judge_steps(got, want, g.BOUNDS[name], D.TAPS)[0]
    for a, b in zip(got, want):
        assert (a["bins"][~b["unsafe"]] == b["bins"][~b["unsafe"]]).all(), name


def test_bounds_follow_the_rule():
    g.test_bounds_follow_the_rule()


def test_band():
    """A band is 16 x the largest difference of its quantity between the fp32 oracle and float64 over all runs: recomputed, the
    recorded figures within a factor 1.25."""
    mel, d0 = 0.0, 0.0
    for name in D.RUNS:
        for a, b in zip(*_oracle_run(name)):
            m32, m64 = D.mel_scale32(a["f0_denorm_pred"]).double().numpy(), b["mel_value"]
            inside = (m32 > 1) & (m32 < 255) & (m64 > 1) & (m64 < 255)
            if inside.any() and not D.RUNS[name]["contour"]:
                mel = max(mel, float(np.abs(m32 - m64)[inside].max()))
            d0 = max(d0, float(np.abs(a["d0"] - b["d0"]).max()))
    print(f"[decoder-vs-f64] largest |mel-scale value 32 - 64| {mel:.3e} (recorded {D.MAX_MEL_ERR:.3e}), |d0 32 - 64| {d0:.3e} (recorded {D.MAX_D0_ERR:.3e})")
    assert (D.BAND_MEL, D.BAND_D0) == (16 * D.MAX_MEL_ERR, 16 * D.MAX_D0_ERR)
    assert D.MAX_MEL_ERR / 1.25 <= mel <= D.MAX_MEL_ERR * 1.25 and D.MAX_D0_ERR / 1.25 <= d0 <= D.MAX_D0_ERR * 1.25


def test_rows_left_out_are_capped_with_the_reference_alone():
    """With the float64 reference's own bins at most 2 % of a run's rows sit behind an unsafe row; the seed table is what find_seeds
    gives; keep_rows leaves out a slot's rows from its first unsafe row to its reset and nothing else."""
    assert D.find_seeds() == D.SEEDS
    for name, run in D.RUNS.items():
        ref = D.run_reference(run, D.voices())
        _, lost, rows = D.keep_rows(run, ref)
        print(f"[decoder-vs-f64] {name}: {lost} of {rows} rows left out")
        assert rows == sum(D.run_frames(run).values()) and lost <= D.MAX_LEFT_OUT * rows, (name, lost, rows)
    run = D.RUNS["long"]
    s1, s0 = run["slots"][1], run["slots"][0]
    fake = [dict(slots=list(sl), T=T, unsafe=np.zeros((len(sl), T), bool)) for sl, T in run["steps"]]
    fake[3]["unsafe"][1, 2] = True      # slot 1, step 3, row 2
    keep, lost, rows = D.keep_rows(run, fake)
    assert [k[s1] for k in keep[1:]] == [4, 4, 2, 0, 0, 0, 0, 4, 4, 4, 4, 4, 4] and all(k[s0] == 4 for k in keep) and lost == 2 + 4 * 4


# ------------------------------------------------------------------------------------------------------------ the bounds discriminate
MUT_RUN = "g33"


class _Over:
    def __init__(self, base, **over):
        self._base, self._over = base, over

    def __getattr__(self, name):
        return self._over[name] if name in self._over else getattr(self._base, name)


def _swap_codes():
    """Rows 1 and 2 of the first tile (two slots, two voices) swap their codes in every step."""
    def codes(k, c):
        c[[1, 2]] = c[[2, 1]]
        return c
    return dict(hooks=dict(codes=codes))


def _ring_off_by_one():
    """The oldest history row of the first decoder conv (k = 5: four rows of history) of one slot reads zero from the second step on."""
    slot = D.RUNS[MUT_RUN]["slots"][5]

    def state(k, states):
        if k >= 1:
            states[slot]["decoder.res_blocks.0.blocks.0.2"][:, :, 0] = 0.0
    return dict(hooks=dict(state=state))


def _neighbours_style():
    """One slot adds the style vector of the next call row's voice (its tokens stay its own)."""
    slot = D.RUNS[MUT_RUN]["slots"][6]
    return dict(hooks=dict(style=lambda s, v: (v + 1) % D.NV if s == slot else v))


def _bf16_tap():
    """Tap 0 of one decoder conv (block 2, first layer) rounded to bf16."""
    sd = dict(P.model()[2])
    w = sd["decoder.res_blocks.2.blocks.0.2.weight"].clone()
    w[:, :, 0] = w[:, :, 0].bfloat16().float()
    sd["decoder.res_blocks.2.blocks.0.2.weight"] = w
    return dict(sd32=sd)


def _bin_off_by_one():
    """One row of one slot in the second step embeds the neighbouring bin (the reported bins stay the law's)."""
    def bins(k, rows, b):
        if k == 1 and 9 in rows:
            j = rows.index(9)
            b[j, 2] = b[j, 2] + 1 if b[j, 2] < 255 else 254
        return b
    return dict(hooks=dict(bins=bins))


def _ln_eps(value=1e-4):
    """Every LayerNorm with eps 1e-4 instead of 1e-5.  (What the bounds do not resolve: eps 1e-6 moves mel_out by 1.9e-6 rms on this
    run, under the bound of 3.9e-6 - a shift of 4.5e-6 / variance in front of each LayerNorm is a few fp32 roundings, which is what
    the factor 8 allows; test_a_smaller_eps_is_not_resolved prints the figure.)"""
    def layer_norm(x, shape, w=None, b=None, eps=1e-5):
        return F.layer_norm(x, shape, w, b, value)

    def layer_norm_c(x, w, b, eps=1e-5):
        return F.layer_norm(x.transpose(1, -1), (x.shape[1],), w, b, value).transpose(1, -1)

    @contextlib.contextmanager
    def patch():
        old = (oconan.F, oconan.layer_norm_c)
        try:
            oconan.F, oconan.layer_norm_c = _Over(F, layer_norm=layer_norm), layer_norm_c
            yield
        finally:
            oconan.F, oconan.layer_norm_c = old
    return dict(patch=patch)


MUTATIONS = {"two_slots_swap_codes": _swap_codes, "ring_off_by_one": _ring_off_by_one, "neighbours_style_vector": _neighbours_style,
             "one_tap_bf16": _bf16_tap, "bin_off_by_one": _bin_off_by_one, "layernorm_eps": _ln_eps}


@pytest.mark.parametrize("change", list(MUTATIONS))
def test_bounds_catch_a_deliberate_change(change):
    """judge() with the GPU test's bounds fails the fp32 oracle with one deliberate change on `g33` (the unmodified oracle passes:
    test_bounds_follow_the_oracle) - on mel_out alone, which is all a persistent launch is judged on - and only the slots the change
    touches fail.  The change is undone afterwards."""
    run = D.RUNS[MUT_RUN]
    before = (oconan.F, oconan.layer_norm_c)
    got, want = D.oracle_run(run, **MUTATIONS[change]())
    assert (oconan.F, oconan.layer_norm_c) == before
    ok, worst, bad = D.judge_steps(got, want, g.BOUNDS[MUT_RUN], ("mel_out",))
    b = g.BOUNDS[MUT_RUN]["mel_out"]
    print(f"\n[decoder-vs-f64] {change}: mel_out rms {worst['mel_out'][0]:.3e} (bound {b[0]:.3e}), max {worst['mel_out'][1]:.3e} (bound {b[1]:.3e}); failed (step, slot): {bad[:8]}")
    assert not ok
    slots = run["slots"]
    touched = {"two_slots_swap_codes": {slots[1], slots[2]}, "ring_off_by_one": {slots[5]}, "neighbours_style_vector": {slots[6]}, "bin_off_by_one": {slots[9]}}.get(change)
    if touched:
        assert {s for _, s in bad} == touched, (change, bad)
    if change == "ring_off_by_one":
        assert {k for k, _ in bad} <= {1, 2} and 1 in {k for k, _ in bad}
    if change == "bin_off_by_one":
        assert min(k for k, _ in bad) == 1


def test_a_smaller_eps_is_not_resolved():
    """The limit of the rule, printed: LayerNorm eps 1e-6 instead of 1e-5 stays inside the mel_out bounds (it is the size of the fp32
    oracle's own error), though it moves every slot."""
    run = D.RUNS[MUT_RUN]
    clean, _ = _oracle_run(MUT_RUN)
    got, want = D.oracle_run(run, **_ln_eps(1e-6))
    ok, worst, bad = D.judge_steps(got, want, g.BOUNDS[MUT_RUN], ("mel_out",))
    b = g.BOUNDS[MUT_RUN]["mel_out"]
    print(f"\n[decoder-vs-f64] layernorm eps 1e-6: mel_out rms {worst['mel_out'][0]:.3e} (bound {b[0]:.3e}), max {worst['mel_out'][1]:.3e} (bound {b[1]:.3e}); failed {len(bad)}")
    assert not torch.equal(got[0]["mel_out"], clean[0]["mel_out"])
    assert worst["mel_out"][0] > 2 * D.yardstick(clean, _oracle_run(MUT_RUN)[1])["mel_out"][0]
