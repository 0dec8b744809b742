"""conv_tall (csrc/conv_tall.hip), the split-K limb GEMM that runs ups.0 / ups.1 of every limb stream-set big enough for it, against
FLOAT64 at the shapes where it can go wrong: both sides of its plan thresholds, ragged last tiles, tiles that start and end inside a
slot, one row per slot, sparse and unordered active lists, slots reset mid-run, mixed frame counts, and the fixed-plan launches whose
split factor comes from max_slots while their tile count comes from the live slot count.

Every active slot is checked on its own (a wrong slot, row or K slice gives errors near 1 in some slot's rows; rounding gives ~1e-7),
over enough steps that every input ring has wrapped at least twice, and every step asserts how many conv_tall launches it made, by
a restatement of conv_tall_plan's predicate (tall_launches): a change of the plan fails here instead of silently moving these
shapes to another kernel.  The f32 stream-sets run the same cases through conv_mfma (0 launches asserted) at twice the bounds
(F32_RMS_BOUND, F32_MAX_BOUND: its longer fp32 sums round more): still four orders of magnitude below a wrong row."""
import math

import numpy as np
import pytest
import torch

from conan_amd import _lib, configs, synth
from tests.conftest import kernels_of, load_golden
from tests.test_gpu_arith import _fold
from tests.vocoder_ref import ref_upsampler, ring_rows, slot_errors, steps_to_wrap_twice  # noqa: F401  (the float64 helpers, shared with test_gpu_vocoder_f64.py)

gpu = pytest.mark.gpu

TALL = "cnk::conv_tall_kernel"
# the shipped vocoder's first two upsamplers (configs.HIFIGAN_16K320_SHUFFLE): (Cin, taps, Cout before the pixel shuffle, input rows
# per frame)
UPS = ((512, 16, 2048, 1), (256, 10, 640, 8))
RMS_BOUND, MAX_BOUND = 1e-6, 3e-5       # per slot: relative rms error; largest |error| / the slot's channel rms
# The f32 stream-sets' yardstick (conv_mfma) at twice these: its ups.0 plans from 256 rows on sum K = 8192 products in fewer, longer
# fp32 partial sums - measured at 128 slots 1.63e-6 relative rms in every slot and one sample at 3.0e-5 of its channel rms (rounding:
# a wrong row or slice is ~1).  2e-6 is test_gpu_arith's fp32-accuracy bound, 2x its slack for single samples.
F32_RMS_BOUND, F32_MAX_BOUND = 2e-6, 6e-5


def tall_launches(n, frames, num_cu, plan_n=0, max_t=32):
    """conv_tall launches of one vocoder step of a limb stream-set: n active slots, `frames` mel frames, plan_n = max_slots for
    STREAMS_FIXED_PLAN stream-sets.  Restates conv_tall_plan (conv_tall.hip:326-338): rows per slot T <= max_T (streams.hip:66,
    default 32), Mp = plan rows >= one 128-row tile, NB = (Cin / 32) x taps >= 64 blocks, and (128 x 128 tiles of the plan rows)
    x min(16, NB / 8) >= CUs.  (The slab / counter limits of :343 never bind for this vocoder: tiles x S <= CUs.)"""
    count = 0
    for cin, k, cout, rate in UPS:
        t = frames * rate
        nb = cin // 32 * k
        mp = (plan_n or n) * t
        if t > max_t or mp < 128 or nb < 64:
            continue
        if math.ceil(mp / 128) * (cout // 128) * min(16, nb // 8) >= num_cu:
            count += 1
    return count


def test_ref_upsampler_matches_the_oracle_streamed():
    """The float64 helper against oracle.hifigan._cconv + pixel_shuffle_1d (pinned to the reference goldens by
    test_oracle_golden.py), two streaming steps concatenated (the oracle carries its causal history between them), at an ups.1-like
    geometry (10 taps, shuffle 5) with small widths; and the weight fold of test_gpu_arith._fold against the oracle's weight-norm."""
    from oracle import hifigan as ohifi
    rng = np.random.default_rng(5)
    cin, cout, k, r = 12, 20, 10, 5
    sd = {"u.weight_v": rng.standard_normal((cout, cin, k)).astype(np.float32),
          "u.weight_g": rng.uniform(0.5, 2.0, (cout, 1, 1)).astype(np.float32),
          "u.bias": rng.standard_normal(cout).astype(np.float32)}
    f = _fold(sd)
    w, b = torch.from_numpy(f["u.weight"]), torch.from_numpy(f["u.bias"])
    x = torch.from_numpy(rng.standard_normal((3, 13, cin)))             # [n, rows, Cin]: steps of 6 and 7 rows
    got = ref_upsampler(x, w, b, r)
    assert got.dtype == torch.float64 and got.shape == (3, 13 * r, cout // r)
    for sdo, tol in (({"u.weight": w.double(), "u.bias": b.double()}, 1e-12),
                     ({k_: torch.from_numpy(v).double() for k_, v in sd.items()}, 1e-6)):
        st = {}
        ys = [ohifi._cconv(sdo, "u", x[:, p:q].transpose(1, 2), 1, st) for p, q in ((0, 6), (6, 13))]
        want = ohifi.pixel_shuffle_1d(torch.cat(ys, 2), r).transpose(1, 2)
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=0, atol=tol * float(want.abs().max()))
    # the helper is causal: the first rows do not see later input
    x2 = x.clone()
    x2[:, 6:] += 1.0
    assert torch.equal(ref_upsampler(x2, w, b, r)[:, :6 * r], got[:, :6 * r])


# ------------------------------------------------------------------------------------------------------------ the sweep
def _uniform(n, frames, max_frames=4):
    return {"slots": n, "max_frames": max_frames, "steps": [(list(range(n)), frames, [])] * steps_to_wrap_twice(frames, max_frames)}


def _sparse():
    """64 slots, a random subset in random order per step (sizes on both sides of both thresholds), slots reset at two steps."""
    rng = np.random.default_rng(3)
    sizes = [40, 33, 21, 64, 50, 31, 20, 47]
    steps = []
    for s in range(32):
        ids = [int(i) for i in rng.permutation(64)[:sizes[s % len(sizes)]]]
        steps.append((ids, 4, [3, 17, 50] if s == 9 else ([17, 60, 61] if s == 18 else [])))
    return {"slots": 64, "max_frames": 4, "steps": steps}


def _mixed():
    """64 slots, the frame count changes from step to step: ups.0's 1-frame launches (64 rows) are not conv_tall's, so a launch reads
    history rows that another kernel, or a launch with another T, wrote."""
    return {"slots": 64, "max_frames": 4, "steps": [(list(range(64)), f, []) for f in [4, 3, 1, 2, 3, 4, 2, 1] * 4]}


CASES = {
    "n20_f4": lambda: _uniform(20, 4), "n21_f4": lambda: _uniform(21, 4), "n31_f4": lambda: _uniform(31, 4),
    "n32_f4": lambda: _uniform(32, 4), "n33_f4": lambda: _uniform(33, 4), "n64_f4": lambda: _uniform(64, 4),
    "n128_f4": lambda: _uniform(128, 4),
    "n43_f3": lambda: _uniform(43, 3), "n64_f3": lambda: _uniform(64, 3),
    "n128_f1": lambda: _uniform(128, 1, max_frames=1),
    "n41_f2": lambda: _uniform(41, 2, max_frames=2), "n64_f2": lambda: _uniform(64, 2, max_frames=2),
    "n128_f2": lambda: _uniform(128, 2, max_frames=2),
    "sparse64_resets": _sparse, "mixed64_frames": _mixed,
}
# the plan as a table (256 CUs): both sides of ups.1's switch (20 | 21 slots of 4 frames) and of ups.0's (31 | 32), and 2-frame
# steps (configs[4]'s 40 ms chunk: ups.1 from 41 slots, ups.0 from 64); tall_launches must agree with it on this device
PLAN_TABLE = {(20, 4): 0, (21, 4): 1, (31, 4): 1, (32, 4): 2, (33, 4): 2, (64, 4): 2, (128, 4): 2, (43, 3): 2, (64, 3): 2,
              (128, 1): 2, (40, 2): 0, (41, 2): 1, (63, 2): 1, (64, 2): 2, (128, 2): 2, (64, 1): 0}


@pytest.fixture(scope="module")
def voc():
    """A vocoder context with the full synthetic checkpoint; the folded fp32 weights and biases of ups.0 / ups.1 (what both the
    library and the float64 reference multiply)."""
    from conan_amd.runtime import Context
    vhp = configs.hifigan_hparams()
    sd = synth.hifigan_state_dict(vhp, 0)
    ctx = Context(None, vhp, 0, False, False, True)
    ctx.load_state_dict("hifigan", sd)
    ctx.finalize()
    f = _fold(sd)
    ups = [(torch.from_numpy(f[f"ups.{i}.conv.conv.weight"]).cuda(), torch.from_numpy(f[f"ups.{i}.conv.conv.bias"]).cuda(),
            vhp["upsample_rates"][i]) for i in range(2)]
    yield ctx, ups
    ctx.close()


def _num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


@gpu
def test_plan_table_matches_the_helper():
    """tall_launches on this device equals the stated table: the switch points the sweep below straddles are where they are said
    to be (a device with another CU count skips rather than retargets)."""
    cu = _num_cu()
    if cu != 256:
        pytest.skip(f"the table is for 256 CUs, this device has {cu}")
    assert {key: tall_launches(*key, cu) for key in PLAN_TABLE} == PLAN_TABLE
    assert [n for n in range(1, 129) if tall_launches(n, 4, cu) >= 1][0] == 21
    assert [n for n in range(1, 129) if tall_launches(n, 4, cu) == 2][0] == 32


def _run_schedule(ctx, arith, case, flags=0):
    """Drive hifigan_step_taps through the case's steps; every step's conv_tall launches counted.  -> per slot, a list of runs (one
    per reset), each {"cpre", "so0", "ups0", "ups1"} concatenated over the run's steps (GPU tensors), and [(n, frames, launches)]."""
    S, steps = case["slots"], case["steps"]
    st = ctx.streams(S, max_frames=case["max_frames"], max_ref_frames=16, arith=arith, flags=flags)
    assert st.arith == arith
    total = sum(f for _, f, _ in steps)
    mels = torch.from_numpy(synth.mel(total, 21, S)).cuda()
    cursor = [0] * S
    runs = [[[]] for _ in range(S)]
    st.reset(list(range(S)))
    counts = []
    for ids, frames, resets in steps:
        if resets:
            st.reset(resets)
            for s in resets:
                if runs[s][-1]:
                    runs[s].append([])
        mel = torch.stack([mels[s, cursor[s]:cursor[s] + frames] for s in ids])
        for s in ids:
            cursor[s] += frames
        out = {}
        names = kernels_of(st, lambda: out.setdefault("t", st.hifigan_step_taps(ids, mel, stage_out=True)))
        counts.append((len(ids), frames, names.get(TALL, 0)))
        _, _, cpre, ups, outs = out["t"]
        rec = (cpre, outs[0], ups[0], ups[1])
        for j, s in enumerate(ids):
            runs[s][-1].append((rec, j))
    torch.cuda.synchronize()
    st.close()
    keys = ("cpre", "so0", "ups0", "ups1")
    res = []
    for s in range(S):
        res.append([{k: torch.cat([rec[q][j] for rec, j in run]) for q, k in enumerate(keys)} for run in runs[s] if run])
    return res, counts


def _check_case(voc, arith, name):
    ctx, ups = voc
    case = CASES[name]()
    runs, counts = _run_schedule(ctx, arith, case)
    cu = _num_cu()
    for n, frames, got in counts:
        assert got == (tall_launches(n, frames, cu) if arith == "limb" else 0), (name, arith, n, frames, got)
    # group the runs by length (every slot of a uniform case is one group) and evaluate each group in float64 on the GPU
    groups = {}
    for s, rs in enumerate(runs):
        for ri, r in enumerate(rs):
            groups.setdefault(r["cpre"].shape[0], []).append((s, ri, r))
    rms_bound, max_bound = (RMS_BOUND, MAX_BOUND) if arith == "limb" else (F32_RMS_BOUND, F32_MAX_BOUND)
    stats, bad = {}, []
    for members in groups.values():
        for u, (xk, yk) in enumerate((("cpre", "ups0"), ("so0", "ups1"))):
            w, b, rate = ups[u]
            x = torch.stack([r[xk] for _, _, r in members])
            got = torch.stack([r[yk] for _, _, r in members])
            want = ref_upsampler(x, w, b, rate)
            assert want.shape == got.shape, (want.shape, got.shape)
            rms, mx, fin = slot_errors(got, want)
            for i, (s, ri, _) in enumerate(members):
                stats.setdefault(f"ups.{u}", []).append((float(rms[i]), float(mx[i]), s))
                if not (bool(fin[i]) and rms[i] <= rms_bound and mx[i] <= max_bound):
                    bad.append((f"ups.{u}", "slot", s, "run", ri, "finite", bool(fin[i]), "rms", float(rms[i]), "max", float(mx[i])))
    launches = sorted({(n, f, c) for n, f, c in counts})
    print(f"\n[conv_tall-vs-f64] {name} {arith}: {len(counts)} steps, (slots, frames, conv_tall launches) {launches}")
    for key, v in sorted(stats.items()):
        r = sorted(v)
        m = max(v, key=lambda e: e[1])
        print(f"  {key}: {len(v)} slot runs, rel rms median {r[len(r) // 2][0]:.3e} worst {r[-1][0]:.3e} (slot {r[-1][2]}), "
              f"max/ch-rms worst {m[1]:.3e} (slot {m[2]})")
    assert not bad, (name, arith, rms_bound, max_bound, bad[:8])


@gpu
@pytest.mark.parametrize("arith", ["limb", "f32"])
@pytest.mark.parametrize("name", list(CASES))
def test_upsamplers_against_float64(voc, name, arith):
    """ups.0 / ups.1 of every active slot against float64 (ref_upsampler on the tensor the launch read), per slot; the conv_tall
    launches of every step as tall_launches says (0 in f32 stream-sets: conv_mfma)."""
    _check_case(voc, arith, name)


# ------------------------------------------------------------------------------------------------------------ stray writes
@gpu
def test_fixed_plan_other_slots_leave_an_idle_slot_untouched(voc):
    """A 64-slot STREAMS_FIXED_PLAN limb stream-set (its bits do not depend on the active set): slot K alone for 3 steps, then
    steps of the other 63 slots with ragged and mid-slot shapes while K is idle, then K alone again.  K's audio and ups taps are
    bit-identical to an uninterrupted run of K alone; the fixed-plan launches with 1, 5 and 33 active slots (plan_n = 64 != n; one
    4-row ups.0 tile for 1 slot) took conv_tall for both upsamplers."""
    ctx, _ = voc
    S, K = 64, 37
    cu = _num_cu()
    mels = torch.from_numpy(synth.mel(64, 33, S)).cuda()
    mk = mels[K:K + 1]

    def k_steps(st, p0, n):
        out = []
        for p in range(p0, p0 + 4 * n, 4):
            wav, _, _, ups = st.hifigan_step_taps([K], mk[:, p:p + 4].contiguous())
            out.append([wav] + ups)
        return out
    a = ctx.streams(S, max_frames=4, max_ref_frames=16, arith="limb", flags=_lib.STREAMS_FIXED_PLAN)
    b = ctx.streams(S, max_frames=4, max_ref_frames=16, arith="limb", flags=_lib.STREAMS_FIXED_PLAN)
    for st in (a, b):
        st.reset(list(range(S)))
    want = k_steps(b, 0, 9)
    got = k_steps(a, 0, 2)
    n1 = kernels_of(a, lambda: got.extend(k_steps(a, 8, 1)))
    assert n1.get(TALL) == tall_launches(1, 4, cu, plan_n=S) == 2, sorted(n1.items())
    others = [s for s in range(S) if s != K]
    rng = np.random.default_rng(8)
    seen = {}
    for cnt, frames in [(63, 4), (33, 3), (5, 1), (20, 2), (33, 4), (1, 4), (43, 3), (31, 4), (21, 4), (5, 4), (63, 1), (63, 3)]:
        ids = [others[int(i)] for i in rng.permutation(len(others))[:cnt]]
        x = mels[ids][:, :frames].contiguous()
        names = kernels_of(a, lambda: a.hifigan_step(ids, x))
        assert names.get(TALL, 0) == tall_launches(cnt, frames, cu, plan_n=S), (cnt, frames, sorted(names.items()))
        seen[(cnt, frames)] = names.get(TALL, 0)
    assert seen[(5, 4)] == 2 and seen[(33, 4)] == 2 and seen[(33, 3)] == 2, seen
    got += k_steps(a, 12, 6)
    torch.cuda.synchronize()
    for step, (g, w) in enumerate(zip(got, want)):
        for i, (x, y) in enumerate(zip(g, w)):
            assert torch.equal(x, y), ("step", step, "wav" if i == 0 else f"ups.{i - 1}", float((x - y).abs().max()))
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------------------ reference goldens
@gpu
@pytest.mark.parametrize("arith", ["limb", "f32"])
@pytest.mark.parametrize("S,K", [(33, 32), (64, 45)])
def test_vocoder_stage_taps_golden_through_conv_tall(voc, S, K, arith):
    """tests/golden/hifigan_full.npz (forward hooks on the imported reference: ups.{i}_12, wav_12) through slot K of an S-slot
    stream-set with synthetic mels in the other slots, 4 frames per step, at test_vocoder_stage_taps_match_reference_goldens'
    tolerances.  At 33 slots K = 32 is ups.0's ragged second tile (4 rows); in limb stream-sets the taps call launched conv_tall for
    ups.0 and ups.1."""
    ctx, _ = voc
    g = load_golden("hifigan_full.npz")
    mels = torch.from_numpy(synth.mel(12, 40, S)).cuda()
    mels[K] = torch.from_numpy(g["mel_12"][0].T).cuda()
    st = ctx.streams(S, max_frames=4, max_ref_frames=16, arith=arith)
    assert st.arith == arith
    ids = list(range(S))
    st.reset(ids)
    parts, out = [], {}
    names = kernels_of(st, lambda: out.setdefault("t", st.hifigan_step_taps(ids, mels[:, :4].contiguous())))
    assert names.get(TALL, 0) == (2 if arith == "limb" else 0), sorted(names.items())
    parts.append(out["t"])
    parts += [st.hifigan_step_taps(ids, mels[:, p:p + 4].contiguous()) for p in (4, 8)]
    wav = torch.cat([p[0][K] for p in parts]).cpu().numpy()
    np.testing.assert_allclose(wav, g["wav_12"], atol=1e-4, rtol=0)
    for i in range(4):
        up = torch.cat([p[3][i][K] for p in parts]).cpu().numpy()
        ref = g[f"ups.{i}_12"].T
        assert up.shape == ref.shape
        np.testing.assert_allclose(up, ref, atol=1e-4 * max(1.0, np.abs(ref).max()), rtol=0)
    st.close()
