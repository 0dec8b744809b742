"""The Emformer step (emformer_step: the content codes everything downstream is conditioned on) against FLOAT64, per slot, across
its launch forms: the fused one-launch step (emformer_fused.hip) at forced cluster sizes 1 / 2 / 4 / 8 and at the cluster sizes the
library chooses itself - alone on the device and beside another stream-set, at stream counts on both sides of every switch, up to
more workgroups than CUs -, the other configurations (2-row segments, no right context, a memory bank with clamp and with tanh up to
the largest bank the fused step accepts), the per-op plan (EMF_UNFUSED=1) at row counts on both sides of every kernel switch of
conan_streams::conv, and the per-op plan where the fused step refuses the shape (banks of 8 and 9 entries: 64 and 65 keys, the last
lane and the second key register set of emf_attn_kernel).

An Emformer-only context with the full six-layer synthetic checkpoint; every slot has its own inputs (synth.mel(T, seed + slot)).
Per step `out`, `logits` and `codes` of every active slot are recorded, concatenated per slot-run (a slot from a reset to its next
reset) and judged by tests/emformer_ref.judge against the float64 reference (tests/emformer_ref.EmformerRef, which carries every
stream's own state and runs beside the schedule on the device): relative rms, largest error over the run's rms, and the codes
wherever the float64 margin allows.  Every schedule runs until each K/V ring has wrapped at least twice, the slot-runs judged are
counted against the schedule's, and every step's launches are asserted against a restatement of the plan."""
import gc
from collections import Counter

import pytest
import torch

from conan_amd import configs, synth
from tests import emformer_ref as er
from tests.conftest import kernels_of
from tests.test_gpu_vocoder_f64 import MAX_FACTOR, RMS_FACTOR

gpu = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------------------ configurations
CONFIGS = {
    "seg4_rc2": {},                                                                   # the shipped configuration
    "seg2_rc2": {"chunk_size": 40},
    "rc0": {"right_context": 0},
    "m4": {"emformer_max_memory_size": 4},                                            # clamp
    "m6_tanh": {"emformer_max_memory_size": 6, "emformer_tanh_on_mem": True},         # the largest bank the fused step accepts: 62 of 64 keys
    "m8": {"emformer_max_memory_size": 8},                                            # 64 keys: the last lane of emf_attn_kernel
    "m9": {"emformer_max_memory_size": 9},                                            # 65 keys: its second key per lane
}
LEFT_CONTEXT, HEADS, FFN, D_IN = 50, 8, 2048, 80       # modules/Emformer/emformer.py:14-22 / _lib.make_cfg


def hparams(config):
    return dict(configs.conan_hparams(), **CONFIGS[config])


# ------------------------------------------------------------------------------------------------------------ bounds
# Per slot-run and tensor: relative rms error; largest |error| / the run's rms.  Neither comes from the kernels:
#   rms bound = RMS_FACTOR (8) x the fp32 ORACLE's rms,   max bound = MAX_FACTOR (16) x the fp32 oracle's max
# where the oracle's figures are oracle/emformer.py (emformer_infer + logits_and_codes, fp32, on the CPU) against the float64 reference
# on the same inputs: 16 lock-step streams x 120 frames from reset, synth.mel seed 1234, synthetic checkpoint seed 0, the worst
# stream (oracle_yardstick below; tests/test_emformer_ref_cpu.py recomputes them).  The factors are the project's own
# (tests/test_gpu_vocoder_f64.py) for the same reasons: K-ordered MFMA accumulation and the 256-wide hidden-chunk order of the
# feed-forward differ from torch's blocked sums, six layers chain through LayerNorm; 8 x 4e-7 still sits well below a product formed
# from two bf16 limbs instead of three (2^-16 = 1.5e-5).  Outputs and logits have rms 1.0.
# configuration: {tensor: (oracle fp32 rms, oracle fp32 max)} as measured
ORACLE_FP32 = {
    "seg4_rc2": {"out": (3.909e-7, 2.022e-6), "logits": (4.073e-7, 2.220e-6)},
    "seg2_rc2": {"out": (4.021e-7, 2.172e-6), "logits": (4.278e-7, 2.285e-6)},
    "rc0": {"out": (3.839e-7, 2.013e-6), "logits": (4.003e-7, 2.146e-6)},
    "m4": {"out": (3.821e-7, 2.033e-6), "logits": (4.017e-7, 2.414e-6)},
    "m6_tanh": {"out": (3.823e-7, 2.143e-6), "logits": (3.960e-7, 2.085e-6)},
    "m8": {"out": (3.843e-7, 2.033e-6), "logits": (3.982e-7, 2.419e-6)},
    "m9": {"out": (3.869e-7, 2.033e-6), "logits": (3.996e-7, 2.419e-6)},
}
BOUNDS = {c: {t: (RMS_FACTOR * r, MAX_FACTOR * m) for t, (r, m) in v.items()} for c, v in ORACLE_FP32.items()}
YARDSTICK_STREAMS, YARDSTICK_FRAMES, YARDSTICK_SEED = 16, 120, 1234
MAX_EXCLUDED = 0.01          # at most 1 % of a schedule's frames may be left out of the code comparison for small margins


def oracle_run(config, mutate=None, streams=YARDSTICK_STREAMS, frames=YARDSTICK_FRAMES, seed=YARDSTICK_SEED):
    """The fp32 oracle and the float64 reference over the yardstick run, on the CPU: `streams` lock-step streams x `frames` frames
    from reset.  mutate: a context manager entered around the ORACLE's steps only (tests/test_emformer_ref_cpu.py's deliberate
    changes).  -> (got = (out, logits, codes) fp32, want = (out, logits) float64), [streams, frames, .]"""
    import contextlib
    from oracle import emformer as oemf
    from oracle.common import to_torch_sd
    hp = hparams(config)
    sd, cfg = to_torch_sd(synth.emformer_state_dict(hp, 0)), oemf.EmformerCfg(hp)
    mel = torch.from_numpy(synth.mel(frames, seed, streams))
    ref = er.EmformerRef(sd, cfg, streams)
    state, rec = None, [[] for _ in range(5)]
    for _, _, chunk in oemf.chunk_iter(mel, cfg.segment_length, cfg.right_context_length):
        with (mutate() if mutate else contextlib.nullcontext()):
            o, _, state = oemf.emformer_infer(sd, cfg, chunk, torch.full((streams,), chunk.shape[1]), state)
            lg, cd = oemf.logits_and_codes(sd, o)
        ro, rl, _ = ref.step(range(streams), chunk)
        assert o.dtype == lg.dtype == torch.float32 and ro.dtype == rl.dtype == torch.float64
        for v, t in zip(rec, (o, lg, cd, ro, rl)):
            v.append(t)
    o, lg, cd, ro, rl = [torch.cat(v, 1) for v in rec]
    return (o, lg, cd), (ro, rl)


def oracle_yardstick(config):
    """{tensor: (rms, max)} of the fp32 oracle against the float64 reference over the yardstick run, the worst stream."""
    got, want = oracle_run(config)
    j = er.judge(got, want, BOUNDS[config])
    assert bool(j["finite"].all())
    return {t: (float(j["rms"][t].max()), float(j["max"][t].max())) for t in ("out", "logits")}


# ------------------------------------------------------------------------------------------------------------ the plan, restated
FUSED = "cnk::emformer_fused_kernel<5, 10>"              # streams.hip:792 (input_dim 80, head_dim 10)
EMF_MAX_CLUSTER, EMF_SHARED_CAP = 8, 64                  # kernels.h:414; streams.hip:781 (workgroups of a launch that may overlap another)
EF_ROWS = 16                                             # emformer_fused.hip:41: rows of the step's one tile
CONV_CFGS = (("cnk::conv_mfma_kernel<64, 64, 2, 2, 1, 32>", 64, 64), ("cnk::conv_mfma_kernel<32, 64, 1, 2, 2, 64>", 32, 64),
             ("cnk::conv_mfma_kernel<32, 32, 1, 1, 4, 128>", 32, 32))            # streams.hip:29 `wide`, conv_mfma.hip:782-793


def _ceil(a, b):
    return -(-a // b)


def _shape(hp):
    seg, rc, M = hp["chunk_size"] // 20, hp["right_context"], int(hp.get("emformer_max_memory_size", 0))
    return seg, rc, M


def streams_per_group(hp):
    """emformer_fused.hip:156 ef_streams_per_block: streams that share the 16-row tile (with a bank: + summary + memory-input row)."""
    seg, rc, M = _shape(hp)
    return min(EF_ROWS // (seg + rc + (2 if M > 0 else 0)), 16 // HEADS)


def fused_accepts(hp):
    """emformer_fused.hip:716-723 emformer_fused_supported, the conditions a configuration of this file can miss: the bank's
    key / value rows of a group fit one prefetch pass (G x M x D/4 <= 256), at most 64 keys."""
    seg, rc, M = _shape(hp)
    return not (M > 0 and streams_per_group(hp) * M * (D_IN // 4) > 256) and M + rc + LEFT_CONTEXT + seg <= 64


def cluster_size(n, cus, alone, forced=0, per_group=2):
    """streams.hip:761-785: workgroups per stream group of a blocking fused step.  The largest power of two <= 8 (or the forced size)
    with groups x size <= cap; cap = one workgroup per CU when the stream-set is the only one alive on the device (or the size is
    forced), else 64 workgroups."""
    groups = _ceil(n, per_group)
    cap = cus if (forced or alone) else EMF_SHARED_CAP
    cs = min(forced, EMF_MAX_CLUSTER) if forced else EMF_MAX_CLUSTER
    while cs & (cs - 1):
        cs &= cs - 1
    while cs > 1 and groups * cs > cap:
        cs >>= 1
    return cs


def pick_cfg(rows, cols, cus):
    """streams.hip:24-51 pick_cfg for one problem of more than 32 columns: the first of 64 x 64, 32 x 64, 32 x 32 tiles with a tile
    for every CU, else the 32 x 32 tiles.  (conv_tall / conv_limb never take an Emformer layer: its activations are not rings.)"""
    assert cols > 32
    for name, tm, tn in CONV_CFGS:
        if _ceil(rows, tm) * _ceil(cols, tn) >= cus:
            return name
    return CONV_CFGS[-1][0]


def per_op_layers(n, hp):
    """(rows, columns) of every conan_streams::conv launch of one per-op step (streams.hip:812-857): per layer q, kv, out_proj, ff1,
    ff2; then proj."""
    seg, rc, M = _shape(hp)
    Q = seg + rc
    QP = Q + (1 if M > 0 else 0)
    per_layer = [(n * QP, D_IN), (n * (M + Q), 2 * D_IN), (n * QP, D_IN), (n * Q, FFN), (n * Q, D_IN)]
    return per_layer * hp["emformer_layers"] + [(n * seg, hp["emformer_output_dim"])]


def per_op_kernels(n, hp, cus):
    return dict(Counter(pick_cfg(r, c, cus) for r, c in per_op_layers(n, hp)))


def per_op_switches(hp, cus, upto):
    """Stream counts n < upto with per_op_kernels(n) != per_op_kernels(n + 1)."""
    return [n for n in range(1, upto) if per_op_kernels(n, hp, cus) != per_op_kernels(n + 1, hp, cus)]


def segments_covered(values, chosen, upto):
    """Every maximal range of n in [1, upto] over which values(n) is constant holds at least one chosen n: the chosen counts lie on
    both sides of every switch."""
    start = 1
    for n in range(1, upto + 1):
        if n == upto or values(n + 1) != values(n):
            if not any(start <= c <= n for c in chosen):
                return False
            start = n + 1
    return True


# ------------------------------------------------------------------------------------------------------------ schedules
def _wrap_steps(hp):
    seg = hp["chunk_size"] // 20
    return er.steps_to_wrap_twice(LEFT_CONTEXT, seg) + 2


def lock_step(n, hp, restart=None):
    """n slots in lock step until the K/V rings have wrapped twice; restart = (slot, step): that slot alone is reset in front of that
    step and the schedule runs on until ITS rings have wrapped twice as well."""
    steps = [(list(range(n)), [])] * _wrap_steps(hp)
    if restart:
        slot, at = restart
        steps = [(ids, [slot] if t == at else []) for t, (ids, _) in enumerate(steps + steps[:at])]
    return {"slots": n, "steps": steps}


def five_of_six(hp):
    """5 of 6 slots in the order [4, 1, 0, 3, 2] (two streams per tile: the last tile holds one).  Slot 1 restarts alone in front of
    step 13: its tile partner has a full left context while it has none.  Then the list shrinks to 3 slots, to 1, and returns to 5
    in another order, so slots change tile and partner between steps.  The first phase lasts until the restarted slot's rings have
    wrapped twice again."""
    w = _wrap_steps(hp)
    steps = [([4, 1, 0, 3, 2], [1] if t == 13 else []) for t in range(13 + w)]
    steps += [([3, 4, 1], [])] * 5 + [([1], [])] * 3 + [([2, 3, 1, 0, 4], [])] * 6
    return {"slots": 6, "steps": steps}


def three_of_four(hp):
    """Slots [3, 0, 2] of a 4-slot set; slot 0 restarts alone in front of step 13 (a bank has saturated by then: one stream's bank
    ramps up beside a saturated one)."""
    w = _wrap_steps(hp)
    return {"slots": 4, "steps": [([3, 0, 2], [0] if t == 13 else []) for t in range(13 + w)]}


def schedule_slot_runs(case):
    """Slot-runs of a schedule (a run = a slot's active steps between two resets), counted from the schedule alone."""
    open_, total = set(), 0
    for ids, resets in case["steps"]:
        open_ -= set(resets)
        for s in ids:
            if s not in open_:
                open_.add(s)
                total += 1
    return total


# ------------------------------------------------------------------------------------------------------------ running
def _num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def emf():
    """config -> (Emformer-only context with the full synthetic checkpoint, hparams, torch state dict, oracle EmformerCfg), made on
    first use and closed at the end of the module."""
    from conan_amd.runtime import Context
    from oracle import emformer as oemf
    from oracle.common import to_torch_sd
    made = {}

    def get(config):
        if config not in made:
            hp = hparams(config)
            sd = synth.emformer_state_dict(hp, 0)
            ctx = Context(hp, None, 0, True, False, False)
            ctx.load_state_dict("emformer", sd)
            ctx.finalize()
            made[config] = (ctx, hp, to_torch_sd(sd), oemf.EmformerCfg(hp))
        return made[config]
    yield get
    for ctx, _, _, _ in made.values():
        ctx.close()


def _run_schedule(env, case, dev_plan, expect, seed, reference=True, keep_open=False):
    """Drive emformer_step through the case's steps in a stream-set of its own, every step's launches against expect(active slots).
    -> (runs: [(slot, [(step, row)])] one entry per slot-run, rec: per step (out, logits, codes) of the library, ref: per step
    (out, logits) of the float64 reference or None, the stream-set if keep_open)."""
    ctx, hp, sd, cfg = env
    seg, rc, _ = _shape(hp)
    S, steps = case["slots"], case["steps"]
    st = ctx.streams(S, max_frames=seg, max_ref_frames=16, dev_plan=dev_plan)
    mels = torch.from_numpy(synth.mel(len(steps) * seg + rc, seed, S)).cuda()          # slot s: synth.mel(T, seed + s)
    ref = er.EmformerRef(sd, cfg, S, "cuda") if reference else None
    cursor = torch.zeros(S, dtype=torch.long, device="cuda")
    ar = torch.arange(seg + rc, device="cuda")
    st.reset(list(range(S)))
    runs, open_run, rec, want = [], {}, [], []
    for step, (ids, resets) in enumerate(steps):
        if resets:
            st.reset(resets, which=1)
            if ref:
                ref.reset(resets)
            for s in resets:
                open_run.pop(s, None)
        idx = torch.tensor(ids, device="cuda")
        chunk = mels[idx[:, None], cursor[idx][:, None] + ar[None, :]]
        cursor[idx] += seg
        out = {}
        names = kernels_of(st, lambda: out.setdefault("t", st.emformer_step(ids, chunk)))
        assert names == expect(len(ids)), ("step", step, "n", len(ids), "launched", sorted(names.items()), "expected", sorted(expect(len(ids)).items()))
        rec.append(out["t"])
        if ref:
            want.append(ref.step(ids, chunk)[:2])
        for j, s in enumerate(ids):
            if s not in open_run:
                open_run[s] = []
                runs.append((s, open_run[s]))
            open_run[s].append((step, j))
    torch.cuda.synchronize()
    if not keep_open:
        st.close()
    return runs, rec, (want if reference else None), (st if keep_open else None)


def _gather(per_step, members, k):
    """[members, frames, .]: tensor k of every step of the members' (identical) step lists, rows as each member had them."""
    steps = [t for t, _ in members[0]]
    rows = torch.tensor([[j for _, j in m] for m in members], device="cuda")
    return torch.cat([per_step[t][k][rows[:, q]] for q, t in enumerate(steps)], 1)


def _judge_runs(config, label, case, runs, rec, want):
    """Every slot-run against float64; prints the figures, asserts the counts, the bounds and the share of excluded frames."""
    groups = {}                                  # runs over the same steps are judged together
    for s, run in runs:
        groups.setdefault(tuple(t for t, _ in run), []).append((s, run))
    bounds = BOUNDS[config]
    assert all(b > 0 for t in bounds.values() for b in t)
    bad, judged, frames, excluded, wrong = [], 0, 0, 0, 0
    worst = {"out": [0.0, 0.0], "logits": [0.0, 0.0]}
    for members in groups.values():
        ms = [m[1] for m in members]
        got = tuple(_gather(rec, ms, k) for k in range(3))
        ref = tuple(_gather(want, ms, k) for k in range(2))
        j = er.judge(got, ref, bounds)
        judged += len(members)
        frames += len(members) * j["frames"]
        excluded += int(j["excluded"].sum())
        wrong += int(j["wrong_codes"].sum())
        for t in ("out", "logits"):
            worst[t][0] = max(worst[t][0], float(j["rms"][t].max()))
            worst[t][1] = max(worst[t][1], float(j["max"][t].max()))
        for i, (s, run) in enumerate(members):
            if not bool(j["ok"][i]):
                bad.append(("slot", s, "from step", run[0][0], "frames", j["frames"], "finite", bool(j["finite"][i]),
                            "out rms/max", float(j["rms"]["out"][i]), float(j["max"]["out"][i]),
                            "logits rms/max", float(j["rms"]["logits"][i]), float(j["max"]["logits"][i]), "wrong codes", int(j["wrong_codes"][i])))
    print(f"\n[emformer-vs-f64] {config} {label}: {len(case['steps'])} steps, {judged} slot runs, {frames} frames; "
          f"out rms {worst['out'][0]:.3e} max {worst['out'][1]:.3e} (bounds {bounds['out'][0]:.2e} {bounds['out'][1]:.2e}); "
          f"logits rms {worst['logits'][0]:.3e} max {worst['logits'][1]:.3e} (bounds {bounds['logits'][0]:.2e} {bounds['logits'][1]:.2e}); "
          f"excluded from the code comparison {excluded} frames = {100.0 * excluded / frames:.3f} %, wrong codes {wrong}")
    # no slot and no step left out
    assert judged == schedule_slot_runs(case) and frames == sum(len(ids) for ids, _ in case["steps"]) * rec[0][0].shape[1], (judged, schedule_slot_runs(case), frames)
    assert excluded <= MAX_EXCLUDED * frames, (excluded, frames)
    assert not bad, (config, label, len(bad), bad[:6])


def _assert_wraps(case, hp):
    """Every slot of the schedule has a run of at least two K/V ring lengths of rows: its rings wrap twice (the ring length is restated
    from build_emformer - er.kv_ring_rows -, not read from the stream-set)."""
    seg = hp["chunk_size"] // 20
    need = 2 * er.kv_ring_rows(LEFT_CONTEXT, seg)
    rows, best = {}, {}
    for ids, resets in case["steps"]:
        for s in resets:
            rows[s] = 0
        for s in ids:
            rows[s] = rows.get(s, 0) + seg
            best[s] = max(best.get(s, 0), rows[s])
    assert best and min(best.values()) >= need, (need, best)


def _check(emf, config, label, case, dev_plan, expect, seed=100, bitwise_plan=None):
    env = emf(config)
    _assert_wraps(case, env[1])
    runs, rec, want, _ = _run_schedule(env, case, dev_plan, expect, seed)
    _judge_runs(config, label, case, runs, rec, want)
    if bitwise_plan is not None:      # the same inputs with one workgroup per group: emformer_fused.hip promises the same bits for every cluster size
        _, rec1, _, _ = _run_schedule(env, case, bitwise_plan, expect, seed, reference=False)
        for t, (a, b) in enumerate(zip(rec, rec1)):
            assert all(torch.equal(x, y) for x, y in zip(a, b)), ("step", t, "differs from EMF_CLUSTER=1")


def _fused(n):
    return {FUSED: 1}


# ------------------------------------------------------------------------------------------------------------ fused, forced cluster size
@gpu
@pytest.mark.parametrize("cs", [1, 2, 4, 8])
def test_fused_forced_cluster_size_against_float64(emf, cs):
    """EMF_CLUSTER = 1 / 2 / 4 / 8 in a 6-slot set over the five_of_six schedule: every slot-run against float64, not only against
    cluster size 1."""
    hp = hparams("seg4_rc2")
    assert cluster_size(5, _num_cu(), False, forced=cs) == cs        # 3 groups x 8 workgroups fit every device this runs on
    _check(emf, "seg4_rc2", f"fused EMF_CLUSTER={cs} 5-of-6", five_of_six(hp), f"EMF_CLUSTER={cs}", _fused, seed=41)


# ------------------------------------------------------------------------------------------------------------ fused, automatic cluster size
ALONE_COUNTS = {"cus/4": lambda c: c // 4, "cus/4+1": lambda c: c // 4 + 1, "cus/2+1": lambda c: c // 2 + 1, "cus": lambda c: c,
                "cus+1": lambda c: c + 1, "2cus+1": lambda c: 2 * c + 1}                # 256 CUs: 64, 65, 129, 256, 257, 513
SHARED_COUNTS = (16, 17, 33, 65)


def test_stream_counts_straddle_every_cluster_switch():
    """The restated choice at 256 CUs switches where streams.hip says (64/65, 128/129, 256/257 alone; 16/17, 32/33, 64/65 beside
    another stream-set), and the counts the sweep runs lie on both sides of every switch - for any CU count a multiple of 8."""
    sw = lambda alone: [n for n in range(1, 600) if cluster_size(n, 256, alone) != cluster_size(n + 1, 256, alone)]
    assert sw(True) == [64, 128, 256] and sw(False) == [16, 32, 64]
    assert [cluster_size(n, 256, True) for n in (64, 65, 129, 256, 257, 513)] == [8, 4, 2, 2, 1, 1]
    assert [cluster_size(n, 256, False) for n in SHARED_COUNTS] == [8, 4, 2, 1]
    for cus in (64, 104, 256, 304):
        chosen = [f(cus) for f in ALONE_COUNTS.values()]
        assert segments_covered(lambda n: cluster_size(n, cus, True), chosen, max(chosen)), (cus, chosen)
        assert segments_covered(lambda n: cluster_size(n, cus, False), SHARED_COUNTS, max(SHARED_COUNTS)), cus


@gpu
@pytest.mark.parametrize("count", list(ALONE_COUNTS))
def test_fused_automatic_cluster_size_alone_against_float64(emf, count):
    """The stream-set is the only one alive (earlier ones are closed), so a blocking step gets up to one workgroup per CU: lock-step
    streams at counts on both sides of every switch of the cluster size, every slot judged; 2 x CUs + 1 streams launch more
    workgroups than CUs, CUs streams at cluster size 2 use the whole exchange buffer (CUs / 2 clusters).  The library does not report
    the size it chose: the choice is restated (cluster_size), the counts straddle its switches, and the same inputs with
    EMF_CLUSTER=1 must give identical bits."""
    gc.collect()                      # (a stream-set another test dropped without closing it would make this one not alone)
    cus = _num_cu()
    chosen = [f(cus) for f in ALONE_COUNTS.values()]
    assert segments_covered(lambda n: cluster_size(n, cus, True), chosen, max(chosen)), (cus, chosen)
    n = ALONE_COUNTS[count](cus)
    hp = hparams("seg4_rc2")
    _check(emf, "seg4_rc2", f"fused auto alone n={n} (cluster size {cluster_size(n, cus, True)})", lock_step(n, hp), None, _fused, seed=500,
           bitwise_plan="EMF_CLUSTER=1")


@gpu
@pytest.mark.parametrize("n", SHARED_COUNTS)
def test_fused_automatic_cluster_size_not_alone_against_float64(emf, n):
    """A second, idle stream-set is alive: at most 64 workgroups, the cluster size switches at 16/17, 32/33 and 64/65 streams."""
    env = emf("seg4_rc2")
    assert segments_covered(lambda m: cluster_size(m, _num_cu(), False), SHARED_COUNTS, max(SHARED_COUNTS))
    idle = env[0].streams(1, max_frames=4, max_ref_frames=16)
    try:
        _check(emf, "seg4_rc2", f"fused auto beside an idle set n={n} (cluster size {cluster_size(n, _num_cu(), False)})", lock_step(n, env[1]), None,
               _fused, seed=700, bitwise_plan="EMF_CLUSTER=1")
    finally:
        idle.close()


# ------------------------------------------------------------------------------------------------------------ fused, other configurations
@gpu
@pytest.mark.parametrize("form", ["EMF_CLUSTER=1", "EMF_CLUSTER=8", "auto65"])
@pytest.mark.parametrize("config", ["seg2_rc2", "rc0", "m4", "m6_tanh"])
def test_fused_other_configurations_against_float64(emf, config, form):
    """2-row segments, no right context, a bank of 4 with clamp and of 6 with tanh (62 of the fused step's 64 keys): forced cluster
    sizes 1 and 8 at 3 of 4 slots, and the automatic size at 65 streams; in each a slot restarts alone, so with a bank one stream's
    bank ramps up beside saturated ones.  The fused kernel must be what runs."""
    hp = hparams(config)
    assert fused_accepts(hp) and streams_per_group(hp) == 2
    if form == "auto65":
        _check(emf, config, "fused auto n=65", lock_step(65, hp, restart=(31, 13)), None, _fused, seed=900)
    else:
        _check(emf, config, f"fused {form} 3-of-4", three_of_four(hp), form, _fused, seed=33)


# ------------------------------------------------------------------------------------------------------------ the per-op plan
def per_op_upto(cus):
    """The per-op sweep straddles every kernel switch up to the largest stream count of the fused sweep, 2 x CUs + 1."""
    return 2 * cus + 1


def per_op_counts(hp, cus):
    ns = {1, 3, 65}
    for s in per_op_switches(hp, cus, per_op_upto(cus)):
        ns |= {s, s + 1}
    return sorted(ns)


PER_OP_SWITCHES = 3          # kernel switches of the per-op plan up to 2 x CUs + 1 streams on a 256-CU device


def test_per_op_plan_restated_at_256_cus():
    """conan_streams::conv's choice for the Emformer's layers at 256 CUs, up to 513 streams: ff1 (2 048 columns, 6 rows per stream)
    leaves the 32 x 32 tiles for 32 x 64 tiles at 38 streams (more than 224 rows) and for 64 x 64 at 75 (more than 448); kv (160
    columns, 6 rows per stream, 10 with a bank of 4) takes 32 x 64 tiles from more than 2 720 rows: 454 streams, 273 with the bank.
    q, out_proj, ff2 (80 columns) and proj (100) stay on 32 x 32 tiles.  The sweep's counts lie on both sides of every switch.  (Within
    the 32-row tiles the inter-block split-K factor - CUs / tiles, streams.hip:135-155 - also moves with the count: ff2 splits its
    K = 2 048 up to 224 streams, 8 ways at 1 - 37, and not at all at 272 and beyond; the same counts cover both.)"""
    want = {"seg4_rc2": [37, 74, 453], "m4": [37, 74, 272]}
    for config, sw in want.items():
        hp = hparams(config)
        assert per_op_switches(hp, 256, per_op_upto(256)) == sw and len(sw) == PER_OP_SWITCHES
        assert per_op_counts(hp, 256) == sorted({1, 3, 65} | set(sw) | {n + 1 for n in sw})
        assert per_op_kernels(3, hp, 256) == {CONV_CFGS[2][0]: 31}
        assert per_op_kernels(38, hp, 256) == {CONV_CFGS[2][0]: 25, CONV_CFGS[1][0]: 6}
        assert per_op_kernels(75, hp, 256) == {CONV_CFGS[2][0]: 25, CONV_CFGS[0][0]: 6}
        assert per_op_kernels(sw[2] + 1, hp, 256) == {CONV_CFGS[2][0]: 19, CONV_CFGS[1][0]: 6, CONV_CFGS[0][0]: 6}
        assert segments_covered(lambda n: tuple(sorted(per_op_kernels(n, hp, 256).items())), per_op_counts(hp, 256), per_op_upto(256))


PER_OP_CASES = ["n1", "n3", "n65", "5of6"] + [f"switch{i}{side}" for i in range(PER_OP_SWITCHES) for side in ("-", "+")]


@gpu
@pytest.mark.parametrize("case", PER_OP_CASES)
@pytest.mark.parametrize("config", ["seg4_rc2", "m4"])
def test_per_op_plan_against_float64(emf, config, case):
    """EMF_UNFUSED=1 - the plan that also runs when the fused kernel refuses a shape -, without a bank and with one: 1, 3 and 65
    lock-step streams, the stream counts on both sides of every kernel switch of conan_streams::conv up to 2 x CUs + 1 streams
    (from this device's CU count), and the five_of_six schedule with its restart.  Every step's conv_mfma launches against
    per_op_kernels; no fused kernel."""
    hp, cus = hparams(config), _num_cu()
    if case == "5of6":
        sched, label = five_of_six(hp), "per-op 5-of-6"
    else:
        if case.startswith("switch"):
            sw = per_op_switches(hp, cus, per_op_upto(cus))
            assert len(sw) == PER_OP_SWITCHES, (cus, sw)          # (another CU count may move a switch out of range: restate the cases then)
            n = sw[int(case[6])] + (1 if case.endswith("+") else 0)
        else:
            n = int(case[1:])
        sched, label = lock_step(n, hp, restart=(0, 13) if n > 1 else None), f"per-op n={n}"
    expect = lambda m: per_op_kernels(m, hp, cus)
    assert all(FUSED not in expect(len(ids)) for ids, _ in sched["steps"])
    _check(emf, config, label, sched, "EMF_UNFUSED=1", expect, seed=300)


@gpu
@pytest.mark.parametrize("config", ["m8", "m9"])
def test_per_op_plan_where_the_fused_step_refuses(emf, config):
    """Banks of 8 and 9 entries: 64 keys - the last lane of emf_attn_kernel's first key per lane - and 65, the first use of its second.
    The fused step refuses both shapes (G x M x D/4 > 256), so without any plan switch the per-op plan must be what runs: its
    conv_mfma launches and nothing else, every step.  3 of 4 slots, one restarted alone beside two saturated banks."""
    hp, cus = hparams(config), _num_cu()
    assert not fused_accepts(hp) and fused_accepts(hparams("m6_tanh"))
    seg, rc, M = _shape(hp)
    assert M + rc + LEFT_CONTEXT + seg == (64 if config == "m8" else 65)
    _check(emf, config, "per-op (fused refuses) 3-of-4", three_of_four(hp), None, lambda m: per_op_kernels(m, hp, cus), seed=33)


# ------------------------------------------------------------------------------------------------------------ the rule
def test_bounds_follow_the_rule():
    """The bounds are the stated rule applied to the recorded oracle figures, per configuration and tensor, a quarter of a
    two-limb product's error at the most, and the code comparison's threshold (twice the logits' max bound, logits rms 1) sits near 1e-4."""
    assert (RMS_FACTOR, MAX_FACTOR) == (8.0, 16.0) and set(ORACLE_FP32) == set(CONFIGS)
    for c, v in ORACLE_FP32.items():
        for t, (r, m) in v.items():
            assert BOUNDS[c][t] == (8 * r, 16 * m)
            assert 2e-6 < BOUNDS[c][t][0] < 2.0 ** -16 / 4 and 2e-5 < BOUNDS[c][t][1] < 5e-5, (c, t, BOUNDS[c][t])
