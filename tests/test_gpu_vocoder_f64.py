"""Every matrix kernel of the vocoder step outside ups.0 / ups.1 (tests/test_gpu_conv_tall.py has those) against FLOAT64, per slot,
across the launch plan: conv_pre, the four MRF stages (resblock_limb / resblock_fused / resblock_pair, the grouped conv_limb and
conv_mfma launches of the C = 256 stage, merged and separate last dilations, mean_act), ups.2 / ups.3 (conv_limb, its split-K-tail
build, conv_mfma), conv_post and the tanh.

Driven through hifigan_step_taps(stage_out=True) with the full synthetic checkpoint in both arithmetic forms.  Per step every tap of
every active slot is recorded, concatenated per slot and run (reset to next reset), and each checked tensor is compared with the
float64 reference (tests/vocoder_ref.py) of the tensor its kernel READ - so an error never carries over from the kernel in front.
Every slot is judged on its own (a wrong slot, row, tap or K slice gives errors near 1 in that slot; rounding ~1e-7), every schedule
runs until each ring has wrapped at least twice, the slot-runs evaluated are counted against the schedule's, and every step's
launches are asserted equal to a restatement of the plan (expected_kernels): a change of the plan fails here instead of silently
moving a shape out of coverage."""
import re
from collections import Counter

import numpy as np
import pytest
import torch

from conan_amd import _lib, configs, synth
from tests import vocoder_ref as vr
from tests.conftest import kernels_of
from tests.test_gpu_arith import _fold
from tests.test_gpu_conv_tall import _mixed, _sparse

gpu = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------------------ bounds
# Per slot and tensor: relative rms error; largest |error| / the slot's rms of that channel.  Neither comes from the kernels:
#   rms bound = min(2e-6, 8 x the fp32 ORACLE's rms),   max bound = min(6e-5, 16 x the fp32 oracle's max)
# where the oracle's figures are oracle/hifigan.py on .float() tensors on the CPU against the same float64 reference on the same
# inputs, slots (0, 29, 63) of the n64_f4 schedule, the worst of the three (oracle_yardstick below; test_bounds_follow_the_oracle
# recomputes them).  2e-6 / 6e-5 are the project's own ceilings (tests/test_gpu_arith.py; F32_RMS_BOUND / F32_MAX_BOUND of
# tests/test_gpu_conv_tall.py).  8 x: a K-ordered fp32 MFMA accumulation over up to 2 816 products, six convolutions chained per
# stage, is a few times less accurate than torch's blocked CPU sums, plan and shape variation needs room on top, and 8 x still sits an
# order below a product formed from two limbs instead of three (2^-16).  16 x for the single largest of 1e5 - 1e7 roundings, which
# scatters by tens of per cent between two correct kernels and grows with the sample count; a wrong row or slice gives ~1.
# tensor: (oracle fp32 rms, oracle fp32 max) as measured
ORACLE_FP32 = {
    "conv_pre": (1.961e-7, 6.794e-6),
    "stage.0": (9.064e-8, 1.519e-6), "stage.1": (8.954e-8, 1.206e-6), "stage.2": (8.613e-8, 1.446e-6), "stage.3": (8.282e-8, 1.532e-6),
    "ups.2": (2.116e-7, 2.023e-6), "ups.3": (1.500e-7, 1.475e-6),
    "conv_post": (1.928e-7, 1.367e-6),
}
# -> rms / max bounds: conv_pre 1.57e-6 / 6e-5 (the ceiling), stage.0 7.25e-7 / 2.43e-5, stage.1 7.16e-7 / 1.93e-5, stage.2 6.89e-7 / 2.31e-5,
#    stage.3 6.63e-7 / 2.45e-5, ups.2 1.69e-6 / 3.24e-5, ups.3 1.20e-6 / 2.36e-5, conv_post 1.54e-6 / 2.19e-5
RMS_CEILING, MAX_CEILING, RMS_FACTOR, MAX_FACTOR = 2e-6, 6e-5, 8.0, 16.0
BOUNDS = {k: (min(RMS_CEILING, RMS_FACTOR * r), min(MAX_CEILING, MAX_FACTOR * m)) for k, (r, m) in ORACLE_FP32.items()}
TANH_ATOL = 1e-6            # wav against tanh (float64) of the step's own fp32 pre_tanh tap: the reference's own tolerance (test_gpu_parity.py)
TENSORS = tuple(ORACLE_FP32)
YARDSTICK_SLOTS = (0, 29, 63)

# ------------------------------------------------------------------------------------------------------------ the plan, restated
TALL = "cnk::conv_tall_kernel"
SK = "cnk::conv_limb_sk_kernel<4, 1, 1, 4>"
RATES, UP_K, RB_K, RB_DIL, C0 = (8, 5, 4, 2), (16, 10, 8, 4), (3, 7, 11), (1, 3, 5), 512       # configs.HIFIGAN_16K320_SHUFFLE
CL_SHAPES = ((4, 1, 1, 4), (5, 1, 1, 4), (5, 2, 2, 2))      # conv_limb.hip:115  {NRW, NCW, RW, CW}: 64 x 64, 80 x 64, 160 x 64 tiles
SLOT_TABLE_PAD = 32                                          # kernels.h:39
LIMB_MAX_SLOTS = 256                                         # kernels.h:234 kResblockLimbMaxSlots
LIMB_ROWS = {32: 160, 64: 80, 128: 32}                       # resblock_limb.hip:699 kLimbCands (16 x NR2); every one has a merged build (:748)
FUSED_CANDS = ((32, 20), (32, 4), (64, 10), (64, 8), (64, 4), (128, 5), (128, 3))       # resblock_fused.hip:514
FUSED_MERGE = {(32, 320), (64, 160)}                         # resblock_fused.hip:599


def _ceil(a, b):
    return -(-a // b)


def _shape_fits(s, n, t, cout, ragged_ok):
    """conv_limb.hip:143-155 shape_fits."""
    tm, tn = 16 * s[0] * s[2], 16 * s[1] * s[3]
    m = n * t
    if t < tm:
        if tm % t or (not ragged_ok and m % tm):
            return False
        if m % tm and tm // t - 1 > SLOT_TABLE_PAD:
            return False
    elif t % tm or m % tm:
        return False
    return (_ceil(cout, 16) * 16) % tn == 0


def _tail_slices(n, t, cin, cout, s, cus):
    """conv_limb.hip:173-181 tail_slices."""
    tm, tn = 16 * s[0] * s[2], 16 * s[1] * s[3]
    tiles = _ceil(n * t, tm) * ((_ceil(cout, 16) * 16) // tn)
    rem = tiles % cus
    if tiles <= cus or rem == 0:
        return 1
    sl = min(8, cus // rem, cin // 32)
    return 1 if sl < 2 else sl


def tall_ok(cin, k, cout, n, t, cus, plan_n):
    """conv_tall.hip:326-338 conv_tall_plan (as tests/test_gpu_conv_tall.py tall_launches): at most 32 rows per slot, one 128-row tile
    of plan rows, 64 K blocks, an item for every CU; 128-column tiles."""
    nb = cin // 32 * k
    mp = (plan_n or n) * t
    if cout % 128 or t > 32 or mp < 128 or nb < 64:
        return False
    return _ceil(mp, 128) * (cout // 128) * min(16, nb // 8) >= cus


def conv_limb_choice(probs, n, t, cout, cus, plan_n, fixed):
    """The conv_limb launch streams.hip:74-96 launch_group makes for a group of problems [(Cin, taps, dilation)] of one (n, T, Cout) in
    a limb stream-set - its kernel name, or None: conv_mfma.  Restates conv_limb.hip:188-227 conv_limb_shape: a shape must fit every
    problem (shape_fits; the full set's rows as well in a fixed-plan set), its LDS window (TM / T slots of T + (k - 1) x dil rows) must
    hold in 32 x CL_NIT = 384 rows and 126 KB (2 buffers x 3 limbs x 48 bf16), its tiles must fill a third of the CUs (a group) or half
    (a single problem), a single problem in tiles below 80 rows needs a split-K tail; the cheapest estimated makespan wins.  The
    split-tail build runs for a single problem in 64-row tiles with >= 2 tail slices, never in a fixed-plan set (streams.hip:91)."""
    nprob = len(probs)
    best, best_cost = -1, 1e30
    for si, s in enumerate(CL_SHAPES):
        tm, tn = 16 * s[0] * s[2], 16 * s[1] * s[3]
        ok, tiles, units, umax = True, 0, 0.0, 0.0
        for cin, k, dil in probs:
            ok = (_shape_fits(s, plan_n, t, cout, nprob > 1) and _shape_fits(s, n, t, cout, True)) if plan_n else _shape_fits(s, n, t, cout, nprob > 1)
            if not ok:
                break
            tt = min(t, tm)
            wr = (tm // tt) * (tt + (k - 1) * dil)
            if wr > 32 * 12 or 2 * 3 * wr * 48 * 2 > 126 * 1024:
                ok = False
                break
            tl = _ceil((plan_n or n) * t, tm) * ((_ceil(cout, 16) * 16) // tn)
            u = float(k * cin * tm * tn)
            tiles, units, umax = tiles + tl, units + u * tl, max(umax, u)
        if not ok or tiles * (3 if nprob > 1 else 2) < cus:
            continue
        tail = _tail_slices(n, t, probs[0][0], cout, s, cus) if (nprob == 1 and not fixed and not plan_n and si == 0) else 1
        if nprob == 1 and tm < 80 and tail < 2:
            continue
        if nprob == 1:
            makespan = ((tiles // cus) + 1.0 / tail + 0.1 if tail >= 2 else float(_ceil(tiles, cus))) * umax
        else:
            makespan = max(units / cus, umax)
        cost = makespan * (1.0 if s[3] == 4 else 1.05)
        if cost < best_cost:
            best, best_cost = si, cost
    if best < 0:
        return None
    if nprob == 1 and not fixed and best == 0 and _tail_slices(n, t, probs[0][0], cout, CL_SHAPES[0], cus) >= 2:
        return SK
    return "cnk::conv_limb_kernel<%d, %d, %d, %d>" % CL_SHAPES[best]


def fused_rows(c, t, n, cus, ksum=sum(RB_K), kmax=max(RB_K)):
    """resblock_fused.hip:522-533 resblock_fused_rows: the candidate tile height with the smallest estimated makespan."""
    best, best_cost = 0, 1e30
    for cc, nr2 in FUSED_CANDS:
        if cc != c:
            continue
        ro = 16 * nr2
        per_cu = max(float(n) * _ceil(t, ro) * ksum / max(1, cus), float(kmax))
        cost = per_cu * (2 * nr2 + 1) + 0.15 * per_cu / kmax * 40
        if cost < best_cost:
            best, best_cost = ro, cost
    return best


def expected_kernels(arith, max_slots, max_frames, n, frames, cus, fixed=False):
    """The matrix-kernel launches of one blocking vocoder step: ({kernel name: launches} of every kernel but conv_mfma, the number of
    conv_mfma launches, a one-line description per stage).  Restates streams.hip build_vocoder (:431-502: which stages run the fused
    tile pass - limb sets from 4 slots, f32 sets from 8, C = 32 always; the pair kernel for C = 256 in f32 sets of >= 16 slots and at
    most 32 rows per step), hifigan_step (:504-649), launch_group (:51-158: conv_tall, then conv_limb, then conv_mfma) and launch_rb
    (:214-246: the limb pass up to 256 plan slots, the tile height, and the merged last dilation - a group per CU, the last round of
    groups at least 90 % full, a merged build for the geometry).  plan slots = max_slots in a fixed-plan set, else the active count."""
    limb = arith == "limb"
    pn = max_slots if fixed else n
    exp, mfma, desc = Counter(), 1, []                       # conv_pre: always conv_mfma (80 input channels, no limb weights: ctx.hip:84)
    cprev, rate = C0, 1
    for i in range(len(RATES)):
        c, t_in = cprev // 2, frames * rate
        rate *= RATES[i]
        t = frames * rate
        up = "mfma"
        if limb:
            if tall_ok(cprev, UP_K[i], c * RATES[i], n, t_in, cus, pn if fixed else 0):
                exp[TALL] += 1
                up = "tall"
            else:
                name = conv_limb_choice([(cprev, UP_K[i], 1)], n, t_in, c * RATES[i], cus, pn if fixed else 0, fixed)
                if name:
                    exp[name] += 1
                    q = [int(v) for v in re.findall(r"\d+", name.split("<")[1])]
                    up = "limb_sk" if name == SK else "limb%d" % (16 * q[0] * q[2])
        if up == "mfma":
            mfma += 1
        fused = c in (32, 64, 128) and (max_slots >= (4 if limb else 8) or c <= 32)
        pair = not fused and not limb and c == 256 and max_slots >= 16 and max_frames * rate <= 32
        if pair:
            exp["cnk::resblock_pair_kernel<%d>" % (2 if t > 16 else 1)] += len(RB_DIL)
            st = "pair"
        elif fused:
            as_limb = limb and pn <= LIMB_MAX_SLOTS
            rows = LIMB_ROWS[c] if as_limb else fused_rows(c, t, pn, cus)
            groups = pn * _ceil(t, rows)
            rounds = _ceil(groups, cus)
            can = True if as_limb else (c, rows) in FUSED_MERGE
            merge = groups >= cus and groups * 10 >= rounds * cus * 9 and can
            for d in range(len(RB_DIL)):
                m = "true" if (merge and d + 1 == len(RB_DIL)) else "false"
                exp[("cnk::resblock_limb_kernel<%d, %d, 50, %s>" % (c, rows // 16, m)) if as_limb else ("cnk::resblock_fused_kernel<%d, %d, %s>" % (c, rows // 16, m))] += 1
            st = ("rl%d" if as_limb else "rf%d") % rows + ("+m" if merge else "")
        else:
            nl = 0
            for d in RB_DIL:
                for dil in (d, 1):                           # c1 (dilated), c2
                    name = conv_limb_choice([(c, k, dil) for k in RB_K], n, t, c, cus, pn if fixed else 0, fixed) if limb else None
                    if name:
                        exp[name] += 1
                        nl += 1
                    else:
                        mfma += 1
            st = "mfma" if nl == 0 else ("cl%d" % nl)
        desc.append("%s>%s" % (up, st))
        cprev = c
    return dict(exp), mfma, " ".join(desc)


# The plan of uniform 4-frame steps (max_slots = active slots) at 256 CUs, per stage "upsampler>stage":
#   upsampler  tall | limb80 / limb160 (conv_limb's 80- / 160-row tiles) | limb_sk (64-row tiles, split-K tail) | mfma
#   stage      mfma | clN (N of the 6 grouped launches are conv_limb's) | pair | rlR / rfR (resblock_limb / resblock_fused in R-row tiles), +m merged
# expected_kernels must agree with it on a 256-CU device: a change of a plan threshold shows here.
PLAN_TABLE = {}      # filled below: PLAN_TABLE[(arith, n)] = description


def _table(text):
    for line in text.strip().splitlines():
        arith, n, d = line.split(None, 2)
        PLAN_TABLE[(arith, int(n))] = d.strip()


_table("""
limb   1  mfma>mfma mfma>mfma mfma>mfma mfma>rl160
limb   3  mfma>mfma mfma>mfma mfma>cl6 mfma>rl160
limb   4  mfma>mfma mfma>rl32 mfma>rl80 mfma>rl160
limb   7  mfma>mfma mfma>rl32 mfma>rl80 mfma>rl160
limb   8  mfma>mfma mfma>rl32 mfma>rl80 mfma>rl160
limb  15  mfma>cl6 mfma>rl32 mfma>rl80 mfma>rl160
limb  16  mfma>cl6 mfma>rl32 limb80>rl80 limb80>rl160
limb  17  mfma>cl6 mfma>rl32 limb80>rl80 limb80>rl160
limb  31  mfma>cl6 tall>rl32 limb80>rl80 limb80>rl160
limb  32  tall>cl6 tall>rl32 limb80>rl80+m limb80>rl160+m
limb  33  tall>cl6 tall>rl32 limb80>rl80 limb_sk>rl160
limb  57  tall>cl6 tall>rl32 limb80>rl80 limb80>rl160
limb  58  tall>cl6 tall>rl32 limb80>rl80+m limb80>rl160+m
limb  64  tall>cl6 tall>rl32 limb80>rl80+m limb80>rl160+m
limb  65  tall>cl6 tall>rl32 limb80>rl80 limb80>rl160
limb  86  tall>cl6 tall>rl32 limb80>rl80 limb_sk>rl160
limb  87  tall>cl6 tall>rl32 limb80>rl80+m limb_sk>rl160+m
limb  92  tall>cl6 tall>rl32 limb80>rl80+m limb80>rl160+m
limb  93  tall>cl6 tall>rl32+m limb80>rl80+m limb80>rl160+m
limb  96  tall>cl6 tall>rl32+m limb80>rl80+m limb80>rl160+m
limb  97  tall>cl6 tall>rl32+m limb80>rl80 limb80>rl160
limb 102  tall>cl6 tall>rl32+m limb80>rl80 limb80>rl160
limb 103  tall>cl6 tall>rl32 limb80>rl80 limb_sk>rl160
limb 115  tall>cl6 tall>rl32 limb80>rl80 limb_sk>rl160
limb 116  tall>cl6 tall>rl32 limb80>rl80+m limb80>rl160+m
limb 128  tall>cl6 tall>rl32 limb80>rl80+m limb80>rl160+m
limb 129  tall>cl6 tall>rl32 limb80>rl80 limb_sk>rl160
limb 256  tall>cl6 tall>rl32+m limb80>rl80+m limb80>rl160+m
limb 257  tall>cl6 tall>rf80 limb80>rf160 limb_sk>rf320
f32    1  mfma>mfma mfma>mfma mfma>mfma mfma>rf64
f32    3  mfma>mfma mfma>mfma mfma>mfma mfma>rf64
f32    4  mfma>mfma mfma>mfma mfma>mfma mfma>rf64
f32    7  mfma>mfma mfma>mfma mfma>mfma mfma>rf64
f32    8  mfma>mfma mfma>rf48 mfma>rf64 mfma>rf64
f32   15  mfma>mfma mfma>rf48 mfma>rf64 mfma>rf64
f32   16  mfma>pair mfma>rf48 mfma>rf64 mfma>rf64
f32   17  mfma>pair mfma>rf48 mfma>rf64 mfma>rf64
f32   24  mfma>pair mfma>rf48 mfma>rf64 mfma>rf64
f32   31  mfma>pair mfma>rf48 mfma>rf128 mfma>rf320
f32   32  mfma>pair mfma>rf48 mfma>rf128 mfma>rf320
f32   33  mfma>pair mfma>rf48 mfma>rf160 mfma>rf320
f32   40  mfma>pair mfma>rf48 mfma>rf160 mfma>rf320
f32   48  mfma>pair mfma>rf48 mfma>rf160 mfma>rf320
f32   57  mfma>pair mfma>rf80 mfma>rf160 mfma>rf320
f32   58  mfma>pair mfma>rf80 mfma>rf160 mfma>rf320
f32   64  mfma>pair mfma>rf80 mfma>rf160+m mfma>rf320+m
f32   65  mfma>pair mfma>rf80 mfma>rf160 mfma>rf320
f32   92  mfma>pair mfma>rf80 mfma>rf160 mfma>rf320
f32   93  mfma>pair mfma>rf80 mfma>rf160 mfma>rf320
f32  102  mfma>pair mfma>rf80 mfma>rf160 mfma>rf320
f32  103  mfma>pair mfma>rf80 mfma>rf160 mfma>rf320
f32  115  mfma>pair mfma>rf80 mfma>rf160 mfma>rf320
f32  116  mfma>pair mfma>rf80 mfma>rf160+m mfma>rf320+m
f32  128  mfma>pair mfma>rf80 mfma>rf160+m mfma>rf320+m
f32  129  mfma>pair mfma>rf80 mfma>rf160 mfma>rf320
""")

# ------------------------------------------------------------------------------------------------------------ schedules
RINGS = vr.vocoder_rings(configs.hifigan_hparams())


def _uniform(n, frames, max_frames=None, least=12):
    mf = max_frames or frames
    return {"slots": n, "max_frames": mf, "steps": [(list(range(n)), frames, [])] * vr.steps_to_wrap_twice(frames, mf, RINGS, least)}


def _sparse15(slots=16):
    """A 16-slot set stepped with all 16 and with 15 slots (one left out, the rest in random order): 15 active slots of 32 rows are
    the fewest whose grouped conv_limb launches give every third CU a tile."""
    rng = np.random.default_rng(15)
    steps = []
    for s in range(vr.steps_to_wrap_twice(4, 4, RINGS) + 8):
        ids = [int(i) for i in rng.permutation(slots)]
        steps.append((ids[:15] if s % 2 else ids, 4, []))
    return {"slots": slots, "max_frames": 4, "steps": steps}


def _sparse_f2():
    """64 slots of a max_frames = 2 set (16 rows per slot in the C = 256 stage: four slots per conv_limb tile), a random subset in
    random order per step - sizes on both sides of the grouped launches' threshold (29) and with every remainder n % 4, so ragged last
    tiles stage slots from all over the table -, 1- and 2-frame steps, slots reset at two steps."""
    rng = np.random.default_rng(12)
    sizes = [64, 30, 29, 28, 47, 33, 61, 35, 57, 31]
    steps = []
    for s in range(40):
        ids = [int(i) for i in rng.permutation(64)[:sizes[s % len(sizes)]]]
        steps.append((ids, 1 if s % 5 == 3 else 2, [2, 30, 63] if s == 11 else ([30, 44] if s == 23 else [])))
    return {"slots": 64, "max_frames": 2, "steps": steps}


UNIFORM_F4 = {
    "limb": (1, 3, 4, 7, 8, 15, 16, 17, 31, 32, 33, 57, 58, 64, 65, 86, 87, 92, 93, 96, 97, 102, 103, 115, 116, 128, 129, 256, 257),
    "f32": (1, 3, 4, 7, 8, 15, 16, 17, 24, 31, 32, 33, 40, 48, 57, 58, 64, 65, 92, 93, 102, 103, 115, 116, 128, 129),
}
CASES = {}
for _n in sorted(set(UNIFORM_F4["limb"]) | set(UNIFORM_F4["f32"])):
    CASES["n%d_f4" % _n] = (lambda n=_n: _uniform(n, 4))
# fewer frames: ragged last row tiles inside a slot (T = 120 / 480 / 960 at 3 frames), several slots per conv_limb tile (T = 8, 16: the
# grouped launches start at 57 / 29 active slots) with ragged last tiles, resblock_pair at T = 8 / 16 / 24; odd and prime counts
for _n in (13, 56, 57, 61, 64):
    CASES["n%d_f1" % _n] = (lambda n=_n: _uniform(n, 1))
for _n in (7, 28, 29, 31, 33, 64):
    CASES["n%d_f2" % _n] = (lambda n=_n: _uniform(n, 2))
for _n in (7, 33):
    CASES["n%d_f3" % _n] = (lambda n=_n: _uniform(n, 3))
for _n in (5, 16, 17, 43, 64):
    CASES["n%d_f3of4" % _n] = (lambda n=_n: _uniform(n, 3, max_frames=4))
# long steps: 128 / 96 rows per slot in the C = 256 stage (no pair kernel; conv_limb's tiles inside a slot / conv_mfma)
for _n, _f in ((3, 16), (20, 16), (5, 12), (16, 12)):
    CASES["n%d_f%d" % (_n, _f)] = (lambda n=_n, f=_f: _uniform(n, f, least=6))
CASES["sparse64_resets"] = _sparse
CASES["mixed64_frames"] = _mixed
CASES["sparse16_of15"] = _sparse15
CASES["sparse64_f2_resets"] = _sparse_f2
LIMB_ONLY = {"n%d_f4" % n for n in set(UNIFORM_F4["limb"]) - set(UNIFORM_F4["f32"])}
F32_ONLY = {"n%d_f4" % n for n in set(UNIFORM_F4["f32"]) - set(UNIFORM_F4["limb"])}
PARAMS = [(name, a) for name in CASES for a in ("limb", "f32") if not (a == "limb" and name in F32_ONLY) and not (a == "f32" and name in LIMB_ONLY)]


def schedule_slot_runs(case):
    """Slot-runs of a schedule (a run = a slot's active steps between two resets), counted from the schedule alone."""
    open_, total = set(), 0
    for ids, _, resets in case["steps"]:
        open_ -= set(resets)
        for s in ids:
            if s not in open_:
                open_.add(s)
                total += 1
    return total


# ------------------------------------------------------------------------------------------------------------ running
@pytest.fixture(scope="module")
def voc():
    """A vocoder context with the full synthetic checkpoint, and the folded fp32 weights (what library and reference multiply) as
    float64 tensors on the GPU."""
    from conan_amd.runtime import Context
    vhp = configs.hifigan_hparams()
    sd = synth.hifigan_state_dict(vhp, 0)
    ctx = Context(None, vhp, 0, False, False, True)
    ctx.load_state_dict("hifigan", sd)
    ctx.finalize()
    folded = _fold(sd)
    sd64 = {k: torch.from_numpy(v).double().cuda() for k, v in folded.items()}
    yield ctx, vhp, sd64, folded
    ctx.close()


def _num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


MATRIX = ("resblock_", "conv_limb", "conv_tall", "conv_mfma")
KEYS = ("mel", "cpre", "ups0", "ups1", "ups2", "ups3", "so0", "so1", "so2", "so3", "pre", "wav")


def _run_schedule(ctx, arith, case, flags=0):
    """Drive hifigan_step_taps(stage_out=True) through the case's steps, every step's launches against expected_kernels.  -> per slot a
    list of runs (one per reset), each {key: tensor concatenated over the run's steps} (GPU tensors), the set of (n, frames,
    description) seen, and the kernel names seen."""
    S, steps = case["slots"], case["steps"]
    fixed = bool(flags & _lib.STREAMS_FIXED_PLAN)
    st = ctx.streams(S, max_frames=case["max_frames"], max_ref_frames=16, arith=arith, flags=flags)
    assert st.arith == arith
    total = sum(f for _, f, _ in steps)
    mels = torch.from_numpy(synth.mel(total, 21, S)).cuda()
    cursor = [0] * S
    runs = [[[]] for _ in range(S)]
    st.reset(list(range(S)))
    cu = _num_cu()
    plans, seen = set(), set()
    for step, (ids, frames, resets) in enumerate(steps):
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
        names = {k: v for k, v in names.items() if any(m in k for m in MATRIX)}
        exp, mfma, desc = expected_kernels(arith, S, case["max_frames"], len(ids), frames, cu, fixed)
        got = {k: v for k, v in names.items() if "conv_mfma" not in k}
        got_mfma = sum(v for k, v in names.items() if "conv_mfma" in k)
        assert got == exp and got_mfma == mfma, ("step", step, "n", len(ids), "frames", frames, desc, "launched", sorted(names.items()), "expected", sorted(exp.items()), "conv_mfma", mfma)
        plans.add((len(ids), frames, desc))
        seen |= set(names)
        wav, pre, cpre, ups, outs = out["t"]
        rec = (mel, cpre, ups[0], ups[1], ups[2], ups[3], outs[0], outs[1], outs[2], outs[3], pre.unsqueeze(2), wav.unsqueeze(2))
        for j, s in enumerate(ids):
            runs[s][-1].append((rec, j))
    torch.cuda.synchronize()
    st.close()
    res = []
    for s in range(S):
        res.append([{k: torch.cat([rec[q][j] for rec, j in run]) for q, k in enumerate(KEYS)} for run in runs[s] if run])
    return res, plans, seen


def reference_of(tensor, r, sd64, vhp):
    """(what the kernel wrote, its float64 reference on what the kernel read) for a group of runs r = {key: [members, rows, C]}."""
    if tensor == "conv_pre":
        return r.get("cpre"), vr.ref_conv_pre(r["mel"], sd64)
    if tensor.startswith("stage."):
        i = int(tensor[6:])
        return r["so%d" % i], vr.ref_stage(r["ups%d" % i], sd64, i, vhp)
    if tensor.startswith("ups."):
        i = int(tensor[4:])
        name = "ups.%d.conv.conv" % i
        return r["ups%d" % i], vr.ref_upsampler(r["so%d" % (i - 1)], sd64[name + ".weight"], sd64[name + ".bias"], vhp["upsample_rates"][i])
    assert tensor == "conv_post"
    return r.get("pre"), vr.ref_conv_post(r["so3"], sd64)


def _check_case(voc, arith, name, flags=0, case=None):
    ctx, vhp, sd64, _ = voc
    case = case or CASES[name]()
    runs, plans, seen = _run_schedule(ctx, arith, case, flags)
    groups = {}                                  # runs of one length are evaluated together
    for s, rs in enumerate(runs):
        for ri, r in enumerate(rs):
            groups.setdefault(r["mel"].shape[0], []).append((s, ri, r))
    stats, bad, tanh_worst, tanh_runs = {}, [], 0.0, 0
    for members in groups.values():
        r = {k: torch.stack([m[2][k] for m in members]) for k in KEYS}
        for tensor in TENSORS:
            got, want = reference_of(tensor, r, sd64, vhp)
            assert want.shape == got.shape, (tensor, want.shape, got.shape)
            # no channel of a reference tensor is silent: the per-channel normalisation of the max statistic clamps nothing
            assert float(want.pow(2).mean(1).min()) > 0.0, (name, tensor)
            rms, mx, fin = vr.slot_errors(got, want)
            rb, mb = BOUNDS[tensor]
            for i, (s, ri, _) in enumerate(members):
                stats.setdefault(tensor, []).append((float(rms[i]), float(mx[i]), s))
                if not (bool(fin[i]) and rms[i] <= rb and mx[i] <= mb):
                    bad.append((tensor, "slot", s, "run", ri, "finite", bool(fin[i]), "rms", float(rms[i]), "max", float(mx[i]), "bounds", rb, mb))
        # the activation alone: wav against tanh, in float64, of the fp32 pre-tanh tap of the same step
        e = (r["wav"].double() - torch.tanh(r["pre"].double())).abs().amax((1, 2))
        fin = torch.isfinite(r["wav"]).flatten(1).all(1)
        tanh_runs += len(members)
        for i, (s, ri, _) in enumerate(members):
            tanh_worst = max(tanh_worst, float(e[i]))
            if not (bool(fin[i]) and e[i] <= TANH_ATOL):
                bad.append(("tanh", "slot", s, "run", ri, "finite", bool(fin[i]), "max abs", float(e[i]), "atol", TANH_ATOL))
    print(f"\n[vocoder-vs-f64] {name} {arith}{' fixed-plan' if flags else ''}: {len(case['steps'])} steps; (slots, frames, plan) {sorted(plans)}")
    print("  kernels: " + "; ".join(sorted(k.replace("cnk::", "") for k in seen)))
    for key in TENSORS:
        v = stats[key]
        r = sorted(v)
        m = max(v, key=lambda e: e[1])
        print(f"  {key:9s}: {len(v)} slot runs, rel rms median {r[len(r) // 2][0]:.3e} worst {r[-1][0]:.3e} (slot {r[-1][2]}), "
              f"max/ch-rms worst {m[1]:.3e} (slot {m[2]})   bounds {BOUNDS[key][0]:.2e} {BOUNDS[key][1]:.2e}")
    print(f"  tanh     : {tanh_runs} slot runs, worst |wav - tanh(pre_tanh)| {tanh_worst:.3e}")
    # no slot and no step left out: every tensor was evaluated for every slot-run of the schedule
    want_runs = schedule_slot_runs(case)
    assert tanh_runs == want_runs and all(len(stats[k]) == want_runs for k in TENSORS), (name, want_runs, tanh_runs, {k: len(v) for k, v in stats.items()})
    assert not bad, (name, arith, len(bad), bad[:8])
    return plans


@gpu
@pytest.mark.parametrize("name,arith", PARAMS)
def test_vocoder_kernels_against_float64(voc, name, arith):
    """conv_pre, the four stages, ups.2 / ups.3, conv_post and the tanh of every active slot of every step, per slot, against float64
    of the tensor each kernel read; every step's launches as expected_kernels says."""
    _check_case(voc, arith, name)


@gpu
@pytest.mark.parametrize("arith", ["limb", "f32"])
@pytest.mark.parametrize("name", ["sparse64_resets", "mixed64_frames", "sparse64_f2_resets"])
def test_fixed_plan_schedules_against_float64(voc, name, arith):
    """The sparse / permuted schedules with resets and the mixed frame counts in a STREAMS_FIXED_PLAN set: plan rows from max_slots
    (64), tiles from the live count, no split tails."""
    _check_case(voc, arith, name, flags=_lib.STREAMS_FIXED_PLAN)


@gpu
def test_plan_table_matches_the_helper():
    """expected_kernels on this device equals the stated table for uniform 4-frame steps (a device with another CU count skips
    rather than retargets), and the switch points the sweep straddles are where the comments say."""
    cu = _num_cu()
    if cu != 256:
        pytest.skip(f"the table is for 256 CUs, this device has {cu}")
    check_plan_table(cu)


def check_plan_table(cu):
    got = {(a, n): expected_kernels(a, n, 4, n, 4, cu)[2] for a, n in PLAN_TABLE}
    assert got == PLAN_TABLE, sorted((k, got[k], PLAN_TABLE[k]) for k in got if got[k] != PLAN_TABLE[k])
    assert {(a, n) for a in UNIFORM_F4 for n in UNIFORM_F4[a]} <= set(PLAN_TABLE)

    def merged(arith, stage):
        return [n for n in range(1, 258) if expected_kernels(arith, n, 4, n, 4, cu)[2].split()[stage].endswith("+m")]

    def spans(v):
        out = []
        for n in v:
            if out and out[-1][1] == n - 1:
                out[-1][1] = n
            else:
                out.append([n, n])
        return [tuple(x) for x in out]
    # merged last dilations (launch_rb): limb C = 64 / 32, 8 row tiles per slot; limb C = 128, 5 per slot; f32 C = 64 / 32, one tile per slot
    assert spans(merged("limb", 2)) == spans(merged("limb", 3)) == [(32, 32), (58, 64), (87, 96), (116, 128), (144, 160), (173, 192), (202, 224), (231, 256)]
    assert spans(merged("limb", 1))[:2] == [(93, 102), (139, 153)]
    assert spans(merged("f32", 3))[:2] == [(64, 64), (116, 128)]
    # the grouped conv_limb launches of the C = 256 stage need a tile for every third CU
    for frames, first in ((4, 15), (2, 29), (1, 57)):
        ns = [n for n in range(1, 129) if expected_kernels("limb", max(n, 16), frames, n, frames, cu)[2].split()[0].split(">")[1].startswith("cl")]
        assert ns[0] == first, (frames, ns[:3])


# ------------------------------------------------------------------------------------------------------------ conv_post's own mean
@gpu
@pytest.mark.parametrize("arith", ["limb", "f32"])
@pytest.mark.parametrize("S", [16, 64])
def test_conv_post_forms_the_same_mean_as_mean_act(voc, S, arith):
    """With stage_out=True the last stage's leaky_relu(mean) comes from mean_act (or a merged launch); without the tap conv_post forms
    it itself from the raw branch outputs and appends it to the xs ring (streams.hip:623-648).  A twin set on the same inputs that
    alternates stage_out=True / stage_out=False / plain hifigan_step must give pre_tanh and wav BIT-identical to the always-tapped set
    at every step (same operations in the same order; the ring valid whichever way a step produced it).  16 slots: no merged last
    dilation; 64: merged in both forms.  (The always-tapped form is the one the sweep checks against float64.)"""
    ctx = voc[0]
    ids = list(range(S))
    steps = vr.steps_to_wrap_twice(4, 4, RINGS)
    mels = torch.from_numpy(synth.mel(4 * steps, 77, S)).cuda()
    a = ctx.streams(S, max_frames=4, max_ref_frames=16, arith=arith)
    b = ctx.streams(S, max_frames=4, max_ref_frames=16, arith=arith)
    for st in (a, b):
        st.reset(ids)
    merged = expected_kernels(arith, S, 4, S, 4, _num_cu())[2].split()[3].endswith("+m")
    if _num_cu() == 256:
        assert merged == (S == 64)
    for t in range(steps):
        x = mels[:, 4 * t:4 * t + 4].contiguous()
        wa, pa = a.hifigan_step_taps(ids, x, stage_out=True)[:2]
        if t % 3 == 0:
            wb, pb = b.hifigan_step_taps(ids, x, stage_out=True)[:2]
        elif t % 3 == 1:
            wb, pb = b.hifigan_step_taps(ids, x, stage_out=False)[:2]
        else:
            wb, pb = b.hifigan_step(ids, x, want_pre_tanh=True)
        assert torch.equal(pa, pb), ("pre_tanh", "step", t, float((pa - pb).abs().max()))
        assert torch.equal(wa, wb), ("wav", "step", t, float((wa - wb).abs().max()))
        assert torch.isfinite(wa).all()
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------------------ the yardstick
def oracle_yardstick(r, folded, vhp):
    """The fp32 ORACLE's error statistics per tensor: r = {key: [slots, rows, C]} CPU tensors of one run; oracle/hifigan.py on float32
    tensors on the CPU against the float64 reference of the same inputs; the worst slot.  -> {tensor: (rms, max)}"""
    from oracle import hifigan as ohifi
    lrelu = torch.nn.functional.leaky_relu
    sd32 = {k: torch.from_numpy(v).float() for k, v in folded.items()}
    sd64 = {k: v.double() for k, v in sd32.items()}
    nb = len(vhp["resblock_kernel_sizes"])
    out = {}
    with torch.no_grad():
        for tensor in TENSORS:
            _, want = reference_of(tensor, r, sd64, vhp)
            if tensor == "conv_pre":
                got = lrelu(ohifi._cconv(sd32, "conv_pre.conv", r["mel"].float().transpose(1, 2)), ohifi.LRELU_SLOPE)
            elif tensor.startswith("stage."):
                i = int(tensor[6:])
                x = r["ups%d" % i].float().transpose(1, 2)
                acc = 0
                for j in range(nb):
                    acc = acc + ohifi.resblock1(sd32, i * nb + j, x, vhp["resblock_dilation_sizes"][j])
                got = lrelu(acc / nb, ohifi.LRELU_SLOPE)
            elif tensor.startswith("ups."):
                i = int(tensor[4:])
                y = ohifi._cconv(sd32, "ups.%d.conv.conv" % i, r["so%d" % (i - 1)].float().transpose(1, 2))
                got = ohifi.pixel_shuffle_1d(y, vhp["upsample_rates"][i])
            else:
                got = ohifi._cconv(sd32, "conv_post.conv", r["so3"].float().transpose(1, 2))
            assert got.dtype == torch.float32
            rms, mx, fin = vr.slot_errors(got.transpose(1, 2).contiguous(), want)
            assert bool(fin.all())
            out[tensor] = (float(rms.max()), float(mx.max()))
    return out


def test_bounds_follow_the_rule():
    """The bounds are the stated rule applied to the recorded oracle figures, per tensor, and never above the project's ceilings."""
    for k, (r, m) in ORACLE_FP32.items():
        assert BOUNDS[k] == (min(2e-6, 8 * r), min(6e-5, 16 * m))
        assert 0 < BOUNDS[k][0] <= 2e-6 and 0 < BOUNDS[k][1] <= 6e-5


@gpu
@pytest.mark.parametrize("arith", ["f32"])
def test_bounds_follow_the_oracle(voc, arith):
    """The recorded ORACLE_FP32 figures are what the fp32 oracle gives on this run's inputs (slots 0, 29, 63 of n64_f4): recomputed and
    printed; each recorded rms within a factor 1.25 of the recomputed one, each recorded max within a factor 2 (the largest single
    rounding scatters by tens of per cent with the inputs' last bits), so the constants cannot drift away from their source."""
    ctx, vhp, _, folded = voc
    runs, _, _ = _run_schedule(ctx, arith, CASES["n64_f4"]())
    r = {k: torch.stack([runs[s][0][k] for s in YARDSTICK_SLOTS]).cpu() for k in KEYS}
    y = oracle_yardstick(r, folded, vhp)
    print("\n[vocoder-vs-f64] fp32 oracle against float64, slots %s of n64_f4 (rms, max/ch-rms) -> bounds" % (YARDSTICK_SLOTS,))
    for k in TENSORS:
        print(f"  {k:9s}: {y[k][0]:.3e} {y[k][1]:.3e}   recorded {ORACLE_FP32[k][0]:.3e} {ORACLE_FP32[k][1]:.3e}   bounds {BOUNDS[k][0]:.3e} {BOUNDS[k][1]:.3e}")
    for k in TENSORS:
        assert ORACLE_FP32[k][0] / 1.25 <= y[k][0] <= ORACLE_FP32[k][0] * 1.25, (k, y[k], ORACLE_FP32[k])
        assert ORACLE_FP32[k][1] / 2 <= y[k][1] <= ORACLE_FP32[k][1] * 2, (k, y[k], ORACLE_FP32[k])
