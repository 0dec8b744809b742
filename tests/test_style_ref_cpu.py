"""tests/style_ref.py alone, on the CPU: the float64 reference of the style pass is pinned to oracle/conan.py, the yardsticks of
tests/test_gpu_style_f64.py (ORACLE_FP32, style_ref.BAND) are recomputed from the fp32 oracle, the share of unsafe tokens is capped
with the reference alone, the cases reach the launch forms they are there for on 256 CUs, and the judge with the GPU test's bounds
rejects deliberate changes to the oracle side."""
import contextlib

import numpy as np
import pytest
import torch

from oracle import conan as oconan
from tests import style_ref as S
from tests import test_gpu_style_f64 as g

_RUNS = {}


def _oracle_run(name):
    if name not in _RUNS:
        _RUNS[name] = S.oracle_run(name)
    return _RUNS[name]


# ------------------------------------------------------------------------------------------------------------ pinning
@pytest.mark.parametrize("name", list(S.CASES))
def test_reference_is_the_oracle(name):
    """With nothing overridden the float64 reference chooses the fp32 oracle's ids on every reference of the case; style_reference in
    fp32 IS the oracle (tokens bit for bit: the part behind the quantiser is restated only to take ids_override); a slot alone is a
    slot of a batch of equal lengths; an override changes what follows the quantiser and nothing in front of it."""
    mels, _ = S.case_references(name)
    for i, m in enumerate(mels):
        w = S.style_reference(m, torch.float64, key=(name, i))
        f = S.style_reference(m, torch.float32, key=(name, i))
        assert w["style"].dtype == w["tokens"].dtype == w["kv"][0].dtype == torch.float64 and f["tokens"].dtype == torch.float32
        assert torch.equal(w["ids"], f["oracle_ids"]) and torch.equal(w["ids"], f["ids"]) and torch.equal(w["ids"], w["oracle_ids"]), (name, i)
        assert torch.equal(f["tokens"], f["oracle_tokens"]) and torch.equal(w["tokens"], w["oracle_tokens"])
        assert w["ids"].shape[0] == S.tokens_of(m.shape[0]) and w["kv"][0].shape == (w["ids"].shape[0], 2 * g.H)
        assert bool((w["mask"] == 1).all())             # no key of a token is ever masked: l1 has a bias
    # the K/V rows are what the attention forms from the tokens: a layer's attention recomputed from them equals the oracle's
    sd, hp = S.sd64(), S.P.model()[0]
    w = S.style_reference(mels[-1], torch.float64, key=(name, len(mels) - 1))
    q_in = torch.randn(3, 1, g.H, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    _, attn = oconan.cross_atten_layer(sd, "align.layers.1", q_in, w["tokens"][:, None], None)
    wq, bq = sd["align.layers.1.multihead_attn.in_proj_weight"][:g.H], sd["align.layers.1.multihead_attn.in_proj_bias"][:g.H]
    dh = g.H // S.NHEAD
    q = (torch.nn.functional.linear(q_in[:, 0], wq, bq) * dh ** -0.5).reshape(3, S.NHEAD, dh)
    k = w["kv"][1][:, :g.H].reshape(-1, S.NHEAD, dh)
    mine = torch.softmax(torch.einsum("thd,shd->hts", q, k), -1).mean(0)
    assert torch.allclose(mine, attn[0], rtol=1e-12, atol=1e-15)
    if name == "short":
        other = w["ids"].clone()
        other[0] = (other[0] + 1) % 64
        o = S.style_reference(mels[-1], torch.float64, ids_override=other, key=(name, len(mels) - 1))
        assert torch.equal(o["style"], w["style"]) and torch.equal(o["ids"], w["ids"]) and not torch.equal(o["tokens"][0], w["tokens"][0])
        assert torch.equal(o["tokens"][1:], w["tokens"][1:]) and torch.equal(o["used"], other)


def test_a_slot_alone_is_a_row_of_its_batch():
    """The library's per-slot meaning: the oracle on a batch of equal lengths gives every row what the row gives alone (float64)."""
    mels = [S.case_mels("short")[4], S.case_mels("passes")[8]]
    assert mels[0].shape == mels[1].shape == (5, 80)
    c = oconan.style_pass(S.sd64(), S.P.model()[0], torch.from_numpy(np.stack(mels)).double())
    for i, m in enumerate(mels):
        w = S.style_reference(m, torch.float64)
        assert torch.allclose(c["style_embed"][i, 0], w["style"], rtol=1e-12, atol=1e-14) and torch.equal(c["vq_ids"][i], w["ids"])
        assert torch.allclose(c["tokens"][i], w["tokens"], rtol=1e-12, atol=1e-14)


def test_position_table():
    """style_ref.position_table is the oracle's table up to the last bit of a frequency: entry (p, d) within (p x f_d + 1) x 2^-22 of
    torch's fp32 table on this machine (two ulps of the angle, one of the sine), row 0 zero; printed: what the difference does to the
    K/V rows of the 512-token voice in float64 (the GPU test judges against position_table, see its docstring)."""
    n, H = 2001, g.H
    t, o = S.position_table(n, H), oconan.sinusoid_table(n, H, 0)
    assert t.dtype == torch.float64 and t.shape == o.shape == (n, H) and not t[0].any()
    half = H // 2
    freq = torch.exp(torch.arange(half, dtype=torch.float64) * -(np.log(10000.0) / (half - 1)))
    allow = (torch.arange(n, dtype=torch.float64)[:, None] * freq[None, :] + 1.0) * 2.0 ** -22
    d = (t - o.double()).abs()
    print(f"\n[style-vs-f64] position table against torch's: max |d| {float(d.max()):.3e} (row {int(d.amax(1).argmax())}), rows 1 .. 8 {float(d[1:9].max()):.3e}")
    assert bool((d <= torch.cat([allow, allow], 1)).all())
    m = S.long_voice_mel()
    a = S.style_reference(m, key=("long", 8))
    b = S.style_reference(m, key=("long", 8), exact_positions=True)
    assert torch.equal(a["ids"], b["ids"]) and torch.equal(a["style"], b["style"])
    rel = [float((a["kv"][l] - b["kv"][l]).norm() / b["kv"][l].norm()) for l in range(2)]
    print(f"[style-vs-f64] K/V rows of the 512-token voice, torch's table against position_table (float64): rel rms {rel[0]:.3e} {rel[1]:.3e}")
    assert max(rel) < 1e-5


# ------------------------------------------------------------------------------------------------------------ yardsticks
@pytest.mark.parametrize("name", list(S.CASES))
def test_bounds_follow_the_oracle(name):
    """The recorded ORACLE_FP32 figures are what the fp32 oracle gives against the float64 reference on the case's inputs: recomputed
    and printed; each recorded rms within a factor 1.25 of the recomputed one, each recorded max within a factor 2 (the largest single
    rounding scatters with the BLAS's summation order).  The clean oracle passes the bounds and the id check."""
    got, want, ids_ok, _ = _oracle_run(name)
    j = S.judge(got, want, g.BOUNDS[name])
    print(f"\n[style-vs-f64] fp32 oracle against float64, {name}: {len(ids_ok)} references")
    for t, y in S.worst(j).items():
        rec = g.ORACLE_FP32[name][t]
        print(f"  {t:8s}: rms {min(j['rms'][t]):.3e} .. {y[0]:.3e}, max {y[1]:.3e}   recorded {rec[0]:.3e} {rec[1]:.3e}   bounds {g.BOUNDS[name][t][0]:.3e} {g.BOUNDS[name][t][1]:.3e}")
        assert rec[0] / 1.25 <= y[0] <= rec[0] * 1.25, (name, t, y, rec)
        assert rec[1] / 2 <= y[1] <= rec[1] * 2, (name, t, y, rec)
    assert all(j["ok"]) and all(ids_ok), j


def test_bounds_follow_the_rule():
    g.test_bounds_follow_the_rule()


def test_band_and_unsafe_tokens():
    """BAND is 16 x the largest |fp32-oracle distance - float64 distance| over the cases (recomputed: the recorded MAX_DIST_ERR within
    a factor 1.25); with the reference alone, at most 1 % of a case's tokens are unsafe."""
    worst = 0.0
    for name in S.CASES:
        mels, _ = S.case_references(name)
        unsafe = tokens = 0
        low = np.inf
        for i, m in enumerate(mels):
            w = S.style_reference(m, torch.float64, key=(name, i))
            f = S.style_reference(m, torch.float32, key=(name, i))
            worst = max(worst, float((f["dist"].double() - w["dist"]).abs().max()))
            unsafe += int((w["margin"] < S.BAND).sum())
            tokens += w["margin"].shape[0]
            low = min(low, float(w["margin"].min()))
        print(f"\n[style-vs-f64] {name}: {unsafe} unsafe of {tokens} tokens, smallest margin {low:.4g} (band {S.BAND:.3g})")
        assert unsafe <= S.MAX_UNSAFE * tokens, (name, unsafe, tokens)
    print(f"[style-vs-f64] largest |d32 - d64| {worst:.3e}, recorded {S.MAX_DIST_ERR:.3e}")
    assert S.BAND == 16 * S.MAX_DIST_ERR and S.MAX_DIST_ERR / 1.25 <= worst <= S.MAX_DIST_ERR * 1.25


# ------------------------------------------------------------------------------------------------------------ the cases reach their forms
def test_cases_reach_their_launch_forms():
    """On 256 CUs the restated plan gives every case the configurations it lists; slot lists are never the identity; token counts and
    last groups of `long` are the ones the case is there for."""
    for name, c in S.CASES.items():
        assert set(S.call_kernels(c["lens"], 256)) == c["reach"], name
        assert c["slots"] != list(range(len(c["slots"]))) and len(set(c["slots"])) == len(c["slots"]) == len(c["lens"]) and max(c["slots"]) < c["max_slots"]
        assert max(c["lens"]) <= c["max_ref"]
    rows = lambda name: S.passes_of(S.CASES[name]["lens"])[0][0] * S.passes_of(S.CASES[name]["lens"])[0][1]
    assert (rows("edge_1992"), rows("tail_2104"), rows("one_997"), rows("wide_4040")) == (1992, 2104, 997, 4040)
    assert S.pick_cfg(1984, 512, 256) == S.C32_64 and S.pick_cfg(1985, 512, 256) == S.C64 and S.pick_cfg(992, 512, 256) == S.C32 and S.pick_cfg(993, 512, 256) == S.C32_64
    assert S.pick_cfg(4032, 256, 256) == S.C32_64 and S.pick_cfg(4033, 256, 256) == S.C64 and S.pick_cfg(2720, 160, 256) == S.C32 and S.pick_cfg(2721, 160, 256) == S.C32_64
    assert S.pick_cfg(8128, 80, 256) == S.C32_64 and S.pick_cfg(8129, 80, 256) == S.C64 and S.pick_cfg(4064, 80, 256) == S.C32
    assert S.tail_split(2104, 512, 31, 256, 256) == 8 and S.tail_split(1992, 512, 31, 256, 256) == 1      # 264 tiles; 256 tiles
    assert S.tail_split(2104, 512, 1, 256, 256) == 1                                                       # (8 K steps: no slice of 8)
    L = S.CASES["long"]["lens"]
    assert [S.tokens_of(x) for x in L] == [512, 1, 16, 17, 63, 64, 65, 127] and [(x - 1) % 4 + 1 for x in L] == [1, 1, 1, 2, 3, 4, 1, 1]
    assert S.tokens_of(S.LONG_VOICE) == 512 == S.CASES["long"]["max_ref"] // 4
    assert S.passes_of(S.CASES["passes"]["lens"]) == [(8, 64), (3, 9)]
    z = S.case_mels("zeros")
    assert not z[0][[5, 6, 7, 8, 100, 262]].any() and not z[0][40:44, 0].any() and z[0][40:44, 1:].all() and not z[1][131:].any() and z[1].shape[0] == 150


# ------------------------------------------------------------------------------------------------------------ the bounds discriminate
class _Over:
    """A module with some names replaced: what oracle.conan sees as `torch` / `F` while a change is in force."""

    def __init__(self, base, **over):
        self._base, self._over = base, over

    def __getattr__(self, name):
        return self._over[name] if name in self._over else getattr(self._base, name)


@contextlib.contextmanager
def _patched(**names):
    old = {k: getattr(oconan, k) for k in names}
    try:
        for k, v in names.items():
            setattr(oconan, k, v)
        yield
    finally:
        for k, v in old.items():
            setattr(oconan, k, v)


def _partial_group_over_four():
    """The last partial group of a reference divided by 4 instead of its frame count.  With the straight-through quantiser everything
    behind it depends on the encoder's output only through the id, so a wrong group shows as a changed id and as nothing else: judge()
    passes every slot (measured: 0 of 9 fail), check_ids fails 6 of the 9 references of `long` - which is why the GPU test holds the
    ids exact on safe tokens."""
    def group(h, seg_ids, max_len):
        h_g, cnt = _REAL["group"](h, seg_ids, max_len)
        return h_g * torch.clamp(cnt[:, :, None], min=1) / 4.0, cnt
    return _patched(group_hidden_by_segs=group)


def _first_64_keys():
    """Attention over the first 64 keys only."""
    def layer(sd, p, src, mem, key_padding_mask, nhead=2):
        out, attn = _REAL["xattn"](sd, p, src, mem[:64], None if key_padding_mask is None else key_padding_mask[:, :64], nhead)
        return out, torch.nn.functional.pad(attn, (0, mem.shape[0] - attn.shape[-1]))
    return _patched(cross_atten_layer=layer)


def _style_mean_one_short():
    """The style mean over len - 1 frames: the sum of ALL frames divided by len - 1 instead of len (a single frame: unchanged).  Every
    torch.div that oracle.conan calls is replaced while the change is in force; temporal_avg_pool's is the only one."""
    def div(z, n):
        return torch.div(z, torch.clamp(n - 1, min=1))
    return _patched(torch=_Over(torch, div=div))


def _two_limbs(x):
    hi = x.bfloat16().float()
    return hi + (x - hi).bfloat16().float()          # round-to-nearest-even limbs, as the limb kernels split


def _two_limb_conv():
    """Every product of one conv - the global encoder's post_net1 (256 -> 256, k = 3), the last layer in front of the style mean -
    formed from two bf16 limbs per operand instead of fp32's three."""
    import torch.nn.functional as F

    def conv1d(x, w, b=None, **kw):
        if tuple(w.shape) == (g.H, g.H, 3) and kw.get("padding") == 1 and x.dtype == torch.float32:
            x, w = _two_limbs(x), _two_limbs(w)
        return F.conv1d(x, w, b, **kw)
    return _patched(F=_Over(F, conv1d=conv1d))


def _displace_kv_row(row, res):
    """One K/V row displaced by a row: token 5 of layer 1 holds token 6's row (the longest reference only)."""
    if row == 0:
        res["kv"][1][5] = res["kv"][1][6].clone()


_REAL = {"group": oconan.group_hidden_by_segs, "xattn": oconan.cross_atten_layer}
MUTATIONS = {
    "last_partial_group_over_4": (_partial_group_over_four, None),
    "attention_over_the_first_64_keys": (_first_64_keys, None),
    "style_mean_over_len_minus_1": (_style_mean_one_short, None),
    "kv_row_displaced": (None, _displace_kv_row),
    "conv_products_two_bf16_limbs": (_two_limb_conv, None),
}


@pytest.mark.parametrize("change", list(MUTATIONS))
def test_bounds_catch_a_deliberate_change(change):
    """The GPU test's checks - judge() with its bounds, check_ids - fail the fp32 oracle with one deliberate change on the `long` case
    (the unmodified oracle passes: test_bounds_follow_the_oracle).  The change is real and it is undone afterwards."""
    name = "long"
    mutate, tamper = MUTATIONS[change]
    before = (oconan.group_hidden_by_segs, oconan.cross_atten_layer, oconan.torch, oconan.F)
    clean, want, _, _ = _oracle_run(name)
    got, want2, ids_ok, _ = S.oracle_run(name, mutate=mutate, tamper=tamper)
    assert (oconan.group_hidden_by_segs, oconan.cross_atten_layer, oconan.torch, oconan.F) == before
    j = S.judge(got, want2, g.BOUNDS[name])
    moved = [t for t in S.TENSORS if any(not torch.equal(a, b) for a, b in zip(got[t], clean[t]))]
    print(f"\n[style-vs-f64] {change}: moved {moved}; slots failed {sum(not o for o in j['ok'])} of {len(j['ok'])}, id checks failed {sum(not o for o in ids_ok)}")
    for t, (r, m) in S.worst(j).items():
        print(f"  {t:8s}: rms {r:.3e} (bound {g.BOUNDS[name][t][0]:.3e}), max {m:.3e} (bound {g.BOUNDS[name][t][1]:.3e})")
    assert moved
    assert not (all(j["ok"]) and all(ids_ok))
    if change == "last_partial_group_over_4":
        # only references whose last group is partial are touched: the 256-frame one (a last group of 4) passes
        assert j["ok"][5] and ids_ok[5] and not all(ids_ok)
    if change == "attention_over_the_first_64_keys":
        # ... and only slots with more than 64 tokens
        assert [j["ok"][i] for i in (1, 2, 3, 4, 5)] == [True] * 5 and not j["ok"][0] and not j["ok"][6]
