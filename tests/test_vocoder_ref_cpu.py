"""The float64 references of tests/vocoder_ref.py against oracle/hifigan.py (resblock1, _cconv, pixel_shuffle_1d - pinned to the
reference goldens by tests/test_oracle_golden.py), the oracle run STATEFULLY over uneven steps (5 + 1 + 6 rows) while the helper
evaluates the whole run at once: to 1e-12 of the output's largest value, at small widths, on the CPU.  Plus causality (changing later
rows leaves the earlier outputs bit-identical), the weight fold against the oracle's weight-norm, and the ring arithmetic."""
import numpy as np
import torch

from conan_amd import configs, synth
from tests import vocoder_ref as vr
from tests.test_gpu_arith import _fold

STEPS = ((0, 5), (5, 6), (6, 12))           # uneven steps of one 12-row run


def _small():
    """The shipped vocoder's topology at an initial width of 32 (stage widths 16 / 8 / 4 / 2): raw (weight-norm) and folded state dicts."""
    vhp = dict(configs.hifigan_hparams(), upsample_initial_channel=32)
    sd = synth.hifigan_state_dict(vhp, 3)
    raw = {k: torch.from_numpy(v).double() for k, v in sd.items()}
    folded = {k: torch.from_numpy(v).double() for k, v in _fold(sd).items()}
    return vhp, raw, folded


def _close(got, want, tol):
    assert got.dtype == torch.float64 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=0, atol=tol * float(want.abs().max()))


def test_ref_stage_matches_the_oracle_streamed():
    from oracle import hifigan as ohifi
    vhp, raw, folded = _small()
    nb = len(vhp["resblock_kernel_sizes"])
    rng = np.random.default_rng(1)
    for stage, c in enumerate((16, 8, 4, 2)):
        x = torch.from_numpy(rng.standard_normal((3, 12, c)).astype(np.float32))
        got = vr.ref_stage(x, folded, stage, vhp)
        for sdo, tol in ((folded, 1e-12), (raw, 1e-6)):             # the same fold; the oracle's own weight-norm of the raw checkpoint
            st, parts = {}, []
            for p, q in STEPS:
                xc = x[:, p:q].double().transpose(1, 2)
                acc = 0
                for j in range(nb):
                    acc = acc + ohifi.resblock1(sdo, stage * nb + j, xc, vhp["resblock_dilation_sizes"][j], st)
                parts.append(torch.nn.functional.leaky_relu(acc / nb, ohifi.LRELU_SLOPE))
            _close(got, torch.cat(parts, 2).transpose(1, 2), tol)
        x2 = x.clone()
        x2[:, 6:] += 1.0
        assert torch.equal(vr.ref_stage(x2, folded, stage, vhp)[:, :6], got[:, :6])
        assert not torch.equal(vr.ref_stage(x2, folded, stage, vhp)[:, 6:], got[:, 6:])


def test_ref_stage_chunks_do_not_change_the_result(monkeypatch):
    vhp, _, folded = _small()
    x = torch.from_numpy(np.random.default_rng(2).standard_normal((5, 12, 16)).astype(np.float32))
    whole = vr.ref_stage(x, folded, 0, vhp)
    monkeypatch.setattr(vr, "_CHUNK_ELEMS", 2 * 12 * 11 * 16)          # two slots per chunk: 2 + 2 + 1
    assert torch.equal(vr.ref_stage(x, folded, 0, vhp), whole)
    assert torch.equal(vr.ref_conv_post(x[:, :, :2].contiguous(), folded), vr.ref_conv_post(x[:, :, :2].contiguous(), folded))


def test_ref_conv_pre_and_conv_post_match_the_oracle_streamed():
    from oracle import hifigan as ohifi
    vhp, raw, folded = _small()
    mel = torch.from_numpy(synth.mel(12, 5, 3))
    x = torch.from_numpy(np.random.default_rng(4).standard_normal((3, 12, 2)).astype(np.float32))
    got_pre, got_post = vr.ref_conv_pre(mel, folded), vr.ref_conv_post(x, folded)
    assert got_pre.shape == (3, 12, 32) and got_post.shape == (3, 12, 1)
    for sdo, tol in ((folded, 1e-12), (raw, 1e-6)):
        st, pre, post = {}, [], []
        for p, q in STEPS:
            pre.append(torch.nn.functional.leaky_relu(ohifi._cconv(sdo, "conv_pre.conv", mel[:, p:q].double().transpose(1, 2), 1, st), ohifi.LRELU_SLOPE))
            post.append(ohifi._cconv(sdo, "conv_post.conv", x[:, p:q].double().transpose(1, 2), 1, st))
        _close(got_pre, torch.cat(pre, 2).transpose(1, 2), tol)
        _close(got_post, torch.cat(post, 2).transpose(1, 2), tol)
    mel2, x2 = mel.clone(), x.clone()
    mel2[:, 6:] += 1.0
    x2[:, 6:] += 1.0
    assert torch.equal(vr.ref_conv_pre(mel2, folded)[:, :6], got_pre[:, :6])
    assert torch.equal(vr.ref_conv_post(x2, folded)[:, :6], got_post[:, :6])


def test_ref_upsampler_matches_the_oracle_over_uneven_steps():
    """ups.2 / ups.3 of the small model (8 and 4 taps, shuffle 4 and 2) on the stage output that feeds them."""
    from oracle import hifigan as ohifi
    vhp, raw, folded = _small()
    rng = np.random.default_rng(6)
    for i, cin in ((2, 8), (3, 4)):
        r = vhp["upsample_rates"][i]
        x = torch.from_numpy(rng.standard_normal((3, 12, cin)).astype(np.float32))
        name = f"ups.{i}.conv.conv"
        got = vr.ref_upsampler(x, folded[name + ".weight"], folded[name + ".bias"], r)
        for sdo, tol in ((folded, 1e-12), (raw, 1e-6)):
            st = {}
            ys = [ohifi._cconv(sdo, name, x[:, p:q].double().transpose(1, 2), 1, st) for p, q in STEPS]
            _close(got, ohifi.pixel_shuffle_1d(torch.cat(ys, 2), r).transpose(1, 2), tol)


def test_slot_errors_sees_one_wrong_slot_only():
    want = torch.from_numpy(np.random.default_rng(7).standard_normal((4, 20, 3)))
    got = want.float()
    got[2, 5] = got[2, 4]                                              # one row of slot 2 repeated
    rms, mx, fin = vr.slot_errors(got, want)
    assert bool(fin.all()) and float(rms[2]) > 1e-2 and float(mx[2]) > 0.1
    assert all(float(rms[i]) < 1e-7 and float(mx[i]) < 1e-6 for i in (0, 1, 3))
    got[1, 0, 0] = float("nan")
    assert vr.slot_errors(got, want)[2].tolist() == [True, False, True, True]


def test_rings_and_schedule_lengths():
    """mk_ring's arithmetic and the rings of the shipped vocoder (streams.hip build_vocoder): conv_pre's output keeps 15 rows, the
    fused stages' unit outputs (11 - 1) x (5 + 1) = 60; a 4-frame step of a max_frames = 4 set wraps conv_pre's 32-row ring twice
    in 16 steps; the ups.0 / ups.1 default (tests/test_gpu_conv_tall.py) is unchanged."""
    vhp = configs.hifigan_hparams()
    assert vr.vocoder_rings(vhp) == ((15, 1), (60, 8), (60, 40), (60, 160), (60, 320))
    assert vr.ring_rows(15, 1, 4) == 32 and vr.ring_rows(60, 8, 4) == 128 and vr.ring_rows(60, 320, 4) == 2048 and vr.ring_rows(60, 8, 16) == 256
    rings = vr.vocoder_rings(vhp)
    assert vr.steps_to_wrap_twice(4, 4, rings) == 16 and vr.steps_to_wrap_twice(1, 1, rings) == 32 and vr.steps_to_wrap_twice(3, 4, rings) == 22
    assert vr.steps_to_wrap_twice(16, 16, rings, least=6) == 6 and vr.steps_to_wrap_twice(12, 12, rings, least=6) == 6
    assert vr.steps_to_wrap_twice(4, 4) == 16 and vr.steps_to_wrap_twice(2, 2) == 32 and vr.steps_to_wrap_twice(1, 1) == 32 and vr.steps_to_wrap_twice(3, 4) == 22
    for frames, mf in ((4, 4), (1, 1), (2, 2), (3, 4), (16, 16), (12, 12)):
        steps = vr.steps_to_wrap_twice(frames, mf, rings, least=6)
        assert all(steps * frames * rate >= 2 * vr.ring_rows(h, rate, mf) for h, rate in rings)
