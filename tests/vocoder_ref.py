"""Float64 references of the vocoder's operators for the GPU sweeps (tests/test_gpu_conv_tall.py, tests/test_gpu_vocoder_f64.py),
and the ring arithmetic that sizes their schedules.  Plain helpers, no fixtures: tests/test_vocoder_ref_cpu.py pins every one of
them to oracle/hifigan.py (which tests/test_oracle_golden.py pins to the reference goldens).

Every reference takes the tensor its kernel READ since the slot's reset, [n, rows, C], with zero history in front of every
convolution (a reset zeroes the rings), and evaluates im2col x weight matrix with torch.matmul on that tensor's device in float64,
in slot chunks - no float64 conv1d, which the GPU back end need not have.  Weights are the host-folded fp32 tensors
(tests/test_gpu_arith._fold) widened to float64: library and reference multiply the same bits."""
import math

import torch

LRELU_SLOPE = 0.1           # hifigan_causal.py:20
_CHUNK_ELEMS = 1 << 25      # largest im2col matrix (elements) of one slot chunk


def _cconv(x, w, b, dil=1):
    """Causal dilated convolution in float64: x [n, rows, Cin] (float64), w [Cout, Cin, k], b [Cout] -> [n, rows, Cout]; (k - 1) x dil
    zero rows in front."""
    n, rows, cin = x.shape
    cout, _, k = w.shape
    w, b = w.to(x.device, torch.float64), b.to(x.device, torch.float64)
    wm = w.permute(2, 1, 0).reshape(k * cin, cout)                      # [(tap, channel), Cout]
    xp = torch.nn.functional.pad(x, (0, 0, (k - 1) * dil, 0))
    cols = torch.stack([xp[:, j * dil:j * dil + rows] for j in range(k)], 2).reshape(n, rows, k * cin)
    return torch.matmul(cols, wm) + b


def _chunks(n, rows, k, cin):
    step = max(1, _CHUNK_ELEMS // max(1, rows * k * cin))
    return [(s, min(n, s + step)) for s in range(0, n, step)]


def ref_upsampler(x, w, b, r, dil=1):
    """What one causal pixel-shuffle upsampler (hifigan_causal.py:191-212) writes, in float64: x [n, rows, Cin] is the tensor it
    read over consecutive steps from a slot's reset on ((k - 1) x dil rows of zero history in front), w [Cout, Cin, k] the folded
    weight, b [Cout] -> [n, rows x r, Cout / r].  im2col of the causal window times the weight matrix (torch.matmul, on x's device),
    then oracle.hifigan.pixel_shuffle_1d; done in slot chunks that keep the im2col matrix below 2^25 elements."""
    from oracle import hifigan as ohifi
    n, rows, cin = x.shape
    k = w.shape[2]
    out = []
    for p, q in _chunks(n, rows, k, cin):
        y = _cconv(x[p:q].double(), w, b, dil)                          # [n, rows, Cout]
        out.append(ohifi.pixel_shuffle_1d(y.transpose(1, 2), r).transpose(1, 2))
    return torch.cat(out)


def ref_stage(x, sd64, stage, vhp):
    """leaky_relu(mean_j ResBlock1_j(x), 0.1) of MRF stage `stage` (hifigan_causal.py:230-238, :324-331) in float64: x [n, rows, C] is
    what the stage read since the slot's reset (the upsampler's output), sd64 the folded state dict ('resblocks.<idx>.convs1.<d>.conv
    .weight' / '.bias', torch tensors), -> [n, rows, C].  Every conv of every unit sees zero history of ITS OWN input (the rings of a
    reset slot), which is what a whole-run causal convolution with zero left padding computes."""
    ks, dils = vhp["resblock_kernel_sizes"], vhp["resblock_dilation_sizes"]
    nb = len(ks)
    n, rows, c = x.shape
    lrelu = torch.nn.functional.leaky_relu
    out = []
    for p, q in _chunks(n, rows, max(ks), c):
        x0 = x[p:q].double()
        acc = torch.zeros_like(x0)
        for j in range(nb):
            idx = stage * nb + j
            y = x0
            for d_i, d in enumerate(dils[j]):
                pre = f"resblocks.{idx}.convs"
                xt = _cconv(lrelu(y, LRELU_SLOPE), sd64[f"{pre}1.{d_i}.conv.weight"], sd64[f"{pre}1.{d_i}.conv.bias"], d)
                xt = _cconv(lrelu(xt, LRELU_SLOPE), sd64[f"{pre}2.{d_i}.conv.weight"], sd64[f"{pre}2.{d_i}.conv.bias"], 1)
                y = y + xt
            acc = acc + y
        out.append(lrelu(acc / nb, LRELU_SLOPE))
    return torch.cat(out)


def ref_conv_pre(mel, sd64):
    """leaky_relu(conv_pre(mel), 0.1) in float64 (hifigan_causal.py:319-321; the library stores conv_pre's output activated):
    mel [n, frames, 80] -> [n, frames, C0]."""
    w, b = sd64["conv_pre.conv.weight"], sd64["conv_pre.conv.bias"]
    n, rows, c = mel.shape
    return torch.cat([torch.nn.functional.leaky_relu(_cconv(mel[p:q].double(), w, b), LRELU_SLOPE) for p, q in _chunks(n, rows, w.shape[2], c)])


def ref_conv_post(x, sd64):
    """conv_post on the last stage's (already activated) output, before the tanh (hifigan_causal.py:329-333), in float64:
    x [n, rows, C] -> [n, rows, 1]."""
    w, b = sd64["conv_post.conv.weight"], sd64["conv_post.conv.bias"]
    n, rows, c = x.shape
    return torch.cat([_cconv(x[p:q].double(), w, b) for p, q in _chunks(n, rows, w.shape[2], c)])


def slot_errors(got, want):
    """Per slot of got [n, rows, C] (fp32) against want (float64): relative rms error, largest |error| / the slot's rms of that
    channel, and whether got is finite."""
    got = got.to(want.device)
    e = got.double() - want
    rms = e.pow(2).sum((1, 2)).sqrt() / want.pow(2).sum((1, 2)).sqrt()
    crms = want.pow(2).mean(1, keepdim=True).sqrt().clamp_min(1e-300)
    mx = (e.abs() / crms).amax((1, 2))
    fin = torch.isfinite(got).flatten(1).all(1)
    return rms.cpu(), mx.cpu(), fin.cpu()


# ------------------------------------------------------------------------------------------------------------ rings
def ring_rows(hist, rate, max_frames):
    """Rows of a vocoder ring (streams.h mk_ring): next_pow2(hist + max_frames x rate)."""
    return 1 << (hist + max_frames * rate - 1).bit_length()


# (history rows, rows per frame) of the rings ups.0 / ups.1 read: conv_pre's ring (15 rows of history, rate 1) and stage 0's branch
# mean (9 rows, rate 8)
UPS01_RINGS = ((15, 1), (9, 8))


def vocoder_rings(vhp):
    """(history rows, rows per frame) of every ring a matrix kernel of the vocoder step reads, the longest history per rate
    (streams.hip build_vocoder, :431-502; a ring's length grows with its history, so the longest one per rate wraps last): the mel
    ring (6), conv_pre's output (k_ups0 - 1); per stage the upsampler's output `up` ((k - 1) x (dil_0 + 1) in the fused plan), the
    unit outputs `xo` ((k - 1) x (dil_next + 1)), c1's output `xt` (k - 1) and the branch mean `xs` (the next upsampler's k - 1,
    conv_post's 6)."""
    kmax = max(vhp["resblock_kernel_sizes"])
    dmax = max(max(d) for d in vhp["resblock_dilation_sizes"])
    rings = [(max(6, vhp["upsample_kernel_sizes"][0] - 1), 1)]
    rate = 1
    for i, r in enumerate(vhp["upsample_rates"]):
        rate *= r
        nxt = vhp["upsample_kernel_sizes"][i + 1] - 1 if i + 1 < len(vhp["upsample_rates"]) else 6
        rings.append((max((kmax - 1) * (dmax + 1), nxt), rate))
    return tuple(rings)


def steps_to_wrap_twice(frames, max_frames, rings=UPS01_RINGS, least=12):
    """Steps of `frames` frames after which every ring of `rings` has wrapped at least twice (at least `least`).  The default rings
    are the inputs of ups.0 / ups.1; vocoder_rings() gives those of the whole vocoder step."""
    need = least
    for hist, rate in rings:
        need = max(need, math.ceil(2 * ring_rows(hist, rate, max_frames) / (frames * rate)))
    return need
