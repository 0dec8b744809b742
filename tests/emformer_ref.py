"""Float64 reference of the streaming Emformer step for the GPU sweep (tests/test_gpu_emformer_f64.py), the error statistics that
sweep asserts (judge) and the ring arithmetic that sizes its schedules.  Plain helpers, no fixtures: tests/test_emformer_ref_cpu.py
pins the reference to oracle/emformer.py (the streaming recursion and the whole-sequence formulation).

The arithmetic is torchaudio's Emformer.infer as oracle/emformer.py restates it (_EmformerImpl.infer / _EmformerLayer.infer /
_EmformerAttention.infer), then `proj` and arg-max, with torch.matmul / softmax / layer_norm in float64 on the input's device.
Weights are the fp32 checkpoint tensors widened to float64: library and reference multiply the same bits.

Unlike the oracle - whose batch shares one past_length - every stream carries its OWN state: the left-context keys and values, the
past length and the per-layer memory bank, per slot.  Streams at different positions are batched in one call: every slot keeps
left_context_length key rows and max_memory_size bank rows (newest last), and the rows a stream does not have yet are masked with
-inf before the softmax, whose float64 exp gives them a weight of exactly 0 - the same numbers as leaving them out."""
import math

import torch
import torch.nn.functional as F

NEG_INF = -1e8          # torchaudio's negative_inf: what the summary query's memory columns are filled with


class EmformerRef:
    """Per-slot float64 state of `slots` streams.  sd: torch state dict (oracle.common.to_torch_sd), cfg: oracle.emformer.EmformerCfg."""

    def __init__(self, sd, cfg, slots, device="cpu"):
        self.cfg, self.dev = cfg, torch.device(device)
        self.sd = {k: v.to(self.dev, torch.float64) for k, v in sd.items()}
        D, LC, M, L = cfg.input_dim, cfg.left_context_length, cfg.max_memory_size, cfg.num_layers
        z = lambda rows: [torch.zeros(slots, rows, D, dtype=torch.float64, device=self.dev) for _ in range(L)]
        self.k, self.v, self.bank = z(LC), z(LC), z(M)          # newest row last
        self.past = torch.zeros(slots, dtype=torch.long, device=self.dev)

    def reset(self, slots):
        """A reset slot starts its utterance again: no left context, no bank, past length 0."""
        idx = torch.as_tensor(list(slots), dtype=torch.long, device=self.dev)
        for t in self.k + self.v + self.bank:
            t[idx] = 0.0
        self.past[idx] = 0

    def _lin(self, x, name):
        return torch.matmul(x, self.sd[name + ".weight"].t()) + self.sd[name + ".bias"]

    def _ln(self, x, name):
        return F.layer_norm(x, (x.shape[-1],), self.sd[name + ".weight"], self.sd[name + ".bias"], 1e-5)

    def _layer(self, l, idx, utt, rc, mems, past):
        """_EmformerLayer.infer for the streams idx: utt [n, U, D], rc [n, R, D], mems [n, 1, D] this step's memory input (appended to
        the bank AFTER the attention has read the bank as it was).  -> (utt, rc, the next layer's memory input)."""
        c = self.cfg
        D, H, LC, M, U, R = c.input_dim, c.num_heads, c.left_context_length, c.max_memory_size, utt.shape[1], rc.shape[1]
        p = f"emformer.emformer_layers.{l}"
        n = utt.shape[0]
        ln_utt, ln_rc = self._ln(utt, p + ".layer_norm_input"), self._ln(rc, p + ".layer_norm_input")
        lc_k, lc_v = self.k[l][idx], self.v[l][idx]
        q_in, kv_in = [ln_rc, ln_utt], [ln_rc, ln_utt]
        if M > 0:
            q_in.append(ln_utt.mean(1, keepdim=True))      # memory_op: AvgPool1d(kernel = stride = segment_length) of the normalised segment
            kv_in.insert(0, self.bank[l][idx])
        q = self._lin(torch.cat(q_in, 1), p + ".attention.emb_to_query")
        k, v = self._lin(torch.cat(kv_in, 1), p + ".attention.emb_to_key_value").chunk(2, -1)
        k = torch.cat([k[:, :M + R], lc_k, k[:, M + R:]], 1)       # keys [bank | rc | left context | utt]
        v = torch.cat([v[:, :M + R], lc_v, v[:, M + R:]], 1)
        T, nk, dh = q.shape[1], k.shape[1], D // H
        # the rows a stream has: the newest min(M, ceil(past / segment)) bank entries and min(LC, past) left-context keys
        have_mem = torch.minimum(torch.full_like(past, M), (past + c.segment_length - 1) // c.segment_length)
        have_lc = past.clamp(max=LC)
        col = torch.arange(nk, device=self.dev)
        valid = torch.ones(n, nk, dtype=torch.bool, device=self.dev)
        valid &= ~((col < M) & (col < (M - have_mem)[:, None]))
        valid &= ~((col >= M + R) & (col < M + R + LC) & (col < (M + R + LC - have_lc)[:, None]))
        heads = lambda t: t.reshape(n, t.shape[1], H, dh).transpose(1, 2)          # [n, H, rows, dh]
        w = torch.matmul(heads(q) * dh ** -0.5, heads(k).transpose(-1, -2))        # [n, H, T, nk]
        if M > 0:
            w[:, :, -1, :M] = NEG_INF                      # the summary query does not see the memory columns
        w = w.masked_fill(~valid[:, None, None, :], -math.inf)
        att = torch.matmul(torch.softmax(w, -1), heads(v)).transpose(1, 2).reshape(n, T, D)
        out = self._lin(att, p + ".attention.out_proj")
        next_mems = None
        if M > 0:
            out, s = out[:, :-1], out[:, -1:]
            next_mems = torch.tanh(s) if c.tanh_on_mem else s.clamp(-10, 10)
            self.bank[l][idx] = torch.cat([self.bank[l][idx], mems], 1)[:, -M:]
        self.k[l][idx] = k[:, M + R:][:, -LC:]             # left context | utt, the newest LC rows
        self.v[l][idx] = v[:, M + R:][:, -LC:]
        res = out + torch.cat([rc, utt], 1)
        ff = self._ln(res, p + ".pos_ff.0")
        ff = self._lin(torch.relu(self._lin(ff, p + ".pos_ff.1")), p + ".pos_ff.4")
        res = self._ln(ff + res, p + ".layer_norm_output")
        return res[:, R:], res[:, :R], next_mems

    @torch.no_grad()
    def step(self, slots, chunk):
        """One chunk [n, segment + right_context, D] (utterance rows first) for the streams `slots`, each from its own position.
        -> (out [n, segment, D], logits [n, segment, K], codes [n, segment]), float64 / int64."""
        c = self.cfg
        U, R = c.segment_length, c.right_context_length
        idx = torch.as_tensor(list(slots), dtype=torch.long, device=self.dev)
        assert chunk.shape == (len(idx), U + R, c.input_dim), chunk.shape
        x = chunk.to(self.dev, torch.float64)
        utt, rc = x[:, :U], x[:, U:]
        past = self.past[idx]
        mems = utt.mean(1, keepdim=True) if c.max_memory_size > 0 else None       # layer 0: the mean of the raw segment
        for l in range(c.num_layers):
            utt, rc, mems = self._layer(l, idx, utt, rc, mems, past)
        self.past[idx] = past + U
        head = "proj1" if "proj1.weight" in self.sd else "proj"
        logits = self._lin(utt, head) if head + ".weight" in self.sd else utt
        return utt, logits, logits.argmax(-1)


# ------------------------------------------------------------------------------------------------------------ judging
def judge(got, want, bounds):
    """The error statistics of slot-runs (a slot-run: one slot from a reset to its next reset), per run and tensor.
    got = (out [r, frames, D], logits [r, frames, K], codes [r, frames]) as the code under test gave them (fp32 / any int),
    want = (out, logits) float64 of the reference, bounds = {"out": (rms bound, max bound), "logits": (rms bound, max bound)}.
    Per run and tensor: the relative rms error |e|_2 / |want|_2, and the largest |e| over the run's rms of want.  Codes must equal
    the reference's arg-max wherever the reference's top-2 logit margin exceeds twice the largest logit error the max bound allows
    (absolute: the bound times the run's logits rms) - closer frames may flip within the bounds and are excluded and counted.
    -> {"rms": {tensor: [r]}, "max": {tensor: [r]}, "finite": [r], "excluded": [r] frames left out of the code comparison,
        "wrong_codes": [r] compared frames whose code differs, "frames": frames per run, "ok": [r]} (CPU tensors)."""
    res = {"rms": {}, "max": {}}
    dev = want[0].device
    ok = torch.ones(want[0].shape[0], dtype=torch.bool, device=dev)
    fin = torch.ones_like(ok)
    run_rms = {}
    for name, g, w in (("out", got[0], want[0]), ("logits", got[1], want[1])):
        assert w.dtype == torch.float64 and g.shape == w.shape, (name, w.dtype, g.shape, w.shape)
        g = g.to(dev)
        e = g.double() - w
        run_rms[name] = w.pow(2).mean((1, 2)).sqrt()
        res["rms"][name] = e.pow(2).sum((1, 2)).sqrt() / w.pow(2).sum((1, 2)).sqrt()
        res["max"][name] = e.abs().amax((1, 2)) / run_rms[name]
        fin &= torch.isfinite(g).flatten(1).all(1)
        ok &= (res["rms"][name] <= bounds[name][0]) & (res["max"][name] <= bounds[name][1])
    top2 = want[1].topk(2, -1)
    margin = top2.values[..., 0] - top2.values[..., 1]
    safe = margin > (2.0 * bounds["logits"][1] * run_rms["logits"])[:, None]
    differs = got[2].to(dev).long() != top2.indices[..., 0]
    res["excluded"] = (~safe).sum(1)
    res["wrong_codes"] = (differs & safe).sum(1)
    res["finite"] = fin
    res["frames"] = want[0].shape[1]
    res["ok"] = ok & fin & (res["wrong_codes"] == 0)
    for k in ("rms", "max"):
        res[k] = {n: t.cpu() for n, t in res[k].items()}
    for k in ("excluded", "wrong_codes", "finite", "ok"):
        res[k] = res[k].cpu()
    return res


# ------------------------------------------------------------------------------------------------------------ rings
def kv_ring_rows(left_context, segment):
    """Rows of a layer's K / V ring per slot (streams.hip build_emformer): next_pow2(left_context_length + segment_length)."""
    return 1 << (left_context + segment - 1).bit_length()


def steps_to_wrap_twice(left_context, segment):
    """Steps of `segment` rows after which the K / V ring has wrapped at least twice."""
    return math.ceil(2 * kv_ring_rows(left_context, segment) / segment)
