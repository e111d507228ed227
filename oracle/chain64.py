"""TEST INFRASTRUCTURE ONLY — float64 restatement of the text side's forward, differentiated by autograd, as the reference of the
hand-written backward launch sequences (encoder_impl.layer_bwd / mha_bwd / crn_bwd / dp_bwd / _sum_grads_to_bf16,
text_models._TextEncoderRunner.backward / _DurationRunner.backward, attentions._EncoderRunner.backward).

Four pieces on [B, C, T] float64 tensors, parameters in a dict keyed by the reference's state_dict names (as oracle/glowtts_ref.py):

  layer          one attentions.Encoder layer: rel-pos MHA, LayerNorm, FFN, LayerNorm       (encoder_impl.layer_fwd)
  prenet         modules.ConvReluNorm                                                        (encoder_impl.crn_fwd)
  duration       models.DurationPredictor                                                    (encoder_impl.dp_fwd)
  text_encoder   embedding * sqrt(C), language vector in the last lin columns, prenet, layers with the speaker vector added before
                 layer COND_LAYER, proj_m / proj_s                                           (text_models._TextEncoderRunner.forward)
  encoder        the stand-alone attentions.Encoder                                          (attentions._EncoderRunner.forward)

LayerNorm is glowtts_ref.layer_norm_c; the attention core restates glowtts_ref.mha_fwd's band form with hooks on q, k, v, P and o
(tests/test_chain64.py pins it to glowtts_ref.encoder_fwd).  Dropout masks are the {site: keep * scale} dicts of oracle/dropmask.py,
under glowtts_ref's site names.  The residual stream is masked after every LayerNorm, as the kernels do; on valid frames and in every
gradient that is the reference's arithmetic (padded frames reach nothing: keys are masked, every conv masks its input).

Every kernel boundary goes through Hooks.force(key, value), every ReLU through Hooks.relu, every edge on which a backward chain stores
a gradient through Hooks.store.  The hooks select the mode:

  exact    force = identity (it records the value: Hooks.seen), ReLU = pre > 0, store = identity.
  forced   teacher forcing: force(key, v) = v + (saved[key] - v).detach() on the valid frames, so the graph stays connected and
           everything downstream is evaluated at the kernels' own activation; a ReLU unit is on where the saved post-ReLU (post-dropout)
           tensor is non-zero.  Dropout masks still come from dropmask (the reference stays independent of the kernels' draw); every
           dropped position of the saved tensor must be zero (asserted).
  twin     forced, and store(key, v, dtype) is an identity whose backward rounds the gradient to `dtype` (bf16 through fp32, or fp32):
           the storage of the intermediate gradients, modelled exactly.  The rounded gradient is kept in Hooks.stored[key].
           Hooks.operand(key, v, dtype) rounds a saved VALUE that a backward kernel re-reads in a narrower dtype (one site).

Storage sites (key suffix: dtype, where the chain stores it):
  layer   df2 bf16, dx1 fp32    encoder_impl.py:189  (_ln_bwd of norm_2: dy, da)
          dc1 bf16              encoder_impl.py:192  (dgrad of conv_2, gate = 3 epilogue)
          dxb1 bf16             encoder_impl.py:194
          dy bf16, dx0 fp32     encoder_impl.py:195  (_ln_bwd of norm_1: dy, da)
          do bf16               encoder_impl.py:147
          dq, dk, dv bf16       encoder_impl.py:150-160 (dqkv, written by gt_attn_bwd)
          dS bf16               encoder_impl.py:154-160: the workspace of gt_attn_bwd / gt_attn_bwd_stats holds dS^T (the factor
                                1 / sqrt(dk) included) as bf16 between the kernels' two passes; dq, dk and dEk are summed from it
                                (csrc/attn_mfma.hip:336, :458, :716; csrc/attn_long.hip:376)
          Pd bf16 (operand)     the same workspace holds dropout(P)^T as bf16; dv and dEv are summed from it (csrc/attn_mfma.hip:459,
                                :716; csrc/attn_long.hip:377).  Not a gradient: Hooks.operand rounds the VALUE the twin's Jacobians
                                see; d P flows unrounded, and the softmax backward reads the saved fp32 P
          dxb0 bf16             encoder_impl.py:166
  prenet  dpre bf16             encoder_impl.py:236  (_sum_grads_to_bf16, :227: bf16 of the masked fp32 sum)
          dx0 = copy of dpre    encoder_impl.py:237-238 (no rounding of its own: both branches read the bf16 dpre)
          dh.n bf16             encoder_impl.py:240
          dc.i bf16             encoder_impl.py:243  (_ln_bwd: dy)
          dh.i bf16             encoder_impl.py:246  (dh.0 is the returned dxb0)
  dp      db bf16               encoder_impl.py:269-270
          dh2 bf16              encoder_impl.py:274
          dr2 bf16              encoder_impl.py:275  (_ln_bwd with relu_in: dy)
          dh1 bf16              encoder_impl.py:277
          dr1 bf16              encoder_impl.py:278
          dx bf16               encoder_impl.py:280  (want_dx: what ops.cond_grad sums)
  text    d bf16                text_models.py:197   (dx_m)
          proj_m.dxb bf16       text_models.py:199   (proj_m's data gradient, stored before it is the addend)
          d2 bf16               text_models.py:201   (dx_logs)
          dxb bf16              text_models.py:203   (one rounding of the sum, after the addend epilogue)
          dx fp32               text_models.py:204   (dxo)
          tot fp32              text_models.py:215   (no rounding: fp32 sum of dx and dxb)
  encoder dx fp32               attentions.py:321;  tot fp32  attentions.py:327

Planted defects (Hooks(defects=...)), each a change of the reference's GRADIENT path only (forward values stay forced):
  "dx1_lost"          the residual into LayerNorm 2 detached
  "proj_s_addend"     xb into proj_s detached (the addend = dxb sum lost)
  "prenet_dxb"        the bf16-copy gradient ignored where the prenet's two streams meet
  "relu_in_norm_2"    the ReLU backward left out before norm_2 of the duration predictor
  "dvec_late"         the speaker vector's gradient taken one layer too late (after layer COND_LAYER - 1's backward)
  "lvec_shift"        the language vector's gradient read from columns shifted by one
  "proj_s_scale"      (value eps) the proj_s path scaled by 1 + eps: the resolution control
(the FFN-mask defect is a different `drop` dict, not a hook).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import rows64
from oracle.glowtts_ref import layer_norm_c

F64 = torch.float64
COND_LAYER = 2          # attentions.Encoder.COND_LAYER


def bf16_round(x):
    """bf16(fp32(x)) of a float64 tensor, as float64 (rows64.bf16_round)"""
    return torch.from_numpy(rows64.bf16_round(x.detach().numpy())).reshape(x.shape)


def _round(x, dtype):
    return bf16_round(x) if dtype == "bf16" else x.float().double()


class _RoundGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, dtype, sink, key):
        ctx.dtype, ctx.sink, ctx.key = dtype, sink, key
        return v.view_as(v)

    @staticmethod
    def backward(ctx, g):
        r = _round(g, ctx.dtype)
        ctx.sink[ctx.key] = r
        return r, None, None, None


class Hooks:
    def __init__(self, mode="exact", saved=None, defects=(), check_drop=True):
        assert mode in ("exact", "forced", "twin")
        assert (mode == "exact") == (saved is None)
        self.mode, self.saved, self.check_drop = mode, saved, check_drop
        self.defects = dict(defects) if isinstance(defects, dict) else {d: True for d in defects}
        self.seen, self.stored, self.used = {}, {}, set()

    def defect(self, name):
        return self.defects.get(name, False)

    def has(self, key):
        return self.mode != "exact" and key in self.saved

    def force(self, key, v, valid):
        """valid: what broadcasts to v, 1 where the saved tensor is defined (the frame mask)"""
        if self.mode == "exact":
            self.seen[key] = v.detach().clone()
            return v
        s = self.saved[key]
        assert s.shape == v.shape, (key, s.shape, v.shape)
        self.used.add(key)
        return v + ((s - v) * valid).detach()

    def relu(self, key, pre, keep=None):
        """key: the saved post-ReLU (post-dropout, masked) tensor; keep: bool, the kept units of the dropout behind the ReLU"""
        if self.mode == "exact":
            return torch.relu(pre)
        self.dropped_zero(key, keep)
        return pre * (self.saved[key] != 0).to(pre.dtype)

    def dropped_zero(self, key, keep):
        """the masks come from dropmask, never from the saved tensor; what it drops must be zero in the saved post-dropout tensor"""
        if self.mode != "exact" and keep is not None and self.check_drop:
            assert float((self.saved[key] * (~keep)).abs().max()) == 0.0, f"{key}: a dropped unit of the saved activation is not zero"

    def operand(self, key, v, dtype):
        """a saved activation that the backward kernels re-read in a narrower dtype: the twin's Jacobians take the rounded value"""
        if self.mode != "twin":
            return v
        return v + (_round(v, dtype) - v).detach()

    def store(self, key, v, dtype):
        if self.mode != "twin":
            return v
        return _RoundGrad.apply(v, dtype, self.stored, key)


# ----------------------------------------------------------------------------- rows <-> [B, C, T]
def unrows(lay, t):
    """rows [R, C] (any dtype; loss64.Layout geometry) -> float64 [B, C, T], zero where a frame is not valid"""
    t = rows64.t64(t)
    out = torch.zeros(lay.B, t.shape[1], lay.T, dtype=F64)
    for b in range(lay.B):
        r = lay.frame_rows(b)
        out[b, :, :len(r)] = t[torch.from_numpy(r)].T
    return out


def rows(lay, x):
    """[B, C, T] -> float64 rows [R, C], zero on halo / padded / rounding rows"""
    out = torch.zeros(lay.R, x.shape[1], dtype=F64)
    for b in range(lay.B):
        r = lay.frame_rows(b)
        out[torch.from_numpy(r)] = x[b, :, :len(r)].T.to(F64)
    return out


def frame_mask(lay):
    return torch.from_numpy((np.arange(lay.T)[None, :] < np.minimum(np.asarray(lay.lens), lay.T)[:, None]).astype(np.float64))[:, None, :]


def saved_layer(lay, s, tag, out=None):
    """what encoder_impl.layer_fwd saved -> {key: [B, C, T]} (P only where a dense P was saved)"""
    out = {} if out is None else out
    s_att, s_ln1, xb1, f1, s_ln2, _ = s
    xb, q, k, v, o, P = s_att[:6]
    for n, t in (("xb", xb), ("q", q), ("k", k), ("v", v), ("o", o), ("x", s_ln1[0]), ("ln1.y", s_ln1[1]), ("xb1", xb1), ("f1", f1),
                 ("ln2.a", s_ln2[0]), ("ln2.y", s_ln2[1])):
        out[tag + n] = unrows(lay, t)
    if isinstance(P, torch.Tensor):
        m = frame_mask(lay)
        am = (m.unsqueeze(2) * m.unsqueeze(-1)).bool()
        out[tag + "P"] = torch.where(am, P.detach().cpu().double(), torch.zeros((), dtype=F64))
    return out


def saved_prenet(lay, s, tag, out=None):
    out = {} if out is None else out
    saved, hlast = s
    for i, (h, s_ln) in enumerate(saved):
        out[tag + f"h.{i}"] = unrows(lay, h)
        out[tag + f"c.{i}"] = unrows(lay, s_ln[1])
    out[tag + f"h.{len(saved)}"] = unrows(lay, hlast)
    return out


def saved_duration(lay, s, tag, out=None):
    out = {} if out is None else out
    for n, t in zip(("xb", "c1", None, "h1", "c2", None, "h2"), s):
        if n is not None:
            out[tag + n] = unrows(lay, t)
    return out


# ----------------------------------------------------------------------------- pieces
def _conv(P, name, x, pad=0):
    return F.conv1d(x, P[name + ".weight"], P[name + ".bias"], padding=pad)


def _drop(drop, key, x):
    return x if drop is None else x * drop[key].to(x.dtype)


def _keep(drop, key):
    return None if drop is None else drop[key] != 0


def _grad_only(v, g):
    """v's value with g's gradient path: v.detach() + (g - g.detach())"""
    return v.detach() + (g - g.detach())


def attention(q, k, v, Ek, Ev, mask, n_heads, w, hk, tag, dropP=None):
    """glowtts_ref.mha_fwd between the q / k / v convs and conv_o (attentions.py:246-272), with the 9-diagonal band; P is forced
    BEFORE the dropout (the kernels save the un-dropped P)."""
    b, d, t = q.shape
    dk = d // n_heads
    am = mask.unsqueeze(2) * mask.unsqueeze(-1)
    qh, kh, vh = (a.view(b, n_heads, dk, t).transpose(2, 3) for a in (q, k, v))
    idx = torch.arange(t)
    rel = idx[None, :] - idx[:, None] + w
    band = (rel >= 0) & (rel <= 2 * w)
    relc = rel.clamp(0, 2 * w)[None, None].expand(b, n_heads, t, t)
    raw = torch.matmul(qh, kh.transpose(-2, -1)) + torch.gather(torch.matmul(qh, Ek.t()), 3, relc) * band
    raw = hk.store(tag + "dS", raw, "bf16")                  # dS with its factor 1 / sqrt(dk): what dq, dk and dEk are summed from
    scores = (raw / math.sqrt(dk)).masked_fill(am == 0, -1e4)
    p = F.softmax(scores, dim=-1)
    if hk.mode == "exact" or hk.has(tag + "P"):
        p = hk.force(tag + "P", p, am)
    if dropP is not None:
        p = p * dropP.to(p.dtype)
    p = hk.operand(tag + "Pd", p, "bf16")                    # dropout(P) as dv and dEv are summed from it; d P itself flows unrounded
    out = torch.matmul(p, vh)
    pw = torch.zeros(b, n_heads, t, 2 * w + 1, dtype=p.dtype).scatter_add(3, relc, p * band)
    out = out + torch.matmul(pw, Ev)
    return out.transpose(2, 3).contiguous().view(b, d, t)


def layer(P, pre, i, xa, xb, mask, hk, drop=None, n_heads=2, window=4, ks=3):
    """one encoder layer from the fp32 stream xa and its bf16 copy xb (one tensor twice, or two leaves) -> the masked output"""
    tag = f"{pre}{i}."
    A, Fn = f"{pre}attn_layers.{i}.", f"{pre}ffn_layers.{i}."
    xa = hk.store(tag + "dx0", hk.force(tag + "x", xa, mask), "f32")
    xb = hk.store(tag + "dxb0", hk.force(tag + "xb", xb, mask), "bf16")
    q, k, v = (hk.store(tag + "d" + n, hk.force(tag + n, _conv(P, A + "conv_" + n, xb), mask), "bf16") for n in "qkv")
    o = attention(q, k, v, P[A + "emb_rel_k"][0], P[A + "emb_rel_v"][0], mask, n_heads, window, hk, tag,
                  None if drop is None else drop[A + "drop:0"])
    o = hk.store(tag + "do", hk.force(tag + "o", o, mask), "bf16")
    y = hk.force(tag + "ln1.y", hk.store(tag + "dy", _conv(P, A + "conv_o", o), "bf16"), mask)
    x1 = layer_norm_c(xa + _drop(drop, f"{pre}drop:{2 * i}", y), P[f"{pre}norm_layers_1.{i}.gamma"], P[f"{pre}norm_layers_1.{i}.beta"]) * mask
    x1a = hk.store(tag + "dx1", hk.force(tag + "ln2.a", x1, mask), "f32")
    if hk.defect("dx1_lost"):
        x1a = x1a.detach()
    xb1 = hk.store(tag + "dxb1", hk.force(tag + "xb1", x1, mask), "bf16")
    c1 = hk.store(tag + "dc1", _conv(P, Fn + "conv_1", xb1 * mask, ks // 2), "bf16")
    f1 = _drop(drop, Fn + "drop:0", hk.relu(tag + "f1", c1, _keep(drop, Fn + "drop:0"))) * mask
    f1 = hk.force(tag + "f1", f1, mask)
    f2 = hk.force(tag + "ln2.y", hk.store(tag + "df2", _conv(P, Fn + "conv_2", f1, ks // 2) * mask, "bf16"), mask)
    return layer_norm_c(x1a + _drop(drop, f"{pre}drop:{2 * i + 1}", f2), P[f"{pre}norm_layers_2.{i}.gamma"],
                        P[f"{pre}norm_layers_2.{i}.beta"]) * mask


def _layers(P, pre, x, mask, hk, vec, n_layers, drop, first_xb=None, **kw):
    """the layer loop of both runners; x: the masked stream; first_xb: layer 0's bf16 input where it is not x itself"""
    for i in range(n_layers):
        if vec is not None and i == COND_LAYER:
            x = (x + (vec.detach() if hk.defect("dvec_late") else vec)[:, :, None]) * mask
        if vec is not None and i == COND_LAYER - 1 and hk.defect("dvec_late"):
            x = x + (vec - vec.detach())[:, :, None] * mask
        x = layer(P, pre, i, x, first_xb if (i == 0 and first_xb is not None) else x, mask, hk, drop, **kw)
    return x


def encoder(P, pre, x, mask, hk, vec=None, n_layers=3, drop=None, **kw):
    """the stand-alone attentions.Encoder (attentions._EncoderRunner): vec [B, C] = cond_g(g) or None"""
    return _layers(P, pre, x * mask, mask, hk, vec, n_layers, drop, **kw)


def prenet(P, pre, xa, xb, mask, hk, drop=None, n_layers=3, ks=5):
    """modules.ConvReluNorm from the fp32 input xa (the residual) and its bf16 copy xb (the convs' input) -> (x0 + proj(h)) * mask"""
    h = hk.store(pre + "dh.0", hk.force(pre + "h.0", xb, mask), "bf16")
    for i in range(n_layers):
        c = hk.force(pre + f"c.{i}", hk.store(pre + f"dc.{i}", _conv(P, pre + f"conv_layers.{i}", h * mask, ks // 2), "bf16"), mask)
        n = layer_norm_c(c, P[pre + f"norm_layers.{i}.gamma"], P[pre + f"norm_layers.{i}.beta"])
        site = pre + f"relu_drop.1:{i}"
        h = _drop(drop, site, hk.relu(pre + f"h.{i + 1}", n, _keep(drop, site))) * mask
        h = hk.store(pre + f"dh.{i + 1}", hk.force(pre + f"h.{i + 1}", h, mask), "bf16")
    return hk.store(pre + "dpre", (xa + _conv(P, pre + "proj", h)) * mask, "bf16")


def duration(P, pre, x, mask, hk, drop=None, vec=None, ks=3):
    """models.DurationPredictor on the (detached) encoder output x; vec [B, C] = cond(g) (+ cond_lang(l)) or None -> logw [B, 1, T]"""
    if vec is not None:
        x = (x + vec[:, :, None]) * mask
    x = hk.store(pre + "dx", hk.force(pre + "xb", x, mask), "bf16")
    h = x
    for j, (cv, nm) in enumerate((("conv_1", "norm_1"), ("conv_2", "norm_2")), 1):
        r = hk.store(pre + f"dr{j}", _conv(P, pre + cv, h * mask, ks // 2), "bf16")
        c = hk.relu(pre + f"c{j}", r)
        if j == 2 and hk.defect("relu_in_norm_2"):
            c = _grad_only(c, r)
        c = hk.force(pre + f"c{j}", c, mask)
        h = _drop(drop, pre + f"drop:{j - 1}", layer_norm_c(c, P[pre + nm + ".gamma"], P[pre + nm + ".beta"])) * mask
        hk.dropped_zero(pre + f"h{j}", _keep(drop, pre + f"drop:{j - 1}"))
        h = hk.store(pre + f"dh{j}", hk.force(pre + f"h{j}", h, mask), "bf16")
    return hk.store(pre + "db", _conv(P, pre + "proj", h) * mask, "bf16")


def text_encoder(P, pre, ids, lengths, hk, vec=None, lvec=None, hidden=192, n_layers=3, prenet_on=True, mean_only=True, drop=None, **kw):
    """models.TextEncoder.forward as text_models._TextEncoderRunner runs it: vec [B, C] = encoder.cond_g(g), lvec [B, lin] or None
    -> (x, x_m, x_logs or None, mask)"""
    B, T = ids.shape
    mask = (torch.arange(T)[None, :] < lengths[:, None]).to(F64)[:, None, :]
    x = F.embedding(ids, P[pre + "emb.weight"]) * math.sqrt(hidden)
    if lvec is not None:
        lin = lvec.shape[1]
        lv = lvec[:, None, :].expand(B, T, lin)
        if hk.defect("lvec_shift"):
            z = torch.zeros(B, T, hidden, dtype=F64)
            shifted = torch.cat((z[:, :, :hidden - lin - 1], lv - lv.detach(), z[:, :, :1]), -1)
            x = torch.cat((x, lv.detach()), -1) + shifted
        else:
            x = torch.cat((x, lv), -1)
    x = x.transpose(1, 2) * mask
    first_xb = None
    if prenet_on:
        x = prenet(P, pre + "pre.", x, x, mask, hk, drop)
        if hk.defect("prenet_dxb"):
            first_xb = x.detach()
    x = _layers(P, pre + "encoder.", x, mask, hk, vec, n_layers, drop, first_xb=first_xb, **kw)
    xo = hk.store(pre + "dx", x, "f32")
    xb = hk.store(pre + "dxb", hk.force(pre + "xb_final", x, mask), "bf16")
    x_m = hk.store(pre + "d", _conv(P, pre + "proj_m", hk.store(pre + "proj_m.dxb", xb, "bf16")) * mask, "bf16")
    x_logs = None
    if not mean_only:
        xs = xb.detach() if hk.defect("proj_s_addend") else xb
        x_logs = _conv(P, pre + "proj_s", xs) * mask
        if hk.defect("proj_s_scale"):
            x_logs = _grad_only(x_logs, x_logs * (1.0 + float(hk.defect("proj_s_scale"))))
        x_logs = hk.store(pre + "d2", x_logs, "bf16")
    return xo, x_m, x_logs, mask


# ----------------------------------------------------------------------------- parameters
def params64(state, prefix="", bf16_gemm=True):
    """{prefix + name: float64 tensor} from a module's state dict (or named parameters).  bf16_gemm: conv weights [Cout, Cin, taps] are
    the bf16 values the packed images hold (rows64.packed_weights); LayerNorm parameters, biases, emb_rel_* and the embedding stay fp32
    values."""
    P = {}
    for n, t in state.items():
        t = t.detach().cpu().float()
        if bf16_gemm and t.dim() == 3 and n.endswith(".weight"):
            P[prefix + n] = rows64.packed_weights(t).permute(1, 2, 0).contiguous()
        else:
            P[prefix + n] = t.double()
    return P


def leaves(P):
    return {k: v.detach().clone().requires_grad_(True) for k, v in P.items()}
