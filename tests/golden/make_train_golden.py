"""Generate tests/golden/train_golden/ by IMPORTING the reference's Python modules in TRAIN mode
(same import shims as make_float_golden.py):

    make -C oracle && python tests/golden/make_train_golden.py

Every nn.Dropout of a reference module is replaced, per instance, by "multiply by the next recorded mask / (1-p)": the
masks are seeded Bernoulli draws, recorded under the site names oracle/glowtts_ref.py's `drop=` uses (the nn.Dropout's
module path, ':', its call ordinal within one forward) and stored bit-packed ("mask/<site>", shape "mshape/<site>",
"mp/<site>" = p).  Inputs, outputs and input / parameter gradients are stored next to them; tests/test_train_golden.py
checks that the oracle, handed these masks, reproduces every array.  Nothing of the reference is copied.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from fill import fill_module  # noqa: E402
from make_float_golden import grads_of, import_reference, lens_mask  # noqa: E402
import shards  # noqa: E402


class MaskRecorder:
    """Replace the forward of every nn.Dropout under `module` (named `prefix + path`) by a recorded Bernoulli mask."""

    def __init__(self, gen):
        self.gen, self.masks, self.count = gen, {}, {}

    def attach(self, module, prefix):
        for name, m in module.named_modules():
            if isinstance(m, torch.nn.Dropout):
                m.forward = self._forward(prefix + name, m.p)
        return module

    def _forward(self, site, p):
        def fwd(x):
            k = self.count.get(site, 0)
            self.count[site] = k + 1
            keep = torch.rand(x.shape, generator=self.gen) >= p
            self.masks[f"{site}:{k}"] = (keep, p)
            return x * (keep.to(x.dtype) * (1.0 / (1.0 - p)))
        return fwd


def main():
    torch.manual_seed(0)
    torch.set_grad_enabled(True)
    commons, modules, attentions, models = import_reference()
    out = {}
    g = torch.Generator().manual_seed(4321)
    rec = MaskRecorder(torch.Generator().manual_seed(777))

    def rnd(*shape, scale=1.0):
        return torch.randn(*shape, generator=g) * scale

    def params(mod, prefix, names=None):
        prm = dict(mod.named_parameters())
        names = names or list(prm)
        return [prefix + n for n in names], [prm[n] for n in names]

    def store_grads(tag, keys, grads):
        for k, v in zip(keys, grads):
            out[f"{tag}_gp_{k}"] = v if v is not None else torch.zeros(1)

    # ---- WN (no conditioning) and WN with g, p = 0.05: input and every parameter gradient
    m = lens_mask([12, 7], 12)
    xh = (rnd(2, 192, 12) * m).requires_grad_(True)
    wn = rec.attach(fill_module(modules.WN(160, 192, 5, 1, 4, 0, 0.05), "wn.").train(), "wn.")
    o = wn(xh, m)
    keys, ps = params(wn, "wn.", ["in_layers.0.weight_g", "in_layers.2.bias", "res_skip_layers.1.weight_g", "res_skip_layers.3.bias",
                                  "res_skip_layers.3.weight_v"])
    gx, *gp = grads_of([(o, 1)], [xh] + ps)
    out.update(wn_x=xh, wn_mask=m, wn_out=o, wn_gx=gx); store_grads("wn", keys, gp)
    wng = rec.attach(fill_module(modules.WN(160, 192, 5, 1, 4, 8, 0.05), "wng.").train(), "wng.")
    gc = rnd(2, 8, 1).requires_grad_(True)
    o = wng(xh, m, gc)
    gx, gg = grads_of([(o, 2)], [xh, gc])
    out.update(wng_g=gc, wng_out=o, wng_gx=gx, wng_gg=gg)

    # ---- CouplingBlock fwd + input grad
    xc = (rnd(2, 160, 12) * m).requires_grad_(True)
    cb = rec.attach(fill_module(attentions.CouplingBlock(160, 192, 5, 1, 4, gin_channels=0, p_dropout=0.05, n_sqz=2), "cb.").train(),
                    "cb.")
    z, ld = cb(xc, m)
    (gx,) = grads_of([(z, 3), (ld, 4)], [xc])
    out.update(cb_x=xc, cb_z=z, cb_logdet=ld, cb_gx=gx)

    # ---- FlowSpecDecoder (2 blocks): fwd, input grad, parameter grads.  ActNorm: initialized (ddi=False), no DDI in train mode
    ym = lens_mask([24, 14], 24)
    yy = (rnd(2, 80, 24) * ym).requires_grad_(True)
    dec = fill_module(models.FlowSpecDecoder(80, 192, 5, 1, 2, 4, p_dropout=0.05, n_split=4, n_sqz=2), "decoder.").train()
    assert all(getattr(f, "initialized", True) for f in dec.flows)
    rec.attach(dec, "decoder.")
    z, ld = dec(yy, ym)
    keys, ps = params(dec, "decoder.", ["flows.2.wn.in_layers.0.weight_g", "flows.2.wn.in_layers.3.bias", "flows.5.wn.res_skip_layers.1.weight_g",
                                        "flows.5.start.weight_v", "flows.2.end.bias", "flows.3.logs"])
    gy, *gp = grads_of([(z, 5), (ld, 6)], [yy] + ps)
    out.update(dec_y=yy, dec_mask=ym, dec_z=z, dec_logdet=ld, dec_gy=gy); store_grads("dec", keys, gp)

    # ---- relative-position MHA at T in {5, 37}, p = 0.1
    for T in (5, 37):
        xm = lens_mask([T, max(1, T - 2)], T)
        xa = (rnd(2, 192, T) * xm).requires_grad_(True)
        mha = rec.attach(fill_module(attentions.MultiHeadAttention(192, 192, 2, window_size=4, p_dropout=0.1), f"mha{T}.").train(),
                         f"mha{T}.")
        am = xm.unsqueeze(2) * xm.unsqueeze(-1)
        o = mha(xa, xa, am)
        keys, ps = params(mha, f"mha{T}.", ["conv_q.weight", "conv_v.weight", "emb_rel_k", "emb_rel_v"])
        ga, *gp = grads_of([(o, 7)], [xa] + ps)
        out.update({f"mha{T}_x": xa, f"mha{T}_mask": xm, f"mha{T}_out": o, f"mha{T}_p": mha.attn, f"mha{T}_gx": ga})
        store_grads(f"mha{T}", keys, gp)

    # ---- FFN, ConvReluNorm (p = 0.5), Encoder (2 layers), DurationPredictor, TextEncoder (prenet + 2 layers)
    T = 11; xm = lens_mask([11, 6], T)
    xe = (rnd(2, 192, T) * xm).requires_grad_(True)
    ffn = rec.attach(fill_module(attentions.FFN(192, 192, 768, 3, p_dropout=0.1), "ffn.").train(), "ffn.")
    o = ffn(xe, xm)
    (gx,) = grads_of([(o, 8)], [xe])
    out.update(enc_x=xe, enc_mask=xm, ffn_out=o, ffn_gx=gx)
    crn = rec.attach(fill_module(modules.ConvReluNorm(192, 192, 192, 5, 3, 0.5), "pre.").train(), "pre.")
    o = crn(xe, xm)
    (gx,) = grads_of([(o, 9)], [xe])
    out.update(crn_out=o, crn_gx=gx)
    enc = rec.attach(fill_module(attentions.Encoder(192, 768, 2, 2, 3, 0.1, window_size=4), "enc.").train(), "enc.")
    o = enc(xe, xm)
    keys, ps = params(enc, "enc.", ["attn_layers.0.conv_k.weight", "attn_layers.1.emb_rel_v", "ffn_layers.0.conv_1.bias",
                                    "ffn_layers.1.conv_2.bias", "norm_layers_1.1.gamma", "norm_layers_2.0.beta"])
    gx, *gp = grads_of([(o, 10)], [xe] + ps)
    out.update(encoder_out=o, encoder_gx=gx); store_grads("encoder", keys, gp)
    dp = rec.attach(fill_module(models.DurationPredictor(192, 256, 3, 0.1), "dp.").train(), "dp.")
    o = dp(xe, xm)
    keys, ps = params(dp, "dp.", ["conv_1.bias", "norm_1.gamma", "conv_2.bias", "norm_2.beta", "proj.weight", "proj.bias"])
    gp = grads_of([(o, 11)], ps)
    out.update(dp_out=o); store_grads("dp", keys, gp)
    ids = torch.randint(1, 148, (2, T), generator=g); xl = torch.tensor([11, 6])
    te = fill_module(models.TextEncoder(148, 80, 192, 768, 256, 2, 2, 3, 0.1, window_size=4, mean_only=True,
                                        prenet=True, use_sdp=False), "encoder.").train()
    rec.attach(te, "encoder.")
    tx, tm, _, _ = te(ids, xl)
    keys, ps = params(te, "encoder.", ["emb.weight", "pre.conv_layers.1.bias", "encoder.attn_layers.1.conv_o.weight", "proj_m.weight"])
    gp = grads_of([(tx, 12), (tm, 13)], ps)
    out.update(te_ids=ids, te_len=xl, te_x=tx, te_m=tm); store_grads("te", keys, gp)

    # ---- DilatedDepthSeparableConv (p = 0.5, modules.py:733)
    Td = 23; dm = lens_mask([23, 11], Td)
    xd = (rnd(2, 192, Td) * dm).requires_grad_(True)
    gcond = rnd(2, 192, Td, scale=0.5)
    dds = rec.attach(fill_module(modules.DilatedDepthSeparableConv(192, 3, 3, 0.5), "dds.").train(), "dds.")
    o = dds(xd, dm, g=gcond)
    keys, ps = params(dds, "dds.", ["convs_sep.0.weight", "convs_1x1.2.weight", "norms_2.1.gamma"])
    gx, *gp = grads_of([(o, 14)], [xd] + ps)
    out.update(dds_mask=dm, dds_x=xd, dds_g=gcond, dds_out=o, dds_gx=gx); store_grads("dds", keys, gp)

    for site, (keep, p) in rec.masks.items():
        out["mask/" + site] = torch.from_numpy(np.packbits(keep.numpy().reshape(-1)))
        out["mshape/" + site] = torch.tensor(list(keep.shape))
        out["mp/" + site] = torch.tensor(p)
    path = os.path.join(HERE, "train_golden")
    n = shards.save(path, {k: v.detach().cpu().numpy() for k, v in out.items()})
    print("wrote", path, len(out), "arrays", len(rec.masks), "masks in", n, "shards")


if __name__ == "__main__":
    main()
