"""Synthesis as ONE captured graph (FlowGenerator.compile_synthesis).

FlowGenerator.infer with the device front end is ~116 dependent launches issued from Python; its GPU work is a fraction of the time
the host needs to issue them.  A Synthesizer captures the whole call — text encoder, duration predictor, durations -> lengths, the
row geometry of the mel axis (gt_synth_geometry, built on the device from the predicted lengths), the sampled prior
(gt_synth_prior_call) and the reverse decoder — once, at sizes that are capacities, with the call's scalars (seed, noise_scale,
length_scale) in a device-side gt_synth_call block.  One call is then one upload, one replay and one readback, nothing of it is baked
into the graph, and the host does not synchronise in between: several calls can be in flight.

A call whose predicted lengths do not fit the capacities (status != 0) is a handled outcome: the kernels stay inside their buffers,
and the handle re-runs the call through the eager path (or raises SynthesisOverflow).

compile_synthesis(stochastic=True) captures the FULL model the same way: the emotion front end, the stochastic
duration predictor in reverse, and the stochastic pitch / energy predictors on a second capacity context — the ragged frame-rate rows,
built on the device by gt_synth_frame_geometry — with noise keyed by (utterance, token / frame) (gt_randn_keyed_call), the call's eight
scalars in a gt_synth_call_ext block, and the contours written into the decoder's rows by gt_synth_contours_call.  One stream, no fork."""
import ctypes
import weakref
from typing import NamedTuple

import torch

from . import _lib, ops

HALO = ops.HALO
GUARD = 256                # canary bytes in front of and behind every static buffer
CANARY = 0xA5


class SynthesisOverflow(RuntimeError):
    """The predicted lengths of a call did not fit the synthesiser's capacities.  status: bit 0 = an utterance longer than max_frames,
    bit 1 = the rows of the batch do not fit max_rows, bit 2 = the frame-rate rows of the pitch / energy predictors do not fit
    max_frame_rows; lengths: the predicted frame counts (unclipped)."""

    def __init__(self, status, lengths):
        super().__init__(f"synthesis overflow (status {status}): predicted lengths {lengths} do not fit the compiled capacities")
        self.status, self.lengths = status, lengths


def default_frame_rows(batch, max_frames, row_round):
    """rows of `batch` utterances of max_frames frames on the un-squeezed axis, rounded up to row_round"""
    need = batch * (max_frames + 2 * HALO)
    return -(-need // row_round) * row_round


def default_rows(batch, max_frames, row_round):
    """rows of `batch` utterances of max_frames frames on the squeezed axis, rounded up to row_round"""
    need = batch * (max_frames // 2 + 2 * HALO)
    return -(-need // row_round) * row_round


# ---- the call: ONE pipeline for infer (device front end off / on) and the captured graph --------------------------------------------------
class CallScalars(NamedTuple):
    """the scalars of one synthesis call, in the field order of gt_synth_call_ext and under infer's keyword names"""
    seed: int
    noise_scale: float = 1.
    noise_scale_w: float = 1.
    length_scale: float = 1.
    f0_noise_scale: float = 1.
    energy_noise_scale: float = 1.
    pitch_scale: float = 1.
    energy_scale: float = 1.

    def words(self, ext):
        """the call block as int32 words: gt_synth_call, or (ext) gt_synth_call_ext, whose first 16 bytes are the gt_synth_call"""
        c = _lib.SynthCall(int(self.seed) & 0xFFFFFFFF, *[float(v) for v in self[1:4]])
        if ext:
            c = _lib.SynthCallExt(c, *[float(v) for v in self[4:]])
        return torch.frombuffer(bytearray(bytes(c)), dtype=torch.int32).clone()


def _launch(device, name, *args):
    """the C-ABI entry `name` on the current stream of device"""
    getattr(_lib.call, name)(*args, _lib.current_stream(device))


def _by_tokens(name, Tx):
    """the front-end entry `name` for texts of Tx tokens: itself to 512 tokens (a short call launches what it always launched), its
    *_long form (csrc/synth_front.hip; to GT_SYNTH_LONG_MAX_TX = 4096 tokens) past them"""
    if Tx <= _lib.SYNTH_MAX_TX:
        return name
    return {"gt_synth_lengths": "gt_synth_lengths_long", "gt_synth_prior": "gt_synth_prior_long",
            "gt_synth_prior_call": "gt_synth_prior_long_call"}[name]


class ByValue:
    """The scalar source of the eager path: a CallScalars, handed to the kernels by value.  keyed: the predictors' draws are keyed by
    (utterance, token / frame), independent of the layout (gt_randn_keyed: what FromBlock reproduces), else by the row (gt_randn_rows).
    noise -> [rc.R, 2] draws of the generator's stream stream_id times scale `which` (1 noise_scale_w, 2 f0_, 3 energy_noise_scale);
    prior / contours launch gt_synth_prior (past 512 tokens gt_synth_prior_long) / gt_synth_contours on the arguments every source
    shares."""

    def __init__(self, scalars, keyed, device):
        self.scalars, self.keyed, self.device, self.length_scale = scalars, keyed, device, scalars.length_scale

    def noise(self, rc, stream_id, which):
        s = self.scalars
        nz = torch.empty(rc.R, 2, dtype=torch.float32, device=self.device)
        scale = float((s.noise_scale, s.noise_scale_w, s.f0_noise_scale, s.energy_noise_scale)[which])
        if self.keyed:
            _launch(self.device, "gt_randn_keyed", nz, rc.row0, rc.Tp, rc.lengths, rc.B, rc.R, 2, s.seed, stream_id, scale)
        else:
            _launch(self.device, "gt_randn_rows", nz, rc.R, 2, s.seed, stream_id, scale)
        return nz

    def prior(self, args):
        args.seed, args.noise_scale = self.scalars.seed, float(self.scalars.noise_scale)
        _launch(self.device, _by_tokens("gt_synth_prior", args.Tx), args)

    def contours(self, *args):
        _launch(self.device, "gt_synth_contours", *args, float(self.scalars.pitch_scale), float(self.scalars.energy_scale))


class FromBlock:
    """The scalar source of a captured graph: the gt_synth_call[_ext] block in device memory, read by the *_call entries at every
    replay; length_scale is a 0-dim view of it, read by the graph's torch plumbing."""
    keyed = True

    def __init__(self, call):
        self.call, self.device, self.length_scale = call, call.device, call.view(torch.float32)[3]

    def noise(self, rc, stream_id, which):
        nz = torch.empty(rc.R, 2, dtype=torch.float32, device=self.device)
        _launch(self.device, "gt_randn_keyed_call", nz, rc.row0, rc.Tp, rc.lengths, rc.B, rc.R, 2, self.call, stream_id, which)
        return nz

    def prior(self, args):
        _launch(self.device, _by_tokens("gt_synth_prior_call", args.Tx), args, self.call)

    def contours(self, *args):
        _launch(self.device, "gt_synth_contours_call", *args, self.call)


def text_stage(gen, ids, x_len, g, l, emo, emo_cartesian, draw):
    """conditioning -> text encoder -> duration predictor (the stochastic one in reverse on the noise draw(rc) [rc.R, 2], or the
    deterministic one) -> g, l, x_m, x_logs, x_mask, the text rows (rc, xb), logw [B, 1, Tx].  The one place synthesis calls the
    encoder from: no backward follows, so past 505 tokens its attention stores no P (keep_p=False)"""
    from .text_models import _DurationRunner
    g = gen.condition(g, emo, emo_cartesian)
    if l is not None:
        l = gen.emb_l(l).unsqueeze(-1)
    xo, x_m, x_logs, x_mask = gen.encoder(ids, x_len, l=l, g=g, prepared=True, keep_p=False)
    rc, xb = gen.encoder._last_rows
    pw = gen.encoder.proj_w
    dvec = pw.cond_vec(g, l)
    if gen.use_sdp:
        logw = rc.from_rows(pw._reverse_rows(rc, xb, dvec, draw(rc))[:, None].contiguous())
    else:
        runner = _DurationRunner(pw, rc, xb, False, 0, has_cond=dvec is not None)
        (logw,), _ = runner.forward(*([dvec] if dvec is not None else []))
    return g, l, x_m, x_logs, x_mask, rc, xb, logw


def lengths_stage(logw, x_mask, length_scale, x_len, cum, y_len, logw_):
    """durations -> gt_synth_lengths (past 512 tokens gt_synth_lengths_long) into the caller's cum [B, Tx], y_len [B] and (or None) logw_ [B, 1, Tx] -> dur, x_len as int32.
    exp, length_scale (a float, or a 0-dim device tensor) and ceil stay in torch on [B, Tx] (plumbing): the durations are bit for bit
    those of infer without the front end"""
    dur = torch.ceil(torch.exp(logw) * x_mask * length_scale).squeeze(1).contiguous()
    xl = x_len.to(torch.int32).contiguous()
    _launch(dur.device, _by_tokens("gt_synth_lengths", dur.shape[1]), dur, xl, cum, y_len, logw_, *dur.shape)
    return dur, xl


def prior_stage(gen, x_m, x_logs, cum, xl, y_len, rcy, bufs, source, Ty):
    """the sampled, squeezed latent into bufs["rows"] on the rows of rcy; z_m, z_logs [B, C, Ty], frame2token [B, Ty] and attn
    [B, 1, Tx, Ty] where bufs has them (None: not written) -> the fp32 x_m / x_logs the launch read"""
    B, C, Tx = x_m.shape
    xm = x_m.float().contiguous()
    xs = None if gen.mean_only else x_logs.float().contiguous()
    source.prior(_lib.fill_args(_lib.SynthPriorArgs, x_m=xm, x_logs=xs, cum=cum, x_len=xl, y_len=y_len, row0=rcy.row0, Tp=rcy.Tp, R=rcy.R,
                                **{k: bufs[k] for k in ("rows", "z_m", "z_logs", "frame2token", "attn")}, B=B, C=C, Tx=Tx, Ty=Ty,
                                seed=0, noise_scale=0.0))
    return xm, xs


def prosody_stage(gen, g, rc, xb, rcy, rcf, bufs, source, Ty):
    """models.py:1203-1228 at the frame rate, on the rows of rcf, on the caller's one stream: token rows gathered by
    bufs["frame2token"] (frames no token owns, -1, are masked rows: not read) -> the stochastic pitch / energy predictors in reverse
    -> pitch, energy [B, Ty] (None for a predictor the model does not have) and the keywords decoder.reverse_rows takes them by"""
    xf = gen._gather_features(rc, xb, rcf, bufs["frame2token"])
    if not source.keyed:                                             # eager only: row-keyed draws, the contours through from_rows
        pitch = energy = None
        if gen.use_spp:
            nz = source.noise(rcf, 2, 2)
            pitch = rcf.from_rows(gen.proj_pitch._reverse_rows(rcf, xf, gen.proj_pitch.cond_vec(g), nz)[:, None].contiguous()).squeeze(1) * source.scalars.pitch_scale
        if gen.use_sep:
            nz = source.noise(rcf, 3, 3)
            energy = rcf.from_rows(gen.proj_energy._reverse_rows(rcf, xf, gen.proj_energy.cond_vec(g), nz)[:, None].contiguous()).squeeze(1) * source.scalars.energy_scale
        return pitch, energy, dict(pitch=pitch, energy=energy)
    prow = erow = None
    if gen.use_spp:
        prow = gen.proj_pitch._reverse_rows(rcf, xf, gen.proj_pitch.cond_vec(g), source.noise(rcf, 2, 2))
    if gen.use_sep:
        erow = gen.proj_energy._reverse_rows(rcf, xf, gen.proj_energy.cond_vec(g), source.noise(rcf, 3, 3))
    # for the return tuple and, squeezed, on the decoder's rows: one launch
    source.contours(prow, erow, rcf.row0, rcf.Tp, rcf.lengths, rcf.R, rcy.row0, rcy.Tp, rcy.lengths, rcy.R, bufs["psig"], bufs["esig"],
                    bufs["pitch"], bufs["energy"], rcy.B, Ty)
    return bufs["pitch"], bufs["energy"], dict(pitch_rows=bufs["psig"], energy_rows=bufs["esig"])


class SynthesisHandle:
    """One call in flight.  lengths() / mel() / aux() wait for the call's event (not for the device).

    Stream order: what mel() / aux() return is safe to use on the stream that is current when they are called.  Views of the static
    buffers are valid until the next call is issued: that call's replay waits for the work queued so far on the streams the views
    were handed out on (and on the stream it is issued from) before it overwrites them.  mel(clone=True) is copied on the
    synthesiser's own stream, so the next replay waits for nothing of the caller's."""

    def __init__(self, synth, slot, inputs, call):
        self._synth, self._slot, self._inputs, self._call = synth, slot, inputs, call
        self._saved = None          # (mel, aux, event, prosody, wav) copies, taken in stream order when a later call was issued before this one was read
        self._read = None           # (lengths, status) once the event has passed
        self._eager = self._eager_wav = None
        # mel() has been handed out: the next call may overwrite the static buffers.  aux() alone does not set it — a caller who
        # looked at the durations first and asks for the mel after the next call still gets this call's (at the price of one copy aside)
        self._done = False

    def _wait(self):
        if self._read is None:
            self._synth._retire(self._slot)              # waits for the call's event, reads y_len | status, sets _read
            assert self._read is not None, "a slot is marked read only together with its live handle"
        return self._read

    @property
    def status(self):
        return self._wait()[1]

    def lengths(self):
        """predicted frame counts [B] (host list); what the eager path returns as y_lengths"""
        return list(self._wait()[0])

    def _fallback(self, fallback):
        lens, status = self._wait()
        if not fallback:
            raise SynthesisOverflow(status, list(lens))
        s = self._synth
        dev = s.device
        if self._eager is None:
            x, xl, g, l, emo, emoc = self._inputs
            c = self._call
            # a full-model synthesiser passes every scalar of the call on; the plain one calls infer as it always did
            more = c._asdict() if s.stochastic else dict(seed=c.seed, noise_scale=c.noise_scale, length_scale=c.length_scale)
            if emo is not None:
                more.update(emo=emo.to(dev), emo_cartesian=emoc.to(dev))
            # on the synthesiser's stream, behind the calls in flight (the eager path shares the model's scratch buffers with the graph)
            # and behind what the caller's stream has queued (it may have produced device-resident inputs).  EVERYTHING the eager call
            # reads is built on that stream: the encoder gathers by token id without a bounds check, so it must never see the padded
            # text before its fill
            s.stream.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(s.stream):
                for t in (x, xl, g, l, emo, emoc):
                    if t is not None and t.is_cuda:
                        t.record_stream(s.stream)                                       # the caller's tensors, read on this stream
                xp = torch.zeros(s.batch, s.max_tokens, dtype=torch.int64, device=dev)   # the text as the graph saw it: padded to max_tokens
                xp[:, :x.shape[1]] = x.to(dev)
                self._eager = s.gen.infer(xp, xl.to(dev), g=None if g is None else g.to(dev), l=None if l is None else l.to(dev), **more)
        cur = torch.cuda.current_stream(dev)
        cur.wait_stream(s.stream)
        for grp in self._eager:                                                        # allocated on s.stream, used on the caller's
            for t in grp:
                if t is not None:
                    t.record_stream(cur)
        return self._eager

    def _from_saved(self):
        """the outputs that were moved aside: the caller's stream waits for that copy and is registered as a user of its memory"""
        mel, aux, ev, pros, wav = self._saved
        cur = torch.cuda.current_stream(self._synth.device)
        cur.wait_event(ev)
        for t in [mel] + list((aux or {}).values()) + [t for t in (pros or ()) if t is not None] + ([] if wav is None else [wav]):
            t.record_stream(cur)
        return mel, aux, pros, wav

    def mel(self, clone=False, fallback=True):
        """[B, C, max(lengths)] fp32 — max(lengths) rounded down to even, as infer returns it: the squeeze drops an odd trailing frame —
        zero past every utterance's length: a view of the synthesiser's static buffer, valid until the next call (clone=True: a copy
        that outlives it).  After an overflow: the eager path's mel of the same call, re-run when this is called (fallback=False:
        SynthesisOverflow is raised here, not when the call was issued)."""
        lens, status = self._wait()
        if status != 0:
            return self._fallback(fallback)[0][0]
        self._done = True
        s = self._synth
        T = max(lens) // 2 * 2
        if self._saved is not None:                      # a later call was issued first: this call's outputs were moved aside
            return self._from_saved()[0][:, :, :T]
        cur = torch.cuda.current_stream(s.device)
        if not clone:
            s._handed.add(cur)                           # the next replay waits for what this stream has queued by then
            return s.mel_static[:, :, :T]
        with torch.cuda.stream(s.stream):                # idle behind this call (its event has passed): ordered before the next replay
            out = s.mel_static[:, :, :T].clone()
        cur.wait_stream(s.stream)
        out.record_stream(cur)
        return out

    def wav(self, clone=False, fallback=True):
        """With a neural vocoder (audio.HiFiGAN, BigVGAN, Vocos, WaveGlow: DESIGN.md 4.26): (wav [B, vocoder.wav_len(T)] fp32, wav_lengths =
        [vocoder.wav_len(2 (lengths[b] // 2))]), bit-identical to vocoder(mel, 2 (lengths // 2)) — for a seeded vocoder (WaveGlow) with
        seed=the call's seed — (after an overflow: that eager call on the eager mel), under the rules below; wav_len(F) is U F for HiFi-GAN and BigVGAN and Griffin-Lim's 256 (F - 1) for Vocos.
        With an audio.GriffinLim: (wav [B, 256 (T - 1)] fp32, wav_lengths) with T = max(lengths) rounded down to even (the mel's
        frames) and wav_lengths[b] = 256 max(2 (lengths[b] // 2) - 1, 0) (a host list) — the call's samples, zero behind every
        utterance's, bit-identical to GriffinLim.from_mel(mel, 2 (lengths // 2), n_iters=vocoder_iters, seed=the call's seed,
        phases="counter").  A view of the synthesiser's static buffer under mel()'s stream-order rules (clone=True: a copy that outlives
        the next call); it is moved aside together with the mel when a later call is issued first.  After an overflow: that eager
        result on the eager path's mel (fallback=False: SynthesisOverflow).  An utterance of fewer than 4 frames is not refused (the
        host has not seen the lengths when the loop runs): it gets what the Griffin-Lim kernels define — a reflected index clamped
        into the utterance, and no sample below 2 frames.
        Like mel(), wav() marks the call as read: the next call then overwrites the static buffers without moving them aside, so take
        everything a handle is asked for (mel, wav, prosody, aux) before the next call is issued — or issue the next call first, which
        moves all of them aside.  A wav() asked of a handle whose outputs a later call has already overwritten raises RuntimeError
        instead of returning that call's samples."""
        s = self._synth
        if s.vocoder is None:
            raise RuntimeError("compile_synthesis(vocoder=audio.GriffinLim(...)) keeps the samples")
        lens, status = self._wait()
        if s.neural:                                                     # the vocoder's own rule
            wav_len = s.vocoder.wav_len
        else:                                                            # audio.GriffinLim: 256 (frames - 1) samples
            wav_len = lambda f: s.vocoder.stft_fn.hop_length * max(f - 1, 0)  # noqa: E731
        wav_lengths = [wav_len(2 * (v // 2)) for v in lens]
        n = wav_len(max(lens) // 2 * 2)
        if status != 0:
            mel = self._fallback(fallback)[0][0]
            if self._eager_wav is None:
                if s.neural:
                    frames = torch.tensor([2 * (v // 2) for v in lens], dtype=torch.int32).to(s.device)
                    kw = dict(seed=self._call.seed) if s.vocoder.seeded else {}
                    self._eager_wav = s.vocoder(mel, frames, mel_lengths_host=[2 * (v // 2) for v in lens], **kw)[0]
                elif mel.shape[2] < 2:
                    self._eager_wav = mel.new_zeros(mel.shape[0], 0)
                else:
                    frames = torch.tensor([2 * (v // 2) for v in lens], dtype=torch.int32).to(s.device)
                    self._eager_wav = s.vocoder.from_mel(mel, frames, n_iters=s.vocoder_iters, seed=self._call.seed, phases="counter")[0]
            return self._eager_wav, wav_lengths
        if self._saved is not None:
            return self._from_saved()[3][:, :n], wav_lengths
        if self._done and s._latest is not None and s._latest() is not self:
            raise RuntimeError("this call's outputs were handed out and a later call has overwritten the static buffers: take wav() "
                               "before the next call is issued, or issue it before anything of this handle is read")
        self._done = True
        cur = torch.cuda.current_stream(s.device)
        if not clone:
            s._handed.add(cur)
            return s.wav_static[:, :n], wav_lengths
        with torch.cuda.stream(s.stream):
            out = s.wav_static[:, :n].clone()
        cur.wait_stream(s.stream)
        out.record_stream(cur)
        return out, wav_lengths

    def prosody(self, fallback=True):
        """(pitch, energy): [B, max(lengths)] fp32 each, zero past every utterance's length, scaled by pitch_scale / energy_scale — what
        infer returns as its last group (None for a predictor the model does not have).  Views of static buffers under the same
        stream-order rules as mel(); they are copied aside together with it."""
        s = self._synth
        lens, status = self._wait()
        if status != 0:
            return tuple(self._fallback(fallback)[3])
        if self._saved is not None:
            src = self._from_saved()[2]
        else:
            src = (s.pitch_static, s.energy_static)
            s._handed.add(torch.cuda.current_stream(s.device))
        Ty = max(lens)
        return tuple(None if t is None else t[:, :Ty] for t in src)

    def aux(self, fallback=True):
        """aux=True: dict(z_m, z_logs [B, C, Ty], attn [B, 1, Tx, Ty], logw, logw_ [B, 1, Tx]) as infer returns them (views, valid until
        the next call)"""
        s = self._synth
        if not s.aux:
            raise RuntimeError("compile_synthesis(aux=True) keeps z_m / z_logs / attn / logw / logw_")
        lens, status = self._wait()
        if status != 0:
            (y, z_m, z_logs, _, _), _, (attn, logw, logw_), _ = self._fallback(fallback)
            return dict(z_m=z_m, z_logs=z_logs, attn=attn, logw=logw, logw_=logw_)
        if self._saved is not None:
            src = self._from_saved()[1]
        else:
            src = s.aux_static
            s._handed.add(torch.cuda.current_stream(s.device))
        Ty = max(lens)
        return dict(z_m=src["z_m"][:, :, :Ty], z_logs=src["z_logs"][:, :, :Ty], attn=src["attn"][:, :, :, :Ty], logw=src["logw"],
                    logw_=src["logw_"])


class Synthesizer:
    """gen.compile_synthesis(...): see FlowGenerator.compile_synthesis.  Attributes: batch, max_tokens, max_frames, max_rows, aux,
    overflows (calls whose lengths did not fit; a call is counted when its status is read — by its handle, or when its ring slot is
    taken again), mel_static / aux_static (the graph's outputs), stream (its own), captured_entries (C-ABI launches inside the graph).
    Any number of calls may be in flight: the RING-th call after an unread one first reads that one's lengths and status into its
    handle (which waits for it), so a handle read late still returns its own call's.
    stochastic=True adds: max_frame_rows, rcf (the capacity context of the frame-rate rows; None for a model without
    pitch / energy predictors), pitch_static / energy_static [batch, max_frames], and status bit 2.
    vocoder=audio.GriffinLim adds the waveform back end behind the decoder, inside the same graph: n_frames (int32
    [batch] = 2 * the squeezed lengths), wav_static [batch, 256 (max_frames - 1)] and voc_bufs (mag [batch, 513, max_frames], the
    spectrum workspace, wav_static) — 4 batch (513 max_frames + 1025 Fp + 256 (max_frames - 1)) bytes with Fp = max_frames rounded up
    to 64: 52 + 109 + 26 MB at batch 32 and 800 frames.  vocoder_iters is fixed at capture; every launch of the loop is sized by
    max_frames, so a call of short utterances pays the loop of the capacity (tiles behind an utterance's end only write zeros).
    vocoder=audio.HiFiGAN, audio.BigVGAN, audio.Vocos or audio.WaveGlow (WaveGlow's latent is seeded by the
    call's seed, read from the call block on the device) puts a neural generator there instead, through the one
    contract of DESIGN.md 4.26 (vocoder_iters is ignored): wav_static [batch, vocoder.wav_len(max_frames)], voc_bufs =
    vocoder.buffer_spec(batch, max_frames)'s buffers as static buffers and wav_static (vocoder.workspace_bytes(batch, max_frames)
    bytes: 14 batch max_frames W + 4 batch U max_frames with W = 8192 for HiFi-GAN V1), captured_entries grows by vocoder.launches.
    Its mel_channels must be the model's mel channels (Vocos: its input_channels, a multiple of 16)."""

    RING = 8

    def __init__(self, gen, batch, max_tokens, max_frames, max_rows=None, aux=False, stochastic=False, max_frame_rows=None,
                 vocoder=None, vocoder_iters=30):
        self.stochastic = bool(stochastic)
        if vocoder is not None:                                          # refused before any allocation
            from . import audio
            self.neural = isinstance(vocoder, audio._MelVocoder)         # the contract is all that is used of it
            if self.neural:                                              # vocoder_iters is not its business
                if any(p.device != next(gen.parameters()).device for p in vocoder.parameters()):
                    raise ValueError("compile_synthesis(vocoder=): the vocoder's parameters are not on the model's device")
                vocoder.check_graph_input()
                if vocoder.mel_channels != gen.out_channels:
                    raise ValueError(f"compile_synthesis(vocoder=): the vocoder takes {vocoder.mel_channels} mel channels, the "
                                     f"model writes {gen.out_channels}")
                vocoder_iters = 0
            elif not isinstance(vocoder, audio.GriffinLim) or not isinstance(vocoder.stft, audio.TacotronSTFT):
                raise TypeError("compile_synthesis(vocoder=) takes an audio.HiFiGAN (or audio.BigVGAN), an audio.Vocos, an audio.WaveGlow, or an audio.GriffinLim built over an audio.TacotronSTFT")
            elif vocoder.stft.mel_basis.device != next(gen.parameters()).device or vocoder.istft.inverse_basis.device != next(gen.parameters()).device:
                raise ValueError("compile_synthesis(vocoder=): the vocoder's buffers are not on the model's device")
            elif vocoder.stft.mel_basis.shape[0] != gen.out_channels:
                raise ValueError(f"compile_synthesis(vocoder=): the vocoder inverts {vocoder.stft.mel_basis.shape[0]} mel channels, the "
                                 f"model writes {gen.out_channels}")
            elif int(vocoder_iters) != vocoder_iters or vocoder_iters < 0:
                raise ValueError("compile_synthesis: vocoder_iters is a non-negative integer")
        else:
            self.neural = False
        self.vocoder, self.vocoder_iters = vocoder, int(vocoder_iters)
        if not self.stochastic and (gen.use_sdp or gen.use_spp or gen.use_sep or gen.use_emo_embeds):
            raise NotImplementedError("compile_synthesis covers the deterministic duration predictor with optional speaker / language "
                                      "vectors; stochastic predictors and emotion inputs (cfg 5) are captured with stochastic=True")
        if self.stochastic and gen.noise_key != "frame":
            raise RuntimeError('compile_synthesis(stochastic=True) needs set_synthesis_front(noise_key="frame") in effect: a capture at '
                               "capacity sizes can only reproduce noise that does not depend on the rows layout")
        if not (gen.synthesis_front and gen.decoder.fused_reverse and gen.decoder._inv_cache is not None):
            raise RuntimeError("compile_synthesis needs store_inverse(fused_reverse=True, device_front=True) in effect")
        if gen.n_sqz != 2:
            raise NotImplementedError("compile_synthesis needs n_sqz = 2 (the rows layout of the fused reverse pass)")
        batch, max_tokens, max_frames = int(batch), int(max_tokens), int(max_frames)
        if batch < 1 or batch > _lib.STEP_MAX_B or max_tokens < 1 or max_tokens > _lib.SYNTH_LONG_MAX_TX or max_frames < 2 or max_frames % 2:
            raise ValueError(f"compile_synthesis: 1 <= batch <= 1024, 1 <= max_tokens <= {_lib.SYNTH_LONG_MAX_TX}, max_frames even and >= 2")
        if aux and batch * max_tokens * max_frames > 2 ** 31 - 1:                 # before any allocation: 4 bytes each
            raise ValueError(f"compile_synthesis(aux=True): the static attn buffer has batch * max_tokens * max_frames = "
                             f"{batch} * {max_tokens} * {max_frames} = {batch * max_tokens * max_frames} elements, more than 2^31 - 1")
        self.gen, self.batch, self.max_tokens, self.max_frames, self.aux = gen, batch, max_tokens, max_frames, bool(aux)
        self.max_rows = int(max_rows) if max_rows is not None else default_rows(batch, max_frames, gen.rows_cfg.row_round)
        if self.max_rows < 2 * HALO * batch:
            raise ValueError("compile_synthesis: max_rows leaves no room for the halos of every utterance")
        if self.max_rows % 8:
            # the kernels state no granularity of R; ragged contexts exist, and are tested, with R rounded to 8 and above
            raise ValueError("compile_synthesis: max_rows must be a multiple of 8")
        self.has_prosody = bool(self.stochastic and (gen.use_spp or gen.use_sep))
        self.max_frame_rows = None
        if self.has_prosody:
            self.max_frame_rows = int(max_frame_rows) if max_frame_rows is not None else \
                default_frame_rows(batch, max_frames, gen.rows_cfg.row_round)
            if self.max_frame_rows < 2 * HALO * batch:
                raise ValueError("compile_synthesis: max_frame_rows leaves no room for the halos of every utterance")
            if self.max_frame_rows % 8:
                raise ValueError("compile_synthesis: max_frame_rows must be a multiple of 8")
        self.device = dev = next(gen.parameters()).device
        self.overflows = 0
        self._guards = []
        B, Tx, Ty, R, C = batch, max_tokens, max_frames, self.max_rows, gen.out_channels
        # ---- static inputs: ONE buffer = ids | x_lengths | call block | g | l, uploaded with one copy
        self.g_dim = (512 if gen.use_spk_embeds else gen.gin_channels) if (gen.gin_channels or gen.use_spk_embeds) else 0
        self.takes_l = bool(gen.use_lang_embeds and gen.lin_channels)
        self.takes_emo = bool(self.stochastic and gen.use_emo_embeds)
        n_call = (_lib.SynthCallExt if self.stochastic else _lib.SynthCall)
        lay, off = {}, 0
        for name, n, dt in (("ids", B * Tx, torch.int64), ("x_len", B, torch.int64), ("call", ctypes.sizeof(n_call) // 4, torch.int32),
                            ("g", B * self.g_dim, torch.float32), ("l", B if self.takes_l else 0, torch.int64),
                            ("emo", B if self.takes_emo else 0, torch.int64), ("emo_cartesian", 3 * B if self.takes_emo else 0, torch.float32)):
            lay[name] = (off, n, dt)
            off += (n * torch.empty(0, dtype=dt).element_size() + 15) // 16 * 16
        self._layout, self._in_bytes = lay, off
        self._in = self._static(off, torch.uint8)
        view = lambda name: self._in[lay[name][0]:lay[name][0] + lay[name][1] * torch.empty(0, dtype=lay[name][2]).element_size()].view(lay[name][2])  # noqa: E731
        self.ids, self.x_len, self.call = view("ids").view(B, Tx), view("x_len"), view("call")
        self.g = view("g").view(B, self.g_dim) if self.g_dim else None
        self.l = view("l") if self.takes_l else None
        self.emo = view("emo") if self.takes_emo else None
        self.emo_cartesian = view("emo_cartesian").view(B, 3) if self.takes_emo else None
        self.source = FromBlock(self.call)
        self.length_scale = self.source.length_scale                     # 0-dim: read by the graph's torch plumbing at replay
        # ---- static outputs
        self._back = self._static(B + 1, torch.int32)                    # y_len | status: the call's one readback
        self.y_len, self.status = self._back[:B], self._back[B:]
        self.y_len_eff = self._static(B, torch.int32)
        self.cum = self._static(B * Tx, torch.int32).view(B, Tx)
        self.rows = self._static(R * 2 * C, torch.float32).view(R, 2 * C)
        self.mel_static = self._static(B * C * Ty, torch.float32).view(B, C, Ty)
        self.aux_static = None
        if self.aux:
            self.aux_static = dict(z_m=self._static(B * C * Ty, torch.float32).view(B, C, Ty),
                                   z_logs=self._static(B * C * Ty, torch.float32).view(B, C, Ty),
                                   attn=self._static(B * Tx * Ty, torch.float32).view(B, 1, Tx, Ty),
                                   logw_=self._static(B * Tx, torch.float32).view(B, 1, Tx))
        self.rc = ops.RowsCtx.capacity(B, Ty // 2, R, dev, alloc=self._static)
        self.rc.stamps = None
        # ---- the pitch / energy predictors: frame-rate rows at capacity, their contours, the frame -> token map between the two
        self.rcf = self.frame2token = self.pitch_static = self.energy_static = self.psig = self.esig = None
        if self.has_prosody:
            self.rcf = ops.RowsCtx.capacity(B, Ty, self.max_frame_rows, dev, alloc=self._static)
            self.frame2token = self._static(B * Ty, torch.int32).view(B, Ty)
            if gen.use_spp:
                self.pitch_static, self.psig = self._static(B * Ty, torch.float32).view(B, Ty), self._static(R * 2, torch.float32).view(R, 2)
            if gen.use_sep:
                self.energy_static, self.esig = self._static(B * Ty, torch.float32).view(B, Ty), self._static(R * 2, torch.float32).view(R, 2)
        # ---- the waveform back end: magnitudes, the spectrum workspace, the samples, the frame counts the mel has
        self.wav_static = self.voc_bufs = self.n_frames = self._voc_images = None
        if self.neural:
            # the vocoder names its buffers and their sizes (buffer_spec, which refuses a capacity past its kernels'
            # 2^31 elements) and the samples a frame count gives (wav_len)
            spec = vocoder.buffer_spec(B, Ty)
            self.n_frames = self._static(B, torch.int32)
            self.wav_static = self._static(B * vocoder.wav_len(Ty), torch.float32).view(B, vocoder.wav_len(Ty))
            self.voc_bufs = {name: self._static(n, dtype) for name, dtype, n in spec}
            self.voc_bufs["wav"] = self.wav_static
            self._voc_images = vocoder.held()                            # kept: the graph holds their addresses
        elif vocoder is not None:
            self.n_frames = self._static(B, torch.int32)
            self.wav_static = self._static(B * 256 * (Ty - 1), torch.float32).view(B, 256 * (Ty - 1))
            self.voc_bufs = dict(mag=self._static(B * 513 * Ty, torch.float32).view(B, 513, Ty),
                                 spec=self._static(_lib.call.gt_gl_spec_bytes(B, Ty) // 4, torch.float32), wav=self.wav_static)
            # packed once, outside the launches that are counted; kept here, because the graph holds their addresses and the vocoder
            # drops them when it repacks (a changed mel_basis, .to())
            self._voc_images = (vocoder.istft._image(), vocoder.stft._image(), vocoder.mel_pinv())
        self._ring, self._ring_i = [], 0
        self._latest = None
        self._handed = set()                                             # streams that views of the static outputs were handed out on
        self.stream = torch.cuda.Stream(device=dev)
        self._capture()

    # ---- buffers ----------------------------------------------------------------------------------------------------------------
    def _static(self, n, dtype):
        """n elements between two canary margins (guards_intact checks them), zero-filled"""
        nbytes = max(n, 1) * torch.empty(0, dtype=dtype).element_size()
        pad = (nbytes + 15) // 16 * 16
        flat = torch.full((pad + 2 * GUARD,), CANARY, dtype=torch.uint8, device=self.device)
        flat[GUARD:GUARD + nbytes] = 0
        self._guards.append((flat, nbytes))
        return flat[GUARD:GUARD + nbytes].view(dtype)[:n]

    def guards_intact(self):
        """True when no byte of the canary margins around the static buffers has changed"""
        ok = torch.ones((), dtype=torch.bool, device=self.device)
        for flat, nbytes in self._guards:
            ok = ok & (flat[:GUARD] == CANARY).all() & (flat[GUARD + nbytes:] == CANARY).all()
        return bool(ok)

    # ---- the call, as launches ------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _body(self):
        gen, rcy, rcf, src = self.gen, self.rc, self.rcf, self.source
        dev, B, Ty = self.device, self.batch, self.max_frames
        gen.rows_cfg.host_lengths.clear()
        # the stochastic duration predictor only under stochastic=True (the constructor)
        g, l, x_m, x_logs, x_mask, rc, xb, logw = text_stage(gen, self.ids, self.x_len, self.g, self.l, self.emo, self.emo_cartesian,
                                                             lambda rcx: src.noise(rcx, 1, 1))
        a = self.aux_static or {}
        dur, xl = lengths_stage(logw, x_mask, src.length_scale, self.x_len, self.cum, self.y_len, a.get("logw_"))
        _launch(dev, "gt_synth_geometry", self.y_len, B, Ty, rcy.R, rcy.row0, rcy.lengths, self.y_len_eff, rcy.rowbatch, rcy.rowframe,
                rcy.rowmask, rcy.rowutt, self.status)
        if rcf is not None:                                              # behind gt_synth_geometry: ORs bit 2 into the status word
            _launch(dev, "gt_synth_frame_geometry", self.y_len_eff, B, Ty, rcf.R, rcf.row0, rcf.lengths, rcf.rowbatch, rcf.rowframe,
                    rcf.rowmask, rcf.rowutt, self.status)
        bufs = dict(rows=self.rows, z_m=a.get("z_m"), z_logs=a.get("z_logs"), frame2token=self.frame2token, attn=a.get("attn"),
                    pitch=self.pitch_static, energy=self.energy_static, psig=self.psig, esig=self.esig)
        xm, xs = prior_stage(gen, x_m, x_logs, self.cum, xl, self.y_len_eff, rcy, bufs, src, Ty)
        contours = prosody_stage(gen, g, rc, xb, rcy, rcf, bufs, src, Ty)[2] if rcf is not None else {}
        gen.decoder.reverse_rows(rcy, self.rows, g=g, out=self.mel_static, **contours)
        if self.vocoder is not None:
            # the frames the mel really has (the squeeze drops an odd trailing frame); the phases' seed is the call block's first word
            torch.mul(rcy.lengths, 2, out=self.n_frames)
            if self.neural:
                kw = dict(seed_dev=self.call[:1]) if self.vocoder.seeded else {}     # the latent's seed: the call block's first word
                self.vocoder.run(self.mel_static, self.n_frames, self.voc_bufs, **kw)
            else:
                self.vocoder.run_from_mel(self.mel_static, self.n_frames, self.voc_bufs, self.vocoder_iters, seed_dev=self.call[:1])
        if self.aux:
            a["logw"] = logw
        return xm, xs, xl, dur, logw                                     # kept: the graph replays into these

    def _capture(self):
        dev = self.device
        cur = torch.cuda.current_stream(dev)
        # warm-up inputs: a full-length text of token 1, no noise — whatever lengths come out, the kernels stay inside the capacities
        self.ids.fill_(1)
        self.x_len.fill_(self.max_tokens)
        warm = CallScalars(0, noise_scale=0.0, noise_scale_w=0.0 if self.stochastic else 1.0, f0_noise_scale=0.0, energy_noise_scale=0.0)
        self.call.copy_(warm.words(self.stochastic).to(dev))
        if self.takes_emo:
            self.g.fill_(1.0)                                            # emb_g normalises the speaker vector: not the zero vector
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            # eager, on the capture stream: one-time attribute calls, scratch growth, pointer tables built "outside graph capture"
            with _lib.record_calls() as names:
                self._body()
            self.captured_entries = len(names)                           # C-ABI launches inside the graph (the rest is aten plumbing)
        self.stream.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=self.stream, capture_error_mode="thread_local"):
            self._keep = self._body()
        cur.wait_stream(self.stream)
        torch.cuda.synchronize(dev)

    # ---- calling ------------------------------------------------------------------------------------------------------------------
    def _slot(self):
        """the next [pinned staging of the inputs, pinned readback, event, weakref of the call's handle, read] of the ring; a slot's
        event is recorded behind the readback of the call that used it.  A slot that is taken again is retired first: its call's
        lengths and status go to its handle (if that is still alive) before the next call's readback replaces them."""
        if len(self._ring) < self.RING:
            self._ring.append([torch.zeros(self._in_bytes, dtype=torch.uint8).pin_memory(),
                               torch.zeros(self.batch + 1, dtype=torch.int32).pin_memory(), torch.cuda.Event(), None, True])
            slot = self._ring[-1]
        else:
            slot = self._ring[self._ring_i % self.RING]
            self._retire(slot)
        self._ring_i += 1
        return slot

    def _retire(self, slot):
        """wait for the slot's call, read its y_len | status ONCE: counted in `overflows`, handed to the call's handle"""
        if slot[4]:
            return
        slot[2].synchronize()
        vals = slot[1].tolist()
        slot[4] = True
        if vals[-1] != 0:
            self.overflows += 1
        h = slot[3]() if slot[3] is not None else None
        if h is not None:
            h._read = (vals[:-1], vals[-1])
            h._slot = None
        slot[3] = None

    def __call__(self, x, x_lengths, g=None, l=None, seed=None, noise_scale=1., length_scale=1., emo=None, emo_cartesian=None,
                 noise_scale_w=1., f0_noise_scale=1., energy_noise_scale=1., pitch_scale=1., energy_scale=1.):
        """-> SynthesisHandle.  x [batch, <= max_tokens] ids (zero-padded to max_tokens), x_lengths [batch], g / l as infer takes them;
        host tensors are staged directly (device tensors are read back first).  Nothing is launched when the shapes do not fit.
        stochastic=True: emo [batch] / emo_cartesian [batch, 3] (exactly when the model has the emotion front end) and the scalars of
        the stochastic predictors, as infer takes them; everything is validated before anything is launched."""
        B, Tx = self.batch, self.max_tokens
        if x.dim() != 2 or x.shape[0] != B or x_lengths.shape != (B,):
            raise ValueError(f"this synthesiser is compiled for a batch of {B}: got x {tuple(x.shape)}, x_lengths {tuple(x_lengths.shape)}")
        if x.shape[1] > Tx:
            raise ValueError(f"x has {x.shape[1]} tokens, the synthesiser is compiled for max_tokens = {Tx}")
        if (g is None) != (self.g is None) or (l is None) != (self.l is None):
            raise ValueError("g / l must be given exactly when the model takes a speaker / language vector")
        if g is not None:
            g2 = g.squeeze(-1) if g.dim() == 3 else g
            if g2.shape != (B, self.g_dim):
                raise ValueError(f"g must be [{B}, {self.g_dim}], got {tuple(g.shape)}")
        if l is not None and l.shape != (B,):
            raise ValueError(f"l must be [{B}], got {tuple(l.shape)}")
        if (emo is None) != (not self.takes_emo) or (emo_cartesian is None) != (not self.takes_emo):
            raise ValueError("emo / emo_cartesian must be given exactly when the synthesiser was compiled with stochastic=True for a "
                             "model with the emotion front end")
        if emo is not None and (emo.shape != (B,) or emo_cartesian.shape != (B, 3)):
            raise ValueError(f"emo must be [{B}] and emo_cartesian [{B}, 3], got {tuple(emo.shape)} and {tuple(emo_cartesian.shape)}")
        call = CallScalars(0, *[float(v) for v in (noise_scale, noise_scale_w, length_scale, f0_noise_scale, energy_noise_scale, pitch_scale,
                                                   energy_scale)])
        if not self.stochastic and (call.noise_scale_w, *call[4:]) != (1., 1., 1., 1., 1.):
            raise ValueError("noise_scale_w / f0_noise_scale / energy_noise_scale / pitch_scale / energy_scale need compile_synthesis(stochastic=True)")
        if seed is None:
            seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())      # torch's default CPU generator, as infer does
        call = call._replace(seed=int(seed) & 0xFFFFFFFF)
        slot = self._slot()
        host, back, ev = slot[:3]
        lay = self._layout

        def put(name, shape=None):
            o, n, dt = lay[name]
            v = host[o:o + n * torch.empty(0, dtype=dt).element_size()].view(dt)
            return v if shape is None else v.view(shape)

        ids = put("ids", (B, Tx))
        ids.zero_()
        ids[:, :x.shape[1]].copy_(x)
        put("x_len").copy_(x_lengths)
        put("call").copy_(call.words(self.stochastic))
        if g is not None:
            put("g", (B, self.g_dim)).copy_(g2)
        if l is not None:
            put("l").copy_(l)
        if emo is not None:
            put("emo").copy_(emo)
            put("emo_cartesian", (B, 3)).copy_(emo_cartesian)
        prev = self._latest() if self._latest is not None else None
        if self._handed:
            # (no wait when nothing was handed out: clones are made on the synthesiser's own stream, so queued calls and callers that
            # only clone never serialise with the caller's stream.)  Views of the static outputs are in use: this replay overwrites them only behind what their streams, and the stream this
            # call comes from, have queued so far
            for st in self._handed | {torch.cuda.current_stream(self.device)}:
                self.stream.wait_stream(st)
            self._handed.clear()
        with torch.cuda.stream(self.stream):
            if prev is not None and not prev._done and prev._saved is None and (prev._read is None or prev._read[1] == 0):
                # the previous call has not been read yet: its outputs move aside, in stream order, before this call overwrites them
                saved_ev = torch.cuda.Event()
                prev._saved = (self.mel_static.clone(), {k: v.clone() for k, v in self.aux_static.items()} if self.aux else None, saved_ev,
                               tuple(None if t is None else t.clone() for t in (self.pitch_static, self.energy_static)),
                               None if self.wav_static is None else self.wav_static.clone())
                saved_ev.record(self.stream)
            self._in.copy_(host, non_blocking=True)
            self.graph.replay()
            back.copy_(self._back, non_blocking=True)
            ev.record(self.stream)
        h = SynthesisHandle(self, slot, (x, x_lengths, g, l, emo, emo_cartesian), call)
        slot[3], slot[4] = weakref.ref(h), False
        self._latest = weakref.ref(h)
        return h
