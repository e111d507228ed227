"""Device mel front end: the reference's STFT / TacotronSTFT (stft.py:41-101, commons.py:279-317) with the transform
run by ONE HIP kernel (csrc/mel_front.hip: gt_mel_pack once, gt_mel_spectrogram per batch) instead of librosa on the CPU.

  STFT              carries `forward_basis` [2 * 513, 1, 1024] built as the reference builds it (float64 np.fft.fft(np.eye(N)), rows
                    [:513] real then imaginary, times the periodic Hann window, rounded to fp32 once).
  TacotronSTFT      carries `mel_basis` [n_mel, 513] (a plain buffer: a checkpoint's or librosa's own matrix loads over it) and
                    `.stft_fn`; `mel_spectrogram(y)` is the reference's call, `mel_spectrogram(y, lengths)` the batched form whose
                    outputs are what `Trainer.step(y=, t_y=, energy=)` and `data.TextMelCollate` use.
  mel_filterbank    NumPy restatement of librosa.filters.mel's defaults (Slaney scale, triangular filters, norm="slaney").
  YIN               the pitch contour of the reference's get_f0 (yin.compute_yin) for padded batches by ONE kernel (csrc/yin_front.hip:
                    gt_yin_f0); `f0(y, lengths)` lines up with `TacotronSTFT.mel_spectrogram(y, lengths)`.
  compute_yin       the reference's signature for one device waveform.
  InverseSTFT       carries `inverse_basis` [2 * 513, 1, 1024] (the reference's pinv(4 fourier_basis).T times the window, float64,
                    rounded once); `inverse(magnitude, phase[, frames])` is the reference's STFT.inverse by two kernels
                    (csrc/griffin_lim.hip: gt_gl_polar, gt_istft).  A class of its own: STFT keeps its buffers.
  GriffinLim        the reference's griffin_lim loop on an STFT / TacotronSTFT: gt_gl_project (analysis, Y = M X / |X|) and gt_istft
                    per iteration, 2 + 2 n launches, no host synchronisation; `from_mel` starts from a log-mel —
                    with phases="counter" through ONE kernel (csrc/gl_mel.hip: gt_gl_from_mel) that writes the
                    magnitudes and the initial spectrum, phases keyed by (seed, utterance, frame, bin); `mel_workspace` /
                    `run_from_mel` are its capacity-sized form for graph callers (synthesis.Synthesizer).
  griffin_lim       the reference's signature.
  Resample          rational-rate conversion of padded batches by ONE kernel (csrc/resample.hip: gt_resample) with the
                    definition of scipy.signal.resample_poly (default window, zero padding); carries the fp32 phase `bank`.
                    `mel_spectrogram(..., sampling_rate=)` and `YIN.f0(..., sampling_rate=)` resample first; `resample_poly` is scipy's
                    signature for one device waveform, `resample_filter64` / `resample_bank64` the float64 prototype and its phases.

  HiFiGAN           the published HiFi-GAN generator (eval mode, weight norm folded) from log-mel to samples, every layer by ONE kernel
                    (csrc/hifigan.hip: gt_voc_conv), every utterance of a ragged batch on its own; loads the original
                    checkpoints (`load_generator_state`, `from_config`); `workspace` / `run` are its capacity-sized form for graph
                    callers (synthesis.Synthesizer).  `transposed_as_conv`, `voc_pack`: the weight forms it runs on.

  BigVGAN           the published BigVGAN generator: HiFiGAN (which it subclasses) with the anti-aliased snake activation, ONE launch of
                    the stand-alone kernel gt_voc_snake (csrc/voc_snake.hip) in front of every convolution but the
                    transposed ones; the original parameter tree and checkpoints; a 24-channel stage runs padded to 32.

  Vocos             the published Vocos generator (ConvNeXt backbone at frame rate, iSTFT head): csrc/vocos.hip's gt_vocos_norm,
                    gt_vocos_mlp (the block's MLP with the hidden activation kept on the chip) and gt_vocos_polar next to gt_voc_conv and
                    gt_istft; the published parameter tree (`load_vocos_state`, `from_config`), the capacity-sized form.

  WaveGlow          the published WaveGlow network in its `infer` direction (the vocoder Glow-TTS was published with): csrc/waveglow.hip's
                    gt_wg_gate (a WaveNet layer's in_layer + conditioning slice + gate as one implicit GEMM) and gt_wg_boundary
                    (everything between two WaveNets) next to gt_voc_conv; a seeded latent from the counter generator;
                    the published parameter tree (`load_waveglow_state`, `from_config`), the capacity-sized form.

  Denoiser          NVIDIA's WaveGlow `Denoiser` (spectral subtraction of the network's own bias spectrum, mode "zeros") by csrc/denoise.hip's
                    gt_denoise_spec (the analysis with the subtraction as its epilogue) and gt_istft; `from_vocoder`
                    measures the bias, `denoise` is the stand-alone use, `workspace` / `run` the capacity-sized form.
  Denoised          a vocoder with a Denoiser behind it, itself a `_MelVocoder`: compile_synthesis(vocoder=Denoised(WaveGlow(...))).

  Loudness          ITU-R BS.1770-4 integrated loudness (K-weighting, 400 ms blocks, both gates) and normalisation to a target under a
                    sample peak ceiling, by csrc/loudness.hip's gt_loudness_measure and gt_loudness_apply: a serial
                    IIR run in parallel over chunks, exactly, in double; `measure` / `normalize` are the stand-alone uses on padded
                    fp32 or int16 batches, `workspace` / `run` the capacity-sized form.  `kweighting64`, `kweighting_transition64`:
                    the float64 coefficients and the chunk transition matrix the kernels read.
  Normalized        a vocoder with a Loudness stage behind it, itself a `_MelVocoder`: Normalized(Denoised(WaveGlow(...))).

  The generators meet one contract, `_MelVocoder`: mel_channels, wav_len, buffer_spec(B, F_max), held, and the
  shared forward / workspace / workspace_bytes / run that compile_synthesis(vocoder=) uses.

Waveforms are fp32 in [-1, 1] or int16 (scaled by 1/32768 in the kernel = the reference's audio / max_wav_value).  There is no CPU
path: a CPU tensor raises."""
from fractions import Fraction

import numpy as np
import torch
from torch import nn

from . import _lib
from ._lib import call

CLIP_VAL = 1e-5                      # audio_processing.dynamic_range_compression's clip_val


class CpuWaveError(_lib.CpuTensorError, ValueError):
    """a CPU waveform: the wrong value for a device op (ValueError), and the CpuTensorError every other op here raises"""


class _Cached:
    """one value derived from buffers, rebuilt when the (data_ptr, _version) of any of them changes (load_state_dict, .to(), an
    in-place edit): the packed images and mel_pinv"""
    def __init__(self):
        self.key, self.value = None, None

    def get(self, tensors, build):
        key = tuple(v for t in tensors for v in (t.data_ptr(), t._version))
        if self.key != key:
            self.value, self.key = build(), key
        return self.value


def _device_rows(y):
    """waveform rows as the kernels take them (16-byte aligned rows of a 4-element pitch): y itself, or a zero-padded copy"""
    if not y.is_cuda:
        raise CpuWaveError("glow_tts_amd.audio runs on the MI355X only (got a CPU waveform); there is no CPU fallback")
    if y.dim() != 2 or y.dtype not in (torch.float32, torch.int16):
        raise ValueError(f"waveforms are [B, T] fp32 or int16, got {tuple(y.shape)} {y.dtype}")
    B, T = y.shape
    if y.stride(1) != 1 or y.stride(0) % 4 or y.data_ptr() % 16:
        padded = y.new_zeros(B, (T + 3) // 4 * 4)
        padded[:, :T] = y
        y = padded
    return y


def _wav_len_arg(wav_len, y):
    if wav_len.device != y.device or wav_len.dtype != torch.int32 or wav_len.numel() != y.shape[0]:
        raise ValueError("wav_len must be int32 [B] on the waveforms' device")
    return wav_len.contiguous()


def _ragged_frames(y, lengths, lengths_host, hop, min_len=None):
    """padded rows y [B, T] and their sample counts (`lengths`, default T) -> (the counts on y's device, in their own dtype (int32 when
    defaulted), F_max frames per output row): F_max = 1 + max(lengths) // hop where the host knows the lengths (lengths_host, or CPU
    `lengths`), else 1 + T // hop with no synchronisation.  TacotronSTFT.mel_spectrogram and YIN.f0 both choose it here.  min_len (mel
    only: filter_length / 2): a length <= it has no reflect padding, a ValueError where the host knows it."""
    if not y.is_cuda:
        raise CpuWaveError("glow_tts_amd.audio runs on the MI355X only (got a CPU waveform); there is no CPU fallback")
    B, T = y.shape
    if lengths is None:
        if min_len is not None and T <= min_len:
            raise ValueError(f"{T} samples: reflect padding needs more than {min_len}")
        return torch.full((B,), T, dtype=torch.int32, device=y.device), 1 + T // hop
    if lengths_host is None and not lengths.is_cuda:
        lengths_host = lengths.tolist()
    F_max = 1 + T // hop
    if lengths_host is not None:
        lengths_host = [int(v) for v in lengths_host]
        if len(lengths_host) != B or max(lengths_host) > T:
            raise ValueError(f"lengths {lengths_host} do not fit waveforms {tuple(y.shape)}")
        if min_len is not None and min(lengths_host) <= min_len:
            raise ValueError(f"an utterance of {min(lengths_host)} samples: reflect padding needs more than {min_len}")
        F_max = 1 + max(lengths_host) // hop
    return lengths.to(y.device, non_blocking=True), F_max


# ---- sample-rate conversion: scipy.signal.resample_poly's definition on csrc/resample.hip -----------------------
def _reduced(up, down):
    up, down = int(up), int(down)
    if up <= 0 or down <= 0:
        raise ValueError(f"up and down are positive integers, got {up}, {down}")
    g = int(np.gcd(up, down))
    return up // g, down // g


def resample_filter64(up, down):
    """float64 [20 max(up, down) + 1]: the prototype filter of scipy.signal.resample_poly(x, up, down) with its default window —
    firwin(2 half + 1, 1 / max(up, down), window=('kaiser', 5.0)) * up with half = 10 max(up, down): fc sinc(fc n) times the
    symmetric Kaiser window (beta = 5), normalised to unit sum, times up.  (up, down) is reduced first.  Our own restatement: the
    product does not import scipy (tests/test_resample_host.py compares the two)."""
    up, down = _reduced(up, down)
    m = max(up, down)
    half = 10 * m
    n = np.arange(-half, half + 1, dtype=np.float64)
    h = np.sinc(n / m) / m * np.kaiser(2 * half + 1, 5.0)
    return h / h.sum() * up


def resample_bank64(up, down):
    """float64 [up, T]: the phases of resample_filter64, bank[p, j] = h[p + j up] and 0 past the end of h, T = ceil(len(h) / up)"""
    up, down = _reduced(up, down)
    h = resample_filter64(up, down)
    T = -(-len(h) // up)
    full = np.zeros(up * T)
    full[:len(h)] = h
    return np.ascontiguousarray(full.reshape(T, up).T)


def resample_out_len(length, up, down):
    """ceil(length up / down): the samples resample_poly returns for `length` (a Python int: no overflow)"""
    return -(-int(length) * up // down)


class Resample(nn.Module):
    """Rational-rate conversion orig_freq -> new_freq of padded batches by ONE HIP kernel (csrc/resample.hip: gt_resample), every
    utterance resampled on its own with the definition of scipy.signal.resample_poly(x, up, down) (default window, zero padding),
    up / down = new_freq / orig_freq reduced.  Carries the fp32 `bank` [up, taps] (resample_bank64 rounded once).  A pair of rates
    the kernel does not take (its bank and a tile's input span do not fit the LDS) is a ValueError here."""

    def __init__(self, orig_freq, new_freq):
        super().__init__()
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        self.up, self.down = _reduced(self.new_freq, self.orig_freq)
        self.taps = call.gt_resample_taps(self.up, self.down)
        if self.taps == 0:
            raise ValueError(f"{orig_freq} -> {new_freq} Hz (up {self.up}, down {self.down}) is outside what gt_resample takes")
        self.register_buffer("bank", torch.from_numpy(resample_bank64(self.up, self.down).astype(np.float32)))

    def out_len(self, length):
        return resample_out_len(length, self.up, self.down)

    def transform(self, y, wav_len, L_cap):
        """the kernel call: y [B, T] fp32 / int16 on the device, wav_len device int32 [B], L_cap samples per output row ->
        (out [B, L_cap] fp32, out_len device int32 [B] = min(ceil(wav_len up / down), L_cap)), row b zero behind its samples; rows at a
        pitch of L_cap rounded up to 4.  No host synchronisation, capturable in a graph."""
        y = _device_rows(y)
        wav_len = _wav_len_arg(wav_len, y)
        bank = self.bank
        if bank.device != y.device or bank.dtype != torch.float32 or tuple(bank.shape) != (self.up, self.taps) or not bank.is_contiguous():
            raise ValueError(f"bank must be a contiguous fp32 [{self.up}, {self.taps}] buffer on the waveforms' device")
        if L_cap <= 0:
            raise ValueError(f"L_cap = {L_cap}: no output sample")
        B = y.shape[0]
        ld = (L_cap + 3) // 4 * 4
        out = torch.empty(B, ld, dtype=torch.float32, device=y.device)
        out_len = torch.empty(B, dtype=torch.int32, device=y.device)
        call.gt_resample(y, int(y.dtype == torch.int16), y.stride(0), wav_len, B, bank, self.up, self.down, self.taps, out, ld, out_len,
                         _lib.current_stream(y.device))
        if ld != L_cap:                                                       # the kernel's capacity is the pitch
            out, out_len = out[:, :L_cap], out_len.clamp_(max=L_cap)
        return out, out_len

    def host_lengths(self, y, lengths, lengths_host):
        """the output lengths where the host knows the input's (lengths_host, CPU `lengths`, or no lengths at all), else None"""
        if lengths is None:
            return [self.out_len(y.shape[1])] * y.shape[0]
        if lengths_host is None and not lengths.is_cuda:
            lengths_host = lengths.tolist()
        return None if lengths_host is None else [self.out_len(v) for v in lengths_host]

    def forward(self, y, lengths=None, lengths_host=None):
        """y [B, T] (lengths: sample counts of the padded rows, default T) -> (out [B, L_cap] fp32, out_lengths int32 [B] on the
        device = ceil(lengths up / down)); L_cap = max(out_lengths) where the host knows the lengths (lengths_host, or CPU `lengths`),
        else ceil(T up / down) with no synchronisation — as _ragged_frames chooses F_max.  Equal rates: the input as fp32 (int16
        scaled by 1/32768) and its lengths, no launch."""
        if not y.is_cuda:
            raise CpuWaveError("glow_tts_amd.audio runs on the MI355X only (got a CPU waveform); there is no CPU fallback")
        if y.dim() != 2 or y.dtype not in (torch.float32, torch.int16):
            raise ValueError(f"waveforms are [B, T] fp32 or int16, got {tuple(y.shape)} {y.dtype}")
        B, T = y.shape
        if lengths is None:
            wav_len = torch.full((B,), T, dtype=torch.int32, device=y.device)
        else:
            if lengths.numel() != B:
                raise ValueError("lengths must be [B]")
            wav_len = lengths.to(y.device, non_blocking=True).to(torch.int32)
        if lengths_host is None and lengths is not None and not lengths.is_cuda:
            lengths_host = lengths.tolist()
        if lengths_host is not None and (len(lengths_host) != B or max(int(v) for v in lengths_host) > T):
            raise ValueError(f"lengths {list(lengths_host)} do not fit waveforms {tuple(y.shape)}")
        if self.up == self.down:
            return (y if y.dtype == torch.float32 else y.float() / 32768.0), wav_len
        out_host = self.host_lengths(y, lengths, lengths_host)
        L_cap = max(out_host) if out_host is not None else self.out_len(T)
        return self.transform(y, wav_len, max(L_cap, 1))


def resample_poly(x, up, down):
    """scipy.signal.resample_poly's signature (default window and padding) for ONE device waveform x [L] (fp32 or int16) ->
    fp32 [ceil(L up / down)]"""
    if x.dim() != 1:
        raise ValueError(f"resample_poly takes one waveform [L], got {tuple(x.shape)}")
    if not x.is_cuda:
        raise CpuWaveError("glow_tts_amd.audio runs on the MI355X only (got a CPU waveform); there is no CPU fallback")
    up, down = _reduced(up, down)
    if x.shape[0] == 0:
        return torch.empty(0, dtype=torch.float32, device=x.device)
    out, _ = Resample(down, up).to(x.device)(x.unsqueeze(0))
    return out[0, :resample_out_len(x.shape[0], up, down)]


class _RateCache:
    """the Resample modules of a front end, one per (input rate, device), built at the first call that names the rate.  Not a
    submodule: the front end's parameters, buffers and state_dict stay what they are."""

    def __init__(self, new_freq):
        self.new_freq, self.mods = new_freq, {}

    def convert(self, y, lengths, lengths_host, sampling_rate):
        """(y, lengths, lengths_host) at `sampling_rate` -> the same at the front end's rate: the device out_len of the kernel as
        the lengths, the host's count beside it where the host knows the input's"""
        if not y.is_cuda:
            raise CpuWaveError("glow_tts_amd.audio runs on the MI355X only (got a CPU waveform); there is no CPU fallback")
        key = (int(sampling_rate), y.device)
        if key not in self.mods:
            self.mods[key] = Resample(sampling_rate, self.new_freq).to(y.device)
        mod = self.mods[key]
        out_host = mod.host_lengths(y, lengths, lengths_host)
        out, out_len = mod(y, lengths, lengths_host)
        return out, (None if lengths is None else out_len), (None if lengths is None else out_host)


def hann_periodic(win_length):
    """scipy.signal.get_window('hann', win_length, fftbins=True) in float64"""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win_length, dtype=np.float64) / win_length)


def _hz_to_mel(f):
    f = np.asanyarray(f, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3.0, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, min_log_hz) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m):
    m = np.asanyarray(m, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3.0, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_filterbank(sr, n_fft, n_mels, fmin=0.0, fmax=None):
    """librosa.filters.mel(sr=, n_fft=, n_mels=, fmin=, fmax=) with its defaults (htk=False, norm="slaney") -> fp32 [n_mels, 1 + n_fft // 2].
    Filter i is the triangle over mel points i, i + 1, i + 2 (equally spaced on the Slaney scale: linear below 1 kHz, log above),
    sampled at the FFT bin frequencies and scaled by 2 / (f[i + 2] - f[i])."""
    fmax = sr / 2.0 if fmax is None else fmax
    freqs = np.linspace(0.0, sr / 2.0, 1 + n_fft // 2)
    pts = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(pts)
    ramps = pts[:, None] - freqs[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    w = np.maximum(0.0, np.minimum(lower, upper))
    w *= (2.0 / (pts[2:] - pts[:-2]))[:, None]
    return w.astype(np.float32)


class STFT(nn.Module):
    def __init__(self, filter_length=1024, hop_length=256, win_length=1024, window="hann"):
        super().__init__()
        if window != "hann":
            raise ValueError("only the reference's 'hann' window is built here; load another basis over forward_basis")
        if win_length > filter_length:
            raise ValueError("win_length > filter_length")
        self.filter_length, self.hop_length, self.win_length, self.window = filter_length, hop_length, win_length, window
        n, cutoff = filter_length, filter_length // 2 + 1
        fourier = np.fft.fft(np.eye(n))
        basis = np.vstack([np.real(fourier[:cutoff]), np.imag(fourier[:cutoff])])
        win = np.zeros(n)
        lpad = (n - win_length) // 2                                          # librosa.util.pad_center
        win[lpad:lpad + win_length] = hann_periodic(win_length)
        self.register_buffer("forward_basis", torch.from_numpy((basis * win[None, :]).astype(np.float32))[:, None, :].contiguous())


class TacotronSTFT(nn.Module):
    def __init__(self, filter_length=1024, hop_length=256, win_length=1024, n_mel_channels=80, sampling_rate=22050, mel_fmin=0.0,
                 mel_fmax=8000.0):
        super().__init__()
        self.n_mel_channels, self.sampling_rate = n_mel_channels, sampling_rate
        self.stft_fn = STFT(filter_length, hop_length, win_length)
        self.register_buffer("mel_basis", torch.from_numpy(mel_filterbank(sampling_rate, filter_length, n_mel_channels, mel_fmin, mel_fmax)))
        self._packed = _Cached()
        self._rates = _RateCache(sampling_rate)

    # -- the fragment-order image of both buffers, rebuilt when either changes
    def _image(self):
        fb, mb = self.stft_fn.forward_basis, self.mel_basis
        def build():
            if fb.dtype != torch.float32 or mb.dtype != torch.float32 or not fb.is_contiguous() or not mb.is_contiguous():
                raise ValueError("forward_basis and mel_basis must be contiguous fp32 buffers")
            if mb.dim() != 2 or mb.shape[1] != self.stft_fn.filter_length // 2 + 1 or fb.shape[0] != 2 * mb.shape[1]:
                raise ValueError(f"mel_basis {tuple(mb.shape)} does not fit forward_basis {tuple(fb.shape)}")
            packed = torch.empty(call.gt_mel_pack_bytes() // 4, dtype=torch.float32, device=fb.device)
            call.gt_mel_pack(fb, mb, self.stft_fn.filter_length, mb.shape[0], packed, _lib.current_stream(fb.device))
            return packed
        return self._packed.get((fb, mb), build)

    def transform(self, y, wav_len, F_max, magnitudes=False):
        """the kernel call: y [B, T] fp32 / int16 on the device, wav_len device int32 [B], F_max frames per output row ->
        (mel [B, n_mel, F_max], energy [B, F_max], mag [B, 513, F_max] or None); no host synchronisation, capturable in a graph
        once the image exists (any earlier call)."""
        y = _device_rows(y)
        wav_len = _wav_len_arg(wav_len, y)
        B = y.shape[0]
        fs = self.stft_fn
        n_mel = self.mel_basis.shape[0]
        packed = self._image()
        mel = torch.empty(B, n_mel, F_max, dtype=torch.float32, device=y.device)
        energy = torch.empty(B, F_max, dtype=torch.float32, device=y.device)
        mag = torch.empty(B, fs.filter_length // 2 + 1, F_max, dtype=torch.float32, device=y.device) if magnitudes else None
        call.gt_mel_spectrogram(y, int(y.dtype == torch.int16), y.stride(0), wav_len, B, F_max, packed, fs.filter_length,
                                fs.hop_length, fs.win_length, n_mel, CLIP_VAL, mel, energy, mag, _lib.current_stream(y.device))
        return mel, energy, mag

    def mel_spectrogram(self, y, lengths=None, lengths_host=None, sampling_rate=None):
        """mel_spectrogram(y): the reference's call, y [B, T] -> (mel [B, n_mel, F], energy [B, F]), F = 1 + T // hop.
        mel_spectrogram(y, lengths[, lengths_host]): padded rows of a batch with their sample counts -> (mel [B, n_mel, F_max],
        mel_lengths = 1 + lengths // hop, energy [B, 1, F_max]), every utterance transformed on its own (reflected about its own ends)
        and zero behind its frames.  F_max comes from the lengths when the host knows them (lengths_host, or CPU `lengths`), else from
        T with no synchronisation.  A length <= filter_length / 2 has no reflect padding: ValueError where the host knows it.
        sampling_rate: the rate of y where it is not this module's — y is resampled first (audio.Resample, cached per rate; its
        device out_len are the lengths of the transform), and everything above holds for the resampled batch."""
        if sampling_rate is not None and int(sampling_rate) != int(self.sampling_rate):
            y, lengths, lengths_host = self._rates.convert(y, lengths, lengths_host, sampling_rate)
        hop = self.stft_fn.hop_length
        ragged = lengths is not None
        lengths, F_max = _ragged_frames(y, lengths, lengths_host, hop, min_len=self.stft_fn.filter_length // 2)
        mel, energy, _ = self.transform(y, lengths.to(torch.int32), F_max)
        if not ragged:
            return mel, energy
        return mel, 1 + lengths // hop, energy.unsqueeze(1)


class YIN(nn.Module):
    """The pitch contour of the reference's get_f0 (yin.compute_yin: frame 1024, hop 256, 50-600 Hz, threshold 0.1, two zero frames
    on each side) for padded batches, by ONE HIP kernel (csrc/yin_front.hip: gt_yin_f0).  No parameters, no buffers.
    A frame of digital silence is f0 = 0, harm = 1, argmin_f0 = 0 (the reference divides 0 / 0 there)."""

    def __init__(self, sampling_rate=22050, frame_length=1024, hop_length=256, f0_min=50, f0_max=600, harm_thresh=0.1, pad_frames=None):
        super().__init__()
        self.sampling_rate, self.frame_length, self.hop_length = sampling_rate, frame_length, hop_length
        self.f0_min, self.f0_max, self.harm_thresh = f0_min, f0_max, harm_thresh
        self.tau_min, self.tau_max = int(sampling_rate / f0_max), int(sampling_rate / f0_min)
        self.pad_frames = int((frame_length / hop_length) / 2) if pad_frames is None else pad_frames
        self._rates = _RateCache(sampling_rate)

    def transform(self, y, wav_len, F_max, aux=False, lead=None):
        """the kernel call: y [B, T] fp32 / int16 on the device, wav_len device int32 [B], F_max positions per output row ->
        (f0 [B, F_max], harm or None, argmin_f0 or None); frame i of an utterance lands at position lead + i (lead: pad_frames),
        every other position is 0.  No host synchronisation, capturable in a graph."""
        y = _device_rows(y)
        wav_len = _wav_len_arg(wav_len, y)
        B = y.shape[0]
        f0 = torch.empty(B, F_max, dtype=torch.float32, device=y.device)
        harm = torch.empty_like(f0) if aux else None
        amin = torch.empty_like(f0) if aux else None
        call.gt_yin_f0(y, int(y.dtype == torch.int16), y.stride(0), wav_len, B, F_max, self.frame_length, self.hop_length,
                       self.tau_min, self.tau_max, float(self.sampling_rate), float(self.harm_thresh),
                       self.pad_frames if lead is None else lead, f0, harm, amin, _lib.current_stream(y.device))
        return f0, harm, amin

    def f0(self, y, lengths=None, lengths_host=None, aux=False, sampling_rate=None):
        """y [B, T] (lengths: sample counts of the padded rows, default T) -> f0 [B, 1, F_max] with F_max = 1 + max(lengths) // hop,
        chosen as TacotronSTFT.mel_spectrogram(y, lengths) chooses it (from the lengths where the host knows them, else from T with
        no synchronisation): the contour lines up with that call's mel and energy, zero behind every utterance's frames.
        aux=True: (f0, harm [B, 1, F_max], argmin_f0 [B, 1, F_max]).
        sampling_rate: the rate of y where it is not this module's — y is resampled first, as mel_spectrogram(..., sampling_rate=)
        does: the two still line up."""
        if sampling_rate is not None and int(sampling_rate) != int(self.sampling_rate):
            y, lengths, lengths_host = self._rates.convert(y, lengths, lengths_host, sampling_rate)
        lengths, F_max = _ragged_frames(y, lengths, lengths_host, self.hop_length)
        f0, harm, amin = self.transform(y, lengths.to(torch.int32), F_max, aux=aux)
        if aux:
            return f0.unsqueeze(1), harm.unsqueeze(1), amin.unsqueeze(1)
        return f0.unsqueeze(1)

    forward = f0


def compute_yin(sig, sr, w_len=512, w_step=256, f0_min=100, f0_max=500, harmo_thresh=0.1):
    """The reference's yin.compute_yin (same signature and defaults) for ONE device waveform sig [L] (fp32 or int16):
    -> (pitches, harmonic_rates, argmins, times), tensors of len(range(0, L - w_len, w_step)) entries, unpadded.  The kernel takes
    w_len = 1024, w_step = 256 and tau_max = int(sr / f0_min) <= 512; any other geometry (the defaults included) raises."""
    if sig.dim() != 1:
        raise ValueError(f"compute_yin takes one waveform [L], got {tuple(sig.shape)}")
    L = sig.shape[0]
    n = len(range(0, L - w_len, w_step))
    mod = YIN(sr, w_len, w_step, f0_min, f0_max, harmo_thresh, pad_frames=0)
    wav_len = torch.full((1,), L, dtype=torch.int32, device=sig.device)
    f0, harm, amin = mod.transform(sig.unsqueeze(0), wav_len, max(n, 1), aux=True)
    times = torch.arange(n, dtype=torch.float32, device=sig.device) * (w_step / float(sr))
    return f0[0, :n], harm[0, :n], amin[0, :n], times


# ---- waveform back end: the reference's STFT.inverse and griffin_lim on csrc/griffin_lim.hip ---------------------
def inverse_basis64(filter_length=1024, hop_length=256, win_length=1024):
    """float64 [2 * cutoff, n]: the reference's pinv(scale * fourier_basis).T times the centre-padded periodic Hann window, scale =
    filter_length / hop_length.  The pseudo-inverse of the real/imaginary DFT rows is the irfft weighting in closed form — row k is
    (cos, -sin)(2 pi k n / n_fft) * c_k / (n_fft * scale), c_k = 1 for bins 0 and n_fft / 2, else 2 (np.linalg.pinv agrees to
    3e-16, tests/test_griffin_lim_host.py) — written so that columns n and n_fft - n are exact mirrors and the sine rows of bins 0
    and n_fft / 2 exact zeros, which the float64 pinv only approximates."""
    n, cutoff, half = filter_length, filter_length // 2 + 1, filter_length // 2
    k = np.arange(cutoff, dtype=np.int64)[:, None]
    m = (k * np.arange(half + 1, dtype=np.int64)[None, :]) % n
    ang = 2.0 * np.pi * m.astype(np.float64) / n
    c_k = np.where((k == 0) | (k == half), 1.0, 2.0) / (n * (filter_length / hop_length))
    cos_h = np.cos(ang) * c_k
    sin_h = np.where((2 * m) % n == 0, 0.0, -np.sin(ang)) * c_k
    win = np.zeros(n)
    lpad = (n - win_length) // 2
    win[lpad:lpad + win_length] = hann_periodic(win_length)
    cos_h, sin_h = cos_h * win[None, :half + 1], sin_h * win[None, :half + 1]
    full = np.empty((2 * cutoff, n))
    full[:cutoff, :half + 1], full[cutoff:, :half + 1] = cos_h, sin_h
    full[:cutoff, half + 1:], full[cutoff:, half + 1:] = cos_h[:, half - 1:0:-1], -sin_h[:, half - 1:0:-1]
    return full


def spec_unpack(spec, B, F_max):
    """dev / tests: the kernels' spectrum workspace (include/glowtts_hip.h, gt_gl_*) -> (re, im) [B, 513, F_max]; Im of bin 512 is 0.
    The Python mirror of the layout that csrc/stft_tile.h defines (frames_padded, spec_row_floats, spec_slot, spec_nyq_slot)."""
    tile = call.gt_gl_tile_frames()
    Fp = (F_max + tile - 1) // tile * tile
    rows = spec.view(B, Fp * 1025)
    k = torch.arange(512, device=spec.device)[:, None]
    f = torch.arange(F_max, device=spec.device)[None, :]
    idx = ((((f >> 5) * 64 + (k >> 3)) * 64 + (k & 1) * 32 + (f & 31)) * 8 + ((k & 7) >> 1)).reshape(-1)
    re = torch.cat([rows[:, idx].view(B, 512, F_max), rows[:, Fp * 1024:Fp * 1024 + F_max].unsqueeze(1)], 1)
    im = torch.cat([rows[:, idx + 4].view(B, 512, F_max), torch.zeros_like(re[:, :1])], 1)
    return re, im


def _check_geometry(fs):
    if (fs.filter_length, fs.hop_length, fs.win_length) != (1024, 256, 1024):
        raise ValueError("the waveform back end takes filter_length = win_length = 1024, hop_length = 256 (every reference config)")


def _spectrogram_arg(t, name):
    if not t.is_cuda:
        raise CpuWaveError("glow_tts_amd.audio runs on the MI355X only (got a CPU tensor); there is no CPU fallback")
    if t.dim() != 3 or t.shape[1] != 513 or t.dtype != torch.float32:
        raise ValueError(f"{name} is fp32 [B, 513, F], got {tuple(t.shape)} {t.dtype}")
    return t.contiguous()


def _frames_arg(frames, frames_host, B, F, device):
    """-> device int32 [B] frame counts; F_b < 4 (no reflect padding: 256 (F_b - 1) <= 512) raises where the host knows the counts"""
    if frames is None:
        if F < 4:
            raise ValueError(f"{F} frames: reflect padding needs at least 4")
        return torch.full((B,), F, dtype=torch.int32, device=device)
    if frames_host is None and not frames.is_cuda:
        frames_host = frames.tolist()
    if frames_host is not None:
        frames_host = [int(v) for v in frames_host]
        if len(frames_host) != B or max(frames_host) > F:
            raise ValueError(f"frame counts {frames_host} do not fit a [{B}, 513, {F}] spectrogram")
        if min(frames_host) < 4:
            raise ValueError(f"an utterance of {min(frames_host)} frames: reflect padding needs at least 4")
    elif F < 2:
        raise ValueError(f"{F} frames: no sample")
    if frames.numel() != B:
        raise ValueError("frames must be [B]")
    return frames.to(device, non_blocking=True).to(torch.int32).contiguous()


class InverseSTFT(nn.Module):
    """The reference's STFT.inverse (stft.py:121-148, CUDA branch) by gt_gl_polar + gt_istft.  Carries `inverse_basis`
    [2 * 513, 1, 1024] = inverse_basis64() rounded to fp32 once; a class of its own, so that STFT / TacotronSTFT keep their buffers."""

    def __init__(self, filter_length=1024, hop_length=256, win_length=1024):
        super().__init__()
        self.filter_length, self.hop_length, self.win_length = filter_length, hop_length, win_length
        basis = inverse_basis64(filter_length, hop_length, win_length).astype(np.float32)
        self.register_buffer("inverse_basis", torch.from_numpy(basis)[:, None, :].contiguous())
        self._packed = _Cached()

    def _image(self):
        ib = self.inverse_basis
        def build():
            _check_geometry(self)
            if ib.dtype != torch.float32 or not ib.is_contiguous() or ib.numel() != 1026 * 1024:
                raise ValueError("inverse_basis must be a contiguous fp32 [1026, 1, 1024] buffer")
            packed = torch.empty(call.gt_gl_pack_bytes() // 4, dtype=torch.float32, device=ib.device)
            call.gt_gl_pack(ib, self.filter_length, packed, _lib.current_stream(ib.device))
            return packed
        return self._packed.get((ib,), build)

    def workspace(self, B, F_max, device):
        return torch.empty(call.gt_gl_spec_bytes(B, F_max) // 4, dtype=torch.float32, device=device)

    def polar(self, magnitude, phase, n_frames, spec):
        """kernel call: spec = (mag cos(phase), mag sin(phase)) in the kernels' order"""
        B, _, F = magnitude.shape
        call.gt_gl_polar(magnitude, phase, n_frames, B, F, self.filter_length, self.hop_length, self.win_length, spec,
                         _lib.current_stream(magnitude.device))

    def synthesize(self, spec, n_frames, B, F_max, out=None):
        """kernel call: the spectrum workspace -> wav [B, 256 (F_max - 1)], row b zero behind its 256 (F_b - 1) samples"""
        if out is None:
            out = torch.empty(B, self.hop_length * (F_max - 1), dtype=torch.float32, device=spec.device)
        call.gt_istft(spec, n_frames, B, F_max, self._image(), self.filter_length, self.hop_length, self.win_length, out, out.stride(0),
                      _lib.current_stream(spec.device))
        return out

    def inverse(self, magnitude, phase, frames=None):
        """inverse(magnitude, phase): the reference's call, [B, 513, F] each -> wav [B, 256 (F - 1)].
        inverse(magnitude, phase, frames): the ragged form, utterance b inverted from its first frames[b] frames alone."""
        magnitude, phase = _spectrogram_arg(magnitude, "magnitude"), _spectrogram_arg(phase, "phase")
        if phase.shape != magnitude.shape or phase.device != magnitude.device:
            raise ValueError("magnitude and phase differ in shape or device")
        B, _, F = magnitude.shape
        if F < 2:
            raise ValueError(f"{F} frames: no sample")
        n_frames = torch.full((B,), F, dtype=torch.int32, device=magnitude.device) if frames is None else \
            frames.to(magnitude.device, non_blocking=True).to(torch.int32).contiguous()
        spec = self.workspace(B, F, magnitude.device)
        self.polar(magnitude, phase, n_frames, spec)
        return self.synthesize(spec, n_frames, B, F)

    forward = inverse


def _plain_stft_image(fb):
    """gt_mel_pack's image of a plain STFT's forward basis: it has no mel basis, the image's mel part is zeros"""
    if fb.dtype != torch.float32 or not fb.is_contiguous():
        raise ValueError("forward_basis must be a contiguous fp32 buffer")
    packed = torch.empty(call.gt_mel_pack_bytes() // 4, dtype=torch.float32, device=fb.device)
    call.gt_mel_pack(fb, torch.zeros(1, 513, dtype=torch.float32, device=fb.device), 1024, 1, packed, _lib.current_stream(fb.device))
    return packed


class GriffinLim(nn.Module):
    """The reference's griffin_lim (audio_processing.py:59-75) on the device: gt_gl_polar, gt_istft, then per iteration gt_gl_project
    (analysis, Y = M X / |X|) and gt_istft — 2 + 2 n_iters launches, no host synchronisation.  `stft` is an audio.STFT or a
    TacotronSTFT (the analysis reads its forward basis image); the inverse basis lives in `.istft`, an InverseSTFT."""

    def __init__(self, stft):
        super().__init__()
        self.stft = stft
        self.stft_fn = stft.stft_fn if isinstance(stft, TacotronSTFT) else stft
        _check_geometry(self.stft_fn)
        self.istft = InverseSTFT(self.stft_fn.filter_length, self.stft_fn.hop_length, self.stft_fn.win_length)
        self._fwd_packed, self._mel_pinv = _Cached(), _Cached()

    def _forward_image(self):
        if isinstance(self.stft, TacotronSTFT):
            return self.stft._image()
        fb = self.stft_fn.forward_basis
        return self._fwd_packed.get((fb,), lambda: _plain_stft_image(fb))

    def project(self, wav, magnitudes, n_frames, spec):
        """kernel call, the analysis half: spec = magnitudes * X / |X|, X the STFT of wav's rows (each reflected about its own ends)"""
        B, _, F = magnitudes.shape
        call.gt_gl_project(wav, wav.stride(0), magnitudes, n_frames, B, F, self._forward_image(), 1024, 256, 1024, spec,
                           _lib.current_stream(wav.device))

    def forward(self, magnitudes, frames=None, frames_host=None, n_iters=30, angles=None, seed=0):
        """magnitudes [B, 513, F] -> wav [B, 256 (F - 1)]; with `frames` (counts per utterance; `frames_host` spares the host a look
        at a device tensor) the ragged form -> (wav, wav_lengths = 256 (frames - 1)), zero behind each utterance.  `angles`
        [B, 513, F] are the initial phases; absent, they are uniform in [-pi, pi) from a device torch.Generator seeded with `seed`
        (one PyTorch op — a caller who captures the loop in a graph passes `angles`)."""
        magnitudes = _spectrogram_arg(magnitudes, "magnitudes")
        B, _, F = magnitudes.shape
        dev = magnitudes.device
        n_frames = _frames_arg(frames, frames_host, B, F, dev)
        if angles is None:
            gen = torch.Generator(device=dev)
            gen.manual_seed(int(seed))
            angles = torch.empty_like(magnitudes).uniform_(-np.pi, np.pi, generator=gen)
        else:
            angles = _spectrogram_arg(angles, "angles")
            if angles.shape != magnitudes.shape or angles.device != dev:
                raise ValueError("angles and magnitudes differ in shape or device")
        inv = self.istft
        spec = inv.workspace(B, F, dev)
        inv.polar(magnitudes, angles, n_frames, spec)
        wav = inv.synthesize(spec, n_frames, B, F)
        for _ in range(n_iters):
            self.project(wav, magnitudes, n_frames, spec)
            inv.synthesize(spec, n_frames, B, F, out=wav)
        if frames is None:
            return wav
        return wav, (n_frames.clamp(min=1) - 1) * self.stft_fn.hop_length

    def mel_pinv(self):
        """fp32 [513, n_mel]: the float64 pseudo-inverse of the TacotronSTFT's mel_basis, computed on the host once per version of it"""
        if not isinstance(self.stft, TacotronSTFT):
            raise ValueError("from_mel needs a TacotronSTFT (a mel basis)")
        mb = self.stft.mel_basis
        return self._mel_pinv.get((mb,), lambda: torch.from_numpy(
            np.linalg.pinv(mb.detach().cpu().numpy().astype(np.float64)).astype(np.float32)).to(mb.device))

    def from_mel(self, mel, mel_lengths=None, mel_lengths_host=None, n_iters=30, angles=None, seed=0, phases="torch"):
        """log-mel [B, n_mel, F] (TacotronSTFT.mel_spectrogram's output) -> wav, or (wav, wav_lengths) with mel_lengths.  The
        reference has no mel inversion: magnitudes = clamp(pinv(mel_basis) exp(mel), min=0) (the least-squares spectrum; the bank's
        null space is lost), then the loop above.
        phases="torch" (default): the inversion is PyTorch plumbing on [513 x n_mel] and the initial phases are `angles`, or a device
        torch.Generator's draw from `seed` (it depends on the batch shape and cannot be captured with a per-call seed).
        phases="counter" (DESIGN.md 4.21): ONE gt_gl_from_mel launch writes the magnitudes and the initial spectrum, its phases from the
        counter generator keyed by (seed, utterance, frame, bin) — 1 + 1 + 2 n_iters launches, no ATen op on the data, no phase tensor,
        an utterance's samples independent of the batch it is in.  `angles` with it is a ValueError."""
        if phases not in ("torch", "counter"):
            raise ValueError(f'phases is "torch" or "counter", got {phases!r}')
        if not mel.is_cuda:
            raise CpuWaveError("glow_tts_amd.audio runs on the MI355X only (got a CPU tensor); there is no CPU fallback")
        if phases == "counter":
            if angles is not None:
                raise ValueError('phases="counter" draws the initial phases in the kernel: angles= cannot be given with it')
            pinv = self.mel_pinv()
            if mel.dim() != 3 or mel.shape[1] != pinv.shape[1]:
                raise ValueError(f"mel is [B, {pinv.shape[1]}, F], got {tuple(mel.shape)}")
            if mel.dtype != torch.float32 or mel.stride(2) != 1:
                mel = mel.float().contiguous()
            B, _, F = mel.shape
            n_frames = _frames_arg(mel_lengths, mel_lengths_host, B, F, mel.device)
            wav = self.run_from_mel(mel, n_frames, self.mel_workspace(B, F, mel.device), n_iters, seed=seed)
            if mel_lengths is None:
                return wav
            return wav, (n_frames.clamp(min=1) - 1) * self.stft_fn.hop_length
        magnitudes = torch.clamp(torch.matmul(self.mel_pinv(), torch.exp(mel.float())), min=0.0)
        return self.forward(magnitudes, mel_lengths, mel_lengths_host, n_iters, angles, seed)

    def mel_workspace(self, B, F_max, device):
        """the buffers of one run_from_mel at capacity (B utterances of up to F_max >= 2 frames): dict(mag [B, 513, F_max], spec (the
        spectrum workspace), wav [B, 256 (F_max - 1)]) — 4 * B * (513 F_max + 1025 Fp + 256 (F_max - 1)) bytes, Fp = F_max rounded up
        to 64"""
        if F_max < 2:
            raise ValueError(f"{F_max} frames: no sample")
        return dict(mag=torch.empty(B, 513, F_max, dtype=torch.float32, device=device), spec=self.istft.workspace(B, F_max, device),
                    wav=torch.empty(B, self.stft_fn.hop_length * (F_max - 1), dtype=torch.float32, device=device))

    def run_from_mel(self, mel, n_frames, bufs, n_iters=30, seed=0, seed_dev=None):
        """kernel calls, the capacity-sized form for graph callers: fp32 log-mel [B, n_mel, >= F_max] (any batch / channel pitch, frames
        contiguous), device int32 [B] frame counts and mel_workspace's buffers (F_max is theirs) -> bufs["wav"], row b zero behind its
        256 (F_b - 1) samples.  gt_gl_from_mel, gt_istft, then n_iters x (gt_gl_project, gt_istft): nothing is allocated once the
        packed images and mel_pinv() exist (any earlier call), n_frames is never looked at on the host — an utterance of fewer than
        4 frames gets what the kernels define (clamped reflection; F_b < 2: no sample) — and every grid is sized by F_max, whatever the
        utterances' lengths are.  The seed of the phases is `seed`, or (seed_dev: a device uint32 / int32 word) read on the device."""
        mag, spec, wav = bufs["mag"], bufs["spec"], bufs["wav"]
        B, _, F_max = mag.shape
        pinv = self.mel_pinv()
        if not mel.is_cuda or mel.dtype != torch.float32 or mel.dim() != 3 or mel.stride(2) != 1:
            raise ValueError("run_from_mel takes a device fp32 log-mel [B, n_mel, F] with contiguous frames")
        if mel.shape[0] != B or mel.shape[1] != pinv.shape[1] or mel.shape[2] < F_max:
            raise ValueError(f"mel {tuple(mel.shape)} does not fit buffers for [{B}, {pinv.shape[1]}, {F_max}]")
        if n_frames.dtype != torch.int32 or n_frames.numel() != B or not n_frames.is_cuda or not n_frames.is_contiguous():
            raise ValueError("n_frames must be a contiguous int32 [B] on the device")
        inv = self.istft
        call.gt_gl_from_mel(mel, mel.stride(0) if B > 1 else max(mel.stride(0), F_max), mel.stride(1), n_frames, B, F_max, pinv.shape[1],
                            pinv, int(seed) & 0xFFFFFFFF, seed_dev, mag, spec, _lib.current_stream(mel.device))
        inv.synthesize(spec, n_frames, B, F_max, out=wav)
        for _ in range(n_iters):
            self.project(wav, mag, n_frames, spec)
            inv.synthesize(spec, n_frames, B, F_max, out=wav)
        return wav


def griffin_lim(magnitudes, stft_fn, n_iters=30, **kw):
    """the reference's signature; stft_fn is an audio.STFT / TacotronSTFT (a GriffinLim is built for the call) or a GriffinLim"""
    gl = stft_fn if isinstance(stft_fn, GriffinLim) else GriffinLim(stft_fn).to(magnitudes.device)
    return gl(magnitudes, n_iters=n_iters, **kw)


# ---- the neural vocoders' contract: what HiFiGAN, BigVGAN and Vocos share, and all the synthesiser knows of them -------
def _pad16(c):
    return (c + 15) // 16 * 16


def _padded(t, shape):
    """t in the leading corner of zeros of `shape`"""
    if tuple(t.shape) == tuple(shape):
        return t
    out = t.new_zeros(shape)
    out[tuple(slice(0, n) for n in t.shape)] = t
    return out


class _MelVocoder(nn.Module):
    """A generator from log-mel to waveform that vocodes every utterance of a ragged batch on its own, in eager mode (`forward`) and in
    its capacity-sized form for graph callers (`buffer_spec` / `workspace` / `run`, synthesis.Synthesizer).  A subclass sets
      hop_length, min_frames   F frames give wav_len(F) = hop_length (F - (min_frames - 1)) samples, none below min_frames
      mel_channels             what run takes per frame; forward takes mel_channels - mel_padding and zero-pads
      launches                 C-ABI calls per run
      seeded                   True for a generator that draws a latent (WaveGlow): forward takes `seed`, run `seed_dev` / `seed`, and
                               _walk receives both
    and supplies buffer_spec(B, F_max) (through _check_capacity), held() and _walk(mel, n_frames, bufs, B, F): the kernel calls."""

    min_frames, mel_padding = 1, 0
    seeded = False

    def wav_len(self, frames):
        """samples of an utterance (or a buffer row) of `frames` frames"""
        return self.hop_length * max(frames - (self.min_frames - 1), 0)

    def check_graph_input(self):
        """ValueError where run cannot take the mel a synthesis graph writes (the model's own channel count)"""

    def _check_capacity(self, B, F_max, elements, bound):
        """the one capacity check: `elements`, the largest element index a run forms at (B, F_max), stays below 2^31"""
        if B < 1 or F_max < self.min_frames or elements >= 2 ** 31:
            raise ValueError(f"workspace for {B} x {F_max} frames: {bound}")

    def workspace_bytes(self, B, F_max):
        """bytes of workspace(B, F_max): buffer_spec's buffers and the samples"""
        return sum(n * dt.itemsize for _, dt, n in self.buffer_spec(B, F_max)) + 4 * B * self.wav_len(F_max)

    def workspace(self, B, F_max, device):
        """the buffers of one run at capacity (B utterances of up to F_max frames): buffer_spec's by name and wav fp32
        [B, wav_len(F_max)]"""
        bufs = {name: torch.empty(n, dtype=dt, device=device) for name, dt, n in self.buffer_spec(B, F_max)}
        bufs["wav"] = torch.empty(B, self.wav_len(F_max), dtype=torch.float32, device=device)
        return bufs

    def run(self, mel, n_frames, bufs, seed_dev=None, seed=0):
        """kernel calls, the capacity-sized form for graph callers: fp32 log-mel [B, mel_channels, >= F_max] (any batch / channel pitch,
        frames contiguous), device int32 [B] frame counts and workspace's buffers (B and F_max are theirs) -> bufs["wav"]
        [B, wav_len(F_max)], row b zero behind its wav_len(F_b) samples.  `launches` C-ABI calls; nothing is allocated once the images
        exist, n_frames is never looked at on the host, every grid is sized by F_max.  A seeded vocoder draws its latent from `seed`,
        or (seed_dev: a device uint32 / int32 word) from the word read on the device; the others take neither."""
        if not self.seeded and (seed_dev is not None or seed):
            raise ValueError(f"{type(self).__name__} draws no latent: it takes no seed")
        wav = bufs["wav"]
        B, F, C = wav.shape[0], wav.shape[1] // self.hop_length + self.min_frames - 1, self.mel_channels
        if not mel.is_cuda:
            raise CpuWaveError("glow_tts_amd.audio runs on the MI355X only (got a CPU tensor); there is no CPU fallback")
        if mel.dtype != torch.float32 or mel.dim() != 3 or mel.stride(2) != 1:
            raise ValueError("run takes a device fp32 log-mel [B, n_mel, F] with contiguous frames")
        if mel.shape[0] != B or mel.shape[1] != C or mel.shape[2] < F:
            raise ValueError(f"mel {tuple(mel.shape)} does not fit buffers for [{B}, {C}, {F}]")
        if n_frames.dtype != torch.int32 or n_frames.numel() != B or not n_frames.is_cuda or not n_frames.is_contiguous():
            raise ValueError("n_frames must be a contiguous int32 [B] on the device")
        if next(self.parameters()).device != mel.device:
            raise ValueError("the vocoder's parameters are not on the mel's device")
        if self.seeded:
            return self._walk(mel, n_frames, bufs, B, F, seed_dev=seed_dev, seed=seed)
        return self._walk(mel, n_frames, bufs, B, F)

    def forward(self, mel, mel_lengths=None, mel_lengths_host=None, seed=0):
        """log-mel [B, mel_channels - mel_padding, F] -> wav [B, wav_len(F)]; with mel_lengths (frames per utterance) the ragged form
        -> (wav, wav_lengths = wav_len(mel_lengths)), zero behind each utterance.  mel_lengths_host spares the host a look at a device
        tensor.  With mel_padding (Vocos's 100-band models) the mel is copied into a zero-padded one first.  `seed`: a seeded vocoder's."""
        C = self.mel_channels - self.mel_padding
        if not mel.is_cuda:
            raise CpuWaveError("glow_tts_amd.audio runs on the MI355X only (got a CPU tensor); there is no CPU fallback")
        if mel.dim() != 3 or mel.shape[1] != C:
            raise ValueError(f"mel is [B, {C}, F], got {tuple(mel.shape)}")
        if mel.dtype != torch.float32 or mel.stride(2) != 1:
            mel = mel.float().contiguous()
        B, _, F = mel.shape
        if mel_lengths is None:
            n_frames = torch.full((B,), F, dtype=torch.int32, device=mel.device)
        else:
            if mel_lengths_host is None and not mel_lengths.is_cuda:
                mel_lengths_host = mel_lengths.tolist()
            if mel_lengths.numel() != B or (mel_lengths_host is not None and (len(mel_lengths_host) != B or max(mel_lengths_host) > F)):
                raise ValueError(f"frame counts do not fit a [{B}, {C}, {F}] mel")
            n_frames = mel_lengths.to(mel.device, non_blocking=True).to(torch.int32).contiguous()
        if F < self.min_frames or B == 0:
            wav = mel.new_zeros(B, self.wav_len(F))
        else:
            if self.mel_padding:
                padded = mel.new_zeros(B, self.mel_channels, F)
                padded[:, :C] = mel
                mel = padded
            wav = _MelVocoder.run(self, mel, n_frames, self.workspace(B, F, mel.device), seed=seed)   # not a subclass's refusal of a padded model
        if mel_lengths is None:
            return wav
        lost = self.min_frames - 1
        n = n_frames.clamp(min=lost, max=max(F, lost))
        return wav, (n - lost if lost else n) * self.hop_length


# ---- neural vocoder: the HiFi-GAN generator on csrc/hifigan.hip ---------------------------------------------------
LRELU_SLOPE = 0.1                    # the generator's; conv_post's input takes F.leaky_relu's default 0.01 (a quirk of the original)


def transposed_as_conv(w, u):
    """ConvTranspose1d weight [Cin, Cout, 2u] (stride u even, padding u / 2) -> the 3-tap convolution weight [u * Cout, Cin, 3] with
    W3[r * Cout + c, ci, j] = w[ci, c, r + u / 2 + u (1 - j)] where that index lies in [0, 2u) and 0 elsewhere: output u q + r of the
    transposed convolution reads inputs q - 1, q, q + 1 only, and [L, u * Cout] channels-last IS [u L, Cout]"""
    Cin, Cout, k = w.shape
    if k != 2 * u or u % 2:
        raise ValueError(f"transposed convolutions are k = 2u with u even, got k = {k}, u = {u}")
    W3 = w.new_zeros(u, Cout, Cin, 3)
    for j in range(3):
        for r in range(u):
            idx = r + u // 2 + u * (1 - j)
            if 0 <= idx < k:
                W3[r, :, :, j] = w[:, :, idx].t()
    return W3.reshape(u * Cout, Cin, 3)


def voc_pack(w):
    """conv weight [N, Cin, taps] (any float dtype) -> gt_voc_conv's bf16 image [taps][Np / 32][Kp / 16][64 lanes][8], lane 32 h + r and
    element e holding W[j][32 nt + r][16 ks + 8 h + e] rounded to nearest even, zeros in the padding (include/glowtts_hip.h)"""
    N, Cin, taps = w.shape
    kc = call.gt_voc_k_chunk(Cin)
    if not kc:
        raise ValueError(f"{Cin} input channels: a multiple of 16 is needed")
    Np, Kp = (N + 31) // 32 * 32, (Cin + kc - 1) // kc * kc
    full = torch.zeros(taps, Np, Kp, dtype=torch.bfloat16, device=w.device)
    full[:, :N, :Cin] = w.detach().permute(2, 0, 1).to(torch.bfloat16)
    return full.view(taps, Np // 32, 32, Kp // 16, 2, 8).permute(0, 1, 3, 4, 2, 5).contiguous().view(-1)


def fold_weight_norm(g, v):
    """weight_norm's w = g v / ||v|| (norm over every dim but 0) in float64, rounded to fp32 once"""
    v64, g64 = v.detach().double().cpu(), g.detach().double().cpu()
    norm = v64.reshape(v64.shape[0], -1).norm(dim=1).reshape(-1, *([1] * (v64.dim() - 1)))
    return (g64 * v64 / norm).float()


class _ResBlock(nn.Module):
    """parameter holder under the original generator's names: convs1 / convs2 (resblock "1") or convs ("2")"""

    def __init__(self, kind, C, k, dilations):
        super().__init__()
        mk = lambda d: nn.Conv1d(C, C, k, dilation=d, padding=d * (k - 1) // 2)  # noqa: E731
        if kind == "1":
            self.convs1 = nn.ModuleList(mk(d) for d in dilations)
            self.convs2 = nn.ModuleList(mk(1) for _ in dilations)
        else:
            self.convs = nn.ModuleList(mk(d) for d in dilations)


class HiFiGAN(_MelVocoder):
    """The published HiFi-GAN `Generator` (eval mode, weight norm folded) from log-mel to waveform, every layer by ONE HIP kernel
    (csrc/hifigan.hip: gt_voc_conv), applied to every utterance of a ragged batch ON ITS OWN: utterance b is
    Generator(mel[b:b+1, :, :F_b]), every convolution zero-padded at that utterance's own ends, so its samples do not depend on the
    batch it is in.  F_b frames give U F_b samples, U the product of the upsample rates (256 for V1 — not Griffin-Lim's 256 (F_b - 1)).

      conv_pre (k 7) -> per stage: lrelu 0.1, transposed conv (k = 2u, stride u even, padding u / 2: run as a 3-tap convolution to
      u * Cout channels read back as u times the positions), the mean of the resblocks -> lrelu 0.01, conv_post (k 7, 1 channel), tanh.

    Parameters are fp32 under the original names (conv_pre, ups.{i}, resblocks.{i K + j}.convs1.{m} / .convs2.{m} or .convs.{m},
    conv_post; transposed weights stay [Cin, Cout, k]); `load_generator_state` takes a checkpoint with or without weight norm.
    Operands are bf16 (the packed images, and the activations after the leaky ReLU), accumulation fp32; the residual stream and the
    resblock sum stay fp32, only the tensor between a resblock's two convolutions is bf16.  `launches` gt_voc_conv calls per run: 78
    for V1.  Any other (k, u), channels that are no multiple of 16, an even or > 11 resblock kernel: ValueError."""

    CHANNEL_MULTIPLE = 16                # of every stage's channel count (BigVGAN pads its images instead: 1)
    UP_SLOPE = LRELU_SLOPE               # in front of a transposed convolution
    use_tanh_at_final = True

    def __init__(self, resblock="1", upsample_rates=(8, 8, 2, 2), upsample_kernel_sizes=(16, 16, 4, 4), upsample_initial_channel=512,
                 resblock_kernel_sizes=(3, 7, 11), resblock_dilation_sizes=((1, 3, 5),) * 3, n_mel_channels=80):
        super().__init__()
        resblock = str(resblock)
        rates, kernels = tuple(int(u) for u in upsample_rates), tuple(int(k) for k in upsample_kernel_sizes)
        rk, rd = tuple(int(k) for k in resblock_kernel_sizes), tuple(tuple(int(d) for d in ds) for ds in resblock_dilation_sizes)
        C0 = int(upsample_initial_channel)
        if resblock not in ("1", "2"):
            raise ValueError(f'resblock is "1" or "2", got {resblock!r}')
        if not rates or len(rates) != len(kernels) or not rk or len(rk) != len(rd) or any(not ds for ds in rd):
            raise ValueError("upsample_rates / upsample_kernel_sizes and resblock_kernel_sizes / resblock_dilation_sizes must pair up")
        for u, k in zip(rates, kernels):
            if k != 2 * u or u % 2 or u < 2:
                raise ValueError(f"transposed convolutions are k = 2u with u even, got k = {k}, u = {u}")
        for k in rk:
            if k % 2 == 0 or k < 1 or k > 11:
                raise ValueError(f"resblock kernels are odd and at most 11, got {k}")
        if any(d < 1 for ds in rd for d in ds):
            raise ValueError("dilations are >= 1")
        chans = [C0 >> i for i in range(len(rates) + 1)]
        if n_mel_channels % 16 or any(c % self.CHANNEL_MULTIPLE or c < self.CHANNEL_MULTIPLE for c in chans) or C0 % (1 << len(rates)):
            raise ValueError(f"channel counts must be multiples of 16, got mel {n_mel_channels} and stages {chans}")
        self.resblock, self.upsample_rates, self.upsample_kernel_sizes = resblock, rates, kernels
        self.resblock_kernel_sizes, self.resblock_dilation_sizes = rk, rd
        self.n_mel_channels, self.channels = int(n_mel_channels), chans
        self.mel_channels, self.padded_channels = self.n_mel_channels, [_pad16(c) for c in chans]   # what the kernels run at
        self.hop_length = int(np.prod(rates))                                      # U: samples per frame
        self.conv_pre = nn.Conv1d(self.n_mel_channels, C0, 7, padding=3)
        self.ups = nn.ModuleList(nn.ConvTranspose1d(chans[i], chans[i + 1], k, u, padding=(k - u) // 2)
                                 for i, (u, k) in enumerate(zip(rates, kernels)))
        self.resblocks = nn.ModuleList(_ResBlock(resblock, chans[i + 1], k, ds) for i in range(len(rates)) for k, ds in zip(rk, rd))
        self.conv_post = nn.Conv1d(chans[-1], 1, 7, padding=3)
        per_block = sum((2 if resblock == "1" else 1) * len(ds) for ds in rd)
        self.launches = 2 + len(rates) * (1 + per_block)
        self._images = _Cached()
        for p in self.parameters():
            p.requires_grad_(False)

    @classmethod
    def from_config(cls, cfg):
        """from the original config.json's keys (num_mels optional: 80)"""
        return cls(resblock=cfg["resblock"], upsample_rates=cfg["upsample_rates"], upsample_kernel_sizes=cfg["upsample_kernel_sizes"],
                   upsample_initial_channel=cfg["upsample_initial_channel"], resblock_kernel_sizes=cfg["resblock_kernel_sizes"],
                   resblock_dilation_sizes=cfg["resblock_dilation_sizes"], n_mel_channels=cfg.get("num_mels", 80))

    def load_generator_state(self, sd):
        """a checkpoint's sd["generator"] or the dict itself, with weight norm (weight_g / weight_v, folded g v / ||v|| over dim 0 in
        float64 and rounded once) or after remove_weight_norm; strict"""
        sd = sd.get("generator", sd) if isinstance(sd, dict) else sd
        out = {}
        for k, t in sd.items():
            if k.endswith(".weight_g"):
                out[k[:-2]] = fold_weight_norm(t, sd[k[:-1] + "v"])
            elif not k.endswith(".weight_v"):
                out[k] = t.detach().float()
        return self.load_state_dict(out, strict=True)

    # ---- the packed images: one per launch, in launch order ---------------------------------------------------------------------------
    def _convs(self):
        """[(weight as a conv [N, Cin, taps] builder, bias builder)] in launch order"""
        K = len(self.resblock_kernel_sizes)
        seq = [self.conv_pre]
        for i in range(len(self.ups)):
            seq += [m for m in self.ups[i].modules() if isinstance(m, nn.ConvTranspose1d)]         # ups[i], or BigVGAN's ups[i][0]
            for j in range(K):
                rb = self.resblocks[i * K + j]
                if self.resblock == "1":
                    for c1, c2 in zip(rb.convs1, rb.convs2):
                        seq += [c1, c2]
                else:
                    seq += list(rb.convs)
        return seq + [self.conv_post]

    def _conv_images(self):
        """[(bf16 image, fp32 bias)] per convolution at the padded widths: zero weight rows / columns and bias in the padding (none for
        a HiFi-GAN), one zero for a convolution without bias"""
        imgs = []
        for m in self._convs():
            w = m.weight.detach().float()
            b = m.bias.detach().float() if m.bias is not None else w.new_zeros(1)
            if isinstance(m, nn.ConvTranspose1d):
                u = m.stride[0]
                w = _padded(w, (_pad16(w.shape[0]), _pad16(w.shape[1]), w.shape[2]))
                imgs.append((voc_pack(transposed_as_conv(w, u)), _padded(b, (w.shape[1],)).repeat(u).contiguous()))
            else:
                N = w.shape[0] if m is self.conv_post else _pad16(w.shape[0])
                imgs.append((voc_pack(_padded(w, (N, _pad16(w.shape[1]), w.shape[2]))), _padded(b, (N,)).contiguous()))
        return imgs

    def images(self):
        """[(bf16 image, fp32 bias)] per launch, rebuilt when any parameter's (data_ptr, _version) changes"""
        return self._images.get(list(self.parameters()), self._conv_images)

    # ---- capacity-sized form ------------------------------------------------------------------------------------------------------------
    def _width(self):
        U, w = 1, self.padded_channels[0]
        for i, u in enumerate(self.upsample_rates):
            U *= u
            w = max(w, U * self.padded_channels[i + 1])
        return w

    @property
    def t_dtype(self):
        """the fourth buffer: bf16 between a resblock "1"'s two convolutions; for resblock "2" a second fp32 residual stream"""
        return torch.bfloat16 if self.resblock == "1" else torch.float32

    def buffer_spec(self, B, F_max):
        """[(name, dtype, elements)] of the buffers a run takes next to wav [B, U F_max]: three fp32 streams u, r, s (a stage's input,
        a resblock's residual stream, the resblock sum / the stage's output) and one bf16 t (between a resblock's two convolutions) of
        E = B F_max W elements each, W = max(C_0, max_i U_i C_i) (U_i the product of the first i rates, C_i the channels behind them:
        8192 for V1), reused across the stages: 14 E + 4 B U F_max bytes — 2.94 GB + 26 MB for V1 at 32 x 800 frames.  Resblock "2" has
        no tensor between two convolutions but reads its own residual stream through a halo, which cannot be updated in place: its t
        is a second fp32 stream (16 E).  B F_max W must stay below 2^31."""
        E = B * F_max * self._width()
        self._check_capacity(B, F_max, E, f"B F_max W = {E} must lie in [1, 2^31)")
        return [("u", torch.float32, E), ("r", torch.float32, E), ("s", torch.float32, E), ("t", self.t_dtype, E)]

    def held(self):
        """what a captured graph of run() reads besides the buffers: its holder keeps it alive (the vocoder drops it when it repacks)"""
        return self.images()

    def _launch(self, dev, n_frames, B, L, mul, X, img, Y, Cin, N, taps, dil, slope, x_sb, y_sb, ldy, x_sc=0, x_mel=0, x_bf16=0,
                y_bf16=0, res=None, acc=None, scale=1.0, tanh=0):
        a = _lib.fill_args(_lib.VocConvArgs, X=X, x_stride_b=x_sb, x_stride_c=x_sc, W=img[0], bias=img[1], res=res, acc=acc, Y=Y,
                           y_stride_b=y_sb, ldy=ldy, len_mul=mul, n_frames=n_frames, B=B, L_cap=L, Cin=Cin, N=N, taps=taps, dil=dil,
                           x_bf16=x_bf16, x_mel=x_mel, y_bf16=y_bf16, tanh_out=tanh, slope=slope, scale=scale)
        call.gt_voc_conv(a, _lib.current_stream(dev))

    def _activation(self, dev, n_frames, B, bufs):
        """act(L, mul, X, C, slope) -> (operand, slope): what the convolution behind an activation of the stream X reads.  Here the
        stream itself, the leaky ReLU being the kernel's prologue"""
        return lambda L, mul, X, C, slope: (X, slope)

    def _walk(self, mel, n_frames, bufs, B, F):
        """run's launches (`launches` of them): conv_pre, per stage the transposed convolution and the resblocks, conv_post.  A bf16
        operand or destination says so by its dtype"""
        dev, imgs, wav = mel.device, iter(self.images()), bufs["wav"]
        u_, r_, s_, t_ = bufs["u"], bufs["r"], bufs["s"], bufs["t"]
        K, ch, n_mel = len(self.resblock_kernel_sizes), self.padded_channels, self.n_mel_channels
        act = self._activation(dev, n_frames, B, bufs)
        bf16 = lambda t: int(t.dtype == torch.bfloat16)  # noqa: E731
        go = lambda L, mul, X, Y, *a, **k: self._launch(dev, n_frames, B, L, mul, X, next(imgs), Y, *a, x_bf16=bf16(X), **k)  # noqa: E731
        L, mul, C = F, 1, ch[0]
        go(L, mul, mel, s_, n_mel, C, 7, 1, 1.0, mel.stride(0) if B > 1 else max(mel.stride(0), F), L * C, C,
           x_sc=mel.stride(1) if n_mel > 1 else max(mel.stride(1), F), x_mel=1)
        for i, u in enumerate(self.upsample_rates):
            Cn = ch[i + 1]
            go(L, mul, s_, u_, C, u * Cn, 3, 1, self.UP_SLOPE, L * C, L * u * Cn, u * Cn)
            L, mul, C = L * u, mul * u, Cn
            sb = L * C
            for j, (k, ds) in enumerate(zip(self.resblock_kernel_sizes, self.resblock_dilation_sizes)):
                src = u_
                for m, d in enumerate(ds):
                    last = m == len(ds) - 1
                    tail = dict(res=src, acc=s_ if j else None, scale=1.0 / K if j == K - 1 else 1.0) if last else dict(res=src)
                    X, slope = act(L, mul, src, C, LRELU_SLOPE)
                    if self.resblock == "1":
                        go(L, mul, X, t_, C, C, k, d, slope, sb, sb, C, y_bf16=bf16(t_))
                        (X, slope), d = act(L, mul, t_, C, LRELU_SLOPE), 1
                    # Y may alias res, but not a stream that X is: a convolution that reads its own residual stream through the halo
                    # ("2" without an activation kernel in between) takes r and t in turns
                    dst = s_ if last else (t_ if X is src and m % 2 else r_)
                    go(L, mul, X, dst, C, C, k, d, slope, sb, sb, C, **tail)
                    src = dst
        X, slope = act(L, mul, s_, C, 0.01)
        go(L, mul, X, wav, C, 1, 7, 1, slope, L * C, wav.stride(0), 1, tanh=int(self.use_tanh_at_final))
        if not self.use_tanh_at_final:
            wav.clamp_(-1.0, 1.0)                                          # capturable, not counted in `launches`
        return wav


# ---- BigVGAN: the HiFi-GAN generator with anti-aliased snake activations, csrc/voc_snake.hip in front of gt_voc_conv ----
def kaiser_sinc_filter64(cutoff=0.25, half_width=0.3, kernel_size=12):
    """BigVGAN's kaiser_sinc_filter1d in float64 [kernel_size]: the one filter of both resamplers of Activation1d"""
    A = 2.285 * (kernel_size // 2 - 1) * np.pi * 4 * half_width + 7.95
    beta = 0.1102 * (A - 8.7) if A > 50 else (0.5842 * (A - 21) ** 0.4 + 0.07886 * (A - 21) if A >= 21 else 0.0)
    time = np.arange(-(kernel_size // 2), kernel_size // 2) + 0.5 if kernel_size % 2 == 0 else np.arange(kernel_size) - kernel_size // 2
    f = 2 * cutoff * np.kaiser(kernel_size, beta) * np.sinc(2 * cutoff * time)
    return f / f.sum()


class _Snake(nn.Module):
    """parameter holder: Snake (alpha) or SnakeBeta (alpha, beta), per channel"""

    def __init__(self, C, kind, logscale):
        super().__init__()
        init = torch.zeros if logscale else torch.ones
        self.alpha = nn.Parameter(init(C))
        if kind == "snakebeta":
            self.beta = nn.Parameter(init(C))


class _Filter(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("filter", torch.from_numpy(kaiser_sinc_filter64()).float().view(1, 1, 12))


class _DownSample(nn.Module):
    def __init__(self):
        super().__init__()
        self.lowpass = _Filter()


class _Activation1d(nn.Module):
    """holder under the original names: act.alpha (act.beta), upsample.filter, downsample.lowpass.filter"""

    def __init__(self, C, kind, logscale):
        super().__init__()
        self.act, self.upsample, self.downsample = _Snake(C, kind, logscale), _Filter(), _DownSample()


class _AMPBlock(_ResBlock):
    def __init__(self, kind, C, k, dilations, act, logscale):
        super().__init__(kind, C, k, dilations)
        n = (2 if kind == "1" else 1) * len(dilations)
        self.activations = nn.ModuleList(_Activation1d(C, act, logscale) for _ in range(n))


class BigVGAN(HiFiGAN):
    """The published BigVGAN generator (eval mode, weight norm folded) from log-mel to waveform: HiFi-GAN's generator with every leaky
    ReLU replaced by the anti-aliased periodic activation Activation1d (2x up-sampling FIR -> snake -> 2x down-sampling FIR per channel)
    and NO activation in front of the transposed convolutions.  The convolutions are gt_voc_conv's, untouched (slope 1, bf16 input);
    each activation is ONE launch of the stand-alone kernel gt_voc_snake (csrc/voc_snake.hip), which writes the bf16
    operand the next convolution reads.  Every utterance of a ragged batch on its own, as for HiFiGAN.

      conv_pre -> per stage: ups[i][0] (transposed, no activation), the mean of the AMP blocks -> activation_post -> conv_post -> tanh
      (use_tanh_at_final False: clamp to [-1, 1]; use_bias_at_final False: conv_post without bias)
      AMPBlock1: x = convs2[m](acts[2m + 1](convs1[m](acts[2m](x)))) + x;  AMPBlock2: x = convs[m](acts[m](x)) + x

    Parameters and buffers carry the published names (ups.{i}.0, resblocks.{j}.activations.{m}.act.alpha / .act.beta /
    .upsample.filter / .downsample.lowpass.filter, activation_post...), so state_dict() round-trips with the original generator's.
    A stage whose channel count is no multiple of 16 (the 24 channels the 112 M configurations end at) runs at the next multiple, padded
    on the host: zero weight rows / columns, zero bias, alpha' = 1, 1 / beta' = 0 — a padded channel is exactly 0 everywhere.
    `launches` C-ABI calls per run — conv_launches gt_voc_conv and snake_launches gt_voc_snake: 78 convolutions + 73 activations =
    151 for the base shape.  The stage walk is HiFiGAN's: this class supplies what a convolution reads (_activation) and the fifth
    buffer."""

    CHANNEL_MULTIPLE = 1
    UP_SLOPE = 1.0                       # no activation in front of the transposed convolutions

    def __init__(self, resblock="1", upsample_rates=(8, 8, 2, 2), upsample_kernel_sizes=(16, 16, 4, 4), upsample_initial_channel=512,
                 resblock_kernel_sizes=(3, 7, 11), resblock_dilation_sizes=((1, 3, 5),) * 3, n_mel_channels=80, activation="snakebeta",
                 snake_logscale=True, use_tanh_at_final=True, use_bias_at_final=True):
        if activation not in ("snake", "snakebeta"):
            raise ValueError(f'activation is "snake" or "snakebeta", got {activation!r}')
        super().__init__(resblock, upsample_rates, upsample_kernel_sizes, upsample_initial_channel, resblock_kernel_sizes,
                         resblock_dilation_sizes, n_mel_channels)
        self.activation, self.snake_logscale = activation, bool(snake_logscale)
        self.use_tanh_at_final, self.use_bias_at_final = bool(use_tanh_at_final), bool(use_bias_at_final)
        ch, rk, rd = self.channels, self.resblock_kernel_sizes, self.resblock_dilation_sizes
        self.ups =nn.ModuleList(nn.ModuleList([up]) for up in self.ups)
        self.resblocks = nn.ModuleList(_AMPBlock(self.resblock, ch[i + 1], k, ds, activation, self.snake_logscale)
                                       for i in range(len(self.upsample_rates)) for k, ds in zip(rk, rd))
        self.activation_post = _Activation1d(ch[-1], activation, self.snake_logscale)
        self.conv_post = nn.Conv1d(ch[-1], 1, 7, padding=3, bias=self.use_bias_at_final)
        self.conv_launches = self.launches
        self.snake_launches = len(self.upsample_rates) * sum(len(rb.activations) for rb in self.resblocks[:len(rk)]) + 1
        self.launches = self.conv_launches + self.snake_launches
        for p in self.parameters():
            p.requires_grad_(False)

    @classmethod
    def from_config(cls, cfg):
        """from the published config.json's keys (num_mels optional: 80; the activation keys default to the published base model's)"""
        return cls(resblock=cfg["resblock"], upsample_rates=cfg["upsample_rates"], upsample_kernel_sizes=cfg["upsample_kernel_sizes"],
                   upsample_initial_channel=cfg["upsample_initial_channel"], resblock_kernel_sizes=cfg["resblock_kernel_sizes"],
                   resblock_dilation_sizes=cfg["resblock_dilation_sizes"], n_mel_channels=cfg.get("num_mels", 80),
                   activation=cfg.get("activation", "snakebeta"), snake_logscale=cfg.get("snake_logscale", True),
                   use_tanh_at_final=cfg.get("use_tanh_at_final", True), use_bias_at_final=cfg.get("use_bias_at_final", True))

    # ---- images and parameter blocks, in launch order, at the padded widths ----------------------------------------------------------------
    def _activations(self):
        return [act for rb in self.resblocks for act in rb.activations] + [self.activation_post]

    def snake_block64(self, act):
        """gt_voc_snake's parameter block of one Activation1d in float64, at the padded width Cp: [Cp] alpha', [Cp] 1 / (beta' + 1e-9),
        [12] the module's up-sampling filter, [12] its down-sampling filter; padding alpha' = 1, 1 / beta' = 0"""
        al = act.act.alpha.detach().double().cpu()
        be = act.act.beta.detach().double().cpu() if self.activation == "snakebeta" else al
        if self.snake_logscale:
            al, be = al.exp(), be.exp()
        C = al.numel()
        Cp = _pad16(C)
        a, ib = torch.ones(Cp, dtype=torch.float64), torch.zeros(Cp, dtype=torch.float64)
        a[:C], ib[:C] = al, 1.0 / (be + 1e-9)
        return torch.cat([a, ib, act.upsample.filter.detach().double().cpu().reshape(-1),
                          act.downsample.lowpass.filter.detach().double().cpu().reshape(-1)])

    def _packed(self):
        """([(bf16 image, fp32 bias)] per convolution, [fp32 parameter block] per activation), both in launch order, rebuilt when any
        parameter's or buffer's (data_ptr, _version) changes"""
        def build():
            imgs, blocks64 = self._conv_images(), [self.snake_block64(act) for act in self._activations()]
            flat = torch.cat(blocks64).float().to(self.conv_pre.weight.device)                 # float64 on the host, rounded once
            offs = np.cumsum([0] + [b.numel() for b in blocks64])
            return imgs, [flat[offs[i]:offs[i + 1]] for i in range(len(blocks64))]
        return self._images.get(list(self.parameters()) + list(self.buffers()), build)

    def images(self):
        return self._packed()[0]

    def snake_blocks(self):
        return self._packed()[1]

    def held(self):
        return self._packed()

    # ---- capacity-sized form ------------------------------------------------------------------------------------------------------------
    @property
    def t_dtype(self):
        """fp32: the tensor between an AMP block's two convolutions is the second activation's input"""
        return torch.float32

    def buffer_spec(self, B, F_max):
        """HiFiGAN's u, r, s and a t of fp32, and one bf16 stream a (every activation's output: the operand of the convolution behind
        it) of E = B F_max W elements each, W over the padded channel counts (8192 for the base shape): 18 E + 4 B U F_max bytes"""
        spec = super().buffer_spec(B, F_max)
        return spec + [("a", torch.bfloat16, spec[0][2])]

    def _snake(self, dev, n_frames, B, L, mul, X, P, Y, C):
        a = _lib.fill_args(_lib.VocSnakeArgs, X=X, x_stride_b=L * C, P=P, Y=Y, y_stride_b=L * C, len_mul=mul, n_frames=n_frames, B=B,
                           L_cap=L, C=C)
        call.gt_voc_snake(a, _lib.current_stream(dev))

    def _activation(self, dev, n_frames, B, bufs):
        """one gt_voc_snake launch per activation, in launch order: the convolution reads its bf16 output a at slope 1"""
        blocks, a_ = iter(self.snake_blocks()), bufs["a"]

        def act(L, mul, X, C, slope):
            self._snake(dev, n_frames, B, L, mul, X, next(blocks), a_, C)
            return a_, 1.0
        return act


# ---- Vocos: a frame-rate ConvNeXt backbone and an iSTFT head on csrc/vocos.hip, gt_voc_conv and gt_istft -------------
VOCOS_EPS = 1e-6                     # every LayerNorm of the published model
VOCOS_BINS = 513                     # n_fft / 2 + 1 of the one geometry gt_istft implements


class _ConvNeXtBlock(nn.Module):
    """parameter holder under the published names: dwconv, norm, pwconv1, pwconv2, gamma"""

    def __init__(self, dim, intermediate_dim, layer_scale):
        super().__init__()
        self.dwconv = nn.Conv1d(dim, dim, 7, padding=3, groups=dim)
        self.norm = nn.LayerNorm(dim, eps=VOCOS_EPS)
        self.pwconv1 = nn.Linear(dim, intermediate_dim)
        self.pwconv2 = nn.Linear(intermediate_dim, dim)
        self.gamma = nn.Parameter(layer_scale * torch.ones(dim))


class _VocosBackbone(nn.Module):
    def __init__(self, input_channels, dim, intermediate_dim, num_layers):
        super().__init__()
        self.embed = nn.Conv1d(input_channels, dim, 7, padding=3)
        self.norm = nn.LayerNorm(dim, eps=VOCOS_EPS)
        self.convnext = nn.ModuleList(_ConvNeXtBlock(dim, intermediate_dim, 1.0 / num_layers) for _ in range(num_layers))
        self.final_layer_norm = nn.LayerNorm(dim, eps=VOCOS_EPS)


class _VocosHead(nn.Module):
    def __init__(self, dim, n_fft):
        super().__init__()
        self.out = nn.Linear(dim, n_fft + 2)


def fold_layer_scale(gamma, w2, b2):
    """ConvNeXt's layer scale folded into its second Linear: (gamma[:, None] w2, gamma b2) formed in float64 and rounded to fp32 once"""
    g = gamma.detach().double()
    return (g[:, None] * w2.detach().double()).float(), (g * b2.detach().double()).float()


class Vocos(_MelVocoder):
    """The published Vocos generator (Siuzdak 2023: `VocosBackbone` + `ISTFTHead`, padding="center") from log-mel to waveform.  The whole
    network runs at FRAME rate, every utterance of a ragged batch ON ITS OWN: utterance b is Vocos(mel[b:b+1, :, :F_b]), every
    convolution zero-padded at that utterance's own ends; F_b frames give 256 (F_b - 1) samples (none below 2 frames: gt_istft's rule).

      embed (k 7, gt_voc_conv on the channel-major mel) -> LayerNorm (gt_vocos_norm) -> per block: depthwise k 7 + LayerNorm
      (gt_vocos_norm, bf16 out), Linear -> GELU -> Linear, layer scale, residual (gt_vocos_mlp, the hidden activation never in global
      memory) -> LayerNorm (gt_vocos_norm) -> Linear to 513 log-magnitudes + 513 phases (gt_voc_conv, taps 1) -> gt_vocos_polar ->
      gt_istft: `launches` = 6 + 2 num_layers, 22 for the published model.

    Parameters are fp32 under the published names (backbone.embed, backbone.norm, backbone.convnext.{i}.dwconv / .norm / .pwconv1 /
    .pwconv2 / .gamma, backbone.final_layer_norm, head.out); `load_vocos_state` takes a published checkpoint.  Operands of the matrix
    products are bf16 (the packed images; the mel, every block's normalised input, the hidden activation, the head's input),
    accumulation, the residual stream, the LayerNorms and the head's nonlinearity fp32, the inverse STFT exact fp32.
    Refused with ValueError: padding="same", a conditional backbone (adanorm_num_embeddings), n_fft / hop_length other than 1024 / 256,
    a dim other than 128 / 256 / 512, an intermediate_dim that is no multiple of gt_vocos_hidden_chunk() or above 2048."""

    min_frames = 2

    def __init__(self, input_channels=80, dim=512, intermediate_dim=1536, num_layers=8, n_fft=1024, hop_length=256, padding="center",
                 adanorm_num_embeddings=None):
        super().__init__()
        input_channels, dim, intermediate_dim, num_layers = int(input_channels), int(dim), int(intermediate_dim), int(num_layers)
        if padding != "center":
            raise ValueError(f'Vocos: padding is "center" (torch.istft(center=True)), got {padding!r}')
        if adanorm_num_embeddings:
            raise ValueError("Vocos: a conditional backbone (AdaLayerNorm, the EnCodec variant) is not supported")
        if (int(n_fft), int(hop_length)) != (1024, 256):
            raise ValueError(f"Vocos: the inverse STFT takes n_fft = 1024, hop_length = 256, got {n_fft} / {hop_length}")
        if input_channels < 1 or num_layers < 1:
            raise ValueError("Vocos: input_channels and num_layers are positive")
        chunk = call.gt_vocos_hidden_chunk()
        if not call.gt_vocos_mlp_lds_bytes(dim):
            raise ValueError(f"Vocos: dim is 128, 256 or 512, got {dim}")
        if intermediate_dim < chunk or intermediate_dim % chunk or intermediate_dim > 2048:
            raise ValueError(f"Vocos: intermediate_dim is a multiple of {chunk} up to 2048, got {intermediate_dim}")
        self.input_channels, self.dim, self.intermediate_dim, self.num_layers = input_channels, dim, intermediate_dim, num_layers
        self.n_fft, self.hop_length, self.padding = 1024, 256, padding
        self.mel_channels = self.padded_channels = _pad16(input_channels)
        self.mel_padding = self.padded_channels - input_channels
        self.backbone = _VocosBackbone(input_channels, dim, intermediate_dim, num_layers)
        self.head = _VocosHead(dim, self.n_fft)
        object.__setattr__(self, "istft", InverseSTFT())                       # not a submodule: the state dict keeps the published names
        self.launches = 6 + 2 * num_layers
        self._images = _Cached()
        for p in self.parameters():
            p.requires_grad_(False)

    def _apply(self, fn, *args, **kw):
        super()._apply(fn, *args, **kw)
        self.istft._apply(fn, *args, **kw)
        return self

    @classmethod
    def from_config(cls, cfg):
        """from the published config.yaml as a dict: the init_args of its `backbone` and `head` entries (the feature extractor's
        n_mels is the backbone's input_channels)"""
        b, h = dict(cfg["backbone"].get("init_args", {})), dict(cfg["head"].get("init_args", {}))
        if "dim" in h and "dim" in b and int(h["dim"]) != int(b["dim"]):
            raise ValueError(f"Vocos: the head's dim {h['dim']} is not the backbone's {b['dim']}")
        return cls(input_channels=b.get("input_channels", 80), dim=b.get("dim", 512), intermediate_dim=b.get("intermediate_dim", 1536),
                   num_layers=b.get("num_layers", 8), n_fft=h.get("n_fft", 1024), hop_length=h.get("hop_length", 256),
                   padding=h.get("padding", "same"), adanorm_num_embeddings=b.get("adanorm_num_embeddings"))

    def load_vocos_state(self, sd):
        """a published checkpoint's state dict: feature_extractor.* and head.istft.window are dropped, the rest is loaded strictly"""
        keep = {k: t.detach().float() for k, t in sd.items() if not k.startswith("feature_extractor.") and k != "head.istft.window"}
        return self.load_state_dict(keep, strict=True)

    # ---- the images: everything a run reads, per parameter version ----------------------------------------------------------------------
    def images(self):
        """dict(embed=(image, bias), norm=(g, b), blocks=[dict(wd, bd, g, b, W1, b1, W2, b2)], final=(g, b), head=(image, bias)): bf16
        images in gt_voc_conv's fragment order (the embedding's input channels zero-padded to a multiple of 16, the layer scale folded
        into W2 / b2), fp32 vectors; rebuilt when any parameter's (data_ptr, _version) changes"""
        params = list(self.parameters())

        def build():
            f = lambda t: t.detach().float().contiguous()  # noqa: E731
            bb = self.backbone
            we = bb.embed.weight.detach().float()
            out = dict(embed=(voc_pack(_padded(we, (self.dim, self.padded_channels, 7))), f(bb.embed.bias)),
                       norm=(f(bb.norm.weight), f(bb.norm.bias)), blocks=[],
                       final=(f(bb.final_layer_norm.weight), f(bb.final_layer_norm.bias)),
                       head=(voc_pack(self.head.out.weight.detach().float()[:, :, None]), f(self.head.out.bias)))
            for blk in bb.convnext:
                w2, b2 = fold_layer_scale(blk.gamma, blk.pwconv2.weight, blk.pwconv2.bias)
                out["blocks"].append(dict(wd=f(blk.dwconv.weight).view(self.dim, 7), bd=f(blk.dwconv.bias), g=f(blk.norm.weight),
                                          b=f(blk.norm.bias), W1=voc_pack(blk.pwconv1.weight.detach().float()[:, :, None]),
                                          b1=f(blk.pwconv1.bias), W2=voc_pack(w2[:, :, None]), b2=b2.contiguous()))
            return out
        return self._images.get(params, build)

    def held(self):
        """what a captured graph of run() reads besides the buffers: its holder keeps it alive (the vocoder drops it when it repacks)"""
        return self.images(), self.istft._image()

    # ---- capacity-sized form ------------------------------------------------------------------------------------------------------------
    def check_graph_input(self):
        if self.mel_padding:
            raise ValueError(f"compile_synthesis(vocoder=): {self.input_channels} mel channels, the graph takes multiples of 16")

    def buffer_spec(self, B, F_max):
        """[(name, dtype, elements)] of the buffers a run takes next to wav [B, 256 (F_max - 1)]: the fp32 residual stream x [B, F, C],
        the bf16 operand a [B, F, C], the head's fp32 output o [B, F, 1026] and the spectrum workspace spec: 6 B F C + 4104 B F +
        4100 B Fp + 1024 B (F - 1) bytes with Fp = F rounded up to 64, 12.3 KB per frame at C = 512"""
        self._check_capacity(B, F_max, B * F_max * 2 * VOCOS_BINS, "B >= 1, F_max >= 2 and B F_max 1026 < 2^31")
        E = B * F_max * self.dim
        return [("x", torch.float32, E), ("a", torch.bfloat16, E), ("o", torch.float32, B * F_max * 2 * VOCOS_BINS),
                ("spec", torch.float32, call.gt_gl_spec_bytes(B, F_max) // 4)]

    def run(self, mel, n_frames, bufs):
        """_MelVocoder.run for a model whose own channel count is a multiple of 16 (forward pads the others' mel)"""
        if self.mel_padding:
            raise ValueError(f"run takes a mel of a multiple of 16 channels; forward pads the {self.input_channels} of this model")
        return super().run(mel, n_frames, bufs)

    def _walk(self, mel, n_frames, bufs, B, F):
        C, H, Cm, wav = self.dim, self.intermediate_dim, self.mel_channels, bufs["wav"]
        dev, im = mel.device, self.images()
        st = _lib.current_stream(dev)
        x, a_, o, spec = bufs["x"], bufs["a"], bufs["o"], bufs["spec"]
        sb = F * C

        def conv(X, img, Y, Cin, N, taps, x_sb, y_sb, **kw):
            call.gt_voc_conv(_lib.fill_args(_lib.VocConvArgs, X=X, x_stride_b=x_sb, W=img[0], bias=img[1], res=None, acc=None, Y=Y,
                                            y_stride_b=y_sb, ldy=N, len_mul=1, n_frames=n_frames, B=B, L_cap=F, Cin=Cin, N=N, taps=taps,
                                            dil=1, y_bf16=0, tanh_out=0, slope=1.0, scale=1.0, **kw), st)

        def norm(gb, Y, y_bf16, wd=None, bd=None):
            call.gt_vocos_norm(_lib.fill_args(_lib.VocosNormArgs, X=x, x_stride_b=sb, wd=wd, bd=bd, g=gb[0], be=gb[1], Y=Y, y_stride_b=sb,
                                              n_frames=n_frames, B=B, L_cap=F, C=C, y_bf16=y_bf16, eps=VOCOS_EPS), st)

        conv(mel, im["embed"], x, Cm, C, 7, mel.stride(0) if B > 1 else max(mel.stride(0), F), sb,
             x_stride_c=mel.stride(1) if Cm > 1 else max(mel.stride(1), F), x_mel=1, x_bf16=0)
        norm(im["norm"], x, 0)
        for blk in im["blocks"]:
            norm((blk["g"], blk["b"]), a_, 1, wd=blk["wd"], bd=blk["bd"])
            call.gt_vocos_mlp(_lib.fill_args(_lib.VocosMlpArgs, A=a_, a_stride_b=sb, W1=blk["W1"], b1=blk["b1"], W2=blk["W2"], b2=blk["b2"],
                                             R=x, r_stride_b=sb, Y=x, y_stride_b=sb, U=None, u_stride_b=0, n_frames=n_frames, B=B, L_cap=F,
                                             C=C, H=H), st)
        norm(im["final"], a_, 1)
        conv(a_, im["head"], o, C, 2 * VOCOS_BINS, 1, sb, F * 2 * VOCOS_BINS, x_stride_c=0, x_mel=0, x_bf16=1)
        call.gt_vocos_polar(_lib.fill_args(_lib.VocosPolarArgs, O=o, o_stride_b=F * 2 * VOCOS_BINS, n_frames=n_frames, spec=spec, B=B,
                                           F_max=F, n_fft=self.n_fft), st)
        self.istft.synthesize(spec, n_frames, B, F, out=wav)
        return wav


# ---- WaveGlow: the reverse flow on csrc/waveglow.hip next to gt_voc_conv ------------------------------------------------
WG_GROUP = 8                         # samples per group position: the one n_group the kernels implement
WG_UP_KERNEL, WG_UP_STRIDE = 1024, 256


def transposed_tail_as_conv(w, u):
    """ConvTranspose1d weight [Cin, Cout, m u] (stride u, no padding, the last (m - 1) u outputs dropped: WaveGlow's upsampler) -> the
    centred (2m - 1)-tap convolution weight [u * Cout, Cin, 2m - 1] with W[r * Cout + c, ci, m - 1 - j] = w[ci, c, r + u j] for j < m
    and 0 in the m - 1 taps that look ahead: output u q + r reads inputs q - (m - 1) .. q only, w[., ., r + u j] meeting input q - j.
    transposed_as_conv's generalisation to a kernel of m strides."""
    Cin, Cout, k = w.shape
    if u < 1 or k % u or k < u:
        raise ValueError(f"the kernel is a multiple of the stride, got k = {k}, u = {u}")
    m = k // u
    W = w.new_zeros(u, Cout, Cin, 2 * m - 1)
    W[..., :m] = w.detach().view(Cin, Cout, m, u).permute(3, 1, 0, 2).flip(3)
    return W.reshape(u * Cout, Cin, 2 * m - 1)


def gate_interleave(C):
    """row order of gt_wg_gate's images: packed row 64 q + r is channel 32 q + r, packed row 64 q + 32 + r channel C + 32 q + r"""
    return torch.arange(2 * C).view(2, C // 32, 32).permute(1, 0, 2).reshape(-1)


class _WaveGlowWN(nn.Module):
    """parameter holder under the published names: start, in_layers, cond_layer (the v5 layout: one 640 -> 2C n convolution),
    res_skip_layers, end"""

    def __init__(self, n_in, n_cond, n_layers, C, k):
        super().__init__()
        self.start = nn.Conv1d(n_in, C, 1)
        self.in_layers = nn.ModuleList(nn.Conv1d(C, 2 * C, k, dilation=2 ** i, padding=2 ** i * (k - 1) // 2) for i in range(n_layers))
        self.cond_layer = nn.Conv1d(n_cond, 2 * C * n_layers, 1)
        self.res_skip_layers = nn.ModuleList(nn.Conv1d(C, 2 * C if i < n_layers - 1 else C, 1) for i in range(n_layers))
        self.end = nn.Conv1d(C, 2 * n_in, 1)


class _InvConv(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv = nn.Conv1d(c, c, 1, bias=False)


class WaveGlow(_MelVocoder):
    """The published WaveGlow network (Prenger et al. 2018) in its `infer` direction, eval mode, weight norm folded: from log-mel and a
    seeded latent to waveform, every utterance of a ragged batch ON ITS OWN (utterance b is infer(mel[b:b+1, :, :F_b]) on its own rows of
    the latent); F_b frames give 256 F_b samples.

      upsample (ConvTranspose1d 80 -> 80, k 1024, stride 256, the last 768 outputs dropped: gt_voc_conv as a 7-tap convolution at frame
      rate whose 20480 outputs per frame ARE spect [32 F, 640], channel 8 band + sample % 8) -> the latent's last n_remaining channels
      (gt_wg_boundary, first form) -> per flow j = n_flows - 1 .. 0: WN_j as n x (gt_wg_gate: in_layer + conditioning slice + gate;
      gt_voc_conv: res_skip onto the x | skip state) and one gt_wg_boundary (end, coupling inverse, inverse 1x1, early-output concat,
      the next start): `launches` = 1 + n_flows 2 n + n_flows + 1, 206 for the published config.

    Z[b, l, 2p], Z[b, l, 2p + 1] = sigma (e0, e1) of randn_pair(randn_key(seed, 5, b), l, p) (csrc/common.h, stream id 5): the flow starts
    from Z[..., 8 - n_remaining:], every early-output point prepends the next two channels towards channel 0.  `seed` is forward's /
    run's argument, or run's device word `seed_dev`.

    Parameters are fp32 under the published names (upsample, WN.{j}.start / .in_layers.{i} / .cond_layer / .res_skip_layers.{i} / .end,
    convinv.{j}.conv.weight); `load_waveglow_state` takes a published state dict.  Operands of the matrix products are bf16 (the packed
    images; the mel, the residual stream as staged, spect, the gate's output), accumulation, the residual stream, the skip sum and
    everything between two WaveNets fp32; the inverse of every 1x1 weight is formed on the host in float64.
    Refused with ValueError: n_group != 8, kernel_size != 3, n_channels no multiple of 64 (or above 512), n_layers > 8, an upsampler
    other than 1024 / 256, n_early_size != 2, an n_flows / n_early_every whose channel count leaves [2, 8], n_mel_channels != 80."""

    seeded = True
    hop_length, min_frames, mel_channels = WG_UP_STRIDE, 1, 80

    def __init__(self, n_mel_channels=80, n_flows=12, n_group=8, n_early_every=4, n_early_size=2, n_layers=8, n_channels=256,
                 kernel_size=3, sigma=0.666, upsample_kernel_size=1024, upsample_stride=256):
        super().__init__()
        n_flows, n_early_every, n_layers, C = int(n_flows), int(n_early_every), int(n_layers), int(n_channels)
        if int(n_group) != WG_GROUP:
            raise ValueError(f"WaveGlow: n_group is {WG_GROUP} (the kernels' 8 slots per position), got {n_group}")
        if int(kernel_size) != 3:
            raise ValueError(f"WaveGlow: kernel_size is 3, got {kernel_size}")
        if C < 64 or C % 64 or C > _lib.WG_MAX_C:
            raise ValueError(f"WaveGlow: n_channels is a multiple of 64 up to {_lib.WG_MAX_C}, got {n_channels}")
        if n_layers < 1 or n_layers > 8:
            raise ValueError(f"WaveGlow: n_layers is 1 .. 8 (dilation 2^7 = 128 is what the gate kernel's LDS holds), got {n_layers}")
        if (int(upsample_kernel_size), int(upsample_stride)) != (WG_UP_KERNEL, WG_UP_STRIDE):
            raise ValueError(f"WaveGlow: the upsampler is ConvTranspose1d(k = 1024, stride = 256), got {upsample_kernel_size} / {upsample_stride}")
        if int(n_early_size) != 2:
            raise ValueError(f"WaveGlow: n_early_size is 2, got {n_early_size}")
        if int(n_mel_channels) != 80:
            raise ValueError(f"WaveGlow: 80 mel bands, got {n_mel_channels}")
        if n_flows < 1 or n_early_every < 1:
            raise ValueError("WaveGlow: n_flows and n_early_every are positive")
        # channels of flow k, as the original's constructor counts them: two fewer from every early-output point on
        self.flow_channels = [WG_GROUP - 2 * len([e for e in range(1, k + 1) if e % n_early_every == 0]) for k in range(n_flows)]
        if min(self.flow_channels) < 2:
            raise ValueError(f"WaveGlow: n_flows = {n_flows} with n_early_every = {n_early_every} leaves {min(self.flow_channels)} channels "
                             "for the last flows; the count must stay within [2, 8]")
        self.n_flows, self.n_group, self.n_early_every, self.n_early_size = n_flows, WG_GROUP, n_early_every, 2
        self.n_layers, self.n_channels, self.kernel_size, self.sigma = n_layers, C, 3, float(sigma)
        if not self.sigma >= 0.0:
            raise ValueError(f"WaveGlow: sigma is non-negative, got {sigma}")
        self.n_mel_channels, self.n_cond = 80, 80 * WG_GROUP
        self.n_remaining = self.flow_channels[-1]
        self.upsample = nn.ConvTranspose1d(80, 80, WG_UP_KERNEL, stride=WG_UP_STRIDE)
        self.WN = nn.ModuleList(_WaveGlowWN(c // 2, self.n_cond, n_layers, C, 3) for c in self.flow_channels)
        self.convinv = nn.ModuleList(_InvConv(c) for c in self.flow_channels)
        self.launches = 1 + n_flows * 2 * n_layers + n_flows + 1
        self._images = _Cached()
        for p in self.parameters():
            p.requires_grad_(False)

    @classmethod
    def from_config(cls, cfg):
        """from NVIDIA's config.json as a dict (its `waveglow_config` entry, or that entry itself); sigma where the dict has one"""
        w = dict(cfg.get("waveglow_config", cfg))
        wn = dict(w.get("WN_config", {}))
        kw = dict(sigma=w["sigma"]) if "sigma" in w else {}
        return cls(n_mel_channels=w.get("n_mel_channels", 80), n_flows=w.get("n_flows", 12), n_group=w.get("n_group", 8),
                   n_early_every=w.get("n_early_every", 4), n_early_size=w.get("n_early_size", 2), n_layers=wn.get("n_layers", 8),
                   n_channels=wn.get("n_channels", 256), kernel_size=wn.get("kernel_size", 3), **kw)

    def load_waveglow_state(self, sd):
        """a state dict under the published names.  The published .pt files pickle the whole module: the caller passes
        ckpt["model"].state_dict().  Both conditioning layouts load — `WN.j.cond_layer` (the universal v5 checkpoints: one 640 -> 2C n
        convolution) and the older per-layer `WN.j.cond_layers.i` (concatenated along the outputs, which is the same function) — each
        with weight norm (weight_g / weight_v, folded g v / ||v|| in float64 and rounded once) or a folded weight; strict."""
        flat = {}
        for k, t in sd.items():
            if k.endswith(".weight_g"):
                flat[k[:-2]] = fold_weight_norm(t, sd[k[:-1] + "v"])
            elif not k.endswith(".weight_v"):
                flat[k] = t.detach().float().cpu()
        out = {k: t for k, t in flat.items() if ".cond_layers." not in k}
        for j in range(self.n_flows):
            for kind in ("weight", "bias"):
                parts = [flat.get(f"WN.{j}.cond_layers.{i}.{kind}") for i in range(self.n_layers)]
                if all(p is not None for p in parts):
                    out[f"WN.{j}.cond_layer.{kind}"] = torch.cat(parts, 0)
                elif any(p is not None for p in parts):
                    raise KeyError(f"WN.{j}.cond_layers: {kind} of some layers is missing")
        extra = [k for k in flat if ".cond_layers." in k and int(k.split(".")[3]) >= self.n_layers]
        if extra:
            raise KeyError(f"unexpected keys {extra}")
        return self.load_state_dict(out, strict=True)

    # ---- the images: everything a run reads, per parameter version ----------------------------------------------------------------------
    def inverse64(self, j):
        """float64 [c, c]: the inverse of convinv.j.conv.weight, formed on the host as store_inverse does for the decoder"""
        return torch.linalg.inv(self.convinv[j].conv.weight.detach().double().cpu()[:, :, 0])

    def images(self):
        """dict(up=(image, bias), flows=[dict(start=(w [C][8], b), layers=[dict(W_in, W_cond, b_in, b_cond, res=(image, bias))],
        end=(w [C][8], b [8]), inv=w [8][8])]): bf16 images in gt_voc_conv's fragment order (the gate's rows interleaved), the
        boundary's fp32 matrices in slot order (include/glowtts_hip.h); rebuilt when any parameter's (data_ptr, _version) changes"""
        params = list(self.parameters())

        def build():
            dev, C, n = params[0].device, self.n_channels, self.n_layers
            f = lambda t: t.detach().float().contiguous().to(dev)  # noqa: E731
            # output 256 q + 8 l + i of band m is channel 640 l + 8 m + i of frame q: spect at the group rate
            W7 = transposed_tail_as_conv(self.upsample.weight.detach().float(), WG_UP_STRIDE)           # [256 * 80, 80, 7], row r * 80 + m
            W7 = W7.view(32, WG_GROUP, 80, 80, 7).permute(0, 2, 1, 3, 4).reshape(32 * 80 * WG_GROUP, 80, 7)
            bias = self.upsample.bias.detach().float().view(1, 80, 1).expand(32, 80, WG_GROUP).reshape(-1)
            out = dict(up=(voc_pack(W7), f(bias)), flows=[])
            perm = gate_interleave(C).to(dev)
            for j, c in enumerate(self.flow_channels):
                wn, lo, h = self.WN[j], WG_GROUP - c, c // 2
                w_start = torch.zeros(C, 8)
                w_start[:, lo:lo + h] = wn.start.weight.detach().float().cpu()[:, :, 0]
                we = wn.end.weight.detach().float().cpu()[:, :, 0]
                be = wn.end.bias.detach().float().cpu()
                w_end, b_end = torch.zeros(C, 8), torch.zeros(8)                       # column s - 4: slot s's shift, column s: its log-scale
                w_end[:, lo + h - 4:4], w_end[:, lo + h:8] = we[:h].t(), we[h:].t()
                b_end[lo + h - 4:4], b_end[lo + h:8] = be[:h], be[h:]
                w_inv = torch.zeros(8, 8, dtype=torch.float64)
                w_inv[lo:, lo:] = self.inverse64(j)
                layers = []
                for i in range(n):
                    wc = wn.cond_layer.weight.detach().float()[2 * C * i:2 * C * (i + 1)]
                    rs = wn.res_skip_layers[i]
                    layers.append(dict(W_in=voc_pack(wn.in_layers[i].weight.detach().float()[perm]), W_cond=voc_pack(wc[perm]),
                                       b_in=f(wn.in_layers[i].bias), b_cond=f(wn.cond_layer.bias.detach()[2 * C * i:2 * C * (i + 1)]),
                                       res=(voc_pack(rs.weight.detach().float()), f(rs.bias))))
                out["flows"].append(dict(start=(f(w_start), f(wn.start.bias)), layers=layers, end=(f(w_end), f(b_end)), inv=f(w_inv)))
            return out
        return self._images.get(params, build)

    def held(self):
        """what a captured graph of run() reads besides the buffers: its holder keeps it alive (the vocoder drops it when it repacks)"""
        return self.images()

    # ---- capacity-sized form ------------------------------------------------------------------------------------------------------------
    def buffer_spec(self, B, F_max):
        """[(name, dtype, elements)] of the buffers a run takes next to wav [B, 256 F_max] (which doubles as the flow's 8 audio slots
        per group position), with L = 32 F_max group positions: the fp32 state x | skip [B, L, 2C], the gate's bf16 output g [B, L, C]
        and the bf16 spect [B, L, 640]: B L (10 C + 1280) + 1024 B F_max bytes, 123 KB per frame at C = 256 — 3.17 GB at 32 x 800
        frames.  B L max(2C, 640) must stay below 2^31."""
        L, C = 32 * F_max, self.n_channels
        E = B * L * max(2 * C, self.n_cond)
        self._check_capacity(B, F_max, E, f"B >= 1, F_max >= 1 and 32 B F_max max(2C, 640) = {E} < 2^31")
        return [("state", torch.float32, B * L * 2 * C), ("g", torch.bfloat16, B * L * C), ("spect", torch.bfloat16, B * L * self.n_cond)]

    def _walk(self, mel, n_frames, bufs, B, F, seed_dev=None, seed=0):
        C, n, Cs, wav = self.n_channels, self.n_layers, self.n_cond, bufs["wav"]
        dev, im = mel.device, self.images()
        st = _lib.current_stream(dev)
        state, g, spect = bufs["state"], bufs["g"], bufs["spect"]
        L = 32 * F

        def conv(X, img, Y, Cin, N, taps, L_cap, mul, x_sb, y_sb, ldy, **kw):
            call.gt_voc_conv(_lib.fill_args(_lib.VocConvArgs, X=X, x_stride_b=x_sb, W=img[0], bias=img[1], res=None, Y=Y, y_stride_b=y_sb,
                                            ldy=ldy, len_mul=mul, n_frames=n_frames, B=B, L_cap=L_cap, Cin=Cin, N=N, taps=taps, dil=1,
                                            tanh_out=0, slope=1.0, scale=1.0, **kw), st)

        def boundary(prev, nxt, c_in, c_out):
            call.gt_wg_boundary(_lib.fill_args(
                _lib.WgBoundaryArgs, state=state, st_stride_b=L * 2 * C, ld=2 * C, C=C, A=wav, a_stride_b=wav.stride(0),
                w_end=prev["end"][0] if prev else None, b_end=prev["end"][1] if prev else None, w_inv=prev["inv"] if prev else None,
                w_start=nxt["start"][0] if nxt else None, b_start=nxt["start"][1] if nxt else None, n_frames=n_frames, seed_dev=seed_dev,
                seed=int(seed) & 0xFFFFFFFF, sigma=self.sigma, len_mul=32, B=B, L_cap=L, c_in=c_in, c_out=c_out), st)

        N_up = 32 * Cs
        conv(mel, im["up"], spect, 80, N_up, 7, F, 1, mel.stride(0) if B > 1 else max(mel.stride(0), F), F * N_up, N_up,
             x_stride_c=max(mel.stride(1), F), x_mel=1, x_bf16=0, y_bf16=1, acc=None)
        chans, flows = self.flow_channels, im["flows"]
        boundary(None, flows[-1], 0, chans[-1])
        for j in range(self.n_flows - 1, -1, -1):
            fl = flows[j]
            for i, ly in enumerate(fl["layers"]):
                call.gt_wg_gate(_lib.fill_args(_lib.WgGateArgs, X=state, x_stride_b=L * 2 * C, ldx=2 * C, Cs=Cs, S=spect, s_stride_b=L * Cs,
                                               W_in=ly["W_in"], W_cond=ly["W_cond"], b_in=ly["b_in"], b_cond=ly["b_cond"], G=g,
                                               g_stride_b=L * C, len_mul=32, n_frames=n_frames, B=B, L_cap=L, C=C, taps=3, dil=2 ** i), st)
                # x += r[:C], skip += r[C:] in one call on the state (Y aliases acc); the last layer's C outputs go to the skip half
                Y = state if i < n - 1 else state[C:]
                conv(g, ly["res"], Y, C, 2 * C if i < n - 1 else C, 1, L, 32, L * C, L * 2 * C, 2 * C, x_stride_c=0, x_mel=0, x_bf16=1,
                     y_bf16=0, acc=Y)
            c_out = chans[j - 1] if j else WG_GROUP
            boundary(fl, flows[j - 1] if j else None, chans[j], c_out)
        return wav


# ---- spectral-subtraction denoiser: NVIDIA's WaveGlow `Denoiser` on csrc/denoise.hip and gt_istft ----------------------
class Denoiser(nn.Module):
    """NVIDIA's WaveGlow `Denoiser` (denoiser.py, mode="zeros") on the device:
    denoised = STFT.inverse(clamp(|X| - strength * bias_spec, min=0), angle X), X = STFT(audio), by TWO C-ABI calls — gt_denoise_spec
    (csrc/denoise.hip: the analysis with Y = X max(|X| - c, 0) / |X| as its epilogue, no atan2 / cos / sin) and gt_istft — every
    utterance of a ragged batch on its own.  Owns `stft` (an audio.STFT at 1024 / 256 / 1024; its forward basis image), `istft` (an
    InverseSTFT), the buffer `bias_spec` fp32 [513] (zeros until from_vocoder / load_state_dict / an assignment fills it) and the
    one-element fp32 buffer `strength_dev` the kernel reads: `set_strength` between two replays of a captured graph changes the next one.
    Samples come in hops of 256: an utterance of L samples is denoised over its first 256 (L // 256)."""

    def __init__(self, stft=None, bias_spec=None, strength=0.1):
        super().__init__()
        self.stft = STFT() if stft is None else stft
        if not isinstance(self.stft, STFT):
            raise TypeError("Denoiser(stft=) takes an audio.STFT")
        _check_geometry(self.stft)
        self.istft = InverseSTFT(self.stft.filter_length, self.stft.hop_length, self.stft.win_length)
        bias = torch.zeros(513) if bias_spec is None else bias_spec.detach().to(torch.float32).reshape(-1).clone()
        if bias.numel() != 513:
            raise ValueError(f"bias_spec is [513], got {bias.numel()} values")
        self.register_buffer("bias_spec", bias)
        self.register_buffer("strength_dev", torch.zeros(1, dtype=torch.float32, device=bias.device), persistent=False)
        self._fwd_packed, self._bias, self._source = _Cached(), _Cached(), None
        self.set_strength(strength)

    # -- the strength: checked on the host (the shrinkage is non-expansive for c >= 0 only), kept in the word the kernel reads
    def set_strength(self, s):
        s = float(s)
        if not (np.isfinite(s) and s >= 0.0):
            raise ValueError(f"Denoiser: strength is finite and non-negative, got {s}")
        self.strength = s
        # a blocking copy from the host: the word holds s when this returns, whichever stream a captured graph is replayed on next
        self.strength_dev.copy_(torch.tensor([s], dtype=torch.float32))
        return self

    def _forward_image(self):
        fb = self.stft.forward_basis
        return self._fwd_packed.get((fb,), lambda: _plain_stft_image(fb))

    def held(self):
        """what a captured graph of run() reads besides the buffers: the two packed images, the bias and the strength word"""
        return self._forward_image(), self.istft._image(), self.bias(), self.strength_dev

    # -- the bias spectrum of a vocoder
    @classmethod
    def from_vocoder(cls, voc, frames=88, strength=0.1):
        """the Denoiser of `voc` (a _MelVocoder on the device): bias_spec = frame 0 of |STFT(voc(zeros [1, n_mel, frames]))|, a seeded
        vocoder (WaveGlow) run at sigma = 0 for that one call.  The vocoder is remembered (in a tuple: not a submodule): bias() rebuilds
        bias_spec, in place, when a parameter of the vocoder has changed (_Cached, as the packed images are)."""
        if not isinstance(voc, _MelVocoder):
            raise TypeError("Denoiser.from_vocoder takes one of audio's vocoders")
        if voc.hop_length != 256:
            raise ValueError(f"Denoiser: the STFT has a hop of 256 samples, the vocoder's is {voc.hop_length}")
        den = cls(strength=strength).to(next(voc.parameters()).device)
        den._source = (voc, int(frames))
        den.bias()
        return den

    def bias(self):
        """bias_spec: as it stands, or (from_vocoder) brought up to date with the vocoder's parameters first"""
        if self._source is None:
            return self.bias_spec
        voc, frames = self._source
        return self._bias.get(tuple(voc.parameters()), lambda: self._measure_bias(voc, frames))

    def _measure_bias(self, voc, frames):
        dev = self.bias_spec.device
        mel = torch.zeros(1, voc.mel_channels - voc.mel_padding, frames, dtype=torch.float32, device=dev)
        sigma = getattr(voc, "sigma", None)
        try:
            if voc.seeded:
                voc.sigma = 0.0                                               # the attribute _walk reads; the vocoder itself is unchanged
            wav = voc(mel)
        finally:
            if voc.seeded:
                voc.sigma = sigma
        hops = wav.shape[1] // 256
        if hops < 1:
            raise ValueError(f"{frames} frames give the vocoder no sample to take a bias spectrum from")
        strength = self.strength
        try:
            self.set_strength(0.0)                                            # strength 0: the kernel writes X itself
            bufs = self.workspace(1, hops, dev)
            self.analyse(wav[:, :256 * hops].contiguous(), torch.full((1,), hops, dtype=torch.int32, device=dev), 0, bufs)
        finally:
            self.set_strength(strength)
        re, im = spec_unpack(bufs["dn_spec"], 1, hops + 1)
        self.bias_spec.copy_(torch.hypot(re[0, :, 0], im[0, :, 0]))
        return self.bias_spec

    # -- capacity-sized form
    def buffer_spec(self, B, F_max, lost=0):
        """[(name, dtype, elements)] of a run behind a vocoder of capacity (B, F_max mel frames): the spectrum workspace at
        Fa_max = F_max - lost + 1 analysis frames and the int32 [B] analysis frame counts"""
        n = call.gt_gl_spec_bytes(B, F_max - lost + 1) // 4
        if n == 0:
            raise ValueError(f"denoiser workspace for {B} x {F_max} frames: outside what gt_denoise_spec takes")
        return [("dn_spec", torch.float32, n), ("dn_frames", torch.int32, B)]

    def workspace(self, B, F_max, device, lost=0):
        return {name: torch.empty(n, dtype=dt, device=device) for name, dt, n in self.buffer_spec(B, F_max, lost)}

    def analyse(self, wav, n_frames, lost, bufs):
        """kernel call: bufs["dn_spec"] = the denoised spectrum of wav's rows, bufs["dn_frames"] = their analysis frame counts"""
        B = wav.shape[0]
        F_max = wav.shape[1] // 256 + lost
        call.gt_denoise_spec(_lib.fill_args(_lib.DenoiseSpecArgs, wav=wav, bias=self.bias_spec, strength=self.strength_dev,
                                            n_frames=n_frames, mel_packed=self._forward_image(), spec=bufs["dn_spec"],
                                            frames_out=bufs["dn_frames"], ld_wav=wav.stride(0), lost=lost, B=B, F_max=F_max, n_fft=1024,
                                            hop=256, win=1024), _lib.current_stream(wav.device))
        return F_max - lost + 1

    def run(self, wav, n_frames, lost, bufs):
        """kernel calls, the capacity-sized form for graph callers: wav fp32 [B, 256 (F_max - lost)] (a vocoder's workspace rows: row b
        holds 256 max(n_frames[b] - lost, 0) samples), device int32 [B] MEL frame counts, lost = the vocoder's min_frames - 1 and
        workspace's buffers -> wav, denoised in place, zero behind each utterance.  gt_denoise_spec, gt_istft: nothing is allocated once
        the images exist, nothing is looked at on the host, both grids are sized by the capacity."""
        if not wav.is_cuda:
            raise CpuWaveError("glow_tts_amd.audio runs on the MI355X only (got a CPU waveform); there is no CPU fallback")
        if wav.dim() != 2 or wav.dtype != torch.float32 or wav.stride(1) != 1 or wav.shape[1] % 256 or wav.shape[1] == 0:
            raise ValueError(f"run takes fp32 rows of a multiple of 256 samples, got {tuple(wav.shape)} {wav.dtype}")
        if lost not in (0, 1):
            raise ValueError(f"lost is 0 or 1, got {lost}")
        if n_frames.dtype != torch.int32 or n_frames.numel() != wav.shape[0] or not n_frames.is_cuda or not n_frames.is_contiguous():
            raise ValueError("n_frames must be a contiguous int32 [B] on the device")
        bias = self.bias()                                                    # from_vocoder: up to date with the vocoder's parameters
        if bias.device != wav.device or bias.dtype != torch.float32 or not bias.is_contiguous() or self.strength_dev.dtype != torch.float32:
            raise ValueError("the denoiser's buffers are contiguous fp32 on the waveforms' device")
        Fa_max = self.analyse(wav, n_frames, lost, bufs)
        self.istft.synthesize(bufs["dn_spec"], bufs["dn_frames"], wav.shape[0], Fa_max, out=wav)
        return wav

    def denoise(self, wav, lengths=None, lengths_host=None, strength=None):
        """the stand-alone use, on any waveform: padded fp32 rows [B, T] (lengths: their sample counts, default T) -> wav_d [B, T], or
        (wav_d, lengths floored to a multiple of 256) with lengths; zero behind each utterance.  `strength` sets the module's first."""
        if not wav.is_cuda:
            raise CpuWaveError("glow_tts_amd.audio runs on the MI355X only (got a CPU waveform); there is no CPU fallback")
        if wav.dim() != 2 or wav.dtype != torch.float32:
            raise ValueError(f"waveforms are [B, T] fp32, got {tuple(wav.shape)} {wav.dtype}")
        if strength is not None:
            self.set_strength(strength)
        B, T = wav.shape
        if lengths is None:
            hops = torch.full((B,), T // 256, dtype=torch.int32, device=wav.device)
        else:
            if lengths_host is None and not lengths.is_cuda:
                lengths_host = lengths.tolist()
            if lengths.numel() != B or (lengths_host is not None and (len(lengths_host) != B or max(lengths_host, default=0) > T)):
                raise ValueError(f"lengths do not fit waveforms {tuple(wav.shape)}")
            hops = (lengths.to(wav.device, non_blocking=True) // 256).to(torch.int32).contiguous()
        F_max = T // 256
        if B and F_max:
            rows = torch.empty(B, 256 * F_max, dtype=torch.float32, device=wav.device)    # run works in place: never on the caller's rows
            self.run(rows.copy_(wav[:, :256 * F_max]), hops, 0, self.workspace(B, F_max, wav.device))
            out = rows if T == 256 * F_max else torch.cat([rows, rows.new_zeros(B, T - 256 * F_max)], 1)
        else:
            out = wav.new_zeros(B, T)
        if lengths is None:
            return out
        return out, hops.clamp(min=0, max=F_max) * 256

    forward = denoise


class Denoised(_MelVocoder):
    """A vocoder with the spectral-subtraction Denoiser behind it, itself a _MelVocoder: everything the
    contract names is the inner vocoder's, `launches` two more, buffer_spec / held the denoiser's on top, and _walk the inner walk
    followed by Denoiser.run on the samples where they stand.  compile_synthesis(vocoder=Denoised(...)) needs nothing else.
    denoiser=None: Denoiser.from_vocoder(vocoder, strength=strength).  Only 256-sample hops (the STFT's)."""

    def __init__(self, vocoder, denoiser=None, strength=0.1):
        super().__init__()
        if not isinstance(vocoder, _MelVocoder):
            raise TypeError("Denoised wraps one of audio's vocoders")
        if vocoder.hop_length != 256:
            raise ValueError(f"Denoised: the denoiser's STFT has a hop of 256 samples, the vocoder's is {vocoder.hop_length}")
        self.vocoder = vocoder
        self.denoiser = Denoiser.from_vocoder(vocoder, strength=strength) if denoiser is None else denoiser
        self.hop_length, self.min_frames = vocoder.hop_length, vocoder.min_frames
        self.mel_channels, self.mel_padding, self.seeded = vocoder.mel_channels, vocoder.mel_padding, vocoder.seeded
        self.launches = vocoder.launches + 2

    def set_strength(self, s):
        self.denoiser.set_strength(s)
        return self

    def check_graph_input(self):
        self.vocoder.check_graph_input()

    def buffer_spec(self, B, F_max):
        return self.vocoder.buffer_spec(B, F_max) + self.denoiser.buffer_spec(B, F_max, self.min_frames - 1)

    def held(self):
        return self.vocoder.held(), self.denoiser.held()

    def _walk(self, mel, n_frames, bufs, B, F, **seed):
        wav = self.vocoder._walk(mel, n_frames, bufs, B, F, **seed)
        return self.denoiser.run(wav, n_frames, self.min_frames - 1, bufs)


# ---- ITU-R BS.1770-4 integrated loudness and normalisation on csrc/loudness.hip ---------------------------------------
KW_SHELF_DB, KW_SHELF_Q, KW_SHELF_HZ, KW_SHELF_VB = 3.99984385397, 0.7071752369554193, 1681.9744509555319, 0.499666774155
KW_HP_Q, KW_HP_HZ = 0.5003270373253953, 38.13547087613982
LOUD_SCAN_RUN = 16                   # the state scan's fan-in: the kernels read M, M^16 and M^256


def kweighting64(fs):
    """the K-weighting cascade at sampling rate fs in float64: ((b, a) of the high shelf, (b, a) of the high-pass), a[0] = 1.  At
    48 kHz the recommendation's table to 1e-11."""
    fs = float(fs)
    K = np.tan(np.pi * KW_SHELF_HZ / fs)
    Vh = 10.0 ** (KW_SHELF_DB / 20.0)
    Vb = Vh ** KW_SHELF_VB
    a0 = 1.0 + K / KW_SHELF_Q + K * K
    shelf = (np.array([(Vh + Vb * K / KW_SHELF_Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / KW_SHELF_Q + K * K) / a0]),
             np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / KW_SHELF_Q + K * K) / a0]))
    K = np.tan(np.pi * KW_HP_HZ / fs)
    a0 = 1.0 + K / KW_HP_Q + K * K
    hp = (np.array([1.0, -2.0, 1.0]), np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / KW_HP_Q + K * K) / a0]))
    return shelf, hp


def kweighting_transition64(fs, n):
    """M [4, 4] float64: the cascade's state after n samples of zero input is M times its state before them.  The state is the
    kernel's: (s1, s2) of the shelf, then of the high-pass, each biquad in transposed direct form II (y = b0 x + s1;
    s1 = b1 x - a1 y + s2; s2 = b2 x - a2 y), the shelf's output the high-pass's input.  The n-th power of the one-sample matrix of
    kweighting64's float64 coefficients is taken in 400-bit fixed point (integer arithmetic, square and multiply) and rounded once:
    every entry is within half an ulp, or 2^-390 where that is more, of the filter's own transition — a float64 product of n factors
    loses 1e-11 of the largest entry by n = 800, and 1e-6 by n = 12 800, to the cancellation in the high-pass's near-double pole."""
    (_, a), (c, d) = kweighting64(fs)
    a1, a2, c0, c1, c2, d1, d2 = (Fraction(float(v)) for v in (a[1], a[2], c[0], c[1], c[2], d[1], d[2]))
    # one sample of zero input: y = s1; s1' = -a1 y + s2; s2' = -a2 y; z = c0 y + t1; t1' = c1 y - d1 z + t2; t2' = c2 y - d2 z
    A = [[-a1, 1, 0, 0], [-a2, 0, 0, 0], [c1 - d1 * c0, 0, -d1, 1], [c2 - d2 * c0, 0, -d2, 0]]
    P = 400                                                # float64 coefficients and their products are exact at this scale
    base = [[int(Fraction(v) * (1 << P)) for v in row] for row in A]

    def mul(X, Y):
        return [[sum(X[i][k] * Y[k][j] for k in range(4)) >> P for j in range(4)] for i in range(4)]

    R, k = [[int(i == j) << P for j in range(4)] for i in range(4)], int(n)
    while k:
        if k & 1:
            R = mul(R, base)
        base, k = mul(base, base), k >> 1
    return np.array([[R[i][j] / (1 << P) for j in range(4)] for i in range(4)])        # int / int: correctly rounded


def loudness_chunk(fs):
    """the chunk length csrc/loudness.hip cuts utterances into at sampling rate fs (the largest divisor of fs / 10 in [16, 50]); 0 for a
    rate the kernels do not take"""
    return call.gt_loudness_chunk(int(fs)) if float(fs) == int(fs) else 0


class Loudness(nn.Module):
    """ITU-R BS.1770-4 integrated loudness (mono: K-weighting, 400 ms blocks at 75 % overlap, the -70 LKFS and the relative -10 LU
    gate) of every utterance of a ragged batch on its own, and normalisation to `target_lufs` (EBU R 128: -23) under a SAMPLE peak
    ceiling of `peak_dbfs`, by TWO C-ABI calls: gt_loudness_measure (four launches, all in double) and gt_loudness_apply (one).  An
    utterance shorter than 400 ms is one block over all its samples; silence and no sample read -inf and are left as they are (g = 1).
    Owns `params`, the float64 words the kernels read on the device: coefficients, the chunk transition matrices, the target and the
    ceiling — `set_target` between two replays of a captured graph changes the next one."""

    launches = 2                     # C-ABI calls of run(): gt_loudness_measure, gt_loudness_apply
    kernels = 5                      # kernel launches behind them
    STATS = ("lufs", "peak", "gain", "blocks", "gated_abs", "gated_rel", "gamma", "samples")   # the columns of a stats row

    def __init__(self, sampling_rate=22050, target_lufs=-23.0, peak_dbfs=-1.0):
        super().__init__()
        if float(sampling_rate) != int(sampling_rate) or not loudness_chunk(sampling_rate):
            raise ValueError(f"Loudness: csrc/loudness.hip takes no sampling rate of {sampling_rate} Hz (a multiple of 10 in "
                             "[8000, 192000] whose tenth has a divisor in [16, 50])")
        self.sampling_rate, self.chunk = int(sampling_rate), loudness_chunk(sampling_rate)
        (b, a), (c, d) = kweighting64(self.sampling_rate)
        p = np.zeros(_lib.LOUD_PARAMS)
        p[0:5], p[5:10] = (*b, a[1], a[2]), (*c, d[1], d[2])
        p[10:26] = kweighting_transition64(self.sampling_rate, self.chunk).reshape(-1)
        p[26:42] = kweighting_transition64(self.sampling_rate, self.chunk * LOUD_SCAN_RUN).reshape(-1)
        p[44:60] = kweighting_transition64(self.sampling_rate, self.chunk * LOUD_SCAN_RUN ** 2).reshape(-1)
        self.register_buffer("params", torch.from_numpy(p), persistent=False)
        self.set_target(target_lufs, peak_dbfs)

    def set_target(self, lufs, peak_dbfs=None):
        """the target in LUFS and (peak_dbfs: not None) the sample peak ceiling in dBFS, checked on the host, kept in the words the
        kernel reads"""
        lufs = float(lufs)
        peak_dbfs = getattr(self, "peak_dbfs", None) if peak_dbfs is None else float(peak_dbfs)
        if not np.isfinite(lufs) or peak_dbfs is None or not np.isfinite(peak_dbfs):
            raise ValueError(f"Loudness: the target and the peak ceiling are finite, got {lufs} LUFS, {peak_dbfs} dBFS")
        self.target_lufs, self.peak_dbfs = lufs, peak_dbfs
        # a blocking copy from the host: the words hold the values when this returns, whichever stream a graph is replayed on next
        self.params[42:44].copy_(torch.tensor([lufs, 10.0 ** (peak_dbfs / 20.0)], dtype=torch.float64))
        return self

    def held(self):
        """what a captured graph of run() reads besides the buffers: the parameter words"""
        return (self.params,)

    # -- capacity-sized form
    def buffer_spec(self, B, F_max, hop=1, lost=0):
        """[(name, dtype, elements)] of a run on rows of hop (F_max - lost) samples: the workspace and the stats rows"""
        n = call.gt_loudness_ws_bytes(B, hop * (F_max - lost), self.sampling_rate) // 4
        if n == 0:
            raise ValueError(f"loudness workspace for {B} x {hop * (F_max - lost)} samples: outside what gt_loudness_measure takes")
        return [("ld_ws", torch.float32, n), ("ld_stats", torch.float32, _lib.LOUD_STATS * B)]

    def workspace(self, B, F_max, device, hop=1, lost=0):
        return {name: torch.empty(n, dtype=dt, device=device) for name, dt, n in self.buffer_spec(B, F_max, hop, lost)}

    def chunk_sums(self, bufs, B, L_cap):
        """dev / tests: the workspace's per-chunk sums of z^2 after a measurement at capacity (B, L_cap samples): a float64 view
        [B, ceil(L_cap / chunk)]; the entries of chunks an utterance does not have are undefined"""
        Kc = -(-L_cap // self.chunk)
        return bufs["ld_ws"].view(torch.float64)[4 * B * Kc:5 * B * Kc].view(B, Kc)

    def _args(self, wav, n_frames, hop, lost, bufs, out=None):
        if self.params.dtype != torch.float64 or self.params.device != wav.device or not self.params.is_contiguous():
            raise ValueError("the loudness parameters are float64 on the waveforms' device")
        return _lib.fill_args(_lib.LoudnessArgs, wav=wav, n_frames=n_frames, params=self.params, stats=bufs["ld_stats"], ws=bufs["ld_ws"],
                              out=out, ws_bytes=bufs["ld_ws"].numel() * 4, ld=wav.stride(0) if wav.shape[0] > 1 else wav.shape[1],
                              ld_out=0 if out is None else out.stride(0) if out.shape[0] > 1 else out.shape[1],
                              is_i16=int(wav.dtype == torch.int16), hop=hop, lost=lost, B=wav.shape[0], L_cap=wav.shape[1],
                              fs=self.sampling_rate)

    def run(self, wav, n_frames, hop, lost, bufs):
        """kernel calls, the capacity-sized form for graph callers: wav fp32 [B, hop (F_max - lost)] (a vocoder's workspace rows: row b
        holds hop max(n_frames[b] - lost, 0) samples), device int32 [B] frame counts and workspace's buffers -> wav, normalised in
        place, zero behind each utterance; bufs["ld_stats"] holds the stats rows.  Nothing is allocated, nothing is looked at on the
        host, every grid is sized by the capacity."""
        if not wav.is_cuda:
            raise CpuWaveError("glow_tts_amd.audio runs on the MI355X only (got a CPU waveform); there is no CPU fallback")
        if hop < 1 or lost < 0:
            raise ValueError(f"hop is positive and lost non-negative, got {hop}, {lost}")
        if wav.dim() != 2 or wav.dtype != torch.float32 or wav.stride(1) != 1 or wav.shape[1] == 0 or wav.shape[1] % hop:
            raise ValueError(f"run takes fp32 rows of a multiple of {hop} samples, got {tuple(wav.shape)} {wav.dtype}")
        if n_frames.dtype != torch.int32 or n_frames.numel() != wav.shape[0] or not n_frames.is_cuda or not n_frames.is_contiguous():
            raise ValueError("n_frames must be a contiguous int32 [B] on the device")
        st = _lib.current_stream(wav.device)
        args = self._args(wav, n_frames, hop, lost, bufs)
        call.gt_loudness_measure(args, st)
        call.gt_loudness_apply(args, st)
        return wav

    # -- the stand-alone uses, on any padded batch
    def _lengths(self, wav, lengths, lengths_host, dtypes):
        if not wav.is_cuda:
            raise CpuWaveError("glow_tts_amd.audio runs on the MI355X only (got a CPU waveform); there is no CPU fallback")
        if wav.dim() != 2 or wav.dtype not in dtypes:
            raise ValueError(f"waveforms are [B, T] {' or '.join(str(d) for d in dtypes)}, got {tuple(wav.shape)} {wav.dtype}")
        B, T = wav.shape
        if lengths is None:
            return torch.full((B,), T, dtype=torch.int32, device=wav.device)
        if lengths_host is None and not lengths.is_cuda:
            lengths_host = lengths.tolist()
        if lengths.numel() != B or (lengths_host is not None and (len(lengths_host) != B or max(lengths_host, default=0) > T)):
            raise ValueError(f"lengths do not fit waveforms {tuple(wav.shape)}")
        return lengths.to(wav.device, non_blocking=True).to(torch.int32).clamp(min=0, max=T).contiguous()

    def _measure(self, wav, n):
        """-> (stats fp32 [B, 8], the buffers) of rows that hold samples; rows of no sample are written on the host's side"""
        B, T = wav.shape
        if B == 0 or T == 0:
            row = torch.tensor([-np.inf, 0.0, 1.0, 0.0, 0.0, 0.0, -np.inf, 0.0], dtype=torch.float32, device=wav.device)
            return row.repeat(B, 1), None
        if wav.stride(1) != 1:
            wav = wav.contiguous()
        bufs = self.workspace(B, T, wav.device)
        call.gt_loudness_measure(self._args(wav, n, 1, 0, bufs), _lib.current_stream(wav.device))
        return bufs["ld_stats"].view(B, _lib.LOUD_STATS), bufs

    def measure(self, wav, lengths=None, lengths_host=None):
        """padded fp32 or int16 rows [B, T] (lengths: their sample counts, default T) -> dict of per-utterance fp32 device tensors:
        lufs (-inf for silence), peak, gain (what normalize would apply), blocks, gated_abs, gated_rel (the counts J, |A|, |R|), gamma,
        samples, and `stats` [B, 8], the rows as the kernel wrote them.  No host synchronisation where lengths is a device tensor."""
        n = self._lengths(wav, lengths, lengths_host, (torch.float32, torch.int16))
        stats, _ = self._measure(wav, n)
        out = {name: stats[:, i] for i, name in enumerate(self.STATS)}
        out["stats"] = stats
        return out

    def normalize(self, wav, lengths=None, lengths_host=None):
        """padded fp32 rows [B, T] -> wav_n [B, T] (a new tensor: never the caller's rows), or (wav_n, lengths) with lengths; every
        utterance at the target, or at the peak ceiling where the target would pass it; zero behind each utterance."""
        n = self._lengths(wav, lengths, lengths_host, (torch.float32,))
        B, T = wav.shape
        out = torch.empty(B, T, dtype=torch.float32, device=wav.device)
        if B and T:
            src = wav if wav.stride(1) == 1 else wav.contiguous()
            _, bufs = self._measure(src, n)
            call.gt_loudness_apply(self._args(src, n, 1, 0, bufs, out=out), _lib.current_stream(wav.device))
        return out if lengths is None else (out, n)

    forward = normalize


class Normalized(_MelVocoder):
    """A vocoder with the Loudness stage behind it, itself a _MelVocoder: everything the contract names is the
    inner vocoder's, `launches` the Loudness stage's more, buffer_spec / held the stage's on top, and _walk the inner walk followed by
    Loudness.run on the samples where they stand.  Any hop; around Denoised too: Normalized(Denoised(WaveGlow(...))).
    loudness=None: Loudness(22050, target_lufs, peak_dbfs) on the vocoder's device."""

    def __init__(self, vocoder, loudness=None, target_lufs=-23.0, peak_dbfs=-1.0):
        super().__init__()
        if not isinstance(vocoder, _MelVocoder):
            raise TypeError("Normalized wraps one of audio's vocoders")
        if loudness is None:
            loudness = Loudness(target_lufs=target_lufs, peak_dbfs=peak_dbfs).to(next(vocoder.parameters()).device)
        if not isinstance(loudness, Loudness):
            raise TypeError("Normalized(loudness=) takes an audio.Loudness")
        self.vocoder, self.loudness = vocoder, loudness
        self.hop_length, self.min_frames = vocoder.hop_length, vocoder.min_frames
        self.mel_channels, self.mel_padding, self.seeded = vocoder.mel_channels, vocoder.mel_padding, vocoder.seeded
        self.launches = vocoder.launches + loudness.launches

    def set_target(self, lufs, peak_dbfs=None):
        self.loudness.set_target(lufs, peak_dbfs)
        return self

    def check_graph_input(self):
        self.vocoder.check_graph_input()

    def buffer_spec(self, B, F_max):
        return self.vocoder.buffer_spec(B, F_max) + self.loudness.buffer_spec(B, F_max, self.hop_length, self.min_frames - 1)

    def held(self):
        return self.vocoder.held(), self.loudness.held()

    def _walk(self, mel, n_frames, bufs, B, F, **seed):
        wav = self.vocoder._walk(mel, n_frames, bufs, B, F, **seed)
        return self.loudness.run(wav, n_frames, self.hop_length, self.min_frames - 1, bufs)
