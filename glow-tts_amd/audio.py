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

Waveforms are fp32 in [-1, 1] or int16 (scaled by 1/32768 in the kernel = the reference's audio / max_wav_value).  There is no CPU
path: a CPU tensor raises."""
import numpy as np
import torch
from torch import nn

from . import _lib
from ._lib import call

CLIP_VAL = 1e-5                      # audio_processing.dynamic_range_compression's clip_val


class CpuWaveError(_lib.CpuTensorError, ValueError):
    """a CPU waveform: the wrong value for a device op (ValueError), and the CpuTensorError every other op here raises"""


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
        self._packed, self._packed_key = None, None

    # -- the fragment-order image of both buffers, rebuilt when either changes (load_state_dict, .to(), an in-place edit)
    def _image(self):
        fb, mb = self.stft_fn.forward_basis, self.mel_basis
        key = (fb.data_ptr(), fb._version, mb.data_ptr(), mb._version)
        if self._packed_key != key:
            if fb.dtype != torch.float32 or mb.dtype != torch.float32 or not fb.is_contiguous() or not mb.is_contiguous():
                raise ValueError("forward_basis and mel_basis must be contiguous fp32 buffers")
            if mb.dim() != 2 or mb.shape[1] != self.stft_fn.filter_length // 2 + 1 or fb.shape[0] != 2 * mb.shape[1]:
                raise ValueError(f"mel_basis {tuple(mb.shape)} does not fit forward_basis {tuple(fb.shape)}")
            packed = torch.empty(call.gt_mel_pack_bytes() // 4, dtype=torch.float32, device=fb.device)
            call.gt_mel_pack(fb, mb, self.stft_fn.filter_length, mb.shape[0], packed, _lib.current_stream(fb.device))
            self._packed, self._packed_key = packed, key
        return self._packed

    def transform(self, y, wav_len, F_max, magnitudes=False):
        """the kernel call: y [B, T] fp32 / int16 on the device, wav_len device int32 [B], F_max frames per output row ->
        (mel [B, n_mel, F_max], energy [B, F_max], mag [B, 513, F_max] or None); no host synchronisation, capturable in a graph
        once the image exists (any earlier call)."""
        if not y.is_cuda:
            raise CpuWaveError("glow_tts_amd.audio runs on the MI355X only (got a CPU waveform); there is no CPU fallback")
        if y.dim() != 2 or y.dtype not in (torch.float32, torch.int16):
            raise ValueError(f"waveforms are [B, T] fp32 or int16, got {tuple(y.shape)} {y.dtype}")
        if wav_len.device != y.device or wav_len.dtype != torch.int32 or wav_len.numel() != y.shape[0]:
            raise ValueError("wav_len must be int32 [B] on the waveforms' device")
        B, T = y.shape
        if y.stride(1) != 1 or y.stride(0) % 4 or y.data_ptr() % 16:          # the kernel takes 16-byte aligned rows of a 4-element pitch
            padded = y.new_zeros(B, (T + 3) // 4 * 4)
            padded[:, :T] = y
            y = padded
        fs = self.stft_fn
        n_mel = self.mel_basis.shape[0]
        packed = self._image()
        mel = torch.empty(B, n_mel, F_max, dtype=torch.float32, device=y.device)
        energy = torch.empty(B, F_max, dtype=torch.float32, device=y.device)
        mag = torch.empty(B, fs.filter_length // 2 + 1, F_max, dtype=torch.float32, device=y.device) if magnitudes else None
        call.gt_mel_spectrogram(y, int(y.dtype == torch.int16), y.stride(0), wav_len.contiguous(), B, F_max, packed, fs.filter_length,
                                fs.hop_length, fs.win_length, n_mel, CLIP_VAL, mel, energy, mag, _lib.current_stream(y.device))
        return mel, energy, mag

    def mel_spectrogram(self, y, lengths=None, lengths_host=None):
        """mel_spectrogram(y): the reference's call, y [B, T] -> (mel [B, n_mel, F], energy [B, F]), F = 1 + T // hop.
        mel_spectrogram(y, lengths[, lengths_host]): padded rows of a batch with their sample counts -> (mel [B, n_mel, F_max],
        mel_lengths = 1 + lengths // hop, energy [B, 1, F_max]), every utterance transformed on its own (reflected about its own ends)
        and zero behind its frames.  F_max comes from the lengths when the host knows them (lengths_host, or CPU `lengths`), else from
        T with no synchronisation.  A length <= filter_length / 2 has no reflect padding: ValueError where the host knows it."""
        if not y.is_cuda:
            raise CpuWaveError("glow_tts_amd.audio runs on the MI355X only (got a CPU waveform); there is no CPU fallback")
        hop, half = self.stft_fn.hop_length, self.stft_fn.filter_length // 2
        B, T = y.shape
        if lengths is None:
            if T <= half:
                raise ValueError(f"{T} samples: reflect padding needs more than {half}")
            wav_len = torch.full((B,), T, dtype=torch.int32, device=y.device)
            mel, energy, _ = self.transform(y, wav_len, 1 + T // hop)
            return mel, energy
        if lengths_host is None and not lengths.is_cuda:
            lengths_host = lengths.tolist()
        if lengths_host is not None:
            lengths_host = [int(v) for v in lengths_host]
            if len(lengths_host) != B or max(lengths_host) > T:
                raise ValueError(f"lengths {lengths_host} do not fit waveforms {tuple(y.shape)}")
            if min(lengths_host) <= half:
                raise ValueError(f"an utterance of {min(lengths_host)} samples: reflect padding needs more than {half}")
            F_max = 1 + max(lengths_host) // hop
        else:
            F_max = 1 + T // hop
        lengths = lengths.to(y.device, non_blocking=True)
        mel, energy, _ = self.transform(y, lengths.to(torch.int32), F_max)
        return mel, 1 + lengths // hop, energy.unsqueeze(1)


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

    def transform(self, y, wav_len, F_max, aux=False, lead=None):
        """the kernel call: y [B, T] fp32 / int16 on the device, wav_len device int32 [B], F_max positions per output row ->
        (f0 [B, F_max], harm or None, argmin_f0 or None); frame i of an utterance lands at position lead + i (lead: pad_frames),
        every other position is 0.  No host synchronisation, capturable in a graph."""
        y = _device_rows(y)
        if wav_len.device != y.device or wav_len.dtype != torch.int32 or wav_len.numel() != y.shape[0]:
            raise ValueError("wav_len must be int32 [B] on the waveforms' device")
        B = y.shape[0]
        f0 = torch.empty(B, F_max, dtype=torch.float32, device=y.device)
        harm = torch.empty_like(f0) if aux else None
        amin = torch.empty_like(f0) if aux else None
        call.gt_yin_f0(y, int(y.dtype == torch.int16), y.stride(0), wav_len.contiguous(), B, F_max, self.frame_length, self.hop_length,
                       self.tau_min, self.tau_max, float(self.sampling_rate), float(self.harm_thresh),
                       self.pad_frames if lead is None else lead, f0, harm, amin, _lib.current_stream(y.device))
        return f0, harm, amin

    def f0(self, y, lengths=None, lengths_host=None, aux=False):
        """y [B, T] (lengths: sample counts of the padded rows, default T) -> f0 [B, 1, F_max] with F_max = 1 + max(lengths) // hop,
        chosen as TacotronSTFT.mel_spectrogram(y, lengths) chooses it (from the lengths where the host knows them, else from T with
        no synchronisation): the contour lines up with that call's mel and energy, zero behind every utterance's frames.
        aux=True: (f0, harm [B, 1, F_max], argmin_f0 [B, 1, F_max])."""
        if not y.is_cuda:
            raise CpuWaveError("glow_tts_amd.audio runs on the MI355X only (got a CPU waveform); there is no CPU fallback")
        B, T = y.shape
        if lengths is None:
            wav_len = torch.full((B,), T, dtype=torch.int32, device=y.device)
            F_max = 1 + T // self.hop_length
        else:
            if lengths_host is None and not lengths.is_cuda:
                lengths_host = lengths.tolist()
            if lengths_host is not None:
                lengths_host = [int(v) for v in lengths_host]
                if len(lengths_host) != B or max(lengths_host) > T:
                    raise ValueError(f"lengths {lengths_host} do not fit waveforms {tuple(y.shape)}")
                F_max = 1 + max(lengths_host) // self.hop_length
            else:
                F_max = 1 + T // self.hop_length
            wav_len = lengths.to(y.device, non_blocking=True).to(torch.int32)
        f0, harm, amin = self.transform(y, wav_len, F_max, aux=aux)
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
