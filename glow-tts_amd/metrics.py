"""Objective synthesis metrics on the device (csrc/dtw.hip): mel-cepstral distortion under dynamic time warping and
F0 errors along the same warping path, for ragged batches, with no host synchronisation.

  MelCepstrum       carries `dct` [n_coef, n_mel] (rows 1..n_coef of the orthonormal DCT-II, float64 rounded once); forward(mel, lengths)
                    is ONE kernel (gt_mel_cepstrum): log-mel [B, n_mel, F] -> [B, F, 16] rows (coefficients n_coef..15 and frames at and
                    past an utterance's length are zero).
  dtw               dynamic time warping of two ragged batches of feature sequences by ONE kernel (gt_dtw_f32) -> DTWResult(cost,
                    path_len, path, status); `.mean` = cost / path_len.
  mcd_dtw           MelCepstrum of both mels, then dtw with scale 10 sqrt(2) / ln 10: `.mean` is MCD-DTW in dB.
  f0_errors         F0 RMSE (Hz and cents), voicing decision error and gross pitch error along a DTWResult's path, the counts and sums
                    by ONE kernel (gt_dtw_f0_stats).
  Evaluator         a synthesised mel (and waveform) against the recording: the reference mel through TacotronSTFT.mel_spectrogram,
                    both contours through YIN.f0, everything above in one go.

The MCD here is on the model's own log-mel (natural log, TacotronSTFT), not on WORLD / SPTK mel-cepstra: it compares runs of this model
with each other and is not comparable with numbers from papers that use those.  There is no CPU path: a CPU tensor raises."""
import math

import numpy as np
import torch
from torch import nn

from . import _lib
from ._lib import call

ALPHA_DB = 10.0 * math.sqrt(2.0) / math.log(10.0)
FEATURES = 16                       # floats of a feature row (64 bytes)
MAX_FRAMES = 4096                   # GT_DTW_MAX_F


def dct_matrix64(n_mel, n_coef):
    """float64 [n_coef, n_mel]: dct[k - 1][n] = sqrt(2 / N) cos(pi k (n + 1/2) / N), k = 1..n_coef — scipy.fft.dct(m, type=2,
    norm="ortho")[1:n_coef + 1] as a matrix (c0 is dropped: a gain in the log domain costs nothing)"""
    n = np.arange(n_mel, dtype=np.float64)
    k = np.arange(1, n_coef + 1, dtype=np.float64)
    return math.sqrt(2.0 / n_mel) * np.cos(math.pi * k[:, None] * (n[None, :] + 0.5) / n_mel)


def _lengths_arg(lengths, B, F, device):
    """frame counts as the kernels take them: device int32 [B] (default: every row whole)"""
    if lengths is None:
        return torch.full((B,), F, dtype=torch.int32, device=device)
    if not torch.is_tensor(lengths):
        lengths = torch.tensor([int(v) for v in lengths], dtype=torch.int32)
    if lengths.numel() != B:
        raise ValueError("lengths must be [B]")
    return lengths.to(device, non_blocking=True).to(torch.int32).contiguous()


class MelCepstrum(nn.Module):
    """log-mel [B, n_mel_channels, F] -> cepstra [B, F, 16] by ONE HIP kernel (csrc/dtw.hip: gt_mel_cepstrum); its only buffer is the
    DCT matrix.  n_mel_channels <= 128, n_coef <= 16."""

    def __init__(self, n_mel_channels=80, n_coef=13):
        super().__init__()
        if not (1 <= n_mel_channels <= 128 and 1 <= n_coef <= FEATURES):
            raise ValueError(f"n_mel_channels = {n_mel_channels}, n_coef = {n_coef}: the kernel takes up to 128 channels and 16 coefficients")
        self.n_mel_channels, self.n_coef = n_mel_channels, n_coef
        self.register_buffer("dct", torch.from_numpy(dct_matrix64(n_mel_channels, n_coef).astype(np.float32)))

    def forward(self, mel, lengths=None):
        _lib.require_cuda(mel)
        if mel.dim() != 3 or mel.shape[1] != self.n_mel_channels or mel.dtype != torch.float32:
            raise ValueError(f"mel is fp32 [B, {self.n_mel_channels}, F], got {tuple(mel.shape)} {mel.dtype}")
        B, N, F = mel.shape
        dct = self.dct
        if dct.device != mel.device or dct.dtype != torch.float32 or tuple(dct.shape) != (self.n_coef, N) or not dct.is_contiguous():
            raise ValueError(f"dct must be a contiguous fp32 [{self.n_coef}, {N}] buffer on the mel's device")
        out = torch.empty(B, max(F, 1), FEATURES, dtype=torch.float32, device=mel.device)
        if B == 0 or F == 0:
            return out[:, :F].zero_()
        mel = mel if mel.is_contiguous() else mel.contiguous()
        call.gt_mel_cepstrum(mel, F, _lengths_arg(lengths, B, F, mel.device), dct, B, N, self.n_coef, F, out,
                             _lib.current_stream(mel.device))
        return out


class DTWResult:
    """per-utterance device tensors of one dtw call: cost fp32 [B], path_len int32 [B], path int32 [B, Fa + Fb - 1, 2] ((i, j) forward
    from (0, 0), -1 past path_len), status int32 [1] (GT_DTW_ST_BAD_LEN = 1: some length was below 0 or above its capacity and was
    treated as 0)"""

    def __init__(self, cost, path_len, path, status):
        self.cost, self.path_len, self.path, self.status = cost, path_len, path, status

    @property
    def mean(self):
        """cost / path_len (NaN for an empty utterance)"""
        return self.cost / self.path_len.to(torch.float32)


_workspaces = {}                    # (device, B, Fa, Fb) -> the direction bits and the walk-order path of one call


def _workspace(device, B, Fa, Fb):
    key = (device, B, Fa, Fb)
    if key not in _workspaces:
        _workspaces[key] = torch.empty(call.gt_dtw_workspace_bytes(B, Fa, Fb), dtype=torch.uint8, device=device)
    return _workspaces[key]


def _feature_rows(x, name):
    if x.dim() != 3 or x.dtype != torch.float32 or x.shape[2] > FEATURES or x.shape[2] < 1:
        raise ValueError(f"{name} is fp32 [B, F, K <= {FEATURES}], got {tuple(x.shape)} {x.dtype}")
    if x.shape[1] > MAX_FRAMES:
        raise ValueError(f"{name} has {x.shape[1]} frames: gt_dtw_f32 takes up to {MAX_FRAMES}")
    if x.shape[2] < FEATURES:
        x = torch.nn.functional.pad(x, (0, FEATURES - x.shape[2]))
    return x if x.is_contiguous() else x.contiguous()


def dtw(a, a_lengths, b, b_lengths, scale=1.0):
    """a [B, Fa, K], b [B, Fb, K] fp32 feature sequences (K <= 16, padded to 16 here) with their frame counts (None: every row whole)
    -> DTWResult: D(i, j) = d(i, j) + min(D(i-1, j-1), D(i-1, j), D(i, j-1)), d = scale * the Euclidean distance of the frames, the
    first of that order on equal values.  ONE kernel (gt_dtw_f32), no host synchronisation, capturable in a graph once the
    workspace of the shape exists (any earlier call); the workspace is cached per (device, B, Fa, Fb)."""
    _lib.require_cuda(a, b)
    a, b = _feature_rows(a, "a"), _feature_rows(b, "b")
    if a.shape[0] != b.shape[0] or a.device != b.device:
        raise ValueError("a and b are two batches of the same size on one device")
    B, Fa, Fb, dev = a.shape[0], a.shape[1], b.shape[1], a.device
    ld = max(Fa + Fb - 1, 1)
    cost = torch.empty(B, dtype=torch.float32, device=dev)
    path_len = torch.empty(B, dtype=torch.int32, device=dev)
    path = torch.empty(B, ld, 2, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    if B == 0 or Fa == 0 or Fb == 0:
        return DTWResult(cost.zero_(), path_len.zero_(), path.fill_(-1), status)
    ws = _workspace(dev, B, Fa, Fb)
    call.gt_dtw_f32(a, b, _lengths_arg(a_lengths, B, Fa, dev), _lengths_arg(b_lengths, B, Fb, dev), B, Fa, Fb, float(scale), cost,
                    path_len, path, ld, ws, ws.numel(), status, _lib.current_stream(dev))
    return DTWResult(cost, path_len, path, status)


_cepstra = {}                       # (n_mel, n_coef, device) -> MelCepstrum


def _cepstrum(n_mel, n_coef, device):
    key = (n_mel, n_coef, device)
    if key not in _cepstra:
        _cepstra[key] = MelCepstrum(n_mel, n_coef).to(device)
    return _cepstra[key]


def mcd_dtw(mel_a, len_a, mel_b, len_b, n_coef=13):
    """log-mels [B, n_mel, Fa] (synthesised) and [B, n_mel, Fb] (reference) with their frame counts -> DTWResult whose `.mean` is the
    mel-cepstral distortion along the warping path in dB: three launches (gt_mel_cepstrum twice, gt_dtw_f32)"""
    _lib.require_cuda(mel_a, mel_b)
    if mel_a.dim() != 3 or mel_b.dim() != 3 or mel_a.shape[1] != mel_b.shape[1]:
        raise ValueError(f"two log-mels [B, n_mel, F] of the same channels, got {tuple(mel_a.shape)} and {tuple(mel_b.shape)}")
    cep = _cepstrum(mel_a.shape[1], n_coef, mel_a.device)
    return dtw(cep(mel_a, len_a), len_a, cep(mel_b, len_b), len_b, scale=ALPHA_DB)


def f0_metrics_from_stats(counts, sums, path_len):
    """counts int [B, 3] (n_vv, n_vu, n_gross), sums [B, 2] (sse_hz, sse_cents), path_len [B] -> dict of per-utterance tensors:
    rmse = sqrt(sse / n_vv), vde = n_vu / P, gpe = n_gross / n_vv, each NaN where its denominator is 0.  Plain tensor arithmetic."""
    n_vv = counts[:, 0].to(torch.float32)
    P = path_len.to(torch.float32)
    nan = torch.full_like(n_vv, float("nan"))
    voiced, any_step = n_vv > 0, P > 0
    den = torch.where(voiced, n_vv, torch.ones_like(n_vv))
    return {"rmse_hz": torch.where(voiced, torch.sqrt(sums[:, 0] / den), nan),
            "rmse_cents": torch.where(voiced, torch.sqrt(sums[:, 1] / den), nan),
            "vde": torch.where(any_step, counts[:, 1].to(torch.float32) / torch.where(any_step, P, torch.ones_like(P)), nan),
            "gpe": torch.where(voiced, counts[:, 2].to(torch.float32) / den, nan),
            "n_voiced": counts[:, 0]}


def _contour(f0, name):
    if f0.dim() == 3 and f0.shape[1] == 1:
        f0 = f0[:, 0]
    if f0.dim() != 2 or f0.dtype != torch.float32 or f0.shape[1] < 1:
        raise ValueError(f"{name} is an fp32 contour [B, F] or [B, 1, F] in Hz, got {tuple(f0.shape)} {f0.dtype}")
    return f0 if f0.is_contiguous() else f0.contiguous()


def f0_stats(f0_a, f0_b, result):
    """the kernel call: contours in Hz (0 = unvoiced, YIN.f0's form) and a DTWResult -> (counts int32 [B, 3], sums fp32 [B, 2])"""
    _lib.require_cuda(f0_a, f0_b, result.path)
    f0_a, f0_b = _contour(f0_a, "f0_a"), _contour(f0_b, "f0_b")
    B, dev = result.path.shape[0], result.path.device
    if f0_a.shape[0] != B or f0_b.shape[0] != B:
        raise ValueError("the contours and the path are batches of the same size")
    counts = torch.empty(B, 3, dtype=torch.int32, device=dev)
    sums = torch.empty(B, 2, dtype=torch.float32, device=dev)
    if B:
        call.gt_dtw_f0_stats(result.path, result.path.shape[1], result.path_len, f0_a, f0_a.shape[1], f0_b, f0_b.shape[1], B, counts, sums,
                             _lib.current_stream(dev))
    return counts, sums


def f0_errors(f0_a, f0_b, result):
    """F0 errors along the warping path of `result` (a: synthesised, b: reference): dict of per-utterance device tensors rmse_hz,
    rmse_cents, vde (steps where exactly one side is voiced / path_len), gpe (both-voiced steps more than 20 % of the reference
    apart / both-voiced steps) and n_voiced.  ONE kernel (gt_dtw_f0_stats) and a few tensor operations."""
    counts, sums = f0_stats(f0_a, f0_b, result)
    return f0_metrics_from_stats(counts, sums, result.path_len)


class Evaluator:
    """Scores a synthesised batch against the recordings it was meant to reproduce.

        ev = Evaluator(audio.TacotronSTFT().to(dev), audio.YIN().to(dev))
        s = ev.score(mel_syn, mel_syn_lengths, wav_ref, wav_ref_lengths, wav_syn, wav_syn_lengths)

    -> dict of per-utterance device tensors: mcd (MCD-DTW in dB), cost, path_len, path, status, and — with a yin and a synthesised
    waveform — rmse_hz, rmse_cents, vde, gpe, n_voiced; with loudness=audio.Loudness(...) (at the stft's rate) and a synthesised
    waveform also lufs_ref, lufs_syn and lufs_diff = lufs_syn - lufs_ref (BS.1770-4 integrated loudness; -inf for
    silence), the other outputs unchanged.  No host synchronisation where the lengths are device tensors."""

    def __init__(self, stft, yin=None, n_coef=13, loudness=None):
        self.stft, self.yin, self.n_coef, self.loudness = stft, yin, n_coef, loudness
        self._meters = {}

    def _meter(self, rate, device):
        """self.loudness, or its like at another sampling rate (kept per rate)"""
        if rate is None or int(rate) == self.loudness.sampling_rate:
            return self.loudness
        if (int(rate), device) not in self._meters:
            from . import audio
            self._meters[int(rate), device] = audio.Loudness(int(rate), self.loudness.target_lufs, self.loudness.peak_dbfs).to(device)
        return self._meters[int(rate), device]

    def score(self, mel_syn, mel_syn_lengths, wav_ref, wav_ref_lengths, wav_syn=None, wav_syn_lengths=None, sampling_rate=None):
        """mel_syn [B, n_mel, F] with its frame counts; wav_ref [B, T] (fp32 or int16) with its sample counts, at `sampling_rate`
        where that is not the stft's; wav_syn (at the stft's rate) with its sample counts for the F0 errors"""
        _lib.require_cuda(mel_syn, wav_ref, wav_syn)
        if wav_ref_lengths is not None and not torch.is_tensor(wav_ref_lengths):
            wav_ref_lengths = torch.tensor([int(v) for v in wav_ref_lengths])
        if wav_ref_lengths is None:
            mel_ref, _ = self.stft.mel_spectrogram(wav_ref, sampling_rate=sampling_rate)
            mel_ref_len = None
        else:
            mel_ref, mel_ref_len, _ = self.stft.mel_spectrogram(wav_ref, wav_ref_lengths, sampling_rate=sampling_rate)
        res = mcd_dtw(mel_syn, mel_syn_lengths, mel_ref, mel_ref_len, n_coef=self.n_coef)
        out = {"mcd": res.mean, "cost": res.cost, "path_len": res.path_len, "path": res.path, "status": res.status}
        if self.yin is not None and wav_syn is not None:
            if wav_syn_lengths is not None and not torch.is_tensor(wav_syn_lengths):
                wav_syn_lengths = torch.tensor([int(v) for v in wav_syn_lengths])
            f0_syn = self.yin.f0(wav_syn, wav_syn_lengths)
            f0_ref = self.yin.f0(wav_ref, wav_ref_lengths, sampling_rate=sampling_rate)
            out.update(f0_errors(f0_syn, f0_ref, res))
        if self.loudness is not None and wav_syn is not None:
            # the same meter on both waveforms, each at its own rate (BS.1770's filter is defined per rate: nothing is resampled)
            out["lufs_ref"] = self._meter(sampling_rate, wav_ref.device).measure(wav_ref, wav_ref_lengths)["lufs"]
            out["lufs_syn"] = self.loudness.measure(wav_syn, wav_syn_lengths)["lufs"]
            out["lufs_diff"] = out["lufs_syn"] - out["lufs_ref"]
        return out
