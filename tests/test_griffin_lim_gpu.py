"""GPU tests of the waveform back end as a whole (glow_tts_amd.audio.InverseSTFT / GriffinLim / griffin_lim, csrc/griffin_lim.hip;
DESIGN.md 4.20): batch invariance bit for bit, zeros and canaries behind the rows, the Python loop against hand-composed kernel
calls, graph capture, seeding, the refusals, convergence against the float64 loop of tests/gl64.py, and mel inversion."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gl64 as G  # noqa: E402
import mel64 as M  # noqa: E402

pytestmark = pytest.mark.gpu
HOP = 256


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def gl_mel():
    from glow_tts_amd import audio
    return audio.GriffinLim(audio.TacotronSTFT()).to(dev())


@functools.lru_cache(maxsize=None)
def ragged():
    """frames, fp32 magnitudes [B, 513, F_max] of the ragged batch's signals (7.0 behind each utterance), fixed angles"""
    from glow_tts_amd import _lib
    frames = G.ragged_frames(_lib.lib().gt_gl_tile_frames(), _lib.lib().gt_gl_tile_hops())
    F_max = max(frames)
    mag = np.full((len(frames), G.NBIN, F_max), 7.0, dtype=np.float32)
    for i, (x, F) in enumerate(zip(G.ragged_signals(frames), frames)):
        mag[i, :, :F] = np.hypot(*G.transform(x))
    ang = np.random.default_rng(7).uniform(-np.pi, np.pi, mag.shape).astype(np.float32)
    return frames, torch.from_numpy(mag).to(dev()), torch.from_numpy(ang).to(dev())


def test_batch_row_equals_the_utterance_alone_and_rows_end_in_zeros(built):
    frames, mag, ang = ragged()
    gl = gl_mel()
    fr = torch.tensor(frames, dtype=torch.int32, device=dev())
    wav, lengths = gl(mag, frames=fr, frames_host=frames, n_iters=2, angles=ang)
    assert wav.shape == (len(frames), HOP * (max(frames) - 1)) and lengths.tolist() == [HOP * (F - 1) for F in frames]
    for i, F in enumerate(frames):
        alone = gl(mag[i:i + 1, :, :F].contiguous(), n_iters=2, angles=ang[i:i + 1, :, :F].contiguous())
        assert alone.shape == (1, HOP * (F - 1))
        assert torch.equal(wav[i, :HOP * (F - 1)], alone[0]), (i, F)
        assert not bool(wav[i, HOP * (F - 1):].any()), (i, F)
        assert bool(torch.isfinite(alone).all()) and float(alone.abs().max()) > 0


def test_canaries_behind_rows_and_workspace_are_intact(built):
    from oracle.guards import Guards
    frames, mag, ang = ragged()
    gl, B, F_max = gl_mel(), len(frames), max(frames)
    fr = torch.tensor(frames, dtype=torch.int32, device=dev())
    cols, ld = HOP * (F_max - 1), HOP * (F_max - 1) + 8
    keep = torch.arange(ld) >= cols                                        # the words between a row's columns and its pitch
    for half in ("polar", "project"):
        g = Guards(dev())
        spec = g.out("spec", (gl.istft.workspace(B, F_max, dev()).numel(),))
        wav = g.out("wav", (B, ld), keep=keep)
        if half == "polar":
            gl.istft.polar(g.inp(mag), g.inp(ang), fr, spec)
        else:
            rows = torch.full((B, ld), float("nan"), device=dev())        # nothing behind an utterance's own samples may be read
            for i, F in enumerate(frames):
                rows[i, :HOP * (F - 1)] = 0.25
            gl.project(rows, g.inp(mag), fr, spec)
        gl.istft.synthesize(spec, fr, B, F_max, out=wav)
        g.verify()


def test_griffin_lim_equals_the_hand_composed_kernel_calls(built):
    from glow_tts_amd import _lib, audio
    frames, mag, ang = ragged()
    gl, B, F_max = gl_mel(), len(frames), max(frames)
    fr = torch.tensor(frames, dtype=torch.int32, device=dev())
    gl.istft._image(), gl.stft._image()                                    # packed once, before the loop that is counted
    with _lib.record_calls() as names:
        wav, _ = audio.griffin_lim(mag, gl, n_iters=3, frames=fr, frames_host=frames, angles=ang)
    launches = [n for n in names if not n.endswith("_bytes")]
    assert launches == ["gt_gl_polar", "gt_istft"] + ["gt_gl_project", "gt_istft"] * 3                       # 2 + 2 n launches
    L, st = _lib.lib(), _lib.current_stream(dev())
    spec = torch.empty(L.gt_gl_spec_bytes(B, F_max) // 4, dtype=torch.float32, device=dev())
    out = torch.empty(B, HOP * (F_max - 1), dtype=torch.float32, device=dev())
    p = lambda t: t.data_ptr()  # noqa: E731
    inv_img, fwd_img = gl.istft._image(), gl.stft._image()
    assert L.gt_gl_polar(p(mag), p(ang), p(fr), B, F_max, 1024, 256, 1024, p(spec), st) == 0
    assert L.gt_istft(p(spec), p(fr), B, F_max, p(inv_img), 1024, 256, 1024, p(out), out.stride(0), st) == 0
    for _ in range(3):
        assert L.gt_gl_project(p(out), out.stride(0), p(mag), p(fr), B, F_max, p(fwd_img), 1024, 256, 1024, p(spec), st) == 0
        assert L.gt_istft(p(spec), p(fr), B, F_max, p(inv_img), 1024, 256, 1024, p(out), out.stride(0), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(wav, out)


def test_graph_capture_replayed_on_new_magnitudes_equals_eager(built):
    frames, mag, ang = ragged()
    gl = gl_mel()
    fr = torch.tensor(frames, dtype=torch.int32, device=dev())
    gl(mag, frames=fr, frames_host=frames, n_iters=1, angles=ang)          # the packed images exist before the capture
    static_mag = mag.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out, _ = gl(static_mag, frames=fr, frames_host=frames, n_iters=2, angles=ang)
    other = (mag * 0.5 + 0.125).contiguous()
    static_mag.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    eager, _ = gl(other, frames=fr, frames_host=frames, n_iters=2, angles=ang)
    assert torch.equal(static_out, eager)
    first, _ = gl(mag, frames=fr, frames_host=frames, n_iters=2, angles=ang)
    assert not torch.equal(first, eager)


def test_seed_decides_the_samples(built):
    _, mag, _ = ragged()
    gl = gl_mel()
    m = mag[2:3, :, :20].contiguous()
    a, b, c = gl(m, n_iters=1, seed=3), gl(m, n_iters=1, seed=3), gl(m, n_iters=1, seed=4)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(c).all())


def test_refusals(built):
    from glow_tts_amd import audio
    _, mag, ang = ragged()
    gl = gl_mel()
    with pytest.raises(ValueError):
        gl(mag[:1, :, :3].contiguous(), n_iters=1)
    with pytest.raises(ValueError):
        gl(mag[:2], frames=torch.tensor([5, 3]), n_iters=1)
    with pytest.raises(ValueError):
        gl(mag[:2], frames=torch.tensor([5, 3], dtype=torch.int32, device=dev()), frames_host=[5, 3], n_iters=1)
    with pytest.raises(audio.CpuWaveError):
        gl(mag.cpu(), n_iters=1)
    with pytest.raises(audio.CpuWaveError):
        gl.istft.inverse(mag.cpu(), ang.cpu())
    with pytest.raises(audio.CpuWaveError):
        gl.from_mel(torch.zeros(1, 80, 8))


@pytest.mark.parametrize("name", ["chirp", "noise"])
def test_convergence_matches_the_float64_loop(built, name):
    """c_i = || |STFT(x_i)| - M || / || M || after 30 iterations, against gl64's float64 loop from the same angles and from two
    other seeds: inside their [min, max] widened on each side by their own spread (how far a perturbed trajectory moves the end
    point — all fp32 can do to it), and below half of c_0."""
    F = 20
    x = M.signal(name, HOP * (F - 1))
    mag64 = np.hypot(*G.transform(x))
    mag32 = mag64.astype(np.float32)
    rng = np.random.default_rng(11)
    angles = [rng.uniform(-np.pi, np.pi, mag32.shape).astype(np.float32) for _ in range(3)]
    ends, starts = [], []
    for a in angles:
        x0, xn = G.griffin_lim64(mag32, a.astype(np.float64), 30)
        starts.append(G.convergence(x0, mag32)); ends.append(G.convergence(xn, mag32))
    gl = gl_mel()
    m, a = torch.from_numpy(mag32[None]).to(dev()), torch.from_numpy(angles[0][None]).to(dev())
    c0 = G.convergence(gl(m, n_iters=0, angles=a)[0].double().cpu().numpy(), mag32)
    c30 = G.convergence(gl(m, n_iters=30, angles=a)[0].double().cpu().numpy(), mag32)
    lo, hi = min(ends), max(ends)
    spread = hi - lo
    print(f"{name}: device c_0 {c0:.4f} c_30 {c30:.4f}; float64 c_0 {min(starts):.4f}..{max(starts):.4f}, c_30 {lo:.4f}..{hi:.4f}")
    assert abs(c0 - starts[0]) < 1e-4                                      # the first inverse is the same linear map of the same angles
    assert lo - spread <= c30 <= hi + spread
    assert c30 < 0.5 * c0


def test_from_mel(built):
    gl = gl_mel()
    lengths = [HOP * 19, HOP * 12 + 100]
    y = np.zeros((2, lengths[0]), dtype=np.float32)
    y[0] = M.signal("chirp", lengths[0])
    y[1, :lengths[1]] = M.signal("loud_quiet", lengths[1])
    y = torch.from_numpy(y).to(dev())
    ln = torch.tensor(lengths, dtype=torch.int32, device=dev())
    mel, mel_len, _ = gl.stft.mel_spectrogram(y, ln, lengths_host=lengths)
    assert mel_len.tolist() == [20, 13]
    dist = []
    for n in (0, 30):
        wav, wav_len = gl.from_mel(mel, mel_len, mel_lengths_host=[20, 13], n_iters=n, seed=5)
        assert wav.shape == (2, HOP * 19) and wav_len.tolist() == [HOP * 19, HOP * 12]
        assert bool(torch.isfinite(wav).all()) and not bool(wav[1, HOP * 12:].any())
        again, again_len, _ = gl.stft.mel_spectrogram(wav, wav_len.to(torch.int32), lengths_host=wav_len.tolist())
        assert again_len.tolist() == [20, 13]
        d = 0.0
        for i, F in enumerate((20, 13)):
            d += float((again[i, :, :F] - mel[i, :, :F]).pow(2).mean().sqrt())
        dist.append(d)
    print(f"from_mel: mel-domain distance {dist[0]:.4f} after 0 iterations, {dist[1]:.4f} after 30")
    assert dist[1] < dist[0]
    one = gl.from_mel(mel[:1], n_iters=1, seed=5)                         # the reference-style call: no lengths, a plain tensor
    assert one.shape == (1, HOP * 19)
