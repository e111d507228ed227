"""TEST INFRASTRUCTURE ONLY — host (numpy) restatement of the product's dropout masks.

Every dropout of the HIP path is a counter hash of (seed, row, col) (glow-tts_amd/csrc/common.h: hash_u32, drop_keep,
drop_keep_gate); the seed of a call is derived in Python from the module's `_step` and fixed per-site offsets, and the
device seed word (ops.seed_word) is XOR-ed in by the kernel.  This module restates all of it on the host, so that a
test can build the exact mask of every site of one module call and hand it to the oracle (oracle/glowtts_ref.py,
`drop=`): {site name: keep * 1/(1-p)} with the site names of the reference's nn.Dropout modules (module path, ':',
call ordinal), e.g. "decoder.flows.2.wn.drop:3" (4th call of that WN's self.drop) or "encoder.encoder.drop:1".

Rows are the rows layout of the product (ops.RowsCtx): frame t of utterance b is row base[b] + HALO + t, with
base[b] = b * (T + 2 HALO) (uniform) or the ragged layout's row0[b] (RowsCtx.row_starts).  The decoder's rows are on the
squeezed time axis.  Attention rows are (b*H + h)*T + i with T the batch's padded text length, the column is key j
(csrc/attn_mfma.hip:153, csrc/encoder_ops.hip:269); every other site's column is the channel of the [R, C] rows matrix.
"""
import numpy as np
import torch

_M32 = 0xFFFFFFFF
SEED_INC = 0x632BE5AB        # ops.bump_seed: the seed word's step (gt_step_zero adds the same constant)


# ----------------------------------------------------------------------------- the hash (csrc/common.h:24-41)
def hash_u32(x):
    """csrc/common.h hash_u32, vectorised: uint32 array in, uint32 array out."""
    x = np.asarray(x, dtype=np.uint64) & _M32
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x7feb352d)) & _M32
    x ^= x >> np.uint64(15); x = (x * np.uint64(0x846ca68b)) & _M32
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def _mix(seed, row, col):
    """seed + row * 0x9E3779B1 + col * 0x85EBCA6B (mod 2^32), broadcast."""
    s = np.asarray(seed, dtype=np.uint64) & _M32
    r = np.asarray(row, dtype=np.uint64) & _M32
    c = np.asarray(col, dtype=np.uint64) & _M32
    return (s + r * np.uint64(0x9E3779B1) + c * np.uint64(0x85EBCA6B)) & _M32


def thresh32(p):
    """(uint32)((double)p * 2^32) with p the fp32 the C-ABI receives (ctypes c_float), as every launcher computes it."""
    return int(float(np.float32(p)) * 4294967296.0)


def thresh16(p):
    """drop_thresh16: the WaveNet gate's 16-bit threshold."""
    return (thresh32(p) + 0x8000) >> 16


def scale(p):
    """1.0f / (1.0f - p) in fp32."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def drop_keep(seed, row, col, thresh):
    """csrc/common.h drop_keep: bool array (broadcast of row, col)."""
    return hash_u32(_mix(seed, row, col)) >= np.uint32(thresh)


def drop_keep_gate(seed, row, chan, t16):
    """csrc/common.h drop_keep_gate -> (keep_t, keep_s): ONE hash per (row, gate channel), low 16 bits for the tanh half,
    high 16 bits for the sigmoid half."""
    h = hash_u32(_mix(seed, row, chan))
    return (h & np.uint32(0xFFFF)) >= np.uint32(t16), (h >> np.uint32(16)) >= np.uint32(t16)


def word_seed(word, seed):
    """The seed a kernel hashes with: the host seed XOR the device word (both uint32)."""
    return (int(word) & _M32) ^ (int(seed) & _M32)


# ----------------------------------------------------------------------------- rows layouts
def row_map(lengths, T, ragged=False, round_to=None):
    """int64 [B, T]: the row of frame t of utterance b in the rows layout of ops.RowsCtx(lengths, T[, lengths_host=lengths,
    round_to]) — the product's own geometry (ops.HALO, RowsCtx.row_starts), not a copy of its arithmetic."""
    from glow_tts_amd import ops
    lengths = [int(v) for v in lengths]
    B = len(lengths)
    if ragged:
        starts, _ = ops.RowsCtx.row_starts(lengths, T, int(round_to or ops.DEFAULT_ROWS.row_round))
        base = np.asarray(starts[:B], dtype=np.int64)
    else:
        base = np.arange(B, dtype=np.int64) * (T + 2 * ops.HALO)
    return base[:, None] + ops.HALO + np.arange(T, dtype=np.int64)[None, :]


def rows_of(rc):
    """row_map of a built ops.RowsCtx (reads its row0 for the ragged layout)."""
    from glow_tts_amd import ops
    if rc.ragged:
        base = rc.row0[:rc.B].cpu().numpy().astype(np.int64)
    else:
        base = np.arange(rc.B, dtype=np.int64) * rc.Tp
    return base[:, None] + ops.HALO + np.arange(rc.T, dtype=np.int64)[None, :]


# ----------------------------------------------------------------------------- one site
def channel_mask(seed, word, rows, C, p):
    """[B, C, T] fp32 keep * scale of a drop_keep(word ^ seed, row, channel) site; rows [B, T]."""
    s = word_seed(word, seed)
    keep = drop_keep(s, rows[:, None, :], np.arange(C)[None, :, None], thresh32(p))
    return torch.from_numpy(keep.astype(np.float32) * scale(p))


def gate_mask(seed, word, rows, H, p):
    """[B, 2H, T] fp32 keep * scale of a WaveNet gate site (drop_keep_gate): channels [0, H) the tanh half, [H, 2H) the
    sigmoid half of the same hash."""
    s = word_seed(word, seed)
    kt, ks = drop_keep_gate(s, rows[:, None, :], np.arange(H)[None, :, None], thresh16(p))
    return torch.from_numpy(np.concatenate([kt, ks], 1).astype(np.float32) * scale(p))


def attn_mask(seed, word, B, H, T, p):
    """[B, H, T, T] fp32 keep * scale of the attention-probability site: row (b*H + h)*T + i, column key j."""
    s = word_seed(word, seed)
    r = (np.arange(B)[:, None, None, None] * H + np.arange(H)[None, :, None, None]) * T + np.arange(T)[None, None, :, None]
    keep = drop_keep(s, r, np.arange(T)[None, None, None, :], thresh32(p))
    return torch.from_numpy(keep.astype(np.float32) * scale(p))


# ----------------------------------------------------------------------------- seeds of one module call
def decoder_seed(step):
    """models.py:85-86: FlowSpecDecoder.forward increments _step, then seed = (_step * 7919) & 0x7fffffff; `step` is the
    value AFTER the increment."""
    return (step * 7919) & 0x7fffffff


def text_encoder_seed(step):
    """text_models.py:122-127: (_step * 104729) & 0x7fffffff after the increment."""
    return (step * 104729) & 0x7fffffff


def duration_seed(step):
    """text_models.py:582: the FlowGenerator's _step (text_models.py:690 increments it) * 31337."""
    return (step * 31337) & 0x7fffffff


# ----------------------------------------------------------------------------- the masks of one module call
def wn_masks(seed, word, rows, n_layers, H, p, pre):
    """modules.WN / WNP self.drop, one call per layer: layer i hashes with seed + i (flow_impl.py:231,242; the whole-WaveNet
    kernel's (drop_seed + layer), csrc/wn_stack.hip:274)."""
    return {f"{pre}drop:{i}": gate_mask(seed + i, word, rows, H, p) for i in range(n_layers)}


def decoder_masks(step, word, rows, n_blocks, n_layers=4, H=192, p=0.05, chain=("wn",), pre="decoder."):
    """Every WaveNet of FlowSpecDecoder.forward: block b, k-th WaveNet of its chain (wn [, wn_energy][, wn_pitch], in that
    order, attentions.py:144-155) uses seed + 16*b + 4*k (flow_impl.py:463,646; models.py:86,166); rows on the squeezed axis."""
    seed = decoder_seed(step)
    out = {}
    for b in range(n_blocks):
        for k, name in enumerate(chain):
            out.update(wn_masks(seed + 16 * b + 4 * k, word, rows, n_layers, H, p, f"{pre}flows.{3 * b + 2}.{name}."))
    return out


def encoder_layer_masks(seed, word, rows, i, B, T, C=192, F=768, n_heads=2, p=0.1, pre="encoder.encoder."):
    """attentions.Encoder layer i (attentions.py:77-84) with the layer seed s (text_models.py:170: seed + 16 + 8 i):
    s + 0 attention P, s + 1 attention output (self.drop call 2i), s + 2 FFN after its ReLU, s + 3 FFN output (self.drop
    call 2i + 1) (encoder_impl.py:131-139)."""
    return {f"{pre}attn_layers.{i}.drop:0": attn_mask(seed + 0, word, B, n_heads, T, p),
            f"{pre}drop:{2 * i}": channel_mask(seed + 1, word, rows, C, p),
            f"{pre}ffn_layers.{i}.drop:0": channel_mask(seed + 2, word, rows, F, p),
            f"{pre}drop:{2 * i + 1}": channel_mask(seed + 3, word, rows, C, p)}


def text_encoder_masks(step, word, rows, B, T, n_layers, C=192, F=768, n_heads=2, p=0.1, prenet=True, p_pre=0.5,
                       pre="encoder."):
    """models.TextEncoder.forward: the prenet's layer i with seed + i (text_models.py:165, encoder_impl.py:163-171, the
    ReLU-then-dropout of modules.py:87), encoder layer i with seed + 16 + 8 i."""
    seed = text_encoder_seed(step)
    out = {}
    if prenet:
        for i in range(3):
            out[f"{pre}pre.relu_drop.1:{i}"] = channel_mask(seed + i, word, rows, C, p_pre)
    for i in range(n_layers):
        out.update(encoder_layer_masks(seed + 16 + 8 * i, word, rows, i, B, T, C, F, n_heads, p, pre + "encoder."))
    return out


def duration_masks(seed, word, rows, F=256, p=0.1, pre="encoder.proj_w."):
    """models.DurationPredictor self.drop after norm_1 (seed + 0) and after norm_2 (seed + 1) (encoder_impl.py:217-223)."""
    return {f"{pre}drop:0": channel_mask(seed, word, rows, F, p), f"{pre}drop:1": channel_mask(seed + 1, word, rows, F, p)}


def dds_masks(seed, word, rows, C=192, n_layers=3, p=0.5, pre="convs."):
    """modules.DilatedDepthSeparableConv self.dropout of layer i with seed + i (predictors.py:78-98)."""
    return {f"{pre}dropout:{i}": channel_mask(seed + i, word, rows, C, p) for i in range(n_layers)}
