"""TEST INFRASTRUCTURE ONLY — the shapes, operands and planted defects that tests/test_loss64.py (float32 twin, CPU) and
tests/test_loss_kernels_fp64_gpu.py (the kernels) both run, so that a bound validated on the twin is the bound the kernel meets.
Every operand is float32-representable and built from a seed that depends on the shape only."""
import torch

from . import loss64 as L64

F32 = torch.float32


def gen(*key):
    return torch.Generator().manual_seed(int(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31)))


# ----------------------------------------------------------------------------- gt_logp_f32
LOGP_SHAPES = [(1, 6, 1, 1), (2, 160, 32, 128), (2, 160, 33, 129), (2, 18, 45, 161), (3, 80, 5, 257)]


def logp_case(shape, with_logs):
    """x_m randn, x_logs randn * 0.7 clamped to +-2 (or None), z randn * 1.5; distinct data per batch"""
    B, C, Tx, Ty = shape
    g = gen(*shape)
    x_m = torch.randn(B, C, Tx, generator=g)
    x_logs = (torch.randn(B, C, Tx, generator=g) * 0.7).clamp_(-2, 2)
    z = torch.randn(B, C, Ty, generator=g) * 1.5
    return x_m, (x_logs if with_logs else None), z


def logp_defects(shape, with_logs):
    B, C, Tx, Ty = shape
    return (["drop_channel"] + (["stale_column"] if Ty >= 2 else []) + (["batch_logs"] if B >= 2 and with_logs else [])
            + (["row_swap"] if Tx >= 5 else []))


# ----------------------------------------------------------------------------- gt_mle_sums / _finish / _bwd
def mle_trip():
    """elements one grid-stride trip of gt_mle_sums covers"""
    return 4 * L64.header_constant("GT_MLE_PARTS") * 256


def mle_ns():
    return [7, 17763, 2 * L64.header_constant("GT_MLE_PARTS") * 1024 + 3]      # the last: a second trip + the scalar tail


MLE_B = [2, 1500]


def mle_case(n, B):
    g = gen(n, B)
    z = torch.randn(n, generator=g)
    m = torch.randn(n, generator=g) * 0.5
    logs = (torch.randn(n, generator=g) * 0.5).clamp_(-2, 2)
    logdet = torch.randn(B, generator=g) * 3
    n_mask = 5 if n < 1000 else 1501                                          # % 4 == 1: gt_mle_finish's scalar tail runs
    mask = (torch.rand(n_mask, generator=g) < 0.7).to(F32)
    mask[0] = mask[-1] = 1
    C = max(1, n // int(mask.sum()))                                          # denom = C sum(mask) ~ n, as in a training step
    return z, m, logs, logdet, mask, C


def mle_probe_indices(n):
    """0, 3, 4, the last element of trip one, the first of trip two, 4 (n / 4) - 1, 4 (n / 4), n - 1 — those that exist"""
    t = mle_trip()
    cand = [0, 3, 4, t - 1, t, 4 * (n // 4) - 1, 4 * (n // 4), n - 1]
    return sorted({i for i in cand if 0 <= i < n})


def mle_bwd_ns():
    return [5, L64.header_constant("GT_MLE_PARTS") * 256 + 5]                # the second: 5 elements on a second grid-stride trip


MLE_BWD_B = [1, 300]


def mle_bwd_case(n):
    g = gen(n, 3)
    z = torch.randn(n, generator=g)
    m = torch.randn(n, generator=g) * 0.5
    logs = (torch.randn(n, generator=g) * 0.5).clamp_(-2, 2)
    return z, m, logs, torch.tensor([1.7]), torch.tensor([5120.0])           # gscale, gdenom


# ----------------------------------------------------------------------------- gt_duration_loss_fwd / _bwd
DUR_SHAPES = [(B, Tx) for B in (1, 3, 70) for Tx in (1, 64, 65, 150)]


def dur_case(B, Tx):
    """lengths include 1 and Tx (where B allows); w: integer durations 0 .. 5 with zeros on valid tokens, junk on padded ones;
    logw zero on padded tokens"""
    g = gen(B, Tx, 5)
    pool = [Tx, 1, max(1, Tx // 2), max(1, Tx - 1)]
    lens = torch.tensor([pool[b % 4] for b in range(B)], dtype=torch.int32)
    on = torch.arange(Tx)[None, :] < lens[:, None]
    w = torch.randint(0, 6, (B, Tx), generator=g).to(F32)
    w[:, 0] = 0                                                              # a valid token with no frame in every utterance
    junk = torch.where(torch.arange(Tx)[None, :] % 2 == 0, torch.tensor(-3.0), torch.tensor(1e30)).expand(B, Tx)
    w = torch.where(on, w, junk)
    logw = torch.randn(B, Tx, generator=g) * on
    gr = torch.randn(B, generator=g)
    return logw, w, lens, gr


# __logf is outside the rule: rel-L2 err_kernel <= max(M err_twin, 2^-23), both against float64 (the protocol of
# tests/test_wn_boundary_fp64_gpu.py).  M: twice the worst err_kernel / err_twin measured on an MI355X, rounded up.
DUR_M = {"fwd": 2, "bwd": 2}


def rel_l2(a, b):
    """|| a - b || / || b || in float64; inf when either holds a non-finite value (a planted log 0)"""
    a, b = a.double(), b.double()
    if not (torch.isfinite(a).all() and torch.isfinite(b).all()):
        return float("inf")
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def dur_defects(B, Tx):
    return ["no_eps"] + (["lens_b"] if B > 1 else [])


# ----------------------------------------------------------------------------- gt_prior_expand / _bwd
PRIOR_SHAPES = [(1, 1), (3, 200), (150, 447), (512, 640), (513, 640)]      # 512: the last Tx of acc[4][512]; 513: the first in dynamic LDS
PRIOR_B, PRIOR_C = 2, 3                                                      # B C = 6: the last workgroup of 4 waves holds 2


def _runs(Tx, Ty, head, tail, g):
    """frame2token of one utterance: the (token, frames) runs of `head`, then the remaining frames but `tail` spread over a random
    subset of the remaining tokens (dropped tokens are jumps of 2 or more), then `tail` frames of -1"""
    f2t = []
    for tok, n in head:
        f2t += [tok] * n
    nxt = head[-1][0] + 2 if head else 0                                      # a jump of 2 right after the head
    left = Ty - tail - len(f2t)
    toks = list(range(nxt, Tx))
    if left > 0 and toks:
        k = min(len(toks), left)
        pick = sorted(torch.randperm(len(toks), generator=g)[:k].tolist())
        dur = torch.ones(k, dtype=torch.int64)
        dur += torch.bincount(torch.randint(0, k, (left - k,), generator=g), minlength=k)
        for p, d in zip(pick, dur.tolist()):
            f2t += [toks[p]] * d
    f2t += [-1] * (Ty - len(f2t))
    return f2t


def prior_maps(Tx, Ty):
    """Hand-built monotone maps [2, Ty], different per utterance: a run that ends exactly on lane 63, one token spanning three
    64-frame chunks, tokens with no frame, a -1 tail, Ty % 64 != 0 (but for 640)."""
    g = gen(Tx, Ty, 11)
    if (Tx, Ty) == (1, 1):
        maps = [[0], [-1]]
    elif (Tx, Ty) == (3, 200):
        maps = [[0] * 64 + [1] * 132 + [-1] * 4,                              # token 0 ends on lane 63, token 1 covers chunks 1, 2, 3
                [0] * 10 + [2] * 141 + [-1] * 49]                             # token 1 has no frame; token 2 covers chunks 0, 1, 2
    else:
        maps = [_runs(Tx, Ty, [(0, 64), (1, 1), (2, 140)], 17, g),            # ends on lane 63; frames 65 .. 204: chunks 1, 2, 3
                _runs(Tx, Ty, [(0, 30), (2, 98), (3, 70)], 0 if Ty % 64 == 0 else 5, g)]   # token 2 ends on frame 127; 128 .. 197: chunks 2, 3
    f2t = torch.tensor(maps, dtype=torch.int32)
    assert f2t.shape == (2, Ty) and int(f2t.max()) < Tx
    for row in f2t.tolist():                                                  # monotone on the valid part, -1 only as a tail
        v = [t for t in row if t >= 0]
        assert v == sorted(v) and row[:len(v)] == v
    return f2t


def prior_case(Tx, Ty):
    g = gen(Tx, Ty, 13)
    return (torch.randn(PRIOR_B, PRIOR_C, Tx, generator=g), prior_maps(Tx, Ty), torch.randn(PRIOR_B, PRIOR_C, Ty, generator=g))


def prior_defects(Tx, Ty):
    return ["second_chunk"] if Ty > 64 else []


# ----------------------------------------------------------------------------- gt_embedding_fwd / _bwd
EMB_DIMS = [(192, 192), (188, 192)]                                           # (channels, row stride)
EMB_SCALE = 192 ** 0.5


def emb_case(ragged, Ce, bwd):
    """forward: vocabulary 11, lengths [5, 1, 9, 3]; backward: vocabulary 5, T = 150 (heavy duplicates).  The padded positions of
    ids hold valid ids that differ from the real ones'."""
    V, lens, T = (5, [150, 1, 77], 150) if bwd else (11, [5, 1, 9, 3], 9)
    g = gen(int(ragged), Ce, int(bwd))
    lay = L64.Layout(lens, T, ragged, rnd=8)
    ids = torch.randint(0, V, (len(lens), T), generator=g)
    on = torch.arange(T)[None, :] < torch.tensor(lens)[:, None]
    ids = torch.where(on, ids, (ids + 1) % V)
    emb = torch.randn(V, Ce, generator=g)
    return lay, ids, emb, V


# ----------------------------------------------------------------------------- gt_rows_add_cond / gt_rows_utt_sum / gt_length_mask
ROWS_LENS, ROWS_T = [1, 64, 65], 65
ROWS_DIMS = [(8, 8), (192, 192), (256, 320)]                                  # (channels, output stride)
LENGTH_MASK_SHAPES = [(3, 67), (5, 123)]                                      # B T = 201, 615: no multiple of 256


def rows_case(ragged, C):
    g = gen(int(ragged), C, 17)
    lay = L64.Layout(ROWS_LENS, ROWS_T, ragged, rnd=8)
    x = torch.randn(lay.R, C, generator=g)
    cond = torch.randn(len(ROWS_LENS), C, generator=g)
    prior = torch.randn(len(ROWS_LENS), C, generator=g) * 3
    return lay, x, cond, prior


# ----------------------------------------------------------------------------- layout kernels
BCT_LENS, BCT_T = [37, 1, 2, 60, 13], 61                                      # ragged: 136 rows, uniform: 325; neither a multiple of 64
BCT_C = [1, 65, 80, 192]
SQZ_C, SQZ_TY = [1, 80], [1, 2, 63, 64, 121]


def sqz_case(C, Ty, ragged):
    """three utterances: full length, len_sq below Ty / 2, len_sq = 1 (0 frames where Ty < 2: then len_sq[b] > Ty / 2 is refused by
    the kernels' own `t' < Ty / 2`)"""
    T2 = max(Ty // 2, 1)
    len_sq = [T2, max(T2 // 2, 0), 1]
    lay = L64.Layout([min(v, Ty // 2) for v in len_sq], T2, ragged, rnd=8)
    g = gen(C, Ty, int(ragged))
    return lay, len_sq, torch.randn(3, C, Ty, generator=g), torch.randn(lay.R, 2 * C, generator=g)

