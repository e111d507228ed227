"""Host restatement of gt_synth_geometry (csrc/synth_front.hip): the ragged rows layout of the squeezed mel axis
from the predicted lengths and the two capacities, clipping included.  Plain Python, sequential — the rule as the header states it,
not the kernel's closed form: utterances in order, every one keeps its two halos, and one whose rows would pass R_cap keeps the
frames that still fit in front of the halos of the utterances behind it."""
HALO = 2
BIT_FRAMES, BIT_ROWS = 1, 2


def geometry(y_len, Ty_cap, R_cap):
    """-> dict(row0 [B + 1], len_sq [B], y_len_eff [B], status, rowbatch / rowframe / rowmask [R_cap])"""
    B = len(y_len)
    assert Ty_cap % 2 == 0 and R_cap >= 2 * HALO * B
    status = 0
    clipped = []
    for v in y_len:
        v = max(int(v), 0)
        if v > Ty_cap:
            status |= BIT_FRAMES
        clipped.append(min(v, Ty_cap))
    want = [v // 2 for v in clipped]
    if sum(w + 2 * HALO for w in want) > R_cap:
        status |= BIT_ROWS
    row0, len_sq, y_eff = [0], [], []
    for b in range(B):
        behind = 2 * HALO * (B - b - 1)                      # the halos of the utterances that follow
        room = R_cap - behind - row0[b] - 2 * HALO
        n = max(0, min(want[b], room))
        len_sq.append(n)
        y_eff.append(clipped[b] if n == want[b] else 2 * n)
        row0.append(row0[b] + n + 2 * HALO)
    row0[B] = R_cap                                          # the last utterance owns the spare rows
    rowbatch, rowframe, rowmask = [], [], []
    b = 0
    for m in range(R_cap):
        while b + 1 < B and row0[b + 1] <= m:
            b += 1
        t = m - row0[b] - HALO
        rowbatch.append(b)
        rowframe.append(t)
        rowmask.append(1.0 if 0 <= t < len_sq[b] else 0.0)
    return dict(row0=row0, len_sq=len_sq, y_len_eff=y_eff, status=status, rowbatch=rowbatch, rowframe=rowframe, rowmask=rowmask)
