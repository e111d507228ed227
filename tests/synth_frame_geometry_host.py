"""Host restatement of gt_synth_frame_geometry (csrc/synth_front.hip): the ragged rows layout of the UN-squeezed mel
axis — the frame rate the stochastic pitch / energy predictors run at — from the (frame-clipped) lengths and the row capacity,
clipping included.  Plain Python, sequential — the rule as the header states it, not the kernel's closed form: utterances in order,
every one keeps its two halos, and one whose rows would pass Rf_cap keeps the frames that still fit in front of the halos of the
utterances behind it.  tests/synth_geometry_host.py is the same rule on the squeezed axis."""
HALO = 2
BIT_FRAME_ROWS = 4


def frame_geometry(y_len_eff, Ty_cap, Rf_cap):
    """-> dict(row0 [B + 1], len_f [B], status (0 or bit 2), rowbatch / rowframe / rowmask [Rf_cap])"""
    B = len(y_len_eff)
    assert Rf_cap >= 2 * HALO * B
    want = [min(max(int(v), 0), Ty_cap) for v in y_len_eff]
    status = BIT_FRAME_ROWS if sum(w + 2 * HALO for w in want) > Rf_cap else 0
    row0, len_f = [0], []
    for b in range(B):
        behind = 2 * HALO * (B - b - 1)                      # the halos of the utterances that follow
        room = Rf_cap - behind - row0[b] - 2 * HALO
        n = max(0, min(want[b], room))
        len_f.append(n)
        row0.append(row0[b] + n + 2 * HALO)
    row0[B] = Rf_cap                                         # the last utterance owns the spare rows
    rowbatch, rowframe, rowmask = [], [], []
    b = 0
    for m in range(Rf_cap):
        while b + 1 < B and row0[b + 1] <= m:
            b += 1
        t = m - row0[b] - HALO
        rowbatch.append(b)
        rowframe.append(t)
        rowmask.append(1.0 if 0 <= t < len_f[b] else 0.0)
    return dict(row0=row0, len_f=len_f, status=status, rowbatch=rowbatch, rowframe=rowframe, rowmask=rowmask)
