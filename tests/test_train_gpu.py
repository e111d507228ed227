"""GPU tests of the training step plumbing: flat AdamW (gt_adamw_flat) against torch.optim.AdamW, the
OneCycleLR restatement against torch's scheduler, and the graph-captured step against the eager one."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def test_flat_adamw_matches_torch(built):
    from glow_tts_amd import ops, train
    torch.manual_seed(0)
    shapes = [(7, 5), (3,), (11, 2, 3), (1,), (64, 33), (192, 192, 5)]
    ref = [torch.nn.Parameter(torch.randn(s, device=dev())) for s in shapes]
    mine = [torch.nn.Parameter(p.detach().clone()) for p in ref]
    lr, betas, eps = 2e-3, (0.9, 0.98), 1e-9
    opt_ref = torch.optim.AdamW(ref, lr=lr, betas=betas, eps=eps)
    gb = train.GradBuckets(mine, world=1)
    opt = train.FlatAdamW(gb, lr, betas, eps)
    for it in range(4):
        gs = [torch.randn(s, device=dev()) * (it + 1) for s in shapes]
        skip = 2            # a parameter that never gets a gradient is left untouched (torch skips grad-None parameters too;
                            # the step count of the bias correction is global here, per parameter in torch)
        for i, (p, q, g) in enumerate(zip(ref, mine, gs)):
            p.grad = None if i == skip else g.clone()
            q.grad = None if i == skip else g.clone()
        opt_ref.step()
        ops.arena_begin(dev())
        gb.reduce_all()
        gn = torch.sqrt(opt.step()).item()
        ops.arena_end(dev())
        want_gn = math.sqrt(sum(g.double().pow(2).sum().item() for i, g in enumerate(gs) if i != skip))
        assert abs(gn - want_gn) <= 1e-4 * want_gn
        for p, q in zip(ref, mine):
            assert torch.allclose(p, q, rtol=1e-5, atol=1e-6), (it, (p - q).abs().max().item())


def test_one_cycle_matches_torch_scheduler():
    from glow_tts_amd import train
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.AdamW([p], lr=2e-4, betas=(0.9, 0.98))
    total = 57
    sch = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=2e-4, total_steps=total)
    for step in range(total):
        lr, b1 = train.one_cycle(step, total, 2e-4)
        assert abs(lr - opt.param_groups[0]["lr"]) <= 1e-9 + 1e-6 * lr, step
        assert abs(b1 - opt.param_groups[0]["betas"][0]) <= 1e-6, step
        opt.step()
        if step < total - 1:
            sch.step()


def test_graph_step_matches_eager_step(built):
    """Same model, same batch, dropout off: the captured-graph step and the eager step give the same losses
    and the same parameters after two updates (the graph only removes launch gaps)."""
    from glow_tts_amd import train
    cfg = dict(train.BASE_MODEL, n_blocks_dec=2, n_layers_enc=1, p_dropout=0.0, p_dropout_dec=0.0)
    torch.manual_seed(0)
    m1 = train.build_model(cfg, device=dev())
    with torch.no_grad():                                     # the zero-initialised convs would hide most of the path
        for n, p in m1.named_parameters():
            if n.endswith("end.weight") or n.endswith("pre.proj.weight"):
                p.normal_(0, 0.02)
    m1.encoder.pre.p_dropout = 0.0                            # the prenet's dropout is a hard-coded 0.5 (models.py:674)
    m2 = train.build_model(cfg, device=dev())
    m2.load_state_dict(m1.state_dict())
    m2.encoder.pre.p_dropout = 0.0
    batch = train.synth_batch(4, 40, 120, 0, dev())
    t1, t2 = train.Trainer(m1, graph=False), train.Trainer(m2, graph=True)
    for _ in range(3):                 # a first-seen graph key is side-effect free: one update per step() on both trainers
        l1, _ = t1.step(*batch)
        l2, _ = t2.step(*batch)
    torch.cuda.synchronize()
    assert t2.graph_mode and t2.n_captures == 1 and t2.adam_steps == t2.n_steps == 3 and t1.adam_steps == 3
    assert math.isfinite(l1.item()) and abs(l2.item() - l1.item()) <= 2e-2 * max(1.0, abs(l1.item())), (l2.item(), l1.item())
    worst = max((a - b).abs().max().item() for a, b in zip(m1.parameters(), m2.parameters()))
    assert worst < 5e-3, worst


def test_graph_replay_follows_new_batches_of_the_same_row_bucket(built):
    """Ragged rows under graphs: ONE captured graph serves different batches whose rounded row counts agree — a replay
    only refreshes the row offsets / masks.  Same updates as the eager trainer on the same batch sequence."""
    from glow_tts_amd import ops, train
    cfg = dict(train.BASE_MODEL, n_blocks_dec=2, n_layers_enc=1, p_dropout=0.0, p_dropout_dec=0.0)
    torch.manual_seed(0)
    m1 = train.build_model(cfg, device=dev())
    with torch.no_grad():
        for n, p in m1.named_parameters():
            if n.endswith("end.weight") or n.endswith("pre.proj.weight"):
                p.normal_(0, 0.02)
    m1.encoder.pre.p_dropout = 0.0
    m2 = train.build_model(cfg, device=dev())
    m2.load_state_dict(m1.state_dict())
    m2.encoder.pre.p_dropout = 0.0
    bA, bB = train.synth_batch(4, 40, 120, 0, dev()), train.synth_batch(4, 40, 120, 7, dev())
    assert bA[1].tolist() != bB[1].tolist() and bA[3].tolist() != bB[3].tolist()
    te, tg = train.Trainer(m1, graph=False), train.Trainer(m2, graph=True)
    te.cfg.row_round = tg.cfg.row_round = 1024              # both batches fall into one bucket
    seq = [bA, bB, bA, bB, bB]
    for b in seq:
        le, _ = te.step(*b)
        lg, _ = tg.step(*b)
    torch.cuda.synchronize()
    assert len(tg._captured) == 1 and tg.n_captures == 1 and tg.adam_steps == len(seq)
    assert abs(le.item() - lg.item()) <= 2e-2 * max(1.0, abs(le.item())), (le.item(), lg.item())
    worst = max((a - b).abs().max().item() for a, b in zip(m1.parameters(), m2.parameters()))
    assert worst < 5e-3, worst


@pytest.mark.parametrize("graph", [False, True])
def test_phased_backward_matches_single_backward(built, graph):
    """The data-parallel form of the step (backward in two calls — everything but the text encoder, then the text
    encoder — with the decoder's gradient slice handed to the collective in between; three graphs when captured) gives
    the same updates as the single-backward step.  world = 1: the collectives are no-ops, the phasing is what is tested."""
    from glow_tts_amd import train
    cfg = dict(train.BASE_MODEL, n_blocks_dec=2, n_layers_enc=1, p_dropout=0.0, p_dropout_dec=0.0)
    torch.manual_seed(0)
    m1 = train.build_model(cfg, device=dev())
    with torch.no_grad():
        for n, p in m1.named_parameters():
            if n.endswith("end.weight") or n.endswith("pre.proj.weight"):
                p.normal_(0, 0.02)
    m1.encoder.pre.p_dropout = 0.0
    m2 = train.build_model(cfg, device=dev())
    m2.load_state_dict(m1.state_dict())
    m2.encoder.pre.p_dropout = 0.0
    batch = train.synth_batch(4, 40, 120, 0, dev())
    lh = (batch[1].tolist(), batch[3].tolist())
    t1 = train.Trainer(m1, graph=False, split_graph=False)
    t2 = train.Trainer(m2, graph=graph, split_graph=True)
    assert 0 < t2.dec0 < len(t2.buckets.params) and t2.dec0_off % 64 == 0
    for _ in range(3):
        l1, _ = t1.step(*batch, lengths_host=lh)
        l2, _ = t2.step(*batch, lengths_host=lh)
    torch.cuda.synchronize()
    if graph:
        assert len(next(iter(t2._captured.values()))[0]) == 3
    assert abs(l1.item() - l2.item()) <= 2e-2 * max(1.0, abs(l1.item())), (l1.item(), l2.item())
    worst = max((a - b).abs().max().item() for a, b in zip(m1.parameters(), m2.parameters()))
    assert worst < 5e-3, worst


def test_trainer_gradients_match_plain_autograd(built):
    """Under a Trainer the atomically accumulated gradients (LayerNorm, ActNorm, InvConvNear, relative-position and
    token embeddings) are written straight into their slices of the flat gradient buffer (ops.grad_accumulator), the
    region being cleared once per step; the rest arrives from the batched wgrad kernels.  Same numbers as the model run
    by plain autograd without a Trainer, step after step (nothing left over from the previous step), and no copy is
    needed for the accumulated ones."""
    from glow_tts_amd import models, ops, train
    cfg = dict(train.BASE_MODEL, n_blocks_dec=2, n_layers_enc=1, p_dropout=0.0, p_dropout_dec=0.0)
    torch.manual_seed(0)
    m1 = train.build_model(cfg, device=dev())
    with torch.no_grad():
        for n, p in m1.named_parameters():
            if n.endswith("end.weight") or n.endswith("pre.proj.weight"):
                p.normal_(0, 0.02)
    m1.encoder.pre.p_dropout = 0.0
    m2 = train.build_model(cfg, device=dev())
    m2.load_state_dict(m1.state_dict())
    m2.encoder.pre.p_dropout = 0.0
    tr = train.Trainer(m2, graph=False)
    gb = tr.buckets
    assert gb.n_accum > 0 and all(p._gt_prezeroed for p in gb.params[:gb.n_accum])
    copied = []
    real = torch._foreach_copy_
    for seed in (0, 7):
        ids, t_x, y, t_y = train.synth_batch(4, 40, 120, seed, dev())
        for p in m1.parameters():
            p.grad = None
        (z, z_m, z_logs, logdet, z_mask), _, (attn, l_length, _, _), _, _ = m1(ids, t_x, y, t_y)
        (models.mle_loss(z, z_m, None, logdet, z_mask) + l_length.sum()).backward()
        want = {n: (None if p.grad is None else p.grad.clone()) for n, p in m1.named_parameters()}
        torch._foreach_copy_ = lambda d, s: (copied.append([t.data_ptr() for t in d]), real(d, s))[1]
        try:
            tr._fwd_bwd(ids, t_x, y, t_y)
        finally:
            torch._foreach_copy_ = real
            ops.arena_end(dev())                 # the step's zero arena is normally closed by Trainer._optim
        head = {gb.view(i).data_ptr() for i in range(gb.n_accum)}
        assert not (head & {q for c in copied for q in c}), "accumulated gradients were copied into the flat buffer"
        for (n, p), q in zip(m1.named_parameters(), m2.parameters()):
            ref = want[n]
            if ref is None:
                assert q.grad is None or q.grad.abs().max().item() == 0, n
                continue
            err = (q.grad - ref).abs().max().item()
            assert err <= 1e-3 * max(1e-6, ref.abs().max().item()) + 1e-6, (seed, n, err)   # atomics: order of the sums differs


def test_speaker_conditioned_graph_step_matches_eager(built):
    """cfg 4 form of the step (gin_channels=256, speaker vectors g [b,256,1] as a fifth static input of the graph):
    captured and eager trainers give the same updates, and the conditioning parameters (Encoder.cond_g,
    DurationPredictor.cond, every WN.cond_layer) do get updated."""
    from glow_tts_amd import train
    cfg = dict(train.BASE_MODEL, n_blocks_dec=2, n_layers_enc=3, p_dropout=0.0, p_dropout_dec=0.0, gin_channels=256)
    torch.manual_seed(0)
    m1 = train.build_model(cfg, device=dev())
    with torch.no_grad():
        for n, p in m1.named_parameters():
            if n.endswith("end.weight") or n.endswith("pre.proj.weight"):
                p.normal_(0, 0.02)
    m1.encoder.pre.p_dropout = 0.0
    m2 = train.build_model(cfg, device=dev())
    m2.load_state_dict(m1.state_dict())
    m2.encoder.pre.p_dropout = 0.0
    before = {n: p.detach().clone() for n, p in m1.named_parameters()}
    batch = train.synth_batch(4, 40, 120, 0, dev())
    spk = torch.randn(4, 256, 1, device=dev())
    lh = (batch[1].tolist(), batch[3].tolist())
    t1, t2 = train.Trainer(m1, graph=False), train.Trainer(m2, graph=True)
    for _ in range(2):
        l1, _ = t1.step(*batch, lengths_host=lh, g=spk)
        l2, _ = t2.step(*batch, lengths_host=lh, g=spk)
    torch.cuda.synchronize()
    assert t2.graph_mode and len(t2._captured) == 1
    assert math.isfinite(l1.item()) and abs(l1.item() - l2.item()) <= 2e-2 * max(1.0, abs(l1.item())), (l1.item(), l2.item())
    worst = max((a - b).abs().max().item() for a, b in zip(m1.parameters(), m2.parameters()))
    assert worst < 5e-3, worst
    moved = {n for n, p in m1.named_parameters() if (p.detach() - before[n]).abs().max().item() > 0}
    for key in ("encoder.encoder.cond_g.weight", "encoder.proj_w.cond.weight", "decoder.flows.2.wn.cond_layer.weight_v",
                "decoder.flows.5.wn.cond_layer.bias"):
        assert key in moved, key


def test_prosody_conditioned_graph_step_matches_eager(built):
    """cfg 5's decoder inputs through the trainer: g, pitch and energy are static inputs of the captured graph; the
    captured and the eager step give the same updates and the WNP parameters (cond_layer1 included) move."""
    from glow_tts_amd import train
    cfg = dict(train.BASE_MODEL, n_blocks_dec=2, n_layers_enc=3, p_dropout=0.0, p_dropout_dec=0.0, gin_channels=512,
               with_prosody_wn=True)
    torch.manual_seed(0)
    m1 = train.build_model(cfg, device=dev())
    with torch.no_grad():
        for n, p in m1.named_parameters():
            if n.endswith("end.weight") or n.endswith("pre.proj.weight"):
                p.normal_(0, 0.02)
    m1.encoder.pre.p_dropout = 0.0
    m2 = train.build_model(cfg, device=dev())
    m2.load_state_dict(m1.state_dict())
    m2.encoder.pre.p_dropout = 0.0
    before = {n: p.detach().clone() for n, p in m1.named_parameters()}
    batch = train.synth_batch(4, 40, 120, 0, dev())
    spk = torch.randn(4, 512, 1, device=dev())
    pitch = (80 + 200 * torch.rand(4, 1, 120, device=dev())) * (torch.rand(4, 1, 120, device=dev()) > 0.3)
    energy = 1 + 10 * torch.rand(4, 1, 120, device=dev())
    lh = (batch[1].tolist(), batch[3].tolist())
    t1, t2 = train.Trainer(m1, graph=False), train.Trainer(m2, graph=True)
    for _ in range(2):
        l1, _ = t1.step(*batch, lengths_host=lh, g=spk, pitch=pitch, energy=energy)
        l2, _ = t2.step(*batch, lengths_host=lh, g=spk, pitch=pitch, energy=energy)
    torch.cuda.synchronize()
    assert t2.graph_mode and len(t2._captured) == 1
    assert math.isfinite(l1.item()) and abs(l1.item() - l2.item()) <= 2e-2 * max(1.0, abs(l1.item())), (l1.item(), l2.item())
    worst = max((a - b).abs().max().item() for a, b in zip(m1.parameters(), m2.parameters()))
    assert worst < 5e-3, worst
    moved = {n for n, p in m1.named_parameters() if (p.detach() - before[n]).abs().max().item() > 0}
    for key in ("decoder.flows.2.wn_pitch.cond_layer1.weight_g", "decoder.flows.5.wn_energy.cond_layer1.bias",
                "decoder.flows.2.wn_energy.in_layers.0.weight_v", "decoder.flows.5.wn_pitch.res_skip_layers.3.bias"):
        assert key in moved, key


def test_failed_capture_falls_back_to_eager_steps(built, monkeypatch):
    """If the step cannot be captured (e.g. a collective that refuses capture), the trainer warns and keeps training with
    eager launches — same updates as a trainer that never tried.  The real _capture runs (warm-ups, snapshot / restore, the open
    wgrad.capture_scope) and fails at graph CONSTRUCTION, before any capture begins, with the host state a capture leaves when it
    aborts between the decoder's flush and the optimizer; Trainer._abandon_capture must unwind all of it."""
    import warnings
    from glow_tts_amd import devstate, ops, train, wgrad
    cfg = dict(train.BASE_MODEL, n_blocks_dec=1, n_layers_enc=1, p_dropout=0.0, p_dropout_dec=0.0)
    torch.manual_seed(0)
    m1 = train.build_model(cfg, device=dev())
    m1.encoder.pre.p_dropout = 0.0
    m2 = train.build_model(cfg, device=dev())
    m2.load_state_dict(m1.state_dict())
    m2.encoder.pre.p_dropout = 0.0
    batch = train.synth_batch(4, 40, 120, 0, dev())
    lh = (batch[1].tolist(), batch[3].tolist())
    t1, t2 = train.Trainer(m1, graph=False), train.Trainer(m2, graph=True)

    front0, seed0 = devstate.get(dev()).stream("front"), ops.seed_word(dev())

    def boom(*a, **k):
        t2.opt._early = (t2.dec_cov_off, t2.buckets.total)
        t2._tail_packed = True
        raise RuntimeError("capture refused")
    monkeypatch.setattr(torch.cuda, "CUDAGraph", boom)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        for _ in range(2):
            l1, _ = t1.step(*batch, lengths_host=lh)
            l2, _ = t2.step(*batch, lengths_host=lh)
    torch.cuda.synchronize()
    assert not t2.graph_mode and any("capture of the training step failed" in str(x.message) for x in w)
    assert t2.adam_steps == t2.n_steps == 2
    assert t2.opt._early is None
    assert not wgrad.capture_keep(torch.empty(1))                    # no capture scope is left open
    assert devstate.get(dev()).stream("front") is not front0         # every auxiliary stream was dropped, the front end's included
    assert ops.seed_word(dev()) is seed0                             # ... and nothing a captured graph has the address of
    assert abs(l1.item() - l2.item()) <= 1e-3 * max(1.0, abs(l1.item()))
    worst = max((a - b).abs().max().item() for a, b in zip(m1.parameters(), m2.parameters()))
    assert worst < 5e-3, worst


def test_graph_trainer_alternates_between_row_buckets(built):
    """A stream of batches over several row buckets (and two padded shapes): one captured graph per key, replays alternate in
    any order, and the graph trainer equals the eager trainer on the SAME sequence with the SAME number of updates — a
    first-seen key costs no extra optimizer steps (VERDICT r1 / ADVICE r1: it used to cost four)."""
    from glow_tts_amd import train
    cfg = dict(train.BASE_MODEL, n_blocks_dec=2, n_layers_enc=1, p_dropout=0.0, p_dropout_dec=0.0)
    torch.manual_seed(0)
    m1 = train.build_model(cfg, device=dev())
    with torch.no_grad():
        for n, p in m1.named_parameters():
            if n.endswith("end.weight") or n.endswith("pre.proj.weight"):
                p.normal_(0, 0.02)
    m1.encoder.pre.p_dropout = 0.0
    m2 = train.build_model(cfg, device=dev())
    m2.load_state_dict(m1.state_dict())
    m2.encoder.pre.p_dropout = 0.0
    bA, bC = train.synth_batch(4, 40, 120, 0, dev()), train.synth_batch(4, 40, 120, 3, dev())
    bD = train.synth_batch(4, 37, 100, 5, dev())            # other padded shapes: (48, 128) vs (48, 128)? -> see assert below
    te, tg = train.Trainer(m1, graph=False, total_steps=40), train.Trainer(m2, graph=True, total_steps=40, max_graphs=2)
    te.cfg.row_round = tg.cfg.row_round = 32                # small buckets: the batches land in different ones
    lh = lambda b: (b[1].tolist(), b[3].tolist())           # noqa: E731
    assert tg._rows_key(48, 128, lh(bA)) != tg._rows_key(48, 128, lh(bC))
    seq = [bA, bC, bA, bD, bC, bA, bA, bD, bC]
    for b in seq:
        le, _ = te.step(*b, lengths_host=lh(b))
        lg, _ = tg.step(*b, lengths_host=lh(b))
    torch.cuda.synchronize()
    assert tg.graph_mode and len(tg._captured) == 2         # LRU: three keys seen, two kept
    assert tg.n_captures >= 3
    assert tg.adam_steps == tg.n_steps == len(seq) == te.adam_steps
    assert abs(le.item() - lg.item()) <= 2e-2 * max(1.0, abs(le.item())), (le.item(), lg.item())
    worst = max((a - b).abs().max().item() for a, b in zip(m1.parameters(), m2.parameters()))
    assert worst < 5e-3, worst


def test_two_trainers_in_one_process_do_not_interfere(built):
    """Rows-layout state lives on the model (ops.RowsConfig), not in module globals: a ragged graph trainer and a uniform
    eager trainer (and a plain evaluation forward of a third model) interleaved in one process give what each gives alone."""
    from glow_tts_amd import models, train
    cfg = dict(train.BASE_MODEL, n_blocks_dec=1, n_layers_enc=1, p_dropout=0.0, p_dropout_dec=0.0)

    def make():
        torch.manual_seed(0)
        m = train.build_model(cfg, device=dev())
        with torch.no_grad():
            for n, p in m.named_parameters():
                if n.endswith("end.weight") or n.endswith("pre.proj.weight"):
                    p.normal_(0, 0.02)
        m.encoder.pre.p_dropout = 0.0
        return m
    batch = train.synth_batch(4, 40, 120, 0, dev())
    lh = (batch[1].tolist(), batch[3].tolist())
    ref_a, ref_b = make(), make()
    ta, tb = train.Trainer(ref_a, graph=True), train.Trainer(ref_b, graph=False, ragged=False)
    for _ in range(2):
        ta.step(*batch, lengths_host=lh)
    for _ in range(2):
        tb.step(*batch, lengths_host=lh)
    ma, mb, mc = make(), make(), make().eval()
    xa, xb = train.Trainer(ma, graph=True), train.Trainer(mb, graph=False, ragged=False)
    assert ma.rows_cfg.ragged and not mb.rows_cfg.ragged and not mc.rows_cfg.ragged
    for _ in range(2):
        xa.step(*batch, lengths_host=lh)
        with torch.no_grad():
            (z, _, _, logdet, _), _, _, _, _ = mc(*batch)
        xb.step(*batch, lengths_host=lh)
    torch.cuda.synchronize()
    assert torch.isfinite(z).all() and torch.isfinite(logdet).all()
    for got, want in ((ma, ref_a), (mb, ref_b)):
        worst = max((a - b).abs().max().item() for a, b in zip(got.parameters(), want.parameters()))
        assert worst < 1e-5, worst


def test_wgrad_workspace_outgrown_by_a_later_capture_lives_as_long_as_its_graphs(built):
    """The partial-sum workspace of the batched weight-gradient launches is shared by every captured step of a stream, and a
    captured step has its address baked in.  When a later row bucket needs a bigger one, the outgrown buffer must not go back to
    the allocator while an older graph can still replay into it (cfg 3 faulted with 'write access to a read-only page' when it
    did) — and must go once those graphs are gone (round 2 kept every outgrown buffer for ever).  The capture that used
    a buffer holds the reference (wgrad.CaptureKeep)."""
    import gc
    import weakref
    from glow_tts_amd import wgrad
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a = wgrad._scratch(dev(), 1 << 20)
        pa, wa = a.data_ptr(), weakref.ref(a)
        assert wgrad._scratch(dev(), 1 << 19).data_ptr() == pa           # big enough: reused
        with wgrad.capture_scope(dev()) as keep:                         # "a capture is open": whoever asks for scratch now registers it
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                assert wgrad._scratch(dev(), 1 << 19).data_ptr() == pa
                _ = torch.ones(4, device=dev()) * 2.0                    # (a graph with a node in it)
        assert any(t.data_ptr() == pa for t in keep if isinstance(t, torch.Tensor))
        b = wgrad._scratch(dev(), 8 << 20)                               # a later bucket outgrows it
        assert b.numel() >= (8 << 20) and b.data_ptr() != pa
        del a
        gc.collect()
        assert wa() is not None                                          # the first capture still owns the old buffer
        keep.release(); del keep, g
        gc.collect()
        assert wa() is None                                              # ... and it is gone with that capture


def test_evicting_captured_graphs_releases_what_they_pinned(built):
    """More graph keys than max_graphs: the trainer's memory stays bounded — evicted keys give back their pinned staging buffers
    (wgrad._POOL) and drop their table arenas (every capture used to leak 8 MB of device memory + its pinned buffers)."""
    import gc
    from glow_tts_amd import train, wgrad
    cfg = dict(train.BASE_MODEL, n_blocks_dec=1, n_layers_enc=1, p_dropout=0.0, p_dropout_dec=0.0)
    torch.manual_seed(0)
    m = train.build_model(cfg, device=dev())
    tr = train.Trainer(m, graph=True, max_graphs=2, capture_after=1)
    tr.cfg.row_round = 32
    shapes = [(40, 120), (37, 100), (44, 140), (33, 90), (48, 150), (29, 80)]
    mem, pool = [], []
    for rnd in range(2):
        for i, (tx, ty) in enumerate(shapes):
            b = train.synth_batch(4, tx, ty, i, dev())
            tr.step(*b, lengths_host=(b[1].tolist(), b[3].tolist()))
            torch.cuda.synchronize(); gc.collect()
            mem.append(torch.cuda.memory_allocated()); pool.append(len(wgrad._POOL))
    assert tr.n_captures >= 10 and len(tr._captured) == 2
    assert not getattr(m, "_wgrad_keep", None) and not getattr(m.decoder, "_wgrad_keep", None)     # nothing hangs on the modules any more
    # the second pass over the shapes re-captures everything: allocated memory and the pinned pool must not keep growing
    first, second = mem[len(shapes) - 1], mem[-1]
    assert second <= first + (32 << 20), (first, second)
    assert min(pool[len(shapes):]) >= min(pool[:len(shapes)]) - 8, pool
    st = tr.capture_stats()
    assert st["captures"] == tr.n_captures and st["replays"] == len(mem) and st["resident"] == 2


def test_actnorm_ddi_survives_the_first_graph_step(built):
    """ActNorm.set_ddi(True) + a graph trainer: the data-dependent init runs as a forward-only pass BEFORE the first
    step (the reference's init.py:17-23), outside the capture's snapshot / restore — the parameters it writes must still be there
    after the step, equal (up to that step's own update) to what a plain no-grad forward of the same batch computes."""
    from glow_tts_amd import train
    cfg = dict(train.BASE_MODEL, n_blocks_dec=2, n_layers_enc=1, p_dropout=0.0, p_dropout_dec=0.0)

    def make():
        torch.manual_seed(0)
        m = train.build_model(cfg, device=dev())
        m.encoder.pre.p_dropout = 0.0
        for b in range(2):
            m.decoder.flows[3 * b].set_ddi(True)
        return m
    batch = train.synth_batch(4, 40, 120, 0, dev())
    lh = (batch[1].tolist(), batch[3].tolist())
    ref = make()
    with torch.no_grad():
        ref(*batch, lengths_host=lh)
    want = [(ref.decoder.flows[3 * b].logs.detach().clone(), ref.decoder.flows[3 * b].bias.detach().clone()) for b in range(2)]
    assert all(w[0].abs().max().item() > 1e-3 for w in want) and want[0][1].abs().max().item() > 1e-3    # the init moved them off zero
    for graph in (False, True):
        m = make()
        tr = train.Trainer(m, graph=graph, capture_after=1)
        for _ in range(2):
            tr.step(*batch, lengths_host=lh)
        torch.cuda.synchronize()
        assert tr.adam_steps == 2
        for b in range(2):
            an = m.decoder.flows[3 * b]
            assert an.initialized
            assert (an.logs.detach() - want[b][0]).abs().max().item() < 5e-3, (graph, b)        # two AdamW updates at lr 2e-4 away
            assert (an.bias.detach() - want[b][1]).abs().max().item() < 5e-3, (graph, b)


def test_step_inputs_one_launch_matches_copies_and_refreshes(built):
    """train._upload_step_inputs (gt_step_inputs: the batch into a captured step's padded static buffers + its ragged row contexts, one
    launch) against the launches it replaces (train._copy_padded per tensor, ops.RowsCtx.refresh per context)."""
    from glow_tts_amd import ops, train
    g = torch.Generator().manual_seed(3)
    B = 7
    lens_a = [33, 17, 40, 5, 29, 40, 12]
    lens_b = [31, 23, 38, 9, 25, 36, 14]                 # same rounded row count, different offsets
    srcs = [torch.randint(0, 99, (B, 37), generator=g).to(dev()), torch.tensor(lens_b).to(dev()),
            torch.randn(B, 80, 123, generator=g).to(dev()), torch.randn(B, 3, generator=g).to(dev()).to(torch.bfloat16).reshape(B, 3)[:, :2].contiguous()]
    shapes = [(B, 48), (B,), (B, 80, 160), (B, 4)]
    want = [torch.full(sh, 7, dtype=t.dtype, device=dev()) for sh, t in zip(shapes, srcs)]
    got = [w.clone() for w in want]
    for w, t in zip(want, srcs):
        train._copy_padded(w, t)
    ctx_w = [ops.RowsCtx(torch.tensor(lens_a, dtype=torch.int32, device=dev()), 40, lengths_host=lens_a, round_to=64) for _ in range(2)]
    ctx_g = [ops.RowsCtx(torch.tensor(lens_a, dtype=torch.int32, device=dev()), 40, lengths_host=lens_a, round_to=64) for _ in range(2)]
    lens2 = [lens_b, [v // 2 * 2 for v in lens_b]]
    if ops.RowsCtx.row_starts(lens2[1], 40, 64)[1] != ctx_w[1].R:
        lens2[1] = lens_b
    for c, l in zip(ctx_w, lens2):
        assert c.refresh(None, l)
    train._upload_step_inputs(list(zip(got, srcs)), list(zip(ctx_g, lens2)))
    torch.cuda.synchronize()
    for w, o in zip(want, got):
        assert torch.equal(w, o)
    for cw, cg in zip(ctx_w, ctx_g):
        for name in ("row0", "lengths", "rowbatch", "rowframe", "rowmask", "rowutt"):
            assert torch.equal(getattr(cw, name), getattr(cg, name)), name
    # a context whose rounded size does not match is refused, as refresh() refuses it
    with pytest.raises(AssertionError):
        train._upload_step_inputs([], [(ctx_g[0], [40] * B)])


def test_early_decoder_update_matches_the_single_optimizer_pass(built):
    """Trainer(early_decoder_adam=True) — the optimizer's pass over the decoder's conv parameters launched right behind the decoder's
    batched weight gradients, the rest after the backward — ends with the same parameters, moments and gradient norm as the single
    pass after the backward, eager and graph-replayed; and the early pass really runs (the decoder's flush covers the buffer's tail)."""
    from glow_tts_amd import train
    cfg = dict(train.BASE_MODEL, n_blocks_dec=2, n_layers_enc=1, p_dropout=0.0, p_dropout_dec=0.0)
    torch.manual_seed(0)
    m0 = train.build_model(cfg, device=dev())
    with torch.no_grad():
        for n, p in m0.named_parameters():
            if n.endswith("end.weight") or n.endswith("pre.proj.weight"):
                p.normal_(0, 0.02)
    batch = train.synth_batch(4, 40, 120, 0, dev())
    outs = {}
    for early in (False, True):
        for graph in (False, True):
            m = train.build_model(cfg, device=dev())
            m.load_state_dict(m0.state_dict())
            m.encoder.pre.p_dropout = 0.0
            tr = train.Trainer(m, graph=graph, capture_after=1, early_decoder_adam=early)
            calls = []
            orig = tr.opt.step_early
            tr.opt.step_early = lambda lo, hi, _o=orig, _c=calls: (_c.append((lo, hi)), _o(lo, hi))[1]
            for _ in range(3):
                tr.step(*batch)
            torch.cuda.synchronize()
            if not graph:
                assert calls == ([(tr.dec_cov_off, tr.buckets.total)] * 3 if early else [])
            assert tr.adam_steps == 3
            # the early pass is followed by the NEXT step's packing of the decoder's weights; a write into the parameters between two
            # steps (here: torch in-place ops, as load_state_dict does them) must not leave the stale images in use
            with torch.no_grad():
                for n, p in m.named_parameters():
                    if n.startswith("decoder.") and n.endswith("in_layers.0.weight_v"):
                        p.mul_(0.5)
            for _ in range(2):
                tr.step(*batch)
            torch.cuda.synchronize()
            outs[(early, graph)] = (tr.opt.flat_p.clone(), tr.opt.m.clone(), tr.opt.v.clone(), float(tr.grad_norm))
    ref = outs[(False, False)]
    for key, o in outs.items():
        for a, b in zip(ref[:3], o[:3]):
            assert (a - b).abs().max().item() < 5e-3, key      # (float atomics order differs from run to run, not the update)
        assert abs(ref[3] - o[3]) < 2e-2 * abs(ref[3]), key


def test_step_head_one_launch_clears_the_regions_and_bumps_the_seed(built):
    """ops.step_head (gt_step_zero): the step's accumulator arena, its pre-zeroed buffer region and one more region cleared, the dropout
    seed word advanced by bump_seed's constant — one launch; what lies behind a region is untouched."""
    from glow_tts_amd import devstate, ops
    d = dev()
    ops.arena_begin(d); ops.big_begin(d)                             # allocate
    a, b = devstate.get(d).small, devstate.get(d).big
    a.buf.fill_(3); b.buf[:8192].fill_(5); b.used = 5000
    extra = torch.full((1000 + 4,), 2.0, device=d)[:1000]            # 4000 bytes: a multiple of 16, with a guard behind it
    guard = extra.storage_offset()
    seed0 = int(ops.seed_word(d).item())
    ops.step_head(d, extra=extra)
    torch.cuda.synchronize()
    assert int(a.buf.count_nonzero()) == 0 and int(b.buf[:8192].count_nonzero()) == 0 and int(extra.count_nonzero()) == 0
    assert (int(ops.seed_word(d).item()) - seed0) & 0xffffffff == 0x632BE5AB
    odd = torch.full((1001,), 2.0, device=d)                         # 4004 bytes: not a multiple of 16 -> the plain fill
    ops.step_head(d, extra=odd, bump=False)
    torch.cuda.synchronize()
    assert int(odd.count_nonzero()) == 0 and (int(ops.seed_word(d).item()) - seed0) & 0xffffffff == 0x632BE5AB
    ops.arena_end(d)


def test_early_decoder_update_with_conditioning_layers(built):
    """A speaker-conditioned decoder (cfg 4): the WaveNets' cond_layer parameters get their gradients through autograd at the end of
    the backward, not from the decoder's weight-gradient flush — they sit in FRONT of the flush's parameters in the flat buffer, the
    early optimizer pass covers the tail behind them, and the result equals the single late pass."""
    from glow_tts_amd import train
    cfg = dict(train.BASE_MODEL, n_blocks_dec=2, n_layers_enc=1, p_dropout=0.0, p_dropout_dec=0.0, gin_channels=32)
    torch.manual_seed(0)
    m0 = train.build_model(cfg, device=dev())
    with torch.no_grad():
        for n, p in m0.named_parameters():
            if n.endswith("end.weight") or n.endswith("pre.proj.weight"):
                p.normal_(0, 0.02)
    batch = train.synth_batch(4, 40, 120, 0, dev())
    g = torch.randn(4, 32, 1, generator=torch.Generator().manual_seed(1)).to(dev())
    outs = {}
    for early in (False, True):
        m = train.build_model(cfg, device=dev())
        m.load_state_dict(m0.state_dict())
        m.encoder.pre.p_dropout = 0.0
        tr = train.Trainer(m, graph=True, capture_after=1, early_decoder_adam=early)
        names = {id(p): n for n, p in m.named_parameters()}
        tail = [names[id(p)] for p in tr.buckets.params[tr.dec_cov:]]
        assert tr.dec0 < tr.dec_cov < len(tr.buckets.params) and all(n.startswith("decoder.") and ".cond_layer." not in n for n in tail)
        assert all(".cond_layer." in names[id(p)] for p in tr.buckets.params[tr.dec0:tr.dec_cov])
        calls = []
        orig = tr.opt.step_early
        tr.opt.step_early = lambda lo, hi, _o=orig, _c=calls: (_c.append((lo, hi)), _o(lo, hi))[1]
        for _ in range(3):
            tr.step(*batch, g=g)
        torch.cuda.synchronize()
        assert bool(calls) == early and all(c == (tr.dec_cov_off, tr.buckets.total) for c in calls)
        outs[early] = ({n: p.detach().clone() for n, p in m.named_parameters()}, float(tr.grad_norm))
    for n, a in outs[False][0].items():
        assert (a - outs[True][0][n]).abs().max().item() < 5e-3, n
    assert abs(outs[False][1] - outs[True][1]) < 2e-2 * abs(outs[False][1])
