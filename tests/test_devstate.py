"""Host logic of the per-device step state (devstate.DeviceState / ZeroArena) and of wgrad.capture_scope, on the CPU device."""
import pytest
import torch

CPU = torch.device("cpu")


def _inside(t, buf):
    lo = buf.data_ptr()
    return lo <= t.data_ptr() and t.data_ptr() + t.numel() * t.element_size() <= lo + buf.numel()


def test_arena_slices_are_zero_disjoint_and_256_byte_granular():
    from glow_tts_amd import devstate
    ar = devstate.ZeroArena(CPU, 1 << 16, item_max=4096)
    ar.begin()
    a = ar.zeros((5,), torch.float32)
    b = ar.zeros((192,), torch.float32)
    c = ar.zeros((3, 7), torch.bfloat16)
    d = ar.zeros(9, torch.int32)                                     # a bare int is a shape too
    base = ar.buf.data_ptr()
    assert [t.data_ptr() - base for t in (a, b, c, d)] == [0, 256, 1024, 1280] and ar.off == 1536
    assert a.shape == (5,) and b.shape == (192,) and c.shape == (3, 7) and d.shape == (9,)
    for t in (a, b, c, d):
        assert int(t.count_nonzero()) == 0 and _inside(t, ar.buf)
    for i, t in enumerate((a, b, c, d)):                             # disjoint: writing one leaves the others zero
        t.fill_(i + 1)
    assert [int(t.float().sum()) for t in (a, b, c, d)] == [5, 2 * 192, 3 * 21, 4 * 9]
    ar.begin()                                                       # the next step finds everything zero again, from offset 0
    assert ar.off == 0 and int(ar.buf.count_nonzero()) == 0


def test_arena_next_offset_after_5_and_192_floats():
    from glow_tts_amd import devstate
    ar = devstate.ZeroArena(CPU, 1 << 16)
    assert ar.open() == 0                                            # first use: allocated zeroed, nothing to clear
    a, b = ar.zeros((5,), torch.float32), ar.zeros((192,), torch.float32)
    assert (a.data_ptr() - ar.buf.data_ptr(), b.data_ptr() - ar.buf.data_ptr(), ar.off) == (0, 256, 1024)


def test_arena_falls_back_to_plain_zeros_outside_the_buffer():
    from glow_tts_amd import devstate, ops
    st = devstate.get(CPU)
    ops.arena_end(CPU)
    never = devstate.ZeroArena(CPU, 4096)
    t = never.zeros((4,), torch.float32)                             # never opened
    assert never.buf is None and int(t.count_nonzero()) == 0
    ops.arena_begin(CPU)
    small = st.small
    assert small.size == devstate.ARENA_BYTES == 1 << 20 and small.item_max == 65536
    ok = ops.zeros_small((65536 // 4,), torch.float32, CPU)          # exactly the largest item
    over = ops.zeros_small((65536 // 4 + 1,), torch.float32, CPU)
    assert _inside(ok, small.buf) and not _inside(over, small.buf) and over.shape == (65536 // 4 + 1,) and int(over.count_nonzero()) == 0
    off = small.off
    while small.off + 65536 <= small.size:                           # fill it up
        assert _inside(ops.zeros_small((65536,), torch.uint8, CPU), small.buf)
    assert small.off == small.size and small.off > off
    full = ops.zeros_small((5,), torch.float32, CPU)
    assert not _inside(full, small.buf) and full.dtype == torch.float32 and int(full.count_nonzero()) == 0
    ops.arena_end(CPU)
    closed = ops.zeros_small((5,), torch.float32, CPU)
    assert not _inside(closed, small.buf) and int(closed.count_nonzero()) == 0


def test_big_arena_clears_what_was_used_rounded_up_to_4096():
    from glow_tts_amd import devstate
    ar = devstate.ZeroArena(CPU, 1 << 20, partial=True)
    assert ar.open() == 0 and ar.used == 0
    ar.close()
    assert ar.open() == ar.size                                      # used == 0: the whole buffer
    ar.zeros((1000,), torch.float32)                                 # 4000 bytes -> 4096 handed out
    ar.zeros((100,), torch.float32)                                  # + 512
    assert ar.used == 4096 + 512
    ar.close()
    assert ar.open() == 8192
    ar.zeros((10,), torch.float32)
    assert ar.used == 4096 + 512                                     # the high-water mark is never reset
    ar.buf[:8192].fill_(7); ar.buf[8192:8200].fill_(9)
    ar.begin()
    assert int(ar.buf[:8192].count_nonzero()) == 0 and int(ar.buf[8192:8200].count_nonzero()) == 8
    ar.used = ar.size - 100
    assert ar.open() == ar.size                                      # never past the buffer
    whole = devstate.ZeroArena(CPU, 1 << 16)                         # the small arena's rule: everything, whatever was used
    whole.open(); whole.zeros((10,), torch.float32)
    assert whole.open() == whole.size


def test_step_head_on_cpu_zeroes_extra_and_bumps_the_seed():
    from glow_tts_amd import devstate, ops
    s0 = int(ops.seed_word(CPU).item())
    x = torch.ones(12)
    ops.step_head(CPU, extra=x)
    assert int(x.count_nonzero()) == 0 and (int(ops.seed_word(CPU).item()) - s0) & 0xffffffff == 0x632BE5AB
    st = devstate.get(CPU)
    assert st.small.on and st.big.on and st.small.off == 0 and st.big.off == 0
    assert _inside(ops.zeros_big((3, 5), torch.float32, CPU), st.big.buf)
    ops.arena_end(CPU)
    assert not st.small.on and not st.big.on


def test_registry_is_one_object_per_device_string_and_keeps_the_seed_word():
    from glow_tts_amd import devstate, ops
    st = devstate.get(CPU)
    assert devstate.get(CPU) is st and devstate.get(torch.device("cpu")) is st and devstate.get("cpu") is st
    seed = ops.seed_word(CPU)
    small = st.small
    ws = st.scratch("t", 100)
    st.streams["front"] = object(); st.pending = True                # (no streams on the CPU device: stand-ins)
    st.drop_streams()
    assert st.streams == {} and st.pending is False
    assert ops.seed_word(CPU) is seed and st.small is small and st.scratch("t", 50) is ws    # nothing address-baked was dropped
    assert st.scratch("t", 200) is not ws and st.scratch("t", 200).numel() >= 200            # grow-only
    assert st.scratch("t", 10, per_stream=True) is not st.scratch("t", 10)                   # a key of its own


def test_capture_scope_closes_itself_on_exit_and_on_an_exception():
    from glow_tts_amd import wgrad
    x, y = torch.empty(1), torch.empty(1)
    assert not wgrad.capture_keep(x)
    with wgrad.capture_scope(CPU, nbytes=1024) as keep:
        sc = wgrad._SCOPE
        assert keep is sc.keep and len(keep) == 1                    # the table arena
        assert wgrad.capture_keep(x) and wgrad.capture_keep(x) and wgrad.capture_keep(y)
        assert sum(o is x for o in keep) == 1 and sum(o is y for o in keep) == 1
        dst, host = sc.arena[:4], torch.tensor([1, 2, 3, 4], dtype=torch.uint8)
        sc.uploads.append((dst, host))
    assert wgrad._SCOPE is None and not wgrad.capture_keep(x) and sc.uploads == []
    assert dst.tolist() == [1, 2, 3, 4] and len(keep) == 3           # tables filled on the way out; the keep is the caller's now
    with pytest.raises(RuntimeError, match="refused"):
        with wgrad.capture_scope(CPU, nbytes=1024) as keep2:
            bad = wgrad._SCOPE
            wgrad.capture_keep(x)
            bad.uploads.append((bad.arena[:4], host))
            raise RuntimeError("capture refused")
    assert wgrad._SCOPE is None and not wgrad.capture_keep(x) and bad.uploads == [] and len(keep2) == 0      # released
    with wgrad.capture_scope(CPU, nbytes=1024) as keep3:             # a scope after a failed one starts empty
        assert len(keep3) == 1 and wgrad._SCOPE.uploads == [] and wgrad._SCOPE.off == 0
    assert not wgrad.capture_keep(x)
