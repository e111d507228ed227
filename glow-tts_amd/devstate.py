"""Per-device state of the training step, one object per device (`get(device)`, the only registry): auxiliary streams, the dropout
seed word, the two pre-zeroed step arenas, grow-only scratch, the CU count.  ops / text_models / wgrad / flow_impl wrap it."""
import functools

import torch

ARENA_BYTES = 1 << 20        # small arena: the step's ~150 tiny zeroed accumulators (atomicAdd targets)
BIG_BYTES = 96 << 20         # big arena: per-layer buffers that kernels only partly write (halo rows must read as zero)


class ZeroArena:
    """A pre-zeroed buffer that hands out 256-byte-granular zeroed slices between open() and close(): one fill per training step
    instead of one per buffer.  Allocated on first open() and never again — captured graphs hold its address."""

    def __init__(self, device, size, item_max=None, partial=False):
        self.device, self.size, self.partial = device, size, partial   # partial: clear only what earlier steps dirtied (`used`)
        self.item_max = size if item_max is None else item_max     # larger requests fall through to torch.zeros
        self.buf, self.off, self.on, self.used = None, 0, False, 0

    def open(self):
        """Open for a step -> bytes at the head of `buf` the caller must clear (0 on first use: the allocation comes back zeroed)."""
        self.off, self.on = 0, True
        if self.buf is None:
            self.buf = torch.zeros(self.size, dtype=torch.uint8, device=self.device)
            return 0
        return min(self.size, (self.used + 4095) & ~4095) if self.partial and self.used else self.size

    def begin(self):
        """open() with the clear as a plain fill (outside ops.step_head)"""
        n = self.open()
        self.buf[:n].zero_()

    def close(self):
        self.on = False

    def zeros(self, shape, dtype):
        """Zeroed tensor: a slice of the arena while it is open and has room, torch.zeros otherwise."""
        n = 1
        for d in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)):
            n *= int(d)
        nbytes = (n * torch.empty(0, dtype=dtype).element_size() + 255) & ~255
        if not self.on or nbytes > self.item_max or self.off + nbytes > self.size:
            return torch.zeros(shape, dtype=dtype, device=self.device)
        off = self.off
        self.off = off + nbytes
        self.used = max(self.used, self.off)
        return self.buf[off:off + nbytes].view(dtype)[:n].view(shape)


class DeviceState:
    def __init__(self, device):
        self.device = torch.device(device)
        self.small = ZeroArena(self.device, ARENA_BYTES, item_max=65536)
        self.big = ZeroArena(self.device, BIG_BYTES, partial=True)
        self.streams = {}            # name -> auxiliary stream ("encoder", "front", "wgrad_side"): a device resource, not model state
        self.pending = False         # a queue was flushed on the wgrad side stream and nobody has joined it yet (wgrad.join)
        # name or (name, stream handle) -> grow-only uint8 buffer; those a capture nobody owns replays into: for the life of the process
        self.scratch_bufs, self._forever = {}, []

    def stream(self, name):
        s = self.streams.get(name)
        if s is None:
            s = self.streams[name] = torch.cuda.Stream(device=self.device)
        return s

    def drop_streams(self):
        """Forget the auxiliary streams (they may be left in capture state by an aborted capture: never synchronised or destroyed
        here) — the next stream(name) makes a fresh one.  Nothing a captured graph has the address of is touched."""
        self.streams = {}
        self.pending = False

    @functools.cached_property
    def seed(self):
        """int32[1] mixed into every dropout seed; allocated once (on first use) — captured graphs hold its address"""
        return torch.zeros(1, dtype=torch.int32, device=self.device)

    @functools.cached_property
    def cus(self):
        return torch.cuda.get_device_properties(self.device).multi_processor_count

    def scratch(self, name, nbytes, per_stream=False):
        """Grow-only device scratch, one per purpose (per_stream: and per stream it is asked for on — flushes that run concurrently
        must not share one).  A captured step has the address of the buffer it was captured with baked into its kernel arguments, and
        a later capture may need a bigger one: freed, the outgrown buffer's pages go back to the allocator and the next replay of the
        older graph writes over whoever owns them then.  So every capture holds a reference to the buffer it used (wgrad.capture_keep:
        it lives exactly as long as the graphs that replay into it), and a capture nobody owns keeps it for the life of the process."""
        cuda = self.device.type == "cuda"
        key = (name, torch.cuda.current_stream(self.device).cuda_stream if cuda else 0) if per_stream else name
        buf = self.scratch_bufs.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = self.scratch_bufs[key] = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=self.device)
        if cuda and torch.cuda.is_current_stream_capturing():
            from . import wgrad
            if not wgrad.capture_keep(buf):
                self._forever.append(buf)
        return buf


_STATES = {}


def get(device):
    """The DeviceState of `device`, keyed by str(device) exactly ("cuda" and "cuda:0" are two entries: two seed words, two arenas)."""
    st = _STATES.get(str(device))
    if st is None:
        st = _STATES[str(device)] = DeviceState(device)
    return st
