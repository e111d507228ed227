"""TEST INFRASTRUCTURE ONLY — guarded device buffers for tests that call a C-ABI entry on hand-made operands.

  inp   an input exactly as long as the kernel may read, between NaN guards (integer inputs: a valid in-range `fill`, so that a kernel
        that reads past the end computes a wrong number instead of faulting);
  out   an output inside canaries and pre-filled with canaries (every element must be written), or pre-filled with `prior` for an
        accumulate-into output; `keep` marks elements the kernel must NOT write (the columns between C and the row stride).

verify() after the launch: no guard was written, no output holds a NaN (a NaN guard was read) or a canary (an element was skipped).
The data starts PAD elements into its buffer: 16-byte aligned for every element type, `shift` moves it off that alignment."""
import torch

CAN = 768.0          # exact in bf16 and fp32
PAD = 64


class Guards:
    def __init__(self, device):
        self.device, self.outs = device, []

    def _place(self, flat, fill, shift):
        buf = torch.full((flat.numel() + 2 * PAD + shift,), fill, dtype=flat.dtype, device=self.device)
        view = buf[PAD + shift:PAD + shift + flat.numel()]
        view.copy_(flat)
        return buf, view

    def inp(self, t, fill=float("nan"), shift=0):
        if t is None:
            return None
        t = t.contiguous()
        assert t.is_floating_point() or fill == fill, "an integer input needs an in-range guard value"
        buf, view = self._place(t.reshape(-1), fill, shift)
        return view.view(t.shape)

    def out(self, name, shape, dtype=torch.float32, prior=None, keep=None):
        if prior is None:
            start = torch.full(tuple(shape), CAN, dtype=dtype)
        else:
            start = prior.to(dtype).reshape(tuple(shape))
        buf, view = self._place(start.reshape(-1), CAN, 0)
        view = view.view(tuple(shape))
        self.outs.append((name, buf, view, prior is None, keep))
        return view

    def verify(self):
        torch.cuda.synchronize()
        for name, buf, view, fresh, keep in self.outs:
            n = view.numel()
            g = torch.cat([buf[:PAD], buf[PAD + n:]]).float()
            assert bool((g == CAN).all()), f"{name}: a guard was written"
            v = view.float().cpu()
            k = torch.zeros(v.shape, dtype=torch.bool) if keep is None else torch.as_tensor(keep).expand(v.shape)
            assert bool((v[k] == CAN).all()), f"{name}: an element outside the kernel's columns was written"
            assert bool(torch.isfinite(v[~k]).all()), f"{name}: a NaN guard was read"
            if fresh:
                assert not bool((v[~k] == CAN).any()), f"{name}: an element was not written"
