"""dev: does a change to the vocoders' host path (glow-tts_amd/audio.py) change what the GPU is asked for, or what it returns?

    vocoder_trace.py > trace.txt                  the full listing
    vocoder_trace.py --digest > digest.txt        per case: the calls counted by entry, a sha256 over their lines, the result's hashes
    vocoder_trace.py --digest-of trace.txt        the same from a saved listing (no GPU)

One line per C-ABI call of every case: the entry's name, every scalar argument (of the argument struct, or of the plain argument
list) and every pointer argument rewritten as "which tensor + byte offset" — mel, n_frames, bufs[name], held[...] (the k-th image /
bias / snake block, Vocos's images by name, the iSTFT image) — so that no address enters; a pointer into no known tensor (forward's own
frame counts, Vocos's zero-padded mel) is anon<k> in order of appearance.  Then a sha256 of the returned samples and lengths.  Two
trees agree if their outputs are equal files; the digests of two equal listings are what is kept
(profiles/vocoder_contract_trace_{parent,new}.txt), the listing is what to diff when they differ.  The library is wrapped below
_lib.call, as _lib.record_calls does, and the modules are built and seeded here: the file runs unchanged on any tree that has the
three vocoders.

Modules: HiFi-GAN tiny with resblock "1" and "2", BigVGAN tiny24 with resblock "1" and tiny with resblock "2" / snake, Vocos tiny with
80 and with 100 bands, BigVGAN tiny without tanh and final bias.  Cases per module: forward on the ragged batch FRAMES; forward of one
utterance (B = 1); forward of a channel-strided view; run() into a workspace of larger capacity with a mel of larger pitch (the last
module: forward only).  No launch is repeated or retried: run it under the caller's timeout.
"""
import ctypes, hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

FRAMES = (13, 1, 2, 40, 0, 7)
TINY = dict(upsample_rates=(4, 2), upsample_kernel_sizes=(8, 4), upsample_initial_channel=64, resblock_kernel_sizes=(3, 7, 11),
            resblock_dilation_sizes=((1, 3, 5),) * 3)
TINY24 = dict(TINY, upsample_rates=(2, 2), upsample_kernel_sizes=(4, 4), upsample_initial_channel=96)
VOCOS_TINY = dict(input_channels=80, dim=128, intermediate_dim=256, num_layers=2)


def modules(audio, dev):
    """[(name, module on the device, mel channels, with the capacity case)]: seeded default initialisation; alpha / beta and Vocos's
    layer scale drawn, so that no activation is the identity"""
    def seeded(seed, build):
        torch.manual_seed(seed)
        voc = build()
        g = torch.Generator().manual_seed(seed + 1)
        with torch.no_grad():
            for name, p in voc.named_parameters():
                if name.endswith((".alpha", ".beta", ".gamma")):
                    p.copy_(torch.rand(p.shape, generator=g) * 0.9 + 0.1)
        return voc.to(dev)
    return [("hifigan tiny resblock 1", seeded(8, lambda: audio.HiFiGAN(resblock="1", **TINY)), 80, True),
            ("hifigan tiny resblock 2", seeded(9, lambda: audio.HiFiGAN(resblock="2", **TINY)), 80, True),
            ("bigvgan tiny24 resblock 1", seeded(10, lambda: audio.BigVGAN(resblock="1", n_mel_channels=16, **TINY24)), 16, True),
            ("bigvgan tiny resblock 2 snake", seeded(11, lambda: audio.BigVGAN(resblock="2", activation="snake", n_mel_channels=16, **TINY)),
             16, True),
            ("vocos tiny", seeded(12, lambda: audio.Vocos(**VOCOS_TINY)), 80, True),
            ("vocos tiny 100 bands", seeded(13, lambda: audio.Vocos(**dict(VOCOS_TINY, input_channels=100))), 100, True),
            ("bigvgan tiny no tanh no bias", seeded(14, lambda: audio.BigVGAN(resblock="2", activation="snake", n_mel_channels=16,
                                                                                 use_tanh_at_final=False, use_bias_at_final=False, **TINY)),
             16, False)]


def extent(t):
    """bytes from t's first element to behind its last"""
    return (sum((n - 1) * s for n, s in zip(t.shape, t.stride())) + 1) * t.element_size() if t.numel() else 0


def flatten(label, v, out):
    if torch.is_tensor(v):
        out.append((label, v))
    elif isinstance(v, dict):
        for k, x in v.items():
            flatten(f"{label}.{k}", x, out)
    elif isinstance(v, (list, tuple)):
        for i, x in enumerate(v):
            flatten(f"{label}[{i}]", x, out)


class Tracer:
    """the library with every gt_* call written out as one line (installed as _lib._LIB)"""

    def __init__(self, L, protos, out):
        self._L, self._protos, self._out = L, protos, out
        self.known, self.anon, self.keep = [], {}, []

    def reset(self, **named):
        self.known, self.anon, self.keep = [], {}, []
        self.register(**named)

    def register(self, **named):
        found = []
        for label, v in named.items():
            flatten(label, v, found)
        for label, t in found:
            self.keep.append(t)                                       # alive for the whole case: no address is handed out twice
            if t.is_cuda and t.numel():
                self.known.append((label, t.data_ptr(), t.data_ptr() + extent(t)))

    def name(self, p):
        if not p:
            return "NULL"
        hits = [(hi - lo, label, lo) for label, lo, hi in self.known if lo <= p < hi]
        if hits:
            _, label, lo = min(hits)                                  # the innermost: a snake block inside the flat parameter tensor
            return f"{label}+{p - lo}"
        return f"anon{self.anon.setdefault(p, len(self.anon))}"

    def fields(self, a):
        return [f"{f}={self.name(getattr(a, f)) if ct is ctypes.c_void_p else repr(getattr(a, f))}" for f, ct in a._fields_]

    def __getattr__(self, name):
        fn = getattr(self._L, name)
        if not name.startswith("gt_"):
            return fn

        def call(*args):
            parts = []
            for i, (a, ct) in enumerate(zip(args, self._protos[name][1])):
                if isinstance(a, ctypes.Structure):
                    parts += self.fields(a)
                elif hasattr(a, "data_ptr"):
                    parts.append(f"{i}={self.name(a.data_ptr())}")
                elif isinstance(a, ctypes.c_void_p):
                    parts.append(f"{i}=stream")
                elif a is None:
                    parts.append(f"{i}=NULL")
                else:
                    parts.append(f"{i}={a!r}")
            self._out(f"  {name} " + " ".join(parts))
            return fn(*args)
        return call


def sha(t):
    return "-" if t is None else f"{tuple(t.shape)} {hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()}"


def digest(lines):
    """the listing with every case's call lines folded into their count per entry and one sha256"""
    out, calls = [], []

    def fold():
        if calls:
            names = [c.split()[0] for c in calls]
            counts = ", ".join(f"{n} x {names.count(n)}" for n in dict.fromkeys(names))
            out.append(f"  {len(calls)} calls ({counts}) sha256 {hashlib.sha256(chr(10).join(calls).encode()).hexdigest()}")
            calls.clear()
    for line in lines:
        if line.startswith("  gt_"):
            calls.append(line)
        else:
            fold()
            out.append(line)
    fold()
    return out


def main(args):
    if "--digest-of" in args:
        with open(args[args.index("--digest-of") + 1]) as f:
            sys.stdout.write("\n".join(digest(f.read().splitlines())) + "\n")
        return
    from glow_tts_amd import _lib, audio
    dev = torch.device("cuda:0")
    lines = []
    emit = lines.append
    tr = Tracer(_lib.lib(), _lib.PROTOTYPES, emit)
    B, F = len(FRAMES), max(FRAMES)
    for name, voc, n_mel, capacity in modules(audio, dev):
        g = torch.Generator().manual_seed(17)
        wide = (torch.randn(B, 2 * n_mel, F + 16, generator=g) * 2 - 5).to(dev)
        for b, n in enumerate(FRAMES):
            wide[b, :, n:] = float("nan")                             # nothing behind an utterance's frames may matter
        mel = wide[:, :n_mel, :F].contiguous()
        lengths = torch.tensor(FRAMES, dtype=torch.int32, device=dev)
        held = voc.held()                                             # packed outside the trace
        workspace = voc.workspace

        def traced_workspace(*a, **k):
            bufs = workspace(*a, **k)
            tr.register(bufs=bufs)
            return bufs

        def case(tag, fn, **named):
            emit(f"{name}: {tag}")
            tr.reset(held=held, **named)
            _lib._LIB = tr
            try:
                out = fn()
            except ValueError as e:
                out = None
                emit(f"  refused: {e}")
            finally:
                _lib._LIB = tr._L
            torch.cuda.synchronize()
            wav, wav_lengths = out if isinstance(out, tuple) else (out, None)
            emit(f"  wav {sha(wav)} lengths {sha(wav_lengths)}")

        voc.workspace = traced_workspace
        case("forward, ragged batch", lambda: voc(mel, lengths, mel_lengths_host=list(FRAMES)), mel=mel, n_frames=lengths)
        one = mel[3:4].contiguous()
        case("forward, B = 1", lambda: voc(one), mel=one)
        view = wide[:, ::2, :F]
        case("forward, channel-strided view", lambda: voc(view, lengths, mel_lengths_host=list(FRAMES)), mel=view, n_frames=lengths)
        del voc.workspace
        if capacity:
            big = wide[:, :n_mel].contiguous()
            big = torch.cat([big, torch.full_like(big[:1], float("nan"))])
            n_frames = torch.tensor(list(FRAMES) + [0], dtype=torch.int32, device=dev)

            def run():
                bufs = voc.workspace(B + 1, F + 11, dev)
                for t in bufs.values():
                    t.view(torch.int16 if t.element_size() == 2 else torch.int32).fill_(-1)    # NaN patterns: nothing stale may matter
                tr.register(bufs=bufs)
                return voc.run(big, n_frames, bufs)
            case("run into a workspace of (B + 1, F_max + 11)", run, mel=big, n_frames=n_frames)
    sys.stdout.write("\n".join(digest(lines) if "--digest" in args else lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
