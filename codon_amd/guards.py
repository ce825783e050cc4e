"""Host-side state that is ordered by a HIP stream: the per-stream cache, and the two device-side guards (stale packed
weights, non-finite inputs) that keep their workspaces in it.  Their on / off switches are with the others in codon_amd.model."""
from __future__ import annotations

import sys
import threading

import torch

from . import _lib as L
from . import ops


class PerStream:
    """Values private to (device index, raw stream handle, host thread): device words, workspaces and side streams, which are
    ordered by the stream they are used on.  Independent callers -- DataParallel replica threads, a hipGraph capture in one
    thread beside eager launches in another -- never share one: no launches that count in each other's words, no false
    cross-dependencies.
    Capture: get() asks is_current_stream_capturing() BEFORE it looks at the table.  What is made under capture belongs to
    the graph's pool and is never cached -- nor is a cached value ever baked into a graph, where a later, larger request or
    the pruning could free it under the replays; it goes to the caller, who keeps it alive (`hold`, bounded).
    Pruning: short-lived caller threads (thread pools, nn.DataParallel's per-forward threads) would add an entry each, so
    before a new entry goes into a table of `keep` or more, entries of dead threads are dropped.  Their device memory returns
    to the caching allocator, which orders its reuse behind the work already enqueued on the stream it was used on."""
    __slots__ = ("table",)

    def __init__(self):
        self.table = {}

    def get(self, dev, make, need: int = 0, stream=None, hold=None, keep: int = 16):
        """The value of (dev, `stream` or dev's current stream, this thread), made by make(capturing) when there is none or
        it does not fit: a tensor of numel() < need (the device is part of the key: a cached tensor is on `dev`)."""
        if torch.cuda.is_current_stream_capturing():
            v = make(True)
            if hold is not None:
                hold.append(v)
                del hold[:-8]
            return v
        key = (dev.index if dev.index is not None else torch.cuda.current_device(),
               ops._stream(dev) if stream is None else stream, threading.get_ident())      # the raw handle: no Stream object
        v = self.table.get(key)
        if v is None or (need and v.numel() < need):
            if len(self.table) >= keep:
                alive = {t.ident for t in threading.enumerate()}
                for k in [k for k in self.table if k[2] not in alive]:
                    del self.table[k]
            v = self.table[key] = make(False)
        return v

    def values(self):
        return self.table.values()


_STALE_MSG = ("codon_amd: a conv weight was written through `.data` (or another path that does not bump Tensor._version, "
              "e.g. `m.weight.data.normal_()`) after its packed MFMA image was built -- the forward(s) since then used the "
              "stale packed weights; call model.invalidate_packed() after such writes")


class _WeightGuard:
    """Default-on detector of stale packed weights.  The pack cache is keyed on (data_ptr, Tensor._version) of each weight,
    which a write through `.data` does not change.  Every forward launches ONE small kernel (codon_weight_checksum) over
    the raw bytes of the 17 MFMA conv weights: the first launch after the host-visible key changed records the checksum the
    packed images are built from, every later one compares and, on a mismatch, sets a flag in pinned host memory.  The
    host reads that word (no synchronisation) at the start of every forward / graph replay and in check_packed(): the
    stale forward itself has already been enqueued by then, the NEXT call raises.  Per (stream, thread) state, because
    the kernel's workspace and reference slot are ordered by the stream they are used on."""

    def __init__(self):
        self.tag = None            # host-visible key of all 17 weights the pack cache was last valid for
        self.flag = None           # pinned int32[1], written by the kernel
        self.flag_np = None
        self.states = PerStream()  # -> [tag, workspace, desc, tensor whose last word is the reference]
        self.captured = []         # states made under a hipGraph capture (GraphedCODON keeps them)
        self.disabled = False
        self._retired = []         # flag words / workspaces of earlier epochs (see reset)

    def tripped(self) -> bool:
        return self.flag_np is not None and bool(self.flag_np[0])

    def devices(self):             # every device a checksum launch went to
        return {st[1].device for st in self.states.values()}

    def reset(self):
        """Forget the recorded checksums and the tripped state.  A checksum launch of the stale forward may still be in
        flight and a captured hipGraph may still hold the addresses: the old flag word and workspaces are retired (kept
        alive, never reused), not cleared or freed -- a late store cannot trip the NEW flag, a replay cannot write into
        memory someone else now owns."""
        self.tag = None
        self._retired.append((self.flag, list(self.states.values()) + self.captured))
        del self._retired[:-8]                 # bounded: each entry is a few KB
        self.states = PerStream()
        self.captured = []
        self.flag = None
        self.flag_np = None

    def run(self, model, ws, dev, clear=None, nclear: int = 0) -> bool:
        """ws: the 17 MFMA conv weights of `model`.  clear / nclear: int32 words on `dev` the launch also zeroes (the input
        guard's per-image words).  True when the launch went out (False: guard disabled for these weights -- the caller
        zeroes them itself)."""
        import ctypes as C
        if self.tripped():
            raise RuntimeError(_STALE_MSG)
        tag = tuple((w.data_ptr(), w._version, w.dtype) for w in ws) + (dev,)
        if tag != self.tag:
            # some weight changed visibly: EVERY packed image is rebuilt, so that all of them belong to the checksum
            # recorded below (a partial rebuild could fold an earlier invisible write into the new reference)
            model._pack_cache.clear()
            self.tag = tag
            self.disabled = any((w.data_ptr() % 16) or ((w.numel() * w.element_size()) % 16) or not w.is_contiguous()
                                for w in ws)
        if self.disabled:
            return False
        if self.flag is None:
            self.flag = torch.zeros(1, dtype=torch.int32).pin_memory()
            self.flag_np = self.flag.numpy()
        lib = L.load()
        st = self.states.get(dev, lambda _: [None, torch.zeros(lib.codon_weight_checksum_workspace_bytes() // 8 + 1,   # + the
                                                               dtype=torch.int64, device=dev), None, None],    # reference slot
                             hold=self.captured)
        mode = 1
        if st[0] != tag:
            d = L.WsumDesc()
            d.n = len(ws)
            for i, w in enumerate(ws):
                d.data[i] = w.data_ptr()
                d.bytes[i] = w.numel() * w.element_size()
            # under hipGraph capture a recording launch would be replayed as a recording launch and never compare: take
            # the reference another stream recorded for these very weights (GraphedCODON's warm-up runs; they are joined
            # before the capture starts) and capture a COMPARING launch
            donor = None
            if torch.cuda.is_current_stream_capturing():
                donor = next((o for o in self.states.values() if o[0] == tag and o[1].device == dev), None)
                if donor is None:
                    raise RuntimeError("codon_amd: hipGraph capture of a forward whose weights no eager forward has seen "
                                       "yet -- the captured weight-checksum launch would RECORD on every replay and never "
                                       "compare; run one forward outside the capture first (GraphedCODON does: warmup >= 1)")
            st[0], st[2] = tag, d
            st[3], mode = (donor[3], 1) if donor is not None else (st[1], 0)
        ref = st[3]
        with torch.cuda.device(dev):
            L.check(lib.codon_weight_checksum_clear(C.byref(st[2]), C.c_void_p(st[1].data_ptr()),
                                                    C.c_void_p(ref.data_ptr() + 8 * (ref.numel() - 1)), mode,
                                                    C.c_void_p(self.flag.data_ptr()),
                                                    C.c_void_p(clear.data_ptr()) if clear is not None else None,
                                                    nclear if clear is not None else 0, C.c_void_p(ops._stream(dev))),
                    "weight_checksum")
        return True


NONFINITE_MODES = ("raise", "propagate", "ignore")


def default_nonfinite_mode() -> str:
    # INPUT_GUARD is with the other switches in codon_amd.model, read at call time (0 = "ignore" is the default mode)
    return "raise" if sys.modules[__package__ + ".model"].INPUT_GUARD else "ignore"


class NonFiniteInputError(RuntimeError):
    """A forward ran on an input that holds NaN, +Inf or -Inf.  .depth / .guidance: which input (x / y) the stems saw it in."""

    def __init__(self, depth: bool, guidance: bool, where: str = ""):
        self.depth, self.guidance = bool(depth), bool(guidance)
        which = " and ".join(n for n, f in (("the depth input x", depth), ("the guidance input y", guidance)) if f)
        super().__init__(
            f"codon_amd: {which} of the previous forward(s) held a non-finite value (NaN or +-Inf){where} -- the forward(s) "
            "enqueued since the last check ran on it and returned an all-NaN map for every image that held one.  Mask such "
            "pixels before the call, or choose model.set_nonfinite_inputs('propagate') (all-NaN maps, "
            "nothing raised) or 'ignore' (no detection)")


class _InputGuard:
    """State of the non-finite input guard of one model.  `words`: two int32 words in pinned host memory --
    [0] depth, [1] guidance -- that the stems store 1 to; allocated once and only ever zeroed IN PLACE, so the address a
    captured hipGraph carries stays valid.  `bad`: the per-image device words the stems mark and the head reads, private to
    a (stream, thread) like the weight guard's workspace, because they are ordered by the stream they are used on."""

    def __init__(self):
        self.words = None
        self.words_np = None
        self.words_ptr = None
        self.bad = PerStream()     # -> int32 tensor on the launch device
        self.devices = set()       # every device a guarded launch went to
        self.home = None           # device of the words' owner (nn.DataParallel replicas elsewhere run unguarded)
        self.captured = []         # `bad` tensors allocated under a hipGraph capture (GraphedCODON keeps them)

    def host_words(self):
        if self.words is None:
            self.words = torch.zeros(2, dtype=torch.int32).pin_memory()
            self.words_np = self.words.numpy()
            self.words_ptr = self.words.data_ptr()
        return self.words

    def bad_words(self, dev, B: int) -> torch.Tensor:
        self.devices.add(dev)
        # under capture no fill launch: the captured checksum launch (or memset) zeroes the words on every replay; held in
        # `captured` so that the graph's pool cannot hand them to a later tensor of the capture
        return self.bad.get(dev, lambda capturing: torch.empty((B,), dtype=torch.int32, device=dev) if capturing else
                            torch.zeros((max(B, 64),), dtype=torch.int32, device=dev), need=B, hold=self.captured)

    def tripped(self):
        w = self.words_np
        return (bool(w[0]), bool(w[1])) if w is not None else (False, False)

    def report(self, synchronize: bool, where: str = ""):
        """Raise NonFiniteInputError if a word is set.  Reporting consumes the trip: the devices are synchronised first (no
        stem of a forward enqueued so far can store after the words are cleared), the words are zeroed in place."""
        if self.words_np is None:
            return
        if synchronize and torch.cuda.is_available():
            for d in self.devices:
                torch.cuda.synchronize(d)
        d, g = self.tripped()
        if not (d or g):
            return
        if torch.cuda.is_available():
            for dv in self.devices:
                torch.cuda.synchronize(dv)
        d2, g2 = self.tripped()
        self.words_np[:] = 0
        raise NonFiniteInputError(d or d2, g or g2, where)


class _NonFiniteMixin:
    """set_nonfinite_inputs / check_inputs and the per-forward plumbing, shared by CODONNet, CODONNet16 and the ablation nets."""

    def set_nonfinite_inputs(self, mode: str):
        """What a forward does with an input image that holds NaN, +Inf or -Inf (depth sensors and .npy / EXR depth files mark
        holes that way).  The reference returns an all-NaN map for such an image and leaves the rest of the batch untouched.
          "raise" (default): the stems detect it on the device, the head stores the all-NaN map, and the NEXT forward, graph
              replay or check_inputs() raises NonFiniteInputError (no synchronisation: the offending forward has been enqueued
              by then, as with the weight guard);
          "propagate": the all-NaN map for every such image, bit-identical maps for the others, nothing raised or read on the host;
          "ignore": no detection (the behaviour before this guard: a finite-looking, wrong map).
        On finite inputs the three modes return the same bits.  CODON_INPUT_GUARD=0 makes "ignore" the default."""
        if mode not in NONFINITE_MODES:
            raise ValueError(f"codon_amd: set_nonfinite_inputs({mode!r}): one of {NONFINITE_MODES}")
        self.__dict__["_nonfinite_mode"] = mode
        return self

    @property
    def nonfinite_inputs(self) -> str:
        """The mode in force: what set_nonfinite_inputs chose, else the default ("raise"; "ignore" with CODON_INPUT_GUARD=0)."""
        return self._nf_mode()

    def _nf_mode(self) -> str:
        return self.__dict__.get("_nonfinite_mode") or default_nonfinite_mode()

    def _nf_state(self) -> "_InputGuard":
        g = self.__dict__.get("_iguard")
        if g is None:
            g = self.__dict__["_iguard"] = _InputGuard()
        return g

    def check_inputs(self, synchronize: bool = True):
        """Raise NonFiniteInputError if a forward since the last report ran on a non-finite input ("raise" mode).
        synchronize=True waits for the devices first, so every forward enqueued so far has been judged."""
        g = self.__dict__.get("_iguard")
        if g is not None:
            g.report(synchronize)
        return self

    def _nf_check(self):
        """Start of every public forward: report a trip of an earlier forward (one host read per word, no synchronisation).
        Never called under a hipGraph capture (GraphedCODON drives _forward_impl)."""
        g = self.__dict__.get("_iguard")
        if g is None:
            return
        w = g.words_np
        if w is None or not (w[0] or w[1]):
            return                            # the whole cost on the usual path: two reads of host memory
        if self._nf_mode() == "raise" and not torch.cuda.is_current_stream_capturing():
            g.report(False)

    def _nf_begin(self, dev, B: int):
        """(bad, address of the depth word, address of the guidance word) for this forward's stems and head -- (None, None,
        None) in "ignore" mode and for nn.DataParallel replicas on another device than the module's own.  `bad` still has to
        be zeroed on the forward's stream: _nf_open."""
        mode = self._nf_mode()
        if mode == "ignore":
            return None, None, None
        g = self._nf_state()
        if self.__dict__.get("_no_guard", False) and g.home is not None and torch.device(dev) != g.home:
            return None, None, None          # an nn.DataParallel replica on another device than the module's own
        bad = g.bad_words(dev, B)
        if mode != "raise":
            return bad, None, None
        p = g.words_ptr
        if p is None:
            g.host_words()
            p = g.words_ptr
        return bad, p, p + 4

    def _nf_open(self, dev, B: int):
        """The guard launches that open a forward: the weight checksum -- which also zeroes `bad` -- or, where that launch is
        absent (CODON_WEIGHT_GUARD=0, nn.DataParallel replicas, a guard disabled for unaligned weights), a memset."""
        bad, wd, wg = self._nf_begin(dev, B)
        if not self._guard(dev, clear=bad, nclear=B) and bad is not None:
            bad[:B].zero_()
        return bad, wd, wg
